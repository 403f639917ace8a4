"""GPU: mode A's default — whitened rows -> Gram matrix -> diagonally pivoted Cholesky -> X = R L^-1 (ovgpu_msckf_compress) — at every tile edge
of its kernels, through the C ABI, against the oracle and the float64 emulation of tests/mode_a_shapes.py (tests/test_mode_a_shapes_cpu.py
vets every snapshot on the oracle alone).  The oracle's triangulation is injected on both sides.

Per case, with the default switches: the route and the three kernels the library reports equal mode_a_shapes.expected(D); feat_status the
oracle's; H, r finite, H of shape (rows, D); the GENUINE rank (rows of H over 1e-6 of the largest row's 2-norm) EQUAL to the emulation's — rows
may exceed it by noise rows only, each under 1e-7; |H^T H - G| / |G| < 1e-11 and |H^T r - g| / |g| < 1e-10 against the oracle's compressed
system (test_gpu_parity.test_mode_a_compressed_system's bounds); (H, r) through the oracle's EKFUpdate within TOL_P / TOL_DX of the oracle's
posterior; the resident covariance bit-equal to the prior.  At 384 columns the Householder triangle comes back (rows = D, upper triangular): an
unpivoted triangle's row norms say nothing of the rank, so the rank of its whitened form H L (singular values over 1e-9 of the largest) is held
to the emulation's genuine rank instead.  The batch whose every feature the gate rejects returns rows = 0 and OVGPU_OK.

Then the same cases with the blocked factor off (D <= 223: k_gram_pchol<1 .. 7>) and the blocked un-whitening off (D <= 256: k_unwhiten<16>), the
prior factored step by step / in two panels behind the un-whitening at 256 and 258 columns, and two runs from ovgpu_reset_state bit for bit.

Measured on one MI355X, 85 booked runs in one process (test_zz_worst_deviations prints them; worst per family, eG / eg / P' / dx):
  k_gram_pchol_blk<4, 9, 2>   (one-pass Gram, either un-whitening for <= 16 tile columns)   7.2e-15 / 5.7e-15 / 4.6e-14 / 4.9e-13
  k_gram_pchol_blk<7, 15, 4>  (one-pass Gram, either un-whitening)                          7.9e-15 / 7.2e-15 / 6.0e-14 / 9.7e-13
  k_gram_pchol<1 .. 8>        (one-pass Gram, either un-whitening)                          2.0e-14 / 1.7e-14 / 7.0e-14 / 1.1e-12
  k_gram_pchol<9>             (k_gram_blk, k_unwhiten_blk<16> or k_unwhiten<16>: D = 256)    7.5e-15 / 7.1e-15 / 8.7e-14 / 2.8e-13
  k_gram_pchol<9 .. 12>       (k_gram_blk, k_unwhiten<24>)                                  2.5e-14 / 3.7e-14 / 1.9e-13 / 1.4e-12
  k_gram_pchol<12>            (k_gram_wide, k_unwhiten<24>)                                 1.8e-14 / 2.9e-14 / 8.8e-14 / 4.5e-13
  Householder triangle        (D = 384)                                                     2.0e-14 / 2.6e-14 / 3.6e-14 / 7.9e-14
against the bounds 1e-11 / 1e-10 / 1e-9 / 1e-8: every family sits 400 to 7000 times under them (the bounds are the suite's shared constants and
stay as they are here; a kernel wrong at 1e-12 would pass them, which a later change may want to close).  The genuine rank equals the emulation's
in every run; the device returns 0 to 2 noise rows beyond it (the emulation 0 to 3, not always the same count), the largest 3.1e-8 of the largest
row (D = 66 with the rank-one factor), under the 1e-7 the rule allows.  No case exposed a fault in a kernel or in the dispatch.
"""
import numpy as np
import pytest

import mode_a_shapes as mas
from test_gpu_parity import TOL_DX, TOL_P

pytestmark = pytest.mark.gpu

TOL_G, TOL_g = 1e-11, 1e-10   # test_gpu_parity.test_mode_a_compressed_system's
NOISE_ROW = mas.GAP[0]        # a row beyond the genuine rank: under 1e-7 of the largest
KERNEL_OPTIONS = ("last_gram_kernel", "last_factor_kernel", "last_unwhiten_kernel")
WORST = {}                    # kernel family -> [eG, eg, P', dx, runs], of the runs of THIS process
RAN = set()                   # their labels


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _compress(Updater, case, R, debug=None, again=False, **optkw):
    """One ovgpu_msckf_compress of the case on a fresh context (again: and a second one from ovgpu_reset_state): the result(s), what the library
    says it ran, and the resident covariance afterwards."""
    up = Updater(case.opts(**optkw))
    for name, val in (debug or {}).items():
        up.debug_option(name, val)
    up.set_problem(case.prob)
    tri = R["tri"]
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    out = [up.compress()]
    ran = (up.lib.ovgpu_last_update_route(up._ctx),) + tuple(up.debug_option(n) for n in KERNEL_OPTIONS)
    P_after = up.get_state()["P"]
    if again:
        up.reset_state()
        out.append(up.compress())
        assert (up.lib.ovgpu_last_update_route(up._ctx),) + tuple(up.debug_option(n) for n in KERNEL_OPTIONS) == ran
    up.close()
    return out, ran, P_after


def _check(oracle, case, cmp, ran, P_after, exp, label):
    """Every per-case assertion of the module's docstring; returns the genuine rank."""
    R = mas.reference(oracle, case)
    ref, prob, D = R["ref"], case.prob, case.D
    H, r, rows = cmp["H"], cmp["r"], cmp["rows"]
    assert ran == mas.codes(exp), (label, ran, mas.codes(exp))
    assert cmp["D"] == D and np.array_equal(cmp["col_cov_id"], R["cols"])
    assert np.array_equal(cmp["feat_status"], ref["feat_status"])
    assert H.shape == (rows, D) and r.shape == (rows,) and np.isfinite(H).all() and np.isfinite(r).all()
    np.testing.assert_array_equal(P_after, prob.P)  # mode A does not touch the state
    if case.group == "reject":
        assert rows == 0 and R["rank"] == 0
        print(f"{label}: every feature rejected, rows 0")
        return 0
    rel = mas.row_rel_norms(H)
    if exp.route == "tsqr":
        assert rows == D and np.abs(np.tril(H, -1)).max() == 0.0
        rank = mas.svd_rank(prob.P, R["cols"], H)
        noise = np.zeros(0)
    else:
        assert 0 < rows <= D
        assert (np.abs(H).sum(axis=1) > 0).all()  # the zero rows stayed on the device
        rank = mas.genuine_rank(H)
        noise = rel[rel <= mas.RANK_REL]
    eG, eg = _rel(H.T @ H, R["G"]), _rel(H.T @ r, R["g"])
    st, P1, dx1 = oracle.ekf_update(prob.P, H, r, cmp["col_cov_id"], 1.0)
    eP, edx = _rel(P1, ref["P"]), _rel(dx1, ref["dx"])
    print(f"{label}: D {D}, rows {rows}, genuine rank {rank} (emulation {R['rank']}, {R['H_emu'].shape[0]} rows), largest noise row "
          f"{noise.max() if noise.size else 0.0:.1e}, eG {eG:.1e}, eg {eg:.1e}, P' {eP:.1e}, dx {edx:.1e}   [{mas.family(exp)}]")
    RAN.add(label)
    w = WORST.setdefault(mas.family(exp), [0.0, 0.0, 0.0, 0.0, 0])
    w[:] = [max(w[0], eG), max(w[1], eg), max(w[2], eP), max(w[3], edx), w[4] + 1]
    assert rank == R["rank"], (label, rank, R["rank"], np.sort(rel)[:4])
    if exp.route == "pchol":  # rows beyond the genuine rank: noise rows only
        assert rows - rank == noise.size and (noise < NOISE_ROW).all(), (label, rows, rank, noise)
    if case.group == "rank":
        assert rank == case.R
    assert eG < TOL_G and eg < TOL_g
    assert st == 0 and eP < TOL_P and edx < TOL_DX
    return rank


@pytest.mark.parametrize("cid", mas.CASE_IDS)
def test_default_switches(Updater, oracle, cid):
    case = mas.BY_ID[cid]
    R = mas.reference(oracle, case)
    (cmp,), ran, P_after = _compress(Updater, case, R)
    exp = mas.expected(case.D)
    assert (cmp["rows"] == case.D) == (exp.route == "tsqr")
    case._rank_default = _check(oracle, case, cmp, ran, P_after, exp, cid)


def _default_rank(Updater, oracle, case):
    if not hasattr(case, "_rank_default"):  # (this test selected on its own)
        R = mas.reference(oracle, case)
        (cmp,), ran, P_after = _compress(Updater, case, R)
        case._rank_default = _check(oracle, case, cmp, ran, P_after, mas.expected(case.D), case.id)
    return case._rank_default


@pytest.mark.parametrize("cid", [c.id for c in mas.CASES if c.D <= 223])
def test_blocked_factor_off(Updater, oracle, cid):
    """"pchol_blocked" = 0: the rank-one k_gram_pchol<1 .. 7>, which nothing else instantiates; the same genuine rank, every bound against the oracle."""
    case = mas.BY_ID[cid]
    R = mas.reference(oracle, case)
    (cmp,), ran, P_after = _compress(Updater, case, R, debug=dict(pchol_blocked=0))
    exp = mas.expected(case.D, False, unwhiten_blocked=True)
    assert exp.factor == "rank-one" and 1 <= exp.nb <= 7
    assert _check(oracle, case, cmp, ran, P_after, exp, cid + " pchol_blocked=0") == _default_rank(Updater, oracle, case)


@pytest.mark.parametrize("cid", [c.id for c in mas.CASES if c.D <= 256])
def test_blocked_unwhitening_off(Updater, oracle, cid):
    """"unwhiten_blocked" = 0: k_unwhiten<16> behind either factor."""
    case = mas.BY_ID[cid]
    R = mas.reference(oracle, case)
    (cmp,), ran, P_after = _compress(Updater, case, R, debug=dict(unwhiten_blocked=0))
    exp = mas.expected(case.D, True, unwhiten_blocked=False)
    assert exp.unwhiten == "subst<16>"
    assert _check(oracle, case, cmp, ran, P_after, exp, cid + " unwhiten_blocked=0") == _default_rank(Updater, oracle, case)


@pytest.mark.parametrize("cid,optkw,debug", [("col-256", dict(no_single_launch_cholesky=1), {}), ("col-258", dict(no_single_launch_cholesky=1), {}),
                                             ("col-258", {}, dict(chol_wide=0))])
def test_prior_factorisation_switches(Updater, oracle, cid, optkw, debug):
    """The un-whitening behind the other prior factorisations: step by step (no inverse diagonal tiles: k_unwhiten<16> at 256 columns), and at 258
    columns behind the two-panel one (the default there) and the step-wise one alike."""
    case = mas.BY_ID[cid]
    R = mas.reference(oracle, case)
    (cmp,), ran, P_after = _compress(Updater, case, R, debug=debug, **optkw)
    exp = mas.expected(case.D, single_launch=False)
    assert exp.unwhiten == ("subst<16>" if case.D == 256 else "subst<24>")
    label = cid + " " + " ".join(f"{k}={v}" for k, v in {**optkw, **debug}.items())
    assert _check(oracle, case, cmp, ran, P_after, exp, label) == _default_rank(Updater, oracle, case)


@pytest.mark.parametrize("cid", ["col-222", "col-300"])
def test_two_runs_are_bit_equal(Updater, oracle, cid):
    """One blocked and one rank-one case twice from ovgpu_reset_state: no atomics, ordered sums — the same bits."""
    case = mas.BY_ID[cid]
    R = mas.reference(oracle, case)
    (a, b), ran, _ = _compress(Updater, case, R, again=True)
    assert ran == mas.codes(mas.expected(case.D))
    assert a["rows"] == b["rows"] and np.array_equal(a["H"], b["H"]) and np.array_equal(a["r"], b["r"])
    assert np.array_equal(a["feat_status"], b["feat_status"])


def test_zz_worst_deviations():
    """Prints the worst deviations per kernel family over the runs of this process (the module's docstring and DESIGN.md section 7 quote the
    values of a run in ONE process); where every default leg ran in this process, every kernel family must be among them.  (Spread over several
    worker processes each sees a part: the legs assert their kernels one by one either way.)"""
    for fam in sorted(WORST):
        eG, eg, eP, edx, n = WORST[fam]
        print(f"{fam}: {n} runs, worst eG {eG:.1e} (bound {TOL_G:g}), eg {eg:.1e} ({TOL_g:g}), P' {eP:.1e} ({TOL_P:g}), dx {edx:.1e} ({TOL_DX:g})")
    if not {c.id for c in mas.CASES if c.group != "reject"} <= RAN:
        return
    fams = " | ".join(WORST)
    for name in ("blk<4,9,2>", "blk<7,15,4>", "rank-one", "gram one-pass", "gram blk", "gram wide", "unwhiten blk<16>", "unwhiten subst<24>", "tsqr"):
        assert name in fams, name
