"""GPU tests (`-m gpu`) of mode A (ovgpu_msckf_compress) on the pivoted Gram route at 384 .. 511 Jacobian columns, selected with
ovgpu_debug_option "mode_a_wide" = 1 and off by default: whitened rows from the fused per-feature kernels, k_gram_blk over four column windows,
the panelled pivoted factor (k_pchol_wide.h: k_pchol_panel, 32 pivots per launch, around k_pchol_schur) and k_unwhiten_blk<32> on the inverse
diagonal tiles of the prior block's factorisation (the two panels' own, or k_uinv_tiles' behind a step-wise one).  All through the C ABI, the
oracle's triangulation injected on both sides.  The batches and what each is named for: tests/mode_a_wide_shapes.py
(tests/test_mode_a_wide_shapes_cpu.py vets every one on the oracle alone).

Per case, every assertion of tests/test_gpu_mode_a_shapes.py's _check: the reported route and the three kernel codes equal the restated rule
(PCHOLQR, 2, 3, 4 or 5); feat_status the oracle's; H finite and of shape (rows, D); the GENUINE rank equal to the emulation's, the rows beyond it
noise rows only, each under 1e-7; |H^T H - G| / |G| < 1e-11 and |H^T r - g| / |g| < 1e-10; (H, r) through the oracle's EKFUpdate within TOL_P /
TOL_DX of the oracle's posterior; the resident covariance bit-equal to the prior; "mode_a_wide_compressions" one higher.  Every deviation is
printed before it is asserted; test_zz_worst_deviations prints the maxima per kernel family (DESIGN.md section 7 quotes a run's).

Then: every feature rejected; the prior factored step-wise (un-whitening code 5), also held to the two-panel run; a semi-definite prior (the
Householder repeat, not counted, the context usable afterwards); what must not move, bit for bit against a context that never named the switch;
the switch itself; context hygiene.

Measured on one MI355X, 24 booked runs in one process, 18.6 s for the file (worst per kernel family, eG / eg / P' / dx / largest noise row, against
the bounds 1e-11 / 1e-10 / 1e-9 / 1e-8 / 1e-7):
  k_pchol_panel / k_pchol_schur + k_gram_blk + k_unwhiten_blk<32> on the two-panel tiles (21 runs)   2.1e-14 / 5.5e-14 / 1.9e-13 / 5.4e-12 / 2.8e-8
  ... on k_uinv_tiles' tiles (3 runs: the step-wise priors and "unwhiten_blocked" = 0)               6.7e-15 / 1.7e-14 / 1.1e-13 / 4.8e-13 / 0
The genuine rank equals the emulation's in every run; the device returns 0 or 1 noise row beyond it.  The step-wise runs against the two-panel run:
eG 2.3e-16, eg 6.2e-16.  The Householder repeat of the semi-definite prior is bit-equal to a context that never named the switch.
"""
import numpy as np
import pytest

import gram_wide_shapes as gws
import mode_a_shapes as mas
import mode_a_wide_shapes as maw
import slam_shapes as ss
import test_gpu_slam_chunked as sc
from open_vins_amd import capi
from test_gpu_parity import TOL_DX, TOL_P

pytestmark = pytest.mark.gpu

TOL_G, TOL_g = 1e-11, 1e-10   # test_gpu_parity.test_mode_a_compressed_system's
NOISE_ROW = mas.GAP[0]        # a row beyond the genuine rank: under 1e-7 of the largest
KERNEL_OPTIONS = ("last_gram_kernel", "last_factor_kernel", "last_unwhiten_kernel")
COUNTER = "mode_a_wide_compressions"
COMPRESS_KEYS = ("feat_status", "chi2", "chi2_thresh", "H", "r", "col_cov_id")
UPDATE_KEYS = ("feat_status", "chi2", "chi2_thresh", "p_FinG", "dx", "P")
WIDE = (capi.COMPRESS_PCHOLQR, maw.GRAM_BLK, maw.FACTOR_PANEL, maw.UNWHITEN_TILES)
WORST = {}                    # kernel family -> [eG, eg, P', dx, largest noise row, runs], of the runs of THIS process


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def context(Updater, opts, level, **debug):
    """a context with "mode_a_wide" (and the other switches) set before anything is uploaded; level = None never names it"""
    up = Updater(opts)
    if level is not None:
        up.debug_option("mode_a_wide", level)
    for name, val in debug.items():
        up.debug_option(name, val)
    return up


def ran_of(up):
    return (up.lib.ovgpu_last_update_route(up._ctx),) + tuple(up.debug_option(n) for n in KERNEL_OPTIONS)


def hand_over(up, prob, tri):
    up.set_problem(prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])


def compress(Updater, prob, opts, tri, level, keep=False, **debug):
    """one ovgpu_msckf_compress on a fresh context: the result with what the library says it ran, the counter and the resident covariance"""
    up = context(Updater, opts, level, **debug)
    hand_over(up, prob, tri)
    out = up.compress()
    out["ran"], out["P_after"] = ran_of(up), up.get_state()["P"]
    out["count"] = up.debug_option(COUNTER) if level is not None else None
    if keep:
        return out, up
    up.close()
    return out


def case_compress(Updater, oracle, case, level, keep=False, debug=None, **optkw):
    R = mas.reference(oracle, case)
    return compress(Updater, case.prob, case.opts(**optkw), R["tri"], level, keep=keep, **(debug or {}))


def assert_same_bits(a, b, what, keys=COMPRESS_KEYS):
    if "rows" in a:
        assert a["rows"] == b["rows"] and a["D"] == b["D"], what
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def check(oracle, case, cmp, want, label):
    """Every per-case assertion of the module's docstring (the counter is the caller's); returns the genuine rank."""
    R = mas.reference(oracle, case)
    ref, prob, D = R["ref"], case.prob, case.D
    H, r, rows = cmp["H"], cmp["r"], cmp["rows"]
    assert cmp["ran"] == want, (label, cmp["ran"], want)
    assert cmp["D"] == D and np.array_equal(cmp["col_cov_id"], R["cols"])
    assert np.array_equal(cmp["feat_status"], ref["feat_status"])
    assert H.shape == (rows, D) and r.shape == (rows,) and np.isfinite(H).all() and np.isfinite(r).all()
    np.testing.assert_array_equal(cmp["P_after"], prob.P)  # mode A does not touch the state
    if case.group == "reject":
        assert rows == 0 and R["rank"] == 0
        print(f"{label}: every feature rejected, rows 0")
        return 0
    assert 0 < rows <= D
    assert (np.abs(H).sum(axis=1) > 0).all()  # the zero rows stayed on the device
    rel = mas.row_rel_norms(H)
    rank = mas.genuine_rank(H)
    noise = rel[rel <= mas.RANK_REL]
    eG, eg = _rel(H.T @ H, R["G"]), _rel(H.T @ r, R["g"])
    st, P1, dx1 = oracle.ekf_update(prob.P, H, r, cmp["col_cov_id"], 1.0)
    eP, edx = _rel(P1, ref["P"]), _rel(dx1, ref["dx"])
    big = noise.max() if noise.size else 0.0
    print(f"{label}: D {D}, rows {rows}, genuine rank {rank} (emulation {R['rank']}, {R['H_emu'].shape[0]} rows), largest noise row {big:.1e}, "
          f"eG {eG:.1e}, eg {eg:.1e}, P' {eP:.1e}, dx {edx:.1e}   [{maw.family(want)}]")
    w = WORST.setdefault(maw.family(want), [0.0, 0.0, 0.0, 0.0, 0.0, 0])
    w[:] = [max(w[0], eG), max(w[1], eg), max(w[2], eP), max(w[3], edx), max(w[4], big), w[5] + 1]
    assert rank == R["rank"], (label, rank, R["rank"], np.sort(rel)[:4])
    assert rows - rank == noise.size and (noise < NOISE_ROW).all(), (label, rows, rank, noise)  # rows beyond the genuine rank: noise rows only
    if case.group == "rank":
        assert rank == case.R
    assert eG < TOL_G and eg < TOL_g
    assert st == 0 and eP < TOL_P and edx < TOL_DX
    return rank


# --------------------------------------------------------------------------- the route, case by case
@pytest.mark.parametrize("cid", maw.CASE_IDS)
def test_wide_route(Updater, oracle, cid):
    case = maw.BY_ID[cid]
    cmp = case_compress(Updater, oracle, case, 1)
    assert maw.expected_codes(case.D, 1) == WIDE
    check(oracle, case, cmp, WIDE, cid)
    assert cmp["count"] == 1  # (every feature rejected: rows 0 with OVGPU_OK — compress() raises on any other status — and the route was taken)


@pytest.mark.parametrize("how", ["no_single_launch_cholesky", "chol_wide_0", "unwhiten_blocked_0"])
def test_stepwise_prior(Updater, oracle, how):
    """the prior factored step-wise (or the blocked un-whitening switched off): no inverse tiles from the factorisation, k_uinv_tiles makes them"""
    case = maw.BY_ID["col-400"]
    optkw = dict(no_single_launch_cholesky=1) if how == "no_single_launch_cholesky" else {}
    debug = dict(chol_wide=0) if how == "chol_wide_0" else (dict(unwhiten_blocked=0) if how == "unwhiten_blocked_0" else {})
    want = maw.expected_codes(400, 1, two_panel=how == "unwhiten_blocked_0", unwhiten_blocked=how != "unwhiten_blocked_0")
    assert want == WIDE[:3] + (maw.UNWHITEN_INVERTED,)
    cmp = case_compress(Updater, oracle, case, 1, debug=debug, **optkw)
    rank = check(oracle, case, cmp, want, f"col-400 {how}")
    assert cmp["count"] == 1
    two = case_compress(Updater, oracle, case, 1)
    assert two["ran"] == WIDE and two["rows"] == cmp["rows"] and mas.genuine_rank(two["H"]) == rank
    eG, eg = _rel(cmp["H"].T @ cmp["H"], two["H"].T @ two["H"]), _rel(cmp["H"].T @ cmp["r"], two["H"].T @ two["r"])
    print(f"col-400 {how} against the two-panel run: eG {eG:.1e}, eg {eg:.1e}")
    assert eG < TOL_G and eg < TOL_g


def test_semi_definite_prior_repeats_through_householder(Updater, oracle):
    """the two newest clones perfectly correlated at 400 columns: the prior block's pivot fails, compress_impl repeats the call through the
    Householder route, the attempt is not counted, and the context serves the positive-definite twin on the wide route afterwards"""
    good = maw.BY_ID["col-400"]
    bad = ss.semi_definite(good.prob)
    opts = good.opts()
    tri = oracle.triangulate(opts, capi.Views(bad))
    on, up = compress(Updater, bad, opts, tri, 1, keep=True)
    off = compress(Updater, bad, opts, tri, None)
    assert on["ran"] == (capi.COMPRESS_TSQR, 0, 0, 0) == off["ran"] and on["count"] == 0
    assert on["rows"] == off["rows"] == 400 and np.array_equal(on["feat_status"], off["feat_status"]) and np.isfinite(on["H"]).all()
    eG = _rel(on["H"].T @ on["H"], off["H"].T @ off["H"])
    print(f"semi-definite prior at 400 columns: the Householder repeat against a context that never named the switch, eG {eG:.1e}")
    assert eG < TOL_G
    R = mas.reference(oracle, good)
    hand_over(up, good.prob, R["tri"])
    again = up.compress()
    again["ran"], again["P_after"] = ran_of(up), up.get_state()["P"]
    assert up.debug_option(COUNTER) == 1
    up.close()
    check(oracle, good, again, WIDE, "col-400 behind the Householder repeat")


# --------------------------------------------------------------------------- what must not move
@pytest.mark.parametrize("D", sorted(maw.NARROW))
def test_narrow_compress_keeps_its_bits(Updater, oracle, D):
    case = maw.NARROW[D]
    on, never = case_compress(Updater, oracle, case, 1), case_compress(Updater, oracle, case, None)
    assert on["ran"] == never["ran"] == mas.codes(mas.expected(D)) == maw.expected_codes(D, 1) and on["count"] == 0
    assert_same_bits(on, never, f"compress at {D} columns")


@pytest.mark.parametrize("what,optkw", [("tsqr", dict(compress_route=capi.COMPRESS_TSQR)), ("fp32", dict(gram_fp32=1))])
def test_off_the_route_compress_keeps_its_bits(Updater, oracle, what, optkw):
    case = maw.BY_ID["col-400"]
    on, never = case_compress(Updater, oracle, case, 1, **optkw), case_compress(Updater, oracle, case, None, **optkw)
    assert on["ran"] == never["ran"] == (capi.COMPRESS_TSQR, 0, 0, 0) and on["count"] == 0 and on["rows"] == 400
    assert_same_bits(on, never, f"compress at 400 columns, {what}")


def _slam_compress(Updater, case, level):
    up = context(Updater, case.opts(), level, slam_fused=0)
    up.set_slam_problem(case.prob)
    out = up.slam_compress()
    out["ran"], out["count"] = ran_of(up), (up.debug_option(COUNTER) if level is not None else None)
    up.close()
    return out


def test_slam_compress_keeps_its_bits(Updater):
    case = gws.SLAM_BY_ID["d-compress-384"]
    on, never = _slam_compress(Updater, case, 1), _slam_compress(Updater, case, None)
    assert on["ran"] == never["ran"] == (capi.COMPRESS_TSQR, 0, 0, 0) and on["count"] == 0 and on["D"] == 384
    assert_same_bits(on, never, "ovgpu_slam_compress at 384 columns")


def _update(Updater, oracle, case, level, keep=False, **debug):
    tri, _ = gws.msckf_oracle_run(oracle, case)
    up = context(Updater, case.opts(), level, **debug)
    hand_over(up, case.prob, tri)
    out = up.update()
    out["route"], out["gram_wide_updates"] = up.lib.ovgpu_last_update_route(up._ctx), up.debug_option("gram_wide_updates")
    out["count"] = up.debug_option(COUNTER) if level is not None else None
    if keep:
        return out, up
    up.close()
    return out


def test_update_keeps_its_bits(Updater, oracle):
    """ovgpu_msckf_update at 400 columns: with this switch alone the Householder route's bits, with "gram_wide" = 1 as well that context's"""
    case = gws.MSCKF_BY_ID["a-400"]
    on, never = _update(Updater, oracle, case, 1), _update(Updater, oracle, case, None)
    assert on["route"] == never["route"] == capi.COMPRESS_TSQR and on["count"] == 0 and on["gram_wide_updates"] == 0
    assert_same_bits(on, never, "ovgpu_msckf_update at 400 columns, mode_a_wide alone", UPDATE_KEYS)
    both, gram = _update(Updater, oracle, case, 1, gram_wide=1), _update(Updater, oracle, case, None, gram_wide=1)
    assert both["route"] == gram["route"] == capi.COMPRESS_GRAM and both["count"] == 0 and both["gram_wide_updates"] == gram["gram_wide_updates"] == 1
    assert_same_bits(both, gram, "ovgpu_msckf_update at 400 columns, both switches against gram_wide alone", UPDATE_KEYS)


def test_512_columns_are_refused_as_before(Updater):
    p = gws.over_the_bound()
    msgs = []
    for level in (1, None):
        up = context(Updater, capi.default_options(chi2_multipler=1.0), level)
        up.set_slam_problem(p)
        with pytest.raises(capi.OvgpuError) as e:
            up.slam_compress()
        assert e.value.code == capi.ERR_CAPACITY
        msgs.append(str(e.value))
        up.close()
    assert msgs[0] == msgs[1] and "512 Jacobian columns, more than 511" in msgs[0]


# --------------------------------------------------------------------------- the switch
def test_the_switch(Updater, oracle):
    case = maw.BY_ID["col-384"]
    R = mas.reference(oracle, case)
    up = Updater(case.opts())
    assert up.debug_option("mode_a_wide") == 0                                              # the default stays 0
    assert up.debug_option("mode_a_wide", 1) == 0 and up.debug_option("mode_a_wide") == 1   # reads back 1
    assert up.debug_option("mode_a_wide", 7) == 1 and up.debug_option("mode_a_wide") == 1   # values above 1 are taken as 1
    assert up.debug_option(COUNTER, 5) == 0 and up.debug_option(COUNTER) == 0               # read only
    assert up.debug_option("gram_wide") == 0                                                # independent of the update's switch
    up.close()
    never, off = case_compress(Updater, oracle, case, None), case_compress(Updater, oracle, case, 0)
    assert never["ran"] == off["ran"] == (capi.COMPRESS_TSQR, 0, 0, 0) and off["count"] == 0 and off["rows"] == 384
    assert_same_bits(off, never, "mode_a_wide = 0 against never set")
    # thrown after the batch was handed over: the resident batch keeps the Householder route, the next ovgpu_set_features takes the switch
    up = context(Updater, case.opts(), 0)
    hand_over(up, case.prob, R["tri"])
    up.debug_option("mode_a_wide", 1)
    first = up.compress()
    assert ran_of(up) == (capi.COMPRESS_TSQR, 0, 0, 0) and up.debug_option(COUNTER) == 0
    assert_same_bits(first, never, "the switch thrown behind ovgpu_set_features")
    up.reset_state()
    up.set_features(case.prob)
    tri = R["tri"]
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    second = up.compress()
    second["ran"], second["P_after"] = ran_of(up), up.get_state()["P"]
    assert up.debug_option(COUNTER) == 1
    up.close()
    check(oracle, case, second, WIDE, "col-384 after the switch was thrown and the batch handed over again")


# --------------------------------------------------------------------------- context hygiene
@pytest.mark.parametrize("cid", ["col-400", "mix-510"])
def test_same_bits_twice_from_reset_state(Updater, oracle, cid):
    case = maw.BY_ID[cid]
    R = mas.reference(oracle, case)
    first, up = case_compress(Updater, oracle, case, 1, keep=True)
    up.reset_state()
    up.set_features(case.prob)
    tri = R["tri"]
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    second = up.compress()
    assert ran_of(up) == first["ran"] == WIDE and up.debug_option(COUNTER) == 2
    up.close()
    assert_same_bits(first, second, f"{cid}: the same call twice from ovgpu_reset_state")


def test_one_context_510_then_208_then_448(Updater, oracle):
    """every link returns a fresh context's bits: nothing of the wider (or narrower) compression before it is left in a workspace"""
    cases = [maw.BY_ID[c] if isinstance(c, str) else maw.NARROW[c] for c in maw.HYGIENE_CHAIN]
    up = context(Updater, cases[0].opts(), 1)
    count = 0
    for case in cases:
        R = mas.reference(oracle, case)
        hand_over(up, case.prob, R["tri"])
        link = up.compress()
        fresh = case_compress(Updater, oracle, case, 1)
        count += 1 if case.D >= 384 else 0
        assert ran_of(up) == fresh["ran"] == maw.expected_codes(case.D, 1) and up.debug_option(COUNTER) == count
        assert_same_bits(link, fresh, f"{case.id} as a link of the chain against a fresh context")
    up.close()


def test_compress_then_update_on_one_context(Updater, oracle):
    """compress at 400 columns on the wide route, then ovgpu_msckf_update with "gram_wide" = 1 on the same context: the update's two factorisations
    reuse the slots of the inverse tiles; it returns a fresh context's bits"""
    case, ucase = maw.BY_ID["col-400"], gws.MSCKF_BY_ID["a-400"]
    cmp, up = case_compress(Updater, oracle, case, 1, keep=True, debug=dict(gram_wide=1))
    assert cmp["ran"] == WIDE and cmp["count"] == 1
    tri, _ = gws.msckf_oracle_run(oracle, ucase)
    hand_over(up, ucase.prob, tri)
    out = up.update()
    assert up.lib.ovgpu_last_update_route(up._ctx) == capi.COMPRESS_GRAM and up.debug_option("gram_wide_updates") == 1 and up.debug_option(COUNTER) == 1
    up.close()
    fresh = _update(Updater, oracle, ucase, 1, gram_wide=1)
    assert fresh["route"] == capi.COMPRESS_GRAM
    assert_same_bits(out, fresh, "ovgpu_msckf_update behind a wide compression against a fresh context", UPDATE_KEYS)


def test_zz_worst_deviations():
    """prints the worst deviations per kernel family over the runs of this process"""
    for fam in sorted(WORST):
        eG, eg, eP, edx, big, n = WORST[fam]
        print(f"{fam}: {n} runs, worst eG {eG:.1e} (bound {TOL_G:g}), eg {eg:.1e} ({TOL_g:g}), P' {eP:.1e} ({TOL_P:g}), dx {edx:.1e} ({TOL_DX:g}), "
              f"largest noise row {big:.1e} ({NOISE_ROW:g})")
