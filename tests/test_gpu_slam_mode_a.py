"""GPU tests (`-m gpu`) of mode A of the SLAM update (ovgpu_slam_compress) on the pivoted Gram route, selected with ovgpu_debug_option
"slam_mode_a" = 1 and off by default: whitened rows from the general per-feature kernel or, under "slam_fused", from k_slam_y; the Gram matrix
and the diagonally pivoted factor chosen by the column count as for ovgpu_msckf_compress; the un-whitening, at 257 .. 383 columns
k_unwhiten_blk<24> on the inverse diagonal tiles of the prior block's factorisation (the two panels' own, or k_uinv_tiles' behind a step-wise
one).  With "mode_a_wide" = 1 as well the route holds 511 columns.  All through the C ABI.  The batches and what each is named for:
tests/slam_mode_a_shapes.py (tests/test_slam_mode_a_shapes_cpu.py vets every one on the oracle alone).

Per case, the assertions of tests/test_gpu_mode_a_shapes.py's _check moved to this entry: the reported route and the kernel codes equal the
restated rule; feat_status the oracle's, chi2 within TOL_CHI2; H finite, of shape (rows, D), no zero row; the GENUINE rank equal to the
emulation's, the rows beyond it noise rows only, each under 1e-7; |H^T H - G| / |G| < 1e-11 and |H^T r - g| / |g| < 1e-10 against the oracle's
stack (scaled to the context's sigma_pix where the batch carries per-feature sigmas); (H, r) through the oracle's EKFUpdate within TOL_P / TOL_DX
of the oracle's posterior; the resident covariance and landmarks bit-equal to what was uploaded; "slam_mode_a_compressions" one higher.  Every
deviation is printed before it is asserted; test_zz_worst_deviations prints the maxima per kernel family (DESIGN.md section 7 quotes a run's).

On a library without the switch every test of this file fails: "slam_mode_a" is an unknown name there.

Measured on one MI355X, 90 tests in 16.5 s (worst per kernel family, eG / eg / P' / dx / largest noise row, against the bounds 1e-11 / 1e-10 / 1e-9 /
1e-8 / 1e-7):
  k_gram_pchol_blk<4,9,2> | <7,15,4> | k_gram_pchol<NB> + one-pass Gram + k_unwhiten_blk<16> (22 runs)   4.3e-15 / 1.4e-13 / 4.2e-14 / 2.9e-10 / 0
  k_gram_pchol<NB> + k_gram_blk | k_gram_wide + k_unwhiten_blk<24> on the two-panel tiles (31 runs)       2.5e-15 / 1.7e-11 / 4.2e-14 / 1.4e-9 / 7.8e-8
  ... on k_uinv_tiles' tiles (6 runs)                                                                     2.3e-15 / 8.8e-14 / 3.2e-14 / 1.8e-11 / 0
  k_pchol_panel / k_pchol_schur + k_gram_blk + k_unwhiten_blk<32> (14 runs)                               2.7e-15 / 4.4e-14 / 3.9e-14 / 1.2e-11 / 0
The genuine rank equals the emulation's in every run.  The three-chunk replay against the oracle's chain: P 2.19e-12, dx 4.83e-11 on the pivoted
route, 2.17e-12, 4.82e-11 on the Householder route.
"""
import copy

import numpy as np
import pytest

import gram_wide_shapes as gws
import mode_a_shapes as mas
import slam_mode_a_shapes as sma
import slam_shapes as ss
import test_gpu_slam_chunked as sc
from open_vins_amd import capi
from test_gpu_parity import TOL_CHI2, TOL_DX, TOL_P

pytestmark = pytest.mark.gpu

TOL_G, TOL_g = 1e-11, 1e-10   # test_gpu_parity.test_mode_a_compressed_system's
NOISE_ROW = mas.GAP[0]        # a row beyond the genuine rank: under 1e-7 of the largest
KERNEL_OPTIONS = ("last_gram_kernel", "last_factor_kernel", "last_unwhiten_kernel")
COUNTER = "slam_mode_a_compressions"
COMPRESS_KEYS = ("feat_status", "chi2", "chi2_thresh", "H", "r", "col_cov_id")
UPDATE_KEYS = ("feat_status", "chi2", "chi2_thresh", "dx", "P")
WORST = {}                    # kernel family -> [eG, eg, P', dx, largest noise row, runs], of the runs of THIS process


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def context(Updater, opts, level, wide=0, **debug):
    """a context with "slam_mode_a" (and the other switches) set before anything is uploaded; level = None never names it"""
    up = Updater(opts)
    if level is not None:
        up.debug_option("slam_mode_a", level)
    if wide:
        up.debug_option("mode_a_wide", wide)
    for name, val in debug.items():
        up.debug_option(name, val)
    return up


def ran_of(up):
    return (up.lib.ovgpu_last_update_route(up._ctx),) + tuple(up.debug_option(n) for n in KERNEL_OPTIONS)


def hand_over(up, prob, active=None, sigma=None, mult=None):
    """ovgpu_set_state, ovgpu_set_landmarks, ovgpu_set_active_landmarks, ovgpu_set_features: the order include/ovgpu.h documents"""
    up.set_slam_problem(prob)
    if active is not None:
        up.set_active_landmarks(np.asarray(active, np.int32))
        up.set_features(prob)
    if sigma is not None or mult is not None:
        up.set_feature_options(sigma_pix=sigma, chi2_multipler=mult)


def compress_on(up, level):
    """one ovgpu_slam_compress on a context that holds its batch: the result with what the library says it ran, the counters and the resident state"""
    before = up.get_landmarks()
    out = up.slam_compress()
    out["ran"], out["kernel"] = ran_of(up), up.debug_option("last_feature_kernel")
    out["count"] = up.debug_option(COUNTER) if level is not None else None
    out["fused_batches"] = up.debug_option("slam_fused_batches")
    out["P_after"], out["lm_before"], out["lm_after"] = up.get_state()["P"], before, up.get_landmarks()
    return out


def compress(Updater, prob, opts, level, wide=0, keep=False, active=None, sigma=None, mult=None, **debug):
    up = context(Updater, opts, level, wide, **debug)
    hand_over(up, prob, active, sigma, mult)
    out = compress_on(up, level)
    if keep:
        return out, up
    up.close()
    return out


def case_compress(Updater, case, level, keep=False, debug=None, wide=None, **optkw):
    return compress(Updater, case.prob, case.opts(**optkw), level, case.wide if wide is None else wide, keep, case.active, case.sigma, case.mult, **(debug or {}))


def assert_same_bits(a, b, what, keys=COMPRESS_KEYS):
    if "rows" in a:
        assert a["rows"] == b["rows"] and a["D"] == b["D"], what
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def check(oracle, case, cmp, want, label):
    """Every per-case assertion of the module's docstring (the counter is the caller's); returns the genuine rank."""
    R = sma.reference(oracle, case)
    ref, prob, D = R["ref"], case.prob, case.columns
    H, r, rows = cmp["H"], cmp["r"], cmp["rows"]
    assert cmp["ran"] == want, (label, cmp["ran"], want)
    assert R["near_gate"] == 0
    assert cmp["D"] == D and np.array_equal(cmp["col_cov_id"], R["cols"])
    assert np.array_equal(cmp["feat_status"], ref["feat_status"]), label
    gate = np.isfinite(ref["chi2"])
    echi = np.abs(cmp["chi2"][gate] / ref["chi2"][gate] - 1.0).max() if gate.any() else 0.0
    assert H.shape == (rows, D) and r.shape == (rows,) and np.isfinite(H).all() and np.isfinite(r).all()
    np.testing.assert_array_equal(cmp["P_after"], prob.P)  # mode A does not touch the state
    for k in ("value", "fej", "cov_id", "anchor_cam", "anchor_clone", "feat_rep"):
        np.testing.assert_array_equal(cmp["lm_after"][k], cmp["lm_before"][k])
    np.testing.assert_array_equal(cmp["lm_after"]["value"], prob.lm_value)
    if case.group == "reject":
        assert rows == 0 and R["rank"] == 0
        print(f"{label}: no feature used, rows 0")
        return 0
    assert 0 < rows <= D
    assert (np.abs(H).sum(axis=1) > 0).all()  # the zero rows stayed on the device
    rel = mas.row_rel_norms(H)
    rank = mas.genuine_rank(H)
    noise = rel[rel <= mas.RANK_REL]
    eG, eg = _rel(H.T @ H, R["G"]), _rel(H.T @ r, R["g"])
    st, P1, dx1 = oracle.ekf_update(prob.P, H, r, cmp["col_cov_id"], case.opts().sigma_pix ** 2)
    eP, edx = _rel(P1, ref["P"]), _rel(dx1, ref["dx"])
    big = noise.max() if noise.size else 0.0
    fam = sma.family(want) + (f" behind feature kernel {cmp['kernel']}" if cmp["kernel"] else "")
    print(f"{label}: D {D}, stack {R['stack_rows']} rows, rows {rows}, genuine rank {rank} (emulation {R['rank']}), largest noise row {big:.1e}, "
          f"chi2 {echi:.1e}, eG {eG:.1e}, eg {eg:.1e}, P' {eP:.1e}, dx {edx:.1e}   [{fam}]")
    w = WORST.setdefault(fam, [0.0, 0.0, 0.0, 0.0, 0.0, 0])
    w[:] = [max(w[0], eG), max(w[1], eg), max(w[2], eP), max(w[3], edx), max(w[4], big), w[5] + 1]
    assert echi < TOL_CHI2
    assert rank == R["rank"], (label, rank, R["rank"], np.sort(rel)[:4])
    assert rows - rank == noise.size and (noise < NOISE_ROW).all(), (label, rows, rank, noise)  # rows beyond the genuine rank: noise rows only
    assert rank <= R["stack_rows"] and rows <= R["stack_rows"] + noise.size                      # a short stack gives a short system
    assert eG < TOL_G and eg < TOL_g
    assert st == 0 and eP < TOL_P and edx < TOL_DX
    return rank


def run_case(Updater, oracle, cid, **kw):
    case = sma.BY_ID[cid]
    cmp = case_compress(Updater, case, 1, **kw)
    rank = check(oracle, case, cmp, case.codes(1), cid)
    assert cmp["count"] == 1 and cmp["kernel"] == 0 and cmp["fused_batches"] == 0  # ("slam_fused" = 0: k_system_t writing whitened rows)
    return case, cmp, rank


# --------------------------------------------------------------------------- column edges
@pytest.mark.parametrize("cid", [c.id for c in sma.CASES if c.group in ("col", "wide")])
def test_column_edges(Updater, oracle, cid):
    case, cmp, _ = run_case(Updater, oracle, cid)
    assert cmp["ran"][0] == capi.COMPRESS_PCHOLQR
    if case.columns > 256 and case.columns <= 383:
        assert cmp["ran"][3] == sma.UNWHITEN_BLK24_TILES


def test_384_columns_with_this_switch_alone_stay_householder(Updater):
    case = sma.BY_ID["wide-384"]
    on, never = case_compress(Updater, case, 1, wide=0), case_compress(Updater, case, None, wide=0)
    assert on["ran"] == never["ran"] == sma.HOUSEHOLDER == sma.expected_codes(384, 1, 0) and on["count"] == 0 and on["rows"] == 384
    assert_same_bits(on, never, "ovgpu_slam_compress at 384 columns, slam_mode_a alone")


# --------------------------------------------------------------------------- short and long stacks, representations, options
@pytest.mark.parametrize("cid", [c.id for c in sma.CASES if c.group == "rows"])
def test_stacks(Updater, oracle, cid):
    case, cmp, rank = run_case(Updater, oracle, cid)
    if case.rows is not None:
        assert rank == case.rows and cmp["rows"] < case.columns  # a short stack, a short system: the Householder triangle returns D rows
    else:
        assert sma.reference(oracle, case)["stack_rows"] > case.columns >= cmp["rows"]


@pytest.mark.parametrize("cid", [c.id for c in sma.CASES if c.group in ("rep", "active")])
def test_representations_and_options(Updater, oracle, cid):
    run_case(Updater, oracle, cid)


def test_per_feature_sigma_and_multiplier(Updater, oracle):
    """the returned rows are scaled to the context's sigma_pix (R = sigma_pix^2 I holds for the caller): held to the oracle's stack scaled row by row,
    and NOT equal to the unscaled one"""
    case, cmp, _ = run_case(Updater, oracle, "noise")
    raw = sma.reference(oracle, case)["ref"]
    e_raw = _rel(cmp["H"].T @ cmp["H"], raw["H"].T @ raw["H"])
    print(f"noise: against the oracle's UNSCALED stack eG {e_raw:.1e}")
    assert e_raw > 1e-3 and cmp["feat_status"][ss.NOISE_F] == capi.FEAT_CHI2_REJECTED


@pytest.mark.parametrize("cid", [c.id for c in sma.CASES if c.group == "reject"])
def test_nothing_used_returns_no_rows(Updater, oracle, cid):
    case, cmp, _ = run_case(Updater, oracle, cid)
    assert cmp["rows"] == 0 and cmp["H"].shape == (0, case.columns)


# --------------------------------------------------------------------------- the fused per-feature stage
@pytest.mark.parametrize("level", [1, 2, 3])
@pytest.mark.parametrize("cid", [c.id for c in sma.CASES if c.group == "fused"])
def test_fused_stage(Updater, oracle, cid, level):
    case = sma.BY_ID[cid]
    want = case.feature_kernel(level)
    cmp = case_compress(Updater, case, 1, debug=dict(slam_fused=level))
    assert cmp["kernel"] == want, (cid, level, cmp["kernel"], want)
    assert cmp["fused_batches"] == (1 if want >= 4 else 0) and cmp["count"] == 1
    check(oracle, case, cmp, case.codes(1), f"{cid} slam_fused {level}")


def test_fused_stage_reports_every_kernel():
    by = sma.BY_ID
    assert [by[f"fused-3dof-{m}"].feature_kernel(3) for m in (62, 63, 126, 127)] == [4, 6, 6, 0]
    assert [by[f"fused-single-{m}"].feature_kernel(3) for m in (62, 63, 126, 127)] == [5, 7, 7, 0]
    assert [by[f"fused-single-{m}"].feature_kernel(1) for m in (62, 63)] == [0, 0] and by["fused-3dof-63"].feature_kernel(2) == 0


# --------------------------------------------------------------------------- the un-whitening band
@pytest.mark.parametrize("how", ["no_single_launch_cholesky", "chol_wide_0", "unwhiten_blocked_0"])
@pytest.mark.parametrize("D", [257, 383])
def test_unwhitening_band(Updater, oracle, D, how):
    """the prior factored step-wise (or the blocked form's switch off): no inverse tiles from the factorisation, k_uinv_tiles makes them"""
    case = sma.BY_ID[f"col-{D}"]
    optkw = dict(no_single_launch_cholesky=1) if how == "no_single_launch_cholesky" else {}
    debug = dict(chol_wide=0) if how == "chol_wide_0" else (dict(unwhiten_blocked=0) if how == "unwhiten_blocked_0" else {})
    want = case.codes(1, two_panel=how == "unwhiten_blocked_0", unwhiten_blocked=how != "unwhiten_blocked_0")
    assert want[3] == sma.UNWHITEN_BLK24_INVERTED
    cmp = case_compress(Updater, case, 1, debug=debug, **optkw)
    rank = check(oracle, case, cmp, want, f"col-{D} {how}")
    assert cmp["count"] == 1
    two = case_compress(Updater, case, 1)
    assert two["ran"] == case.codes(1) and two["ran"][3] == sma.UNWHITEN_BLK24_TILES and two["rows"] == cmp["rows"] and mas.genuine_rank(two["H"]) == rank
    eG, eg = _rel(cmp["H"].T @ cmp["H"], two["H"].T @ two["H"]), _rel(cmp["H"].T @ cmp["r"], two["H"].T @ two["r"])
    print(f"col-{D} {how} against the two-panel run: eG {eG:.1e}, eg {eg:.1e}")
    assert eG < TOL_G and eg < TOL_g


# --------------------------------------------------------------------------- what must not move
def test_switch_at_0_keeps_its_bits(Updater):
    case = sma.BY_ID["col-300"]
    off, never = case_compress(Updater, case, 0), case_compress(Updater, case, None)
    assert off["ran"] == never["ran"] == sma.HOUSEHOLDER and off["count"] == 0 and off["rows"] == 300 and off["kernel"] == 0
    assert_same_bits(off, never, "slam_mode_a = 0 against never set")


@pytest.mark.parametrize("what,optkw", [("tsqr", dict(compress_route=capi.COMPRESS_TSQR)), ("fp32", dict(gram_fp32=1)), ("no-whiten", dict(gram_no_whiten=1))])
def test_off_the_route_compress_keeps_its_bits(Updater, what, optkw):
    case = sma.BY_ID["col-300"]
    on, never = case_compress(Updater, case, 1, debug=dict(slam_fused=2), **optkw), case_compress(Updater, case, None, **optkw)
    assert on["ran"] == never["ran"] == sma.HOUSEHOLDER and on["count"] == 0 and on["rows"] == 300 and on["kernel"] == 0 and on["fused_batches"] == 0
    assert_same_bits(on, never, f"ovgpu_slam_compress at 300 columns, {what}")


def test_semi_definite_prior_repeats_through_householder(Updater, oracle):
    """the two newest clones perfectly correlated: the prior block's pivot fails, compress_impl repeats the call through the Householder route with
    the bits of a context that never named the switch, neither counter counts the attempt, and the context serves the positive-definite twin on the
    new route afterwards"""
    good = sma.BY_ID["col-300"]
    bad = ss.semi_definite(good.prob)
    on, up = compress(Updater, bad, good.opts(), 1, keep=True, slam_fused=2)
    never = compress(Updater, bad, good.opts(), None)
    assert on["ran"] == never["ran"] == sma.HOUSEHOLDER and on["count"] == 0 and on["fused_batches"] == 0 and on["kernel"] == 0 and on["rows"] == 300
    assert_same_bits(on, never, "the Householder repeat against a context that never named the switch")
    hand_over(up, good.prob)
    again = compress_on(up, 1)
    up.close()
    assert again["count"] == 1 and again["kernel"] == 5 and again["fused_batches"] == 1  # (the batch observes single-depth landmarks)
    check(oracle, good, again, good.codes(1), "col-300 behind the Householder repeat")


def _slam_update(Updater, case, level, chunks=None):
    up = context(Updater, case.opts(), level)
    up.set_slam_problem(case.prob)
    out = up.slam_update(case.prob.lm_index) if chunks is None else up.slam_update_chunked(case.prob.lm_index, chunks)
    out["route"], out["count"] = up.lib.ovgpu_last_update_route(up._ctx), (up.debug_option(COUNTER) if level is not None else None)
    up.close()
    return out


def test_slam_updates_keep_their_bits(Updater):
    case = sma.BY_ID["col-300"]
    on, never = _slam_update(Updater, case, 1), _slam_update(Updater, case, None)
    assert on["route"] == never["route"] == capi.COMPRESS_GRAM and on["count"] == 0
    assert_same_bits(on, never, "ovgpu_slam_update at 300 columns", UPDATE_KEYS + ("landmarks",))
    first = [0, 4, 8, case.prob.F]
    on, never = _slam_update(Updater, case, 1, first), _slam_update(Updater, case, None, first)
    assert on["count"] == 0
    assert_same_bits(on, never, "ovgpu_slam_update_chunked at 300 columns", ("feat_status", "chi2", "chi2_thresh", "dx_seq", "P", "landmarks"))


def _msckf(Updater, oracle, case, tri, level, entry):
    up = context(Updater, case.opts(), level)
    up.set_problem(case.prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    out = up.compress() if entry == "compress" else up.update()
    out["ran"], out["count"] = ran_of(up), (up.debug_option(COUNTER) if level is not None else None)
    up.close()
    return out


def test_msckf_entries_keep_their_bits(Updater, oracle):
    case = mas.BY_ID["col-300"]
    tri = mas.reference(oracle, case)["tri"]
    on, never = _msckf(Updater, oracle, case, tri, 1, "compress"), _msckf(Updater, oracle, case, tri, None, "compress")
    assert on["ran"] == never["ran"] == mas.codes(mas.expected(300)) and on["ran"][3] == 3 and on["count"] == 0  # k_unwhiten<24> stays the MSCKF entry's
    assert_same_bits(on, never, "ovgpu_msckf_compress at 300 columns")
    ucase = gws.MSCKF_BY_ID["f-208"]
    tri, _ = gws.msckf_oracle_run(oracle, ucase)
    on, never = _msckf(Updater, oracle, ucase, tri, 1, "update"), _msckf(Updater, oracle, ucase, tri, None, "update")
    assert on["ran"][0] == never["ran"][0] == capi.COMPRESS_GRAM and on["count"] == 0
    assert_same_bits(on, never, "ovgpu_msckf_update at 208 columns", UPDATE_KEYS + ("p_FinG",))


def test_512_columns_are_refused_as_before(Updater):
    p = gws.over_the_bound()
    msgs = []
    for level in (1, None):
        up = context(Updater, capi.default_options(chi2_multipler=1.0), level, wide=1 if level else 0)
        up.set_slam_problem(p)
        with pytest.raises(capi.OvgpuError) as e:
            up.slam_compress()
        assert e.value.code == capi.ERR_CAPACITY
        msgs.append(str(e.value))
        up.close()
    assert msgs[0] == msgs[1] and "512 Jacobian columns, more than 511" in msgs[0]


# --------------------------------------------------------------------------- the switch
def test_the_switch(Updater, oracle):
    case = sma.BY_ID["col-300"]
    up = Updater(case.opts())
    assert up.debug_option("slam_mode_a") == 0                                              # the default stays 0
    assert up.debug_option("slam_mode_a", 1) == 0 and up.debug_option("slam_mode_a") == 1   # reads back 1
    assert up.debug_option("slam_mode_a", 7) == 1 and up.debug_option("slam_mode_a") == 1   # a large value is taken as the highest level
    assert up.debug_option(COUNTER, 5) == 0 and up.debug_option(COUNTER) == 0               # read only
    assert up.debug_option("mode_a_wide") == 0 and up.debug_option("slam_fused") == 0       # independent of the other switches
    up.close()
    never = case_compress(Updater, case, None)
    # thrown after the batch was handed over: the resident batch keeps the Householder route, the next ovgpu_set_features takes the switch
    up = context(Updater, case.opts(), 0)
    hand_over(up, case.prob)
    up.debug_option("slam_mode_a", 1)
    first = compress_on(up, 0)
    assert first["ran"] == sma.HOUSEHOLDER and first["count"] == 0
    assert_same_bits(first, never, "the switch thrown behind ovgpu_set_features")
    up.set_features(case.prob)
    second = compress_on(up, 1)
    up.close()
    assert second["count"] == 1
    check(oracle, case, second, case.codes(1), "col-300 after the switch was thrown and the batch handed over again")


# --------------------------------------------------------------------------- sequences
@pytest.mark.parametrize("cid", ["col-300", "wide-511"])
def test_same_bits_twice_from_reset_state(Updater, cid):
    case = sma.BY_ID[cid]
    first, up = case_compress(Updater, case, 1, keep=True)
    up.reset_state()
    up.set_features(case.prob)
    second = compress_on(up, 1)
    up.close()
    assert second["ran"] == first["ran"] == case.codes(1) and second["count"] == 2
    assert_same_bits(first, second, f"{cid}: the same call twice from ovgpu_reset_state")


def test_one_context_383_then_128_then_300(Updater):
    """every link returns a fresh context's bits: nothing of the wider (or narrower) compression before it is left in a workspace"""
    cases = [sma.BY_ID[c] for c in sma.HYGIENE_CHAIN]
    up = context(Updater, cases[0].opts(), 1)
    for n, case in enumerate(cases):
        hand_over(up, case.prob)
        link = compress_on(up, 1)
        fresh = case_compress(Updater, case, 1)
        assert link["ran"] == fresh["ran"] == case.codes(1) and link["count"] == n + 1
        assert_same_bits(link, fresh, f"{case.id} as a link of the chain against a fresh context")
    up.close()


def test_compress_then_update_on_one_context(Updater):
    """compress at 300 columns on the new route, then ovgpu_slam_update on the same context: the update's two factorisations reuse the slots of the
    inverse tiles the un-whitening read; it returns a fresh context's bits"""
    case = sma.BY_ID["col-300"]
    cmp, up = case_compress(Updater, case, 1, keep=True)
    assert cmp["ran"] == case.codes(1) and cmp["count"] == 1
    out = up.slam_update(case.prob.lm_index)
    assert up.lib.ovgpu_last_update_route(up._ctx) == capi.COMPRESS_GRAM and up.debug_option(COUNTER) == 1
    up.close()
    fresh = _slam_update(Updater, case, 1)
    assert_same_bits(out, fresh, "ovgpu_slam_update behind a compression against a fresh context", UPDATE_KEYS + ("landmarks",))


REPLAY_REPS = [0, 2, ss.SINGLE, 4, 1, 3, ss.SINGLE, 0, 2, 4, 1, 3]
REPLAY_FIRST = [0, 4, 8, 12]


def _replay(Updater, oracle, opts, q, first, level):
    """per chunk: set_state / set_landmarks / set_active_landmarks / set_features / slam_compress, the oracle's EKFUpdate on what came back, the next
    chunk linearised at the result (Landmark::update: single depth moves rho alone)"""
    cur, dx_sum, status = copy.copy(q), np.zeros(q.N), np.zeros(q.F, np.int32)
    single = np.asarray(q.lm_rep_each) == ss.SINGLE
    up = context(Updater, opts, level)
    for a, b in zip(first[:-1], first[1:]):
        qk = cur.subset(np.arange(a, b))
        qk.lm_index = np.ascontiguousarray(q.lm_index[a:b], dtype=np.int32)
        hand_over(up, qk, active=np.unique(qk.lm_index))
        cmp = up.slam_compress()
        status[a:b] = cmp["feat_status"]
        st, P1, dx = oracle.ekf_update(cur.P, cmp["H"], cmp["r"], cmp["col_cov_id"], 1.0)
        assert st == 0
        post = oracle.apply_dx(opts, capi.Views(qk), dx)
        lm = np.array(cur.lm_value, dtype=np.float64)
        for l in range(lm.shape[0]):
            c0 = int(q.lm_cov_id[l])
            lm[l] += np.array([0.0, 0.0, dx[c0]]) if single[l] else dx[c0:c0 + 3]
        cur = copy.copy(cur)
        cur.P, cur.lm_value = P1, lm
        cur.clone_q_p, cur.calib_q_p, cur.intrinsics = post["clone_q_p"], post["calib_q_p"], post["intrinsics"]
        dx_sum += dx
    count = up.debug_option(COUNTER) if level is not None else 0
    up.close()
    return dict(P=np.asarray(cur.P), dx=dx_sum, feat_status=status, count=count, landmarks=np.asarray(cur.lm_value))


def test_three_chunk_replay(Updater, oracle):
    """three chunks of four landmarks through ovgpu_slam_compress and the stock EKFUpdate, against three oracle.slam_update calls; the same replay
    on the Householder route for comparison"""
    opts = capi.default_options(chi2_multipler=1.0)
    q = ss.slam(12, REPLAY_REPS, 3)
    ref = sc.oracle_chain(oracle, opts, q, REPLAY_FIRST)
    assert ref["near_gate"] == 0 and min(ref["n_used"]) >= 1
    new, old = _replay(Updater, oracle, opts, q, REPLAY_FIRST, 1), _replay(Updater, oracle, opts, q, REPLAY_FIRST, None)
    dx_ref = ref["dx_seq"].sum(axis=0)
    for name, out in (("pivoted route", new), ("Householder route", old)):
        print(f"three-chunk replay, {name}: P {_rel(out['P'], ref['P']):.2e}  dx {_rel(out['dx'], dx_ref):.2e}  landmarks {np.abs(out['landmarks'] - ref['landmarks']).max():.2e}")
    assert new["count"] == 3 and old["count"] == 0
    for out in (new, old):
        assert np.array_equal(out["feat_status"], ref["feat_status"])
        assert _rel(out["P"], ref["P"]) < TOL_P and _rel(out["dx"], dx_ref) < TOL_DX


def test_zz_worst_deviations():
    """prints the worst deviations per kernel family over the runs of this process"""
    for fam in sorted(WORST):
        eG, eg, eP, edx, big, n = WORST[fam]
        print(f"{fam}: {n} runs, worst eG {eG:.1e} (bound {TOL_G:g}), eg {eg:.1e} ({TOL_g:g}), P' {eP:.1e} ({TOL_P:g}), dx {edx:.1e} ({TOL_DX:g}), "
              f"largest noise row {big:.1e} ({NOISE_ROW:g})")
