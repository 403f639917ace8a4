"""GPU tests (`-m gpu`) of mode A's pivoted Gram route at 256 .. 383 Jacobian columns on the panelled factor, selected with ovgpu_debug_option
"mode_a_panel" = 1 and off by default: 17 .. 24 tile columns of [H | r] go to k_pchol_panel / k_pchol_schur (k_pchol_wide.h) instead of the
rank-one k_gram_pchol<9 .. 12>, and ovgpu_msckf_compress un-whitens 257 .. 383 columns with k_unwhiten_blk<24>, as ovgpu_slam_compress does.
15 and 16 tile columns (224 .. 255 columns) keep the rank-one k_gram_pchol<8>: the cases there are held to the same checks on the kernels they
keep, bit-equal to a context that never named the switch.  All through the C ABI, the oracle's triangulation injected on both sides of the MSCKF
entry.  The batches and what each is named for: tests/mode_a_panel_shapes.py (tests/test_mode_a_panel_shapes_cpu.py vets every one on the oracle
alone).

Per case, every assertion of tests/test_gpu_mode_a_wide.py's check (ovgpu_slam_compress: tests/test_gpu_slam_mode_a.py's): the reported route and
the three kernel codes equal the restated rule; feat_status the oracle's; the GENUINE rank equal to the emulation's, the rows beyond it noise rows
only, each under 1e-7; |H^T H - G| / |G| < 1e-11 and |H^T r - g| / |g| < 1e-10; (H, r) through the oracle's EKFUpdate within TOL_P / TOL_DX; the
resident covariance bit-equal to the prior; "mode_a_panel_compressions" one higher.  The highest level the library keeps is 1 (a second level — a
panel kernel with row read-ahead — was measured slower and left out: DESIGN.md section 7), so a value above it must return level 1's bits.

Then: the prior factored step-wise and "unwhiten_blocked" = 0 (un-whitening code 7), held to the two-panel run; a semi-definite prior (the
Householder repeat, not counted, the bits of a context that never named the switch, the context usable afterwards); what must not move, bit for
bit against a context that never named the switch; the switch itself; context hygiene.

On a library without the switch every route assertion fails: "mode_a_panel" is an unknown name there.

Measured on one MI355X, 52 tests in 14.2 s.  Worst over the file's runs, eG / eg / P' / dx / largest noise row, against the bounds 1e-11 / 1e-10 /
1e-9 / 1e-8 / 1e-7: 2.6e-14 / 8.5e-14 / 2.0e-13 / 1.5e-11 / 2.4e-8 (test_zz_worst_deviations prints them per kernel family).  The genuine rank
equals the emulation's in every run.  The step-wise priors against the two-panel run: eG 2.3e-16, eg 1.7e-16.
"""
import numpy as np
import pytest

import mode_a_panel_shapes as mps
import mode_a_shapes as mas
import mode_a_wide_shapes as maw
import slam_mode_a_shapes as sma
import slam_shapes as ss
import test_gpu_mode_a_wide as tw
import test_gpu_slam_mode_a as tsm
from open_vins_amd import capi
from test_gpu_parity import TOL_DX, TOL_P

pytestmark = pytest.mark.gpu

TOL_G, TOL_g = tw.TOL_G, tw.TOL_g     # 1e-11, 1e-10
NOISE_ROW = mas.GAP[0]
SWITCH, COUNTER = "mode_a_panel", "mode_a_panel_compressions"
COMPRESS_KEYS = tw.COMPRESS_KEYS
TOP = mps.TOP_LEVEL
LEVELS = tuple(sorted({1, TOP}))   # level 1 and the highest level kept
M, S = mps.MSCKF, mps.SLAM
HOUSEHOLDER = sma.HOUSEHOLDER
WORST = {}                            # kernel family -> [eG, eg, P', dx, largest noise row, runs], of the runs of THIS process
RUNS = {}                             # (entry, case id, level) -> the compression, for the level-against-level comparison


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def context(Updater, opts, level, **debug):
    """a context with "mode_a_panel" (and the other switches) set before anything is uploaded; level = None never names it"""
    up = Updater(opts)
    if level is not None:
        up.debug_option(SWITCH, level)
    for name, val in debug.items():
        up.debug_option(name, val)
    return up


def compress_on(up, level, slam=False):
    """one compression on a context that holds its batch: the result with what the library says it ran, the counter and the resident state"""
    before = up.get_landmarks() if slam else None
    out = up.slam_compress() if slam else up.compress()
    out["ran"], out["P_after"] = tw.ran_of(up), up.get_state()["P"]
    out["count"] = up.debug_option(COUNTER) if level is not None else None
    if slam:
        out["kernel"], out["lm_before"], out["lm_after"] = up.debug_option("last_feature_kernel"), before, up.get_landmarks()
    return out


def msckf_run(Updater, oracle, case, level, keep=False, debug=None, prob=None, tri=None, **optkw):
    up = context(Updater, case.opts(**optkw), level, **(debug or {}))
    tw.hand_over(up, case.prob if prob is None else prob, mas.reference(oracle, case)["tri"] if tri is None else tri)
    out = compress_on(up, level)
    if keep:
        return out, up
    up.close()
    return out


def slam_run(Updater, case, level, slam_level=1, keep=False, debug=None, **optkw):
    debug = dict(debug or {})
    if slam_level is not None:
        debug["slam_mode_a"] = slam_level
    up = context(Updater, case.opts(**optkw), level, **debug)
    tsm.hand_over(up, case.prob, case.active, case.sigma, case.mult)
    out = compress_on(up, level, slam=True)
    if keep:
        return out, up
    up.close()
    return out


def check(oracle, entry, case, cmp, want, label):
    """the sibling file's check with its figures booked under THIS file's kernel families; returns the genuine rank"""
    mod = tw if entry == M else tsm
    saved, mod.WORST = mod.WORST, {}
    try:
        rank = mod.check(oracle, case, cmp, want, label)
    finally:
        mine, mod.WORST = mod.WORST, saved
    for fig in mine.values():
        w = WORST.setdefault(f"{mps.family(want)} [{entry}]", [0.0, 0.0, 0.0, 0.0, 0.0, 0])
        w[:] = [max(a, b) for a, b in zip(w[:5], fig[:5])] + [w[5] + fig[5]]
    return rank


def get_run(Updater, oracle, entry, cid, level):
    key = (entry, cid, level)
    if key not in RUNS:
        RUNS[key] = msckf_run(Updater, oracle, mps.MSCKF_BY_ID[cid], level) if entry == M else slam_run(Updater, mps.SLAM_BY_ID[cid], level)
    return RUNS[key]


# --------------------------------------------------------------------------- the route, case by case
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("cid", mps.MSCKF_IDS)
def test_msckf_route(Updater, oracle, cid, level):
    case = mps.MSCKF_BY_ID[cid]
    want, band = mps.expected_codes(case.D, level), mps.in_band(case.D)
    assert want[0] == capi.COMPRESS_PCHOLQR and want[2] == (mps.FACTOR_PANEL if band else 40) and band == (case.D >= 256)
    assert want[3] == (sma.UNWHITEN_BLK24_TILES if case.D > 256 else 1)
    cmp = get_run(Updater, oracle, M, cid, level)
    rank = check(oracle, M, case, cmp, want, f"{cid} level {level}")
    assert cmp["count"] == (1 if band else 0)  # (every feature rejected: rows 0 with OVGPU_OK, and the route was taken)
    if not band:
        tw.assert_same_bits(cmp, msckf_run(Updater, oracle, case, None), f"{cid}: below the edge, against a context that never named the switch")
    if case.group == "rank":
        assert rank == case.R and cmp["rows"] < case.D


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("cid", mps.SLAM_IDS)
def test_slam_route(Updater, oracle, cid, level):
    case = mps.SLAM_BY_ID[cid]
    want, band = mps.slam_codes(case, level), mps.in_band(case.columns)
    assert want[0] == capi.COMPRESS_PCHOLQR and want[2] == (mps.FACTOR_PANEL if band else 40) and band == (case.columns >= 256)
    cmp = get_run(Updater, oracle, S, cid, level)
    rank = check(oracle, S, case, cmp, want, f"slam {cid} level {level}")
    assert cmp["count"] == (1 if band else 0) and cmp["kernel"] == 0
    if not band:
        tw.assert_same_bits(cmp, slam_run(Updater, case, None), f"slam {cid}: below the edge, against a context that never named the switch")
    if case.rows is not None:
        assert rank == case.rows and cmp["rows"] < case.columns


@pytest.mark.parametrize("entry,cid", [(M, "col-300"), (M, "col-382"), (S, "col-319")])
def test_a_level_above_the_top_returns_its_bits(Updater, oracle, entry, cid):
    """values above the highest level kept are taken as it: the same kernels, the same bits"""
    one, two = get_run(Updater, oracle, entry, cid, TOP), get_run(Updater, oracle, entry, cid, TOP + 1)
    assert one["ran"] == two["ran"] and one["ran"][2] == mps.FACTOR_PANEL and two["count"] == 1
    tw.assert_same_bits(one, two, f"{entry} {cid}: level {TOP + 1} against level {TOP}")


# --------------------------------------------------------------------------- prior variants
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("how", ["no_single_launch_cholesky", "chol_wide_0", "unwhiten_blocked_0"])
def test_stepwise_prior(Updater, oracle, how, level):
    """the prior factored step-wise (or the blocked un-whitening's switch off): no inverse tiles from the factorisation, k_uinv_tiles makes them"""
    case = mps.MSCKF_BY_ID["col-300"]
    optkw = dict(no_single_launch_cholesky=1) if how == "no_single_launch_cholesky" else {}
    debug = dict(chol_wide=0) if how == "chol_wide_0" else (dict(unwhiten_blocked=0) if how == "unwhiten_blocked_0" else {})
    want = mps.expected_codes(300, level, two_panel=how == "unwhiten_blocked_0", unwhiten_blocked=how != "unwhiten_blocked_0")
    assert want[3] == sma.UNWHITEN_BLK24_INVERTED
    cmp = msckf_run(Updater, oracle, case, level, debug=debug, **optkw)
    rank = check(oracle, M, case, cmp, want, f"col-300 {how} level {level}")
    assert cmp["count"] == 1
    two = get_run(Updater, oracle, M, "col-300", level)
    assert two["ran"] == mps.expected_codes(300, level) and two["rows"] == cmp["rows"] and mas.genuine_rank(two["H"]) == rank
    eG, eg = _rel(cmp["H"].T @ cmp["H"], two["H"].T @ two["H"]), _rel(cmp["H"].T @ cmp["r"], two["H"].T @ two["r"])
    print(f"col-300 {how} level {level} against the two-panel run: eG {eG:.1e}, eg {eg:.1e}")
    assert eG < TOL_G and eg < TOL_g


def test_semi_definite_prior_repeats_through_householder(Updater, oracle):
    """the two newest clones perfectly correlated at 300 columns: the prior block's pivot fails, compress_impl repeats the call through the
    Householder route with the bits of a context that never named the switch, the attempt is not counted, and the context serves the
    positive-definite twin on the new route afterwards"""
    good = mps.MSCKF_BY_ID["col-300"]
    bad = ss.semi_definite(good.prob)
    tri = oracle.triangulate(good.opts(), capi.Views(bad))
    on, up = msckf_run(Updater, oracle, good, TOP, keep=True, prob=bad, tri=tri)
    never = msckf_run(Updater, oracle, good, None, prob=bad, tri=tri)
    assert on["ran"] == never["ran"] == HOUSEHOLDER and on["count"] == 0 and on["rows"] == never["rows"] == 300
    tw.assert_same_bits(on, never, "the Householder repeat against a context that never named the switch")
    tw.hand_over(up, good.prob, mas.reference(oracle, good)["tri"])
    again = compress_on(up, TOP)
    up.close()
    assert again["count"] == 1
    check(oracle, M, good, again, mps.expected_codes(300, TOP), "col-300 behind the Householder repeat")


# --------------------------------------------------------------------------- what must not move
def test_below_the_band_keeps_its_bits(Updater, oracle):
    case = mps.BELOW
    on, never = msckf_run(Updater, oracle, case, TOP), msckf_run(Updater, oracle, case, None)
    assert on["ran"] == never["ran"] == mps.expected_codes(222, TOP) == mas.codes(mas.expected(222)) and on["count"] == 0
    tw.assert_same_bits(on, never, "ovgpu_msckf_compress at 222 columns")
    case = mps.SLAM_BELOW
    on, never = slam_run(Updater, case, TOP), slam_run(Updater, case, None)
    assert case.columns == 223 and on["ran"] == never["ran"] == mps.slam_codes(case, TOP) == case.codes(1) and on["count"] == 0
    tw.assert_same_bits(on, never, "ovgpu_slam_compress at 223 columns")


@pytest.mark.parametrize("wide", [0, 1])
def test_384_columns_keep_their_bits(Updater, oracle, wide):
    case = mps.ABOVE
    on, never = msckf_run(Updater, oracle, case, TOP, debug=dict(mode_a_wide=wide)), msckf_run(Updater, oracle, case, None, debug=dict(mode_a_wide=wide))
    assert on["ran"] == never["ran"] == mps.expected_codes(384, TOP, wide=wide) == maw.expected_codes(384, wide) and on["count"] == 0
    tw.assert_same_bits(on, never, f"ovgpu_msckf_compress at 384 columns, mode_a_wide {wide}")


def test_slam_compress_without_slam_mode_a_keeps_its_bits(Updater):
    case = mps.SLAM_BY_ID["col-300"]
    on, never = slam_run(Updater, case, TOP, slam_level=None), slam_run(Updater, case, None, slam_level=None)
    assert on["ran"] == never["ran"] == HOUSEHOLDER == mps.slam_codes(case, TOP, slam_level=0) and on["count"] == 0 and on["rows"] == 300
    tw.assert_same_bits(on, never, "ovgpu_slam_compress at 300 columns without slam_mode_a")


@pytest.mark.parametrize("what,optkw", [("tsqr", dict(compress_route=capi.COMPRESS_TSQR)), ("fp32", dict(gram_fp32=1)), ("no-whiten", dict(gram_no_whiten=1))])
def test_off_the_route_compress_keeps_its_bits(Updater, oracle, what, optkw):
    case = mps.MSCKF_BY_ID["col-300"]
    on, never = msckf_run(Updater, oracle, case, TOP, **optkw), msckf_run(Updater, oracle, case, None, **optkw)
    want = mps.expected_codes(300, TOP, compress_route=optkw.get("compress_route", capi.COMPRESS_GRAM), fp32=optkw.get("gram_fp32", 0), whiten=not optkw.get("gram_no_whiten", 0))
    assert on["ran"] == never["ran"] == want == HOUSEHOLDER and on["count"] == 0 and on["rows"] == 300
    tw.assert_same_bits(on, never, f"ovgpu_msckf_compress at 300 columns, {what}")


def test_updates_keep_their_bits(Updater, oracle):
    case = mps.MSCKF_BY_ID["col-300"]
    tri = mas.reference(oracle, case)["tri"]
    outs = []
    for level in (TOP, None):
        up = context(Updater, case.opts(), level)
        tw.hand_over(up, case.prob, tri)
        out = up.update()
        assert up.lib.ovgpu_last_update_route(up._ctx) == capi.COMPRESS_GRAM and (level is None or up.debug_option(COUNTER) == 0)
        up.close()
        outs.append(out)
    tw.assert_same_bits(outs[0], outs[1], "ovgpu_msckf_update at 300 columns", tw.UPDATE_KEYS)
    on, never = _slam_update(Updater, TOP), _slam_update(Updater, None)
    tw.assert_same_bits(on, never, "ovgpu_slam_update at 300 columns", tsm.UPDATE_KEYS + ("landmarks",))


def _slam_update(Updater, level):
    case = mps.SLAM_BY_ID["col-300"]
    up = context(Updater, case.opts(), level, slam_mode_a=1)
    up.set_slam_problem(case.prob)
    out = up.slam_update(case.prob.lm_index)
    assert up.lib.ovgpu_last_update_route(up._ctx) == capi.COMPRESS_GRAM and (level is None or up.debug_option(COUNTER) == 0)
    up.close()
    return out


# --------------------------------------------------------------------------- the switch
def test_the_switch(Updater, oracle):
    case = mps.MSCKF_BY_ID["col-300"]
    R = mas.reference(oracle, case)
    up = Updater(case.opts())
    assert up.debug_option(SWITCH) == 0                                                  # the default stays 0
    assert up.debug_option(SWITCH, 1) == 0 and up.debug_option(SWITCH) == 1              # reads back 1
    assert up.debug_option(SWITCH, 7) == 1 and up.debug_option(SWITCH) == TOP == 1       # values above the top level are taken as it
    assert up.debug_option(COUNTER, 5) == 0 and up.debug_option(COUNTER) == 0            # read only
    assert up.debug_option("mode_a_wide") == 0 and up.debug_option("slam_mode_a") == 0   # independent of the other switches
    up.close()
    never, off = msckf_run(Updater, oracle, case, None), msckf_run(Updater, oracle, case, 0)
    assert never["ran"] == off["ran"] == mas.codes(mas.expected(300)) == mps.expected_codes(300, 0) and off["count"] == 0
    tw.assert_same_bits(off, never, "mode_a_panel = 0 against never set")
    # thrown after the batch was handed over: the resident batch keeps the rank-one factor, the next ovgpu_set_features takes the switch
    up = context(Updater, case.opts(), 0)
    tw.hand_over(up, case.prob, R["tri"])
    up.debug_option(SWITCH, TOP)
    first = compress_on(up, 0)
    assert first["ran"] == never["ran"] and first["count"] == 0
    tw.assert_same_bits(first, never, "the switch thrown behind ovgpu_set_features")
    up.reset_state()
    up.set_features(case.prob)
    tri = R["tri"]
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    second = compress_on(up, TOP)
    up.close()
    assert second["count"] == 1
    check(oracle, M, case, second, mps.expected_codes(300, TOP), "col-300 after the switch was thrown and the batch handed over again")


# --------------------------------------------------------------------------- context hygiene
@pytest.mark.parametrize("cid", ["col-300", "rank-300-R33"])
def test_same_bits_twice_from_reset_state(Updater, oracle, cid):
    case = mps.MSCKF_BY_ID[cid]
    tri = mas.reference(oracle, case)["tri"]
    first, up = msckf_run(Updater, oracle, case, TOP, keep=True)
    up.reset_state()
    up.set_features(case.prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    second = compress_on(up, TOP)
    up.close()
    assert second["ran"] == first["ran"] == mps.expected_codes(300, TOP) and second["count"] == 2
    tw.assert_same_bits(first, second, f"{cid}: the same call twice from ovgpu_reset_state")


def test_one_context_382_then_208_then_300(Updater, oracle):
    """every link returns a fresh context's bits: nothing of the wider (or narrower) compression before it is left in a workspace"""
    cases = [mps.MSCKF_BY_ID[c] if isinstance(c, str) else c for c in mps.HYGIENE_CHAIN]
    up = context(Updater, cases[0].opts(), TOP)
    count = 0
    for case in cases:
        tw.hand_over(up, case.prob, mas.reference(oracle, case)["tri"])
        link = compress_on(up, TOP)
        fresh = msckf_run(Updater, oracle, case, TOP)
        count += 1 if mps.in_band(case.D) else 0
        assert link["ran"] == fresh["ran"] == mps.expected_codes(case.D, TOP) and link["count"] == count
        tw.assert_same_bits(link, fresh, f"{case.id} as a link of the chain against a fresh context")
    up.close()
    assert count == 2


def test_compress_then_slam_update_on_one_context(Updater):
    """ovgpu_slam_compress at 300 columns on the new route, then ovgpu_slam_update on the same context: it returns a fresh context's bits"""
    case = mps.SLAM_BY_ID["col-300"]
    cmp, up = slam_run(Updater, case, TOP, keep=True)
    assert cmp["ran"] == mps.slam_codes(case, TOP) and cmp["count"] == 1
    out = up.slam_update(case.prob.lm_index)
    assert up.lib.ovgpu_last_update_route(up._ctx) == capi.COMPRESS_GRAM and up.debug_option(COUNTER) == 1
    up.close()
    tw.assert_same_bits(out, _slam_update(Updater, TOP), "ovgpu_slam_update behind a compression against a fresh context", tsm.UPDATE_KEYS + ("landmarks",))


def test_zz_worst_deviations():
    """prints the worst deviations per kernel family over the runs of this process"""
    for fam in sorted(WORST):
        eG, eg, eP, edx, big, n = WORST[fam]
        print(f"{fam}: {n} runs, worst eG {eG:.1e} (bound {TOL_G:g}), eg {eg:.1e} ({TOL_g:g}), P' {eP:.1e} ({TOL_P:g}), dx {edx:.1e} ({TOL_DX:g}), "
              f"largest noise row {big:.1e} ({NOISE_ROW:g})")
