"""GPU parity tests (run with `-m gpu` on an MI355X): the HIP path, called through the C ABI, against the CPU
oracle on identical seeded inputs.

Tolerances (floating point path; stated per SURVEY.md §8c and confirmed by measurement):
  * triangulation + Gauss-Newton: |p_FinG - oracle| <= 1e-9 m for every feature (measured max 5e-11 m over
    776 features).  The LM loop of the reference accepts / rejects steps on float32-rounded costs (Q3); the
    kernels reproduce every float rounding of that path (no FMA contraction of float products, correctly
    rounded float sqrt), so the same branches are taken and only double round-off from the summation order
    (serial in the oracle, wavefront butterfly on the GPU) remains.
  * everything after loop A, with the SAME positions injected on both sides: chi2 rel 1e-8, dx rel 1e-8,
    P rel-Frobenius 1e-9, identical accept / reject sets (features within 1e-8 of the gate — parity_util.GATE_MARGIN, the chi2 tolerance — are excused).
  * end to end (positions triangulated on each side): same bounds as with injected positions, relaxed by 10x.
"""
import numpy as np
import pytest

from open_vins_amd import capi, synth
import tsqr_shapes as ts
from parity_util import assert_chi2, oracle_with_the_same_gate_verdicts

pytestmark = pytest.mark.gpu

TOL_TRI = 1e-9
TOL_CHI2 = 1e-8
TOL_DX = 1e-8
TOL_P = 1e-9


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _check_tri(out, ref, ok):
    assert np.abs(out["p_FinG"][ok] - ref["p_FinG"][ok]).max() < TOL_TRI
    assert np.abs(out["p_FinA"][ok] - ref["p_FinA"][ok]).max() < TOL_TRI


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _check_given(Updater, oracle, prob, opts, tol_dx=TOL_DX, tol_p=TOL_P, require_gate=True, debug=None):
    """Injects the oracle's triangulation on both sides and compares everything downstream.
    debug: ovgpu_debug_option settings of the contexts (e.g. the per-feature kernel's shape)."""
    v = capi.Views(prob)
    tri = oracle.triangulate(opts, v)
    ref = oracle.msckf_update(opts, v, want_compressed=True, given=tri)
    up = Updater(opts)
    for name, val in (debug or {}).items():
        up.debug_option(name, val)
    up.set_problem(prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    out = up.update()
    # accept / reject sets: identical, or (features within parity_util.GATE_MARGIN = 1e-8 of the gate) the oracle re-run with the GPU's verdicts — dx / P are
    # compared either way
    ref = oracle_with_the_same_gate_verdicts(oracle, opts, v, tri, ref, out)
    diff = np.nonzero(out["feat_status"] != ref["feat_status"])[0]
    assert len(diff) == 0
    gate = np.isfinite(ref["chi2"])
    assert gate.sum() > 0 or not require_gate
    if gate.sum() == 0:  # nothing triangulated: the update is a no-op on both sides
        assert len(diff) == 0 and not out["dx"].any() and np.array_equal(out["P"], prob.P)
        up.close()
        return out, ref
    assert_chi2(out, ref, TOL_CHI2, strict=bool(opts.gate_always_factor))
    np.testing.assert_allclose(out["chi2_thresh"][gate], ref["chi2_thresh"][gate], rtol=1e-12)
    if len(diff) == 0:
        assert out["stats"]["n_used"] == ref["stats"]["n_used"]
        assert out["stats"]["n_rows"] == ref["stats"]["n_rows"]
        assert _rel(out["dx"], ref["dx"]) < tol_dx
        assert _rel(out["P"], ref["P"]) < tol_p
        assert np.abs(out["clone_q_p"] - ref["clone_q_p"]).max() < 1e-9
        assert np.abs(out["calib_q_p"] - ref["calib_q_p"]).max() < 1e-9
        assert np.abs(out["intrinsics"] - ref["intrinsics"]).max() < 1e-8
        assert np.array_equal(out["P"], out["P"].T)
    up.close()
    if not opts.gate_always_factor:
        # ... and once more with every gate matrix formed and factored: every chi2 is then the reference's statistic, and the
        # update is the one the residual bound's shortcut gave (same accept sets; the stack differs by nothing)
        full = capi.default_options(**{k: getattr(opts, k) for k, _ in opts._fields_ if not k.startswith("_")})
        full.gate_always_factor = 1
        up = Updater(full)
        for name, val in (debug or {}).items():
            up.debug_option(name, val)
        up.set_problem(prob)
        up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
        out1 = up.update()
        up.close()
        assert_chi2(out1, ref, TOL_CHI2, strict=True)
        # (features that take the full gate run the same code in both modes; a bound only ever accepts 1e-9 under the threshold)
        assert np.array_equal(out1["feat_status"], out["feat_status"])
        assert _rel(out1["dx"], out["dx"]) < 1e-12 and _rel(out1["P"], out["P"]) < 1e-12
    return out, ref


# --------------------------------------------------------------------------- loop A
@pytest.mark.parametrize("kw", [dict(), dict(track="ragged"), dict(fisheye=True), dict(K=1, C=12), dict(cfg=4, F=150)])
def test_triangulation_parity(Updater, oracle, kw):
    kw = dict(kw)
    prob = synth.make_problem(kw.pop("cfg", 2), F=kw.pop("F", 300), **kw)
    opts = capi.default_options()
    ref = oracle.triangulate(opts, capi.Views(prob))
    up = Updater(opts)
    up.set_problem(prob)
    out = up.triangulate()
    assert np.array_equal(out["anchor_meas"], ref["anchor_meas"])
    same = out["status"] == ref["status"]
    assert same.all()
    ok = same & (ref["status"] == capi.FEAT_USED)
    assert ok.sum() > 0.5 * prob.F
    _check_tri(out, ref, ok)
    up.close()


def test_triangulation_1d_parity(Updater, oracle):
    prob = synth.make_problem(2, F=200)
    opts = capi.default_options(triangulate_1d=1)
    ref = oracle.triangulate(opts, capi.Views(prob))
    up = Updater(opts)
    up.set_problem(prob)
    out = up.triangulate()
    ok = (out["status"] == ref["status"]) & (ref["status"] == capi.FEAT_USED)
    assert ok.sum() > 0.5 * prob.F
    _check_tri(out, ref, ok)
    up.close()


def test_triangulation_without_refinement_is_tight(Updater, oracle):
    """Without the LM loop there is no float-cost branch: the linear triangulation agrees to round-off."""
    prob = synth.make_problem(2, F=200)
    opts = capi.default_options(refine_features=0)
    ref = oracle.triangulate(opts, capi.Views(prob))
    up = Updater(opts)
    up.set_problem(prob)
    out = up.triangulate()
    assert np.array_equal(out["status"], ref["status"])
    ok = ref["status"] == capi.FEAT_USED
    assert np.abs(out["p_FinG"][ok] - ref["p_FinG"][ok]).max() < 1e-9
    up.close()


# --------------------------------------------------------------------------- loops B, C and the EKF update (positions injected)
@pytest.mark.parametrize("kw", [
    dict(F=120),
    dict(F=120, track="ragged"),
    dict(F=100, fisheye=True),
    dict(F=100, outlier_frac=0.25),
    dict(F=60, K=1, C=12),
    dict(F=7),
    dict(F=1),
    dict(cfg=4, F=40),
])
def test_update_parity_given_positions(Updater, oracle, kw):
    kw = dict(kw)
    prob = synth.make_problem(kw.pop("cfg", 2), **kw)
    opts = capi.default_options(chi2_multipler=1.0)
    out, ref = _check_given(Updater, oracle, prob, opts)
    if kw.get("outlier_frac"):
        assert np.sum(ref["feat_status"] == capi.FEAT_CHI2_REJECTED) >= 5  # the gate was exercised


@pytest.mark.parametrize("rep", [capi.REP_GLOBAL_FULL_INVERSE_DEPTH, capi.REP_ANCHORED_3D, capi.REP_ANCHORED_FULL_INVERSE_DEPTH,
                                 capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE])
def test_update_parity_feature_representations(Updater, oracle, rep):
    prob = synth.make_problem(2, F=60, C=14)
    _check_given(Updater, oracle, prob, capi.default_options(chi2_multipler=1.0, feat_rep_msckf=rep))


@pytest.mark.parametrize("flags", [dict(do_fej=0), dict(do_calib_camera_pose=0), dict(do_calib_camera_intrinsics=0),
                                   dict(do_calib_camera_pose=0, do_calib_camera_intrinsics=0), dict(sigma_pix=2.0, chi2_multipler=3.0)])
def test_update_parity_state_options(Updater, oracle, flags):
    prob = synth.make_problem(2, F=60, C=14)
    _check_given(Updater, oracle, prob, capi.default_options(**{"chi2_multipler": 1.0, **flags}))


@pytest.mark.parametrize("general", [0, 1])
def test_update_parity_long_tracks(Updater, oracle, general):
    """cfg-5 geometry (50 clones x 4 cameras, up to 200 measurements per feature).  Default: the gate matrix (25 tile rows) is
    factored block row by block row (k_featy_big.h); no_fast_feature_kernel: the general kernel, whose gate matrix no longer fits
    LDS and goes through the HBM workspace."""
    prob = synth.make_problem(5, F=12)
    assert np.diff(prob.meas_offsets).max() > 120
    _check_given(Updater, oracle, prob, capi.default_options(chi2_multipler=1.0, no_fast_feature_kernel=general))


@pytest.mark.parametrize("kw", [dict(F=300), dict(F=200, track="ragged", outlier_frac=0.3), dict(cfg=4, F=100), dict(F=150, C=11, K=1)])
def test_block_row_gate_equals_the_one_pass_gate(Updater, kw):
    """k_feat_y_big (k_featy_big.h) on batches the one-pass kernel holds: with the same tile budget (one pass) and with 5 tiles per
    wavefront (2 .. 5 passes over 8 .. 15 tile rows).  A tile of the gate matrix receives the same updates in the same order
    whatever the pass structure, so chi2 is BIT-identical between the two block-row shapes; the stacked rows differ in the
    summation order of V^T Y only.  Against the one-pass kernel the statistic agrees to rounding of a DIFFERENT elimination (round 5: that
    kernel carries the right-hand sides [r | H_f] as four augmented ROWS of the gate matrix, the block-row kernel as a tile column of their own;
    round 6: it eliminates by 4 x 4 blocks without square roots — block L D L^T, k_feat.h — where the block-row kernel keeps the Cholesky
    form): 1e-9 relative, an order below the suite's own chi2 tolerance against the oracle."""
    kw = dict(kw)
    prob = synth.make_problem(kw.pop("cfg", 2), **kw)
    opts = capi.default_options(chi2_multipler=1.0, gate_always_factor=1)  # the test is about the gate's pass structure
    outs = []
    for big in (0, 1, 2):
        up = Updater(opts)
        assert up.debug_option("featy_big", big) == 0
        up.set_problem(prob)
        outs.append(up.update())
        up.close()
    ref = outs[0]
    gate = np.isfinite(ref["chi2"])
    assert gate.sum() > 0.5 * prob.F
    assert np.array_equal(outs[1]["chi2"][gate], outs[2]["chi2"][gate])
    for out in outs[1:]:
        assert np.array_equal(out["feat_status"], ref["feat_status"])
        np.testing.assert_allclose(out["chi2"][gate], ref["chi2"][gate], rtol=1e-9)
        assert out["stats"]["n_rows"] == ref["stats"]["n_rows"]
        assert _rel(out["dx"], ref["dx"]) < 1e-10
        assert _rel(out["P"], ref["P"]) < 1e-11


@pytest.mark.parametrize("kw", [dict(F=300), dict(F=200, track="ragged", outlier_frac=0.3), dict(cfg=3, F=260)])
def test_batch_tables_rebuilt_on_every_update(Updater, kw):
    """ovgpu_debug_option "layout_every_update": the integer tables ovgpu_set_features derives once per batch (anchor measurements,
    clone-major positions, column-block lists of the tile rows) rebuilt at the head of every update (one launch, k_batch_layout) -- bench.py's
    headline loop since round 6.  The same kernel on the same batch: the update must not change."""
    kw = dict(kw)
    prob = synth.make_problem(kw.pop("cfg", 2), **kw)
    opts = capi.default_options(chi2_multipler=1.0)
    outs = []
    for flag in (0, 1):
        up = Updater(opts)
        assert up.debug_option("layout_every_update", flag) == 0
        up.set_problem(prob)
        outs.append(up.update())
        assert up.debug_option("layout_every_update") == flag
        up.close()
    ref, out = outs
    assert (ref["feat_status"] == capi.FEAT_USED).sum() > 0.3 * prob.F
    assert np.array_equal(out["feat_status"], ref["feat_status"])
    assert out["stats"]["n_rows"] == ref["stats"]["n_rows"]
    assert _rel(out["dx"], ref["dx"]) < 1e-12
    assert _rel(out["P"], ref["P"]) < 1e-12


def test_short_and_empty_tracks(Updater, oracle):
    prob = synth.make_problem(2, F=12)
    keep, offs = [], [0]
    for f in range(prob.F):
        a, b = int(prob.meas_offsets[f]), int(prob.meas_offsets[f + 1])
        if f == 2:
            b = a + 1
        if f == 4:
            b = a
        if f == 6:
            b = a + 2
        keep += list(range(a, b))
        offs.append(offs[-1] + (b - a))
    keep = np.asarray(keep)
    prob.meas_offsets = np.asarray(offs, dtype=np.int32)
    prob.uv = prob.uv.reshape(-1, 2)[keep].reshape(-1)
    prob.uvn = prob.uvn.reshape(-1, 2)[keep].reshape(-1)
    prob.clone_idx, prob.cam_idx = prob.clone_idx[keep], prob.cam_idx[keep]
    opts = capi.default_options(chi2_multipler=1.0)
    out, ref = _check_given(Updater, oracle, prob, opts)
    assert out["feat_status"][2] == capi.FEAT_TOO_FEW_MEAS and out["feat_status"][4] == capi.FEAT_TOO_FEW_MEAS
    # end to end as well (statuses come from the GPU triangulation here)
    up = Updater(opts)
    up.set_problem(prob)
    o2 = up.update()
    assert o2["feat_status"][2] == capi.FEAT_TOO_FEW_MEAS and o2["feat_status"][4] == capi.FEAT_TOO_FEW_MEAS
    up.close()


def test_no_features_is_a_no_op(Updater):
    prob = synth.make_problem(2, F=5)
    empty = prob.subset([])
    up = Updater(capi.default_options())
    up.set_problem(empty)
    out = up.update()
    assert out["stats"]["n_used"] == 0 and out["stats"]["n_rows"] == 0
    np.testing.assert_array_equal(out["P"], prob.P)  # UpdaterMSCKF.cpp:61-62 returns early
    assert np.all(out["dx"] == 0)
    up.close()


def test_all_features_rejected_leaves_state_untouched(Updater):
    prob = synth.make_problem(2, F=20)
    up = Updater(capi.default_options(chi2_multipler=1e-9))
    up.set_problem(prob)
    out = up.update()
    assert out["stats"]["n_used"] == 0
    np.testing.assert_allclose(out["P"], prob.P, rtol=0, atol=0)
    assert np.all(out["dx"] == 0)
    up.close()


# --------------------------------------------------------------------------- end to end + mode A
def test_end_to_end_update(Updater, oracle):
    prob = synth.make_problem(2, F=200)
    opts = capi.default_options(chi2_multipler=1.0)
    ref = oracle.msckf_update(opts, capi.Views(prob))
    up = Updater(opts)
    up.set_problem(prob)
    out = up.update()
    assert np.array_equal(out["feat_status"], ref["feat_status"])
    ok = ref["feat_status"] == 0
    assert np.abs(out["p_FinG"][ok] - ref["p_FinG"][ok]).max() < TOL_TRI
    assert _rel(out["dx"], ref["dx"]) < 10 * TOL_DX
    assert _rel(out["P"], ref["P"]) < 10 * TOL_P
    up.close()


@pytest.mark.parametrize("kw", [dict(no_single_launch_cholesky=1), dict(no_prior_overlap=1), dict(no_single_launch_cholesky=1, no_prior_overlap=1),
                                dict(no_timing=1), dict(feature_kernel_shape=2), dict(no_fast_feature_kernel=1)])
def test_mode_a_default_under_the_library_switches(Updater, oracle, kw):
    """Mode A's default (pivoted factor of the whitened Gram matrix, un-whitened with the prior block's factor) takes that factor from
    whichever factorisation ran — the single-launch Cholesky or the step-wise one, on the side stream or on the main one — and the
    whitened rows from whichever per-feature kernel produced them: same compressed system (Gram matrices 1e-11) and posterior."""
    prob = synth.make_problem(2, F=150)
    v = capi.Views(prob)
    base = capi.default_options(chi2_multipler=1.0)
    tri = oracle.triangulate(base, v)
    ref = oracle.msckf_update(base, v, want_compressed=True, given=tri)
    G, g = ref["H_comp"].T @ ref["H_comp"], ref["H_comp"].T @ ref["r_comp"]
    cmp = _compress_with(Updater, prob, base, tri, **kw)
    H, r = cmp["H"], cmp["r"]
    assert 0 < cmp["rows"] <= cmp["D"] == ref["D"] and np.array_equal(cmp["feat_status"], ref["feat_status"])
    assert np.linalg.norm(H.T @ H - G) / np.linalg.norm(G) < 1e-11 and np.linalg.norm(H.T @ r - g) / np.linalg.norm(g) < 1e-10
    st, P1, dx1 = oracle.ekf_update(prob.P, H, r, cmp["col_cov_id"], 1.0)
    assert st == 0 and _rel(P1, ref["P"]) < TOL_P and _rel(dx1, ref["dx"]) < TOL_DX


@pytest.mark.parametrize("route", ["default", "tsqr"])
def test_mode_a_compressed_system(Updater, oracle, route):
    """ovgpu_msckf_compress hands back (H, r) for the stock StateHelper::EKFUpdate: H^T H and H^T r equal the reference's compressed
    system's, and feeding it to the oracle's EKFUpdate reproduces the oracle's posterior.
    default: the diagonally PIVOTED Cholesky factor of the whitened stack's Gram matrix, un-whitened (k_gram_pchol) — dense, rows =
             its numerical rank, at the Gram route's cost; the closed loop holds it to the Householder level (test_closed_loop.py);
    tsqr:    the triangle of the Householder TSQR, the reference's own form (R is unique up to row signs).
    (The UNPIVOTED factor, rounds 3-5's OVGPU_COMPRESS_CHOLQR — good on a snapshot like this one, drifting in the closed loop — left the
    library in round 6: ovgpu_create refuses the value, test_retired_compress_route_is_refused.)"""
    prob = synth.make_problem(2, F=100)
    code = dict(default=capi.COMPRESS_GRAM, tsqr=capi.COMPRESS_TSQR)[route]
    opts = capi.default_options(chi2_multipler=1.0, compress_route=code)
    v = capi.Views(prob)
    tri = oracle.triangulate(opts, v)
    ref = oracle.msckf_update(opts, v, want_compressed=True, given=tri)
    up = Updater(opts)
    up.set_problem(prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    cmp = up.compress()
    assert cmp["D"] == ref["D"] and (cmp["rows"] == cmp["D"] if route != "default" else 0 < cmp["rows"] <= cmp["D"])
    assert np.array_equal(cmp["col_cov_id"], oracle.column_map(opts, v))
    assert up.lib.ovgpu_last_update_route(up._ctx) == (capi.COMPRESS_PCHOLQR if route == "default" else code)
    H, r = cmp["H"], cmp["r"]
    G = ref["H_comp"].T @ ref["H_comp"]
    g = ref["H_comp"].T @ ref["r_comp"]
    eG, eg = np.linalg.norm(H.T @ H - G) / np.linalg.norm(G), np.linalg.norm(H.T @ r - g) / np.linalg.norm(g)
    print(f"mode A, {route}: |H^T H - G| / |G| = {eG:.1e}, |H^T r - g| / |g| = {eg:.1e}")
    if route == "tsqr":
        assert np.abs(np.tril(H, -1)).max() == 0.0
    assert eG < 1e-11 and eg < 1e-10
    st, P1, dx1 = oracle.ekf_update(prob.P, H, r, cmp["col_cov_id"], 1.0)
    assert st == 0
    assert _rel(P1, ref["P"]) < TOL_P and _rel(dx1, ref["dx"]) < TOL_DX
    # the resident state was not touched by mode A
    np.testing.assert_array_equal(up.get_state()["P"], prob.P)
    up.close()


@pytest.mark.parametrize("cfg,F,track", [(1, 3, "full"), (1, 12, "ragged"), (2, 40, "full"), (2, 400, "ragged"), (3, 600, "full"), (4, 300, "full"),
                                         (5, 60, "full"), (5, 3, "ragged")])  # configs[4]'s geometry: D = 356 columns (round 4: k_gram_pchol<12>, k_unwhiten<24>)
def test_mode_a_pivoted_factor_shapes(Updater, oracle, cfg, F, track):
    """Mode A's default — the diagonally pivoted Cholesky factor of the whitened stack's Gram matrix (k_gram_pchol), un-whitened —
    on short, ragged and tall stacks, mono / stereo / four cameras: the stack of an MSCKF update is rank deficient (gauge directions;
    a 3-feature update leaves most columns unobserved), the factor stops at the numerical rank and its remaining rows are zero.
    (H, r) through the stock EKFUpdate (the oracle's restatement) reproduces the oracle's posterior at the update's own tolerances."""
    prob = synth.make_problem(cfg, F=F, track=track)
    opts = capi.default_options(chi2_multipler=1.0)
    v = capi.Views(prob)
    tri = oracle.triangulate(opts, v)
    ref = oracle.msckf_update(opts, v, want_compressed=True, given=tri)
    up = Updater(opts)
    up.set_problem(prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    cmp = up.compress()
    assert up.lib.ovgpu_last_update_route(up._ctx) == capi.COMPRESS_PCHOLQR  # the default of mode A
    assert np.array_equal(cmp["feat_status"], ref["feat_status"])
    H, r = cmp["H"], cmp["r"]
    rank = cmp["rows"]
    assert H.shape == (rank, ref["D"]) and 0 < rank <= ref["D"] and np.isfinite(H).all() and np.isfinite(r).all()
    assert (np.abs(H).sum(axis=1) > 0).all()  # the rows beyond the numerical rank stayed on the device
    G, g = ref["H_comp"].T @ ref["H_comp"], ref["H_comp"].T @ ref["r_comp"]
    st, P1, dx1 = oracle.ekf_update(prob.P, H, r, cmp["col_cov_id"], 1.0)
    assert st == 0
    eP, edx = _rel(P1, ref["P"]), _rel(dx1, ref["dx"])
    print(f"mode A, pivoted, cfg {cfg} F {F} {track}: rank {rank} of {ref['D']} ({ref['rows_comp']} rows), |H^T H - G| / |G| = "
          f"{np.linalg.norm(H.T @ H - G) / np.linalg.norm(G):.1e}, |H^T r - g| / |g| = {np.linalg.norm(H.T @ r - g) / np.linalg.norm(g):.1e}, P {eP:.1e}, dx {edx:.1e}")
    assert eP < TOL_P and edx < TOL_DX
    # the mode B update of the same context is the Gram route's, untouched by the option
    out = up.update()
    assert up.lib.ovgpu_last_update_route(up._ctx) == capi.COMPRESS_GRAM
    assert _rel(out["P"], ref["P"]) < TOL_P and _rel(out["dx"], ref["dx"]) < TOL_DX
    up.close()


@pytest.mark.parametrize("cfg,F,track,C", [(1, 12, "ragged", None), (2, 40, "full", None), (3, 600, "full", None), (4, 300, "full", None),
                                           (2, 60, "full", 12), (2, 60, "ragged", 17), (2, 80, "full", 21), (2, 80, "ragged", 26), (2, 100, "full", 29)])
def test_mode_a_blocked_kernels_equal_the_kernels_they_replace(Updater, cfg, F, track, C):
    """Round 6's blocked kernels of mode A — k_gram_pchol_blk (k_pchol.h: the pivoted factor with the matrix as MFMA tiles and the panel's
    rank-4 update in instalments) and k_unwhiten_blk (k_unwhiten.h: X = R L^-1 right-looking, the diagonal tiles' inverses from the prior's
    factorisation) — against the rank-one factor and the substitution kernel of rounds 3-5 (ovgpu_debug_option pchol_blocked / unwhiten_blocked
    = 0): the same pivots, the same rank, the compressed system equal at rounding (the products are summed in a different order).
    C: windows of 12 .. 29 clones, i.e. 100 .. 202 Jacobian columns = 7 .. 13 tile columns, most of them with a partial last tile."""
    prob = synth.make_problem(cfg, F=F, track=track, C=C)
    opts = capi.default_options(chi2_multipler=1.0)
    got = {}
    for name, flags in (("blocked", (1, 1)), ("factor rank-one", (0, 1)), ("substitution", (1, 0)), ("rounds 3-5", (0, 0))):
        up = Updater(opts)
        assert up.debug_option("pchol_blocked") == 1 and up.debug_option("unwhiten_blocked") == 1  # the defaults
        up.debug_option("pchol_blocked", flags[0])
        up.debug_option("unwhiten_blocked", flags[1])
        up.set_problem(prob)
        cmp = up.compress()
        assert up.lib.ovgpu_last_update_route(up._ctx) == capi.COMPRESS_PCHOLQR
        got[name] = cmp
        up.close()
    ref = got["rounds 3-5"]
    G0, g0 = ref["H"].T @ ref["H"], ref["H"].T @ ref["r"]
    for name in ("blocked", "factor rank-one", "substitution"):
        c = got[name]
        assert np.array_equal(c["feat_status"], ref["feat_status"])
        # (a pivot at the stop rule's threshold — rounding noise of the Gram sum — may fall on either side: a row of ~1e-8 of the others' size)
        assert abs(c["rows"] - ref["rows"]) <= 1
        G, g = c["H"].T @ c["H"], c["H"].T @ c["r"]
        eG, eg = np.linalg.norm(G - G0) / np.linalg.norm(G0), np.linalg.norm(g - g0) / np.linalg.norm(g0)
        same = c["rows"] == ref["rows"]
        eH = np.abs(c["H"] - ref["H"]).max() / np.abs(ref["H"]).max() if same else float("nan")
        print(f"cfg {cfg} F {F} C {C} D {c['H'].shape[1]}: {name} vs rounds 3-5: rank {c['rows']} / {ref['rows']}, |dH| / max|H| = {eH:.1e}, |d H^T H| = {eG:.1e}, |d H^T r| = {eg:.1e}")
        assert eG < 1e-12 and eg < 1e-11
        if same:
            assert eH < 1e-7


def test_compress_leaves_the_triangulation_readable(Updater, oracle):
    """Mode A of the shim: ONE triangulation — ovgpu_msckf_compress runs it, ovgpu_get_triangulation reads back what the Feature
    objects need (anchor, p_FinA, p_FinG); the values are those of a stand-alone ovgpu_triangulate on the same batch, bit for bit."""
    prob = synth.make_problem(2, F=120)
    opts = capi.default_options(chi2_multipler=1.0)
    up = Updater(opts)
    up.set_problem(prob)
    cmp = up.compress()
    got = up.get_triangulation()
    up2 = Updater(opts)
    up2.set_problem(prob)
    tri = up2.triangulate()
    ok = tri["status"] == 0
    assert ok.sum() > 100 and np.array_equal(np.isin(cmp["feat_status"], (0, 4)), ok)  # used or gated out = triangulated
    np.testing.assert_array_equal(got["anchor_meas"][ok], tri["anchor_meas"][ok])
    np.testing.assert_array_equal(got["p_FinA"][ok], tri["p_FinA"][ok])
    np.testing.assert_array_equal(got["p_FinG"][ok], tri["p_FinG"][ok])
    ref = oracle.triangulate(opts, capi.Views(prob))
    assert np.abs(got["p_FinG"][ok] - ref["p_FinG"][ok]).max() < TOL_TRI
    up.close(), up2.close()


def test_consecutive_updates_see_the_posterior(Updater, oracle):
    """VioManager calls the updaters back to back on the evolving state (VioManager.cpp:525-547)."""
    prob = synth.make_problem(2, F=60)
    second = synth.make_problem(2, F=40, shard=1)
    opts = capi.default_options(chi2_multipler=1.0)
    v1 = capi.Views(prob)
    t1 = oracle.triangulate(opts, v1)
    r1 = oracle.msckf_update(opts, v1, given=t1)
    import copy
    p2 = copy.copy(second)
    p2.P, p2.clone_q_p, p2.calib_q_p, p2.intrinsics = r1["P"], r1["clone_q_p"], r1["calib_q_p"], r1["intrinsics"]
    v2 = capi.Views(p2)
    t2 = oracle.triangulate(opts, v2)
    r2 = oracle.msckf_update(opts, v2, given=t2)
    up = Updater(opts)
    up.set_problem(prob)
    up.set_triangulation(t1["p_FinG"], t1["p_FinA"], t1["anchor_meas"], t1["status"])
    up.update()
    up.set_features(second)
    up.set_triangulation(t2["p_FinG"], t2["p_FinA"], t2["anchor_meas"], t2["status"])
    o2 = up.update()
    assert np.array_equal(o2["feat_status"], r2["feat_status"])
    assert _rel(o2["P"], r2["P"]) < 1e-8 and _rel(o2["dx"], r2["dx"]) < 1e-6
    up.close()


def test_reset_state_is_idempotent(Updater):
    prob = synth.make_problem(2, F=80)
    up = Updater(capi.default_options(chi2_multipler=1.0))
    up.set_problem(prob)
    a = up.update()
    up.reset_state()
    b = up.update()
    np.testing.assert_array_equal(a["P"], b["P"])  # same kernels, same inputs, no atomics: bitwise repeatable
    np.testing.assert_array_equal(a["dx"], b["dx"])
    up.close()


# --------------------------------------------------------------------------- feature sharding on one GPU
def test_sharded_update_equals_unsharded(Updater, oracle):
    """Two contexts each compress half of the features; QR of the two stacked triangles + one EKF update must
    equal the single-context update (QR([R1; R2]) has the same R^T R as QR of the full stack)."""
    import torch
    from open_vins_amd import parallel
    prob = synth.make_problem(2, F=120)
    opts = capi.default_options(chi2_multipler=1.0)
    v = capi.Views(prob)
    tri = oracle.triangulate(opts, v)
    full = Updater(opts)
    full.set_problem(prob)
    full.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    ref = full.update()
    G = 2
    tris = []
    ups = []
    for rank in range(G):
        ids = parallel.shard_features(prob.meas_offsets, rank, G)
        sub = prob.subset(ids)
        u = Updater(opts)
        u.set_problem(sub)
        off = prob.meas_offsets
        anchor_local = tri["anchor_meas"][ids] - off[ids] + sub.meas_offsets[:-1]
        u.set_triangulation(tri["p_FinG"][ids], tri["p_FinA"][ids], anchor_local, tri["status"][ids])
        t = torch.empty(u.triangle_len(), dtype=torch.float64, device="cuda")
        u.local(t.data_ptr(), want_outputs=False)
        tris.append(t)
        ups.append(u)
    gathered = torch.cat(tris)
    torch.cuda.synchronize()
    out = ups[0].merge_update(gathered.data_ptr(), G)
    assert _rel(out["P"], ref["P"]) < 1e-10
    assert _rel(out["dx"], ref["dx"]) < 1e-9
    for u in ups:
        u.close()
    full.close()


def test_sharded_gram_exchange_equals_unsharded(Updater, oracle):
    """The Gram form of the exchange (parallel.py): the shards' Gram matrices ADD UP to the Gram matrix of the full stack, so
    two contexts' buffers summed (what the all-reduce does) and factored once give the single-context update; the trailing
    element carries the accepted-row count."""
    import torch
    from open_vins_amd import parallel
    prob = synth.make_problem(2, F=120)
    opts = capi.default_options(chi2_multipler=1.0)
    v = capi.Views(prob)
    tri = oracle.triangulate(opts, v)
    ref = oracle.msckf_update(opts, v, given=tri)
    full = Updater(opts)
    full.set_problem(prob)
    full.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    one = full.update()
    G = 2
    total, ups = None, []
    for rank in range(G):
        ids = parallel.shard_features(prob.meas_offsets, rank, G)
        sub = prob.subset(ids)
        u = Updater(opts)
        u.set_problem(sub)
        anchor_local = tri["anchor_meas"][ids] - prob.meas_offsets[ids] + sub.meas_offsets[:-1]
        u.set_triangulation(tri["p_FinG"][ids], tri["p_FinA"][ids], anchor_local, tri["status"][ids])
        n = u.gram_len()
        assert n == (16 * 14) ** 2 + 1
        t = torch.empty(n, dtype=torch.float64, device="cuda")
        u.local_gram(t.data_ptr(), want_outputs=False)
        total = t if total is None else total + t
        ups.append(u)
    torch.cuda.synchronize()
    assert int(total[-1].item()) == ref["stats"]["n_rows"]
    Gm = total[:-1].reshape(224, 224).cpu().numpy()
    assert np.array_equal(Gm, Gm.T) and not Gm[209:, :].any()
    out = ups[1].gram_update(total.data_ptr())
    assert _rel(out["P"], one["P"]) < 1e-10 and _rel(out["dx"], one["dx"]) < 1e-9
    assert _rel(out["P"], ref["P"]) < 1e-9 and _rel(out["dx"], ref["dx"]) < 1e-7
    # and through the protocol driver (world size 1: no collective, same code path)
    class _Dist:
        @staticmethod
        def get_world_size():
            return 1
    full.reset_state()
    drv = parallel.distributed_update(parallel.GpuShardBackend(full), _Dist, torch.device("cuda"))
    assert _rel(drv["P"], one["P"]) < 1e-12 and _rel(drv["dx"], one["dx"]) < 1e-10
    for u in ups:
        u.close()
    full.close()


# --------------------------------------------------------------------------- BASELINE.json full sizes: properties
def test_cfg2_full_size_against_oracle(Updater, oracle):
    """configs[1]: 30 clones, stereo, 800 features — the bench workload, compared with the oracle directly."""
    prob = synth.make_problem(2)
    assert prob.F == 800 and prob.N == 224
    _check_given(Updater, oracle, prob, capi.default_options(chi2_multipler=1.0), tol_dx=1e-7, tol_p=1e-8)


def test_cfg3_full_size_properties(Updater):
    """configs[2] (2000 features): size-independent properties — symmetric PSD posterior, shrinking marginals,
    information-form identity dx = P' H^T r / sigma^2 evaluated through the compressed system."""
    prob = synth.make_problem(3)
    assert prob.F == 2000
    opts = capi.default_options(chi2_multipler=1.0)
    up = Updater(opts)
    up.set_problem(prob)
    cmp = up.compress()
    up.reset_state()
    out = up.update()
    P1 = out["P"]
    assert np.array_equal(P1, P1.T)
    assert np.linalg.eigvalsh(P1).min() > -1e-12
    assert np.all(np.diag(P1) <= np.diag(prob.P) + 1e-15)
    H = np.zeros((cmp["rows"], prob.N))
    H[:, cmp["col_cov_id"]] = cmp["H"]
    Pinf = np.linalg.inv(np.linalg.inv(prob.P) + H.T @ H)
    assert _rel(P1, Pinf) < 1e-7
    assert _rel(out["dx"], Pinf @ H.T @ cmp["r"]) < 1e-6
    up.close()


# --------------------------------------------------------------------------- measurement compression variants
def _opts_with(opts, **fields):
    """A copy of the options with library switches set (include/ovgpu.h: they are fields of ovgpu_options, not environment)."""
    import ctypes
    o = capi.Options()
    ctypes.memmove(ctypes.byref(o), ctypes.byref(opts), ctypes.sizeof(o))
    for k, v in fields.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


def _compress_with(Updater, prob, opts, tri, **fields):
    up = Updater(_opts_with(opts, **fields))
    up.set_problem(prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    cmp = up.compress()
    up.close()
    return cmp


def test_retired_compress_route_is_refused(Updater):
    """ABI 8: compress_route = 2 (the unpivoted Cholesky factor of the Gram matrix, rounds 3-5's documented negative result) no longer exists."""
    with pytest.raises(capi.OvgpuError) as ei:
        Updater(capi.default_options(compress_route=2))
    assert ei.value.code == capi.ERR_INVALID


def _update_with(Updater, prob, opts, tri, **fields):
    up = Updater(_opts_with(opts, **fields))
    up.set_problem(prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    out = up.update()
    up.close()
    return out


@pytest.mark.parametrize("kw", [dict(F=300), dict(cfg=4, F=120), dict(F=200, K=1, C=12), dict(F=3), dict(F=150, track="ragged"),
                                dict(F=40, C=6, K=1)])
def test_gram_route_gives_the_householder_posterior(Updater, oracle, kw):
    """The on-device update accumulates the Gram matrix [H r]^T [H r] on the matrix cores (k_gram.h) and updates in coordinates
    whitened by the prior (k_ekf.h) unless options.compress_route = OVGPU_COMPRESS_TSQR selects the Householder TSQR + the reference-shaped update:
    same dx and P, far inside the parity tolerance against the oracle (which compresses with Givens rotations like the
    reference).  LD = 209 / 237 / 87 / 51 columns: 14, 15, 6 and 4 column tiles; F = 3 has hardly more rows than columns.
    (tests/test_closed_loop.py runs the default through 52 frames.)"""
    kw = dict(kw)
    prob = synth.make_problem(kw.pop("cfg", 2), **kw)
    opts = capi.default_options(chi2_multipler=1.0)
    v = capi.Views(prob)
    tri = oracle.triangulate(opts, v)
    ref = oracle.msckf_update(opts, v, given=tri)
    a = _update_with(Updater, prob, opts, tri, compress_route=capi.COMPRESS_TSQR)
    b = _update_with(Updater, prob, opts, tri, compress_route=capi.COMPRESS_GRAM)
    b2 = _update_with(Updater, prob, opts, tri, compress_route=capi.COMPRESS_GRAM)
    for o in (a, b):
        assert np.array_equal(o["feat_status"], ref["feat_status"]) and o["stats"]["status"] == 0 and np.array_equal(o["P"], o["P"].T)
    assert np.array_equal(b["dx"], b2["dx"]) and np.array_equal(b["P"], b2["P"])  # ordered sums: reproducible bit for bit
    assert _rel(b["dx"], a["dx"]) < 1e-9 and _rel(b["P"], a["P"]) < 1e-10
    assert _rel(b["dx"], ref["dx"]) < 1e-8 and _rel(b["P"], ref["P"]) < 1e-9


def test_semi_definite_prior_takes_the_householder_route(Updater, oracle):
    """The Gram-form update factors the PRIOR block of the involved variables.  A valid covariance may be singular there (here:
    the newest clone an exact copy of the one before, as right after StateHelper::clone of a pose that already is a clone): the
    device notices (pivot below 1e-12 of the diagonal), skips everything behind that factorisation — nothing modified — and the
    call repeats through the Householder route, whose S = R P R^T + sigma^2 I is positive definite for any covariance."""
    prob = synth.make_problem(2, F=120)
    A = np.eye(prob.N)
    i, j = int(prob.clone_cov_id[28]), int(prob.clone_cov_id[29])      # the two newest of the 30 clones
    A[j:j + 6, :] = 0.0
    A[j:j + 6, i:i + 6] = np.eye(6)
    prob.P = A @ prob.P @ A.T            # positive semi-definite, rank N - 6
    opts = capi.default_options(chi2_multipler=1.0)
    v = capi.Views(prob)
    tri = oracle.triangulate(opts, v)
    ref = oracle.msckf_update(opts, v, given=tri)
    assert ref["stats"]["status"] == 0 and ref["stats"]["n_used"] > 30
    up = Updater(opts)
    up.set_problem(prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    out = up.update()
    assert out["stats"]["status"] == 0 and np.array_equal(out["feat_status"], ref["feat_status"])
    assert _rel(out["dx"], ref["dx"]) < 1e-7 and _rel(out["P"], ref["P"]) < 1e-8
    assert np.abs(out["clone_q_p"] - ref["clone_q_p"]).max() < 1e-9
    # mode A on the same singular prior: the whitened Gram matrix has nothing to stand on (its whitening IS the prior's factor), the
    # call repeats through the Householder TSQR of the raw rows and says so
    up.set_problem(prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    cmp = up.compress()
    assert up.lib.ovgpu_last_update_route(up._ctx) == capi.COMPRESS_TSQR and cmp["rows"] == cmp["D"]
    assert np.abs(np.tril(cmp["H"], -1)).max() == 0.0
    st, P1, dx1 = oracle.ekf_update(prob.P, cmp["H"], cmp["r"], cmp["col_cov_id"], 1.0)
    assert st == 0 and _rel(dx1, ref["dx"]) < 1e-7 and _rel(P1, ref["P"]) < 1e-8
    np.testing.assert_array_equal(up.get_state()["P"], prob.P)
    up.close()


@pytest.mark.parametrize("kw", [dict(F=300), dict(cfg=4, F=120), dict(F=200, K=1, C=12)])
def test_compression_is_independent_of_the_tree_shape(Updater, oracle, kw):
    """QR([R_1; R_2; ...]) = QR of the full stack: any number of leaves, and the pipelined single-launch merge
    tree vs one launch per level, with the tree started next to the leaves (second stream) or after them, give the same R^T R / R^T c (upper triangular, D x D)."""
    kw = dict(kw)
    prob = synth.make_problem(kw.pop("cfg", 2), **kw)
    opts = capi.default_options(chi2_multipler=1.0)
    tri = oracle.triangulate(opts, capi.Views(prob))
    opts.compress_route = capi.COMPRESS_TSQR
    base = _compress_with(Updater, prob, opts, tri, tsqr_workers=1)
    G0, g0 = base["H"].T @ base["H"], base["H"].T @ base["r"]
    for env in (dict(tsqr_workers=2), dict(tsqr_workers=5), dict(tsqr_workers=64), dict(tsqr_workers=64, tsqr_no_pipeline=1),
                dict(tsqr_workers=64, tsqr_overlap=2), dict(tsqr_workers=256), dict(tsqr_workers=256, tsqr_overlap=1)):
        c = _compress_with(Updater, prob, opts, tri, **env)
        assert c["rows"] == base["rows"] and c["D"] == base["D"]
        assert np.abs(np.tril(c["H"], -1)).max() == 0.0
        assert np.linalg.norm(c["H"].T @ c["H"] - G0) / np.linalg.norm(G0) < 1e-12, env
        assert np.linalg.norm(c["H"].T @ c["r"] - g0) / np.linalg.norm(g0) < 1e-11, env


def test_cfg4_full_size_properties(Updater):
    """configs[3] shape on one GPU (30 clones, 4 cameras, D = 236: the 15-tile path of the TSQR, N = 252): a 1250-feature
    shard — what one of 8 ranks holds — through size-independent properties of the posterior."""
    prob = synth.make_problem(4, F=1250)
    assert prob.K == 4 and prob.N == 252
    opts = capi.default_options(chi2_multipler=1.0)
    up = Updater(opts)
    up.set_problem(prob)
    cmp = up.compress()
    assert cmp["D"] == 236 and up.lib.ovgpu_last_update_route(up._ctx) == capi.COMPRESS_PCHOLQR and 200 < cmp["rows"] <= 236
    up.reset_state()
    out = up.update()
    P1 = out["P"]
    assert np.array_equal(P1, P1.T)
    assert np.linalg.eigvalsh(P1).min() > -1e-12
    H = np.zeros((cmp["rows"], prob.N))
    H[:, cmp["col_cov_id"]] = cmp["H"]
    # the posterior of the compressed system in the Kalman form: the information matrix P^-1 + H^T H of this shape has a condition
    # number of ~1e10, and inverting it on the host alone puts 5e-7 .. 7e-7 of error into the reference dx (varying with the BLAS
    # thread count) against the 1e-6 bound; through S = H P H^T + I (~5e5) the host's share is ~1e-12
    P0 = prob.P
    PHt = P0 @ H.T
    S = H @ PHt + np.eye(cmp["rows"])
    Pinf = P0 - PHt @ np.linalg.solve(S, PHt.T)
    assert _rel(P1, Pinf) < 1e-7
    assert _rel(out["dx"], PHt @ np.linalg.solve(S, cmp["r"])) < 1e-6
    up.close()


# --------------------------------------------------------------------------- UpdaterSLAM::update
@pytest.mark.parametrize("kw", [dict(L=12), dict(L=3, K=1, C=12), dict(L=24), dict(L=12, track="ragged")])
def test_slam_update_parity(Updater, oracle, kw):
    """landmarks that live in the state (GLOBAL_3D) — Jacobian with the landmark's columns, gate on all
    2m rows, stacking, EKF update.  The GPU compresses the stack before the update, the reference does not: same
    posterior.  L = 12 gives D = 244 (16 column tiles), L = 24 gives D = 280 (generic TSQR path; the oracle, like the reference, does not
    compress the SLAM stack: its S is rows x rows, which is what makes this case slow on the CPU)."""
    kw = dict(kw)
    prob = synth.make_slam_problem(2, **kw)
    opts = capi.default_options(chi2_multipler=1.0)
    ref = oracle.slam_update(opts, capi.Views(prob))
    up = Updater(opts)
    up.set_slam_problem(prob)
    out = up.slam_update()
    assert np.array_equal(out["feat_status"], ref["feat_status"])
    gate = np.isfinite(ref["chi2"])
    np.testing.assert_allclose(out["chi2"][gate], ref["chi2"][gate], rtol=TOL_CHI2)
    np.testing.assert_allclose(out["chi2_thresh"][gate], ref["chi2_thresh"][gate], rtol=1e-12)
    assert out["stats"]["n_used"] == ref["stats"]["n_used"] and out["stats"]["n_rows"] == ref["stats"]["n_rows"]
    assert _rel(out["dx"], ref["dx"]) < 1e-7
    assert _rel(out["P"], ref["P"]) < 1e-8 and np.array_equal(out["P"], out["P"].T)
    assert np.abs(out["landmarks"] - ref["landmarks"]).max() < 1e-9
    up.close()


def test_slam_then_msckf_on_one_context(Updater, oracle):
    """ovgpu_set_state clears the landmarks: the same context goes back to the MSCKF rules afterwards."""
    opts = capi.default_options(chi2_multipler=1.0)
    up = Updater(opts)
    up.set_slam_problem(synth.make_slam_problem(2, L=6))
    up.slam_update()
    prob = synth.make_problem(2, F=60)
    ref = oracle.msckf_update(opts, capi.Views(prob))
    up.set_problem(prob)
    out = up.update()
    assert np.array_equal(out["feat_status"], ref["feat_status"])
    assert _rel(out["dx"], ref["dx"]) < 1e-7
    up.close()


def test_slam_mode_a_compressed_system(Updater, oracle):
    """ovgpu_slam_compress: R^T R / R^T c of the compressed stack equal those of the reference's uncompressed SLAM stack,
    landmark columns included, and feeding it to the oracle's EKFUpdate reproduces the oracle's posterior."""
    prob = synth.make_slam_problem(2, L=10)
    opts = capi.default_options(chi2_multipler=1.0)
    ref = oracle.slam_update(opts, capi.Views(prob), want_stack=True)
    up = Updater(opts)
    up.set_slam_problem(prob)
    cmp = up.slam_compress()
    assert cmp["D"] == ref["D"] and np.array_equal(cmp["col_cov_id"], ref["col_cov_id"])
    assert np.array_equal(cmp["feat_status"], ref["feat_status"])
    H, r = cmp["H"], cmp["r"]
    assert np.abs(np.tril(H, -1)).max() == 0.0
    G, g = ref["H"].T @ ref["H"], ref["H"].T @ ref["r"]
    assert np.linalg.norm(H.T @ H - G) / np.linalg.norm(G) < 1e-11
    assert np.linalg.norm(H.T @ r - g) / np.linalg.norm(g) < 1e-10
    st, P1, dx1 = oracle.ekf_update(prob.P, H, r, cmp["col_cov_id"], 1.0)
    assert st == 0 and _rel(P1, ref["P"]) < 1e-8 and _rel(dx1, ref["dx"]) < 1e-7
    up.close()


# --------------------------------------------------------------------------- the helpers as standalone calls
@pytest.mark.parametrize("shape", [(500, 60), (3000, 208), (40, 90), (700, 300)])
def test_standalone_measurement_compress(Updater, oracle, shape):
    """UpdaterHelper::measurement_compress_inplace on a caller-supplied dense system (the ZUPT updater's use): upper
    triangular, same H^T H / H^T r as the oracle's Givens sweep; rows <= cols comes back unchanged (UpdaterHelper.cpp:459)."""
    rows, cols = shape
    rng = np.random.default_rng(rows + cols)
    H = rng.normal(size=(rows, cols)) * rng.uniform(0.1, 30.0, cols)
    r = rng.normal(size=rows)
    up = Updater(capi.default_options())
    Hc, rc = up.measurement_compress(H, r)
    up.close()
    Ho, ro = oracle.measurement_compress(H.copy(), r.copy())
    assert Hc.shape == Ho.shape
    if rows <= cols:
        np.testing.assert_array_equal(Hc, H)
        np.testing.assert_array_equal(rc, r)
        return
    assert np.abs(np.tril(Hc, -1)).max() == 0.0
    G = Ho.T @ Ho
    assert np.linalg.norm(Hc.T @ Hc - G) / np.linalg.norm(G) < 1e-12
    assert np.linalg.norm(Hc.T @ rc - Ho.T @ ro) / np.linalg.norm(Ho.T @ ro) < 1e-11
    # ... and entry by entry on the column-normalised Gram matrix, against LAPACK's own error (tests/tsqr_shapes.py): the norms above are
    # dominated by the largest columns
    Gl, n = ts.gram_ref(H, r)
    e_ref = ts.metric(*ts.lapack_compress(H, r), Gl, n)
    assert ts.metric(Hc, rc, Gl, n) <= ts.bound(e_ref)


def test_standalone_ekf_update(Updater, oracle):
    """StateHelper::EKFUpdate on the resident state with an arbitrary dense system — here one that touches the IMU block
    and the time offset, which the feature Jacobians never do — against the oracle's EKFUpdate."""
    prob = synth.make_problem(2, F=5)
    rng = np.random.default_rng(3)
    cols = np.concatenate([np.arange(0, 16), prob.clone_cov_id[-1] + np.arange(6)]).astype(np.int32)  # IMU 15, dt, newest clone
    H = rng.normal(size=(9, cols.size))
    r = rng.normal(size=9) * 0.01
    st, P1, dx1 = oracle.ekf_update(prob.P, H, r, cols, 1e-4)
    assert st == 0
    up = Updater(capi.default_options())
    up.set_problem(prob)
    dx, P = up.ekf_update(H, r, cols, 1e-4)
    assert _rel(dx, dx1) < 1e-9 and _rel(P, P1) < 1e-10 and np.array_equal(P, P.T)
    # the resident tables took the correction: the newest clone moved by its part of dx
    got = up.get_state(P=False)["clone_q_p"][-1, 4:]
    np.testing.assert_allclose(got, prob.clone_q_p[-1, 4:] + dx1[prob.clone_cov_id[-1] + 3: prob.clone_cov_id[-1] + 6], atol=1e-12)
    up.close()


def test_triangulation_from_explicit_camera_poses(Updater, oracle):
    """ovgpu_set_camera_poses: the clonesCAM argument of FeatureInitializer::single_* supplied directly gives the same
    triangulation as the state snapshot; the update entry points refuse to run without a covariance."""
    prob = synth.make_problem(2, F=150)
    opts = capi.default_options()
    ref = oracle.triangulate(opts, capi.Views(prob))
    up = Updater(opts)
    up.set_camera_poses_from(prob)
    out = up.triangulate()
    assert np.array_equal(out["status"], ref["status"]) and np.array_equal(out["anchor_meas"], ref["anchor_meas"])
    ok = ref["status"] == capi.FEAT_USED
    _check_tri(out, ref, ok)
    assert up.lib.ovgpu_msckf_update_async(up._ctx) == capi.ERR_NO_STATE
    up.close()


# --------------------------------------------------------------------------- SLAM landmarks in other representations, delayed initialisation
@pytest.mark.parametrize("rep", [capi.REP_GLOBAL_FULL_INVERSE_DEPTH, capi.REP_ANCHORED_3D, capi.REP_ANCHORED_FULL_INVERSE_DEPTH,
                                 capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE])
def test_slam_update_parity_representations(Updater, oracle, rep):
    """UpdaterSLAM::update with feat_rep_slam != GLOBAL_3D (EuRoC's default is ANCHORED_MSCKF_INVERSE_DEPTH): the landmark
    is stored in representation coordinates, its columns are dz/dp * dp/dlambda, anchored ones add the anchor clone /
    anchor extrinsics blocks."""
    prob = synth.make_slam_problem(2, L=10, lm_rep=rep)
    opts = capi.default_options(chi2_multipler=1.0)
    ref = oracle.slam_update(opts, capi.Views(prob))
    up = Updater(opts)
    up.set_slam_problem(prob)
    out = up.slam_update()
    assert np.array_equal(out["feat_status"], ref["feat_status"]) and (ref["feat_status"] == capi.FEAT_USED).sum() >= 6
    gate = np.isfinite(ref["chi2"])
    np.testing.assert_allclose(out["chi2"][gate], ref["chi2"][gate], rtol=TOL_CHI2)
    assert _rel(out["dx"], ref["dx"]) < 1e-7
    assert _rel(out["P"], ref["P"]) < 1e-8
    np.testing.assert_allclose(out["landmarks"], ref["landmarks"], rtol=1e-9, atol=1e-11)
    up.close()


def _check_delayed_init(out, ref, post, prob=None, tri=None):
    assert np.array_equal(out["feat_status"], ref["feat_status"])
    gate = np.isfinite(ref["chi2"])
    np.testing.assert_allclose(out["chi2"][gate], ref["chi2"][gate], rtol=1e-7)
    np.testing.assert_allclose(out["chi2_thresh"][gate], ref["chi2_thresh"][gate], rtol=1e-12)
    assert out["N"] == ref["N"] and np.array_equal(out["lm_cov_id"], ref["lm_cov_id"])
    acc = ref["lm_cov_id"] >= 0
    # anchored landmarks report their anchor; every other feature the anchor of its triangulation (FeatureInitializer.cpp:36-46
    # writes it into the Feature for every representation; UpdaterSLAM.cpp:214 takes Landmark::_unique_camera_id from it)
    anchored = ref["anchor_cam"] >= 0
    assert np.array_equal(out["anchor_cam"][anchored], ref["anchor_cam"][anchored]) and np.array_equal(out["anchor_clone"][anchored], ref["anchor_clone"][anchored])
    if prob is not None and tri is not None:
        am = tri["anchor_meas"]
        want_cam = np.where(am >= 0, prob.cam_idx[np.maximum(am, 0)], -1)
        want_clone = np.where(am >= 0, prob.clone_idx[np.maximum(am, 0)], -1)
        assert np.array_equal(out["anchor_cam"][~anchored], want_cam[~anchored]) and np.array_equal(out["anchor_clone"][~anchored], want_clone[~anchored])
    np.testing.assert_allclose(out["lm_value"][acc], ref["lm_value"][acc], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(out["lm_fej"][acc], ref["lm_fej"][acc], rtol=1e-12, atol=1e-14)
    assert np.isnan(out["lm_value"][~acc]).all()
    assert _rel(out["dx_seq"], ref["dx_seq"]) < 1e-6 and not out["dx_seq"][~acc].any()
    assert _rel(out["P"], ref["P"]) < 1e-7
    np.testing.assert_allclose(out["P"], out["P"].T, rtol=0, atol=1e-13 * np.abs(out["P"]).max())
    for k in ("clone_q_p", "calib_q_p", "intrinsics"):
        assert np.abs(post[k] - ref[k]).max() < 1e-9


@pytest.mark.parametrize("rep", [capi.REP_GLOBAL_3D, capi.REP_GLOBAL_FULL_INVERSE_DEPTH, capi.REP_ANCHORED_3D, capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH,
                                 capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE])
def test_delayed_init_parity(Updater, oracle, rep):
    """UpdaterSLAM::delayed_init: a chain of StateHelper::initialize calls (Givens split in the oracle, Householder on the
    GPU), each on the state the previous one left, against the oracle run with the same triangulation."""
    prob = synth.make_problem(2, F=16, outlier_frac=0.2)
    opts = capi.default_options(chi2_multipler=1.0)
    v = capi.Views(prob)
    tri = oracle.triangulate(opts, v)
    ref = oracle.slam_delayed_init(opts, v, feat_rep=rep, tri=tri)
    acc = ref["lm_cov_id"] >= 0
    assert ref["rc"] == 0 and 4 <= acc.sum() < 16
    up = Updater(opts)
    up.set_problem(prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    out = up.delayed_init(rep)
    post = up.get_state(P=True)
    _check_delayed_init(out, ref, post, prob, tri)
    assert post["P"].shape == out["P"].shape and np.array_equal(post["P"], out["P"])
    lm = up.get_landmarks()
    assert np.array_equal(lm["cov_id"], ref["lm_cov_id"][acc]) and np.array_equal(lm["value"], out["lm_value"][acc])
    up.close()


def test_triangulation_stays_readable_after_delayed_init(Updater, oracle):
    """include/ovgpu.h: ovgpu_get_triangulation reads what the triangulation stage of the LAST pipeline call left — ovgpu_slam_delayed_init included
    (the drop-in's UpdaterSLAM::delayed_init writes the Feature side effects from it).  The delayed initialisation rebuilds the column map, which
    marks the feature batch stale for further updates; until late round 4 that also made the triangulation unreadable (OVGPU_ERR_NO_STATE)."""
    prob = synth.make_problem(2, F=16, outlier_frac=0.2)
    opts = capi.default_options(chi2_multipler=1.0)
    tri = oracle.triangulate(opts, capi.Views(prob))
    up = Updater(opts)
    up.set_problem(prob)
    out = up.delayed_init(0)
    got = up.get_triangulation()
    ok = tri["status"] == capi.FEAT_USED
    assert ok.sum() >= 8 and (out["lm_cov_id"] >= 0).sum() >= 4
    assert np.abs(got["p_FinG"][ok] - tri["p_FinG"][ok]).max() < 1e-9 and np.array_equal(got["anchor_meas"][ok], tri["anchor_meas"][ok])
    with pytest.raises(capi.OvgpuError):  # ... while another update from the stale batch is still refused
        up.update()
    up.close()


def _aruco_options(F, seed):
    """Mixed per-feature options as UpdaterSLAM applies them: tag corners (landmark id < 4 * max_aruco) use sigma_pix_aruco
    and aruco_chi2_multipler, the others the SLAM values."""
    rng = np.random.default_rng(seed)
    tag = rng.random(F) < 0.4
    return np.where(tag, 2.5, 1.0), np.where(tag, 3.0, 1.0)


@pytest.mark.parametrize("rep", [capi.REP_GLOBAL_3D, capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE])
def test_slam_update_per_feature_options(Updater, oracle, rep):
    """UpdaterSLAM.cpp:392-409, :444: ArUco landmarks carry their own sigma_pix and chi2 multiplier; R_big is then diagonal but not
    isotropic.  The device scales each feature's rows by sigma / sigma_f so that ONE noise level describes the stack (which
    is what lets the stack be compressed), the oracle uses the reference's R_big."""
    prob = synth.make_slam_problem(2, L=12, lm_rep=rep)
    opts = capi.default_options(chi2_multipler=1.0)
    v = capi.Views(prob)
    sig, mult = _aruco_options(v.features.F, 3)
    ref = oracle.slam_update(opts, v, feat_sigma=sig, feat_chi2mult=mult)
    base = oracle.slam_update(opts, v)
    assert not np.array_equal(ref["feat_status"], base["feat_status"]) or _rel(ref["dx"], base["dx"]) > 1e-3  # the options matter
    up = Updater(opts)
    up.set_slam_problem(prob)
    up.set_feature_options(sig, mult)
    out = up.slam_update()
    assert np.array_equal(out["feat_status"], ref["feat_status"])
    gate = np.isfinite(ref["chi2"])
    np.testing.assert_allclose(out["chi2"][gate], ref["chi2"][gate], rtol=TOL_CHI2)
    np.testing.assert_allclose(out["chi2_thresh"][gate], ref["chi2_thresh"][gate], rtol=1e-12)
    assert _rel(out["dx"], ref["dx"]) < 1e-7 and _rel(out["P"], ref["P"]) < 1e-8
    assert np.abs(out["landmarks"] - ref["landmarks"]).max() < 1e-9
    # the options belong to the batch: the next upload runs with the context's values again
    up.set_slam_problem(prob)
    out2 = up.slam_update()
    assert np.array_equal(out2["feat_status"], base["feat_status"]) and _rel(out2["dx"], base["dx"]) < 1e-7
    up.close()


@pytest.mark.parametrize("rep", [capi.REP_GLOBAL_3D, capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE])
def test_delayed_init_per_feature_options(Updater, oracle, rep):
    """UpdaterSLAM.cpp:226-232: delayed initialisation of ArUco corners with their own noise and gate."""
    prob = synth.make_problem(2, F=16, outlier_frac=0.2)
    opts = capi.default_options(chi2_multipler=1.0)
    v = capi.Views(prob)
    tri = oracle.triangulate(opts, v)
    sig, mult = _aruco_options(16, 5)
    ref = oracle.slam_delayed_init(opts, v, feat_rep=rep, tri=tri, feat_sigma=sig, feat_chi2mult=mult)
    base = oracle.slam_delayed_init(opts, v, feat_rep=rep, tri=tri)
    assert ref["rc"] == 0 and (ref["lm_cov_id"] >= 0).sum() >= 4
    assert ref["N"] != base["N"] or _rel(ref["P"], base["P"]) > 1e-4
    up = Updater(opts)
    up.set_problem(prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    up.set_feature_options(sig, mult)
    out = up.delayed_init(rep)
    _check_delayed_init(out, ref, up.get_state(P=True))
    up.close()


def _split_tracks(prob, pred, feats=None):
    """Tracks restricted to the measurements whose clone index satisfies pred (and to the features `feats`)."""
    feats = range(len(prob.meas_offsets) - 1) if feats is None else feats
    keep, cnt = [], []
    for f in feats:
        ids = np.arange(prob.meas_offsets[f], prob.meas_offsets[f + 1])
        ids = ids[pred(prob.clone_idx[ids])]
        keep.append(ids)
        cnt.append(len(ids))
    keep = np.concatenate(keep)
    return dict(meas_offsets=np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32), uv=np.asarray(prob.uv).reshape(-1, 2)[keep].reshape(-1),
                uvn=np.asarray(prob.uvn).reshape(-1, 2)[keep].reshape(-1),
                clone_idx=prob.clone_idx[keep], cam_idx=prob.cam_idx[keep])


def test_delayed_init_end_to_end_then_slam_update(Updater, oracle):
    """Device triangulation -> delayed initialisation (older half of every track) on a state that already holds landmarks
    -> UpdaterSLAM::update of the landmarks that were just created with the newer half of the tracks, everything
    resident: the oracle is walked through the same steps."""
    prob = synth.make_slam_problem(2, L=3, seed=11)
    tracks = synth.make_problem(2, F=10, seed=11)
    old_value = prob.lm_value.copy()
    for k, a in _split_tracks(tracks, lambda c: c < 15).items():
        setattr(prob, k, a)
    opts = capi.default_options(chi2_multipler=1.0)
    v = capi.Views(prob)
    ref = oracle.slam_delayed_init(opts, v, feat_rep=0)
    acc = ref["lm_cov_id"] >= 0
    assert acc.sum() >= 5
    up = Updater(opts)
    up.set_slam_problem(prob)
    out = up.delayed_init(0)
    # device triangulation differs from the oracle's in the last digits (TOL_TRI), the chain amplifies that a little
    assert np.array_equal(out["feat_status"], ref["feat_status"]) and out["N"] == ref["N"]
    np.testing.assert_allclose(out["lm_value"][acc], ref["lm_value"][acc], rtol=1e-6, atol=1e-8)
    assert _rel(out["P"], ref["P"]) < 1e-6 and _rel(out["dx_seq"], ref["dx_seq"]) < 1e-5
    lm = up.get_landmarks()
    assert lm["value"].shape[0] == 3 + acc.sum()
    np.testing.assert_allclose(lm["value"][:3], ref["landmarks_existing"], rtol=1e-7, atol=1e-9)
    assert np.abs(lm["value"][:3] - old_value).max() > 0
    # ---- a SLAM update of the new landmarks with the newer measurements, on the resident state
    idx = np.flatnonzero(acc)
    newer = _split_tracks(tracks, lambda c: c >= 15, idx)
    sub = synth.make_problem(2, F=10, seed=11)
    p2 = synth.make_problem(2, F=10, seed=11)  # the oracle's side: the posterior of its own delayed init as the prior
    p2.N, p2.P = ref["N"], ref["P"]
    p2.clone_q_p, p2.calib_q_p, p2.intrinsics = ref["clone_q_p"], ref["calib_q_p"], ref["intrinsics"]
    for k, a in newer.items():
        setattr(p2, k, a)
        setattr(sub, k, a)
    p2.lm_value = np.concatenate([ref["landmarks_existing"], ref["lm_value"][acc]])
    p2.lm_fej = np.concatenate([prob.lm_fej, ref["lm_fej"][acc]])
    p2.lm_cov_id = np.concatenate([prob.lm_cov_id, ref["lm_cov_id"][acc]]).astype(np.int32)
    p2.lm_index = (3 + np.arange(len(idx))).astype(np.int32)
    ref2 = oracle.slam_update(opts, capi.Views(p2))
    assert (ref2["feat_status"] == capi.FEAT_USED).sum() >= 3
    up.set_features(sub)
    out2 = up.slam_update(lm_index=p2.lm_index)
    assert np.array_equal(out2["feat_status"], ref2["feat_status"])
    assert _rel(out2["dx"], ref2["dx"]) < 1e-5 and _rel(out2["P"], ref2["P"]) < 1e-6
    np.testing.assert_allclose(out2["landmarks"], ref2["landmarks"], rtol=1e-6, atol=1e-8)
    up.close()


def test_msckf_update_with_resident_landmarks(Updater, oracle):
    """UpdaterMSCKF::update on a state that holds SLAM landmarks (VioManager.cpp:525 runs it before the SLAM update): the
    landmark columns stay zero, the landmarks are corrected through their cross-covariance only."""
    prob = synth.make_slam_problem(2, L=5, seed=3)
    tracks = synth.make_problem(2, F=40, seed=4)
    for k in ("meas_offsets", "uv", "uvn", "clone_idx", "cam_idx", "p_FinG_true"):
        setattr(prob, k, getattr(tracks, k))
    opts = capi.default_options(chi2_multipler=1.0)
    plain = synth.make_problem(2, F=40, seed=4)
    plain.N, plain.P = prob.N, prob.P
    plain.clone_q_p, plain.clone_q_p_fej, plain.calib_q_p, plain.intrinsics = prob.clone_q_p, prob.clone_q_p_fej, prob.calib_q_p, prob.intrinsics
    ref = oracle.msckf_update(opts, capi.Views(plain))
    up = Updater(opts)
    up.set_slam_problem(prob)
    out = up.update()
    assert np.array_equal(out["feat_status"], ref["feat_status"])
    assert _rel(out["dx"], ref["dx"]) < 1e-7 and _rel(out["P"], ref["P"]) < 1e-8
    up.close()


# --------------------------------------------------------------------------- window bookkeeping on the resident covariance
def test_state_propagate_clone_marginalize_parity(Updater, oracle):
    """StateHelper::EKFPropagation, clone / augment_clone (with the time-offset Jacobian) and marginalize on the resident P,
    each step against the oracle applied to the covariance read back before it; then an MSCKF update on the new window."""
    prob = synth.make_problem(2, F=60)
    opts = capi.default_options(chi2_multipler=1.0)
    up = Updater(opts)
    up.set_problem(prob)
    rng = np.random.default_rng(3)
    N, C = prob.N, prob.C
    # ---- EKFPropagation of the IMU block (ids 0..14, State.cpp:33-41) with a dense Phi
    Phi = np.eye(15) + 0.05 * rng.normal(size=(15, 15))
    Q = np.diag(rng.uniform(1e-6, 1e-4, 15))
    Q[0, 3] = 1e-5  # only the upper triangle is read (StateHelper.cpp:87)
    rc, ref = oracle.propagate(prob.P, 0, np.arange(15), Phi, Q)
    up.state_propagate(0, np.arange(15), Phi, Q)
    P1 = up.get_state(P=True)["P"]
    assert rc == 0 and _rel(P1, ref) < 1e-14
    # ---- augment_clone: the IMU pose (ids 0..5) cloned to the end, time offset at id 15
    dnc = rng.normal(size=6)
    q_new = synth.boxplus_pose(prob.clone_q_p[-1], 0.01 * rng.normal(size=6))
    nid = up.state_augment_clone(0, q_new, dt_cov_id=15, dnc_dt=dnc)
    P2 = up.get_state(P=True)["P"]
    assert nid == N and up.N == N + 6 and up.Cn == C + 1
    assert _rel(P2, oracle.augment_clone(P1, 0, 6, dt_id=15, dnc_dt=dnc)) < 1e-15
    st = up.get_state(P=False)
    np.testing.assert_array_equal(st["clone_q_p"][-1], q_new)
    np.testing.assert_array_equal(st["clone_q_p"][:-1], prob.clone_q_p)
    # ---- marginalize the oldest clone: pure data movement, bit-exact
    old_id = int(prob.clone_cov_id[0])
    up.state_marginalize(old_id, 6)
    P3 = up.get_state(P=True)["P"]
    np.testing.assert_array_equal(P3, oracle.marginalize(P2, old_id, 6))
    st = up.get_state(P=False)
    assert up.N == N and up.Cn == C
    np.testing.assert_array_equal(st["clone_q_p"][:-1], prob.clone_q_p[1:])
    # ---- the update on the shifted window: tracks without the measurements of the dropped clone, indices moved down
    keep = prob.clone_idx > 0
    cnt = np.add.reduceat(keep.astype(np.int64), prob.meas_offsets[:-1])
    win = synth.make_problem(2, F=60)
    win.meas_offsets = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    win.uv, win.uvn = prob.uv.reshape(-1, 2)[keep].reshape(-1), prob.uvn.reshape(-1, 2)[keep].reshape(-1)
    win.clone_idx, win.cam_idx = (prob.clone_idx[keep] - 1).astype(np.int32), prob.cam_idx[keep]
    win.P = P3
    win.clone_q_p = st["clone_q_p"]
    win.clone_q_p_fej = np.vstack([prob.clone_q_p_fej[1:], q_new[None, :]])
    win.clone_cov_id = np.concatenate([prob.clone_cov_id[:-1], [N - 6]]).astype(np.int32)  # ids behind the dropped clone moved forward
    ref_u = oracle.msckf_update(opts, capi.Views(win))
    up.set_features(win)
    out = up.update()
    assert np.array_equal(out["feat_status"], ref_u["feat_status"]) and (ref_u["feat_status"] == capi.FEAT_USED).sum() > 30
    assert _rel(out["dx"], ref_u["dx"]) < 1e-7 and _rel(out["P"], ref_u["P"]) < 1e-8
    up.close()


def test_state_bookkeeping_rejects_bad_blocks(Updater):
    prob = synth.make_problem(2, F=4)
    up = Updater(capi.default_options())
    up.set_problem(prob)
    cid = int(prob.clone_cov_id[3])
    for args in ((cid + 1, 6), (cid, 5), (prob.N - 2, 6), (-1, 3)):
        with pytest.raises(RuntimeError):
            up.state_marginalize(*args)
    with pytest.raises(RuntimeError):
        up.state_propagate(prob.N - 3, np.arange(6), np.eye(6), np.eye(6))
    rc = up.lib.ovgpu_state_propagate(up._ctx, 0, 3, 3, np.arange(3, dtype=np.int32).ctypes.data_as(capi.c_int32_p),
                                      np.eye(3).ctypes.data_as(capi.c_double_p), (-1e6 * np.eye(3)).ctypes.data_as(capi.c_double_p))
    assert rc == capi.ERR_NEGATIVE_DIAGONAL
    up.close()


@pytest.mark.parametrize("rep", [capi.REP_ANCHORED_3D, capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE])
def test_change_anchors_parity_then_marginalize(Updater, oracle, rep):
    """UpdaterSLAM::change_anchors: the landmarks anchored in the oldest clone move to the newest one
    (value, first estimate, covariance through EKFPropagation) exactly as the oracle moves them one after the other; then
    the clone can be marginalised and a SLAM update on the shifted window matches the oracle's."""
    prob = synth.make_slam_problem(2, L=10, lm_rep=rep)
    moved = np.flatnonzero(prob.lm_anchor_clone == 0)   # most tracks start in the oldest clone
    other = np.flatnonzero(prob.lm_anchor_clone != 0)
    assert len(moved) >= 3 and len(other) >= 1
    opts = capi.default_options(chi2_multipler=1.0)
    up = Updater(opts)
    up.set_slam_problem(prob)
    assert up.change_anchors(0, prob.C - 1) == len(moved)
    ref = synth.make_slam_problem(2, L=10, lm_rep=rep)
    for l in moved:  # the oracle, landmark by landmark, each on the covariance the previous one left
        o = oracle.anchor_change(opts, capi.Views(ref), int(l), int(ref.lm_anchor_cam[l]), ref.C - 1)
        assert o["rc"] == 0
        ref.P, ref.lm_value[l], ref.lm_fej[l], ref.lm_anchor_clone[l] = o["P"], o["value"], o["fej"], ref.C - 1
    lm = up.get_landmarks()
    np.testing.assert_allclose(lm["value"], ref.lm_value, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(lm["fej"], ref.lm_fej, rtol=1e-12, atol=1e-13)
    np.testing.assert_array_equal(lm["anchor_clone"], ref.lm_anchor_clone)
    assert _rel(up.get_state(P=True)["P"], ref.P) < 1e-12
    k = int(other[0])
    up.change_anchor(k, int(ref.lm_anchor_cam[k]), 0)
    with pytest.raises(RuntimeError):  # a landmark anchored in a clone that goes away must move first; nothing is modified
        up.state_marginalize(int(prob.clone_cov_id[0]), 6)
    up.change_anchor(k, int(ref.lm_anchor_cam[k]), int(ref.lm_anchor_clone[k]))
    # ---- marginalise the oldest clone, update with the remaining measurements
    up.state_marginalize(int(prob.clone_cov_id[0]), 6)
    post = up.get_state(P=True)
    lm2 = up.get_landmarks()
    np.testing.assert_array_equal(lm2["anchor_clone"], ref.lm_anchor_clone - 1)
    keep = prob.clone_idx > 0
    cnt = np.add.reduceat(keep.astype(np.int64), prob.meas_offsets[:-1])
    win = synth.make_slam_problem(2, L=10, lm_rep=rep)
    win.C, win.N = prob.C - 1, prob.N - 6
    win.meas_offsets = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    win.uv, win.uvn = prob.uv.reshape(-1, 2)[keep].reshape(-1), prob.uvn.reshape(-1, 2)[keep].reshape(-1)
    win.clone_idx, win.cam_idx = (prob.clone_idx[keep] - 1).astype(np.int32), prob.cam_idx[keep]
    win.P, win.clone_q_p, win.clone_q_p_fej = post["P"], post["clone_q_p"], prob.clone_q_p_fej[1:]
    win.clone_cov_id = prob.clone_cov_id[:-1]
    win.lm_value, win.lm_fej, win.lm_cov_id = lm2["value"], lm2["fej"], lm2["cov_id"]
    win.lm_anchor_cam, win.lm_anchor_clone = lm2["anchor_cam"], lm2["anchor_clone"]
    ref_u = oracle.slam_update(opts, capi.Views(win))
    up.set_features(win)
    out = up.slam_update(lm_index=win.lm_index)
    assert np.array_equal(out["feat_status"], ref_u["feat_status"]) and (ref_u["feat_status"] == capi.FEAT_USED).sum() >= 5
    assert _rel(out["dx"], ref_u["dx"]) < 1e-7 and _rel(out["P"], ref_u["P"]) < 1e-8
    up.close()


def test_slam_edge_cases(Updater, oracle):
    """Empty and degenerate inputs of the SLAM entry points: no features, tracks too short to initialise, global
    landmarks in change_anchors (skipped, UpdaterSLAM.cpp:493-496), a bad landmark index, a marginalised landmark."""
    opts = capi.default_options(chi2_multipler=1.0)
    up = Updater(opts)
    # ---- delayed_init without features / with tracks of one measurement only
    prob = synth.make_problem(2, F=6)
    empty = synth.make_problem(2, F=6)
    empty.meas_offsets = np.zeros(1, np.int32)
    empty.uv = empty.uvn = np.zeros(0, np.float32)
    empty.clone_idx = empty.cam_idx = np.zeros(0, np.int32)
    up.set_problem(empty)
    out = up.delayed_init(0)
    assert out["N"] == prob.N and out["P"].shape == (prob.N, prob.N) and np.array_equal(out["P"], prob.P)
    short = synth.make_problem(2, F=6)
    first = short.meas_offsets[:-1]
    short.uv, short.uvn = short.uv.reshape(-1, 2)[first].reshape(-1), short.uvn.reshape(-1, 2)[first].reshape(-1)
    short.clone_idx, short.cam_idx = short.clone_idx[first], short.cam_idx[first]
    short.meas_offsets = np.arange(7, dtype=np.int32)
    up.set_problem(short)
    out = up.delayed_init(0)
    assert (out["feat_status"] == capi.FEAT_TOO_FEW_MEAS).all() and out["N"] == prob.N and (out["lm_cov_id"] == -1).all()
    assert np.array_equal(out["P"], prob.P) and not out["dx_seq"].any()
    # ---- global landmarks: change_anchors is a no-op, change_anchor an error; bad landmark index
    slam = synth.make_slam_problem(2, L=5)
    up.set_slam_problem(slam)
    assert up.change_anchors(0, slam.C - 1) == 0
    with pytest.raises(RuntimeError):
        up.change_anchor(0, 0, 1)
    with pytest.raises(RuntimeError):
        up.slam_update(lm_index=np.array([0, 1, 2, 3, 9], np.int32))
    # ---- StateHelper::marginalize_slam: landmark 1 leaves the state, the update of the others still matches the oracle
    up.state_marginalize(int(slam.lm_cov_id[1]), 3)
    lm = up.get_landmarks()
    assert lm["value"].shape[0] == 4 and np.array_equal(lm["cov_id"], np.r_[slam.lm_cov_id[0], slam.lm_cov_id[1:4]])
    keepf = np.array([0, 2, 3, 4])
    sub = _split_tracks(slam, lambda c: c >= 0, keepf)
    ref_p = synth.make_slam_problem(2, L=5)
    for k, a in sub.items():
        setattr(ref_p, k, a)
    idx = np.r_[0:slam.lm_cov_id[1], slam.lm_cov_id[1] + 3:slam.N]
    ref_p.N, ref_p.P = slam.N - 3, slam.P[np.ix_(idx, idx)]
    ref_p.lm_value, ref_p.lm_fej, ref_p.lm_cov_id = slam.lm_value[keepf], slam.lm_fej[keepf], lm["cov_id"]
    ref_p.lm_index = np.arange(4, dtype=np.int32)
    ref = oracle.slam_update(opts, capi.Views(ref_p))
    up.set_features(ref_p)
    out = up.slam_update(lm_index=ref_p.lm_index)
    assert np.array_equal(out["feat_status"], ref["feat_status"])
    assert _rel(out["dx"], ref["dx"]) < 1e-7 and _rel(out["P"], ref["P"]) < 1e-8
    up.close()


# --------------------------------------------------------------------------- randomised shapes
@pytest.mark.parametrize("seed", range(40))
def test_update_parity_random_shapes(Updater, oracle, seed):
    """A seeded sweep over window sizes, camera counts, batch sizes, track patterns, lens models, feature representations
    and state options: ragged and tiny inputs, D from 18 to 296, with and without outliers."""
    rng = np.random.default_rng(1000 + seed)
    C = int(rng.integers(3, 41))
    K = int(rng.integers(1, 5))
    F = int(rng.integers(1, 90))
    kw = dict(C=C, K=K, F=F, track=("full", "ragged")[int(rng.integers(2))], fisheye=bool(rng.integers(2)), seed=int(rng.integers(1 << 20)),
              outlier_frac=float(rng.choice([0.0, 0.0, 0.3])), min_obs=int(rng.integers(2, 6)))
    rep = int(rng.integers(0, 6))
    flags = dict(do_fej=int(rng.integers(2)), do_calib_camera_pose=int(rng.integers(2)), do_calib_camera_intrinsics=int(rng.integers(2)))
    prob = synth.make_problem(int(rng.choice([2, 4])), rep, **kw)
    opts = capi.default_options(chi2_multipler=float(rng.choice([1.0, 5.0])), feat_rep_msckf=rep, **flags)
    _check_given(Updater, oracle, prob, opts, require_gate=False)


@pytest.mark.parametrize("seed", range(12))
def test_slam_update_parity_random_shapes(Updater, oracle, seed):
    rng = np.random.default_rng(2000 + seed)
    kw = dict(C=int(rng.integers(6, 31)), K=int(rng.integers(1, 4)), track=("full", "ragged")[int(rng.integers(2))], fisheye=bool(rng.integers(2)),
              seed=int(rng.integers(1 << 20)))
    prob = synth.make_slam_problem(2, L=int(rng.integers(1, 13)), lm_rep=int(rng.integers(0, 6)), **kw)
    opts = capi.default_options(chi2_multipler=float(rng.choice([1.0, 5.0])), do_fej=int(rng.integers(2)),
                                do_calib_camera_pose=int(rng.integers(2)), do_calib_camera_intrinsics=int(rng.integers(2)))
    ref = oracle.slam_update(opts, capi.Views(prob))
    up = Updater(opts)
    up.set_slam_problem(prob)
    out = up.slam_update()
    up.close()
    assert np.array_equal(out["feat_status"], ref["feat_status"])  # at these seeds no landmark sits within round-off of its gate
    if ref["stats"]["n_used"] > 0:
        assert _rel(out["dx"], ref["dx"]) < 1e-6 and _rel(out["P"], ref["P"]) < 1e-7
        np.testing.assert_allclose(out["landmarks"], ref["landmarks"], rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("seed", range(12))
def test_delayed_init_parity_random_shapes(Updater, oracle, seed):
    rng = np.random.default_rng(3000 + seed)
    kw = dict(C=int(rng.integers(6, 31)), K=int(rng.integers(1, 4)), F=int(rng.integers(1, 21)), track=("full", "ragged")[int(rng.integers(2))],
              fisheye=bool(rng.integers(2)), seed=int(rng.integers(1 << 20)), outlier_frac=float(rng.choice([0.0, 0.3])))
    rep = int(rng.integers(0, 6))
    prob = synth.make_problem(2, **kw)
    opts = capi.default_options(chi2_multipler=float(rng.choice([1.0, 5.0])), do_fej=int(rng.integers(2)),
                                do_calib_camera_pose=int(rng.integers(2)), do_calib_camera_intrinsics=int(rng.integers(2)))
    v = capi.Views(prob)
    tri = oracle.triangulate(opts, v)
    ref = oracle.slam_delayed_init(opts, v, feat_rep=rep, tri=tri)
    up = Updater(opts)
    up.set_problem(prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    out = up.delayed_init(rep)
    post = up.get_state(P=True)
    up.close()
    assert ref["rc"] == 0
    gate = np.isfinite(ref["chi2"])
    if gate.any() and np.abs(ref["chi2"][gate] / ref["chi2_thresh"][gate] - 1.0).min() < 1e-8:
        pytest.skip("a feature sits on the gate threshold: the chains may legitimately diverge")
    _check_delayed_init(out, ref, post)


# --------------------------------------------------------------------------- FeatureDatabase on the device
def test_track_store_builds_the_same_batch_as_the_host(Updater, oracle):
    """Observations are appended frame by frame (FeatureDatabase::update_feature), tracks get lost, erased and re-opened;
    the batch assembled on the device equals — bit for bit — clean_old_measurements + the shim's flattening done in numpy,
    and an update on it equals the update on the uploaded batch."""
    prob = synth.make_problem(2, F=4)   # the state only (30 clones, 2 cameras)
    opts = capi.default_options(chi2_multipler=1.0)
    up = Updater(opts)
    up.set_problem(prob)
    up.tracks_create(512, 96)
    rng = np.random.default_rng(17)
    T = 40                                   # frames; the window is the last 30
    times = 100.0 + 0.05 * np.arange(T)
    db = {}                                  # host FeatureDatabase: id -> list of (cam, time, uv, uvn)
    alive = list(range(60))
    next_id = 60
    for t in range(T):
        for cam in range(prob.K):
            seen = [i for i in alive if rng.random() < 0.8]
            if not seen:
                continue
            uv = rng.uniform(0, 700, (len(seen), 2)).astype(np.float32)
            uvn = rng.uniform(-1, 1, (len(seen), 2)).astype(np.float32)
            up.tracks_append(times[t], seen, np.full(len(seen), cam), uv, uvn)
            for j, i in enumerate(seen):
                db.setdefault(i, []).append((cam, times[t], uv[j], uvn[j]))
        if t % 7 == 6:  # some tracks end, new ones start (ids are never reused by the front end, slots are)
            lost = list(rng.choice(alive, 8, replace=False))
            alive = [i for i in alive if i not in lost] + list(range(next_id, next_id + 8))
            next_id += 8
        if t == 20:     # FeatureDatabase::cleanup of used features
            gone = [i for i in db if i not in alive][:10]
            up.tracks_erase(gone)
            for i in gone:
                del db[i]
    assert up.tracks_count() == len(db)
    lost_ref = sorted(i for i, obs in db.items() if not max(o[1] for o in obs) >= times[T - 1])
    np.testing.assert_array_equal(up.tracks_not_containing_newer(times[T - 1]), lost_ref)
    # ---- the batch of an update: the lost tracks + an unknown id, window = last C frames
    clone_times = times[T - prob.C:]
    sel = lost_ref[:25] + [10 ** 9]
    up.tracks_to_features(sel, clone_times)
    got = up.get_features()
    offs, uv, uvn, ci, cam_idx = [0], [], [], [], []
    lut = {tt: k for k, tt in enumerate(clone_times)}
    mixed = 0
    for i in sel:
        obs = db.get(i, [])
        first_seen = list(dict.fromkeys(o[0] for o in obs))   # keys of Feature::timestamps in order of insertion
        mixed += first_seen == [1, 0]
        for cam in reversed(first_seen):    # libstdc++ iterates the unordered_map in reverse order of first insertion (k_tracks.h)
            for (c_, tt, a, b) in obs:
                if c_ == cam and tt in lut:
                    uv += list(a), ; uvn += list(b), ; ci.append(lut[tt]); cam_idx.append(cam)
        offs.append(len(ci))
    np.testing.assert_array_equal(got["meas_offsets"], offs)
    np.testing.assert_array_equal(got["clone_idx"], ci)
    np.testing.assert_array_equal(got["cam_idx"], cam_idx)
    np.testing.assert_array_equal(got["uv"], np.asarray(uv, np.float32).reshape(-1))
    np.testing.assert_array_equal(got["uvn"], np.asarray(uvn, np.float32).reshape(-1))
    assert got["meas_offsets"][-1] == got["meas_offsets"][-2]   # the unknown id is an empty track
    assert mixed > 0                                            # some tracks were first seen by camera 1: they iterate 0, 1
    # the explicit orders: by camera id, whatever the history
    for order, cams in ((capi.GROUPS_DESCENDING, range(prob.K - 1, -1, -1)), (capi.GROUPS_ASCENDING, range(prob.K))):
        up.tracks_group_order(order)
        up.tracks_to_features(sel, clone_times)
        got = up.get_features()
        want = [cam for i in sel for cam in cams for (c_, tt, a, b) in db.get(i, []) if c_ == cam and tt in lut]
        np.testing.assert_array_equal(got["cam_idx"], want)
    up.close()


def test_track_store_feeds_the_update(Updater, oracle):
    """Real tracks go through the store: the update on the device-assembled batch is bit-identical to the update on the
    uploaded one (same bytes in, same kernels).  (Round 6: an uploaded batch stacks UNPROJECTED rows in regions laid out from the host's
    measurement codes, k_gram_regions; a device-assembled batch has no host codes and keeps the projected stack — the bit comparison runs with
    ovgpu_debug_option raw_stack = 0, the default against it at rounding.)"""
    prob = synth.make_problem(2, F=50)
    # synth lists the camera groups in descending id (the reference's iteration order when camera 0 is inserted first) and the
    # front end below delivers camera 0 before camera 1 in every frame: the store must reproduce synth's batch as it is
    feat_of = np.repeat(np.arange(prob.F), np.diff(prob.meas_offsets))
    first_cam = prob.cam_idx[prob.meas_offsets[:-1]]
    assert (first_cam == prob.K - 1).sum() > 0.8 * prob.F
    opts = capi.default_options(chi2_multipler=1.0)
    up = Updater(opts)
    up.set_problem(prob)
    ref_default = up.update()
    assert up.debug_option("raw_stack", 0) == 1
    up.set_problem(prob)
    ref = up.update()
    assert _rel(ref["dx"], ref_default["dx"]) < 1e-10 and _rel(ref["P"], ref_default["P"]) < 1e-11
    np.testing.assert_array_equal(ref["feat_status"], ref_default["feat_status"])
    up.reset_state()
    up.tracks_create(128, 66)
    clone_times = 50.0 + 0.1 * np.arange(prob.C)
    uv2, uvn2 = prob.uv.reshape(-1, 2), prob.uvn.reshape(-1, 2)
    seen_cams = [sorted(set(prob.cam_idx[prob.meas_offsets[f]:prob.meas_offsets[f + 1]].tolist())) for f in range(prob.F)]
    for f in range(prob.F):  # the first frame of every track: one observation per camera, camera 0 first (the front ends' insertion order)
        up.tracks_append(1.0, np.full(len(seen_cams[f]), 1000 + f), seen_cams[f], np.zeros((len(seen_cams[f]), 2)), np.zeros((len(seen_cams[f]), 2)))
    for cl in range(prob.C):                       # frame by frame, camera by camera, as a front end would deliver them
        for cam in range(prob.K):
            idx = np.flatnonzero((prob.clone_idx == cl) & (prob.cam_idx == cam))
            if len(idx):
                up.tracks_append(clone_times[cl], 1000 + feat_of[idx], np.full(len(idx), cam), uv2[idx], uvn2[idx])
    up.tracks_to_features(1000 + np.arange(prob.F), clone_times)   # the frame at t = 1.0 is not a clone time: cleaned away
    got = up.get_features()
    np.testing.assert_array_equal(got["meas_offsets"], prob.meas_offsets)
    np.testing.assert_array_equal(got["clone_idx"], prob.clone_idx)
    np.testing.assert_array_equal(got["cam_idx"], prob.cam_idx)
    np.testing.assert_array_equal(got["uv"], prob.uv)
    out = up.update()
    for k in ("feat_status", "chi2", "dx", "P"):
        np.testing.assert_array_equal(out[k], ref[k])
    with pytest.raises(RuntimeError):   # a full track refuses the whole call
        up.tracks_append(99.0, np.full(67, 5), np.zeros(67), np.zeros((67, 2)), np.zeros((67, 2)))
    up.close()


def test_track_store_anchors_tied_stereo_tracks_like_the_reference(Updater, oracle):
    """Full stereo tracks: both cameras hold the same number of observations, FeatureInitializer.cpp:36-46 keeps the FIRST group of
    its iteration over Feature::timestamps, and libstdc++ iterates that unordered_map in reverse order of insertion: camera 1 when
    the front end inserted camera 0 first (the rule), camera 0 for a track that camera 1 saw first.  The batch assembled on the
    device must anchor every track where the host-flattened batch (which walks the map itself) does — checked through the anchors,
    the accept sets and a complete update in the representation that depends on the anchor most, ANCHORED_MSCKF_INVERSE_DEPTH."""
    prob = synth.make_problem(2, F=60, track="full")
    counts = [np.bincount(prob.cam_idx[prob.meas_offsets[f]:prob.meas_offsets[f + 1]], minlength=2) for f in range(prob.F)]
    tied = np.array([c[0] == c[1] for c in counts])
    assert tied.sum() > 20, "the scene should hold many full stereo tracks"
    # host path = what shim/ovgpu_flatten.h produces from the reference's map: groups in reverse order of first insertion.  Tracks
    # with an odd index are first seen by camera 1 ALONE (one frame before the window), the others by camera 0 then camera 1.
    uv2, uvn2 = prob.uv.reshape(-1, 2), prob.uvn.reshape(-1, 2)
    feat_of = np.repeat(np.arange(prob.F), np.diff(prob.meas_offsets))
    host_sel = []
    for f in range(prob.F):
        a, b = int(prob.meas_offsets[f]), int(prob.meas_offsets[f + 1])
        delivered = ([1] if f % 2 else []) + [int(prob.cam_idx[i]) for i in sorted(range(a, b), key=lambda i: (prob.clone_idx[i], prob.cam_idx[i]))]
        order = list(reversed(list(dict.fromkeys(delivered))))   # the map's iteration: reverse order of first insertion
        host_sel += [i for cam in order for i in range(a, b) if prob.cam_idx[i] == cam]
    host_sel = np.asarray(host_sel)
    import copy
    host = copy.copy(prob)
    host.uv, host.uvn = uv2[host_sel].reshape(-1).copy(), uvn2[host_sel].reshape(-1).copy()
    host.clone_idx, host.cam_idx = prob.clone_idx[host_sel].copy(), prob.cam_idx[host_sel].copy()
    opts = capi.default_options(chi2_multipler=1.0, feat_rep_msckf=capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH)
    ref = oracle.msckf_update(opts, capi.Views(host))
    tri_ref = oracle.triangulate(opts, capi.Views(host))
    anchor_cam_ref = host.cam_idx[tri_ref["anchor_meas"]]
    first_group = host.cam_idx[host.meas_offsets[:-1]]
    assert (anchor_cam_ref[tied] == first_group[tied]).all()           # a tie is anchored in the first group of the iteration
    assert (first_group[tied] == 1).sum() > 5 and (first_group[tied] == 0).sum() > 5
    up = Updater(opts)
    up.set_problem(prob)
    up.tracks_create(128, 70)
    clone_times = 50.0 + 0.1 * np.arange(prob.C)
    odd = np.arange(1, prob.F, 2)
    up.tracks_append(49.0, 2000 + odd, np.ones(len(odd)), np.zeros((len(odd), 2)), np.zeros((len(odd), 2)))   # camera 1 alone, before the window
    for cl in range(prob.C):
        for cam in range(prob.K):
            idx = np.flatnonzero((prob.clone_idx == cl) & (prob.cam_idx == cam))
            if len(idx):
                up.tracks_append(clone_times[cl], 2000 + feat_of[idx], np.full(len(idx), cam), uv2[idx], uvn2[idx])
    up.tracks_to_features(2000 + np.arange(prob.F), clone_times)
    got = up.get_features()
    np.testing.assert_array_equal(got["cam_idx"], host.cam_idx)
    np.testing.assert_array_equal(got["clone_idx"], host.clone_idx)
    np.testing.assert_array_equal(got["uv"], host.uv)
    tri = up.triangulate()
    np.testing.assert_array_equal(tri["anchor_meas"], tri_ref["anchor_meas"])
    out = up.update()
    np.testing.assert_array_equal(out["feat_status"], ref["feat_status"])
    assert _rel(out["dx"], ref["dx"]) < 1e-7 and _rel(out["P"], ref["P"]) < 1e-8
    # and what the wrong order would have done: other anchors for the tied tracks
    up.reset_state()
    up.tracks_group_order(capi.GROUPS_ASCENDING)
    up.tracks_to_features(2000 + np.arange(prob.F), clone_times)
    tri_asc = up.triangulate()
    asc_cam = up.get_features()["cam_idx"][tri_asc["anchor_meas"]]
    assert (asc_cam[tied] == 0).all()
    up.close()


def test_retriangulation_of_the_active_tracks(Updater):
    """SURVEY row N4, VioManager::retriangulate_active_tracks (VioManagerHelper.cpp:190-387): nine frames of a stereo rig, tracks
    entering, missing frames and returning; the device's running systems against the oracle's maps after EVERY frame."""
    from oracle import retri_oracle
    from tests.retri_scene import Scene
    sc = Scene(T=9, n_pts=60, noise=2e-3, p_see=(0.85, 0.7), seed=5)
    opts = capi.default_options()
    up = Updater(opts)
    R, p = sc.pose_table()
    capi.check(up.lib.ovgpu_set_camera_poses(up._ctx, sc.T, sc.K, R.ctypes.data_as(capi.c_double_p), p.ctypes.data_as(capi.c_double_p)), "ovgpu_set_camera_poses")
    at = retri_oracle.ActiveTracks(opts.max_cond_number, opts.min_dist, opts.max_dist)
    n_tri = n_uvd = 0
    for t in range(sc.T):
        ref_pos, ref_uvd = at.frame(sc.R_GtoI[t], sc.p_IinG[t], sc.cams(), sc.obs[t], 752, 480)
        out = up.retriangulate(t, *sc.flat(t), cam0=0, img_w=752, img_h=480)
        assert sorted(out["featid"].tolist()) == sorted(at.count)                       # exactly the tracks alive in this frame
        got = {int(f): q for f, q in zip(out["featid"], out["p_FinG"]) if not np.isnan(q[0])}
        assert set(got) == set(ref_pos)
        for f, q in got.items():
            assert np.abs(q - ref_pos[f]).max() < 1e-9 * max(1.0, np.abs(ref_pos[f]).max())
        guvd = {int(f): q for f, q in zip(out["featid"], out["uvd"]) if not np.isnan(q[0])}
        assert set(guvd) == set(ref_uvd)
        for f, q in guvd.items():
            assert q[0] == ref_uvd[f][0] and q[1] == ref_uvd[f][1] and abs(q[2] - ref_uvd[f][2]) < 1e-9
        n_tri += len(got)
        n_uvd += len(guvd)
    assert n_tri > 100 and n_uvd > 60
    up.retriangulate_reset()
    out = up.retriangulate(0, *sc.flat(0))
    assert np.isnan(out["p_FinG"]).all()                                                 # every system was dropped
    up.close()


def test_zero_velocity_update_algebra(Updater, oracle):
    """the linear algebra of UpdaterZeroVelocity::try_update (UpdaterZeroVelocity.cpp:100-203, :266-277) on the resident
    state through the standalone entry points — compression of the whitened IMU system, the chi2 test on the marginal covariance of
    (orientation, gyro bias, accelerometer bias) with the bias random walk added, bias propagation, EKFUpdate with R = multiplier x I
    — against the same sequence composed from the oracle's functions."""
    prob = synth.make_problem(2, F=4)
    rng = np.random.default_rng(17)
    n_imu, dt, sig_w, sig_a, sig_wb, sig_ab, mult = 21, 0.005, 1.6968e-4, 2.0e-3, 1.9393e-5, 3.0e-3, 10.0
    idx = np.r_[0:3, 9:12, 12:15].astype(np.int32)          # q, bg, ba of the IMU block (State.cpp: q p v bg ba)
    R_GtoI, g = synth.quat_2_rot(prob.clone_q_p[-1, :4]), np.array([0.0, 0.0, 9.81])
    m = 6 * (n_imu - 1)
    H, res = np.zeros((m, 9)), np.zeros(m)
    w_om, w_ac = np.sqrt(dt) / sig_w, np.sqrt(dt) / sig_a       # :127-129
    for i in range(n_imu - 1):
        w_hat = rng.normal(0, 2e-4, 3)                           # a resting IMU: gyro noise, accelerometer = gravity + noise
        a_hat = R_GtoI @ g + rng.normal(0, 3e-3, 3)
        res[6 * i:6 * i + 3] = -w_om * w_hat                                           # :132
        res[6 * i + 3:6 * i + 6] = -w_ac * (a_hat - R_GtoI @ g)                        # :134
        H[6 * i:6 * i + 3, 3:6] = -w_om * np.eye(3)                                    # :141
        Rg = R_GtoI @ g
        H[6 * i + 3:6 * i + 6, 0:3] = -w_ac * np.array([[0, -Rg[2], Rg[1]], [Rg[2], 0, -Rg[0]], [-Rg[1], Rg[0], 0]])  # :143
        H[6 * i + 3:6 * i + 6, 6:9] = -w_ac * np.eye(3)                                # :144
    dt_sum = dt * (n_imu - 1)
    Qb = np.diag([dt_sum * sig_wb ** 2] * 3 + [dt_sum * sig_ab ** 2] * 3)              # :188-190
    # ---- the oracle's sequence
    Hc, rc = oracle.measurement_compress(H, res)
    Pm = prob.P[np.ix_(idx, idx)].copy()
    Pm[3:, 3:] += Qb
    S = Hc @ Pm @ Hc.T + mult * np.eye(len(rc))
    chi2_ref = float(rc @ np.linalg.solve(S, rc))
    st0, P1 = oracle.propagate(prob.P, 9, np.arange(9, 15), np.eye(6), Qb)
    st, P2, dx_ref = oracle.ekf_update(P1, Hc, rc, idx, mult)
    assert st0 == 0 and st == 0 and len(rc) == 9
    # ---- the device
    up = Updater(capi.default_options(chi2_multipler=1.0))
    up.set_problem(prob)
    np.testing.assert_array_equal(up.marginal_covariance(idx), prob.P[np.ix_(idx, idx)])
    out = up.zupt(H, res, idx, Qb, mult)
    assert out["rows"] == 9 and out["accepted"]
    # Every IMU sample contributes the same 6 x 9 Jacobian [0 -w I 0; -w skew(R g) 0 -w I]: H has rank 6, and the compressed 9 x 9
    # system keeps, next to the 6 directions of range(H), THREE directions of the residual space that depend on the elimination order
    # (Givens sweeps in the reference, Householder here).  Their residual entries shift chi2 by (entry)^2 / multiplier and touch
    # nothing else: dx and P' do not see them.  Compared: chi2 of the part inside range(H), which every valid compression shares, and
    # the device's chi2 against numpy on the device's own compressed system.
    Hg, rg = up.measurement_compress(H, res)

    def chi2_in_range(Hm, rm):
        U, sv, _ = np.linalg.svd(Hm)
        k = int((sv > 1e-9 * sv[0]).sum())
        assert k == 6
        Hk, rk = U[:, :k].T @ Hm, U[:, :k].T @ rm
        return float(rk @ np.linalg.solve(Hk @ Pm @ Hk.T + mult * np.eye(k), rk))
    assert abs(chi2_in_range(Hg, rg) / chi2_in_range(Hc, rc) - 1.0) < 1e-9
    Sg = Hg @ Pm @ Hg.T + mult * np.eye(9)
    assert abs(out["chi2"] / float(rg @ np.linalg.solve(Sg, rg)) - 1.0) < 1e-12
    assert abs(out["chi2_thresh"] - oracle.chi2_quantile_95(9)) < 1e-9
    assert _rel(out["dx"], dx_ref) < 1e-8 and _rel(out["P"], P2) < 1e-10
    # a moving IMU (1 rad/s) fails the test and nothing is touched
    res2 = res.copy()
    res2[0::6] += -w_om * 1.0
    again = up.zupt(H, res2, idx, Qb, mult)
    assert not again["accepted"] and "dx" not in again
    np.testing.assert_array_equal(up.get_state()["P"], out["P"])
    up.close()


def test_refinement_alone_from_a_given_estimate(Updater, oracle):
    """FeatureInitializer::single_gaussnewton by itself (ovgpu_refine): seeded with the unrefined triangulation it reproduces, bit for
    bit, what triangulation + refinement in one pass give; seeded with a perturbed estimate it converges to the same point."""
    prob = synth.make_problem(2, F=90)
    lin = Updater(capi.default_options(refine_features=0))
    lin.set_problem(prob)
    seed = lin.triangulate()
    lin.close()
    up = Updater(capi.default_options())
    up.set_problem(prob)
    full = up.triangulate()
    ok = (seed["status"] == 0) & (full["status"] == 0)
    assert ok.sum() > 70
    out = up.refine(seed["p_FinA"], seed["anchor_meas"])
    assert np.array_equal(out["status"][ok], full["status"][ok])
    np.testing.assert_array_equal(out["p_FinA"][ok], full["p_FinA"][ok])
    np.testing.assert_array_equal(out["p_FinG"][ok], full["p_FinG"][ok])
    off = seed["p_FinA"] * (1.0 + 0.02 * np.random.default_rng(5).normal(size=seed["p_FinA"].shape))
    out2 = up.refine(off, seed["anchor_meas"])
    good = ok & (out2["status"] == 0)
    assert good.sum() > 60 and np.abs(out2["p_FinG"][good] - full["p_FinG"][good]).max() < 1e-3
    ref = oracle.triangulate(capi.default_options(), capi.Views(prob))
    assert np.abs(out["p_FinG"][ok] - ref["p_FinG"][ok]).max() < TOL_TRI
    up.close()


def _with_a_long_first_track(prob, length):
    """prob with its first track's observations repeated up to `length` (a track longer than any camera rig produces in one window)."""
    import copy
    a, b = int(prob.meas_offsets[0]), int(prob.meas_offsets[1])
    m = b - a
    reps = -(-length // m)
    sel = np.concatenate([np.tile(np.arange(a, b), reps)[:length], np.arange(b, prob.M)])
    q = copy.copy(prob)
    q.uv = np.ascontiguousarray(prob.uv.reshape(-1, 2)[sel].reshape(-1))
    q.uvn = np.ascontiguousarray(prob.uvn.reshape(-1, 2)[sel].reshape(-1))
    q.clone_idx, q.cam_idx = np.ascontiguousarray(prob.clone_idx[sel]), np.ascontiguousarray(prob.cam_idx[sel])
    q.meas_offsets = np.concatenate([[0], prob.meas_offsets[1:] + (length - m)]).astype(np.int32)
    return q


def test_tracks_beyond_254_observations_are_gated(Updater, oracle):
    """A track of 280 observations: 2m + 4 = 564 gate rows, dof = 557 >= 500 (the reference computes that quantile on the fly,
    UpdaterMSCKF.cpp:216-222).  Beyond the fused kernels (232 observations) and, until round 5, beyond the library (the general kernel's
    panel routine held 512 rows: OVGPU_ERR_CAPACITY): now the panel takes the trapezoid 512 rows at a time (k_system.h) and the
    statistic, the threshold and the update are the oracle's."""
    prob = synth.make_problem(2, F=3)
    q = _with_a_long_first_track(prob, 280)  # (the row store of the general kernel: 160 KB of LDS hold 294 records of 48 doubles next to a 208-column chunk, tests/system_shapes.py)
    out, ref = _check_given(Updater, oracle, q, capi.default_options(chi2_multipler=1.0, gate_always_factor=1), tol_dx=1e-7, tol_p=1e-8)
    assert np.isfinite(out["chi2"][0]) and out["chi2_thresh"][0] > 600.0  # chi2_95(557) = 613.0: beyond the reference's table of 500


def test_tracks_beyond_the_general_kernel_tables_are_refused(Updater):
    """A track of 2500 observations: its block ids and reflectors (80 bytes per observation) do not fit LDS next to the general kernel's
    T chunk — OVGPU_ERR_CAPACITY at ovgpu_set_features, never a silently mis-gated feature.  (The Jacobian records themselves move to a
    global workspace when they do not fit, k_system_t<true>: the fixture ref_msckf_dof_beyond_table, 256 observations at 440 columns.)"""
    prob = synth.make_problem(5, F=3)
    q = _with_a_long_first_track(prob, 2500)
    up = Updater(capi.default_options())
    with pytest.raises(capi.OvgpuError) as ei:
        up.set_problem(q)
    assert ei.value.code == capi.ERR_CAPACITY
    # the context is still usable: the original batch (tracks <= 200) goes through
    up.set_problem(prob)
    out = up.update()
    assert (out["feat_status"] == capi.FEAT_USED).any()
    up.close()


def test_cholesky_follower_timeout_leaves_the_state_untouched_and_recovers(Updater, oracle):
    """k_chol.h: the follower workgroups of the single-launch Cholesky wait (bounded) for a factor workgroup on another stream.  With
    the bound forced to zero every follower gives up: the kernels behind the factorisation must be switched off on the device (the
    resident P / poses stay what they were), and the synchronous call must repeat the update with the step-wise kernels and deliver
    the normal result."""
    prob = synth.make_problem(2, F=120)
    opts = capi.default_options(chi2_multipler=1.0)
    v = capi.Views(prob)
    tri = oracle.triangulate(opts, v)
    ref = oracle.msckf_update(opts, v, given=tri)
    up = Updater(opts)
    up.set_problem(prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    good = up.update()
    assert up.debug_option("chol_timeouts") == 0
    # asynchronous call: nobody repeats it, the error surfaces at synchronize and NOTHING was modified
    up.reset_state()
    assert up.debug_option("chol_follow_spin_limit", 0) == 1 << 22
    up.update_async()
    with pytest.raises(capi.OvgpuError):
        up.synchronize()
    st = up.get_state()
    np.testing.assert_array_equal(st["P"], prob.P)
    np.testing.assert_array_equal(st["clone_q_p"], prob.clone_q_p)
    # synchronous call: repeated with the step-wise kernels
    out = up.update()
    assert up.debug_option("chol_timeouts") == 1
    np.testing.assert_array_equal(out["feat_status"], ref["feat_status"])
    assert _rel(out["dx"], ref["dx"]) < TOL_DX and _rel(out["P"], ref["P"]) < TOL_P
    assert _rel(out["dx"], good["dx"]) < 1e-10
    up.debug_option("chol_follow_spin_limit", 1 << 22)
    up.reset_state()
    again = up.update()
    assert up.debug_option("chol_timeouts") == 1
    np.testing.assert_array_equal(again["dx"], good["dx"])
    up.close()
