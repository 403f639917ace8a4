"""GPU tests (`-m gpu`) of the anchored MSCKF representations on the fused per-feature kernels (k_featy.h: k_feat_rows_anchored).

For an anchored MSCKF feature the nullspace projection annihilates the anchor blocks of the Jacobian (tests/test_anchored_identity.py checks the
identity on the CPU), so such a batch runs the global batch's kernels on 48-double records whose H_f = A dl is evaluated at the p_FinG the
anchor gives.  Everything here is compared against the oracle AT THE ANCHORED REPRESENTATION, with the tolerances and the chi2 rule of
tests/test_gpu_parity.py / tests/parity_util.py (imported): chi2 1e-8, dx 1e-8, P' 1e-9 relative with the oracle's triangulation injected on both
sides, identical accept sets.  Where an existing test of the global representation sets another tolerance for the same situation (resident
landmarks and the semi-definite prior, end to end: 1e-7 / 1e-8; mode A's Gram matrices: 1e-11 / 1e-10; the fp32 stack at 300 features of
configs[2]: 1e-4 / 1e-3) that tolerance is used and the test named."""
import numpy as np
import pytest

from open_vins_amd import capi, synth
from parity_util import assert_chi2, oracle_with_the_same_gate_verdicts
from test_anchored_identity import ANCHORED, SHAPES, make
from test_gpu_msckf_lm import _mix, case, check_landmarks, check_oracle, hand_over
from test_gpu_parity import TOL_CHI2, TOL_DX, TOL_P, _rel

pytestmark = pytest.mark.gpu

MSCKF_ID = capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _opts(rep, **kw):
    return capi.default_options(chi2_multipler=1.0, feat_rep_msckf=rep, **kw)


def _run(Updater, prob, opts, tri, debug=None, p_FinG=None, call="update"):
    """one context: the batch, the oracle's triangulation (p_FinA and the anchor with it), one call; which kernels ran"""
    up = Updater(opts)
    for name, val in (debug or {}).items():
        up.debug_option(name, val)
    up.set_problem(prob)
    up.set_triangulation(tri["p_FinG"] if p_FinG is None else p_FinG, tri["p_FinA"], tri["anchor_meas"], tri["status"])
    out = getattr(up, call)()
    out["kernel"], out["raw"], out["stack_f32"] = up.debug_option("last_feature_kernel"), up.debug_option("last_stack_raw"), up.debug_option("stack_is_f32")
    out["last_route"] = up.lib.ovgpu_last_update_route(up._ctx)
    up.close()
    return out


def _check(oracle, opts, prob, tri, ref, out, tol_dx=TOL_DX, tol_p=TOL_P, what=""):
    """test_gpu_parity._check_given's comparison of one update against the oracle's"""
    ref = oracle_with_the_same_gate_verdicts(oracle, opts, capi.Views(prob), tri, ref, out)
    assert np.array_equal(out["feat_status"], ref["feat_status"])
    gate = np.isfinite(ref["chi2"])
    assert gate.sum() >= 10
    assert_chi2(out, ref, TOL_CHI2, strict=bool(opts.gate_always_factor))
    np.testing.assert_allclose(out["chi2_thresh"][gate], ref["chi2_thresh"][gate], rtol=1e-12)
    e_dx, e_P = _rel(out["dx"], ref["dx"]), _rel(out["P"], ref["P"])
    print(f"{what}: kernel {out['kernel']} raw {out['raw']} used {out['stats']['n_used']}  dx {e_dx:.3e}  P {e_P:.3e}")
    assert out["stats"]["n_used"] == ref["stats"]["n_used"] and out["stats"]["n_rows"] == ref["stats"]["n_rows"] and out["stats"]["D"] == ref["D"]
    assert e_dx < tol_dx and e_P < tol_p
    # the posterior state: 1e-9 / 1e-8 at the float64 tolerances; with a wider dx tolerance (the fp32 stack) dx's tolerance times the size of the
    # correction, test_gpu_fullsize._parity's rule (|dx| ~ 0.1 - 0.3 on these snapshots)
    tol_x = 1e-9 if tol_dx <= TOL_DX else 0.3 * tol_dx
    assert np.abs(out["clone_q_p"] - ref["clone_q_p"]).max() < tol_x and np.abs(out["calib_q_p"] - ref["calib_q_p"]).max() < tol_x
    assert np.abs(out["intrinsics"] - ref["intrinsics"]).max() < 10 * tol_x
    assert np.array_equal(out["P"], out["P"].T)
    return ref


@pytest.fixture(scope="module")
def cases(Updater, oracle):
    """per shape, computed once and shared: the problem, the oracle's triangulation, the oracle's update per representation and the GLOBAL_3D run
    of the library (the twin: which kernel and which stack a global batch of this shape takes)"""
    cache = {}

    def get(shape):
        if shape not in cache:
            prob = make(shape)
            v = capi.Views(prob)
            tri = oracle.triangulate(_opts(capi.REP_GLOBAL_3D), v)
            refs = {}

            def ref(rep):
                if rep not in refs:
                    refs[rep] = oracle.msckf_update(_opts(rep), v, want_compressed=True, given=tri)
                return refs[rep]
            cache[shape] = dict(prob=prob, tri=tri, ref=ref, twin=_run(Updater, prob, _opts(capi.REP_GLOBAL_3D), tri))
        return cache[shape]
    return get


# --------------------------------------------------------------------------- routing
@pytest.mark.parametrize("rep", ANCHORED)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_anchored_batches_take_the_fused_kernels(Updater, oracle, cases, shape, rep):
    c = cases(shape)
    opts = _opts(rep)
    out = _run(Updater, c["prob"], opts, c["tri"])
    assert out["kernel"] in (1, 2)
    assert out["route"] == capi.COMPRESS_GRAM
    assert c["twin"]["kernel"] in (1, 2) and out["raw"] == c["twin"]["raw"]
    _check(oracle, opts, c["prob"], c["tri"], c["ref"](rep), out, what=f"{shape} rep {rep}")
    # what the call hands back keeps its meaning: p_FinG is the triangulation's on every feature it accepted, and the array is the twin's
    ok = c["tri"]["status"] == capi.FEAT_USED
    assert ok.sum() >= 10 and np.array_equal(out["p_FinG"][ok], c["tri"]["p_FinG"][ok])
    assert np.array_equal(out["p_FinG"], c["twin"]["p_FinG"], equal_nan=True)


# --------------------------------------------------------------------------- long tracks, the fp32 stack, every gate matrix factored
def test_long_tracks_take_the_block_row_kernel(Updater, oracle):
    """cfg-5 geometry (50 clones x 4 cameras, up to 200 measurements per feature), as test_gpu_parity.test_update_parity_long_tracks"""
    prob = synth.make_problem(5, F=12)
    assert np.diff(prob.meas_offsets).max() > 120
    opts = _opts(MSCKF_ID)
    tri = oracle.triangulate(opts, capi.Views(prob))
    ref = oracle.msckf_update(opts, capi.Views(prob), given=tri)
    out = _run(Updater, prob, opts, tri)
    assert out["kernel"] == 3 and out["route"] == capi.COMPRESS_GRAM
    _check(oracle, opts, prob, tri, ref, out, what="cfg 5 rep 4")


def test_fp32_stack(Updater, oracle):
    """options.gram_fp32 on 300 features of configs[2]: the shape and the tolerances (dx 1e-4, P 1e-3: float sums of the Gram matrix) of
    test_gpu_fullsize.test_fp32_gram_variant; gate, accept sets and chi2 stay float64"""
    prob = synth.make_problem(2, F=300)
    opts = _opts(MSCKF_ID, gram_fp32=1)
    tri = oracle.triangulate(opts, capi.Views(prob))
    ref = oracle.msckf_update(opts, capi.Views(prob), want_compressed=True, given=tri)
    out = _run(Updater, prob, opts, tri)
    assert out["kernel"] in (1, 2) and out["route"] == capi.COMPRESS_GRAM and out["stack_f32"] == 1 and out["raw"] == 0
    _check(oracle, opts, prob, tri, ref, out, tol_dx=1e-4, tol_p=1e-3, what="fp32 stack rep 4")


@pytest.mark.parametrize("rep", [capi.REP_ANCHORED_FULL_INVERSE_DEPTH, MSCKF_ID])
def test_every_gate_matrix_factored(Updater, oracle, cases, rep):
    """gate_always_factor = 1: every chi2 is the reference's statistic (assert_chi2, strict)"""
    c = cases("ragged_outliers")
    opts = _opts(rep, gate_always_factor=1)
    out = _run(Updater, c["prob"], opts, c["tri"])
    assert out["kernel"] in (1, 2) and out["stats"].get("n_gate_bound", 0) == 0
    _check(oracle, opts, c["prob"], c["tri"], c["ref"](rep), out, what=f"gate_always_factor rep {rep}")


# --------------------------------------------------------------------------- against the global twin
@pytest.mark.parametrize("shape", list(SHAPES))
def test_anchored_run_agrees_with_the_global_twin(Updater, cases, shape):
    """p_FinA and the anchor uploaded through ovgpu_set_triangulation; a second context runs the same batch under GLOBAL_3D at the p_FinG of the
    same triangulation: the same per-feature kernel and the same stack, the same update at the suite's tolerances, equal accept sets"""
    c = cases(shape)
    g = c["twin"]
    for rep in (capi.REP_ANCHORED_3D, capi.REP_ANCHORED_FULL_INVERSE_DEPTH, MSCKF_ID):
        a = _run(Updater, c["prob"], _opts(rep), c["tri"])
        assert a["kernel"] == g["kernel"] and a["kernel"] in (1, 2) and a["raw"] == g["raw"] and a["route"] == g["route"] == capi.COMPRESS_GRAM
        assert np.array_equal(a["feat_status"], g["feat_status"]) and (g["feat_status"] == capi.FEAT_USED).sum() >= 10
        e_dx, e_P = _rel(a["dx"], g["dx"]), _rel(a["P"], g["P"])
        print(f"{shape} rep {rep} against GLOBAL_3D: dx {e_dx:.3e}  P {e_P:.3e}")
        assert e_dx < TOL_DX and e_P < TOL_P
        assert a["stats"]["n_rows"] == g["stats"]["n_rows"] and a["stats"]["D"] == g["stats"]["D"] and a["stats"]["n_used"] == g["stats"]["n_used"]


# --------------------------------------------------------------------------- a p_FinG that disagrees with p_FinA loses
@pytest.mark.parametrize("rep", [capi.REP_ANCHORED_3D, MSCKF_ID])
def test_inconsistent_p_FinG_loses(Updater, cases, rep):
    """UpdaterHelper.cpp:268-280: an anchored feature's p_FinG is formed from p_FinA through the anchor's current pose.  The record kernel never
    reads the supplied p_FinG, so the update is the consistent hand-over's bit for bit; the p_FinG output stays what the caller supplied, as the
    general kernel leaves it."""
    c = cases("14_clones_stereo")
    rng = np.random.default_rng(7)
    wrong = c["tri"]["p_FinG"] + rng.normal(0.0, 0.5, c["tri"]["p_FinG"].shape)
    good = _run(Updater, c["prob"], _opts(rep), c["tri"])
    bad = _run(Updater, c["prob"], _opts(rep), c["tri"], p_FinG=wrong)
    assert good["kernel"] in (1, 2) and bad["kernel"] == good["kernel"]
    assert (good["feat_status"] == capi.FEAT_USED).sum() >= 10
    assert np.array_equal(bad["feat_status"], good["feat_status"]) and np.array_equal(bad["chi2"], good["chi2"], equal_nan=True)
    assert np.array_equal(bad["dx"], good["dx"]) and np.array_equal(bad["P"], good["P"])
    assert np.array_equal(bad["p_FinG"], wrong)
    # ... and so does the general kernel (today's behaviour, kept)
    gen = _run(Updater, c["prob"], _opts(rep), c["tri"], p_FinG=wrong, debug=dict(anchored_fast=0))
    assert gen["kernel"] == 0 and np.array_equal(gen["feat_status"], good["feat_status"])
    assert _rel(gen["dx"], good["dx"]) < TOL_DX and _rel(gen["P"], good["P"]) < TOL_P


# --------------------------------------------------------------------------- the switch
@pytest.mark.parametrize("rep", ANCHORED)
def test_anchored_fast_off_restores_the_general_kernel(Updater, oracle, cases, rep):
    c = cases("ragged_outliers")
    opts = _opts(rep)
    up = Updater(opts)
    assert up.debug_option("anchored_fast") == 1  # on by default
    up.close()
    off = _run(Updater, c["prob"], opts, c["tri"], debug=dict(anchored_fast=0))
    on = _run(Updater, c["prob"], opts, c["tri"])
    assert off["kernel"] == 0 and on["kernel"] in (1, 2) and off["route"] == on["route"] == capi.COMPRESS_GRAM
    ref = _check(oracle, opts, c["prob"], c["tri"], c["ref"](rep), off, what=f"anchored_fast = 0 rep {rep}")
    _check(oracle, opts, c["prob"], c["tri"], ref, on, what=f"anchored_fast = 1 rep {rep}")
    assert np.array_equal(off["feat_status"], on["feat_status"])
    assert _rel(off["dx"], on["dx"]) < TOL_DX and _rel(off["P"], on["P"]) < TOL_P
    assert off["stats"]["n_rows"] == on["stats"]["n_rows"] and off["stats"]["D"] == on["stats"]["D"]
    # a global batch never asked: the switch changes nothing there
    g = _run(Updater, c["prob"], _opts(capi.REP_GLOBAL_3D), c["tri"], debug=dict(anchored_fast=0))
    assert g["kernel"] == c["twin"]["kernel"] and np.array_equal(g["dx"], c["twin"]["dx"]) and np.array_equal(g["P"], c["twin"]["P"])


# --------------------------------------------------------------------------- resident landmarks
@pytest.mark.parametrize("rep", [capi.REP_ANCHORED_FULL_INVERSE_DEPTH, MSCKF_ID])
def test_update_lm_with_anchored_msckf_features(Updater, oracle, rep):
    """ovgpu_msckf_update_lm on a state with resident landmarks (global, anchored and single-depth ones) and an anchored feat_rep_msckf: the
    fused kernel, the oracle's update of the landmark-free twin (test_gpu_msckf_lm's tolerances, end to end: dx 1e-7, P 1e-8), and the landmarks
    corrected: value_in + dx, exactly.  ovgpu_msckf_update on the same state keeps the general kernel."""
    L = 8
    slam, msckf, plain = case(2, L, 60, _mix(L), seed=3)
    opts = _opts(rep)
    ref = oracle.msckf_update(opts, capi.Views(plain))
    up = Updater(opts)
    hand_over(up, msckf)
    out = up.update_lm()
    assert out["route"] == capi.COMPRESS_GRAM and up.debug_option("last_feature_kernel") in (1, 2)
    check_oracle(out, ref, f"update_lm, feat_rep_msckf {rep}")
    check_landmarks(up, msckf, out)
    up.close()
    up = Updater(opts)
    hand_over(up, msckf)
    out = up.update()
    assert up.debug_option("last_feature_kernel") == 0
    check_oracle(out, ref, f"update on a landmark state, feat_rep_msckf {rep}")
    up.close()


# --------------------------------------------------------------------------- mode A
def test_mode_a_takes_the_pivoted_gram_factor(Updater, oracle):
    """ovgpu_msckf_compress under ANCHORED_MSCKF_INVERSE_DEPTH: the fused kernels' projected whitened stack, the pivoted Cholesky factor of its
    Gram matrix, un-whitened — H^T H / H^T r against the oracle's compressed system at test_gpu_parity.test_mode_a_compressed_system's tolerance"""
    prob = synth.make_problem(2, F=100)
    opts = _opts(MSCKF_ID)
    v = capi.Views(prob)
    tri = oracle.triangulate(opts, v)
    ref = oracle.msckf_update(opts, v, want_compressed=True, given=tri)
    cmp = _run(Updater, prob, opts, tri, call="compress")
    assert cmp["last_route"] == capi.COMPRESS_PCHOLQR and cmp["kernel"] in (1, 2) and cmp["raw"] == 0
    assert cmp["D"] == ref["D"] and 0 < cmp["rows"] <= cmp["D"]
    assert np.array_equal(cmp["col_cov_id"], oracle.column_map(opts, v)) and np.array_equal(cmp["feat_status"], ref["feat_status"])
    H, r = cmp["H"], cmp["r"]
    G, g = ref["H_comp"].T @ ref["H_comp"], ref["H_comp"].T @ ref["r_comp"]
    eG, eg = np.linalg.norm(H.T @ H - G) / np.linalg.norm(G), np.linalg.norm(H.T @ r - g) / np.linalg.norm(g)
    print(f"mode A, rep 4: |H^T H - G| / |G| = {eG:.1e}, |H^T r - g| / |g| = {eg:.1e}")
    assert eG < 1e-11 and eg < 1e-10
    st, P1, dx1 = oracle.ekf_update(prob.P, H, r, cmp["col_cov_id"], 1.0)
    assert st == 0 and _rel(P1, ref["P"]) < TOL_P and _rel(dx1, ref["dx"]) < TOL_DX


# --------------------------------------------------------------------------- fall-backs
def test_semi_definite_prior_still_falls_back(Updater, oracle):
    """test_gpu_parity.test_semi_definite_prior_takes_the_householder_route's prior (the newest clone an exact copy of the one before) and its
    tolerances, under an anchored representation: the call repeats through the Householder route, on the general kernel"""
    prob = synth.make_problem(2, F=120)
    A = np.eye(prob.N)
    i, j = int(prob.clone_cov_id[28]), int(prob.clone_cov_id[29])
    A[j:j + 6, :] = 0.0
    A[j:j + 6, i:i + 6] = np.eye(6)
    prob.P = A @ prob.P @ A.T
    opts = _opts(MSCKF_ID)
    v = capi.Views(prob)
    tri = oracle.triangulate(opts, v)
    ref = oracle.msckf_update(opts, v, given=tri)
    assert ref["stats"]["status"] == 0 and ref["stats"]["n_used"] > 30
    out = _run(Updater, prob, opts, tri)
    assert out["stats"]["status"] == 0 and out["route"] == capi.COMPRESS_TSQR and out["kernel"] == 0
    assert np.array_equal(out["feat_status"], ref["feat_status"])
    assert _rel(out["dx"], ref["dx"]) < 1e-7 and _rel(out["P"], ref["P"]) < 1e-8
    assert np.abs(out["clone_q_p"] - ref["clone_q_p"]).max() < 1e-9


def test_per_feature_sigma_still_falls_back(Updater, oracle, cases):
    """a per-feature sigma (the options' own value for every feature, so the oracle's update is the expected one) keeps the general kernel"""
    c = cases("14_clones_stereo")
    opts = _opts(MSCKF_ID)
    up = Updater(opts)
    up.set_problem(c["prob"])
    tri = c["tri"]
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    up.set_feature_options(sigma_pix=np.full(c["prob"].F, opts.sigma_pix))
    out = up.update()
    out["kernel"], out["raw"] = up.debug_option("last_feature_kernel"), up.debug_option("last_stack_raw")
    up.close()
    assert out["kernel"] == 0 and out["route"] == capi.COMPRESS_GRAM
    _check(oracle, opts, c["prob"], tri, c["ref"](MSCKF_ID), out, what="per-feature sigma rep 4")


def test_no_fast_feature_kernel_still_falls_back(Updater, oracle, cases):
    c = cases("14_clones_stereo")
    opts = _opts(MSCKF_ID, no_fast_feature_kernel=1)
    out = _run(Updater, c["prob"], opts, c["tri"])
    assert out["kernel"] == 0 and out["route"] == capi.COMPRESS_GRAM
    _check(oracle, opts, c["prob"], c["tri"], c["ref"](MSCKF_ID), out, what="no_fast_feature_kernel rep 4")
