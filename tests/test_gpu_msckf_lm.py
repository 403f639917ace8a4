"""GPU tests (`-m gpu`) of ovgpu_msckf_update_lm: UpdaterMSCKF::update (VioManager.cpp:525) on a state that carries SLAM landmarks, with the resident
landmark values corrected on the device (Landmark::update) so that the SLAM update that follows (VioManager.cpp:529-547) linearises at current
estimates without an ovgpu_set_landmarks in between.

Inputs are built as tests/test_gpu_parity.py::test_msckf_update_with_resident_landmarks builds them: the state and landmarks of
synth.make_slam_problem, the MSCKF batch of synth.make_problem, and the landmark-free twin — the same N, P, clones and calibration with the landmarks
undeclared, their rows of P extra rows as the IMU block's are.

Tolerances.  Against the oracle: dx 1e-7 and P' 1e-8 relative, accept sets identical (that test's).  Landmarks: value_in + dx[id .. id + dof) computed
in numpy from the RETURNED dx — one float64 add, compared exactly.  Against the landmark-free route of the same library, and between a context that
kept its landmarks resident and one that had them uploaded again: the same kernels run on the same column map and the same inputs, so every output is
compared bit for bit."""
import copy

import numpy as np
import pytest

from open_vins_amd import capi, synth

pytestmark = pytest.mark.gpu

MIX = [capi.REP_GLOBAL_3D, capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE, capi.REP_ANCHORED_3D, capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE,
       capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, capi.REP_GLOBAL_3D, capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE, capi.REP_GLOBAL_FULL_INVERSE_DEPTH]
BATCH = ("meas_offsets", "uv", "uvn", "clone_idx", "cam_idx", "p_FinG_true")


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _mix(L):
    return np.array((MIX * ((L + 7) // 8))[:L], np.int32)


def case(cfg, L, F, lm_rep, seed, **kw):
    """(slam, msckf, plain): the landmark state with its own SLAM tracks, the same state with an MSCKF batch, and the landmark-free twin of that"""
    slam = synth.make_slam_problem(cfg, L=L, lm_rep=lm_rep, seed=seed, **kw)
    tracks = synth.make_problem(cfg, F=F, seed=seed + 1, **kw)
    msckf = copy.copy(slam)
    for k in BATCH:
        setattr(msckf, k, getattr(tracks, k))
    plain = synth.make_problem(cfg, F=F, seed=seed + 1, **kw)
    plain.N, plain.P = slam.N, slam.P
    plain.clone_q_p, plain.clone_q_p_fej, plain.calib_q_p, plain.intrinsics = slam.clone_q_p, slam.clone_q_p_fej, slam.calib_q_p, slam.intrinsics
    return slam, msckf, plain


def reps_of(prob):
    L = prob.lm_cov_id.shape[0]
    each = getattr(prob, "lm_rep_each", None)
    return np.asarray(each, np.int32) if each is not None else np.full(L, prob.lm_rep, np.int32)


def corrected(prob, dx):
    """Landmark::update on the host: value += dx[id .. id + dof); a single-depth landmark's last stored value takes dx[id] (Landmark.cpp:130-140)"""
    val = np.array(prob.lm_value, dtype=np.float64, copy=True)
    for l, (rep, cid) in enumerate(zip(reps_of(prob), prob.lm_cov_id)):
        if rep == capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE:
            val[l, 2] = val[l, 2] + dx[cid]
        else:
            val[l] = val[l] + dx[cid:cid + 3]
    return val


def hand_over(up, prob, active=()):
    """ovgpu_set_state, ovgpu_set_landmarks, ovgpu_set_active_landmarks, ovgpu_set_features: the order include/ovgpu.h documents"""
    up.set_slam_state(prob)
    up.set_active_landmarks(active)
    up.set_features(prob)


def check_landmarks(up, prob, out):
    """lm_out and the resident values are value_in + dx, exactly; FEJ values and anchors as uploaded"""
    want = corrected(prob, out["dx"])
    assert np.abs(want - prob.lm_value).max() > 0  # the correction reaches them through P
    assert np.array_equal(out["landmarks"], want)
    got = up.get_landmarks()
    assert np.array_equal(got["value"], want)
    assert np.array_equal(got["fej"], prob.lm_fej) and np.array_equal(got["cov_id"], prob.lm_cov_id)
    assert np.array_equal(got["feat_rep"], reps_of(prob))
    anchored = reps_of(prob) >= capi.REP_ANCHORED_3D
    if anchored.any():
        assert np.array_equal(got["anchor_cam"][anchored], prob.lm_anchor_cam[anchored])
        assert np.array_equal(got["anchor_clone"][anchored], prob.lm_anchor_clone[anchored])
    assert (got["anchor_cam"][~anchored] == -1).all() and (got["anchor_clone"][~anchored] == -1).all()


def check_oracle(out, ref, what=""):
    print(f"{what}: used {out['stats']['n_used']}  dx {_rel(out['dx'], ref['dx']):.3e}  P {_rel(out['P'], ref['P']):.3e}")
    assert np.array_equal(out["feat_status"], ref["feat_status"])
    assert (ref["feat_status"] == capi.FEAT_USED).sum() >= 10
    assert _rel(out["dx"], ref["dx"]) < 1e-7 and _rel(out["P"], ref["P"]) < 1e-8
    for k in ("clone_q_p", "calib_q_p"):
        assert np.abs(out[k] - ref[k]).max() < 1e-9


# --------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("lm_rep", [capi.REP_GLOBAL_3D, capi.REP_ANCHORED_FULL_INVERSE_DEPTH, "mix"], ids=["global", "anchored", "mix_single_depth"])
def test_update_lm_against_the_oracle(Updater, oracle, lm_rep):
    L = 8
    slam, msckf, plain = case(2, L, 60, _mix(L) if lm_rep == "mix" else lm_rep, seed=3)
    if lm_rep == "mix":
        assert (reps_of(msckf) == capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE).sum() == 3 and msckf.N == plain.N == slam.N
    opts = capi.default_options(chi2_multipler=1.0)
    ref = oracle.msckf_update(opts, capi.Views(plain))
    up = Updater(opts)
    hand_over(up, msckf)
    out = up.update_lm()
    check_oracle(out, ref, f"update_lm rep {lm_rep}")
    check_landmarks(up, msckf, out)
    assert out["route"] == capi.COMPRESS_GRAM and up.debug_option("last_feature_kernel") in (1, 2)  # the fused per-feature kernel
    up.close()


# --------------------------------------------------------------------------- 2. against the landmark-free route of the same library
@pytest.mark.parametrize("shape", [dict(cfg=2, F=200), dict(cfg=2, F=80, C=6, max_baseline=400.0), dict(cfg=5, F=12, L=3)],
                         ids=["30_clones_stereo", "6_clones", "long_tracks"])
def test_update_lm_returns_the_bits_of_the_landmark_free_route(Updater, shape):
    """The twin runs ovgpu_msckf_update with the landmarks undeclared (unchanged code): same N, same column map, same kernels, same inputs.  The
    landmark states carry anchored landmarks, whose 72-double Jacobian records are the general kernel's: the fused kernels keep their 48."""
    kw = dict(shape)
    cfg, F, L = kw.pop("cfg"), kw.pop("F"), kw.pop("L", 8)
    # (six clones span a short baseline: FeatureInitializerOptions::max_baseline = 40 rejects every feature of that window, 400 accepts 79 of 80)
    opts = capi.default_options(chi2_multipler=1.0, max_baseline=kw.pop("max_baseline", 40.0))
    slam, msckf, plain = case(cfg, L, F, _mix(L), seed=5, **kw)
    assert (reps_of(msckf) >= capi.REP_ANCHORED_3D).any()
    a = Updater(opts)
    a.set_problem(plain)
    ra = a.update()
    want_kernel = a.debug_option("last_feature_kernel")
    if cfg == 5:
        assert np.diff(msckf.meas_offsets).max() > 120 and want_kernel == 3  # k_feat_y_big
    else:
        assert want_kernel in (1, 2)
    b = Updater(opts)
    hand_over(b, msckf)
    rb = b.update_lm()
    assert rb["route"] == ra["route"] == capi.COMPRESS_GRAM
    assert b.debug_option("last_feature_kernel") == want_kernel and b.debug_option("last_stack_raw") == a.debug_option("last_stack_raw")
    assert (ra["feat_status"] == capi.FEAT_USED).sum() >= min(10, F // 2)
    for k in ("dx", "P", "chi2", "chi2_thresh", "p_FinG"):
        d = np.abs(np.nan_to_num(rb[k]) - np.nan_to_num(ra[k])).max()
        print(f"{k}: max |difference| {d:.3e}")
    assert np.array_equal(rb["feat_status"], ra["feat_status"])
    for k in ("chi2", "chi2_thresh", "p_FinG"):
        assert np.array_equal(rb[k], ra[k], equal_nan=True), k
    assert np.array_equal(rb["dx"], ra["dx"]) and np.array_equal(rb["P"], ra["P"])
    for k in ("clone_q_p", "calib_q_p", "intrinsics"):
        assert np.array_equal(rb[k], ra[k]), k
    assert rb["stats"]["n_used"] == ra["stats"]["n_used"] and rb["stats"]["n_rows"] == ra["stats"]["n_rows"] and rb["stats"]["D"] == ra["stats"]["D"]
    check_landmarks(b, msckf, rb)
    a.close(), b.close()


# --------------------------------------------------------------------------- 3. the landmarks are current
def test_slam_update_after_update_lm_needs_no_landmark_upload(Updater):
    """One context keeps the landmarks resident through update_lm and runs the frame's SLAM update; a second one gets the first update's posterior
    uploaded, landmarks corrected on the host, and runs the same SLAM call: identical.  A third repeats the first with update() — stale landmarks —
    and must differ, or a correction that does nothing would pass."""
    L = 8
    slam, msckf, plain = case(2, L, 60, _mix(L), seed=3)
    ids = np.arange(L, dtype=np.int32)
    opts = capi.default_options(chi2_multipler=1.0)

    def slam_call(up):
        up.set_active_landmarks(ids)
        up.set_features(slam)
        return up.slam_update(lm_index=slam.lm_index)

    a = Updater(opts)
    hand_over(a, msckf)
    first = a.update_lm()
    assert first["stats"]["n_used"] >= 10
    ra = slam_call(a)
    assert (ra["feat_status"] == capi.FEAT_USED).sum() >= 3

    post = copy.copy(slam)  # the posterior of the MSCKF update as a caller without the entry hands it over again
    post.P, post.clone_q_p, post.calib_q_p, post.intrinsics = first["P"], first["clone_q_p"], first["calib_q_p"], first["intrinsics"]
    post.lm_value = corrected(msckf, first["dx"])
    b = Updater(opts)
    b.set_slam_problem(post)
    rb = slam_call(b)
    for k in ("dx", "P", "landmarks"):
        print(f"{k}: max |difference| {np.abs(rb[k] - ra[k]).max():.3e}")
    assert np.array_equal(ra["feat_status"], rb["feat_status"])
    assert np.array_equal(ra["chi2"], rb["chi2"], equal_nan=True)
    assert np.array_equal(ra["dx"], rb["dx"]) and np.array_equal(ra["P"], rb["P"]) and np.array_equal(ra["landmarks"], rb["landmarks"])

    c = Updater(opts)
    hand_over(c, msckf)
    stale = c.update()
    assert np.array_equal(stale["feat_status"], first["feat_status"]) and _rel(stale["dx"], first["dx"]) < 1e-9
    rc = slam_call(c)
    assert not np.array_equal(rc["dx"], ra["dx"]) and not np.array_equal(rc["landmarks"], ra["landmarks"])
    assert np.abs(rc["landmarks"] - ra["landmarks"]).max() > 1e-6  # the MSCKF update's correction of the landmarks is missing
    a.close(), b.close(), c.close()


# --------------------------------------------------------------------------- 4. fall-backs and refusals
def test_batch_laid_out_with_landmark_columns_is_refused(Updater):
    slam, msckf, plain = case(2, 8, 40, _mix(8), seed=3)
    up = Updater(capi.default_options(chi2_multipler=1.0))
    up.set_slam_problem(msckf)  # no active set named: every landmark has its columns
    for attempt in ("all", "some"):
        if attempt == "some":
            up.set_active_landmarks([1, 4])
            up.set_features(msckf)
        out = up.update_lm(check=False)
        assert out["rc"] == capi.ERR_INVALID
        msg = up.lib.ovgpu_last_error().decode()
        assert "ovgpu_set_active_landmarks(ctx, NULL, 0)" in msg and "ovgpu_set_features" in msg
        assert not out["dx"].any() and not out["landmarks"].any()  # nothing was written
        st, lm = up.get_state(), up.get_landmarks()
        assert np.array_equal(st["P"], msckf.P) and np.array_equal(st["clone_q_p"], msckf.clone_q_p) and np.array_equal(st["calib_q_p"], msckf.calib_q_p)
        assert np.array_equal(lm["value"], msckf.lm_value) and np.array_equal(lm["fej"], msckf.lm_fej)
    # the fix the message names
    up.set_active_landmarks([])
    up.set_features(msckf)
    out = up.update_lm()
    check_landmarks(up, msckf, out)
    up.close()


def test_semi_definite_prior_repeats_through_householder_and_corrects_once(Updater, oracle):
    """The two perfectly correlated variables of tests/test_gpu_parity.py::test_semi_definite_prior_takes_the_householder_route: the device skips
    everything behind the prior block's factorisation — the landmark correction with it — and the repeat corrects the landmarks once."""
    slam, msckf, plain = case(2, 8, 120, _mix(8), seed=3)
    A = np.eye(msckf.N)
    i, j = int(msckf.clone_cov_id[28]), int(msckf.clone_cov_id[29])
    A[j:j + 6, :] = 0.0
    A[j:j + 6, i:i + 6] = np.eye(6)
    msckf.P = plain.P = A @ msckf.P @ A.T  # positive semi-definite, rank N - 6
    opts = capi.default_options(chi2_multipler=1.0)
    ref = oracle.msckf_update(opts, capi.Views(plain))
    assert ref["stats"]["status"] == 0 and ref["stats"]["n_used"] > 30
    up = Updater(opts)
    hand_over(up, msckf)
    out = up.update_lm()
    assert out["stats"]["status"] == 0 and out["route"] == capi.COMPRESS_TSQR
    check_oracle(out, ref, "semi-definite prior")
    check_landmarks(up, msckf, out)  # value_in + dx: once
    up.close()


@pytest.mark.parametrize("how", ["no_fast_feature_kernel", "per_feature_sigma"])
def test_general_kernel_fallback_corrects_the_landmarks(Updater, oracle, how):
    """Where the landmark-free conditions fail the call takes the general kernel, as ovgpu_msckf_update does.  The per-feature sigma is the options'
    own value for every feature, so the oracle's update is the expected one."""
    slam, msckf, plain = case(2, 8, 60, _mix(8), seed=3)
    opts = capi.default_options(chi2_multipler=1.0, no_fast_feature_kernel=1 if how == "no_fast_feature_kernel" else 0)
    ref = oracle.msckf_update(opts, capi.Views(plain))
    up = Updater(opts)
    hand_over(up, msckf)
    if how == "per_feature_sigma":
        up.set_feature_options(sigma_pix=np.full(msckf.F, opts.sigma_pix))
    out = up.update_lm()
    assert up.debug_option("last_feature_kernel") == 0 and out["route"] == capi.COMPRESS_GRAM
    check_oracle(out, ref, how)
    check_landmarks(up, msckf, out)
    up.close()


def test_without_landmarks_the_entry_is_msckf_update(Updater):
    prob = synth.make_problem(2, F=120, seed=6)
    opts = capi.default_options(chi2_multipler=1.0)
    outs = []
    for entry in ("update", "update_lm"):
        up = Updater(opts)
        up.set_problem(prob)
        outs.append(getattr(up, entry)())
        up.close()
    a, b = outs
    assert b["landmarks"].shape == (0, 3) and a["stats"]["n_used"] >= 10
    assert np.array_equal(a["feat_status"], b["feat_status"]) and np.array_equal(a["chi2"], b["chi2"], equal_nan=True)
    assert np.array_equal(a["dx"], b["dx"]) and np.array_equal(a["P"], b["P"]) and np.array_equal(a["clone_q_p"], b["clone_q_p"])
    assert a["route"] == b["route"] == capi.COMPRESS_GRAM


@pytest.mark.parametrize("active", [None, ()], ids=["all_landmarks", "empty_set"])
def test_msckf_update_still_leaves_the_landmarks_alone(Updater, oracle, active):
    """ovgpu_msckf_update keeps its behaviour on a landmark state: the general kernel, dx and P' over all N rows, landmark values as uploaded."""
    slam, msckf, plain = case(2, 8, 60, _mix(8), seed=3)
    opts = capi.default_options(chi2_multipler=1.0)
    ref = oracle.msckf_update(opts, capi.Views(plain))
    up = Updater(opts)
    if active is None:
        up.set_slam_problem(msckf)
    else:
        hand_over(up, msckf, active)
    out = up.update()
    assert up.debug_option("last_feature_kernel") == 0
    check_oracle(out, ref, "ovgpu_msckf_update")
    lm = up.get_landmarks()
    assert np.array_equal(lm["value"], msckf.lm_value) and np.array_equal(lm["fej"], msckf.lm_fej)
    assert np.abs(out["dx"][msckf.lm_cov_id[0]:]).max() > 0
    up.close()
