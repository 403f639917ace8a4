"""GPU parity tests (`-m gpu`): ovgpu_slam_delayed_init_fused (csrc/k_init_fused.h: five launches per candidate) against

  (a) the oracle's slam_delayed_init,
  (b) the existing entry ovgpu_slam_delayed_init,
  (c) the new entry,

all three on the oracle's triangulation.  Statuses, lm_cov_id, N, anchors and landmark slots are identical across the three; (c) against (a) and (c)
against (b) meet the tolerances of tests/test_gpu_parity.py::_check_delayed_init (restated in _check); get_state(P=True) and get_landmarks() equal what
the call returned; "delayed_init_fused_steps" counts the candidates with two or more measurements and "delayed_init_chain_steps" stays 0, except where
a case says otherwise.  Every gated candidate of every case is further than GATE_MARGIN from its threshold on the oracle (asserted, never skipped):
a candidate within rounding of the gate could legitimately go either way and the chains would diverge from there.

Shapes: the smallest at which the named part of the step can go wrong (C <= 12, F <= 20 unless the case needs more).
"""
import numpy as np
import pytest

import track_shapes as ts
from open_vins_amd import capi, synth

pytestmark = pytest.mark.gpu

GATE_MARGIN = 1e-6
M_MAX = 64  # include/ovgpu.h: the fused step holds tracks of m <= 64 measurements
SINGLE = capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE
REPS5 = [capi.REP_GLOBAL_3D, capi.REP_GLOBAL_FULL_INVERSE_DEPTH, capi.REP_ANCHORED_3D, capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, SINGLE]
TRACK_KEYS = ("meas_offsets", "uv", "uvn", "clone_idx", "cam_idx", "p_FinG_true")


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


class Case:
    def __init__(self, prob, rep=0, opts=None, each=None, sig=None, mult=None, slam=False):
        self.prob, self.rep, self.each, self.sig, self.mult, self.slam = prob, rep, each, sig, mult, slam
        self.opts = opts if opts is not None else capi.default_options(chi2_multipler=1.0)
        self.L0 = len(prob.lm_cov_id) if slam else 0


def _oracle(oracle, case):
    v = capi.Views(case.prob)
    tri = oracle.triangulate(case.opts, v)
    ref = oracle.slam_delayed_init(case.opts, v, feat_rep=case.rep, tri=tri, feat_sigma=case.sig, feat_chi2mult=case.mult, feat_rep_each=case.each)
    assert ref["rc"] == 0
    gate = np.isfinite(ref["chi2"]) & (ref["chi2_thresh"] > 0)
    # a candidate on its threshold fails loudly here
    assert (np.abs(ref["chi2"][gate] / ref["chi2_thresh"][gate] - 1.0) > GATE_MARGIN).all(), "a candidate sits on its gate threshold: pick another seed"
    return tri, ref


def _run(Updater, case, tri, fused, debug=None):
    up = Updater(case.opts)
    for name, val in (debug or {}).items():
        up.debug_option(name, val)
    if case.slam:  # include/ovgpu.h: state, landmarks, the (empty) active set, then the batch
        up.set_slam_problem(case.prob)
        up.set_active_landmarks([])
        up.set_features(case.prob)
    else:
        up.set_problem(case.prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    if case.sig is not None or case.mult is not None:
        up.set_feature_options(case.sig, case.mult)
    up.debug_option("delayed_init_fused_steps", 0), up.debug_option("delayed_init_chain_steps", 0)
    out = up.delayed_init(case.rep, feat_rep_each=case.each, fused=fused)
    post, lm = up.get_state(P=True), up.get_landmarks()
    steps = (up.debug_option("delayed_init_fused_steps"), up.debug_option("delayed_init_chain_steps"))
    return up, out, post, lm, steps


def _check(out, ref, post, ref_post, gate, tag):
    """tests/test_gpu_parity.py::_check_delayed_init, restated: chi2 1e-7, values 1e-8 / 1e-10, FEJ 1e-12, dx_seq 1e-6, P 1e-7, P symmetric to
    1e-13 of its largest entry, poses 1e-9; the integer outputs identical."""
    assert np.array_equal(out["feat_status"], ref["feat_status"])
    np.testing.assert_allclose(out["chi2"][gate], ref["chi2"][gate], rtol=1e-7)
    np.testing.assert_allclose(out["chi2_thresh"][gate], ref["chi2_thresh"][gate], rtol=1e-12)
    assert out["N"] == ref["N"] and np.array_equal(out["lm_cov_id"], ref["lm_cov_id"])
    acc = ref["lm_cov_id"] >= 0
    anchored = ref["anchor_cam"] >= 0  # (the oracle reports an anchor for the anchored representations only)
    assert np.array_equal(out["anchor_cam"][anchored], ref["anchor_cam"][anchored]) and np.array_equal(out["anchor_clone"][anchored], ref["anchor_clone"][anchored])
    d_dx = _rel(out["dx_seq"], ref["dx_seq"]) if ref["dx_seq"].any() else float(np.abs(out["dx_seq"]).max(initial=0.0))
    d_val = float(np.abs(out["lm_value"][acc] - ref["lm_value"][acc]).max(initial=0.0))
    d_pose = max(float(np.abs(post[k] - ref_post[k]).max()) for k in ("clone_q_p", "calib_q_p", "intrinsics"))
    print(f"{tag}: dx_seq {d_dx:.3e}  P {_rel(out['P'], ref['P']):.3e}  values {d_val:.3e}  poses {d_pose:.3e}")
    np.testing.assert_allclose(out["lm_value"][acc], ref["lm_value"][acc], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(out["lm_fej"][acc], ref["lm_fej"][acc], rtol=1e-12, atol=1e-14)
    assert np.isnan(out["lm_value"][~acc]).all()
    assert d_dx < 1e-6 and not out["dx_seq"][~acc].any()
    assert _rel(out["P"], ref["P"]) < 1e-7
    np.testing.assert_allclose(out["P"], out["P"].T, rtol=0, atol=1e-13 * np.abs(out["P"]).max())
    assert d_pose < 1e-9


def _three(Updater, oracle, case, want_steps=None, keep=False):
    """Runs (a), (b), (c) and every comparison of the module's docstring; returns (ref, (b), (c)) — with the two contexts still open when keep."""
    tri, ref = _oracle(oracle, case)
    b = _run(Updater, case, tri, fused=False)
    c = _run(Updater, case, tri, fused=True)
    (up_b, out_b, post_b, lm_b, steps_b), (up_c, out_c, post_c, lm_c, steps_c) = b, c
    try:
        gate = np.isfinite(ref["chi2"])
        acc = ref["lm_cov_id"] >= 0
        # ---- identical across the three
        for k in ("feat_status", "lm_cov_id", "anchor_cam", "anchor_clone"):
            assert np.array_equal(out_b[k], out_c[k]), k
        assert out_b["N"] == out_c["N"] == ref["N"]
        for k in ("cov_id", "anchor_cam", "anchor_clone", "feat_rep"):
            assert np.array_equal(lm_b[k], lm_c[k]), k
        assert len(lm_c["cov_id"]) == case.L0 + acc.sum() and np.array_equal(lm_c["cov_id"][case.L0:], ref["lm_cov_id"][acc])
        # ---- (c) against (a), (c) against (b)
        _check(out_c, ref, post_c, ref, gate, "(c)-(a)")
        _check(out_c, out_b, post_c, post_b, gate, "(c)-(b)")
        if case.L0:
            np.testing.assert_allclose(lm_c["value"][:case.L0], ref["landmarks_existing"], rtol=1e-8, atol=1e-10)
            np.testing.assert_allclose(lm_c["value"][:case.L0], lm_b["value"][:case.L0], rtol=1e-8, atol=1e-10)
        # ---- the resident state is what the call returned
        assert post_c["P"].shape == out_c["P"].shape and np.array_equal(post_c["P"], out_c["P"])
        assert np.array_equal(lm_c["value"][case.L0:], out_c["lm_value"][acc]) and np.array_equal(lm_c["fej"][case.L0:], out_c["lm_fej"][acc])
        # ---- which step the candidates took
        n2 = int((np.diff(case.prob.meas_offsets) >= 2).sum())
        assert steps_c == ((n2, 0) if want_steps is None else want_steps)
        assert steps_b == (0, 0)  # the existing entry does not count
    finally:
        if not keep:
            up_b.close(), up_c.close()
    return ref, b, c


def _tracks_from(prob, tracks):
    for k in TRACK_KEYS:
        setattr(prob, k, getattr(tracks, k))
    return prob


# --------------------------------------------------------------------------- accepted and rejected candidates interleaved, every representation
@pytest.mark.parametrize("rep", REPS5)
def test_representations_with_interleaved_rejections(Updater, oracle, rep):
    """The predicated tail and the counters: rejected candidates between accepted ones.  rep = single depth: sz = 1, the covariance grows by 1, only
    the third row of G initialises the landmark."""
    case = Case(synth.make_problem(2, C=12, F=16, outlier_frac=0.2), rep)
    ref, _, _ = _three(Updater, oracle, case)
    acc = ref["lm_cov_id"] >= 0
    assert 4 <= acc.sum() < 16 and not acc[np.flatnonzero(acc)[0]:np.flatnonzero(acc)[-1]].all()  # a rejection between two acceptances
    assert ref["N"] == case.prob.N + (1 if rep == SINGLE else 3) * acc.sum()


# --------------------------------------------------------------------------- W's row tiles
@pytest.mark.parametrize("m", [2, 8, 9])
def test_track_length_at_the_row_tile_edges(Updater, oracle, m):
    """m = 2: one projected row.  m = 8: the 2m rows of W fill one 16-row tile exactly.  m = 9: one row in a second tile."""
    prob = ts.exact_length(synth.make_problem(2, C=12, F=8, seed=31), m, patterns=("stride",))
    assert (np.diff(prob.meas_offsets) == m).all()
    ref, _, _ = _three(Updater, oracle, Case(prob, capi.REP_GLOBAL_3D))
    assert (ref["lm_cov_id"] >= 0).sum() >= 3


def test_batch_mixing_one_two_and_twelve_measurements(Updater, oracle):
    """The candidate with one measurement is skipped (OVGPU_FEAT_TOO_FEW_MEAS) and takes neither step."""
    lengths = [12, 1, 2, 12, 2, 1, 12, 2]
    prob = ts.with_lengths(synth.make_problem(2, C=12, F=8, seed=32), lengths, patterns=("stride",))
    ref, _, (_, out_c, _, _, steps_c) = _three(Updater, oracle, Case(prob, capi.REP_ANCHORED_3D))
    assert (out_c["feat_status"][np.array(lengths) == 1] == capi.FEAT_TOO_FEW_MEAS).all() and steps_c == (6, 0)
    assert (ref["lm_cov_id"] >= 0).sum() >= 3


# --------------------------------------------------------------------------- the covariance dimension at a tile edge
@pytest.mark.parametrize("edge", [-1, 0, 1])
def test_covariance_dimension_crosses_a_tile_edge(Updater, oracle, edge):
    """N at entry 16k - 1, 16k, 16k + 1 (11 clones and one camera give 96; resident landmarks of 15 dof / of 1 dof move it to 111 / 97), and six or
    more accepted candidates carry the dimension over the next multiple of 16 inside the chain."""
    tracks = synth.make_problem(2, C=11, K=1, F=12, seed=33)
    if edge == 0:
        case = Case(tracks, capi.REP_GLOBAL_3D)
    else:
        reps = np.full(5, capi.REP_GLOBAL_3D, np.int32) if edge < 0 else np.array([SINGLE], np.int32)
        case = Case(_tracks_from(synth.make_slam_problem(2, L=len(reps), lm_rep=reps, C=11, K=1, seed=33), tracks), capi.REP_GLOBAL_3D, slam=True)
    assert case.prob.N % 16 == edge % 16
    ref, _, _ = _three(Updater, oracle, case)
    assert (ref["lm_cov_id"] >= 0).sum() >= 6 and ref["N"] // 16 > case.prob.N // 16


# --------------------------------------------------------------------------- per-feature representations, sigma and multiplier
def test_per_feature_representations_sigma_and_multiplier(Updater, oracle):
    """3-dof and single-depth candidates in one chain (tests/test_gpu_mixed_reps.py), the ArUco corners with their own noise and gate
    (test_delayed_init_per_feature_options): sigma_f enters S and P_LL through the scaled rows."""
    tag = np.random.default_rng(5).random(16) < 0.4
    each = np.where(tag, SINGLE, capi.REP_GLOBAL_3D).astype(np.int32)
    case = Case(synth.make_problem(2, C=12, F=16, outlier_frac=0.2), capi.REP_GLOBAL_3D, each=each, sig=np.where(tag, 2.5, 1.0), mult=np.where(tag, 3.0, 1.0))
    ref, _, (_, _, _, lm_c, _) = _three(Updater, oracle, case)
    acc = ref["lm_cov_id"] >= 0
    assert (acc & tag).any() and (acc & ~tag).any() and np.array_equal(lm_c["feat_rep"], each[acc])
    assert ref["N"] == case.prob.N + int(np.where(each[acc] == SINGLE, 1, 3).sum())


@pytest.mark.parametrize("rep", [capi.REP_GLOBAL_3D, SINGLE])
def test_per_feature_sigma_and_multiplier(Updater, oracle, rep):
    rng = np.random.default_rng(5)
    tag = rng.random(16) < 0.4
    case = Case(synth.make_problem(2, C=12, F=16, outlier_frac=0.2), rep, sig=np.where(tag, 2.5, 1.0), mult=np.where(tag, 3.0, 1.0))
    ref, _, _ = _three(Updater, oracle, case)
    assert (ref["lm_cov_id"] >= 0).sum() >= 4


# --------------------------------------------------------------------------- resident landmarks under the empty active set
def test_resident_landmarks_follow_every_step_then_slam_update(Updater, oracle):
    """Six resident landmarks of mixed representations (anchored ones among them) without a column: their values follow every step's dx through P
    alone.  Then the same set_features + slam_update on the grown state after (b) and after (c): the follow-up's inputs agree to the delayed
    initialisation's tolerances, so its outputs are held to those (dx 1e-6, P 1e-7), the verdicts to identity."""
    each = np.array([0, 4, 5, 2, 4, 5], np.int32)
    mk = lambda: synth.make_slam_problem(2, L=6, lm_rep=each, C=12, seed=21)
    tracks = synth.make_problem(2, C=12, F=10, seed=34)
    case = Case(_tracks_from(mk(), tracks), capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, slam=True)
    ref, b, c = _three(Updater, oracle, case, keep=True)
    try:
        assert (ref["lm_cov_id"] >= 0).sum() >= 3
        assert np.abs(c[3]["value"][:6] - case.prob.lm_value).max() > 0  # they moved
        outs = []
        for up, out, post, lm, _ in (b, c):
            nxt = mk()  # the six landmarks' own tracks
            nxt.N, nxt.P, nxt.clone_q_p, nxt.calib_q_p, nxt.intrinsics = out["N"], post["P"], post["clone_q_p"], post["calib_q_p"], post["intrinsics"]
            nxt.lm_value, nxt.lm_fej, nxt.lm_cov_id = lm["value"], lm["fej"], lm["cov_id"]
            nxt.lm_anchor_cam, nxt.lm_anchor_clone, nxt.lm_rep_each = lm["anchor_cam"], lm["anchor_clone"], lm["feat_rep"]
            nxt.lm_index = np.arange(6, dtype=np.int32)
            up.set_active_landmarks(None)
            up.set_features(nxt)
            outs.append(up.slam_update(lm_index=nxt.lm_index))
        u_b, u_c = outs
        assert np.array_equal(u_b["feat_status"], u_c["feat_status"]) and (u_c["feat_status"] == capi.FEAT_USED).sum() >= 3
        print(f"follow-up (c)-(b): dx {_rel(u_c['dx'], u_b['dx']):.3e}  P {_rel(u_c['P'], u_b['P']):.3e}")
        assert _rel(u_c["dx"], u_b["dx"]) < 1e-6 and _rel(u_c["P"], u_b["P"]) < 1e-7
        np.testing.assert_allclose(u_c["landmarks"], u_b["landmarks"], rtol=1e-8, atol=1e-10)
    finally:
        b[0].close(), c[0].close()


# --------------------------------------------------------------------------- one candidate; nobody accepted
def _one_feature(outlier):
    prob = synth.make_problem(2, C=12, F=4, seed=35).subset([1])
    return ts.make_outlier(prob, 0) if outlier else prob


@pytest.mark.parametrize("outlier", [False, True])
def test_single_candidate(Updater, oracle, outlier):
    case = Case(_one_feature(outlier), capi.REP_GLOBAL_3D)
    ref, _, (_, out_c, _, _, _) = _three(Updater, oracle, case)
    assert np.isfinite(ref["chi2"][0])  # the gate was reached
    assert (ref["lm_cov_id"][0] >= 0) == (not outlier)
    if outlier:
        assert out_c["feat_status"][0] == capi.FEAT_CHI2_REJECTED and out_c["N"] == case.prob.N and np.array_equal(out_c["P"], case.prob.P)


def test_every_candidate_rejected_leaves_the_state_bit_for_bit(Updater, oracle):
    prob = synth.make_problem(2, C=12, F=5, seed=36)
    for f in range(prob.F):
        prob = ts.make_outlier(prob, f)
    case = Case(prob, capi.REP_ANCHORED_3D)
    ref, _, (_, out_c, post_c, lm_c, _) = _three(Updater, oracle, case)
    assert np.isfinite(ref["chi2"]).sum() >= 3 and not (ref["lm_cov_id"] >= 0).any()
    assert out_c["N"] == prob.N and np.array_equal(out_c["P"], prob.P) and not out_c["dx_seq"].any() and len(lm_c["cov_id"]) == 0
    assert np.array_equal(post_c["clone_q_p"], prob.clone_q_p) and np.array_equal(post_c["calib_q_p"], prob.calib_q_p)


# --------------------------------------------------------------------------- the reset baseline after the covariance shrank to its own dimension
@pytest.mark.parametrize("fused", [False, True])
def test_reset_state_returns_to_what_the_call_left(Updater, oracle, fused):
    """Four clones, one camera, one resident landmark; three candidates of three measurements, the middle one a planted outlier (tracks 2, 3, 6 of
    the window: the ones that triangulate over so short a baseline).  The chain runs at the padded dimension N + 9 and leaves N + 6: after
    ovgpu_reset_state the covariance, at that dimension and its own leading dimension, the clones, the calibration and the intrinsics read back
    bit for bit as the call returned and left them."""
    window = synth.make_problem(2, C=4, K=1, F=12, seed=32, min_obs=3)
    tracks = ts.make_outlier(ts.exact_length(window, 3, patterns=("stride",)).subset([2, 3, 6]), 1)
    case = Case(_tracks_from(synth.make_slam_problem(2, L=1, C=4, K=1, seed=32, min_obs=3), tracks), capi.REP_GLOBAL_3D, slam=True)
    tri, ref = _oracle(oracle, case)
    assert list(ref["feat_status"]) == [capi.FEAT_USED, capi.FEAT_CHI2_REJECTED, capi.FEAT_USED]
    up, out, post, lm, _ = _run(Updater, case, tri, fused)
    try:
        assert np.array_equal(out["feat_status"], ref["feat_status"]) and out["N"] == case.prob.N + 6 and len(lm["cov_id"]) == 3
        assert post["P"].shape == (out["N"], out["N"]) and np.array_equal(post["P"], out["P"])
        assert np.abs(post["clone_q_p"] - case.prob.clone_q_p).max() > 0  # the chain moved the state
        up.reset_state()
        back = up.get_state(P=True)
        for k in post:
            assert back[k].shape == post[k].shape and np.array_equal(back[k], post[k]), k
    finally:
        up.close()


# --------------------------------------------------------------------------- calibration and FEJ flags
@pytest.mark.parametrize("do_fej,K,pose,intr", [(0, 2, 1, 1), (1, 1, 0, 0), (0, 1, 1, 0), (1, 2, 0, 1)])
def test_calibration_and_fej_flags(Updater, oracle, do_fej, K, pose, intr):
    """FEJ on and off, mono, and the smallest D (both calibration flags off: the clones' columns only)."""
    opts = capi.default_options(chi2_multipler=1.0, do_fej=do_fej, do_calib_camera_pose=pose, do_calib_camera_intrinsics=intr)
    case = Case(synth.make_problem(2, C=10, K=K, F=10, seed=42), capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, opts=opts)
    ref, _, (_, out_c, _, _, _) = _three(Updater, oracle, case)
    assert (ref["lm_cov_id"] >= 0).sum() >= 4 and out_c["stats"]["D"] == 6 * 10 + K * (6 * pose + 8 * intr)


# --------------------------------------------------------------------------- a track beyond the fused step's bound
def test_track_beyond_the_bound_takes_the_chain_step_in_place(Updater, oracle):
    """m = 65, the smallest track above the bound, between shorter ones: 33 stereo clones are the fewest that observe a point 65 times.  That
    candidate alone takes the chain's step, where it stands, and the chain goes on."""
    prob = synth.make_problem(2, C=33, K=2, F=8, seed=50)
    prob = prob.subset(np.flatnonzero(np.diff(prob.meas_offsets) > M_MAX)[:4])
    assert prob.F == 4
    lengths = [10, M_MAX + 1, 12, 9]
    prob = ts.with_lengths(prob, lengths, patterns=("stride",))
    assert np.diff(prob.meas_offsets).tolist() == lengths
    ref, _, _ = _three(Updater, oracle, Case(prob, capi.REP_GLOBAL_3D), want_steps=(3, 1))
    acc = ref["lm_cov_id"] >= 0
    assert acc[1] and acc[2:].any()  # the long one is accepted, and so is a candidate behind it


def test_switch_off_reproduces_the_existing_entry_bit_for_bit(Updater, oracle):
    case = Case(synth.make_problem(2, C=12, F=16, outlier_frac=0.2), capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH)
    tri, ref = _oracle(oracle, case)
    up_b, out_b, post_b, lm_b, _ = _run(Updater, case, tri, fused=False)
    up_c, out_c, post_c, lm_c, steps_c = _run(Updater, case, tri, fused=True, debug={"delayed_init_fused": 0})
    try:
        assert up_c.debug_option("delayed_init_fused") == 0 and up_b.debug_option("delayed_init_fused") == 1
        assert (ref["lm_cov_id"] >= 0).sum() >= 4 and steps_c == (0, 16)
        for k in ("feat_status", "chi2", "chi2_thresh", "lm_cov_id", "lm_value", "lm_fej", "anchor_cam", "anchor_clone", "dx_seq", "P"):
            assert np.array_equal(out_b[k], out_c[k], equal_nan=out_b[k].dtype.kind == "f"), k
        assert out_b["N"] == out_c["N"]
        for k in ("P", "clone_q_p", "calib_q_p", "intrinsics"):
            assert np.array_equal(post_b[k], post_c[k]), k
        for k in lm_b:
            assert np.array_equal(lm_b[k], lm_c[k]), k
    finally:
        up_b.close(), up_c.close()


# --------------------------------------------------------------------------- random shapes
# Seeds at which the oracle finds every gated candidate further than GATE_MARGIN from its threshold (chosen on the CPU; _oracle asserts it again).
RANDOM_SEEDS = [0, 2, 5, 7, 9, 10, 12, 14]  # (5: nothing triangulates, nothing is gated, nothing changes)


def _random_case(seed):
    rng = np.random.default_rng(4100 + seed)
    kw = dict(C=int(rng.integers(6, 13)), K=int(rng.integers(1, 4)), F=int(rng.integers(1, 21)), track=("full", "ragged")[int(rng.integers(2))],
              fisheye=bool(rng.integers(2)), seed=int(rng.integers(1 << 20)), outlier_frac=float(rng.choice([0.0, 0.3])))
    rep = int(rng.integers(0, 6))
    opts = capi.default_options(chi2_multipler=float(rng.choice([1.0, 5.0])), do_fej=int(rng.integers(2)),
                                do_calib_camera_pose=int(rng.integers(2)), do_calib_camera_intrinsics=int(rng.integers(2)))
    return Case(synth.make_problem(2, **kw), rep, opts=opts)


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_shapes(Updater, oracle, seed):
    _three(Updater, oracle, _random_case(seed))
