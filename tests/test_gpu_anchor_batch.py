"""GPU tests (`-m gpu`) of the batched anchor change (ABI 10): ovgpu_slam_change_anchors_batched — every landmark anchored in the clone that
leaves moves in a fixed number of launches (k_anchor_change_all, k_cov_propagate_multi) — and its mode-A export
ovgpu_slam_anchor_systems(_len).

The reference moves the landmarks one after the other (UpdaterSLAM.cpp:492-502), each Phi computed after the previous propagation — but from
state values only, so the sequence is one joint propagation.  The oracle (oracle.anchor_change, pinned to the reference in
tests/test_ref_build.py) is chained landmark by landmark as tests/test_gpu_parity.py::test_change_anchors_parity_then_marginalize and
tests/test_gpu_active_landmarks.py::test_change_anchors_with_120_landmarks chain it; the problems come from the generators those two use and
the tolerances are theirs: values and first estimates rtol 1e-12 / atol 1e-13, P' 1e-12 in relative Frobenius norm, a SLAM update behind the
change 1e-7 (dx) / 1e-8 (P').  Mode A is replayed through a numpy restatement of StateHelper::EKFPropagation (StateHelper.cpp:36-114)."""
import copy
import ctypes as C

import numpy as np
import pytest

from open_vins_amd import capi, synth

pytestmark = pytest.mark.gpu

ANCHORED = [capi.REP_ANCHORED_3D, capi.REP_ANCHORED_FULL_INVERSE_DEPTH, capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE]
MIXED = np.array([4, 0, 5, 2, 1, 3, 4, 0, 5, 2], np.int32)  # tests/test_gpu_mixed_reps.py: global landmarks and the single depth among the anchored


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _reps_of(prob, L):
    return np.asarray(prob.lm_rep_each) if prob.lm_rep_each is not None else np.full(L, prob.lm_rep, np.int32)


def _moving(prob):
    L = len(prob.lm_cov_id)
    return np.flatnonzero((prob.lm_anchor_clone == 0) & (_reps_of(prob, L) >= capi.REP_ANCHORED_3D))


def oracle_chain(oracle, opts, prob, moved):
    """the oracle, landmark by landmark in landmark order, each on the covariance the previous one left (the reference's sequence)"""
    ref = copy.deepcopy(prob)
    for l in moved:
        o = oracle.anchor_change(opts, capi.Views(ref), int(l), int(ref.lm_anchor_cam[l]), ref.C - 1)
        assert o["rc"] == 0
        ref.P, ref.lm_value[l], ref.lm_fej[l], ref.lm_anchor_clone[l] = o["P"], o["value"], o["fej"], ref.C - 1
    return ref


def check_against(lm, P, ref, what):
    """the assertions of the two existing change_anchors tests, and exact symmetry"""
    print(f"{what}: P' {_rel(P, ref.P):.3e} (relative Frobenius)  values {np.abs(lm['value'] - ref.lm_value).max():.3e}  "
          f"first estimates {np.abs(lm['fej'] - ref.lm_fej).max():.3e} (max abs)")
    np.testing.assert_allclose(lm["value"], ref.lm_value, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(lm["fej"], ref.lm_fej, rtol=1e-12, atol=1e-13)
    anchored = ref.lm_anchor_clone >= 0
    np.testing.assert_array_equal(lm["anchor_clone"][anchored], ref.lm_anchor_clone[anchored])
    np.testing.assert_array_equal(lm["anchor_cam"][anchored], ref.lm_anchor_cam[anchored])
    assert _rel(P, ref.P) < 1e-12
    assert np.array_equal(P, P.T)


def ekf_propagation(P, new_id, lsz, order_old, Phi):
    """StateHelper::EKFPropagation (StateHelper.cpp:36-114) with Q = 0 and one new variable: order_old [(covariance id, size)]"""
    Cov_PhiT = np.zeros((P.shape[0], lsz))
    at = 0
    for vid, size in order_old:  # :78-85
        Cov_PhiT += P[:, vid:vid + size] @ Phi[:, at:at + size].T
        at += size
    assert at == Phi.shape[1] and Phi.shape[0] == lsz  # :65-66
    Phi_Cov_PhiT = np.zeros((lsz, lsz))
    at = 0
    for vid, size in order_old:  # :88-92
        Phi_Cov_PhiT += Phi[:, at:at + size] @ Cov_PhiT[vid:vid + size, :]
        at += size
    P = P.copy()
    P[new_id:new_id + lsz, :] = Cov_PhiT.T  # :98-100
    P[:, new_id:new_id + lsz] = Cov_PhiT
    P[new_id:new_id + lsz, new_id:new_id + lsz] = Phi_Cov_PhiT
    assert (np.diag(P) >= 0.0).all()  # :103-113
    return P


def replay_mode_a(prob, systems):
    """what the mode-A body of UpdaterSLAM::change_anchors does with the export: the stock EKFPropagation landmark after landmark, then the landmark"""
    out = copy.deepcopy(prob)
    for s in systems:
        l = s["lm_index"]
        out.P = ekf_propagation(out.P, s["cov_id"], s["lsz"], s["phi_order"], s["Phi"])
        out.lm_value[l], out.lm_fej[l] = s["value"], s["fej"]
        out.lm_anchor_cam[l], out.lm_anchor_clone[l] = s["anchor_cam"], s["anchor_clone"]
    return out


def expected_phi_order(prob, opts, l, new_clone):
    """the reference's phi_order_OLD (UpdaterSLAM.cpp:587-607): x_order_old (anchor clone, its camera's extrinsics if estimated), what x_order_new
    adds (the new clone; the extrinsics again only for another camera — change_anchors keeps the camera), the landmark"""
    cam = int(prob.lm_anchor_cam[l])
    order = [(int(prob.clone_cov_id[prob.lm_anchor_clone[l]]), 6)]
    if opts.do_calib_camera_pose:
        order.append((int(prob.calib_cov_id[cam]), 6))
    order.append((int(prob.clone_cov_id[new_clone]), 6))
    order.append((int(prob.lm_cov_id[l]), 1 if _reps_of(prob, len(prob.lm_cov_id))[l] == capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE else 3))
    return order


def reanchor(prob, l, cam, clone):
    """landmark l of the generator's state re-expressed in camera `cam` of clone `clone`, value and first estimate alike (the same point)"""
    rep = int(_reps_of(prob, len(prob.lm_cov_id))[l])
    qa, qn = prob.clone_q_p[prob.lm_anchor_clone[l]], prob.clone_q_p[clone]
    qk, qm = prob.calib_q_p[prob.lm_anchor_cam[l]], prob.calib_q_p[cam]
    R_a, R_n, R_k, R_m = synth.quat_2_rot(qa[:4]), synth.quat_2_rot(qn[:4]), synth.quat_2_rot(qk[:4]), synth.quat_2_rot(qm[:4])
    for arr in (prob.lm_value, prob.lm_fej):
        pA = synth.landmark_to_xyz(rep, arr[l:l + 1])[0]
        pG = R_a.T @ (R_k.T @ (pA - qk[4:7])) + qa[4:7]
        arr[l] = synth.landmark_from_xyz(rep, (R_m @ (R_n @ (pG - qn[4:7])) + qm[4:7])[None, :])[0]
    prob.lm_anchor_cam[l], prob.lm_anchor_clone[l] = cam, clone


def two_camera_problem(rep):
    """synth.make_slam_problem(2, L=10) as the two existing tests use it; its tracks all start in one camera of the stereo pair, so every second
    landmark anchored in clone 0 is re-expressed in the other one: both cameras anchor landmarks that move"""
    prob = synth.make_slam_problem(2, L=10, lm_rep=rep)
    for l in _moving(prob)[::2]:
        reanchor(prob, l, 1 - int(prob.lm_anchor_cam[l]), 0)
    assert set(int(c) for c in prob.lm_anchor_cam[_moving(prob)]) == {0, 1}
    return prob


def all_in_clone_0(L, seed):
    """L anchored landmarks of the four anchored representations, every one anchored in clone 0 (30 clones, stereo, online calibration), in
    the two cameras alternately"""
    reps = np.array((ANCHORED * ((L + 3) // 4))[:L], np.int32)
    prob = synth.make_slam_problem(2, L=L, lm_rep=reps, seed=seed)
    for l in range(L):
        reanchor(prob, l, (l // 4) % 2, 0)
    return prob


def shifted_window(prob, post, lm2, make):
    """the batch on the window without its oldest clone (tests/test_gpu_parity.py::test_change_anchors_parity_then_marginalize)"""
    keep = prob.clone_idx > 0
    cnt = np.add.reduceat(keep.astype(np.int64), prob.meas_offsets[:-1])
    win = make()
    win.C, win.N = prob.C - 1, prob.N - 6
    win.meas_offsets = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    win.uv, win.uvn = prob.uv.reshape(-1, 2)[keep].reshape(-1), prob.uvn.reshape(-1, 2)[keep].reshape(-1)
    win.clone_idx, win.cam_idx = (prob.clone_idx[keep] - 1).astype(np.int32), prob.cam_idx[keep]
    win.P, win.clone_q_p, win.clone_q_p_fej = post["P"], post["clone_q_p"], prob.clone_q_p_fej[1:]
    win.clone_cov_id = prob.clone_cov_id[:-1]
    win.lm_value, win.lm_fej, win.lm_cov_id = lm2["value"], lm2["fej"], lm2["cov_id"]
    win.lm_anchor_cam, win.lm_anchor_clone = lm2["anchor_cam"], lm2["anchor_clone"]
    return win


CASES = [(rep, {}) for rep in ANCHORED] + [(MIXED, {}), (MIXED, dict(do_calib_camera_pose=0)), (capi.REP_ANCHORED_3D, dict(do_calib_camera_pose=0))]


# --------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("rep,flags", CASES, ids=lambda v: "mixed" if isinstance(v, np.ndarray) else ("fixed-extrinsics" if v else "estimated") if isinstance(v, dict) else f"rep{v}")
def test_batched_against_the_oracle_then_marginalize(Updater, oracle, rep, flags):
    """The four anchored representations, a mixed state with global landmarks and the single depth, estimated and fixed extrinsics; both
    cameras of the stereo pair anchor landmarks.  Then the old clone can be marginalised."""
    prob = two_camera_problem(rep)
    moved = _moving(prob)
    assert len(moved) >= 2
    opts = capi.default_options(chi2_multipler=1.0, **flags)
    up = Updater(opts)
    up.set_slam_problem(prob)
    assert up.change_anchors_batched(0, prob.C - 1) == len(moved)
    ref = oracle_chain(oracle, opts, prob, moved)
    check_against(up.get_landmarks(), up.get_state(P=True)["P"], ref, f"batched vs oracle, {len(moved)} moved")
    up.state_marginalize(int(prob.clone_cov_id[0]), 6)
    assert np.array_equal(up.get_landmarks()["anchor_clone"][ref.lm_anchor_clone >= 0], ref.lm_anchor_clone[ref.lm_anchor_clone >= 0] - 1)
    up.close()


# --------------------------------------------------------------------------- 2. every landmark at once
def test_fifty_landmarks_all_anchored_in_the_clone_that_leaves(Updater, oracle):
    prob = all_in_clone_0(50, seed=11)
    assert prob.C == 30 and prob.K == 2 and len(_moving(prob)) == 50
    opts = capi.default_options(chi2_multipler=1.0)
    up = Updater(opts)
    up.set_slam_problem(prob)
    up.set_active_landmarks([])
    assert up.change_anchors_batched(0, prob.C - 1) == 50
    ref = oracle_chain(oracle, opts, prob, np.arange(50))
    check_against(up.get_landmarks(), up.get_state(P=True)["P"], ref, "batched vs oracle, 50 of 50 moved")
    up.state_marginalize(int(prob.clone_cov_id[0]), 6)
    up.close()


# --------------------------------------------------------------------------- 3. against the sequential entry
@pytest.mark.parametrize("which", ["mixed10", "all50"])
def test_batched_against_the_sequential_entry(Updater, which):
    """Same inputs, two contexts.  The joint propagation sums in another order than the chain: no bit-identity, the oracle's tolerance."""
    prob = synth.make_slam_problem(2, L=10, lm_rep=MIXED) if which == "mixed10" else all_in_clone_0(50, seed=11)
    opts = capi.default_options(chi2_multipler=1.0)
    a, b = Updater(opts), Updater(opts)
    a.set_slam_problem(prob), b.set_slam_problem(prob)
    n = a.change_anchors(0, prob.C - 1)
    assert b.change_anchors_batched(0, prob.C - 1) == n == len(_moving(prob))
    Pa, Pb, la, lb = a.get_state(P=True)["P"], b.get_state(P=True)["P"], a.get_landmarks(), b.get_landmarks()
    print(f"batched vs sequential ({which}, {n} moved): P' {_rel(Pb, Pa):.3e} (relative Frobenius)  values {np.abs(lb['value'] - la['value']).max():.3e}  "
          f"first estimates {np.abs(lb['fej'] - la['fej']).max():.3e} (max abs)")
    assert _rel(Pb, Pa) < 1e-12 and np.array_equal(Pb, Pb.T)
    np.testing.assert_allclose(lb["value"], la["value"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(lb["fej"], la["fej"], rtol=1e-12, atol=1e-13)
    np.testing.assert_array_equal(lb["anchor_clone"], la["anchor_clone"])
    np.testing.assert_array_equal(lb["anchor_cam"], la["anchor_cam"])
    a.close(), b.close()


# --------------------------------------------------------------------------- 4. mode A
@pytest.mark.parametrize("rep,flags", CASES, ids=lambda v: "mixed" if isinstance(v, np.ndarray) else ("fixed-extrinsics" if v else "estimated") if isinstance(v, dict) else f"rep{v}")
def test_mode_a_export_replayed_through_ekf_propagation(Updater, oracle, rep, flags):
    prob = two_camera_problem(rep)
    moved = _moving(prob)
    opts = capi.default_options(chi2_multipler=1.0, **flags)
    up = Updater(opts)
    up.set_slam_problem(prob)
    st0, lm0 = up.get_state(P=True), up.get_landmarks()
    systems = up.anchor_systems(0, prob.C - 1)
    st1, lm1 = up.get_state(P=True), up.get_landmarks()
    for k in st0:  # the resident state is left exactly as it was
        assert np.array_equal(st0[k], st1[k]), k
    for k in lm0:
        assert np.array_equal(lm0[k], lm1[k]), k
    assert [s["lm_index"] for s in systems] == list(moved)
    reps = _reps_of(prob, 10)
    for s in systems:
        l = s["lm_index"]
        assert s["phi_order"] == expected_phi_order(prob, opts, l, prob.C - 1)
        assert s["cov_id"] == prob.lm_cov_id[l] and s["feat_rep"] == reps[l] and s["lsz"] == (1 if reps[l] == 5 else 3)
        assert s["anchor_cam"] == prob.lm_anchor_cam[l] and s["anchor_clone"] == prob.C - 1
        assert s["Phi"].shape == (s["lsz"], sum(sz for _, sz in s["phi_order"]))
    got = replay_mode_a(prob, systems)
    ref = oracle_chain(oracle, opts, prob, moved)
    Pg = got.P
    print(f"mode A replay vs oracle: P' {_rel(Pg, ref.P):.3e}")
    np.testing.assert_allclose(got.lm_value, ref.lm_value, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(got.lm_fej, ref.lm_fej, rtol=1e-12, atol=1e-13)
    np.testing.assert_array_equal(got.lm_anchor_clone, ref.lm_anchor_clone)
    assert _rel(Pg, ref.P) < 1e-12
    # ... and against the batched mode-B result on the same context
    assert up.change_anchors_batched(0, prob.C - 1) == len(moved)
    Pb, lb = up.get_state(P=True)["P"], up.get_landmarks()
    print(f"mode A replay vs batched mode B: P' {_rel(Pg, Pb):.3e}")
    assert _rel(Pg, Pb) < 1e-12
    np.testing.assert_allclose(got.lm_value, lb["value"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(got.lm_fej, lb["fej"], rtol=1e-12, atol=1e-13)
    up.close()


def test_mode_a_len_and_capacity(Updater):
    prob = synth.make_slam_problem(2, L=10, lm_rep=MIXED)
    moved = _moving(prob)
    up = Updater(capi.default_options(chi2_multipler=1.0))
    up.set_slam_problem(prob)
    sz = capi.AnchorSizes()
    assert up.lib.ovgpu_slam_anchor_systems_len(up._ctx, 0, prob.C - 1, C.byref(sz)) == capi.OK
    systems = up.anchor_systems(0, prob.C - 1)
    assert sz.n_sys == len(moved) == len(systems)
    assert sz.n_vars == sum(len(s["phi_order"]) for s in systems) and sz.n_phi == sum(s["Phi"].size for s in systems)
    n = int(sz.n_sys)
    sys_ = (capi.AnchorSystem * n)()
    vid, vsz, Phi, val, fej = np.zeros(sz.n_vars, np.int32), np.zeros(sz.n_vars, np.int32), np.zeros(sz.n_phi), np.zeros(3 * n), np.zeros(3 * n)
    ip, dp = (lambda a: a.ctypes.data_as(capi.c_int32_p)), (lambda a: a.ctypes.data_as(capi.c_double_p))
    for field in ("n_sys", "n_vars", "n_phi"):
        small = capi.AnchorSizes(sz.n_sys, sz.n_vars, sz.n_phi)
        setattr(small, field, getattr(sz, field) - 1)
        rc = up.lib.ovgpu_slam_anchor_systems(up._ctx, 0, prob.C - 1, C.byref(small), sys_, ip(vid), ip(vsz), dp(Phi), dp(val), dp(fej))
        assert rc == capi.ERR_CAPACITY, field
    assert not Phi.any() and not val.any()  # nothing was written
    assert up.lib.ovgpu_slam_anchor_systems(up._ctx, 0, prob.C - 1, C.byref(sz), sys_, ip(vid), ip(vsz), dp(Phi), dp(val), dp(fej)) == capi.OK
    assert sys_[n - 1].phi_off + sys_[n - 1].lsz * sys_[n - 1].n_old == sz.n_phi and sys_[n - 1].var_off + sys_[n - 1].n_vars == sz.n_vars
    up.close()


# --------------------------------------------------------------------------- 5. edges
def test_edges(Updater):
    opts = capi.default_options(chi2_multipler=1.0)
    up = Updater(opts)
    n = C.c_int32(5)
    sz = capi.AnchorSizes(1, 1, 1)
    # before any state: what the sequential entry says
    assert up.lib.ovgpu_slam_change_anchors(up._ctx, 0, 1, C.byref(n)) == capi.ERR_NO_STATE
    assert up.lib.ovgpu_slam_change_anchors_batched(up._ctx, 0, 1, C.byref(n)) == capi.ERR_NO_STATE and n.value == 0
    assert up.lib.ovgpu_slam_anchor_systems_len(up._ctx, 0, 1, C.byref(sz)) == capi.ERR_NO_STATE
    # a state without landmarks, and one whose landmarks are all global: 0 moved, nothing launched, the state untouched (:493-496)
    plain = synth.make_problem(2, F=8)
    up.set_problem(plain)
    for fn in (up.lib.ovgpu_slam_change_anchors, up.lib.ovgpu_slam_change_anchors_batched):
        n.value = 5
        assert fn(up._ctx, 0, plain.C - 1, C.byref(n)) == capi.OK and n.value == 0
    glob = synth.make_slam_problem(2, L=5)
    up.set_slam_problem(glob)
    assert up.change_anchors_batched(0, glob.C - 1) == 0 and up.anchor_systems(0, glob.C - 1) == []
    assert up.lib.ovgpu_slam_anchor_systems_len(up._ctx, 0, glob.C - 1, C.byref(sz)) == capi.OK and (sz.n_sys, sz.n_vars, sz.n_phi) == (0, 0, 0)
    assert np.array_equal(up.get_state(P=True)["P"], glob.P) and np.array_equal(up.get_landmarks()["value"], glob.lm_value)
    # anchored landmarks, none of them in the clone asked for
    prob = synth.make_slam_problem(2, L=10, lm_rep=MIXED)
    free = int(np.setdiff1d(np.arange(1, prob.C - 1), prob.lm_anchor_clone)[0])
    up.set_slam_problem(prob)
    assert up.change_anchors_batched(free, prob.C - 1) == 0 and up.anchor_systems(free, prob.C - 1) == []
    assert np.array_equal(up.get_state(P=True)["P"], prob.P) and np.array_equal(up.get_landmarks()["value"], prob.lm_value)
    # bad clones
    for marg, new in ((0, 0), (-1, 3), (0, prob.C), (prob.C, 0)):
        assert up.lib.ovgpu_slam_change_anchors(up._ctx, marg, new, C.byref(n)) == capi.ERR_INVALID
        assert up.lib.ovgpu_slam_change_anchors_batched(up._ctx, marg, new, C.byref(n)) == capi.ERR_INVALID
        assert up.lib.ovgpu_slam_anchor_systems_len(up._ctx, marg, new, C.byref(sz)) == capi.ERR_INVALID
    assert np.array_equal(up.get_state(P=True)["P"], prob.P)
    up.close()


def test_active_landmark_set_does_not_change_the_result(Updater):
    """perform_anchor_change reads no column table: no set, the empty set and the moving landmarks give the same bits"""
    prob = synth.make_slam_problem(2, L=10, lm_rep=MIXED)
    moved = _moving(prob)
    opts = capi.default_options(chi2_multipler=1.0)
    outs = []
    for active in (None, [], moved):
        up = Updater(opts)
        up.set_slam_problem(prob)
        if active is not None:
            up.set_active_landmarks(active)
        sysm = up.anchor_systems(0, prob.C - 1)
        assert up.change_anchors_batched(0, prob.C - 1) == len(moved)
        outs.append((up.get_state(P=True)["P"], up.get_landmarks(), sysm))
        up.close()
    for P, lm, sysm in outs[1:]:
        assert np.array_equal(P, outs[0][0])
        for k in lm:
            assert np.array_equal(lm[k], outs[0][1][k]), k
        for s, s0 in zip(sysm, outs[0][2]):
            assert np.array_equal(s["Phi"], s0["Phi"]) and s["phi_order"] == s0["phi_order"] and np.array_equal(s["value"], s0["value"])


@pytest.mark.parametrize("rep", [capi.REP_ANCHORED_3D, capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE])
def test_slam_update_after_the_batched_change_equals_one_after_the_sequential(Updater, rep):
    make = lambda: synth.make_slam_problem(2, L=10, lm_rep=rep)
    prob = make()
    opts = capi.default_options(chi2_multipler=1.0)
    outs = []
    for batched in (False, True):
        up = Updater(opts)
        up.set_slam_problem(prob)
        n = up.change_anchors_batched(0, prob.C - 1) if batched else up.change_anchors(0, prob.C - 1)
        assert n == len(_moving(prob)) >= 3
        up.state_marginalize(int(prob.clone_cov_id[0]), 6)
        win = shifted_window(prob, up.get_state(P=True), up.get_landmarks(), make)
        up.set_features(win)
        outs.append(up.slam_update(lm_index=win.lm_index))
        up.close()
    s, b = outs
    print(f"update after batched vs after sequential: dx {_rel(b['dx'], s['dx']):.3e}  P {_rel(b['P'], s['P']):.3e}")
    assert np.array_equal(b["feat_status"], s["feat_status"]) and (s["feat_status"] == capi.FEAT_USED).sum() >= 5
    assert _rel(b["dx"], s["dx"]) < 1e-7 and _rel(b["P"], s["P"]) < 1e-8
    np.testing.assert_allclose(b["landmarks"], s["landmarks"], rtol=1e-9, atol=1e-11)
