"""GPU tests (`-m gpu`) of the window entries — ovgpu_state_propagate, ovgpu_state_augment_clone, ovgpu_state_marginal_covariance,
ovgpu_state_marginalize (k_cov_propagate, k_cov_clone, k_cov_dt, k_cov_gather, k_cov_remove, k_cov_copy of csrc/k_slam.h) — at the shapes of
tests/window_edge_shapes.py, every one on a state that has landmarks BETWEEN its clones (window_order's `steady` order), against
pyoracle.propagate / augment_clone / marginalize and plain numpy indexing.

Bounds: 1e-14 in relative Frobenius norm where arithmetic happens (the propagation, the time-offset Jacobian of augment_clone: the bound of
tests/test_gpu_parity.py::test_state_propagate_clone_marginalize_parity, whose one shape these cases widen), bit equality where the call is a copy
(the clone's rows and columns, the marginal covariance, the marginalisation).  The updates behind a marginalisation are held to
tests/test_gpu_parity.py::test_msckf_update_with_resident_landmarks (dx 1e-7, P' 1e-8).
"""
import copy

import numpy as np
import pytest

import window_edge_shapes as we
import window_order as wo
from open_vins_amd import capi, synth

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def note(entry, what, v):
    print(f"{what}: {v:.3e}")
    WORST[entry] = max(WORST.get(entry, 0.0), float(v))


def resident(Updater, p):
    up = Updater(capi.default_options(chi2_multipler=1.0))
    up.set_slam_state(p)
    return up


def landmarks_untouched(up, p):
    lm = up.get_landmarks()
    assert np.array_equal(lm["value"], p.lm_value) and np.array_equal(lm["fej"], p.lm_fej) and np.array_equal(lm["cov_id"], p.lm_cov_id)


# --------------------------------------------------------------------------- ovgpu_state_propagate
@pytest.mark.parametrize("cid", [c.id for c in we.PROPAGATE])
def test_propagate(Updater, oracle, cid):
    case = we.PROPAGATE_BY_ID[cid]
    p = case.prob
    rc, ref = oracle.propagate(p.P, case.new_id, case.old_ids, case.Phi, case.Q)
    assert rc == 0
    up = resident(Updater, p)
    up.state_propagate(case.new_id, case.old_ids, case.Phi, case.Q)
    P1 = up.get_state(P=True)["P"]
    landmarks_untouched(up, p)
    up.close()
    note("ovgpu_state_propagate", f"{cid} ({case.n_new} x {case.old_ids.size}, N {p.N})", _rel(P1, ref))
    assert _rel(P1, ref) < 1e-14
    assert _rel(P1, we.numpy_propagate(p.P, case.new_id, case.old_ids, case.Phi, case.Q)) < 1e-14
    # what the call does not own stays bit for bit, and the result is symmetric bit for bit
    out = np.setdiff1d(np.arange(p.N), np.arange(case.new_id, case.new_id + case.n_new))
    assert np.array_equal(P1[np.ix_(out, out)], p.P[np.ix_(out, out)]) and np.array_equal(P1[out][:, case.new_id:case.new_id + case.n_new],
                                                                                         P1[case.new_id:case.new_id + case.n_new][:, out].T)


def test_propagate_reports_a_negative_diagonal_outside_the_block(Updater, oracle):
    """ovgpu_set_state accepts a covariance with a negative diagonal entry; the reference's EKFPropagation scans the WHOLE diagonal
    (StateHelper.cpp:101-113), the oracle does, and so does the call: OVGPU_ERR_NEGATIVE_DIAGONAL, the covariance written as the oracle's."""
    p, case, j = we.negative_outside()
    assert not (case.new_id <= j < case.new_id + case.n_new)
    rc_ref, ref = oracle.propagate(p.P, case.new_id, case.old_ids, case.Phi, case.Q)
    assert rc_ref == capi.ERR_NEGATIVE_DIAGONAL and (np.diag(ref)[case.new_id:case.new_id + case.n_new] > 0).all()
    up = resident(Updater, p)
    ids, Phi, Q = np.ascontiguousarray(case.old_ids, dtype=np.int32), np.ascontiguousarray(case.Phi), np.ascontiguousarray(case.Q)
    rc = up.lib.ovgpu_state_propagate(up._ctx, case.new_id, case.n_new, ids.size, ids.ctypes.data_as(capi.c_int32_p), Phi.ctypes.data_as(capi.c_double_p),
                                      Q.ctypes.data_as(capi.c_double_p))
    P1 = up.get_state(P=True)["P"]
    up.close()
    assert rc == capi.ERR_NEGATIVE_DIAGONAL
    assert _rel(P1, ref) < 1e-14 and P1[j, j] == p.P[j, j]


# --------------------------------------------------------------------------- ovgpu_state_augment_clone
@pytest.mark.parametrize("cid", [c.id for c in we.AUGMENT])
def test_augment_clone(Updater, oracle, cid):
    case = we.AUGMENT_BY_ID[cid]
    p = case.prob
    rng = we.rng_of(cid)
    up = resident(Updater, p)
    P, clones, fej = p.P, p.clone_q_p, p.clone_q_p_fej
    src = case.src_id(p)
    for k in range(case.times):
        dnc = rng.normal(size=6) if case.dt else None
        q, qf = synth.boxplus_pose(clones[-1], 0.01 * rng.normal(size=6)), synth.boxplus_pose(fej[-1], 0.01 * rng.normal(size=6))
        N = P.shape[0]
        nid = up.state_augment_clone(src, q, qf, dt_cov_id=15 if case.dt else -1, dnc_dt=dnc)
        ref = oracle.augment_clone(P, src, 6, dt_id=15 if case.dt else -1, dnc_dt=dnc)
        st = up.get_state(P=True)
        assert nid == N and up.N == N + 6 and up.Cn == clones.shape[0] + 1
        note("ovgpu_state_augment_clone", f"{cid} clone {k} (N {N} -> {N + 6})", _rel(st["P"], ref))
        if case.dt:
            assert _rel(st["P"], ref) < 1e-14
            assert np.array_equal(st["P"][:N, :N], P)  # the time-offset Jacobian touches the new rows and columns only
        else:
            assert np.array_equal(st["P"], ref)  # a copy
            assert np.array_equal(st["P"][N:, N:], P[src:src + 6, src:src + 6]) and np.array_equal(st["P"][:N, N:], P[:, src:src + 6])
        clones, fej = np.vstack([clones, q[None]]), np.vstack([fej, qf[None]])
        assert np.array_equal(st["clone_q_p"], clones)
        P = st["P"]
    landmarks_untouched(up, p)
    # the first estimates arrived too: the MSCKF update on the grown window matches the oracle (the new clones unobserved)
    msckf, plain = wo.msckf_on(p)
    for x in (msckf, plain):
        x.N, x.C, x.P, x.clone_q_p, x.clone_q_p_fej = P.shape[0], clones.shape[0], P, clones, fej
        x.clone_cov_id = np.concatenate([p.clone_cov_id, p.N + 6 * np.arange(case.times)]).astype(np.int32)
    opts = capi.default_options(chi2_multipler=1.0)
    ref_u = oracle.msckf_update(opts, capi.Views(plain))
    up.set_features(msckf)
    out = up.update()
    up.close()
    assert np.array_equal(out["feat_status"], ref_u["feat_status"]) and (ref_u["feat_status"] == capi.FEAT_USED).sum() >= 10
    assert _rel(out["dx"], ref_u["dx"]) < 1e-7 and _rel(out["P"], ref_u["P"]) < 1e-8


# --------------------------------------------------------------------------- ovgpu_state_marginal_covariance
def test_marginal_covariance(Updater):
    p = we.state_of_dimension(127)
    up = resident(Updater, p)
    for name in we.MARGINAL:
        idx = we.marginal_indices(name, p.N)
        out = up.marginal_covariance(idx)
        assert out.shape == (idx.size, idx.size) and np.array_equal(out, p.P[np.ix_(idx, idx)]), name  # a gather: bit for bit
    for bad in (np.zeros(0, np.int32), np.zeros(1025, np.int32), np.array([0, p.N], np.int32), np.array([-1], np.int32)):
        out = np.zeros((max(bad.size, 1), max(bad.size, 1)))
        rc = up.lib.ovgpu_state_marginal_covariance(up._ctx, int(bad.size), bad.ctypes.data_as(capi.c_int32_p), out.ctypes.data_as(capi.c_double_p))
        assert rc == capi.ERR_INVALID and not out.any(), bad.size
    assert np.array_equal(up.get_state(P=True)["P"], p.P)
    up.close()


# --------------------------------------------------------------------------- ovgpu_state_marginalize
@pytest.mark.parametrize("name", we.MARGINALIZE)
def test_marginalize(Updater, oracle, name):
    p = we.state_of_dimension(127)
    cov_id, size = we.marginalize_block(name, p)
    msckf, plain = wo.msckf_on(p)
    exp = we.after_block(msckf, cov_id, size)
    up = resident(Updater, p)
    up.state_marginalize(cov_id, size)
    st, lm = up.get_state(P=True), up.get_landmarks()
    assert up.N == p.N - size == exp.N and up.Cn == exp.C
    assert np.array_equal(st["P"], oracle.marginalize(p.P, cov_id, size)) and np.array_equal(st["P"], exp.P)  # pure data movement
    assert np.array_equal(lm["cov_id"], exp.lm_cov_id) and np.array_equal(lm["value"], exp.lm_value) and np.array_equal(lm["fej"], exp.lm_fej)
    assert np.array_equal(st["clone_q_p"], exp.clone_q_p)
    # ---- the MSCKF update behind it: the oracle on the landmark-free twin with the shifted ids (a calibration block that left: its id at -1)
    twin = copy.copy(plain)
    twin.N, twin.P = exp.N, exp.P
    twin.clone_cov_id, twin.calib_cov_id, twin.intr_cov_id = exp.clone_cov_id, exp.calib_cov_id, exp.intr_cov_id
    if name in ("extrinsics", "intrinsics"):
        assert (np.concatenate([twin.calib_cov_id, twin.intr_cov_id]) == -1).sum() == 1
    opts = capi.default_options(chi2_multipler=1.0)
    ref = oracle.msckf_update(opts, capi.Views(twin))
    up.set_active_landmarks([])  # no landmark has a column: the column map is the twin's
    up.set_features(exp)
    out = up.update()
    up.close()
    note("ovgpu_msckf_update behind ovgpu_state_marginalize", f"{name}: dx", _rel(out["dx"], ref["dx"]))
    assert out["stats"]["D"] == ref["D"] == 28 + 6 * p.C - (size if name in ("extrinsics", "intrinsics") else 0)
    assert np.array_equal(out["feat_status"], ref["feat_status"]) and (ref["feat_status"] == capi.FEAT_USED).sum() >= 10
    assert _rel(out["dx"], ref["dx"]) < 1e-7 and _rel(out["P"], ref["P"]) < 1e-8


def test_zz_worst_deviations():
    for entry, v in sorted(WORST.items()):
        print(f"{entry}: worst deviation against the oracle {v:.2e}")
