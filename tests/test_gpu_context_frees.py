"""A destroyed context leaves nothing allocated (run with `-m gpu` on an MI355X).

ovgpu_debug_option "live_allocations" / "live_allocation_bytes" count what the library's buffers hold in the whole process.  A reader context stays
alive and supplies the baseline; a second context is driven through small calls that between them reserve every family of buffers — among them
the twelve that the hand-written release list of ovgpu_destroy used to miss (lm_repd, trk_order, isx_arena, isx_save, isx_cols, cls_of_clone,
raw_featbase, raw_dst, raw_runs, Hraw, gram_wg, sys_rows_ws) — and is destroyed: both counters are the baseline again, exactly.  The same for
ovgpu_multi_create / ovgpu_multi_destroy on a loop-back communicator of two ranks on one device after one sharded update (LoopComm::sum).

Every step asserts, through the library's read-only names, that it took the route it is here for; none is held to the oracle (the catalogues
the shapes come from are: tests/test_gpu_gram_regions_shapes.py, test_gpu_system_edges.py, test_gpu_mixed_reps.py,
test_gpu_delayed_init_mode_a.py, test_gpu_parity.py, test_gpu_fullsize.py).

The third test runs a context on device 0 and then one on device 1 in one process (the per-device latch of the kernels' LDS limit,
api_context.inc: with_max_lds); it needs two devices and skips without them."""
import functools
import gc

import numpy as np
import pytest

import slam_long_shapes as s3
import system_shapes as sy
import test_gpu_slam_fused as tf
import track_shapes as ts
from open_vins_amd import capi, synth
from test_gpu_parity import TOL_DX, TOL_P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


@pytest.fixture()
def reader(Updater):
    """the context that stays alive, and the counters before the context under test exists"""
    gc.collect()  # (an updater an earlier test dropped without close() would free its context in the middle of this one)
    up = Updater(capi.default_options())
    yield up, live(up)
    up.close()


def live(up):
    return up.debug_option("live_allocations"), up.debug_option("live_allocation_bytes")


def _msckf_fused_raw_stack(up):
    """12 clones, one camera (D = 86: six tile columns, the smallest state with the unprojected stack), eight full tracks: k_feat_y writes the
    stack in regions, k_gram_regions forms the Gram matrix (cls_of_clone, raw_featbase, raw_dst, raw_runs, Hraw, gram_wg)"""
    up.set_problem(ts.region_batch("nt6"))
    out = up.update()
    assert up.debug_option("last_feature_kernel") in (1, 2) and up.debug_option("last_stack_raw") == 1 and up.debug_option("last_gram_kernel") == 4
    assert out["stats"]["n_used"] >= 1


def _records_in_the_workspace(up):
    """16 clones, one camera, six anchored landmarks, the longest track at the first length whose Jacobian records leave LDS: k_system_t<true>
    (sys_rows_ws)"""
    limit = up.debug_option("sys_lds_limit")
    _, r72 = sy.edges(72, ts.n_columns(16, 1) + 18, limit)
    _, prob, _ = sy.slam_mixed(sy.E_ANCHORED, r72, 42)
    up.set_slam_problem(prob)
    out = up.slam_update(prob.lm_index)
    assert up.debug_option("sys_rows_global") == 1 and up.debug_option("last_feature_kernel") == 0 and out["stats"]["n_used"] >= 1


def _slam_mixed_then_marginalize(up):
    """four landmarks of four representations, one of them single-depth (lm_repd and its second buffer); then the 1-dof landmark and, its
    landmarks re-anchored, the oldest clone leave the state (the scratch buffers of ovgpu_state_marginalize)"""
    each = np.array([0, 4, 5, 2], np.int32)
    prob = synth.make_slam_problem(2, L=4, lm_rep=each, C=14, seed=21)
    up.set_slam_problem(prob)
    out = up.slam_update(prob.lm_index)
    assert out["stats"]["n_used"] >= 1
    N = up.N
    up.state_marginalize(int(prob.lm_cov_id[2]), 1)
    up.change_anchors(0, prob.C - 1)
    first = int(prob.clone_cov_id[0])
    up.state_marginalize(first - (1 if prob.lm_cov_id[2] < first else 0), 6)
    assert up.N == N - 7 and up.Cn == prob.C - 1 and len(up.get_landmarks()["cov_id"]) == 3


def _init_systems(up):
    """four clones, two cameras, two resident landmarks, three candidates: mode A of the delayed initialisation (isx_arena, isx_save, isx_cols)"""
    kw = dict(C=4, K=2, min_obs=3)
    prob = synth.make_slam_problem(2, L=2, lm_rep=np.array([capi.REP_GLOBAL_3D, capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH], np.int32), seed=71, **kw)
    tracks = synth.make_problem(2, F=16, seed=71, shard=1, **kw).subset([0, 6, 7])
    for k in ("meas_offsets", "uv", "uvn", "clone_idx", "cam_idx"):
        setattr(prob, k, getattr(tracks, k))
    up.set_slam_problem(prob)
    sys_ = up.init_systems(capi.REP_ANCHORED_3D)
    assert len(sys_) == 3 and any(s["H_x"] is not None for s in sys_)


def _track_store(up):
    """five clones, two cameras, twelve tracks through the device's track store, the batch assembled in the reference's camera-group order (trk_order)"""
    prob = synth.make_problem(2, F=12, C=5, K=2)
    up.set_problem(prob)
    up.tracks_create(32, 16)
    clone_times = 50.0 + 0.1 * np.arange(prob.C)
    feat_of = np.repeat(np.arange(prob.F), np.diff(prob.meas_offsets))
    uv2, uvn2 = prob.uv.reshape(-1, 2), prob.uvn.reshape(-1, 2)
    for cl in range(prob.C):
        for cam in range(prob.K):
            idx = np.flatnonzero((prob.clone_idx == cl) & (prob.cam_idx == cam))
            if len(idx):
                up.tracks_append(clone_times[cl], 1000 + feat_of[idx], np.full(len(idx), cam), uv2[idx], uvn2[idx])
    up.tracks_group_order(capi.GROUPS_REFERENCE)
    up.tracks_to_features(1000 + np.arange(prob.F), clone_times)
    got = up.get_features()
    assert len(got["meas_offsets"]) == prob.F + 1 and got["meas_offsets"][-1] == prob.meas_offsets[-1]


def _cam_distort(up):
    dp = capi.c_double_p
    cam = np.array(synth._INTRINSICS[0])
    uvn = np.linspace(-0.5, 0.5, 16).reshape(8, 2).copy()
    uv, a, b = np.zeros((8, 2)), np.zeros((8, 4)), np.zeros((8, 16))
    capi.check(up.lib.ovgpu_cam_distort(up._ctx, 0, cam.ctypes.data_as(dp), 8, uvn.ctypes.data_as(dp), uv.ctypes.data_as(dp), a.ctypes.data_as(dp),
                                        b.ctypes.data_as(dp)), "ovgpu_cam_distort")
    assert np.isfinite(uv).all() and np.abs(uv).max() > 0


STEPS = (_msckf_fused_raw_stack, _records_in_the_workspace, _slam_mixed_then_marginalize, _init_systems, _track_store, _cam_distort)


def test_a_destroyed_context_leaves_nothing_allocated(Updater, reader):
    rd, base = reader
    up = Updater(capi.default_options(chi2_multipler=1.0, gate_always_factor=1))
    for step in STEPS:
        step(up)
        print(f"live after {step.__name__}: {live(rd)}")
    held = live(rd)
    assert held[0] >= base[0] + 50 and held[1] > base[1]  # (the counters count: the steps above reserve about a hundred buffers)
    up.close()
    after = live(rd)
    print(f"live allocations / bytes: baseline {base}, before the destroy {held}, after it {after}: left {after[0] - base[0]} / {after[1] - base[1]}")
    assert after == base


def test_a_destroyed_multi_context_leaves_nothing_allocated(reader):
    from open_vins_amd.updater import MultiUpdater
    rd, base = reader
    m = MultiUpdater(capi.default_options(chi2_multipler=1.0), devices=[0, 0])
    m.set_problem(synth.make_problem(2, F=12))
    out = m.update()
    assert out["stats"]["n_used"] >= 1
    held = live(rd)
    assert held[0] > base[0]
    m.close()
    after = live(rd)
    print(f"two ranks on one device: baseline {base}, before the destroy {held}, after it {after}: left {after[0] - base[0]} / {after[1] - base[1]}")
    assert after == base


def test_contexts_on_two_devices_in_one_process(Updater, oracle):
    """device 0 first, then device 1: one MSCKF update on the fused per-feature kernel (D = 86, the unprojected stack) and one SLAM update at
    "slam_fused" = 3 (63 observations: the long shape) on each, held to the oracle with the bounds of tests/test_gpu_slam_long.py"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    msckf, slam = ts.BY_ID["f-nt6"], s3.BY_ID["len-3dof-63"]
    tri, ref = ts.oracle_run(oracle, msckf)
    for device in (0, 1):
        On = functools.partial(Updater, device=device)
        up = On(msckf.opts())
        up.set_problem(msckf.prob)
        up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
        out = up.update()
        assert up.debug_option("last_feature_kernel") in (1, 2) and up.debug_option("last_stack_raw") == 1
        up.close()
        assert np.array_equal(out["feat_status"], ref["feat_status"]) and ref["stats"]["n_used"] >= 1
        assert out["stats"]["n_used"] == ref["stats"]["n_used"] and out["stats"]["n_rows"] == ref["stats"]["n_rows"]
        assert tf._rel(out["dx"], ref["dx"]) < 10 * TOL_DX and tf._rel(out["P"], ref["P"]) < 10 * TOL_P and np.array_equal(out["P"], out["P"].T)
        on = tf.run(On, slam, 3)
        assert on["kernel"] == 6 and on["batches"] == 1
        tf.check_oracle(oracle, slam, on, s3.oracle_run(oracle, slam), f"{slam.id} on device {device}")
