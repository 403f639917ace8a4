"""An upload that does not fit the page-locked arena computes what the arena path computes (run with `-m gpu`).

ovgpu_set_state / ovgpu_set_features pack their arrays into one page-locked arena (open_vins_amd/csrc/host_link.h: Uplink).  An array that does
not fit what is left of it bypasses the arena: it is copied from the caller's memory, the stream is synchronised inside the call, and — in
ovgpu_set_state — the device-side copy of the prior that ovgpu_reset_state restores is made by copy_reset_baseline instead of a second
destination of the arena bytes.  ovgpu_debug_option "upload_arena_bytes" = 4096 before the first upload makes that path reachable at a small
shape: the covariance (73 x 73 doubles) is ten times the arena.  Context A has the default arena, context B the small one; both run
ovgpu_set_state, ovgpu_set_features, ovgpu_msckf_update, ovgpu_reset_state and the same batch and update once more, and agree BIT FOR BIT on
feat_status, chi2, dx and P' of both updates (the second proves the restored prior).  That the bypassed array's source may die when the call
returns is what tests/test_host_link_host.py proves on the CPU; a run on the device cannot show it.

The batch is tests/test_gpu_featy_big_after_layout.py's: 5 clones x 2 cameras, 12 tracks of 10 observations, the true positions handed over."""
import ctypes as C

import numpy as np
import pytest

from open_vins_amd import capi, synth

pytestmark = pytest.mark.gpu

BITWISE = ("feat_status", "chi2", "dx", "P")
SMALL = 4096


def _run(prob, arena_bytes):
    from open_vins_amd.updater import UpdaterMSCKF
    up = UpdaterMSCKF(capi.default_options(chi2_multipler=1.0, gate_always_factor=1), device=0)
    if arena_bytes:
        assert up.debug_option("upload_arena_bytes", arena_bytes) == 0  # nothing uploaded yet: no arena
    truth = np.ascontiguousarray(prob.p_FinG_true, np.float64).reshape(-1, 3)
    anchors, used = np.ascontiguousarray(prob.meas_offsets[:-1], np.int32), np.full(prob.F, capi.FEAT_USED, np.int32)
    outs = []
    up.set_problem(prob)  # ovgpu_set_state, ovgpu_set_features
    up.set_triangulation(truth, truth, anchors, used)
    outs.append(up.update())
    up.reset_state()
    up.set_features(prob)
    up.set_triangulation(truth, truth, anchors, used)
    outs.append(up.update())
    capi.check(up.lib.ovgpu_set_state(up._ctx, C.byref(up._views.state)), "ovgpu_set_state")
    info = {"bypasses": up.debug_option("upload_bypasses"), "arena": up.debug_option("upload_arena_bytes")}
    up.close()
    return outs, info


def test_arena_bypass_equals_arena_path_bit_for_bit():
    import torch
    assert torch.cuda.is_available(), "this test needs a GPU"
    prob = synth.make_problem(2, F=12, C=5, K=2)
    a, info_a = _run(prob, 0)
    b, info_b = _run(prob, SMALL)
    print(f"default arena: {info_a}; arena of {SMALL} bytes: {info_b}")
    assert info_a["bypasses"] == 0 and info_a["arena"] == 8 << 20
    assert info_b["bypasses"] > 0 and info_b["arena"] > SMALL  # the arena has grown by the second ovgpu_set_state
    for i in range(2):
        used = int(np.sum(a[i]["feat_status"] == capi.FEAT_USED))
        assert used == prob.F and np.linalg.norm(a[i]["dx"]) > 0  # every feature's rows reached the update
        for k in BITWISE:
            x, y = np.asarray(b[i][k]), np.asarray(a[i][k])
            assert x.shape == y.shape and x.dtype == y.dtype, (i, k)
            assert np.array_equal(x, y, equal_nan=True), (i, k, int(np.sum(~((x == y) | ((x != x) & (y != y))))))
