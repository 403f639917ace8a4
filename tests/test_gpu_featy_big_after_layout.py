"""ovgpu_debug_option "featy_big" thrown AFTER the batch was laid out (run with `-m gpu`).

Every other test sets its switches before ovgpu_set_features.  Thrown behind it, the switch meets a batch whose column-block lists were built for the
one-pass kernel's 64-column blocks and whose plan reserved no workspace for the block-row kernel: enqueue_system (open_vins_amd/csrc/api_pipeline.inc)
builds the lists again for 32-column blocks and reserves k_feat_y_big's row-panel workspace at the launch.  The same kernel then runs on the same
tables as in a context that had the switch before the layout, so the two agree BIT FOR BIT: feat_status, chi2, dx, P' and "last_feature_kernel"
(which keeps the code of the shape the batch was laid out for).

The batch: 5 clones x 2 cameras (D = 58: one block of 64 columns, two of 32), 12 features of 10 observations (laid out for k_feat_y<4, 9>), one
workgroup each.  Five clones are too short a baseline for the triangulation (the oracle's Gauss-Newton fails on every track of this window), so the
positions are handed over — the synthetic truth, anchored at each track's first observation: every feature reaches the gate and passes it."""
import numpy as np
import pytest

from open_vins_amd import capi, synth

pytestmark = pytest.mark.gpu

BITWISE = ("feat_status", "chi2", "dx", "P")


def _update(prob, big, after):
    from open_vins_amd.updater import UpdaterMSCKF
    up = UpdaterMSCKF(capi.default_options(chi2_multipler=1.0, gate_always_factor=1), device=0)
    if not after:
        assert up.debug_option("featy_big", big) == 0
    up.set_problem(prob)
    truth = np.ascontiguousarray(prob.p_FinG_true, np.float64).reshape(-1, 3)
    up.set_triangulation(truth, truth, np.ascontiguousarray(prob.meas_offsets[:-1], np.int32), np.full(prob.F, capi.FEAT_USED, np.int32))
    if after:
        assert up.debug_option("featy_big", big) == 0
    out = up.update()
    out["kernel"] = up.debug_option("last_feature_kernel")
    assert up.debug_option("featy_big") == big
    up.close()
    return out


def test_featy_big_thrown_after_the_layout_equals_thrown_before():
    import torch
    assert torch.cuda.is_available(), "this test needs a GPU"
    prob = synth.make_problem(2, F=12, C=5, K=2)
    for big in (1, 2):
        before, after = _update(prob, big, False), _update(prob, big, True)
        used = int(np.sum(before["feat_status"] == capi.FEAT_USED))
        print(f"featy_big {big}: kernel {before['kernel']} / {after['kernel']}, {used} of {prob.F} features used")
        assert before["kernel"] == 1 and used == prob.F and np.linalg.norm(before["dx"]) > 0  # the fast path ran, and every feature's rows reached the update
        assert after["kernel"] == before["kernel"]
        for k in BITWISE:
            x, y = np.asarray(after[k]), np.asarray(before[k])
            assert x.shape == y.shape and x.dtype == y.dtype, (big, k)
            assert np.array_equal(x, y, equal_nan=True), (big, k, int(np.sum(~((x == y) | ((x != x) & (y != y))))))
