"""The per-feature kernels at every track-length and region edge (run with `-m gpu` on an MI355X).

The MSCKF fast path picks its kernel from the longest track of the batch — k_feat_y<4, 9, 2> up to 62 observations, <8, 17, 1> up to 126,
k_feat_y_big up to 232, k_system beyond — and stacks unprojected rows in regions for 6 .. 15 tile columns.  Every batch of tests/track_shapes.py
(built to sit ON those edges, and shown non-vacuous on the oracle alone by tests/test_track_shapes_cpu.py) runs here with the oracle's
positions injected, is held to the ORACLE at the suite's tolerances — chi2 1e-8, thresholds 1e-12, dx 1e-8, P 1e-9 and exactly symmetric,
poses 1e-9, accept sets identical with no excuse — and must report the kernel and the stack layout that the documented rule gives
(track_shapes.expected_kernel / expected_raw: never read back from the library).  gate_always_factor = 1 unless the case says otherwise, so every
chi2 is the reference's statistic.

Groups: (a) uniform batches of one length over the sweep, (b) one long track next to tracks of 0 .. 32 observations, both orders, (c) the
kernels forced by their switches, (d) options.gram_fp32 (dx 1e-4, P 1e-3 as tests/test_gpu_fullsize.py holds that option; the gate stays float64:
chi2 1e-8), (e) an anchored feat_rep_msckf, (f) region edges of the unprojected stack, each positive case also against the projected stack of
the same library (dx 1e-10, P 1e-11, same statuses: the bounds of test_gpu_parity.test_track_store_feeds_the_update).
Each case prints one line `edge ...` with its deviations (DESIGN §3 quotes the worst per kernel)."""
import numpy as np
import pytest

import track_shapes as ts
from open_vins_amd import capi
from parity_util import assert_chi2

pytestmark = pytest.mark.gpu

TOL_CHI2, TOL_THR, TOL_DX, TOL_P, TOL_POSE = 1e-8, 1e-12, 1e-8, 1e-9, 1e-9
TOL_DX_F32, TOL_P_F32 = 1e-4, 1e-3   # options.gram_fp32: float sums of the Gram matrix (tests/test_gpu_fullsize.py::test_fp32_gram_variant)
TOL_DX_RAW, TOL_P_RAW = 1e-10, 1e-11  # unprojected against projected stack


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _run(Updater, case, tri, **debug):
    up = Updater(case.opts())
    for name, val in {**case.debug, **debug}.items():
        up.debug_option(name, val)
    up.set_problem(case.prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    out = up.update()
    out["kernel"], out["raw"], out["stack_f32"] = up.debug_option("last_feature_kernel"), up.debug_option("last_stack_raw"), up.debug_option("stack_is_f32")
    up.close()
    return out


def _hold_to_the_oracle(case, out, ref, want_raw):
    fp32 = bool(case.options.get("gram_fp32", 0))
    strict = bool(case.options.get("gate_always_factor", 1))
    gate = np.isfinite(ref["chi2"])
    assert gate.sum() > 0
    dchi = np.abs(out["chi2"][gate] / ref["chi2"][gate] - 1.0).max() if strict else float("nan")
    ddx, dP = _rel(out["dx"], ref["dx"]), _rel(out["P"], ref["P"])
    print(f"edge {case.id} kernel {out['kernel']} raw {out['raw']} f32 {out['stack_f32']} m_max {case.longest_track} D {case.D}: chi2 {dchi:.2e} dx {ddx:.2e} P {dP:.2e}")
    assert out["kernel"] == case.kernel, (out["kernel"], case.kernel)
    assert out["raw"] == want_raw, (out["raw"], want_raw)
    assert out["stack_f32"] == (1 if fp32 else 0)
    assert out["route"] == capi.COMPRESS_GRAM
    assert np.array_equal(out["feat_status"], ref["feat_status"]), (out["feat_status"], ref["feat_status"])  # every feature, no excuse
    assert_chi2(out, ref, TOL_CHI2, strict=strict)
    np.testing.assert_allclose(out["chi2_thresh"][gate], ref["chi2_thresh"][gate], rtol=TOL_THR)
    assert out["stats"]["n_used"] == ref["stats"]["n_used"] and out["stats"]["n_rows"] == ref["stats"]["n_rows"]
    assert ddx < (TOL_DX_F32 if fp32 else TOL_DX)
    assert dP < (TOL_P_F32 if fp32 else TOL_P)
    assert np.array_equal(out["P"], out["P"].T)
    if not fp32:
        assert np.abs(out["clone_q_p"] - ref["clone_q_p"]).max() < TOL_POSE
        assert np.abs(out["calib_q_p"] - ref["calib_q_p"]).max() < TOL_POSE
        assert np.abs(out["intrinsics"] - ref["intrinsics"]).max() < 1e-8


@pytest.mark.parametrize("cid", [c.id for c in ts.CASES])
def test_track_edge(Updater, oracle, cid):
    case = ts.BY_ID[cid]
    tri, ref = ts.oracle_run(oracle, case)
    out = _run(Updater, case, tri)
    _hold_to_the_oracle(case, out, ref, case.raw)
    if case.raw:  # the same batch on the projected stack: the other layout of the same rows
        proj = _run(Updater, case, tri, raw_stack=0)
        ddx, dP = _rel(out["dx"], proj["dx"]), _rel(out["P"], proj["P"])
        print(f"edge {case.id} raw against projected: dx {ddx:.2e} P {dP:.2e}")
        assert proj["raw"] == 0 and proj["kernel"] == case.kernel
        assert np.array_equal(proj["feat_status"], out["feat_status"])
        assert ddx < TOL_DX_RAW and dP < TOL_P_RAW
        if case.group == "f":
            _hold_to_the_oracle(case, proj, ref, 0)  # (... and the projected layout of these widths against the oracle as well)
