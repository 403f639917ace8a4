"""GPU tests (`-m gpu`) of the fused per-feature kernel of UpdaterSLAM::update (csrc/k_slam_y.h), selected with
ovgpu_debug_option "slam_fused" = 1 and off by default.

Comparators: the oracle's slam_update, and a second context of the same library with "slam_fused" = 0 (the general kernel, k_system_t).  Bounds
are tests/test_gpu_parity.py's, the ones tests/test_gpu_slam_chunked.py uses (imported): 10 TOL_DX on dx, 10 TOL_P on P' (exactly symmetric),
TOL_CHI2, 1e-9 on landmarks and poses.  Accept sets are compared as they are: for every batch the ORACLE ALONE leaves no feature within
parity_util.GATE_MARGIN of its threshold (tests/test_slam_shapes_cpu.py, asserted again here on the oracle's own numbers).  Every case
asserts "last_feature_kernel" against slam_shapes' restatement of the eligibility rule; a batch the kernel does not take must return the
switch-off context's BITS with "slam_fused_batches" unchanged.  The batches and what each is named for: tests/slam_shapes.py.

Worst deviations over the kernel-4 cases, measured on the MI355X (every test prints its own; test_zz_worst_deviations the maxima): against the
oracle chi2 8.7e-13, dx 6.2e-13, P' 8.9e-14, landmarks 1.2e-13, poses 5.1e-13; against the switch-off context chi2 8.9e-13, dx 5.7e-13,
P' 5.2e-14, landmarks 3.0e-14, poses 6.8e-13.
"""
import copy
import ctypes

import numpy as np
import pytest

import slam_shapes as ss
from open_vins_amd import capi, synth
from test_gpu_parity import TOL_CHI2, TOL_DX, TOL_P
from test_gpu_slam_chunked import assert_equal_outputs, chain, chunked

pytestmark = pytest.mark.gpu

STATE_KEYS = ("clone_q_p", "calib_q_p", "intrinsics")
OUT_KEYS = ("feat_status", "chi2", "chi2_thresh", "dx", "P", "landmarks") + STATE_KEYS
WORST = {}  # (comparator, quantity) -> largest deviation over the kernel-4 cases run so far


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def switched(Updater, value):
    """an Updater factory whose contexts have "slam_fused" set before anything is uploaded (the name is unknown to a library without the kernel)"""
    def make(opts):
        up = Updater(opts)
        if value is not None:
            up.debug_option("slam_fused", value)
        return up
    return make


def run(Updater, case, fused, keep=False):
    up = switched(Updater, fused)(case.opts())
    p = case.prob
    up.set_slam_problem(p)
    if case.sigma is not None or case.mult is not None:
        up.set_feature_options(sigma_pix=case.sigma, chi2_multipler=case.mult)
    if case.entry == "compress":
        out = up.slam_compress()
    else:
        out = up.slam_update(p.lm_index)
        out.update(up.get_state(P=False))
    out["kernel"], out["batches"] = up.debug_option("last_feature_kernel"), up.debug_option("slam_fused_batches")
    if keep:
        return out, up
    up.close()
    return out


def note(comparator, **dev):
    for k, v in dev.items():
        WORST[(comparator, k)] = max(WORST.get((comparator, k), 0.0), float(v))


def check_oracle(oracle, case, out, ref, what):
    assert ref["near_gate"] == 0
    assert np.array_equal(out["feat_status"], ref["feat_status"]), what
    gate = np.isfinite(ref["chi2"])
    post = oracle.apply_dx(case.opts(), capi.Views(case.prob), ref["dx"])
    dev = dict(chi2=np.abs(out["chi2"][gate] / ref["chi2"][gate] - 1.0).max(), dx=_rel(out["dx"], ref["dx"]), P=_rel(out["P"], ref["P"]),
               landmarks=np.abs(out["landmarks"] - ref["landmarks"]).max(), poses=max(np.abs(out[k] - post[k]).max() for k in STATE_KEYS))
    print(f"{what} kernel {out['kernel']} against the oracle: " + "  ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    if out["kernel"] == 4:
        note("oracle", **dev)
    np.testing.assert_allclose(out["chi2"][gate], ref["chi2"][gate], rtol=TOL_CHI2)
    np.testing.assert_allclose(out["chi2_thresh"][gate], ref["chi2_thresh"][gate], rtol=1e-12)
    assert np.isnan(out["chi2"][~gate]).all()
    assert out["stats"]["n_used"] == ref["stats"]["n_used"] and out["stats"]["n_rows"] == ref["stats"]["n_rows"]
    assert dev["dx"] < 10 * TOL_DX
    assert dev["P"] < 10 * TOL_P and np.array_equal(out["P"], out["P"].T)
    assert dev["landmarks"] < 1e-9 and dev["poses"] < 1e-9


def check_pair(a, b, what, comparator="switch-off context"):
    """the fused context against the general kernel's, with the oracle's bounds"""
    assert np.array_equal(a["feat_status"], b["feat_status"]), what
    gate = np.isfinite(b["chi2"])
    assert np.array_equal(np.isfinite(a["chi2"]), gate)
    dev = dict(chi2=np.abs(a["chi2"][gate] / b["chi2"][gate] - 1.0).max() if gate.any() else 0.0, dx=_rel(a["dx"], b["dx"]), P=_rel(a["P"], b["P"]),
               landmarks=np.abs(a["landmarks"] - b["landmarks"]).max(), poses=max(np.abs(a[k] - b[k]).max() for k in STATE_KEYS))
    print(f"{what} against the {comparator}: " + "  ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    note(comparator, **dev)
    assert np.array_equal(a["chi2_thresh"][gate], b["chi2_thresh"][gate])
    assert dev["chi2"] < TOL_CHI2 and dev["dx"] < 10 * TOL_DX and dev["P"] < 10 * TOL_P and np.array_equal(a["P"], a["P"].T)
    assert dev["landmarks"] < 1e-9 and dev["poses"] < 1e-9
    for k in ("n_used", "n_rows", "D", "status"):
        assert a["stats"][k] == b["stats"][k], k


def check_case(Updater, oracle, case):
    """kernel as the rule says; kernel 4: oracle + switch-off context within the bounds; kernel 0: the switch-off context's bits, counter unchanged"""
    ref = ss.oracle_run(oracle, case)
    on, off = run(Updater, case, 1), run(Updater, case, 0)
    assert off["kernel"] == 0 and off["batches"] == 0
    assert on["kernel"] == case.kernel, (case.id, on["kernel"])
    if case.kernel == 4:
        assert on["batches"] == 1
        check_oracle(oracle, case, on, ref, case.id)
        check_pair(on, off, case.id)
    else:
        assert on["batches"] == 0
        assert_equal_outputs(on, off, f"{case.id}: kernel 0 against the switch-off context", keys=OUT_KEYS)
        check_oracle(oracle, case, on, ref, case.id)
    return on, off, ref


# --------------------------------------------------------------------------- representations, anchors, fisheye, FEJ
@pytest.mark.parametrize("cid", [c.id for c in ss.CASES if c.group == "rep"])
def test_representations(Updater, oracle, cid):
    on, _, ref = check_case(Updater, oracle, ss.BY_ID[cid])
    assert on["kernel"] == 4
    if ss.BY_ID[cid].outliers:
        assert (on["feat_status"] == capi.FEAT_CHI2_REJECTED).any() and (on["feat_status"] == capi.FEAT_USED).any()


# --------------------------------------------------------------------------- track lengths: every tile-row edge, the lane edge, the bound
@pytest.mark.parametrize("cid", [c.id for c in ss.CASES if c.group == "len"])
def test_track_lengths(Updater, oracle, cid):
    case = ss.BY_ID[cid]
    on, off, ref = check_case(Updater, oracle, case)
    assert on["kernel"] == (4 if case.m_max <= ss.BOUND else 0)
    m = np.diff(case.prob.meas_offsets)
    assert (on["feat_status"][m == 0] == capi.FEAT_TOO_FEW_MEAS).all() and (m == 0).sum() == 1
    assert on["stats"]["n_used"] == ref["stats"]["n_used"] and on["stats"]["n_rows"] == ref["stats"]["n_rows"]
    if case.outliers:
        assert (on["feat_status"] == capi.FEAT_CHI2_REJECTED).sum() == 1


# --------------------------------------------------------------------------- column counts
@pytest.mark.parametrize("cid", [c.id for c in ss.CASES if c.group == "col"])
def test_columns(Updater, oracle, cid):
    case = ss.BY_ID[cid]
    on, _, _ = check_case(Updater, oracle, case)
    assert on["stats"]["D"] == case.D
    assert on["kernel"] == (4 if case.D <= 383 else 0)


# --------------------------------------------------------------------------- per-feature noise and multiplier
def test_feature_noise_and_multiplier(Updater, oracle):
    case = ss.BY_ID["noise"]
    on, _, _ = check_case(Updater, oracle, case)
    assert on["kernel"] == 4 and on["feat_status"][ss.NOISE_F] == capi.FEAT_CHI2_REJECTED
    ones = copy.copy(case)
    ones.mult = case.mult.copy()
    ones.mult[ss.NOISE_F] = 1.0
    alt = run(Updater, ones, 1)
    assert alt["kernel"] == 4 and alt["feat_status"][ss.NOISE_F] == capi.FEAT_USED  # the multiplier alone decided
    assert alt["chi2"][ss.NOISE_F] == on["chi2"][ss.NOISE_F] and alt["chi2_thresh"][ss.NOISE_F] > on["chi2_thresh"][ss.NOISE_F]


# --------------------------------------------------------------------------- fall-backs: kernel 0, the switch-off context's bits
@pytest.mark.parametrize("cid", ["fb-single-depth", "fb-general", "fb-tsqr", "fb-semi-definite"])
def test_fall_backs(Updater, oracle, cid):
    case = ss.BY_ID[cid]
    on, off, ref = check_case(Updater, oracle, case)
    assert on["kernel"] == 0 and on["batches"] == 0 and on["stats"]["status"] == 0
    if cid == "fb-semi-definite":  # repeated through the Householder route: the landmarks moved ONCE (a second correction would show as |dx| ~ 1e-2)
        assert np.abs(on["landmarks"] - ref["landmarks"]).max() < 1e-9 < np.abs(ref["landmarks"] - case.prob.lm_value).max()


def test_mode_a_keeps_the_general_kernel(Updater):
    case = ss.BY_ID["fb-mode-a"]
    on, off = run(Updater, case, 1), run(Updater, case, 0)
    assert on["kernel"] == 0 and on["batches"] == 0 and on["rows"] == off["rows"] and on["D"] == off["D"]
    for k in ("feat_status", "chi2", "chi2_thresh", "H", "r", "col_cov_id"):
        assert np.array_equal(on[k], off[k], equal_nan=True), k


# --------------------------------------------------------------------------- chunks
def _batch(p):
    q = p.subset(np.arange(p.F))
    q.lm_index = np.arange(p.F, dtype=np.int32)
    return q


@pytest.mark.parametrize("which", ["3dof", "single_depth_in_every_chunk"])
def test_chunks_equal_the_chain_with_the_switch_on(Updater, which):
    """FIRST_5 = [0, 9, 9, 22, 38, 50]: every non-empty chunk takes k_slam_y on the five 3-dof representations, none on the six in turn"""
    opts = capi.default_options(chi2_multipler=1.0)
    q = _batch(ss.chunk_problem_3dof() if which == "3dof" else ss.chunk_problem())
    kernel, pipelines = (4, 4) if which == "3dof" else (0, 0)  # four non-empty chunks
    out, up = chunked(switched(Updater, 1), opts, q, ss.FIRST_5, keep=True)
    ref, up2 = chain(switched(Updater, 1), opts, q, ss.FIRST_5, keep=True)
    for u in (up, up2):
        assert u.debug_option("last_feature_kernel") == kernel and u.debug_option("slam_fused_batches") == pipelines
        u.close()
    assert_equal_outputs(out, ref, f"five chunks ({which}), switch on, against the chain, switch on")
    assert sum(s["n_used"] for s in out["stats"]) >= 30
    if which == "3dof":  # ... and the general kernel's pass within the bounds
        off = chunked(switched(Updater, 0), opts, q, ss.FIRST_5)
        assert np.array_equal(out["feat_status"], off["feat_status"])
        dev = dict(dx=max(_rel(out["dx_seq"][k], off["dx_seq"][k]) for k in (0, 2, 3, 4)), P=_rel(out["P"], off["P"]),
                   landmarks=np.abs(out["landmarks"] - off["landmarks"]).max())
        print("five chunks, switch on against switch off: " + "  ".join(f"{k} {v:.3e}" for k, v in dev.items()))
        note("switch-off context", **dev)
        assert dev["dx"] < 10 * TOL_DX and dev["P"] < 10 * TOL_P and dev["landmarks"] < 1e-9


def test_one_chunk_is_the_single_call(Updater):
    opts = capi.default_options(chi2_multipler=1.0)
    q = _batch(ss.chunk_problem_3dof())
    out, up0 = chunked(switched(Updater, 1), opts, q, [0, 50], keep=True)
    assert up0.debug_option("last_feature_kernel") == 4
    up0.close()
    up = switched(Updater, 1)(opts)
    up.set_slam_problem(q)
    up.set_active_landmarks(np.unique(q.lm_index))
    up.set_features(q)
    one = up.slam_update()
    assert up.debug_option("last_feature_kernel") == 4
    one.update(up.get_state(P=False))
    up.close()
    one["dx_seq"] = one["dx"][None, :]
    assert_equal_outputs(out, one, "n_chunks = 1 against ovgpu_slam_update, switch on")


# --------------------------------------------------------------------------- what a fused update leaves behind
def test_state_left_behind(Updater):
    """a second SLAM batch on the same context, then ovgpu_msckf_update_lm behind it: the fused context against the switch-off one"""
    case = ss.BY_ID["rep-mix"]
    p = case.prob
    tracks = synth.make_problem(2, F=40, seed=p.seed)  # the same window (the state stream follows the seed), forty tracks
    msckf = copy.copy(p)
    for k in ("meas_offsets", "uv", "uvn", "clone_idx", "cam_idx", "p_FinG_true"):
        setattr(msckf, k, getattr(tracks, k))
    res = []
    for fused in (1, 0):
        first, up = run(Updater, case, fused, keep=True)
        up.set_features(p)
        second = up.slam_update(p.lm_index)
        second.update(up.get_state(P=False))
        second["kernel"] = up.debug_option("last_feature_kernel")
        up.set_active_landmarks([])
        up.set_features(msckf)
        third = up.update_lm()
        third["kernel"] = up.debug_option("last_feature_kernel")
        up.close()
        res.append((first, second, third))
    (a1, a2, a3), (b1, b2, b3) = res
    assert (a1["kernel"], a2["kernel"]) == (4, 4) and (b1["kernel"], b2["kernel"]) == (0, 0) and a3["kernel"] == b3["kernel"] != 4
    check_pair(a2, b2, "the second SLAM batch")
    assert a2["stats"]["n_used"] >= 5 and np.abs(a2["landmarks"] - a1["landmarks"]).max() > 0
    assert np.array_equal(a3["feat_status"], b3["feat_status"]) and a3["stats"]["n_used"] >= 20
    dev = dict(dx=_rel(a3["dx"], b3["dx"]), P=_rel(a3["P"], b3["P"]), landmarks=np.abs(a3["landmarks"] - b3["landmarks"]).max(),
               poses=max(np.abs(a3[k] - b3[k]).max() for k in STATE_KEYS))
    print("ovgpu_msckf_update_lm behind the SLAM updates, fused against switch off: " + "  ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    assert dev["dx"] < 10 * TOL_DX and dev["P"] < 10 * TOL_P and np.array_equal(a3["P"], a3["P"].T) and dev["landmarks"] < 1e-9 and dev["poses"] < 1e-9


# --------------------------------------------------------------------------- determinism, and the switch
def test_same_bits_twice_from_reset_state(Updater):
    case = ss.BY_ID["rep-mix-outliers"]
    first, up = run(Updater, case, 1, keep=True)
    up.reset_state()  # the prior and the pose tables; the landmarks the first call corrected are handed over again, then the batch
    capi.check(up.lib.ovgpu_set_landmarks(up._ctx, ctypes.byref(up._views.landmarks)), "ovgpu_set_landmarks")
    up.set_features(case.prob)
    second = up.slam_update(case.prob.lm_index)
    second.update(up.get_state(P=False))
    assert up.debug_option("last_feature_kernel") == 4 and up.debug_option("slam_fused_batches") == 2
    up.close()
    assert_equal_outputs(first, second, "the same call twice from ovgpu_reset_state", keys=OUT_KEYS)
    assert (first["feat_status"] == capi.FEAT_CHI2_REJECTED).any()


def test_switch_is_off_by_default(Updater):
    case = ss.BY_ID["rep-mix"]
    never = run(Updater, case, None)
    zero = run(Updater, case, 0)
    assert never["kernel"] == 0 and zero["kernel"] == 0 and never["batches"] == 0
    assert_equal_outputs(never, zero, "never set against slam_fused = 0", keys=OUT_KEYS)
    up = Updater(case.opts())
    assert up.debug_option("slam_fused") == 0
    assert up.debug_option("slam_fused", 1) == 0 and up.debug_option("slam_fused") == 1
    up.set_slam_problem(case.prob)
    up.debug_option("slam_fused", 0)  # takes effect with the next ovgpu_set_features: the batch in force was laid out with the switch on
    up.slam_update(case.prob.lm_index)
    assert up.debug_option("last_feature_kernel") == 4
    up.reset_state()
    up.set_features(case.prob)
    up.slam_update(case.prob.lm_index)
    assert up.debug_option("last_feature_kernel") == 0 and up.debug_option("slam_fused_batches") == 1
    up.close()


def test_zz_worst_deviations():
    """prints what the kernel-4 cases of this file measured (DESIGN.md section 7 quotes the figures)"""
    for (comparator, k), v in sorted(WORST.items()):
        print(f"k_slam_y against the {comparator}: worst {k} {v:.3e}")
