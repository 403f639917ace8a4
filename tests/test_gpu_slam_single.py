"""GPU tests (`-m gpu`) of k_slam_y<true>: the fused per-feature kernel of UpdaterSLAM::update with the projection of single-depth landmarks
(csrc/k_slam_y.h), selected with ovgpu_debug_option "slam_fused" = 2 and off by default.

Every case runs three times: on the oracle, on a context at level 0 (the general kernel, k_system_t) and on a context at level 2.  The level-2
context must report the kernel slam_single_shapes' restatement of the rule names (5 where a single-depth landmark is observed) and count one
pipeline; feat_status, n_used and n_rows are identical across the three with no excuse (tests/test_slam_single_shapes_cpu.py: the oracle alone
leaves no statistic within parity_util.GATE_MARGIN of its threshold, asserted again here).  chi2, dx, P', landmarks and poses are held to
the bounds tests/test_gpu_slam_fused.py uses, against both comparators: TOL_CHI2 = 1e-8, 10 TOL_DX = 1e-7, 10 TOL_P = 1e-8 (P' exactly
symmetric), 1e-9, 1e-9.  A batch the kernel does not take returns the level-0 context's BITS and reports kernel 0.

Worst deviations over the kernel-5 cases, measured on the MI355X (every test prints its own; test_zz_worst_deviations the maxima): against the
oracle chi2 1.9e-13, dx 4.1e-13, P' 4.1e-14, landmarks 6.7e-14, poses 2.3e-13; against the level-0 context chi2 1.7e-13, dx 6.3e-13, P' 5.3e-14,
landmarks 3.8e-14, poses 4.0e-13.
"""
import copy
import ctypes

import numpy as np
import pytest

import slam_single_shapes as s2
from open_vins_amd import capi
from test_gpu_parity import TOL_CHI2, TOL_DX, TOL_P
from test_gpu_slam_chunked import assert_equal_outputs, assert_oracle, chunked, oracle_chain

pytestmark = pytest.mark.gpu

STATE_KEYS = ("clone_q_p", "calib_q_p", "intrinsics")
OUT_KEYS = ("feat_status", "chi2", "chi2_thresh", "dx", "P", "landmarks") + STATE_KEYS
WORST = {}  # (comparator, quantity) -> largest deviation over the kernel-5 cases run so far


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def at_level(Updater, level):
    """an Updater factory whose contexts have "slam_fused" at `level` before anything is uploaded"""
    def make(opts):
        up = Updater(opts)
        if level is not None:
            up.debug_option("slam_fused", level)
        return up
    return make


def run(Updater, case, level, keep=False):
    up = at_level(Updater, level)(case.opts())
    p = case.prob
    up.set_slam_problem(p)
    if case.sigma is not None or case.mult is not None:
        up.set_feature_options(sigma_pix=case.sigma, chi2_multipler=case.mult)
    if case.entry == "compress":
        out = up.slam_compress()
    else:
        out = up.slam_update(p.lm_index)
        out.update(up.get_state(P=False))
    out["kernel"], out["batches"], out["level"] = up.debug_option("last_feature_kernel"), up.debug_option("slam_fused_batches"), up.debug_option("slam_fused")
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
    if out["kernel"] == 5:
        note("oracle", **dev)
    np.testing.assert_allclose(out["chi2"][gate], ref["chi2"][gate], rtol=TOL_CHI2)
    np.testing.assert_allclose(out["chi2_thresh"][gate], ref["chi2_thresh"][gate], rtol=1e-12)
    assert np.isnan(out["chi2"][~gate]).all()
    assert out["stats"]["n_used"] == ref["stats"]["n_used"] and out["stats"]["n_rows"] == ref["stats"]["n_rows"]
    assert dev["dx"] < 10 * TOL_DX
    assert dev["P"] < 10 * TOL_P and np.array_equal(out["P"], out["P"].T)
    assert dev["landmarks"] < 1e-9 and dev["poses"] < 1e-9


def check_pair(a, b, what, comparator="level-0 context"):
    """the level-2 context against the general kernel's, with the oracle's bounds"""
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
    """the oracle, level 0, level 2.  Kernel as the rule says; kernel 5: both comparators within the bounds; kernel 0: the level-0 context's bits"""
    ref = s2.oracle_run(oracle, case)
    two, zero = run(Updater, case, 2), run(Updater, case, 0)
    assert zero["kernel"] == 0 and zero["batches"] == 0 and zero["level"] == 0
    assert two["level"] == 2
    assert two["kernel"] == case.kernel2, (case.id, two["kernel"])
    for out in (two, zero):  # identical across the three, no excuse
        assert np.array_equal(out["feat_status"], ref["feat_status"]), case.id
        assert out["stats"]["n_used"] == ref["stats"]["n_used"] and out["stats"]["n_rows"] == ref["stats"]["n_rows"], case.id
    if case.kernel2 == 5:
        assert two["batches"] == 1
        check_oracle(oracle, case, two, ref, case.id)
        check_pair(two, zero, case.id)
    else:
        assert two["batches"] == 0
        assert_equal_outputs(two, zero, f"{case.id}: kernel 0 against the level-0 context", keys=OUT_KEYS)
        check_oracle(oracle, case, two, ref, case.id)
    return two, zero, ref


# --------------------------------------------------------------------------- representations, anchors, fisheye, FEJ
@pytest.mark.parametrize("cid", [c.id for c in s2.CASES if c.group == "rep"])
def test_representations(Updater, oracle, cid):
    case = s2.BY_ID[cid]
    two, _, _ = check_case(Updater, oracle, case)
    assert two["kernel"] == 5
    single = case.reps_observed == s2.SINGLE
    assert ((two["feat_status"] == capi.FEAT_USED) & single).any()
    if case.outliers:
        assert ((two["feat_status"] == capi.FEAT_CHI2_REJECTED) & single).any()


# --------------------------------------------------------------------------- track lengths of a single-depth landmark
@pytest.mark.parametrize("cid", [c.id for c in s2.CASES if c.group == "len"])
def test_track_lengths(Updater, oracle, cid):
    case = s2.BY_ID[cid]
    two, zero, ref = check_case(Updater, oracle, case)
    assert two["kernel"] == (5 if case.m_max <= s2.BOUND else 0)
    m = np.diff(case.prob.meas_offsets)
    assert m[case.named] == case.m_max
    assert two["feat_status"][case.named] == (capi.FEAT_USED if case.m_max >= 2 else capi.FEAT_TOO_FEW_MEAS)
    assert (two["feat_status"][m == 0] == capi.FEAT_TOO_FEW_MEAS).all() and (m == 0).sum() == 1
    if case.rejected is not None:
        assert two["feat_status"][case.rejected] == capi.FEAT_CHI2_REJECTED and (two["feat_status"] == capi.FEAT_CHI2_REJECTED).sum() == 1


# --------------------------------------------------------------------------- the single-depth column at a block edge
@pytest.mark.parametrize("cid", [c.id for c in s2.CASES if c.group == "col"])
def test_column_edges(Updater, oracle, cid):
    case = s2.BY_ID[cid]
    two, _, _ = check_case(Updater, oracle, case)
    assert two["stats"]["D"] == case.D and two["kernel"] == 5


# --------------------------------------------------------------------------- per-feature noise and multiplier
def test_feature_noise_and_multiplier(Updater, oracle):
    case = s2.BY_ID["noise"]
    two, _, _ = check_case(Updater, oracle, case)
    assert two["kernel"] == 5 and two["feat_status"][s2.NOISE_F] == capi.FEAT_CHI2_REJECTED
    ones = copy.copy(case)
    ones.mult = case.mult.copy()
    ones.mult[s2.NOISE_F] = 1.0
    alt = run(Updater, ones, 2)
    assert alt["kernel"] == 5 and alt["feat_status"][s2.NOISE_F] == capi.FEAT_USED  # the multiplier alone decided
    assert alt["chi2"][s2.NOISE_F] == two["chi2"][s2.NOISE_F] and alt["chi2_thresh"][s2.NOISE_F] > two["chi2_thresh"][s2.NOISE_F]


# --------------------------------------------------------------------------- fall-backs: kernel 0, the level-0 context's bits
@pytest.mark.parametrize("cid", ["fb-general", "fb-tsqr"])  # (the 63-observation tracks: test_track_lengths, the same check)
def test_fall_backs(Updater, oracle, cid):
    two, zero, _ = check_case(Updater, oracle, s2.BY_ID[cid])
    assert two["kernel"] == 0 and two["batches"] == 0 and two["stats"]["status"] == 0


def test_mode_a_keeps_the_general_kernel(Updater):
    case = s2.BY_ID["fb-mode-a"]
    two, zero = run(Updater, case, 2), run(Updater, case, 0)
    assert two["kernel"] == 0 and two["batches"] == 0 and two["rows"] == zero["rows"] and two["D"] == zero["D"]
    for k in ("feat_status", "chi2", "chi2_thresh", "H", "r", "col_cov_id"):
        assert np.array_equal(two[k], zero[k], equal_nan=True), k


def test_level_one_keeps_the_mixed_batch_on_the_general_kernel(Updater):
    case = s2.BY_ID["mix"]
    one, zero = run(Updater, case, 1), run(Updater, case, 0)
    assert one["level"] == 1 and one["kernel"] == 0 and one["batches"] == 0
    assert_equal_outputs(one, zero, "level 1 on the mixed batch against level 0", keys=OUT_KEYS)


def test_the_switch_is_a_level(Updater):
    case = s2.BY_ID["mix"]
    up = Updater(case.opts())
    assert up.debug_option("slam_fused") == 0
    assert up.debug_option("slam_fused", 2) == 0 and up.debug_option("slam_fused") == 2
    assert up.debug_option("slam_fused", 1) == 2 and up.debug_option("slam_fused") == 1
    up.debug_option("slam_fused", 2)
    up.set_slam_problem(case.prob)
    up.slam_update(case.prob.lm_index)
    assert up.debug_option("last_feature_kernel") == 5 and up.debug_option("slam_fused_batches") == 1
    up.debug_option("slam_fused", 0)  # takes effect with the next layout of a batch
    up.reset_state()
    up.set_features(case.prob)
    up.slam_update(case.prob.lm_index)
    assert up.debug_option("last_feature_kernel") == 0 and up.debug_option("slam_fused_batches") == 1
    up.close()


# --------------------------------------------------------------------------- chunks
def _batch(p):
    q = p.subset(np.arange(p.F))
    q.lm_index = np.arange(p.F, dtype=np.int32)
    return q


def chain_kernels(Updater, opts, q, first):
    """test_gpu_slam_chunked.chain — the documented chain of single calls on a context of its own — that also records every chunk's kernel"""
    up = Updater(opts)
    up.set_slam_problem(q)
    F, n = q.F, len(first) - 1
    out = dict(feat_status=np.zeros(F, np.int32), chi2=np.zeros(F), chi2_thresh=np.zeros(F), dx_seq=np.zeros((n, q.N)), stats=[None] * n,
               P=np.array(q.P, dtype=np.float64), landmarks=np.array(q.lm_value, dtype=np.float64), p_FinG=np.zeros((F, 3)), p_FinA=np.zeros((F, 3)))
    kernels = []
    for k in range(n):
        a, b = int(first[k]), int(first[k + 1])
        if a == b:
            continue
        qk = q.subset(np.arange(a, b))
        lm = np.ascontiguousarray(q.lm_index[a:b], dtype=np.int32)
        up.set_active_landmarks(np.unique(lm))
        up.set_features(qk)
        o = up.slam_update(lm)
        kernels.append(up.debug_option("last_feature_kernel"))
        for key in ("feat_status", "chi2", "chi2_thresh"):
            out[key][a:b] = o[key]
        out["dx_seq"][k], out["P"], out["landmarks"], out["stats"][k] = o["dx"], o["P"], o["landmarks"], o["stats"]
        tri = up.get_triangulation()
        out["p_FinG"][a:b], out["p_FinA"][a:b] = tri["p_FinG"], tri["p_FinA"]
    out.update(up.get_state(P=False))
    out["kernels"], out["batches"] = kernels, up.debug_option("slam_fused_batches")
    up.close()
    return out


def test_chunks_equal_the_chain_at_level_two(Updater, oracle):
    """FIRST_5 = [0, 9, 9, 22, 38, 50] on the six representations in turn: every non-empty chunk holds a single-depth landmark and takes kernel 5"""
    opts = capi.default_options(chi2_multipler=1.0)
    q = _batch(s2.chunk_problem())
    out, up = chunked(at_level(Updater, 2), opts, q, s2.FIRST_5, keep=True)
    assert up.debug_option("last_feature_kernel") == 5 and up.debug_option("slam_fused_batches") == 4  # four non-empty chunks
    up.close()
    ref = chain_kernels(at_level(Updater, 2), opts, q, s2.FIRST_5)
    assert ref["kernels"] == [5, 5, 5, 5] and ref["batches"] == 4
    del ref["kernels"], ref["batches"]
    assert_equal_outputs(out, ref, "five chunks at level 2 against the chain at level 2")
    assert sum(s["n_used"] for s in out["stats"] if s) >= 30
    # ... the general kernel's pass: the same accept set, the bounds
    off = chunked(at_level(Updater, 0), opts, q, s2.FIRST_5)
    assert np.array_equal(out["feat_status"], off["feat_status"])
    assert [s["n_rows"] if s else 0 for s in out["stats"]] == [s["n_rows"] if s else 0 for s in off["stats"]]
    dev = dict(dx=max(_rel(out["dx_seq"][k], off["dx_seq"][k]) for k in (0, 2, 3, 4)), P=_rel(out["P"], off["P"]),
               landmarks=np.abs(out["landmarks"] - off["landmarks"]).max(), poses=max(np.abs(out[k] - off[k]).max() for k in STATE_KEYS))
    print("five chunks, level 2 against level 0: " + "  ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    note("level-0 context", **dev)
    assert dev["dx"] < 10 * TOL_DX and dev["P"] < 10 * TOL_P and dev["landmarks"] < 1e-9 and dev["poses"] < 1e-9
    # ... and the oracle's chain
    assert_oracle(out, oracle_chain(oracle, opts, q, s2.FIRST_5), "five chunks at level 2")


# --------------------------------------------------------------------------- determinism
def test_same_bits_twice_from_reset_state(Updater):
    case = s2.BY_ID["mix-outliers"]
    first, up = run(Updater, case, 2, keep=True)
    up.reset_state()  # the prior and the pose tables; the landmarks the first call corrected are handed over again, then the batch
    capi.check(up.lib.ovgpu_set_landmarks(up._ctx, ctypes.byref(up._views.landmarks)), "ovgpu_set_landmarks")
    up.set_features(case.prob)
    second = up.slam_update(case.prob.lm_index)
    second.update(up.get_state(P=False))
    assert up.debug_option("last_feature_kernel") == 5 and up.debug_option("slam_fused_batches") == 2
    up.close()
    assert_equal_outputs(first, second, "the same call twice from ovgpu_reset_state at level 2", keys=OUT_KEYS)
    assert (first["feat_status"] == capi.FEAT_CHI2_REJECTED).any()


def test_zz_worst_deviations():
    """prints what the kernel-5 cases of this file measured (DESIGN.md section 7 quotes the figures)"""
    for (comparator, k), v in sorted(WORST.items()):
        print(f"k_slam_y<true> against the {comparator}: worst {k} {v:.3e}")
