"""GPU tests (`-m gpu`) of the LONG shape of the fused per-feature kernel of UpdaterSLAM::update — k_slam_y<.., 17, 32, 126>, tracks of 63 to
126 observations (csrc/k_slam_y.h), selected with ovgpu_debug_option "slam_fused" = 3 and off by default.

Comparators and bounds are tests/test_gpu_slam_fused.py's, imported: the oracle's slam_update and a second context of the same library with
"slam_fused" = 0 (the general kernel, k_system_t); 10 TOL_DX on dx, 10 TOL_P on P' (exactly symmetric), TOL_CHI2, 1e-9 on landmarks and poses;
accept sets, n_used and n_rows equal.  For every batch the ORACLE ALONE leaves no feature within parity_util.GATE_MARGIN of its threshold
(tests/test_slam_long_shapes_cpu.py, asserted again here on the oracle's own numbers).  Every case asserts "last_feature_kernel" against
slam_long_shapes' restatement of the level-3 rule; a batch the kernel does not take must return the switch-off context's BITS with
"slam_fused_batches" unchanged.  The batches and what each is named for: tests/slam_long_shapes.py.

A rejected feature's rows of the stack are not an output of the library: that the 252 rows of the rejected 126-observation track ARE zero is
held through what they would do — n_rows without them and dx, P' within the bounds of an oracle that never stacks them (a gross outlier's rows
left in the stack move dx by orders of magnitude more).

Worst deviations over the kernel-6 / kernel-7 cases, measured on the MI355X (every test prints its own; test_zz_worst_deviations the maxima):
against the oracle chi2 2.1e-13, dx 1.1e-12, P' 5.3e-14, landmarks 1.3e-13, poses 6.3e-13; against the switch-off context chi2 2.2e-13,
dx 4.1e-13, P' 5.4e-14, landmarks 9.2e-14, poses 2.8e-13.
"""
import copy
import ctypes

import numpy as np
import pytest

import slam_long_shapes as s3
import test_gpu_slam_fused as tf
from open_vins_amd import capi, synth
from test_gpu_parity import TOL_DX, TOL_P
from test_gpu_slam_chunked import assert_equal_outputs, chain, chunked

pytestmark = pytest.mark.gpu

STATE_KEYS, OUT_KEYS = tf.STATE_KEYS, tf.OUT_KEYS
WORST = {}  # (comparator, quantity) -> largest deviation over the kernel-6 / kernel-7 cases run so far
_rel, run, switched = tf._rel, tf.run, tf.switched


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _note(comparator, a, b, post=None):
    gate = np.isfinite(b["chi2"])
    dev = dict(chi2=np.abs(a["chi2"][gate] / b["chi2"][gate] - 1.0).max(), dx=_rel(a["dx"], b["dx"]), P=_rel(a["P"], b["P"]),
               landmarks=np.abs(a["landmarks"] - b["landmarks"]).max(), poses=max(np.abs(a[k] - (post or b)[k]).max() for k in STATE_KEYS))
    for k, v in dev.items():
        WORST[(comparator, k)] = max(WORST.get((comparator, k), 0.0), float(v))


_OFF = {}


def off_run(Updater, case):
    """the switch-off context's outputs of a case: computed once, shared, left unchanged"""
    if case.id not in _OFF:
        _OFF[case.id] = run(Updater, case, 0)
    return _OFF[case.id]


def check_case(Updater, oracle, case, level=3):
    """kernel as the rule says; kernel 4 .. 7: oracle + switch-off context within the bounds; kernel 0: the switch-off context's bits, counter unchanged"""
    ref = s3.oracle_run(oracle, case)
    on, off = run(Updater, case, level), off_run(Updater, case)
    assert off["kernel"] == 0 and off["batches"] == 0
    assert on["kernel"] == case.kernel_at(level), (case.id, on["kernel"])
    if on["kernel"]:
        assert on["batches"] == 1
        tf.check_oracle(oracle, case, on, ref, case.id)
        tf.check_pair(on, off, case.id)
        if on["kernel"] >= 6:
            _note("oracle", on, ref, oracle.apply_dx(case.opts(), capi.Views(case.prob), ref["dx"]))
            _note("switch-off context", on, off)
    else:
        assert on["batches"] == 0
        assert_equal_outputs(on, off, f"{case.id}: kernel 0 against the switch-off context", keys=OUT_KEYS)
        tf.check_oracle(oracle, case, on, ref, case.id)
    return on, off, ref


# --------------------------------------------------------------------------- track lengths: the first long one, the lane and tile-row edges, the bound
@pytest.mark.parametrize("cid", [c.id for c in s3.CASES if c.group == "len"])
def test_track_lengths(Updater, oracle, cid):
    case = s3.BY_ID[cid]
    on, off, ref = check_case(Updater, oracle, case)
    single = (case.reps_observed == s3.SINGLE).any()
    assert on["kernel"] == ((7 if single else 6) if case.m_max <= s3.BOUND_LONG else 0)
    m = np.diff(case.prob.meas_offsets)
    assert (on["feat_status"][m == 0] == capi.FEAT_TOO_FEW_MEAS).all() and (m == 0).sum() == 1
    assert on["feat_status"][case.rejected] == capi.FEAT_CHI2_REJECTED and (on["feat_status"] == capi.FEAT_CHI2_REJECTED).sum() == 1
    assert on["feat_status"][int(np.argmax(m))] == capi.FEAT_USED


# --------------------------------------------------------------------------- the outlier on the 126-observation track
@pytest.mark.parametrize("cid", ["outlier-long-3dof", "outlier-long-single"])
def test_outlier_on_the_long_track(Updater, oracle, cid):
    case = s3.BY_ID[cid]
    on, off, ref = check_case(Updater, oracle, case)
    assert on["kernel"] == (7 if cid.endswith("single") else 6)
    assert on["feat_status"][0] == capi.FEAT_CHI2_REJECTED and on["chi2"][0] > 20 * on["chi2_thresh"][0]
    m = np.diff(case.prob.meas_offsets)
    single = case.reps_observed == s3.SINGLE
    used = on["feat_status"] == capi.FEAT_USED
    assert used.sum() == 4 and on["stats"]["n_rows"] == int(np.where(single, 2 * m - 2, 2 * m)[used].sum()) < 2 * 126


# --------------------------------------------------------------------------- every track long; long and short tracks on the long shape
@pytest.mark.parametrize("cid", [c.id for c in s3.CASES if c.group == "mix"])
def test_mixed_lengths(Updater, oracle, cid):
    case = s3.BY_ID[cid]
    on, _, _ = check_case(Updater, oracle, case)
    assert on["kernel"] == (7 if cid.endswith("single") else 6)
    if case.rejected is not None:
        assert on["feat_status"][case.rejected] == capi.FEAT_CHI2_REJECTED and (on["feat_status"] == capi.FEAT_USED).sum() == 5
    else:
        assert (on["feat_status"] == capi.FEAT_USED).all()


# --------------------------------------------------------------------------- the sweep's last column block, and the first column count beyond the route
@pytest.mark.parametrize("cid", ["col-383", "col-384"])
def test_columns(Updater, oracle, cid):
    case = s3.BY_ID[cid]
    on, _, _ = check_case(Updater, oracle, case)
    assert on["stats"]["D"] == case.D
    assert on["kernel"] == (6 if case.D <= 383 else 0)


# --------------------------------------------------------------------------- per-feature noise and multiplier
def test_feature_noise_and_multiplier(Updater, oracle):
    case = s3.BY_ID["noise"]
    on, _, _ = check_case(Updater, oracle, case)
    assert on["kernel"] == 7 and on["feat_status"][case.rejected] == capi.FEAT_CHI2_REJECTED
    plain = copy.copy(case)
    plain.sigma = plain.mult = None
    alt = run(Updater, plain, 3)
    gate = np.isfinite(on["chi2"])  # sigma_f enters S0 and the stack, the multiplier the threshold: both move with the per-feature options
    assert alt["kernel"] == 7 and np.array_equal(np.isfinite(alt["chi2"]), gate) and gate.sum() == 5
    assert (alt["chi2"][gate] != on["chi2"][gate]).sum() >= 4 and (alt["chi2_thresh"][gate] != on["chi2_thresh"][gate]).sum() >= 3


# --------------------------------------------------------------------------- the levels
def test_the_levels(Updater, oracle):
    long3, long1 = s3.BY_ID["len-3dof-63"], s3.BY_ID["len-single-63"]
    up = Updater(long3.opts())
    assert up.debug_option("slam_fused") == 0                                              # the default stays 0
    assert up.debug_option("slam_fused", 3) == 0 and up.debug_option("slam_fused") == 3    # reads back 3
    assert up.debug_option("slam_fused", 9) == 3 and up.debug_option("slam_fused") == 3    # values above 3 are taken as 3
    up.close()
    for case, kernel in ((long3, 6), (long1, 7)):
        three, two, one, off = run(Updater, case, 3), run(Updater, case, 2), run(Updater, case, 1), off_run(Updater, case)
        assert three["kernel"] == kernel and three["batches"] == 1
        for low in (two, one):  # 63 observations fall back at levels 1 and 2, with the switch-off context's bits
            assert low["kernel"] == 0 and low["batches"] == 0
            assert_equal_outputs(low, off, f"{case.id} below level 3 against the switch-off context", keys=OUT_KEYS)
    never = run(Updater, long3, None)
    assert never["kernel"] == 0 and never["batches"] == 0
    assert_equal_outputs(never, off_run(Updater, long3), "never set against slam_fused = 0", keys=OUT_KEYS)


@pytest.mark.parametrize("cid,kernel", [("short-3dof", 4), ("short-single", 5)])
def test_sixty_observations_take_the_short_shapes_at_level_three(Updater, oracle, cid, kernel):
    case = s3.BY_ID[cid]
    three, two = run(Updater, case, 3), run(Updater, case, 2)
    assert three["kernel"] == two["kernel"] == kernel and three["batches"] == two["batches"] == 1
    assert_equal_outputs(three, two, f"{cid}: level 3 against level 2", keys=OUT_KEYS)
    tf.check_oracle(oracle, case, three, s3.oracle_run(oracle, case), cid)


# --------------------------------------------------------------------------- fall-backs at level 3 with a long batch
@pytest.mark.parametrize("cid", ["fb-general", "fb-tsqr", "fb-semi-definite"])
def test_fall_backs(Updater, oracle, cid):
    case = s3.BY_ID[cid]
    on, off, ref = check_case(Updater, oracle, case)
    assert on["kernel"] == 0 and on["batches"] == 0 and on["stats"]["status"] == 0
    if cid == "fb-semi-definite":  # repeated through the Householder route: the landmarks moved ONCE, not twice
        assert np.abs(on["landmarks"] - ref["landmarks"]).max() < 1e-9 < np.abs(ref["landmarks"] - case.prob.lm_value).max()


def test_mode_a_keeps_the_general_kernel(Updater):
    case = s3.BY_ID["fb-mode-a"]
    on, off = run(Updater, case, 3), run(Updater, case, 0)
    assert on["kernel"] == 0 and on["batches"] == 0 and on["rows"] == off["rows"] and on["D"] == off["D"]
    for k in ("feat_status", "chi2", "chi2_thresh", "H", "r", "col_cov_id"):
        assert np.array_equal(on[k], off[k], equal_nan=True), k


# --------------------------------------------------------------------------- chunks
def _batch(p):
    q = p.subset(np.arange(p.F))
    q.lm_index = np.arange(p.F, dtype=np.int32)
    return q


def test_chunks_equal_the_chain_at_level_three(Updater):
    """CHUNK_FIRST = [0, 3, 3, 6] on the "all-long-single" batch: chunk 0 holds the single-depth 126-observation track (kernel 7), chunk 2 the
    second single-depth landmark, 80 observations (kernel 7 as well)"""
    opts = capi.default_options(chi2_multipler=1.0)
    q = _batch(s3.chunk_problem())
    out, up = chunked(switched(Updater, 3), opts, q, s3.CHUNK_FIRST, keep=True)
    ref, up2 = chain(switched(Updater, 3), opts, q, s3.CHUNK_FIRST, keep=True)
    for u in (up, up2):
        assert u.debug_option("last_feature_kernel") == 7 and u.debug_option("slam_fused_batches") == 2  # two non-empty chunks
        u.close()
    assert_equal_outputs(out, ref, "three chunks at level 3 against the chain at level 3")
    off = chunked(switched(Updater, 0), opts, q, s3.CHUNK_FIRST)
    assert np.array_equal(out["feat_status"], off["feat_status"]) and (out["feat_status"] == capi.FEAT_USED).sum() == 5
    dev = dict(dx=max(_rel(out["dx_seq"][k], off["dx_seq"][k]) for k in (0, 2)), P=_rel(out["P"], off["P"]),
               landmarks=np.abs(out["landmarks"] - off["landmarks"]).max(), poses=max(np.abs(out[k] - off[k]).max() for k in STATE_KEYS))
    print("three chunks, level 3 against level 0: " + "  ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    assert dev["dx"] < 10 * TOL_DX and dev["P"] < 10 * TOL_P and dev["landmarks"] < 1e-9 and dev["poses"] < 1e-9


def test_one_chunk_is_the_single_call(Updater):
    opts = capi.default_options(chi2_multipler=1.0)
    q = _batch(s3.BY_ID["all-long"].prob)
    out, up0 = chunked(switched(Updater, 3), opts, q, [0, 6], keep=True)
    assert up0.debug_option("last_feature_kernel") == 6
    up0.close()
    up = switched(Updater, 3)(opts)
    up.set_slam_problem(q)
    up.set_active_landmarks(np.unique(q.lm_index))
    up.set_features(q)
    one = up.slam_update()
    assert up.debug_option("last_feature_kernel") == 6
    one.update(up.get_state(P=False))
    up.close()
    one["dx_seq"] = one["dx"][None, :]
    assert_equal_outputs(out, one, "n_chunks = 1 against ovgpu_slam_update at level 3")


# --------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("cid,kernel", [("all-long", 6), ("all-long-single", 7)])
def test_same_bits_twice_from_reset_state(Updater, cid, kernel):
    case = s3.BY_ID[cid]
    first, up = run(Updater, case, 3, keep=True)
    up.reset_state()  # the prior and the pose tables; the landmarks the first call corrected are handed over again, then the batch
    capi.check(up.lib.ovgpu_set_landmarks(up._ctx, ctypes.byref(up._views.landmarks)), "ovgpu_set_landmarks")
    up.set_features(case.prob)
    second = up.slam_update(case.prob.lm_index)
    second.update(up.get_state(P=False))
    assert up.debug_option("last_feature_kernel") == kernel and up.debug_option("slam_fused_batches") == 2
    up.close()
    assert_equal_outputs(first, second, "the same call twice from ovgpu_reset_state at level 3", keys=OUT_KEYS)
    assert (first["feat_status"] == capi.FEAT_CHI2_REJECTED).any()


# --------------------------------------------------------------------------- what a long fused update leaves behind
def test_state_left_behind(Updater):
    """a second SLAM batch on the same context, then ovgpu_msckf_update_lm behind it: the level-3 context against the switch-off one"""
    case = s3.BY_ID["stride-single"]
    p = case.prob
    tracks = synth.make_problem(2, F=40, seed=p.seed, **s3.RIG)  # the same window (the state stream follows the seed), forty tracks
    msckf = copy.copy(p)
    for k in ("meas_offsets", "uv", "uvn", "clone_idx", "cam_idx", "p_FinG_true"):
        setattr(msckf, k, getattr(tracks, k))
    res = []
    for level in (3, 0):
        first, up = run(Updater, case, level, keep=True)
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
    assert (a1["kernel"], a2["kernel"]) == (7, 7) and (b1["kernel"], b2["kernel"]) == (0, 0) and a3["kernel"] == b3["kernel"] and a3["kernel"] not in (4, 5, 6, 7)
    tf.check_pair(a2, b2, "the second SLAM batch")
    assert a2["stats"]["n_used"] >= 5 and np.abs(a2["landmarks"] - a1["landmarks"]).max() > 0
    assert np.array_equal(a3["feat_status"], b3["feat_status"]) and a3["stats"]["n_used"] >= 20
    dev = dict(dx=_rel(a3["dx"], b3["dx"]), P=_rel(a3["P"], b3["P"]), landmarks=np.abs(a3["landmarks"] - b3["landmarks"]).max(),
               poses=max(np.abs(a3[k] - b3[k]).max() for k in STATE_KEYS))
    print("ovgpu_msckf_update_lm behind the SLAM updates, level 3 against switch off: " + "  ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    assert dev["dx"] < 10 * TOL_DX and dev["P"] < 10 * TOL_P and np.array_equal(a3["P"], a3["P"].T) and dev["landmarks"] < 1e-9 and dev["poses"] < 1e-9


def test_zz_worst_deviations():
    """prints what the kernel-6 / kernel-7 cases of this file measured (DESIGN.md section 7 quotes the figures)"""
    for (comparator, k), v in sorted(WORST.items()):
        print(f"k_slam_y, long shape, against the {comparator}: worst {k} {v:.3e}")
