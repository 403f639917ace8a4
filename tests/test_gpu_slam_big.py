"""GPU tests (`-m gpu`) of the BLOCK-ROW shape of the fused per-feature kernel of UpdaterSLAM::update — k_slam_y_big, tracks of 127 to 232
observations (csrc/k_slam_y_big.h), selected with ovgpu_debug_option "slam_fused_big" = 1 under "slam_fused" = 3 and off by default.

Comparators and bounds are tests/test_gpu_slam_fused.py's, imported and unchanged: the oracle's slam_update and a second context of the same
library with "slam_fused" = 0 (the general kernel, k_system_t); TOL_CHI2 = 1e-8 on chi2, 10 TOL_DX = 1e-7 on dx, 10 TOL_P = 1e-8 on P' (exactly
symmetric), 1e-9 on landmarks and poses; accept sets, n_used and n_rows equal.  For every batch the ORACLE ALONE leaves no feature within
parity_util.GATE_MARGIN of its threshold (tests/test_slam_big_shapes_cpu.py, asserted again here on the oracle's own numbers).  Every case
asserts "last_feature_kernel" against slam_big_shapes' restatement of the rule; a batch the kernel does not take must return the switch-off
context's BITS with "slam_fused_batches" unchanged, a batch of at most 126 observations the level-3 context's bits.  The batches and what each
is named for: tests/slam_big_shapes.py.

A rejected feature's rows of the stack are not an output of the library: that the 464 rows of the rejected 232-observation track ARE zero is
held through what they would do — n_rows without them and dx, P' within the bounds of an oracle that never stacks them.

On a library without the switch every kernel-8 / 9 assertion and the read-back of "slam_fused_big" fail: the name is unknown there.
Every test prints its deviations before it asserts; test_zz_worst_deviations the maxima over the kernel-8 / 9 cases.

Worst deviations over the kernel-8 / kernel-9 cases, measured on the MI355X: against the oracle chi2 1.5e-13, dx 1.1e-12, P' 5.3e-14, landmarks
4.7e-13, poses 9.1e-13; against the switch-off context chi2 1.3e-13, dx 4.2e-13, P' 4.7e-14, landmarks 6.8e-14, poses 3.4e-13.  61 tests in 26 s,
the slowest (every track beyond 126 observations: two contexts and the oracle) 4 s.
"""
import copy
import ctypes

import numpy as np
import pytest

import slam_big_shapes as sb
import test_gpu_slam_fused as tf
import test_gpu_slam_mode_a as tm
from open_vins_amd import capi, synth
from test_gpu_parity import TOL_CHI2, TOL_DX, TOL_P
from test_gpu_slam_chunked import assert_equal_outputs, chain, chunked

pytestmark = pytest.mark.gpu

STATE_KEYS, OUT_KEYS = tf.STATE_KEYS, tf.OUT_KEYS
WORST = {}  # (comparator, quantity) -> largest deviation over the kernel-8 / kernel-9 cases run so far
_rel, run, switched = tf._rel, tf.run, tf.switched


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def with_big(Updater, big=1, **debug):
    """an Updater factory whose contexts have "slam_fused_big" (and further switches) set before anything is uploaded; big = None never names it"""
    def make(opts):
        up = Updater(opts)
        if big is not None:
            up.debug_option("slam_fused_big", big)
        for name, val in debug.items():
            up.debug_option(name, val)
        return up
    return make


def _note(comparator, a, b, post=None):
    gate = np.isfinite(b["chi2"])
    dev = dict(chi2=np.abs(a["chi2"][gate] / b["chi2"][gate] - 1.0).max(), dx=_rel(a["dx"], b["dx"]), P=_rel(a["P"], b["P"]),
               landmarks=np.abs(a["landmarks"] - b["landmarks"]).max(), poses=max(np.abs(a[k] - (post or b)[k]).max() for k in STATE_KEYS))
    for k, v in dev.items():
        WORST[(comparator, k)] = max(WORST.get((comparator, k), 0.0), float(v))


_OFF = {}


def off_run(Updater, case, **debug):
    """the switch-off context's outputs of a case: computed once, shared, left unchanged"""
    key = (case.id,) + tuple(sorted(debug.items()))
    if key not in _OFF:
        _OFF[key] = run(with_big(Updater, None, **debug), case, 0)
    return _OFF[key]


def check_case(Updater, oracle, case, level=3, big=1, max_d=sb.GRAM_MAX_D, **debug):
    """kernel as the rule says; kernel 4 .. 9: oracle + switch-off context within the bounds; kernel 0: the switch-off context's bits, counter unchanged"""
    ref = sb.oracle_run(oracle, case)
    on, off = run(with_big(Updater, big, **debug), case, level), off_run(Updater, case, **debug)
    assert off["kernel"] == 0 and off["batches"] == 0
    assert on["kernel"] == case.kernel_at(level, big, max_d), (case.id, on["kernel"])
    if on["kernel"]:
        assert on["batches"] == 1
        tf.check_oracle(oracle, case, on, ref, case.id)
        tf.check_pair(on, off, case.id)
        if on["kernel"] >= 8:
            _note("oracle", on, ref, oracle.apply_dx(case.opts(), capi.Views(case.prob), ref["dx"]))
            _note("switch-off context", on, off)
    else:
        assert on["batches"] == 0
        assert_equal_outputs(on, off, f"{case.id}: kernel 0 against the switch-off context", keys=OUT_KEYS)
        tf.check_oracle(oracle, case, on, ref, case.id)
    return on, off, ref


# --------------------------------------------------------------------------- track lengths: level 3's bound, the first big one, the tile-row and pass edges, the bound
@pytest.mark.parametrize("cid", [c.id for c in sb.CASES if c.group == "len"])
def test_track_lengths(Updater, oracle, cid):
    case = sb.BY_ID[cid]
    on, off, ref = check_case(Updater, oracle, case)
    single = (case.reps_observed == sb.SINGLE).any()
    want = (7 if single else 6) if case.m_max <= sb.BOUND_LONG else ((9 if single else 8) if case.m_max <= sb.BOUND_BIG else 0)
    assert on["kernel"] == want
    m = np.diff(case.prob.meas_offsets)
    assert (on["feat_status"][m == 0] == capi.FEAT_TOO_FEW_MEAS).all() and (m == 0).sum() == 1
    assert on["feat_status"][case.rejected] == capi.FEAT_CHI2_REJECTED and (on["feat_status"] == capi.FEAT_CHI2_REJECTED).sum() == 1
    assert on["feat_status"][int(np.argmax(m))] == capi.FEAT_USED
    if case.m_max <= sb.BOUND_LONG:  # level 3's kernel and its bits, whatever "slam_fused_big" says
        three = run(with_big(Updater, None), case, 3)
        assert three["kernel"] == want and three["batches"] == 1
        assert_equal_outputs(on, three, f"{cid}: slam_fused_big = 1 against level 3 alone", keys=OUT_KEYS)


@pytest.mark.parametrize("cid", ["beyond-3dof", "beyond-single"])
def test_one_observation_beyond_the_bound_keeps_the_whole_batch_general(Updater, oracle, cid):
    on, _, _ = check_case(Updater, oracle, sb.BY_ID[cid])
    assert on["kernel"] == 0 and on["batches"] == 0


# --------------------------------------------------------------------------- the outlier on the 232-observation track
@pytest.mark.parametrize("cid", ["outlier-big-3dof", "outlier-big-single"])
def test_outlier_on_the_longest_track(Updater, oracle, cid):
    case = sb.BY_ID[cid]
    on, off, ref = check_case(Updater, oracle, case)
    assert on["kernel"] == (9 if cid.endswith("single") else 8)
    assert on["feat_status"][0] == capi.FEAT_CHI2_REJECTED and on["chi2"][0] > 20 * on["chi2_thresh"][0]
    m = np.diff(case.prob.meas_offsets)
    single = case.reps_observed == sb.SINGLE
    used = on["feat_status"] == capi.FEAT_USED
    assert used.sum() == 3 and on["stats"]["n_rows"] == int(np.where(single, 2 * m - 2, 2 * m)[used].sum()) < 2 * 232


# --------------------------------------------------------------------------- every track big; long and short tracks on the big shape; configs[4]'s rig
@pytest.mark.parametrize("cid", [c.id for c in sb.CASES if c.group in ("mix", "rigb")])
def test_mixed_lengths(Updater, oracle, cid):
    case = sb.BY_ID[cid]
    on, _, _ = check_case(Updater, oracle, case)
    assert on["kernel"] == (9 if cid.endswith("single") else 8)
    if case.rejected is not None:
        assert on["feat_status"][case.rejected] == capi.FEAT_CHI2_REJECTED
        assert (on["feat_status"] == capi.FEAT_USED).sum() == (4 if case.group == "rigb" else 5)
    else:
        assert (on["feat_status"] == capi.FEAT_USED).all()


# --------------------------------------------------------------------------- the sweep's twelfth column block, and the first column count beyond the route
def test_383_columns(Updater, oracle):
    case = sb.BY_ID["col-383"]
    on, _, _ = check_case(Updater, oracle, case)
    assert on["stats"]["D"] == 383 and on["kernel"] == 8


def test_384_columns(Updater, oracle):
    case = sb.BY_ID["col-384"]
    on, _, _ = check_case(Updater, oracle, case)
    assert on["stats"]["D"] == 384 and on["kernel"] == 0
    wide, _, _ = check_case(Updater, oracle, case, max_d=511, gram_wide=1)  # both contexts on the wide Gram route
    assert wide["stats"]["D"] == 384 and wide["kernel"] == 9


# --------------------------------------------------------------------------- per-feature noise and multiplier
def test_feature_noise_and_multiplier(Updater, oracle):
    case = sb.BY_ID["noise"]
    on, _, _ = check_case(Updater, oracle, case)
    assert on["kernel"] == 9 and on["feat_status"][case.rejected] == capi.FEAT_CHI2_REJECTED
    plain = copy.copy(case)
    plain.sigma = plain.mult = None
    alt = run(with_big(Updater), plain, 3)
    gate = np.isfinite(on["chi2"])  # sigma_f enters S0 and the stack, the multiplier the threshold: both move with the per-feature options
    assert alt["kernel"] == 9 and np.array_equal(np.isfinite(alt["chi2"]), gate) and gate.sum() == 5
    assert (alt["chi2"][gate] != on["chi2"][gate]).sum() >= 4 and (alt["chi2_thresh"][gate] != on["chi2_thresh"][gate]).sum() >= 3


# --------------------------------------------------------------------------- the levels
def test_the_levels(Updater, oracle):
    big3, big1 = sb.BY_ID["len-3dof-127"], sb.BY_ID["len-single-127"]
    up = Updater(big3.opts())
    assert up.debug_option("slam_fused_big") == 0                                                  # the default stays 0
    assert up.debug_option("slam_fused_big", 1) == 0 and up.debug_option("slam_fused_big") == 1    # reads back 1
    assert up.debug_option("slam_fused_big", 9) == 1 and up.debug_option("slam_fused_big") == 1    # 9 is taken as 1
    assert up.debug_option("slam_fused") == 0 and up.debug_option("slam_fused", 9) == 0 and up.debug_option("slam_fused") == 3
    up.close()
    for case, kernel in ((big3, 8), (big1, 9)):
        nine, two, off = run(with_big(Updater, 9), case, 3), run(with_big(Updater, 1), case, 2), off_run(Updater, case)
        assert nine["kernel"] == kernel and nine["batches"] == 1
        assert two["kernel"] == 0 and two["batches"] == 0                                          # it acts only when "slam_fused" is at 3
        assert_equal_outputs(two, off, f"{case.id}: slam_fused_big under level 2 against the switch-off context", keys=OUT_KEYS)
        zero = run(with_big(Updater, 0), case, 3)
        assert zero["kernel"] == 0 and zero["batches"] == 0
        assert_equal_outputs(zero, off, f"{case.id}: slam_fused_big = 0 at level 3 against the switch-off context", keys=OUT_KEYS)
    never = run(with_big(Updater, None), big3, 3)
    assert never["kernel"] == 0 and never["batches"] == 0
    assert_equal_outputs(never, off_run(Updater, big3), "never set against the switch-off context", keys=OUT_KEYS)


@pytest.mark.parametrize("cid,kernel", [("short-60-3dof", 4), ("short-60-single", 5), ("short-100-3dof", 6), ("short-100-single", 7)])
def test_sixty_and_a_hundred_observations_keep_level_three_s_bits(Updater, oracle, cid, kernel):
    case = sb.BY_ID[cid]
    big, three = run(with_big(Updater, 1), case, 3), run(with_big(Updater, None), case, 3)
    assert big["kernel"] == three["kernel"] == kernel and big["batches"] == three["batches"] == 1
    assert_equal_outputs(big, three, f"{cid}: slam_fused_big = 1 against level 3 alone", keys=OUT_KEYS)
    tf.check_oracle(oracle, case, big, sb.oracle_run(oracle, case), cid)


# --------------------------------------------------------------------------- fall-backs with a 200-observation batch
@pytest.mark.parametrize("cid", ["fb-general", "fb-tsqr", "fb-semi-definite"])
def test_fall_backs(Updater, oracle, cid):
    case = sb.BY_ID[cid]
    on, off, ref = check_case(Updater, oracle, case)
    assert on["kernel"] == 0 and on["batches"] == 0 and on["stats"]["status"] == 0
    if cid == "fb-semi-definite":  # repeated through the Householder route: the landmarks moved ONCE, not twice
        assert np.abs(on["landmarks"] - ref["landmarks"]).max() < 1e-9 < np.abs(ref["landmarks"] - case.prob.lm_value).max()


# --------------------------------------------------------------------------- mode A
@pytest.mark.parametrize("cid,kernel", [("mode-a-3dof", 8), ("mode-a-single", 9)])
def test_mode_a_takes_the_big_shape_under_slam_mode_a_only(Updater, cid, kernel):
    case = sb.BY_ID[cid]
    opts = case.opts()
    house = tm.compress(Updater, case.prob, opts, 0)
    plain = tm.compress(Updater, case.prob, opts, None, slam_fused=3, slam_fused_big=1)
    assert house["kernel"] == plain["kernel"] == 0 and plain["fused_batches"] == 0     # without "slam_mode_a": the general kernel, the Householder leg's bits
    tm.assert_same_bits(plain, house, f"{cid}: ovgpu_slam_compress without slam_mode_a")
    on = tm.compress(Updater, case.prob, opts, 1, slam_fused=3, slam_fused_big=1)
    assert on["kernel"] == kernel and on["fused_batches"] == 1 and on["count"] == 1 and on["ran"][0] == capi.COMPRESS_PCHOLQR
    assert np.array_equal(on["feat_status"], house["feat_status"]) and (on["feat_status"] == capi.FEAT_USED).sum() == 4
    gate = np.isfinite(house["chi2"])
    echi = np.abs(on["chi2"][gate] / house["chi2"][gate] - 1.0).max()
    eG, eg = _rel(on["H"].T @ on["H"], house["H"].T @ house["H"]), _rel(on["H"].T @ on["r"], house["H"].T @ house["r"])
    print(f"{cid}: mode A behind kernel {on['kernel']} against the Householder leg: rows {on['rows']} | {house['rows']}, chi2 {echi:.3e}, eG {eG:.3e}, eg {eg:.3e}")
    assert np.isfinite(on["H"]).all() and on["D"] == house["D"] == case.columns and 0 < on["rows"] <= case.columns
    assert echi < TOL_CHI2 and eG < tm.TOL_G and eg < tm.TOL_g


# --------------------------------------------------------------------------- chunks
def _batch(p):
    q = p.subset(np.arange(p.F))
    q.lm_index = np.arange(p.F, dtype=np.int32)
    return q


def test_chunks_equal_the_chain(Updater):
    """CHUNK_FIRST = [0, 3, 3, 6] on the "all-big-single" batch: chunk 0 holds the single-depth 232-observation track (kernel 9), chunk 2 the
    second single-depth landmark, 129 observations (kernel 9 as well)"""
    opts = sb.BY_ID["all-big-single"].opts()
    q = _batch(sb.chunk_problem())
    out, up = chunked(switched(with_big(Updater), 3), opts, q, sb.CHUNK_FIRST, keep=True)
    ref, up2 = chain(switched(with_big(Updater), 3), opts, q, sb.CHUNK_FIRST, keep=True)
    for u in (up, up2):
        assert u.debug_option("last_feature_kernel") == 9 and u.debug_option("slam_fused_batches") == 2  # two non-empty chunks
        u.close()
    assert_equal_outputs(out, ref, "three chunks on the big shape against the chain of single calls")
    off = chunked(switched(Updater, 0), opts, q, sb.CHUNK_FIRST)
    assert np.array_equal(out["feat_status"], off["feat_status"]) and (out["feat_status"] == capi.FEAT_USED).sum() == 5
    dev = dict(dx=max(_rel(out["dx_seq"][k], off["dx_seq"][k]) for k in (0, 2)), P=_rel(out["P"], off["P"]),
               landmarks=np.abs(out["landmarks"] - off["landmarks"]).max(), poses=max(np.abs(out[k] - off[k]).max() for k in STATE_KEYS))
    print("three chunks, the big shape against the switch-off context: " + "  ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    assert dev["dx"] < 10 * TOL_DX and dev["P"] < 10 * TOL_P and dev["landmarks"] < 1e-9 and dev["poses"] < 1e-9


def test_one_chunk_is_the_single_call(Updater):
    case = sb.BY_ID["all-big-3dof"]
    opts = case.opts()
    q = _batch(case.prob)
    out, up0 = chunked(switched(with_big(Updater), 3), opts, q, [0, 6], keep=True)
    assert up0.debug_option("last_feature_kernel") == 8
    up0.close()
    up = switched(with_big(Updater), 3)(opts)
    up.set_slam_problem(q)
    up.set_active_landmarks(np.unique(q.lm_index))
    up.set_features(q)
    one = up.slam_update()
    assert up.debug_option("last_feature_kernel") == 8
    one.update(up.get_state(P=False))
    up.close()
    one["dx_seq"] = one["dx"][None, :]
    assert_equal_outputs(out, one, "n_chunks = 1 against ovgpu_slam_update on the big shape")


# --------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("cid,kernel", [("all-big-3dof", 8), ("all-big-single", 9)])
def test_same_bits_twice_from_reset_state(Updater, cid, kernel):
    case = sb.BY_ID[cid]
    first, up = run(with_big(Updater), case, 3, keep=True)
    up.reset_state()  # the prior and the pose tables; the landmarks the first call corrected are handed over again, then the batch
    capi.check(up.lib.ovgpu_set_landmarks(up._ctx, ctypes.byref(up._views.landmarks)), "ovgpu_set_landmarks")
    up.set_features(case.prob)
    second = up.slam_update(case.prob.lm_index)
    second.update(up.get_state(P=False))
    assert up.debug_option("last_feature_kernel") == kernel and up.debug_option("slam_fused_batches") == 2
    up.close()
    assert_equal_outputs(first, second, "the same call twice from ovgpu_reset_state on the big shape", keys=OUT_KEYS)
    assert (first["feat_status"] == capi.FEAT_CHI2_REJECTED).any()


# --------------------------------------------------------------------------- what a big fused update leaves behind
def test_state_left_behind(Updater):
    """a second SLAM batch on the same context, then ovgpu_msckf_update_lm behind it: the big-shape context against the switch-off one"""
    case = sb.BY_ID["rig-b-single"]
    p = case.prob
    tracks = synth.make_problem(2, F=40, seed=p.seed, **sb.RIG_B)  # the same window (the state stream follows the seed), forty tracks
    msckf = copy.copy(p)
    for k in ("meas_offsets", "uv", "uvn", "clone_idx", "cam_idx", "p_FinG_true"):
        setattr(msckf, k, getattr(tracks, k))
    res = []
    for level, big in ((3, 1), (0, None)):
        first, up = run(with_big(Updater, big), case, level, keep=True)
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
    assert (a1["kernel"], a2["kernel"]) == (9, 9) and (b1["kernel"], b2["kernel"]) == (0, 0) and a3["kernel"] == b3["kernel"] and a3["kernel"] not in (4, 5, 6, 7, 8, 9)
    tf.check_pair(a2, b2, "the second SLAM batch")
    assert a2["stats"]["n_used"] >= 4 and np.abs(a2["landmarks"] - a1["landmarks"]).max() > 0
    assert np.array_equal(a3["feat_status"], b3["feat_status"]) and a3["stats"]["n_used"] >= 20
    dev = dict(dx=_rel(a3["dx"], b3["dx"]), P=_rel(a3["P"], b3["P"]), landmarks=np.abs(a3["landmarks"] - b3["landmarks"]).max(),
               poses=max(np.abs(a3[k] - b3[k]).max() for k in STATE_KEYS))
    print("ovgpu_msckf_update_lm behind the SLAM updates, the big shape against switch off: " + "  ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    assert dev["dx"] < 10 * TOL_DX and dev["P"] < 10 * TOL_P and np.array_equal(a3["P"], a3["P"].T) and dev["landmarks"] < 1e-9 and dev["poses"] < 1e-9


def test_zz_worst_deviations():
    """prints what the kernel-8 / kernel-9 cases of this file measured (DESIGN.md section 7 quotes the figures)"""
    for (comparator, k), v in sorted(WORST.items()):
        print(f"k_slam_y_big against the {comparator}: worst {k} {v:.3e}")
