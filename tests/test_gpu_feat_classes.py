"""ovgpu_debug_option "feat_classes" on the device (run with `-m gpu` on an MI355X): an MSCKF batch of mixed track lengths served by a per-feature
kernel per length class, each track on the smallest shape that holds it.

The batches are tests/class_shapes.py's (shown non-vacuous on the oracle alone by tests/test_class_shapes_cpu.py); the oracle's triangulation is
injected, as tests/test_gpu_track_edges.py does.  What the library must report — the classes launched, the features in each, the stack layout — is
restated there from the documented rule and never read back from the library.

  1. every case at level 1, gate_always_factor = 1, held to the ORACLE at that file's tolerances: chi2 1e-8, thresholds 1e-12, dx 1e-8, P 1e-9 and
     exactly symmetric, poses 1e-9, feat_status identical with no excuse; "last_feature_classes", the four "last_class_features_k" and
     "last_stack_raw" as restated, "feat_class_batches" advanced by one (by none for a batch of one class);
  2. a batch of one class: every output of level 1 equals level 0's bit for bit;
  3. level 0: one bit, the longest track's kernel;
  4. per-feature independence: the statistics of `two`'s short tracks at level 1 against the same tracks at level 0 in a batch without the long
     one — the same kernel and arithmetic, only the launch's carve and slot range differ — bit for bit;
  5. one leg each on `two`: the default gate (bound first), options.gram_fp32 (dx 1e-4, P 1e-3 as the suite holds that option), an anchored
     feat_rep_msckf, ovgpu_msckf_update_lm with landmarks resident under the empty active set (corrected once, exactly value + dx, as
     tests/test_gpu_msckf_lm.py checks), ovgpu_msckf_compress (H^T H 1e-11, H^T r 1e-10 against the oracle's, tests/test_gpu_mode_a_shapes.py's bounds);
     and "layout_every_update" = 1 on `three`, the batch with instance lists at both block widths;
  6. a loop-back set of two ranks on one device over `ragged-600` at level 1 against the single-context level-1 result at
     tests/test_gpu_shard_edges.py's bounds;
  7. options.feature_kernel_shape = 2 and "featy_big" = 1 rule the classes out: one bit, and level 0's results bit for bit.
Every leg prints a line `classes ...` with its deviations before it asserts."""
import copy
import ctypes as C

import numpy as np
import pytest

import class_shapes as cs
import shard_shapes as sh
from open_vins_amd import capi, synth
from parity_util import assert_chi2

pytestmark = pytest.mark.gpu

TOL_CHI2, TOL_THR, TOL_DX, TOL_P, TOL_POSE = 1e-8, 1e-12, 1e-8, 1e-9, 1e-9   # tests/test_gpu_track_edges.py's
TOL_DX_F32, TOL_P_F32 = 1e-4, 1e-3
TOL_G, TOL_g = 1e-11, 1e-10                                                 # tests/test_gpu_mode_a_shapes.py's
OUT_KEYS = ("feat_status", "chi2", "chi2_thresh", "p_FinG", "dx", "P", "clone_q_p", "calib_q_p", "intrinsics")
READ = ("last_feature_kernel", "last_stack_raw", "stack_is_f32", "last_feature_classes", "last_class_features_0", "last_class_features_1",
        "last_class_features_2", "last_class_features_3", "feat_class_batches")


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _reads(up):
    r = {n: up.debug_option(n) for n in READ}
    return dict(kernel=r["last_feature_kernel"], raw=r["last_stack_raw"], f32=r["stack_is_f32"], mask=r["last_feature_classes"],
                counts=[r[f"last_class_features_{k}"] for k in range(4)], batches=r["feat_class_batches"])


def _run(Updater, case, tri, level, prob=None, entry="update", opts=None, **debug):
    up = Updater(case.opts() if opts is None else opts)
    up.debug_option("feat_classes", level)
    for name, val in debug.items():
        up.debug_option(name, val)
    up.set_problem(case.prob if prob is None else prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    before = up.debug_option("feat_class_batches")
    out = getattr(up, entry)()
    out.update(_reads(up))
    out["batches"] -= before
    up.close()
    return out


def _inputs_hold(ref):
    """a leg with options of its own: the condition tests/test_class_shapes_cpu.py puts on the catalogue's inputs, on the oracle alone"""
    gate = np.isfinite(ref["chi2"])
    assert (ref["feat_status"] == capi.FEAT_USED).any() and gate.any()
    assert np.abs(ref["chi2"][gate] / ref["chi2_thresh"][gate] - 1.0).min() > 1e-6


def _hold_to_the_oracle(what, out, ref, strict=True, fp32=False):
    gate = np.isfinite(ref["chi2"])
    dchi = np.abs(out["chi2"][gate] / ref["chi2"][gate] - 1.0).max() if strict else float("nan")
    ddx, dP = _rel(out["dx"], ref["dx"]), _rel(out["P"], ref["P"])
    print(f"classes {what}: kernel {out['kernel']} mask {out['mask']:04b} counts {out['counts']} raw {out['raw']} f32 {out['f32']} batches +{out['batches']}: "
          f"chi2 {dchi:.2e} dx {ddx:.2e} P {dP:.2e}")
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


def _reports_the_partition(out, case, raw=None, f32=0):
    many = len(case.classes) > 1
    assert out["mask"] == case.mask, (out["mask"], case.mask)
    assert out["counts"] == case.counts, (out["counts"], case.counts)
    assert out["kernel"] == case.classes[0]                     # "last_feature_kernel" keeps its meaning: the longest track's
    assert out["batches"] == (1 if many else 0)
    assert out["raw"] == (case.raw if raw is None else raw) and out["f32"] == f32


def _same_bits(a, b, what, keys=OUT_KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


# --------------------------------------------------------------------------- 1. every case against the oracle
@pytest.mark.parametrize("cid", [c.id for c in cs.CASES])
def test_classes_against_the_oracle(Updater, oracle, cid):
    case = cs.BY_ID[cid]
    tri, ref = cs.oracle_run(oracle, case)
    out = _run(Updater, case, tri, 1)
    _hold_to_the_oracle(cid, out, ref)
    _reports_the_partition(out, case)


# --------------------------------------------------------------------------- 2. one class: the switch changes nothing
def test_one_class_is_level_zero_bit_for_bit(Updater, oracle):
    case = cs.BY_ID["one-class"]
    tri, _ = cs.oracle_run(oracle, case)
    a, b = _run(Updater, case, tri, 0), _run(Updater, case, tri, 1)
    _same_bits(a, b, "one-class")
    for k in ("kernel", "raw", "f32", "mask", "counts", "batches"):
        assert a[k] == b[k], k
    assert a["mask"] == 1 << 1 and a["counts"] == [0, case.prob.F, 0, 0] and a["batches"] == 0


# --------------------------------------------------------------------------- 3. level 0: the longest track decides
@pytest.mark.parametrize("cid", ["two", "four"])
def test_level_zero_launches_one_kernel(Updater, oracle, cid):
    case = cs.BY_ID[cid]
    tri, ref = cs.oracle_run(oracle, case)
    out = _run(Updater, case, tri, 0)
    _hold_to_the_oracle(cid + " level 0", out, ref)
    k = case.classes[0]
    counts = [0, 0, 0, 0]
    counts[k] = case.prob.F
    assert out["mask"] == 1 << k and out["kernel"] == k and out["counts"] == counts and out["batches"] == 0


# --------------------------------------------------------------------------- 4. a feature's statistic does not depend on its neighbours' class
def test_short_tracks_do_not_feel_the_long_one(Updater, oracle):
    case = cs.BY_ID["two"]
    tri, _ = cs.oracle_run(oracle, case)
    short = cs.two_without_long()
    tri_s = sh.shard_triangulation(case.prob, tri, list(range(1, case.prob.F)))
    with_long = _run(Updater, case, tri, 1)
    alone = _run(Updater, case, tri_s, 0, prob=short)
    assert with_long["mask"] == 0b110 and alone["mask"] == 0b010 and alone["kernel"] == 1
    gate = np.isfinite(alone["chi2"])
    d = np.abs(with_long["chi2"][1:][gate] / alone["chi2"][gate] - 1.0).max()
    print(f"classes independence: {int(gate.sum())} gated short tracks, chi2 level 1 with the long track against level 0 without it: {d:.2e}")
    assert gate.sum() >= 2
    assert np.array_equal(with_long["feat_status"][1:], alone["feat_status"])
    assert np.array_equal(with_long["chi2"][1:], alone["chi2"], equal_nan=True)
    assert np.array_equal(with_long["chi2_thresh"][1:], alone["chi2_thresh"], equal_nan=True)


# --------------------------------------------------------------------------- 5. one leg each
def test_leg_default_gate(Updater, oracle):
    case = cs.BY_ID["two"]
    tri, ref = cs.oracle_run(oracle, case)
    out = _run(Updater, case, tri, 1, opts=case.opts(gate_always_factor=0))
    _hold_to_the_oracle("two, bound first", out, ref, strict=False)
    _reports_the_partition(out, case)


def test_leg_float_stack(Updater, oracle):
    case = cs.BY_ID["two"]
    tri, ref = cs.oracle_run(oracle, case)
    out = _run(Updater, case, tri, 1, opts=case.opts(gram_fp32=1))
    _hold_to_the_oracle("two, gram_fp32", out, ref, fp32=True)
    _reports_the_partition(out, case, raw=0, f32=1)


def test_leg_anchored_representation(Updater, oracle):
    case = cs.BY_ID["two"]
    rep = dict(feat_rep_msckf=capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH)
    tri, ref = cs.oracle_run(oracle, case, None, **rep)
    _inputs_hold(ref)
    out = _run(Updater, case, tri, 1, opts=case.opts(**rep))
    _hold_to_the_oracle("two, anchored", out, ref)
    _reports_the_partition(out, case)


def test_leg_update_lm_corrects_the_landmarks_once(Updater, oracle):
    """The state of `two`'s window with eight SLAM landmarks behind the clones (synth.make_slam_problem on the window's seed: the same clones and
    calibration), the empty active set, `two`'s batch: the fused classes run as without landmarks, the landmarks take value + dx exactly."""
    from test_gpu_msckf_lm import BATCH, _mix, check_landmarks
    case = cs.BY_ID["two"]
    s = case.state
    slam = synth.make_slam_problem(5, L=8, lm_rep=_mix(8), seed=cs.SEED["two"], C=s["C"], K=s["K"])
    assert np.array_equal(slam.clone_q_p, case.prob.clone_q_p) and np.array_equal(slam.calib_q_p, case.prob.calib_q_p)
    msckf, plain = copy.copy(slam), copy.copy(case.prob)
    for k in BATCH:
        setattr(msckf, k, getattr(case.prob, k))
    plain.N, plain.P = slam.N, slam.P
    opts = case.opts()
    v = capi.Views(plain)
    tri = oracle.triangulate(opts, v)
    ref = oracle.msckf_update(opts, v, want_compressed=False, given=tri)
    _inputs_hold(ref)
    up = Updater(opts)
    up.debug_option("feat_classes", 1)
    up.set_slam_state(msckf)
    up.set_active_landmarks(())
    up.set_features(msckf)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    out = up.update_lm()
    out.update(_reads(up))
    _hold_to_the_oracle("two, update_lm", out, ref)
    _reports_the_partition(out, case)
    check_landmarks(up, msckf, out)
    up.close()


def test_leg_compress(Updater, oracle):
    case = cs.BY_ID["two"]
    tri, _ = cs.oracle_run(oracle, case)
    ref = oracle.msckf_update(case.opts(), capi.Views(case.prob), want_compressed=True, given=tri)
    Hc, rc = ref["H_comp"], ref["r_comp"]
    cmp = _run(Updater, case, tri, 1, entry="compress")
    H, r = cmp["H"], cmp["r"]
    eG, eg = _rel(H.T @ H, Hc.T @ Hc), _rel(H.T @ r, Hc.T @ rc)
    print(f"classes two, compress: rows {cmp['rows']} mask {cmp['mask']:04b} batches +{cmp['batches']}: H^T H {eG:.2e} H^T r {eg:.2e}")
    assert np.array_equal(cmp["feat_status"], ref["feat_status"])
    assert cmp["mask"] == case.mask and cmp["counts"] == case.counts and cmp["batches"] == 1
    assert eG < TOL_G and eg < TOL_g


def test_leg_layout_every_update(Updater, oracle):
    case = cs.BY_ID["three"]
    tri, ref = cs.oracle_run(oracle, case)
    out = _run(Updater, case, tri, 1, layout_every_update=1)
    _hold_to_the_oracle("three, layout_every_update", out, ref)
    _reports_the_partition(out, case)
    _same_bits(out, _run(Updater, case, tri, 1), "three: the lists rebuilt at the head of the update against the ones of the hand-over")


# --------------------------------------------------------------------------- 6. two ranks on one device
def test_loop_back_set_follows_the_switch(Updater, oracle):
    import torch
    from open_vins_amd.updater import MultiUpdater
    case = cs.BY_ID["ragged-600"]
    prob, G = case.prob, 2
    tri, ref = cs.oracle_run(oracle, case)
    one = _run(Updater, case, tri, 1)
    deal = sh.deal(case.lengths, G)

    class Rank(Updater):
        def __init__(self, m, g):
            self.lib, self._ctx = m.lib, C.c_void_p(m.lib.ovgpu_multi_ctx(m._m, g))
            assert self._ctx
            self.N, self.Cn, self.K, self.F = int(prob.N), int(prob.C), int(prob.K), len(deal[g])

        def close(self):
            self._ctx = C.c_void_p()

    m = MultiUpdater(case.opts(), devices=[0] * G)
    ranks = [Rank(m, g) for g in range(G)]
    for r in ranks:
        r.debug_option("feat_classes", 1)
    m.set_problem(prob)
    for g, r in enumerate(ranks):
        assert np.array_equal(r.get_features()["meas_offsets"], sh.shard_problem(prob, deal[g]).meas_offsets), "the deal"
        t = sh.shard_triangulation(prob, tri, deal[g])
        r.set_triangulation(t["p_FinG"], t["p_FinA"], t["anchor_meas"], t["status"])
    out = m.update()
    for g, r in enumerate(ranks):
        rd = _reads(r)
        part = cs.expected_partition(case.lengths[deal[g]])
        assert rd["mask"] == sum(1 << k for k, _, _, _ in part) == 0b110 and rd["batches"] == 1, (g, rd)
        assert [rd["counts"][k] for k, _, _, _ in part] == [b - a for _, a, b, _ in part], (g, rd)
    out.update(ranks[0].get_state(P=False))
    for r in ranks:
        r.close()
    m.close()
    gate = np.isfinite(one["chi2"])
    dev = dict(chi2=np.abs(out["chi2"][gate] / one["chi2"][gate] - 1.0).max(), thr=np.abs(out["chi2_thresh"][gate] / one["chi2_thresh"][gate] - 1.0).max(),
               dx=_rel(out["dx"], one["dx"]), P=_rel(out["P"], one["P"]), poses=max(np.abs(out[k] - one[k]).max() for k in ("clone_q_p", "calib_q_p", "intrinsics")))
    print("classes ragged-600, two ranks against one context at level 1: " + "  ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    assert np.array_equal(out["feat_status"], one["feat_status"]) and np.array_equal(out["feat_status"], ref["feat_status"])
    assert dev["chi2"] < sh.TOL_CHI2 and dev["thr"] < sh.TOL_THR and dev["dx"] < sh.TOL_DX
    assert dev["P"] < sh.TOL_P and np.array_equal(out["P"], out["P"].T) and dev["poses"] < sh.TOL_POSE


# --------------------------------------------------------------------------- 7. what rules the classes out
@pytest.mark.parametrize("how", ["shape2", "featy_big"])
def test_forced_shapes_ignore_the_switch(Updater, oracle, how):
    case = cs.BY_ID["two"]
    tri, _ = cs.oracle_run(oracle, case)
    opts = case.opts(feature_kernel_shape=2) if how == "shape2" else case.opts()
    debug = dict(featy_big=1) if how == "featy_big" else {}
    a, b = _run(Updater, case, tri, 0, opts=opts, **debug), _run(Updater, case, tri, 1, opts=opts, **debug)
    _same_bits(a, b, how)
    assert a["mask"] == b["mask"] == 1 << 2 and b["kernel"] == 2 and b["counts"] == [0, 0, case.prob.F, 0] and b["batches"] == 0
