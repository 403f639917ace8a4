"""GPU tests (`-m gpu`) of the whitened Gram route of mode B at 384 .. 511 Jacobian columns, selected with ovgpu_debug_option "gram_wide" = 1 and
off by default: per-feature kernels write Y = H L over 7 and 8 column blocks of 64 (13 to 16 of 32), k_gram_blk forms Y^T Y over FOUR column
windows of 8 tiles (ten block pairs), two two-panel Cholesky-with-carry factorisations and k_tf_tail follow.

Comparators: the oracle, and a second context of the same library with the switch off (the Householder route).  Bounds, against either: chi2
1e-8 (relative), thresholds 1e-12, dx 1e-8, P' 1e-9 (relative Frobenius) and exactly symmetric, landmarks 1e-9, poses 1e-9 — the project's
tolerances of DESIGN.md section 3.  Accept sets are compared as they are: for every batch the ORACLE ALONE leaves no feature within
parity_util.GATE_MARGIN of its threshold (tests/test_gram_wide_shapes_cpu.py).  Every positive case asserts the Gram route, "last_gram_kernel" 2,
two more "chol_wide_factorisations", one more "gram_wide_updates", and "last_feature_kernel" against gram_wide_shapes' restatement of the rules;
a case the route does not take must return the switch-off context's BITS with "gram_wide_updates" unchanged.  The batches and what each is
named for: tests/gram_wide_shapes.py.  MSCKF cases run with the oracle's positions injected and gate_always_factor = 1, as
tests/test_gpu_track_edges.py runs its own.

Worst deviations over the positive cases, measured on the MI355X (every test prints its own; test_zz_worst_deviations the maxima): DESIGN.md
section 7 quotes them."""
import copy

import numpy as np
import pytest

import gram_wide_shapes as gw
import test_gpu_slam_chunked as sc
from open_vins_amd import capi
from parity_util import assert_chi2

pytestmark = pytest.mark.gpu

TOL_CHI2, TOL_THR, TOL_DX, TOL_P, TOL_LM, TOL_POSE = 1e-8, 1e-12, 1e-8, 1e-9, 1e-9, 1e-9
STATE_KEYS = ("clone_q_p", "calib_q_p", "intrinsics")
MSCKF_KEYS = ("feat_status", "chi2", "chi2_thresh", "p_FinG", "dx", "P") + STATE_KEYS
SLAM_KEYS = ("feat_status", "chi2", "chi2_thresh", "dx", "P", "landmarks") + STATE_KEYS
WORST = {}  # (comparator, quantity) -> largest deviation over the positive cases run so far


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def context(Updater, opts, wide, **debug):
    """a context with "gram_wide" (and the other switches) set before anything is uploaded; wide = None leaves the name alone"""
    up = Updater(opts)
    if wide is not None:
        up.debug_option("gram_wide", wide)
    for name, val in debug.items():
        up.debug_option(name, val)
    return up


def report(up, out):
    out["kernel"], out["gram"] = up.debug_option("last_feature_kernel"), up.debug_option("last_gram_kernel")
    out["wide"], out["chol"] = up.debug_option("gram_wide_updates"), up.debug_option("chol_wide_factorisations")
    out["route"] = up.lib.ovgpu_last_update_route(up._ctx)
    return out


def note(comparator, **dev):
    for k, v in dev.items():
        if np.isfinite(v):
            WORST[(comparator, k)] = max(WORST.get((comparator, k), 0.0), float(v))


def deviations(a, b, poses_of=None, landmarks=False):
    gate = np.isfinite(b["chi2"])
    assert np.array_equal(np.isfinite(a["chi2"]), gate)
    post = b if poses_of is None else poses_of
    dev = dict(chi2=np.abs(a["chi2"][gate] / b["chi2"][gate] - 1.0).max(), thr=np.abs(a["chi2_thresh"][gate] / b["chi2_thresh"][gate] - 1.0).max(),
               dx=_rel(a["dx"], b["dx"]), P=_rel(a["P"], b["P"]), poses=max(np.abs(a[k] - post[k]).max() for k in STATE_KEYS))
    if landmarks:
        dev["landmarks"] = np.abs(a["landmarks"] - b["landmarks"]).max()
    return dev


def hold(dev, out, what):
    """the bounds of the docstring; every figure is printed before it is asserted"""
    print(f"{what}: " + "  ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    assert dev["chi2"] < TOL_CHI2 and dev["thr"] < TOL_THR, what
    assert dev["dx"] < TOL_DX, what
    assert dev["P"] < TOL_P and np.array_equal(out["P"], out["P"].T), what
    assert dev["poses"] < TOL_POSE, what
    if "landmarks" in dev:
        assert dev["landmarks"] < TOL_LM, what


def assert_positive(on, off, case_id, kernel, updates=1, factorisations=2):
    """the route, the Gram kernel, the counters and the per-feature kernel of a case the wide route takes; the switch-off context took none of it"""
    assert on["route"] == capi.COMPRESS_GRAM, (case_id, on["route"])
    assert on["gram"] == 2, (case_id, on["gram"])
    assert on["wide"] == updates and on["chol"] == factorisations, (case_id, on["wide"], on["chol"])
    assert on["kernel"] == kernel, (case_id, on["kernel"], kernel)
    if off is not None:
        assert off["route"] == capi.COMPRESS_TSQR and off["wide"] == 0 and off["gram"] == 0 and off["kernel"] == 0, case_id


# --------------------------------------------------------------------------- MSCKF runs
def run_msckf(Updater, case, tri, wide, keep=False, **debug):
    up = context(Updater, case.opts(), wide, **{**case.debug, **debug})
    up.set_problem(case.prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    out = report(up, up.compress() if case.entry == "compress" else up.update())
    if keep:
        return out, up
    up.close()
    return out


_OFF_MSCKF, _OFF_SLAM = {}, {}  # (the two catalogues share an id)


def off_msckf(Updater, case, tri):
    """the switch-off context's outputs of a case: computed once, shared, left unchanged"""
    if case.id not in _OFF_MSCKF:
        _OFF_MSCKF[case.id] = run_msckf(Updater, case, tri, 0)
    return _OFF_MSCKF[case.id]


def check_msckf(Updater, oracle, case):
    tri, ref = gw.msckf_oracle_run(oracle, case)
    on, off = run_msckf(Updater, case, tri, 1), off_msckf(Updater, case, tri)
    for out, what in ((on, "switch on"), (off, "switch off")):
        assert np.array_equal(out["feat_status"], ref["feat_status"]), (case.id, what)  # every feature, no excuse
        for k in ("D", "n_rows", "n_used"):
            assert out["stats"][k] == ref["stats"][k], (case.id, what, k)
        assert_chi2(out, ref, TOL_CHI2, strict=True)
    if case.wide_at(1):
        assert_positive(on, off, case.id, case.kernel_at(1))
        d_or, d_off = deviations(on, ref), deviations(on, off)
        note("oracle", **d_or), note("switch-off context", **d_off)
        hold(d_or, on, f"{case.id} D {case.D} kernel {on['kernel']} against the oracle")
        hold(d_off, on, f"{case.id} D {case.D} kernel {on['kernel']} against the switch-off context")
        assert np.abs(on["intrinsics"] - ref["intrinsics"]).max() < 1e-8
    else:
        assert on["wide"] == 0 and on["kernel"] == case.kernel_at(1) == off["kernel"] and on["route"] == off["route"] and on["gram"] == off["gram"]
        sc.assert_equal_outputs(on, off, f"{case.id}: off the wide route, against the switch-off context", keys=MSCKF_KEYS)
        hold(deviations(on, ref), on, f"{case.id} D {case.D} against the oracle")
    return on, off, ref


# --------------------------------------------------------------------------- (a) ovgpu_msckf_update at both sides of every edge
@pytest.mark.parametrize("cid", [c.id for c in gw.MSCKF_CASES if c.group == "a"])
def test_msckf_update_columns(Updater, oracle, cid):
    case = gw.MSCKF_BY_ID[cid]
    on, off, ref = check_msckf(Updater, oracle, case)
    assert on["stats"]["D"] == case.D and on["kernel"] == 1
    assert on["route"] == capi.COMPRESS_GRAM and on["wide"] == (1 if case.D >= 384 else 0)
    assert on["feat_status"][case.rejected] == capi.FEAT_CHI2_REJECTED and (on["feat_status"] == capi.FEAT_USED).sum() >= 5


# --------------------------------------------------------------------------- (c) the MSCKF kernels by track length, at 384 and at 510 columns
@pytest.mark.parametrize("cid", [c.id for c in gw.MSCKF_CASES if c.group == "c"])
def test_msckf_kernels(Updater, oracle, cid):
    case = gw.MSCKF_BY_ID[cid]
    on, off, ref = check_msckf(Updater, oracle, case)
    want = 0 if cid.endswith("general") else gw.KERNEL_TRACKS[case.m_max]
    assert on["kernel"] == want and on["wide"] == 1 and on["stats"]["D"] == case.D
    m = np.diff(case.prob.meas_offsets)
    assert on["feat_status"][int(np.argmax(m))] == capi.FEAT_USED and on["feat_status"][case.rejected] == capi.FEAT_CHI2_REJECTED


# --------------------------------------------------------------------------- (b) ovgpu_slam_update over all columns
def run_slam(Updater, case, wide, level=None, keep=False):
    up = context(Updater, case.opts(), wide, slam_fused=case.level if level is None else level)
    p = case.prob
    up.set_slam_problem(p)
    if case.entry == "compress":
        out = up.slam_compress()
    else:
        out = up.slam_update(p.lm_index)
        out.update(up.get_state(P=False))
    report(up, out)
    out["batches"] = up.debug_option("slam_fused_batches")
    if keep:
        return out, up
    up.close()
    return out


def off_slam(Updater, case):
    if case.id not in _OFF_SLAM:
        _OFF_SLAM[case.id] = run_slam(Updater, case, 0)
    return _OFF_SLAM[case.id]


def check_slam(Updater, oracle, case):
    ref = gw.slam_oracle_run(oracle, case)
    assert ref["near_gate"] == 0
    on, off = run_slam(Updater, case, 1), off_slam(Updater, case)
    post = oracle.apply_dx(case.opts(), capi.Views(case.prob), ref["dx"])
    gate = np.isfinite(ref["chi2"])
    for out, what in ((on, "switch on"), (off, "switch off")):
        assert np.array_equal(out["feat_status"], ref["feat_status"]), (case.id, what)
        for k in ("D", "n_rows", "n_used"):
            assert out["stats"][k] == ref["stats"][k], (case.id, what, k)
        assert np.isnan(out["chi2"][~gate]).all()
    assert_positive(on, off, case.id, case.kernel_wide(1))
    assert on["batches"] == (1 if on["kernel"] >= 4 else 0) and off["batches"] == 0
    d_or, d_off = deviations(on, ref, post, landmarks=True), deviations(on, off, landmarks=True)
    note("oracle", **d_or), note("switch-off context", **d_off)
    hold(d_or, on, f"{case.id} D {case.D} kernel {on['kernel']} against the oracle")
    hold(d_off, on, f"{case.id} D {case.D} kernel {on['kernel']} against the switch-off context")
    return on, off, ref


@pytest.mark.parametrize("cid", [c.id for c in gw.SLAM_CASES if c.group == "b"])
def test_slam_update_columns_general_kernel(Updater, oracle, cid):
    case = gw.SLAM_BY_ID[cid]
    on, _, _ = check_slam(Updater, oracle, case)
    assert on["kernel"] == 0 and on["stats"]["D"] == case.D
    assert on["feat_status"][case.rejected] == capi.FEAT_CHI2_REJECTED and (on["feat_status"] == capi.FEAT_USED).sum() >= 5


@pytest.mark.parametrize("cid", [c.id for c in gw.SLAM_CASES if c.group == "bf"])
def test_slam_update_columns_fused_kernels(Updater, oracle, cid):
    case = gw.SLAM_BY_ID[cid]
    on, _, _ = check_slam(Updater, oracle, case)
    want = (6 if "long" in cid else 4) + (1 if cid.endswith("single") else 0)
    assert on["kernel"] == want and on["stats"]["D"] == case.D
    assert on["feat_status"][case.rejected] == capi.FEAT_CHI2_REJECTED and on["feat_status"][0] == capi.FEAT_USED


# --------------------------------------------------------------------------- ovgpu_msckf_update_lm: landmarks resident, none with a column
def test_msckf_update_lm_takes_the_route(Updater, oracle):
    """400 columns (62 clones, stereo) under six resident landmarks and the empty active set: the MSCKF batch of case a-400"""
    import test_gpu_msckf_lm as ml
    case = gw.MSCKF_BY_ID["a-400"]
    plain = case.prob
    slam = gw.ss.slam(6, (gw.ss.REPS5 + [gw.SINGLE]), gw.msckf_seed(400), C=plain.C, K=plain.K)  # a-400's window: the state stream follows the seed
    assert np.array_equal(slam.clone_q_p, plain.clone_q_p) and np.array_equal(slam.intrinsics, plain.intrinsics)
    msckf = copy.copy(slam)
    for k in ml.BATCH:
        setattr(msckf, k, getattr(plain, k))
    twin = copy.copy(plain)
    twin.N, twin.P = slam.N, slam.P
    opts = case.opts()
    v = capi.Views(twin)
    tri = oracle.triangulate(opts, v)
    ref = oracle.msckf_update(opts, v, want_compressed=False, given=tri)
    gate = np.isfinite(ref["chi2"])
    assert np.abs(ref["chi2"][gate] / ref["chi2_thresh"][gate] - 1.0).min() > gw.ss.GATE_MARGIN and (ref["feat_status"] == capi.FEAT_CHI2_REJECTED).sum() == 1
    res = {}
    for wide in (1, 0):
        up = context(Updater, opts, wide)
        ml.hand_over(up, msckf)
        up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
        out = report(up, up.update_lm())
        ml.check_landmarks(up, msckf, out)
        up.close()
        assert np.array_equal(out["feat_status"], ref["feat_status"])
        res[wide] = out
    on, off = res[1], res[0]
    assert_positive(on, off, "update_lm a-400", 1)
    hold(deviations(on, ref), on, "ovgpu_msckf_update_lm at 400 columns against the oracle")
    d = deviations(on, off, landmarks=True)
    note("switch-off context", **d)
    hold(d, on, "ovgpu_msckf_update_lm at 400 columns against the switch-off context")


# --------------------------------------------------------------------------- (d) what must not move
@pytest.mark.parametrize("cid", ["d-tsqr-400", "d-fp32-400"])
def test_off_the_route_nothing_moves_msckf(Updater, oracle, cid):
    case = gw.MSCKF_BY_ID[cid]
    tri, ref = gw.msckf_oracle_run(oracle, case)
    on, off = run_msckf(Updater, case, tri, 1), off_msckf(Updater, case, tri)
    assert on["wide"] == 0 and on["route"] == capi.COMPRESS_TSQR == off["route"] and on["kernel"] == 0 and on["gram"] == 0
    sc.assert_equal_outputs(on, off, f"{cid}: switch on against switch off", keys=MSCKF_KEYS)
    assert np.array_equal(on["feat_status"], ref["feat_status"])


def test_off_the_route_nothing_moves_383_columns(Updater, oracle):
    case = gw.SLAM_BY_ID["d-383"]
    on, off = run_slam(Updater, case, 1), off_slam(Updater, case)
    assert on["stats"]["D"] == 383 and on["route"] == capi.COMPRESS_GRAM == off["route"] and on["gram"] == off["gram"] == 2
    assert on["wide"] == 0 and on["kernel"] == off["kernel"] == 0
    sc.assert_equal_outputs(on, off, "383 columns: switch on against switch off", keys=SLAM_KEYS)
    assert np.array_equal(on["feat_status"], gw.slam_oracle_run(oracle, case)["feat_status"])


def test_mode_a_keeps_the_householder_triangle_at_384(Updater, oracle):
    case = gw.MSCKF_BY_ID["d-compress-384"]
    tri, _ = gw.msckf_oracle_run(oracle, case)
    on, off = run_msckf(Updater, case, tri, 1), run_msckf(Updater, case, tri, 0)
    assert on["wide"] == 0 and on["D"] == off["D"] == 384 and on["rows"] == off["rows"] > 0 and on["gram"] == 0
    for k in ("feat_status", "chi2", "chi2_thresh", "H", "r", "col_cov_id"):
        assert np.array_equal(on[k], off[k], equal_nan=True), k
    case = gw.SLAM_BY_ID["d-compress-384"]
    on, off = run_slam(Updater, case, 1), run_slam(Updater, case, 0)
    assert on["wide"] == 0 and on["D"] == off["D"] == 384 and on["rows"] == off["rows"] and on["gram"] == 0
    for k in ("feat_status", "chi2", "chi2_thresh", "H", "r", "col_cov_id"):
        assert np.array_equal(on[k], off[k], equal_nan=True), k


def test_semi_definite_prior_repeats_through_householder(Updater, oracle):
    """the two newest clones perfectly correlated at 400 columns: the prior block's pivot fails (in the second panel), the call repeats through the
    Householder route, the attempt is not counted and the context stays usable"""
    case = gw.MSCKF_BY_ID["d-semi-definite-400"]
    tri, ref = gw.msckf_oracle_run(oracle, case)
    on, up = run_msckf(Updater, case, tri, 1, keep=True)
    off = off_msckf(Updater, case, tri)
    assert on["stats"]["status"] == 0 and on["route"] == capi.COMPRESS_TSQR and on["wide"] == 0 and on["kernel"] == 0
    assert np.array_equal(on["feat_status"], ref["feat_status"]) and np.array_equal(off["feat_status"], ref["feat_status"])
    hold(deviations(on, ref), on, "semi-definite prior at 400 columns, the Householder repeat, against the oracle")
    hold(deviations(on, off), on, "semi-definite prior at 400 columns, the Householder repeat, against the switch-off context")
    # the context is usable: the positive-definite twin of the batch takes the wide route on it
    good = gw.MSCKF_BY_ID["a-400"]
    tri2, ref2 = gw.msckf_oracle_run(oracle, good)
    up.set_problem(good.prob)
    up.set_triangulation(tri2["p_FinG"], tri2["p_FinA"], tri2["anchor_meas"], tri2["status"])
    again = report(up, up.update())
    up.close()
    assert again["route"] == capi.COMPRESS_GRAM and again["wide"] == 1 and np.array_equal(again["feat_status"], ref2["feat_status"])
    hold(deviations(again, ref2), again, "a-400 behind the Householder repeat, against the oracle")


@pytest.mark.parametrize("how", ["no_single_launch_cholesky", "chol_wide_0"])
def test_stepwise_cholesky_stays_on_the_gram_route(Updater, oracle, how):
    case = gw.MSCKF_BY_ID["d-stepwise-400"] if how == "no_single_launch_cholesky" else gw.MSCKF_BY_ID["a-400"]
    tri, ref = gw.msckf_oracle_run(oracle, case)
    on = run_msckf(Updater, case, tri, 1, **({} if how == "no_single_launch_cholesky" else dict(chol_wide=0)))
    assert_positive(on, None, f"{case.id} {how}", 1, factorisations=0)
    assert np.array_equal(on["feat_status"], ref["feat_status"])
    hold(deviations(on, ref), on, f"400 columns, {how}, against the oracle")
    two_panel = run_msckf(Updater, gw.MSCKF_BY_ID["a-400"], tri, 1)
    hold(deviations(on, two_panel), on, f"400 columns, {how}, against the two-panel factorisations")


def test_512_columns_are_refused_as_before(Updater):
    p = gw.over_the_bound()
    msgs = []
    for wide in (1, 0):
        up = context(Updater, capi.default_options(chi2_multipler=1.0), wide)
        up.set_slam_problem(p)
        with pytest.raises(capi.OvgpuError) as e:
            up.slam_update(p.lm_index)
        assert e.value.code == capi.ERR_CAPACITY and "512 Jacobian columns, more than 511" in str(e.value)
        assert up.debug_option("gram_wide_updates") == 0
        msgs.append(str(e.value))
        st = up.get_state()
        assert np.array_equal(st["P"], p.P)
        up.close()
    assert msgs[0] == msgs[1]


def test_the_switch(Updater, oracle):
    case = gw.MSCKF_BY_ID["a-384"]
    tri, ref = gw.msckf_oracle_run(oracle, case)
    up = Updater(case.opts())
    assert up.debug_option("gram_wide") == 0                                            # the default stays 0
    assert up.debug_option("gram_wide", 1) == 0 and up.debug_option("gram_wide") == 1   # reads back 1
    assert up.debug_option("gram_wide", 7) == 1 and up.debug_option("gram_wide") == 1   # values above 1 are taken as 1
    assert up.debug_option("gram_wide_updates", 5) == 0 and up.debug_option("gram_wide_updates") == 0  # read only
    up.close()
    never, off = run_msckf(Updater, case, tri, None), off_msckf(Updater, case, tri)
    assert never["wide"] == 0 and never["route"] == capi.COMPRESS_TSQR
    sc.assert_equal_outputs(never, off, "never set against gram_wide = 0", keys=MSCKF_KEYS)
    # thrown after the batch was handed over: the resident batch keeps its route, the next ovgpu_set_features takes the switch
    up = context(Updater, case.opts(), 0)
    up.set_problem(case.prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    up.debug_option("gram_wide", 1)
    first = report(up, up.update())
    assert first["route"] == capi.COMPRESS_TSQR and first["wide"] == 0
    sc.assert_equal_outputs(first, off, "the switch thrown behind ovgpu_set_features", keys=MSCKF_KEYS)
    up.reset_state()
    up.set_features(case.prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    second = report(up, up.update())
    up.close()
    assert second["route"] == capi.COMPRESS_GRAM and second["wide"] == 1 and second["gram"] == 2
    hold(deviations(second, ref), second, "a-384 after the switch was thrown and the batch handed over again, against the oracle")
    # ... a SLAM batch too, which the update lays out again for its own rows: the level in force is the one the batch was handed over under
    scase = gw.SLAM_BY_ID["b-400"]
    p = scase.prob
    up = context(Updater, scase.opts(), 0, slam_fused=0)
    up.set_slam_problem(p)
    up.debug_option("gram_wide", 1)
    first = up.slam_update(p.lm_index)
    first.update(up.get_state(P=False))
    report(up, first)
    assert first["route"] == capi.COMPRESS_TSQR and first["wide"] == 0
    sc.assert_equal_outputs(first, off_slam(Updater, scase), "SLAM: the switch thrown behind ovgpu_set_features", keys=SLAM_KEYS)
    up.close()


# --------------------------------------------------------------------------- (e) ovgpu_slam_update_chunked
def test_chunks_equal_the_chain(Updater, oracle):
    """three chunks of four landmarks over 64 clones (412 columns and the chunk's own 10 .. 12): one device pass against the chain of single calls,
    both with the switch on, for equality in every output; against the oracle's chain within the bounds"""
    opts = capi.default_options(chi2_multipler=1.0)
    q = gw.chunk_problem()
    q.lm_index = np.arange(q.F, dtype=np.int32)

    def wide_on(o):
        return context(Updater, o, 1)

    out, up = sc.chunked(wide_on, opts, q, gw.CHUNK_FIRST, keep=True)
    ref, up2 = sc.chain(wide_on, opts, q, gw.CHUNK_FIRST, keep=True)
    for u in (up, up2):
        assert u.debug_option("gram_wide_updates") == 3 and u.debug_option("last_gram_kernel") == 2 and u.debug_option("chol_wide_factorisations") == 6
        assert u.debug_option("slam_chunked_fallbacks") == 0
        u.close()
    assert [s["D"] for s in out["stats"]] == gw.chunk_columns()[1]
    sc.assert_equal_outputs(out, ref, "three chunks against the chain, both with the switch on")
    orc = sc.oracle_chain(oracle, opts, q, gw.CHUNK_FIRST)
    assert orc["near_gate"] == 0 and np.array_equal(out["feat_status"], orc["feat_status"])
    dev = dict(dx=max(_rel(out["dx_seq"][k], orc["dx_seq"][k]) for k in range(3)), P=_rel(out["P"], orc["P"]),
               landmarks=np.abs(out["landmarks"] - orc["landmarks"]).max(), poses=max(np.abs(out[k] - orc[k]).max() for k in STATE_KEYS))
    print("three chunks with the switch on against the oracle's chain: " + "  ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    assert dev["dx"] < TOL_DX and dev["P"] < TOL_P and np.array_equal(out["P"], out["P"].T) and dev["landmarks"] < TOL_LM and dev["poses"] < TOL_POSE


# --------------------------------------------------------------------------- (f) context hygiene
def test_one_context_510_then_208_then_448(Updater, oracle):
    """every link returns a fresh context's bits: nothing of the wider (or narrower) update before it is left in a workspace"""
    cases = [gw.MSCKF_BY_ID[c] for c in gw.HYGIENE_CHAIN]
    up = context(Updater, cases[0].opts(), 1)
    wide = 0
    for case in cases:
        tri, ref = gw.msckf_oracle_run(oracle, case)
        up.set_problem(case.prob)
        up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
        link = report(up, up.update())
        fresh = run_msckf(Updater, case, tri, 1)
        wide += 1 if case.D >= 384 else 0
        assert link["wide"] == wide and link["kernel"] == fresh["kernel"] == 1 and link["route"] == capi.COMPRESS_GRAM and link["gram"] == fresh["gram"]
        sc.assert_equal_outputs(link, fresh, f"{case.id} as a link of the chain against a fresh context", keys=MSCKF_KEYS)
        assert np.array_equal(link["feat_status"], ref["feat_status"])
    up.close()


@pytest.mark.parametrize("cid", ["a-510", "c-510-127"])
def test_same_bits_twice_from_reset_state(Updater, oracle, cid):
    case = gw.MSCKF_BY_ID[cid]
    tri, _ = gw.msckf_oracle_run(oracle, case)
    first, up = run_msckf(Updater, case, tri, 1, keep=True)
    up.reset_state()
    up.set_features(case.prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    second = report(up, up.update())
    up.close()
    assert second["wide"] == 2 and second["kernel"] == first["kernel"]
    sc.assert_equal_outputs(first, second, f"{cid}: the same call twice from ovgpu_reset_state", keys=MSCKF_KEYS)


def test_zz_worst_deviations():
    """prints what the positive cases of this file measured (DESIGN.md section 7 quotes the figures)"""
    for (comparator, k), v in sorted(WORST.items()):
        print(f"gram_wide, against the {comparator}: worst {k} {v:.3e}")
