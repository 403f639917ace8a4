"""The batches of tests/test_gpu_init_gate.py on the oracle alone (no GPU): every one of tests/init_gate_shapes.py must hold what it is named for
BEFORE it travels — every gated candidate further than GATE_MARGIN from its threshold (test_gpu_delayed_init_fused._oracle asserts it, never
skips), the planted outliers and nothing else CHI2_REJECTED, the track lengths and the entry dimension in its name — so that the GPU file compares
verdicts with no excuse.  Also include/ovgpu.h: the three levels of "delayed_init_fused" and the counter "delayed_init_rows_steps"."""
import os
import re

import numpy as np
import pytest

import init_gate_shapes as g
import test_gpu_delayed_init_fused as tf
from open_vins_amd import capi

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.parametrize("sid", [s.id for s in g.SHAPES])
def test_shape_holds_what_it_is_named_for(oracle, sid):
    shape = g.BY_ID[sid]
    case = shape.case
    prob = case.prob
    m = np.diff(prob.meas_offsets)
    assert prob.F <= 12 and (prob.C <= 12 or sid in ("len-64", "len-65"))
    tri, ref = tf._oracle(g.oracle_for(oracle, shape), case)  # asserts GATE_MARGIN on every gated candidate
    st = ref["feat_status"]
    gated = np.isfinite(ref["chi2"]) & (ref["chi2_thresh"] > 0)
    assert gated.sum() >= min(3, prob.F)
    assert np.flatnonzero(st == capi.FEAT_CHI2_REJECTED).tolist() == sorted(shape.planted)
    assert (st[list(shape.planted)] == capi.FEAT_CHI2_REJECTED).all()
    if shape.planted and len(shape.planted) < prob.F:
        assert (st == capi.FEAT_USED).any()
    for f, code in shape.tri_failed.items():
        assert st[f] == code and not np.isfinite(ref["chi2"][f]) and ref["lm_cov_id"][f] < 0
        assert (st[:f] == capi.FEAT_USED).any() and (st[f + 1:] == capi.FEAT_USED).any()  # between two accepted ones
    if shape.lengths is not None:
        assert m.tolist() == list(shape.lengths)
    if shape.n0_mod16 is not None:  # 3-dof candidates carry the dimension over the next multiple of 16 inside the chain
        assert prob.N % 16 == shape.n0_mod16 and case.rep == capi.REP_GLOBAL_3D and ref["N"] // 16 > prob.N // 16
    dof = np.where((case.each if case.each is not None else np.full(prob.F, case.rep)) == tf.SINGLE, 1, 3)
    assert ref["N"] == prob.N + int(dof[ref["lm_cov_id"] >= 0].sum())


def test_what_the_shapes_are_named_for(oracle):
    by = g.BY_ID
    assert g.TRACKS == [2, 3, 8, 9, 10] and tf.M_MAX == 64 and g.EDGES == [14, 15, 0]
    assert [2 * m - 3 for m in g.TRACKS] == [1, 3, 13, 15, 17]  # r: one row; r + 3 = 16; r on either side of 16
    assert 2 * tf.M_MAX - 3 + 3 == 128
    for m in (64, 65):
        c = by[f"len-{m}"].case
        assert c.prob.C == 33 and c.prob.K == 2 and c.prob.F == 3 and np.diff(c.prob.meas_offsets).max() == m
    # every representation the entry accepts under the four flag sets; fisheye on the mono ones
    assert sorted(g.REPS6) == list(range(6)) and len(g.FLAG_SETS) == 4
    for rep in g.REPS6:
        for i, (do_fej, K, pose, intr) in enumerate(g.FLAG_SETS):
            c = by[f"rep{rep}-flags{i}"].case
            assert c.rep == rep and c.prob.K == K and bool(c.prob.cam_is_fisheye.all()) == (K == 1)
            assert (c.opts.do_fej, c.opts.do_calib_camera_pose, c.opts.do_calib_camera_intrinsics) == (do_fej, pose, intr)
    # where the decision moved: first, middle, last, two in a row, all, and the determinism batch of twelve with two rejections
    F = g.GATE_F
    assert [by[k].planted for k in ("out-first", "out-middle", "out-last", "out-pair")] == [(0,), (5,), (F - 1,), (4, 5)]
    assert by["out-all"].planted == tuple(range(by["out-all"].case.prob.F))
    assert by["two-rejected"].case.prob.F == 12 and len(by["two-rejected"].planted) == 2
    # an accepted candidate behind the rejected first one: the oracle hands it the covariance id the first would have had
    _, ref = tf._oracle(oracle, by["out-first"].case)
    first_acc = int(np.flatnonzero(ref["lm_cov_id"] >= 0)[0])
    assert first_acc > 0 and ref["lm_cov_id"][first_acc] == by["out-first"].case.prob.N
    # the single depth gates against the quantile of 2m - 2 rows, the others of 2m (UpdaterSLAM.cpp:181-196, StateHelper.cpp:466)
    _, r3 = tf._oracle(oracle, by["rep0-flags0"].case)
    _, r1 = tf._oracle(oracle, by["rep5-flags0"].case)
    both = np.isfinite(r3["chi2"]) & np.isfinite(r1["chi2"])
    assert both.sum() >= 3 and (r1["chi2_thresh"][both] < r3["chi2_thresh"][both]).all()
    # per-feature sigma: the statistic does not depend on the context's sigma when every candidate brings its own
    for rep in ("global", "single"):
        _, a = tf._oracle(oracle, by[f"sigma-{rep}"].case)
        _, b = tf._oracle(oracle, by[f"sigma-{rep}-ctx3"].case)
        gate = np.isfinite(a["chi2"])
        assert by[f"sigma-{rep}-ctx3"].case.opts.sigma_pix == 3.0 and np.array_equal(gate, np.isfinite(b["chi2"]))
        np.testing.assert_allclose(b["chi2"][gate], a["chi2"][gate], rtol=1e-7)
    assert by["resident"].case.L0 == 6 and by["resident"].case.slam


def test_header_names_the_levels_and_the_counter():
    text = open(os.path.join(ROOT, "include", "ovgpu.h")).read()
    assert '"delayed_init_fused"' in text and '"delayed_init_rows_steps"' in text
    # the option's entry in ovgpu_debug_option's table: the three levels on lines of their own, the counter on its own line behind them
    entry = re.search(r'^ \*   "delayed_init_fused" .*\n((?: \* {10,}.*\n)+)', text, re.M)
    assert entry, 'no entry for "delayed_init_fused" in the table of debug options'
    for level in ("0:", "1:", "2:"):
        assert re.search(r"^ \*\s+" + level, entry.group(1), re.M), f"level {level} of delayed_init_fused is not on a line of its own"
    assert re.search(r'^ \*   "delayed_init_rows_steps" ', text, re.M)
