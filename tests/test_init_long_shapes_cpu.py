"""The batches of tests/test_gpu_delayed_init_long.py on the oracle alone (no GPU): every one of tests/init_long_shapes.py must hold what it is
named for BEFORE it travels — every gated candidate further than GATE_MARGIN (1e-6) from its threshold (test_gpu_delayed_init_fused._oracle
asserts it, never skips), the planted rejections and nothing else CHI2_REJECTED, the track lengths of its name in chain order — so that the GPU
file compares verdicts with no excuse.  Also include/ovgpu.h: the switch "delayed_init_fused_long", its counter and its bounds."""
import os
import re

import numpy as np
import pytest

import init_gate_shapes as g
import init_long_shapes as ls
import test_gpu_delayed_init_fused as tf
from open_vins_amd import capi

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.parametrize("sid", [s.id for s in ls.SHAPES])
def test_shape_holds_what_it_is_named_for(oracle, sid):
    shape = ls.BY_ID[sid]
    case = shape.case
    prob = case.prob
    m = np.diff(prob.meas_offsets)
    assert prob.F <= 5 and m.tolist() == list(shape.lengths)
    assert tf.GATE_MARGIN == 1e-6
    tri, ref = tf._oracle(g.oracle_for(oracle, shape), case)  # asserts GATE_MARGIN on every gated candidate
    st = ref["feat_status"]
    gated = np.isfinite(ref["chi2"]) & (ref["chi2_thresh"] > 0)
    assert gated.sum() == prob.F - len(shape.tri_failed)
    assert np.flatnonzero(st == capi.FEAT_CHI2_REJECTED).tolist() == sorted(shape.planted)
    rest = np.ones(prob.F, bool)
    rest[list(shape.planted) + list(shape.tri_failed)] = False
    assert (st[rest] == capi.FEAT_USED).all() and (ref["lm_cov_id"][rest] >= 0).all()
    for f in shape.planted:  # a LONG rejected candidate between accepted ones
        assert ls.M_MAX < m[f] <= ls.M_LONG and (st[:f] == capi.FEAT_USED).any() and (st[f + 1:] == capi.FEAT_USED).any()
    for f, code in shape.tri_failed.items():
        assert ls.M_MAX < m[f] <= ls.M_LONG
        assert st[f] == code and not np.isfinite(ref["chi2"][f]) and ref["lm_cov_id"][f] < 0
        assert (st[:f] == capi.FEAT_USED).any() and (st[f + 1:] == capi.FEAT_USED).any()
    dof = 1 if case.rep == tf.SINGLE else 3
    assert ref["N"] == prob.N + dof * int((ref["lm_cov_id"] >= 0).sum())
    assert ls.n_long(shape) >= 1


def test_what_the_shapes_are_named_for(oracle):
    by = ls.BY_ID
    assert tf.M_MAX == 64 and ls.M_LONG == 232 and ls.M_PANEL == 129
    assert [2 * m - 3 for m in ls.LEN_PANEL[1:4]] == [253, 255, 257] and 2 * ls.M_PANEL - 3 <= 256 < 2 * (ls.M_PANEL + 1) - 3
    assert [2 * m - 3 for m in ls.LEN_BOUND[1:4]] == [459, 461, 463] and ls.LEN_BOUND[2] == ls.M_LONG
    assert ls.LEN_STEREO[1:3] == [tf.M_MAX, tf.M_MAX + 1]
    # the smallest windows that reach each length
    for sid, (C, K) in (("stereo-64-65", (33, 2)), ("panel-rep0", (33, 4)), ("bound-rep0", (59, 4))):
        p = by[sid].case.prob
        assert (p.C, p.K) == (C, K) and (C - 1) * K < np.diff(p.meas_offsets).max() <= C * K
    # the 4-camera states in each of the six representations; the single depth gates against the quantile of 2m - 2 rows
    assert sorted(ls.REPS6) == list(range(6))
    for rep in ls.REPS6:
        assert by[f"panel-rep{rep}"].case.rep == rep and by[f"bound-rep{rep}"].case.rep == rep
    _, r3 = tf._oracle(oracle, by["panel-rep0"].case)
    _, r1 = tf._oracle(oracle, by[f"panel-rep{tf.SINGLE}"].case)
    assert (r1["chi2_thresh"] < r3["chi2_thresh"]).all()
    # a long candidate first, last and alone
    assert by["long-first"].lengths[0] == 130 and by["long-last"].lengths[-1] == 130 and by["long-alone"].lengths == [130]
    assert max(by["long-first"].lengths[1:]) <= tf.M_MAX and max(by["long-last"].lengths[:-1]) <= tf.M_MAX
    # resident landmarks (one anchored, one single depth among them) under the empty active set; per-feature sigma on long candidates
    c = by["resident"].case
    assert c.slam and c.L0 == 3 and c.prob.N == by["panel-rep0"].case.prob.N + 7
    tag, sig, mult = ls.sigma_arrays()
    c = by["sigma"].case
    assert np.array_equal(c.sig, sig) and np.array_equal(c.mult, mult) and (np.diff(c.prob.meas_offsets)[tag] > tf.M_MAX).any() and (sig != 1).any()
    # the long rejections: one panel, two panels, the bound — and the one nobody planted, on a state whose calibration is not estimated
    assert [by[k].lengths[by[k].planted[0]] for k in ("out-129", "out-130", "out-232", "uncalibrated-232")] == [129, 130, 232, 232]
    c = by["uncalibrated-232"].case
    assert (c.opts.do_calib_camera_pose, c.opts.do_calib_camera_intrinsics) == (0, 0) and c.rep == tf.SINGLE
    _, ref = tf._oracle(oracle, c)
    print("uncalibrated-232: chi2 / threshold", (ref["chi2"] / ref["chi2_thresh"]).round(3).tolist())
    assert 1.05 < ref["chi2"][1] / ref["chi2_thresh"][1] < 2.0  # its own error, not a gross outlier's
    (f, code), = by["tri-failed-130"].tri_failed.items()
    assert by["tri-failed-130"].lengths[f] == 130 and code == capi.FEAT_TRI_FAILED


def test_header_names_the_switch_its_counter_and_its_bounds():
    text = open(os.path.join(ROOT, "include", "ovgpu.h")).read()
    entry = re.search(r'^ \*   "delayed_init_fused_long" .*\n((?: \* {10,}.*\n)*)', text, re.M)
    assert entry, 'no entry for "delayed_init_fused_long" in the table of debug options'
    body = entry.group(0)
    assert "232" in body and "65" in body and "default 0" in body
    assert re.search(r'^ \*   "delayed_init_long_steps" ', text, re.M)
    assert re.search(r"#define OVGPU_ABI_VERSION\s+10\b", text)
