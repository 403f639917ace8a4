"""The batches of tests/test_gpu_delayed_init_long.py: ovgpu_debug_option "delayed_init_fused_long" (csrc/k_init_fused.h: the fused step of
ovgpu_slam_delayed_init_fused for candidates of 65 .. 232 measurements; r = 2m - 3 > 256, m >= 130, factored by the two panels of k_chol_wide.h).
tests/test_init_long_shapes_cpu.py holds every one of them on the oracle alone to what it is named for: the track lengths in chain order, the
planted rejections and nothing else rejected, no gated candidate within GATE_MARGIN of its threshold.

Shapes: the smallest windows that reach each length — 33 stereo clones for 64 / 65, 33 clones x 4 cameras for 128 .. 130 (r = 253, 255: the last
single panel; 257: the first two-panel one), 59 clones x 4 cameras for 231 .. 233 (the upper bound; 233 takes the chain's step in place).  Five
candidates at most.  A helper module in the manner of tests/init_gate_shapes.py, not a conftest: nothing here is collected.
"""
import functools

import numpy as np

import init_gate_shapes as g
import track_shapes as ts
from open_vins_amd import capi, synth
from test_gpu_delayed_init_fused import Case, SINGLE, M_MAX

M_LONG = 232   # include/ovgpu.h: the fused step's bound under "delayed_init_fused_long"
M_PANEL = 129  # r = 2m - 3 <= 256: one panel of the factorisation up to here, two beyond
REPS6 = g.REPS6

STEREO = dict(C=33, K=2)   # tracks of up to 66 measurements
QUAD = dict(C=33, K=4)     # up to 132
QUAD59 = dict(C=59, K=4)   # up to 236
LEN_STEREO = [10, 64, 65, 12, 9]      # 64 unchanged, 65 the first long one, the chain goes on
LEN_PANEL = [10, 128, 129, 130, 12]   # r = 253, 255, 257
LEN_BOUND = [9, 231, 232, 233, 12]    # r = 459, 461 (the bound), 463 (the chain's step)
SEED = 50


Shape = g.Shape  # id; make() -> Case (built once); planted: the rejected candidates; lengths: the track lengths in chain order; tri_failed


@functools.lru_cache(maxsize=None)
def _window(C, K, seed, calib_noise=1.0):
    """The five full tracks of the C x K window of seed `seed` (the longest of eight: all five are seen by every camera from every clone)."""
    prob = ts.longest(synth.make_problem(2, C=C, K=K, F=8, seed=seed, calib_noise=calib_noise), 5)
    assert (np.diff(prob.meas_offsets) == C * K).all()
    return prob


def _batch(state, lengths, seed=SEED, calib_noise=1.0):
    """Candidate f trimmed to lengths[f] observations at the widest stride; every track holds that many (nothing is topped up by repetition)."""
    prob = _window(state["C"], state["K"], seed, calib_noise).subset(np.arange(len(lengths)))
    assert max(lengths) <= state["C"] * state["K"]
    prob = ts.with_lengths(prob, lengths, patterns=("stride",))
    assert np.diff(prob.meas_offsets).tolist() == list(lengths)
    return prob


def _opts(pose=1, intr=1, **kw):
    return capi.default_options(chi2_multipler=1.0, do_calib_camera_pose=pose, do_calib_camera_intrinsics=intr, **kw)


def _plain(state, lengths, rep, planted=(), seed=SEED):
    return Case(g._plant(_batch(state, lengths, seed), planted), rep)


# --------------------------------------------------------------------------- resident landmarks under the empty active set
RESIDENT_REPS = np.array([0, 4, 5], np.int32)


def _resident():
    tracks = _batch(QUAD, LEN_PANEL)
    state = synth.make_slam_problem(2, L=len(RESIDENT_REPS), lm_rep=RESIDENT_REPS, C=QUAD["C"], K=QUAD["K"], seed=SEED)
    return Case(g._tracks_from(state, tracks), capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, slam=True)


# --------------------------------------------------------------------------- per-feature sigma and multiplier
def sigma_arrays(F=5):
    tag = np.array([False, True, False, True, True])[:F]
    return tag, np.where(tag, 2.5, 1.0), np.where(tag, 3.0, 1.0)


def _sigma():
    _, sig, mult = sigma_arrays()
    return Case(_batch(QUAD, LEN_PANEL), capi.REP_GLOBAL_3D, opts=_opts(), sig=sig, mult=mult)


# --------------------------------------------------------------------------- a calibration that is not estimated: a ready-made long rejection
def _uncalibrated():
    """59 clones x 4 cameras whose calibration the state does not estimate, the estimate off the truth by synth's usual noise: an error the filter
    does not model, which the 232-measurement single-depth candidate fails its gate on while its short neighbours pass."""
    return Case(_batch(QUAD59, [9, 232, 12]), SINGLE, opts=_opts(pose=0, intr=0))


def _shapes():
    out = [Shape("stereo-64-65", functools.partial(_plain, STEREO, LEN_STEREO, capi.REP_GLOBAL_3D), lengths=LEN_STEREO)]
    for rep in REPS6:  # the 4-camera states in each of the six representations in turn
        out.append(Shape(f"panel-rep{rep}", functools.partial(_plain, QUAD, LEN_PANEL, rep), lengths=LEN_PANEL))
        out.append(Shape(f"bound-rep{rep}", functools.partial(_plain, QUAD59, LEN_BOUND, rep), lengths=LEN_BOUND))
    # the carve and the step words before and after short steps
    out.append(Shape("long-first", functools.partial(_plain, QUAD, [130, 10, 12], capi.REP_ANCHORED_3D), lengths=[130, 10, 12]))
    out.append(Shape("long-last", functools.partial(_plain, QUAD, [10, 12, 130], capi.REP_GLOBAL_FULL_INVERSE_DEPTH), lengths=[10, 12, 130]))
    out.append(Shape("long-alone", functools.partial(_plain, QUAD, [130], capi.REP_GLOBAL_3D), lengths=[130]))
    out.append(Shape("resident", _resident, lengths=LEN_PANEL))
    out.append(Shape("sigma", _sigma, lengths=LEN_PANEL))
    # a long rejected candidate between accepted ones: planted on one panel, planted on two, and the uncalibrated state's own
    out.append(Shape("out-129", functools.partial(_plain, QUAD, LEN_PANEL, capi.REP_GLOBAL_3D, (2,)), planted=(2,), lengths=LEN_PANEL))
    out.append(Shape("out-130", functools.partial(_plain, QUAD, LEN_PANEL, capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, (3,)), planted=(3,), lengths=LEN_PANEL))
    out.append(Shape("out-232", functools.partial(_plain, QUAD59, LEN_BOUND, capi.REP_GLOBAL_3D, (2,)), planted=(2,), lengths=LEN_BOUND))
    out.append(Shape("uncalibrated-232", _uncalibrated, planted=(1,), lengths=[9, 232, 12]))
    # a long candidate whose triangulation failed
    out.append(Shape("tri-failed-130", functools.partial(_plain, QUAD, LEN_PANEL, capi.REP_GLOBAL_3D), lengths=LEN_PANEL, tri_failed={3: capi.FEAT_TRI_FAILED}))
    return out


SHAPES = _shapes()
BY_ID = {s.id: s for s in SHAPES}
assert len(BY_ID) == len(SHAPES)


def n_long(shape):
    """Candidates the long bound adds to the fused step: 65 .. 232 measurements."""
    m = np.diff(shape.case.prob.meas_offsets)
    return int(((m > M_MAX) & (m <= M_LONG)).sum())
