"""The batches of tests/test_gpu_init_gate.py: level 2 of ovgpu_debug_option "delayed_init_fused" (csrc/k_init_fused.h: k_init_rows in front of the
fused step, the gate decided in k_initf_tail_gate from the step's own factorisation).  tests/test_init_gate_shapes_cpu.py holds every one of them
on the oracle alone to what it is named for: the planted outliers, and nothing else, rejected; no gated candidate within GATE_MARGIN of its
threshold; the track lengths and the covariance dimension in its name.

Shapes: the smallest at which the named part can go wrong — C <= 12 clones and F <= 12 candidates, except the 64 / 65-measurement tracks, which
need 33 stereo clones (F = 3 there).  Seeds were chosen on the oracle so that no candidate that was not planted is rejected or near its gate.
synth's fisheye switch covers every camera of a problem: the fisheye cases are the mono (K = 1) ones, "fisheye on one camera".
"""
import copy
import functools

import numpy as np

import track_shapes as ts
from open_vins_amd import capi, synth
from test_gpu_delayed_init_fused import Case, TRACK_KEYS, SINGLE, M_MAX

REPS6 = [capi.REP_GLOBAL_3D, capi.REP_GLOBAL_FULL_INVERSE_DEPTH, capi.REP_ANCHORED_3D, capi.REP_ANCHORED_FULL_INVERSE_DEPTH,
         capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, SINGLE]
# (do_fej, K, calibrate pose, calibrate intrinsics): tests/test_gpu_delayed_init_fused.py::test_calibration_and_fej_flags
FLAG_SETS = [(0, 2, 1, 1), (1, 1, 0, 0), (0, 1, 1, 0), (1, 2, 0, 1)]
TRACKS = [2, 3, 8, 9, 10]  # r = 2m - 3 = 1 (a one-row factorisation), 3, 13 (r + 3 = 16), 15 and 17 (r crosses 16)
EDGES = [14, 15, 0]        # the covariance dimension at entry, modulo 16


class Shape:
    """id; make() -> Case (built once); planted: the candidates made gross outliers; lengths: the exact track lengths, or None; n0_mod16: the entry
    dimension modulo 16, or None; tri_failed: {candidate: status} injected through set_triangulation."""

    def __init__(self, id, make, planted=(), lengths=None, n0_mod16=None, tri_failed=None):
        self.id, self._make, self.planted, self.lengths, self.n0_mod16 = id, make, tuple(planted), lengths, n0_mod16
        self.tri_failed = dict(tri_failed or {})

    @functools.cached_property
    def case(self):
        return self._make()


def _plant(prob, planted, seed=0):
    for f in planted:
        prob = ts.make_outlier(prob, f, seed=seed)
    return prob


def _tracks_from(prob, tracks):
    for k in TRACK_KEYS:
        setattr(prob, k, getattr(tracks, k))
    return prob


def _opts(do_fej=1, pose=1, intr=1, **kw):
    return capi.default_options(chi2_multipler=1.0, do_fej=do_fej, do_calib_camera_pose=pose, do_calib_camera_intrinsics=intr, **kw)


# --------------------------------------------------------------------------- track length at the tile edges
LEN_SEED = {2: 31, 3: 31, 8: 31, 9: 31, 10: 31}


def _len_case(m):
    prob = ts.exact_length(synth.make_problem(2, C=12, F=8, seed=LEN_SEED[m]), m, patterns=("stride",))
    return Case(prob, capi.REP_GLOBAL_3D)


def _long_case(m_long):
    prob = synth.make_problem(2, C=33, K=2, F=8, seed=50)
    prob = prob.subset(np.flatnonzero(np.diff(prob.meas_offsets) > M_MAX)[:3])
    return Case(ts.with_lengths(prob, long_lengths(m_long), patterns=("stride",)), capi.REP_GLOBAL_3D)


def long_lengths(m_long):
    return [10, m_long, 12]


# --------------------------------------------------------------------------- representations and flags
REP_SEED = 42
REP_PLANTED = (3,)


def _rep_case(rep, flags):
    do_fej, K, pose, intr = flags
    prob = synth.make_problem(2, C=10, K=K, F=8, seed=REP_SEED, fisheye=(K == 1))
    return Case(_plant(prob, REP_PLANTED), rep, opts=_opts(do_fej, pose, intr))


# --------------------------------------------------------------------------- where the decision moved
GATE_SEED = 61
GATE_F = 12


def _gate_case(planted, rep=capi.REP_GLOBAL_3D, F=GATE_F, outlier_seed=0):
    return Case(_plant(synth.make_problem(2, C=12, F=F, seed=GATE_SEED), planted, outlier_seed), rep)


# --------------------------------------------------------------------------- the covariance dimension at a tile edge
EDGE_PLANTED = (5,)
EDGE_LM = {14: [0, 0, 0, 0, SINGLE, SINGLE], 15: [0, 0, 0, 0, 0], 0: []}  # resident landmarks behind N = 96 (11 clones, one camera)


def _edge_case(mod):
    tracks = _plant(synth.make_problem(2, C=11, K=1, F=12, seed=33), EDGE_PLANTED)
    reps = np.array(EDGE_LM[mod], np.int32)
    if len(reps) == 0:
        return Case(tracks, capi.REP_GLOBAL_3D)
    return Case(_tracks_from(synth.make_slam_problem(2, L=len(reps), lm_rep=reps, C=11, K=1, seed=33), tracks), capi.REP_GLOBAL_3D, slam=True)


# --------------------------------------------------------------------------- per-feature sigma and multiplier
SIGMA_PLANTED = (1, 7)


def sigma_arrays(F=GATE_F):
    tag = np.random.default_rng(5).random(F) < 0.4
    return tag, np.where(tag, 2.5, 1.0), np.where(tag, 3.0, 1.0)


def _sigma_case(rep, sigma_pix=1.0):
    _, sig, mult = sigma_arrays()
    prob = _plant(synth.make_problem(2, C=12, F=GATE_F, seed=GATE_SEED), SIGMA_PLANTED)
    return Case(prob, rep, opts=_opts(sigma_pix=sigma_pix), sig=sig, mult=mult)


# --------------------------------------------------------------------------- resident landmarks
RESIDENT_REPS = np.array([0, 4, 5, 2, 4, 5], np.int32)
RESIDENT_PLANTED = (5,)


def resident_state():
    return synth.make_slam_problem(2, L=6, lm_rep=RESIDENT_REPS, C=12, seed=21)


def _resident_case():
    tracks = _plant(synth.make_problem(2, C=12, F=10, seed=34), RESIDENT_PLANTED)
    return Case(_tracks_from(resident_state(), tracks), capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, slam=True)


def _shapes():
    out = []
    for m in TRACKS:
        out.append(Shape(f"len-{m}", functools.partial(_len_case, m), lengths=[m] * 8))
    for m in (M_MAX, M_MAX + 1):
        out.append(Shape(f"len-{m}", functools.partial(_long_case, m), lengths=long_lengths(m)))
    for rep in REPS6:
        for i, flags in enumerate(FLAG_SETS):
            out.append(Shape(f"rep{rep}-flags{i}", functools.partial(_rep_case, rep, flags), planted=REP_PLANTED))
    out.append(Shape("out-first", functools.partial(_gate_case, (0,)), planted=(0,)))
    out.append(Shape("out-middle", functools.partial(_gate_case, (5,)), planted=(5,)))
    out.append(Shape("out-last", functools.partial(_gate_case, (GATE_F - 1,), outlier_seed=1), planted=(GATE_F - 1,)))
    out.append(Shape("out-pair", functools.partial(_gate_case, (4, 5)), planted=(4, 5)))
    out.append(Shape("out-all", functools.partial(_gate_case, tuple(range(5)), capi.REP_ANCHORED_3D, 5), planted=tuple(range(5))))
    out.append(Shape("tri-failed", functools.partial(_gate_case, ()), tri_failed={5: capi.FEAT_TRI_FAILED}))
    out.append(Shape("two-rejected", functools.partial(_gate_case, (2, 7), capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH), planted=(2, 7)))
    for mod in EDGES:
        out.append(Shape(f"edge-{mod}", functools.partial(_edge_case, mod), planted=EDGE_PLANTED, n0_mod16=mod))
    out.append(Shape("sigma-global", functools.partial(_sigma_case, capi.REP_GLOBAL_3D), planted=SIGMA_PLANTED))
    out.append(Shape("sigma-single", functools.partial(_sigma_case, SINGLE), planted=SIGMA_PLANTED))
    # the same per-feature sigma for every candidate under another context sigma: oscale = sigma / sigma_f differs, the statistic must not
    out.append(Shape("sigma-global-ctx3", functools.partial(_sigma_case, capi.REP_GLOBAL_3D, 3.0), planted=SIGMA_PLANTED))
    out.append(Shape("sigma-single-ctx3", functools.partial(_sigma_case, SINGLE, 3.0), planted=SIGMA_PLANTED))
    out.append(Shape("resident", _resident_case, planted=RESIDENT_PLANTED))
    return out


SHAPES = _shapes()
BY_ID = {s.id: s for s in SHAPES}
assert len(BY_ID) == len(SHAPES)


class TriangulationWith:
    """The oracle with statuses injected into its triangulation (a candidate whose triangulation failed, as ovgpu_set_triangulation hands it over)."""

    def __init__(self, oracle, failed):
        self._oracle, self._failed = oracle, failed

    def triangulate(self, opts, views):
        tri = dict(self._oracle.triangulate(opts, views))
        tri["status"] = np.array(tri["status"], copy=True)
        for f, st in self._failed.items():
            tri["status"][f] = st
        return tri

    def slam_delayed_init(self, *args, **kw):
        return self._oracle.slam_delayed_init(*args, **kw)


def oracle_for(oracle, shape):
    return TriangulationWith(oracle, shape.tri_failed) if shape.tri_failed else oracle
