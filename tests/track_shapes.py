"""Snapshots with PRESCRIBED tracks, and the catalogue of batches that pin the per-feature kernels at their track-length and region edges
(tests/test_track_shapes_cpu.py checks every batch on the oracle alone, tests/test_gpu_track_edges.py runs it on the device).

The MSCKF fast path picks its per-feature kernel from the observation count m_max of the batch's longest track (set_row_layout, api_state.inc),
and the unprojected stack from the column count D of the state (build_columns / raw_stack_layout).  expected_kernel() and expected_raw() below
restate those two rules FROM THE DOCUMENTED TILE BUDGETS, not from the library: the tests compare what the library reports with them.

A helper module, not a conftest: nothing here is collected.
"""
from __future__ import annotations

import copy
import functools
from dataclasses import dataclass, field

import numpy as np

from open_vins_amd import capi, synth

PATTERNS = ("prefix", "suffix", "stride", "one_camera")


# --------------------------------------------------------------------------- the one entry: feature f keeps exactly picks[f]
def keep_tracks(prob, picks):
    """A Problem whose feature f keeps exactly the observations picks[f]: indices INTO ITS OWN track (0 .. m_f - 1), in the order given, repeats
    allowed (an ascending list keeps synth's order: camera groups descending, clones ascending, as Problem.subset does).  An empty list leaves
    an empty track."""
    assert len(picks) == prob.F
    sel, offs = [], [0]
    for f, pk in enumerate(picks):
        a, b = int(prob.meas_offsets[f]), int(prob.meas_offsets[f + 1])
        pk = np.asarray(pk, dtype=np.int64).reshape(-1)
        assert pk.size == 0 or (pk.min() >= 0 and pk.max() < b - a), (f, b - a)
        sel.append(a + pk)
        offs.append(offs[-1] + pk.size)
    sel = np.concatenate(sel) if sel else np.zeros(0, np.int64)
    q = copy.copy(prob)
    q.meas_offsets = np.asarray(offs, dtype=np.int32)
    q.uv = np.ascontiguousarray(prob.uv.reshape(-1, 2)[sel].reshape(-1))
    q.uvn = np.ascontiguousarray(prob.uvn.reshape(-1, 2)[sel].reshape(-1))
    q.clone_idx, q.cam_idx = np.ascontiguousarray(prob.clone_idx[sel]), np.ascontiguousarray(prob.cam_idx[sel])
    return q


def pick(prob, f, length, pattern="prefix", clones=None):
    """`length` observations of feature f as a list for keep_tracks.  pattern: "prefix" / "suffix" of the track, "stride" (every k-th
    observation from the first on, k the largest that still gives `length`: the widest baseline), "one_camera" (only the camera that saw the point most often); clones = (c0, c1)
    keeps observations of clones c0 <= c < c1 only.  A track that holds fewer than `length` such observations keeps ALL of them, in order, and is
    topped up by repeating them from the start (distinct (camera, clone) pairs first, repetition only tops up)."""
    a, b = int(prob.meas_offsets[f]), int(prob.meas_offsets[f + 1])
    idx = np.arange(b - a)
    cl, cam = prob.clone_idx[a:b], prob.cam_idx[a:b]
    if clones is not None:
        idx = idx[(cl >= clones[0]) & (cl < clones[1])]
    if pattern == "one_camera" and idx.size:
        cams, cnt = np.unique(cam[idx], return_counts=True)
        idx = idx[cam[idx] == cams[np.argmax(cnt)]]
    if length == 0:
        return idx[:0]
    assert idx.size > 0, f"feature {f} has no observation to keep"
    if idx.size >= length:
        if pattern == "suffix":
            return idx[idx.size - length:]
        if pattern == "stride":
            return idx[::max(1, (idx.size - 1) // max(1, length - 1))][:length]
        return idx[:length]
    return np.concatenate([idx, np.resize(idx, length - idx.size)])


def with_lengths(prob, lengths, patterns=PATTERNS, clones=None):
    """Feature f trimmed (or topped up) to exactly lengths[f] observations by patterns[f % len(patterns)]; None leaves a track as it is."""
    picks = []
    for f in range(prob.F):
        m = int(prob.meas_offsets[f + 1] - prob.meas_offsets[f])
        picks.append(np.arange(m) if lengths[f] is None else pick(prob, f, int(lengths[f]), patterns[f % len(patterns)], clones))
    return keep_tracks(prob, picks)


def exact_length(prob, m, n=None, patterns=PATTERNS, clones=None):
    """Every feature (n = None) or only the first n features trimmed to exactly m observations, one pick pattern after the other."""
    n = prob.F if n is None else n
    return with_lengths(prob, [m if f < n else None for f in range(prob.F)], patterns, clones)


def clone_range(prob, c0, c1):
    """Every track restricted to the clones c0 <= c < c1 (the oldest n: (0, n); the newest n: (C - n, C))."""
    picks = []
    for f in range(prob.F):
        cl = prob.clone_idx[int(prob.meas_offsets[f]):int(prob.meas_offsets[f + 1])]
        picks.append(np.flatnonzero((cl >= c0) & (cl < c1)))
    return keep_tracks(prob, picks)


def one_per_class(prob, cls_of_clone):
    """Every track reduced to exactly ONE observation per class of clones (cls_of_clone[c]: region_classes): its first one in that class."""
    picks = []
    for f in range(prob.F):
        cl = prob.clone_idx[int(prob.meas_offsets[f]):int(prob.meas_offsets[f + 1])]
        k = np.asarray(cls_of_clone)[cl]
        pk = sorted(int(np.flatnonzero(k == c)[0]) for c in np.unique(k))
        picks.append(np.asarray(pk))
    return keep_tracks(prob, picks)


def longest(prob, n):
    """The n features with the most observations, in batch order."""
    m = np.diff(prob.meas_offsets)
    return prob.subset(np.sort(np.argsort(-m, kind="stable")[:n]))


def reorder(prob, order):
    return prob.subset(order)


def make_outlier(prob, f, px=15.0, seed=0):
    """Feature f's pixels moved by +-px in both coordinates, signs drawn per observation — synth.make_problem's gross outlier on a feature of
    one's choice; the normalised coordinates follow through the same undistortion.  Returns a copy."""
    q = copy.copy(prob)
    a, b = int(prob.meas_offsets[f]), int(prob.meas_offsets[f + 1])
    rng = np.random.default_rng([int(seed), 17, int(f)])
    uv = prob.uv.reshape(-1, 2).copy()
    uvn = prob.uvn.reshape(-1, 2).copy()
    uv[a:b] = (uv[a:b].astype(np.float64) + px * rng.choice([-1.0, 1.0], (b - a, 2))).astype(np.float32)
    fisheye = bool(prob.meta.get("fisheye"))
    intr = np.asarray(synth._INTRINSICS_EQUI if fisheye else synth._INTRINSICS, dtype=np.float64)
    und = synth.equi_undistort if fisheye else synth.radtan_undistort
    for i in range(a, b):
        x, y = und(intr[prob.cam_idx[i]], np.float64(uv[i, 0]), np.float64(uv[i, 1]))
        uvn[i] = np.float32(x), np.float32(y)
    q.uv, q.uvn = np.ascontiguousarray(uv.reshape(-1)), np.ascontiguousarray(uvn.reshape(-1))
    return q


# --------------------------------------------------------------------------- the two rules, restated
def expected_kernel(m_max, shape=0, general=False):
    """ovgpu_debug_option "last_feature_kernel" for a batch whose longest track holds m_max observations: the gate matrix of the one-pass kernels has
    2 m + 4 rows in nta = ceil((2 m + 4) / 16) tile rows, nta (nta + 1) / 2 tiles of its upper triangle: <4 wavefronts x 9 tiles> hold 36 (1:
    m <= 62), <8 x 17> hold 136 (2: m <= 126), the block-row kernel nt = ceil(2 m / 16) <= 29 tile rows (3: m <= 232), the general kernel
    the rest (0).  options.feature_kernel_shape = 2 puts every batch that <8 x 17> holds there and leaves the others to the general kernel."""
    nta, nt = (2 * m_max + 4 + 15) // 16, (2 * m_max + 15) // 16
    tiles = nta * (nta + 1) // 2
    if general or m_max < 2:
        return 0
    if tiles <= 36 and shape != 2:
        return 1
    if tiles <= 136:
        return 2
    return 3 if (nt <= 29 and shape == 0) else 0


def n_columns(C, K, pose=1, intr=1):
    return 6 * C + K * (6 * (1 if pose else 0) + 8 * (1 if intr else 0))


def expected_raw(D, kernel, big=0, fp32=0):
    """ovgpu_debug_option "last_stack_raw": the unprojected stack in regions for 6 <= ceil((D + 1) / 16) <= 15 (synth's states keep the calibration
    columns left of the clones and carry no landmarks); written by the one-pass float64 kernels only."""
    return int(6 <= (D + 1 + 15) // 16 <= 15 and kernel in (1, 2) and not big and not fp32)


def region_classes(C, K, pose=1, intr=1):
    """The classes of clones of the unprojected stack for synth's column order (per camera [pose 6 | intrinsics 8], then the clones): region t of
    t = 4, 6, ... tile columns below the top ends at column 16 t - 4 and exists when the calibration columns and one clone block fit in
    front of it; a clone belongs to the first region its block ends in, the top region otherwise.  Returns (class of every clone, count)."""
    D = n_columns(C, K, pose, intr)
    calib_end = D - 6 * C
    ntf = (D + 1 + 15) // 16
    top = 15 if ntf == 15 else (ntf + 1) & ~1
    rcol = [16 * t - 4 for t in range(4, top, 2) if 16 * t - 4 >= calib_end + 6]
    cls = [next((k for k, r in enumerate(rcol) if calib_end + 6 * c + 6 <= r), len(rcol)) for c in range(C)]
    return np.asarray(cls), len(rcol) + 1


# --------------------------------------------------------------------------- states and base tracks
@functools.lru_cache(maxsize=None)
def _base(C, K, F, seed, calib_noise):
    """F full tracks (the longest of 4 F candidates) on the C x K window of seed `seed`.  Cached: the helpers above copy, never modify.
    calib_noise = 0: the calibration estimate is the truth — for states whose calibration is NOT estimated (an error the filter does not
    model would reject every long track at chi2_multipler = 1)."""
    return longest(synth.make_problem(5 if K == 4 else 2, C=C, K=K, F=4 * F, seed=seed, calib_noise=calib_noise), F)


SMALL = dict(C=30, K=2)                  # D = 208: 14 tile columns, the unprojected stack
MID = dict(C=30, K=4)                    # D = 236: 15
LARGE = dict(C=60, K=4, pose=0, intr=0)  # D = 360 <= 383: the Gram route (and with it the fused kernels) up to 240 observations per track


def state_for(m):
    return SMALL if m <= 57 else (MID if m <= 121 else LARGE)


@dataclass
class Case:
    id: str
    group: str
    build: object                      # () -> Problem
    state: dict
    options: dict = field(default_factory=dict)   # capi.default_options keywords on top of chi2_multipler = 1
    debug: dict = field(default_factory=dict)     # ovgpu_debug_option settings
    m_max: int | None = None           # None: whatever the batch holds (the expected kernel follows from it by the same rule)
    outliers: bool = True

    @property
    def D(self):
        s = self.state
        return n_columns(s["C"], s["K"], s.get("pose", 1), s.get("intr", 1))

    @property
    def kernel(self):
        return expected_kernel(self.longest_track, self.options.get("feature_kernel_shape", 0), bool(self.options.get("no_fast_feature_kernel", 0)))

    @property
    def raw(self):
        return expected_raw(self.D, self.kernel, self.debug.get("featy_big", 0), self.options.get("gram_fp32", 0))

    def opts(self, **more):
        s = self.state
        kw = dict(chi2_multipler=1.0, gate_always_factor=1, do_calib_camera_pose=s.get("pose", 1), do_calib_camera_intrinsics=s.get("intr", 1))
        kw.update(self.options)
        kw.update(more)
        return capi.default_options(**kw)

    @functools.cached_property
    def prob(self):
        return self.build()

    @property
    def longest_track(self):
        return int(np.diff(self.prob.meas_offsets).max()) if self.m_max is None else self.m_max


def _window(state, F, seed):
    return _base(state["C"], state["K"], F, seed, 1.0 if state.get("pose", 1) and state.get("intr", 1) else 0.0)


# (a) uniform batches: six features of one length, one per pick pattern (the four, then the widest one on two more points), one an outlier
SIX = PATTERNS + ("stride", "stride")
SWEEP = [2, 3, 6, 7, 8, 9, 14, 15, 16, 17, 54, 55, 56, 57, 62, 63, 64, 65, 70, 71, 72, 118, 119, 120, 121, 126, 127, 128, 129,
         199, 200, 201, 224, 231, 232, 233, 240]
EDGES = [62, 63, 126, 127, 232, 233]
# Gross offset of the outlier: 15 px as synth.make_problem's, 10 px under ten observations (a larger one fails the triangulation of so short a
# track instead of reaching the gate).  A 2-observation track leaves ONE projected row against a prior of tens of pixels: of the offsets that still
# triangulate (6 .. 200 px tried on five seeds) none is rejected — chi2 stays under 0.91 of the threshold — so that batch alone expects no rejection.


def uniform_batch(m, seed=0):
    st = state_for(m)
    p = exact_length(_window(st, 6, 100 + seed), m, patterns=SIX)
    return make_outlier(p, 4, 10.0 if m < 10 else 15.0, seed)


MIXED_SHORT = [2, 3, 7, 8, 9, 15, 16, 31, 32, 1, 0]


def mixed_batch(m_long, long_first, seed=0):
    """One track of m_long observations, nine short ones, a 1-observation track and an empty one: features of one tile row under the longest's."""
    st = state_for(m_long)
    p = with_lengths(_window(st, 12, 200 + seed), [m_long] + MIXED_SHORT)
    p = make_outlier(p, 9, 15.0, seed)  # the 32-observation track
    return p if long_first else reorder(p, list(range(1, 12)) + [0])


def _cases():
    out = []
    for m in SWEEP:
        out.append(Case(f"a-{m}", "a", functools.partial(uniform_batch, m), state_for(m), m_max=m, outliers=m > 2))
    for m in EDGES:  # one leg per edge with the library's default gate (residual bound first)
        out.append(Case(f"a-{m}-default", "a", functools.partial(uniform_batch, m), state_for(m), options=dict(gate_always_factor=0), m_max=m))
    for m in (62, 63, 126, 127, 232):
        for first in (True, False):
            out.append(Case(f"b-{m}-{'first' if first else 'last'}", "b", functools.partial(mixed_batch, m, first), state_for(m), m_max=m))
    forced = [("big1", {}, dict(featy_big=1)), ("big2", {}, dict(featy_big=2)), ("shape2", dict(feature_kernel_shape=2), {}),
              ("general", dict(no_fast_feature_kernel=1), {})]
    for name, o, d in forced:
        out.append(Case(f"c-9-{name}", "c", functools.partial(uniform_batch, 9), state_for(9), options=o, debug=d, m_max=9))
        out.append(Case(f"c-119-{name}", "c", functools.partial(uniform_batch, 119), state_for(119), options=o, debug=d, m_max=119))
        out.append(Case(f"c-mixed126-{name}", "c", functools.partial(mixed_batch, 126, True), state_for(126), options=o, debug=d, m_max=126))
    for m in (62, 63, 126, 127):
        out.append(Case(f"d-{m}-fp32", "d", functools.partial(uniform_batch, m), state_for(m), options=dict(gram_fp32=1), m_max=m))
    anch = dict(feat_rep_msckf=capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH)
    out.append(Case("e-63-anchored", "e", functools.partial(uniform_batch, 63), state_for(63), options=anch, m_max=63))
    out.append(Case("e-mixed126-anchored", "e", functools.partial(mixed_batch, 126, True), state_for(126), options=anch, m_max=126))
    out += _region_cases()
    return out


# (f) states by ceil((D + 1) / 16), full tracks of 8 points (one an outlier) unless the case says otherwise
REGION_STATES = {
    "nt5": dict(C=10, K=1),                       # D = 74: off
    "nt6": dict(C=12, K=1),                       # D = 86
    "nt7": dict(C=16, K=1),                       # D = 110: an odd count, the top region rounded to 8
    "nt14": dict(C=34, K=1),                      # D = 218
    "nt15": dict(C=35, K=2),                      # D = 238: k_gram_il<15>
    "nt16": dict(C=36, K=2),                      # D = 244: off
    "D96": dict(C=14, K=2, pose=1, intr=0),       # D = 96: the top tile column holds the residual column alone
    "D144": dict(C=24, K=1, pose=0, intr=0),      # D = 144, and no calibration column at all
    "K4": dict(C=20, K=4),                        # D = 176, calibration ends at 56: 56 + 6 > 60, the narrowest region class is dropped
}


def region_batch(name, F=8, how="full", seed=0):
    st = REGION_STATES[name]
    p = _window(st, F, 300 + seed)
    if how == "oldest":  # only clones of the narrowest region: the top region holds no rows of Y
        cls, _ = region_classes(st["C"], st["K"], st.get("pose", 1), st.get("intr", 1))
        p = clone_range(p, 0, int(np.sum(cls == 0)))
    elif how == "newest":  # only clones of the top region
        cls, n = region_classes(st["C"], st["K"], st.get("pose", 1), st.get("intr", 1))
        p = clone_range(p, int(np.sum(cls < n - 1)), st["C"])
    elif how == "one_per_class":
        cls, n = region_classes(st["C"], st["K"], st.get("pose", 1), st.get("intr", 1))
        p = one_per_class(p, cls)
        assert int(np.diff(p.meas_offsets).max()) == n
    return make_outlier(p, F - 1, 15.0, seed) if F >= 5 else p


def _region_cases():
    out = []

    def add(cid, name, outliers=True, **kw):
        build = functools.partial(region_batch, name, **kw)
        out.append(Case(cid, "f", build, REGION_STATES[name], outliers=outliers and kw.get("F", 8) >= 5))

    for name in REGION_STATES:
        add(f"f-{name}", name, seed=4 if name == "nt5" else 0)  # (seeds: the oracle triangulates at least one full track of the window)
    for how in ("oldest", "newest", "one_per_class"):
        add(f"f-K4-{how}", "K4", how=how)
    add("f-nt14-newest", "nt14", how="newest")
    add("f-nt14-one_per_class", "nt14", how="one_per_class")
    add("f-nt15-one_per_class", "nt15", how="one_per_class")
    add("f-nt15-oldest", "nt15", outliers=False, how="oldest")  # (ten observations from five neighbouring clones: two of the eight points triangulate, the outlier does not)
    for F in (1, 2, 5):
        add(f"f-nt14-F{F}", "nt14", F=F)
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def oracle_run(oracle, case):
    """(triangulation, update) of the oracle for a case: the reference every leg of the case is held to.  Cached on the case."""
    if not hasattr(case, "_ref"):
        v = capi.Views(case.prob)
        opts = case.opts()
        tri = oracle.triangulate(opts, v)
        case._ref = (tri, oracle.msckf_update(opts, v, want_compressed=False, given=tri))
    return case._ref
