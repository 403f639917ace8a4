"""The catalogue of batches that pin the GENERAL per-feature kernel (csrc/k_system.h: k_system_t<false> / <true>) at its LDS-carve, panel and loop
edges: tests/test_system_shapes_cpu.py checks every batch on the oracle alone, tests/test_gpu_system_edges.py runs it on the device.

carve() restates the kernel's LDS carve FROM ITS DOCUMENTED TERMS (the header of k_system.h and size_feature_stage's comments, api_state.inc), not
from the library: the GPU tests compare what the library reports ("sys_m_lds_max", "sys_rows_global", "sys_row_stride") with it.

  fixed part of the carve for a batch whose longest track holds m observations, records of `stride` doubles, D Jacobian columns:
      32 m bytes of block ids (rounded up to 16) + 8 stride m of records + 48 m of reflectors + 512 of scratch + 128 D of T chunk, rounded up to 16;
  when that does not fit under the limit the records leave LDS (a global workspace, k_system_t<true>) and the fixed part loses their term;
  when it still does not fit the batch is refused;
  the gate matrix of a track of m' observations holds n (n + 1) / 2 + 4 n doubles, n = 2 m': m_lds_max is the largest m' <= m whose matrix fits
  in what the fixed part leaves.

Role edges of a (stride, D, limit): g the first longest-track length whose OWN gate matrix is global, r the first whose records are global.  The
lengths of groups (b), (d) and (e) are computed from the limit the device reports ("sys_lds_limit"), so every case takes a byte limit.

Triangulated kinds (MSCKF, delayed initialisation) inject the oracle's positions OF THE CLEAN BATCH on both sides: the planted outlier then reaches
the gate whatever its length (a gross offset fails the triangulation of a short track otherwise, tests/track_shapes.py).

A helper module, not a conftest: nothing here is collected.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import slam_shapes as ss
import track_shapes as ts
from open_vins_amd import capi

LIMITS = (160 * 1024, 64 * 1024)  # the MI355X's workgroup limit, and the limit of a 64 KB part
FUSED_MAX = 232                   # the longest track the fused MSCKF kernels hold (track_shapes.expected_kernel)
SINGLE = capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE


# --------------------------------------------------------------------------- the carve, restated
def _up16(b):
    return (b + 15) & ~15


def fixed_bytes(m, row_stride, D, rows_in_lds=True):
    b = _up16(32 * m)
    if rows_in_lds:
        b += 8 * row_stride * m
    return _up16(b + 48 * m + 512 + 128 * D)


def gate_doubles(m):
    n = 2 * m
    return n * (n + 1) // 2 + 4 * n


def carve(m_max, row_stride, D, lds_limit):
    """(m_lds_max, rows_global, refused) of a batch whose longest track holds m_max observations"""
    m = max(int(m_max), 1)
    fixed, rows_global = fixed_bytes(m, row_stride, D), False
    if fixed >= lds_limit:
        fixed, rows_global = fixed_bytes(m, row_stride, D, False), True
    if fixed >= lds_limit:
        return 0, rows_global, True
    m_lds = 0
    while m_lds < m_max and 8 * gate_doubles(m_lds + 1) <= lds_limit - fixed:
        m_lds += 1
    return m_lds, rows_global, False


def lds_bytes(m_max, row_stride, D, lds_limit):
    """the launch's dynamic LDS size: the fixed part and the largest resident gate matrix"""
    m_lds, rows_global, refused = carve(m_max, row_stride, D, lds_limit)
    assert not refused
    return fixed_bytes(max(int(m_max), 1), row_stride, D, not rows_global) + 8 * gate_doubles(m_lds)


@functools.lru_cache(maxsize=None)
def edges(row_stride, D, lds_limit):
    """(g, r); None where the role does not exist below the refusal edge"""
    g = r = None
    for m in range(1, 4096):
        m_lds, rows_global, refused = carve(m, row_stride, D, lds_limit)
        if refused:
            break
        if g is None and m_lds < m:
            g = m
        if r is None and rows_global:
            r = m
    return g, r


def role_length(role, row_stride, D, lds_limit):
    if isinstance(role, int):
        return role
    g, r = edges(row_stride, D, lds_limit)
    return {"g-1": g - 1, "g": g, "g+1": g + 1, "r-1": r - 1, "r": r}[role]


def panel_blocks(m):
    """how the gate's 2 m + 4 trapezoid rows are factored: ("p2",) up to 128 rows, ("p8",) up to 512, then the resident panel and one rest block per
    further 512 rows"""
    rows = 2 * m + 4
    if rows <= 128:
        return ("p2",)
    if rows <= 512:
        return ("p8",)
    return ("p8-resident",) + ("rest",) * (-(-(rows - 512) // 512))


# --------------------------------------------------------------------------- cases
@dataclass
class Case:
    id: str
    group: str
    kind: str                                      # "msckf" | "slam" | "init"
    role: object                                   # the longest track: a length, or "g-1" / "g" / "g+1" / "r-1" / "r" of the case's own (stride, D)
    make: object                                   # (m_long, limit) -> (clean Problem, Problem with the outlier planted, index of the long track)
    state: dict                                    # C, K, pose, intr (and for SLAM the landmarks' representations in `reps`)
    options: dict = field(default_factory=dict)
    debug: dict = field(default_factory=dict)
    rep: int = 0                                   # "init": the representation the candidates are initialised in
    sigma: object = None                           # "slam": per-feature sigma_pix / chi2_multipler
    mult: object = None
    long_rejected: bool = False                    # the long track is the planted outlier

    @property
    def row_stride(self):
        if self.kind == "slam":
            anchored = any(int(r) >= capi.REP_ANCHORED_3D for r in self.state["reps"])
        elif self.kind == "init":
            anchored = self.rep >= capi.REP_ANCHORED_3D
        else:
            anchored = False
        return 72 if anchored or self.options.get("feat_rep_msckf", 0) >= capi.REP_ANCHORED_3D else 48

    @property
    def D(self):
        s = self.state
        d = ts.n_columns(s["C"], s["K"], s.get("pose", 1), s.get("intr", 1))
        if self.kind == "slam":
            d += int(sum(1 if int(r) == SINGLE else 3 for r in s["reps"]))
        return d

    def length(self, limit):
        return role_length(self.role, self.row_stride, self.D, limit)

    def carve(self, limit):
        return carve(self.length(limit), self.row_stride, self.D, limit)

    def opts(self, **more):
        s = self.state
        kw = dict(chi2_multipler=1.0, gate_always_factor=1, do_calib_camera_pose=s.get("pose", 1), do_calib_camera_intrinsics=s.get("intr", 1))
        if self.length(LIMITS[0]) <= FUSED_MAX or isinstance(self.role, str):
            kw["no_fast_feature_kernel"] = 1       # (beyond the fused kernels' bound the default dispatch reaches the general kernel by itself)
        kw.update(self.options)
        kw.update(more)
        return capi.default_options(**kw)

    @functools.lru_cache(maxsize=None)
    def batch(self, limit):
        clean, prob, f_long = self.make(self.length(limit), limit)
        return clean, prob, f_long

    def __hash__(self):
        return hash(self.id)


MONO = dict(C=16, K=1)   # D = 110 (REGION_STATES "nt7"): groups (a), (d) and (e)
STEREO = dict(C=30, K=2)  # D = 208: group (b) and the cross-checks, the window of configs[2]


def _window(state, F, seed):
    return ts._window(state, F, seed)


def msckf_mixed(state, m_long, shorts, outlier, long_first, seed, px=15.0):
    """the long track, the short ones (none longer than the long one), feature `outlier` (an index into [long] + shorts, 0: the long track) moved
    by px pixels; long_first = False: the long track goes last"""
    lens = [m_long] + [min(int(s), m_long) for s in shorts]
    clean = ts.with_lengths(_window(state, len(lens), seed), lens, patterns=("stride",))
    prob = ts.make_outlier(clean, outlier, px, seed)
    f_long = 0
    if not long_first:
        order = list(range(1, len(lens))) + [0]
        clean, prob, f_long = ts.reorder(clean, order), ts.reorder(prob, order), len(lens) - 1
    return clean, prob, f_long


A_LENGTHS = [2, 3, 7, 8, 9, 61, 62, 63, 64, 65, 254, 255, 256, 257, 510, 511]
A_SHORTS = [0, 1, 2, 3, 8, 9, 32, 16]  # (the 16-observation track is the gross outlier of the "first" legs)
# seeds and offsets: chosen on the CPU (tests/test_system_shapes_cpu.py holds every case to it)
A_SEED = {(2, True): 2, (9, True): 2}
A_PX = {2: 60.0, 3: 30.0}  # a track of 2 / 3 observations leaves one / three projected rows against a prior of tens of pixels


def _a_case(m, first):
    seed = A_SEED.get((m, first), 0)

    def make(m_long, limit):
        if first:
            return msckf_mixed(MONO, m_long, A_SHORTS, len(A_SHORTS), True, seed, A_PX.get(m, 15.0))
        return msckf_mixed(MONO, m_long, A_SHORTS[:-1], 0, False, seed, A_PX.get(m, 15.0))
    return Case(f"a-{m}-{'first' if first else 'last'}", "a", "msckf", m, make, MONO, long_rejected=not first)


B_STATES = {
    "global3d": (dict(), dict()),
    "anchored-msckf-invdepth": (dict(feat_rep_msckf=capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH), dict(anchored_fast=0)),
    "anchored3d": (dict(feat_rep_msckf=capi.REP_ANCHORED_3D), dict(anchored_fast=0)),
}
B_ROLES = ["g-1", "g", "g+1", "r-1", "r"]
B_SEED = {}


def _b_case(name, role):
    o, d = B_STATES[name]
    stride = 72 if o else 48

    def make(m_long, limit):
        m_lds = carve(m_long, stride, 208, limit)[0]
        both = [m_lds, m_lds + 1] if role == "r-1" else [2, 3]  # at r - 1: a track whose S is resident and one whose S is global, in one batch
        return msckf_mixed(STEREO, m_long, both + [8, 9, 32, 1, 0, 16], 8, True, B_SEED.get((name, role), 0))
    return Case(f"b-{name}-{role}", "b", "msckf", role, make, STEREO, options=o, debug=d)


C_MSCKF = {250: dict(C=37, K=2), 256: dict(C=38, K=2), 262: dict(C=39, K=2)}
C_SLAM = (255, 257)
C_SEED = {}


def _c_msckf(D, m):
    st = C_MSCKF[D]

    def make(m_long, limit):
        return msckf_mixed(st, m_long, [3, 9, 32, 0, 16], 5, True, C_SEED.get((D, m), 0))
    return Case(f"c-msckf-D{D}-{m}", "c", "msckf", m, make, st)


def slam_mixed(state, m_long, seed, outlier=3, **kw):
    """ss.length_batch on a state of one's choice: the long track first, an EMPTY track, four shorter ones, the 12-observation one a gross outlier"""
    reps = list(state["reps"])
    L = len(reps)
    p = ss.slam(L, reps, seed, C=state["C"], K=state["K"], pose=state.get("pose", 1), intr=state.get("intr", 1), **kw)
    short = [5, 0, 12, 9, 3] + [7, 10, 4, 6, 11, 8][:max(0, L - 6)]
    clean = ts.with_lengths(p, [m_long] + [min(s, m_long) for s in short[:L - 1]], patterns=("prefix",))
    prob = ts.make_outlier(clean, outlier, 15.0, seed) if outlier is not None else clean
    return clean, prob, 0


def _c_slam(D, m):
    cs = ss.COLUMN_STATES[D]
    st = dict(C=cs["C"], K=cs["K"], reps=(ss.REPS5 * 3)[:cs["L"]])

    def make(m_long, limit):
        return slam_mixed(st, m_long, C_SEED.get((D, m), 21))
    return Case(f"c-slam-D{D}-{m}", "c", "slam", m, make, st)


D_ROLES = [62, 63, "g-1", "g"]
D_SLAM_REPS = ss.REPS5 + [SINGLE]
D_INIT_REPS = [capi.REP_GLOBAL_3D, capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, SINGLE]
D_SEED = {}


def _d_slam(rep, role):
    st = dict(MONO, reps=[rep] * 6)

    def make(m_long, limit):
        return slam_mixed(st, m_long, D_SEED.get(("slam", rep, role), 40 + rep))
    return Case(f"d-slam-rep{rep}-{role}", "d", "slam", role, make, st)


def _d_init(rep, role):
    def make(m_long, limit):
        return msckf_mixed(MONO, m_long, [5, 0, 12, 9, 3], 3, True, D_SEED.get(("init", rep, role), 0))
    return Case(f"d-init-rep{rep}-{role}", "d", "init", role, make, MONO, rep=rep)


def _d_noise(role):
    st = dict(MONO, reps=ss.MIX10)

    def make(m_long, limit):
        return slam_mixed(st, m_long, D_SEED.get(("noise", role), 3), outlier=None)
    return Case(f"d-noise-{role}", "d", "slam", role, make, st, sigma=ss.NOISE_SIGMA, mult=ss.NOISE_MULT)


def _cases():
    out = [_a_case(m, first) for m in A_LENGTHS for first in (True, False)]
    out += [_b_case(name, role) for name in B_STATES for role in B_ROLES]
    out += [_c_msckf(D, m) for D in C_MSCKF for m in (62, 63)]
    out += [_c_slam(D, m) for D in C_SLAM for m in (62, 63)]
    out += [_d_slam(rep, role) for rep in D_SLAM_REPS for role in D_ROLES]
    out += [_d_init(rep, role) for rep in D_INIT_REPS for role in D_ROLES]
    out += [_d_noise(role) for role in D_ROLES]
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


# --------------------------------------------------------------------------- the two cross-checks and the chain of group (e)
X_SHORTS = [3, 8, 9, 32, 16, 5]


def cross_check_batches(limit):
    """(short tracks alone, the same with a track of r - 1 appended, the same with a track of r appended) on the stereo window, stride 48: alone
    every gate matrix is resident; under r - 1 m_lds_max is below every short track (same instantiation, S in the global workspace); under r the
    records are global (the other instantiation) and the short tracks' S resident again"""
    g, r = edges(48, 208, limit)
    m_lds = carve(r - 1, 48, 208, limit)[0]
    assert m_lds < min(X_SHORTS) and carve(r, 48, 208, limit)[0] >= max(X_SHORTS) and max(X_SHORTS) < g
    base = _window(STEREO, len(X_SHORTS) + 1, 7)
    full = lambda m: ts.with_lengths(base, X_SHORTS + [m], patterns=("stride",))
    alone = ts.with_lengths(base, X_SHORTS + [0], patterns=("stride",)).subset(np.arange(len(X_SHORTS)))
    return alone, full(r - 1), full(r)


E_ANCHORED = dict(MONO, reps=[capi.REP_ANCHORED_3D] * 6)


def chain_links(limit):
    """group (e): [(kind, options, Problem, expected (stride, longest track))] — stride 48 at g - 1, stride 72 at r (anchored landmarks of a SLAM
    batch), stride 48 at g + 1, a 9-observation batch; all on the mono window, every link with a state of its own"""
    D48 = ts.n_columns(16, 1)
    g48, _ = edges(48, D48, limit)
    D72 = D48 + 18
    _, r72 = edges(72, D72, limit)
    gen = dict(chi2_multipler=1.0, gate_always_factor=1, no_fast_feature_kernel=1)
    links = []
    for kind, m in (("msckf", g48 - 1), ("slam", r72), ("msckf", g48 + 1), ("msckf", 9)):
        if kind == "msckf":
            _, prob, _ = msckf_mixed(MONO, m, A_SHORTS, len(A_SHORTS), True, 2) if m == 9 else msckf_mixed(MONO, m, [3, 9, 32, 0, 16], 5, True, 11)
            links.append((kind, gen, prob, (48, m)))
        else:
            _, prob, _ = slam_mixed(E_ANCHORED, m, 42)
            links.append((kind, gen, prob, (72, m)))
    return links


# --------------------------------------------------------------------------- the oracle
def oracle_run(oracle, case, limit=LIMITS[0]):
    """(injected triangulation or None, reference outputs) of a case at a limit, cached on the case"""
    cache = case.__dict__.setdefault("_ref", {})
    if limit not in cache:
        clean, prob, _ = case.batch(limit)
        opts, v = case.opts(), capi.Views(prob)
        if case.kind == "slam":
            tri, ref = None, oracle.slam_update(opts, v, feat_sigma=case.sigma, feat_chi2mult=case.mult)
            ref.update(oracle.apply_dx(opts, v, ref["dx"]))
        else:
            tri = oracle.triangulate(opts, capi.Views(clean))
            if case.kind == "msckf":
                ref = oracle.msckf_update(opts, v, want_compressed=False, given=tri)
            else:
                ref = oracle.slam_delayed_init(opts, v, feat_rep=case.rep, tri=tri)
                assert ref["rc"] == 0
        cache[limit] = (tri, ref)
    return cache[limit]


def accepted(case, ref):
    """per feature: gated and accepted"""
    if case.kind == "init":
        return ref["lm_cov_id"] >= 0
    return ref["feat_status"] == capi.FEAT_USED
