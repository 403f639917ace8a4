"""The cases that pin k_triangulate (csrc/k_triangulate.h) and the anchors of k_batch_layout at every rejection clause, loop exit, stride-loop
trip and seeded refusal (tests/test_tri_shapes_cpu.py shows on the oracle alone that every case reaches what it is named for and that nothing in
it sits within round-off of a threshold; tests/test_gpu_tri_edges.py runs them on the device).

Thresholds are moved by OPTIONS on stock scenes — B = synth.make_problem(2, F=120, track="ragged") —, never by building exotic geometry: every
accepted point stays in the depth range where the suite's TOL_TRI was measured.  A claim is (kind, name) -> the least number of features the
oracle's trace must show for it ("reject" / "exit": pyoracle.REJECT / EXIT; "status": capi.FEAT_*).  The counts the oracle gave when the cases were
written are quoted next to each claim; the claim itself is about half of that, so that a change of synth moves a case before it empties it.

A helper module, not a conftest: nothing here is collected.
"""
from __future__ import annotations

import copy
import functools
from dataclasses import dataclass, field

import numpy as np

import track_shapes as ts
from open_vins_amd import capi, synth

THRESHOLD_FLOOR = 1e-6   # no tested quantity within this (relative) of a threshold in force: five orders above the measured GPU-to-oracle differences
DECISION_FLOOR = 1e-10   # no LM decision margin below this: summation-order noise is ~ m 2^-53 ~ 1e-14
MODES = {"full": {}, "1d": dict(triangulate_1d=1), "lin": dict(refine_features=0), "1d-lin": dict(triangulate_1d=1, refine_features=0)}
USED, TOO_FEW, TRI_FAILED, GN_FAILED = capi.FEAT_USED, capi.FEAT_TOO_FEW_MEAS, capi.FEAT_TRI_FAILED, capi.FEAT_GN_FAILED


@functools.lru_cache(maxsize=None)
def base():
    """B: 30 clones, stereo, 120 features of 5 .. 60 observations."""
    return synth.make_problem(2, F=120, track="ragged")


@functools.lru_cache(maxsize=None)
def quad():
    """Four cameras, 30 clones, 40 features of 120 observations: the stock for the re-cut tracks."""
    return synth.make_problem(4, F=40)


@dataclass
class Case:
    id: str
    prob_fn: object              # () -> Problem, built on first use
    options: dict                # capi.default_options(**options)
    claims: dict = field(default_factory=dict)   # (kind, name) -> least count
    group: str = ""
    named: tuple = ()            # features the case is named for (never dropped; the tests look at them one by one)

    @property
    def prob(self):
        return self.prob_fn()

    def opts(self):
        return capi.default_options(**self.options)


# --------------------------------------------------------------------------- thresholds and loop exits on B, in the four modes
# (option, {mode: claims}); counts in the comments: what the oracle gave on B when this was written
_R, _E, _S = "reject", "exit", "status"
B_CASES = [
    ("default", {}, {
        "full": {(_E, "dcost"): 100, (_S, USED): 60},
        "1d": {(_S, USED): 60}, "lin": {(_S, USED): 60}, "1d-lin": {(_S, USED): 60}}),
    ("max_dist-5", dict(max_dist=5.0), {       # full: lin-hi 44, gn-hi 65, baseline 1 (the first clause that holds is the one counted), accepted 10
        "full": {(_R, "lin_hi"): 22, (_R, "gn_hi"): 32, (_R, "baseline"): 1, (_S, USED): 5},
        "1d": {(_S, USED): 5, (_S, TRI_FAILED): 15, (_S, GN_FAILED): 40},      # {0: 10, 2: 31, 3: 79}
        "lin": {(_R, "lin_hi"): 22, (_S, USED): 30},
        "1d-lin": {(_R, "lin_hi"): 15, (_S, USED): 30}}),
    ("min_dist-5.5", dict(min_dist=5.5), {     # full: lin-lo 105, accepted 15
        "full": {(_R, "lin_lo"): 52, (_S, USED): 7},
        "1d": {(_R, "lin_lo"): 52, (_S, USED): 7},                               # {2: 105, 0: 14, 3: 1}
        "lin": {(_R, "lin_lo"): 52, (_S, USED): 7},
        "1d-lin": {(_R, "lin_lo"): 52, (_S, USED): 7}}),
    ("max_cond-2000", dict(max_cond_number=2000.0), {   # cond 27
        "full": {(_R, "cond"): 13, (_S, USED): 40}, "lin": {(_R, "cond"): 13, (_S, USED): 40},
        "1d": {(_S, USED): 40}, "1d-lin": {(_S, USED): 40}}),           # (the 1-D routine has no condition number: the option must change nothing)
    ("max_baseline-15", dict(max_baseline=15.0), {      # baseline 45
        "full": {(_R, "baseline"): 22, (_S, USED): 30}, "1d": {(_R, "baseline"): 22, (_S, USED): 30},
        "lin": {(_S, USED): 60}, "1d-lin": {(_S, USED): 60}}),
    ("max_runs-1", dict(max_runs=1), {                  # every loop leaves by runs: 120
        "full": {(_E, "runs"): 60}, "1d": {(_E, "runs"): 60}, "lin": {(_S, USED): 60}, "1d-lin": {(_S, USED): 60}}),
    ("max_lamda-10", dict(max_lamda=10.0), {            # lam exit after rejected steps: 24
        "full": {(_E, "lam"): 12}, "1d": {(_E, "lam"): 8}, "lin": {(_S, USED): 60}, "1d-lin": {(_S, USED): 60}}),
    ("max_lamda-init", dict(max_lamda=1e-3), {          # = init_lamda: the body is never entered, 120, all accepted
        "full": {(_E, "not_entered"): 100}, "1d": {(_E, "not_entered"): 100}, "lin": {(_S, USED): 60}, "1d-lin": {(_S, USED): 60}}),
    ("min_dx-1e-2", dict(min_dx=1e-2), {                # dx exit: 92
        "full": {(_E, "dx"): 46}, "1d": {(_E, "dx"): 30}, "lin": {(_S, USED): 60}, "1d-lin": {(_S, USED): 60}}),
    ("min_dcost-1e-2", dict(min_dcost=1e-2), {          # dcost on the first accepted step
        "full": {(_E, "dcost"): 100}, "1d": {(_E, "dcost"): 100}, "lin": {(_S, USED): 60}, "1d-lin": {(_S, USED): 60}}),
]


# --------------------------------------------------------------------------- re-cut tracks
def _spread(mf, m):
    """m observations of a track of mf, ascending (every camera's observations stay contiguous): spread over the whole track, repeats where
    m > mf."""
    if m <= mf:
        return np.unique(np.round(np.linspace(0, mf - 1, m)).astype(np.int64)) if m > 1 else np.arange(m, dtype=np.int64)
    return np.sort(np.resize(np.arange(mf, dtype=np.int64), m))


LENGTHS = [0, 1, 2, 3, 4, 63, 64, 65, 66, 127, 128, 129, 130, 191, 192, 193, 200, 254]


@functools.lru_cache(maxsize=None)
def lengths_problem():
    """Tracks of LENGTHS observations cut from quad()'s 120-observation tracks; empty tracks first, last and between the others."""
    q = quad()
    want = [0]
    for i, m in enumerate(LENGTHS[1:]):
        want.append(m)
        if i % 4 == 3:
            want.append(0)
    want.append(0)
    picks = []
    for f, m in enumerate(want):
        mf = int(q.meas_offsets[f + 1] - q.meas_offsets[f])
        pk = _spread(mf, m)
        assert pk.size == m
        picks.append(pk)
    p = ts.keep_tracks(q.subset(np.arange(len(want))), picks)
    assert np.diff(p.meas_offsets).tolist() == want
    return p


RUNS = [(3, 3), (3, 4), (2, 5, 5, 1), (1, 1), (60, 70), (70, 60), (64, 64), (63, 65), (129,), (10, 64, 10, 46)]


def camera_runs(prob, f):
    """[(camera, first, length)] of feature f's runs of equal camera ids, positions inside the track."""
    a, b = int(prob.meas_offsets[f]), int(prob.meas_offsets[f + 1])
    cam = prob.cam_idx[a:b]
    out, i = [], 0
    while i < b - a:
        j = i
        while j < b - a and cam[j] == cam[i]:
            j += 1
        out.append((int(cam[i]), i, j - i))
        i = j
    return out


def rule_anchor(prob, f):
    """FeatureInitializer.cpp:36-46 restated: the last measurement of the first run with strictly the most measurements (flat index; -1: empty)."""
    best, end = 0, -1
    for _, first, n in camera_runs(prob, f):
        if n > best:
            best, end = n, first + n - 1
    return int(prob.meas_offsets[f]) + end if end >= 0 else -1


@functools.lru_cache(maxsize=None)
def runs_problem():
    """Feature f has camera runs of RUNS[f] observations: run j from the j-th camera group of quad()'s track f, spread over the group's clones."""
    q = quad().subset(np.arange(len(RUNS)))
    picks = []
    for f, runs in enumerate(RUNS):
        groups = camera_runs(q, f)
        assert len(groups) >= len(runs)
        pk = [first + _spread_group(n, want) for (_, first, n), want in zip(groups, runs)]
        picks.append(np.concatenate(pk))
    p = ts.keep_tracks(q, picks)
    for f, runs in enumerate(RUNS):
        assert tuple(n for _, _, n in camera_runs(p, f)) == runs
    return p


def _spread_group(n, want):
    pk = _spread(n, want)
    if pk.size < want:  # (np.unique dropped a repeat of the rounding: top up from the front, sorted)
        pk = np.sort(np.concatenate([pk, np.setdiff1d(np.arange(n), pk)[: want - pk.size]]))
    assert pk.size == want
    return pk


# --------------------------------------------------------------------------- degenerate inputs among healthy neighbours
ONE_POSE_F, NAN_F = 3, 6


@functools.lru_cache(maxsize=None)
def degenerate_problem():
    """quad()'s first ten tracks; feature ONE_POSE_F observes one (camera, clone) pose five times, feature NAN_F (120 observations) has one NaN
    normalised coordinate — not at its anchor, at the third trip's reach of neither loop: observation 70."""
    q = quad().subset(np.arange(10))
    picks = [np.arange(int(q.meas_offsets[f + 1] - q.meas_offsets[f])) for f in range(q.F)]
    picks[ONE_POSE_F] = np.full(5, 7, dtype=np.int64)
    p = ts.keep_tracks(q, picks)
    uvn = p.uvn.reshape(-1, 2).copy()
    uvn[int(p.meas_offsets[NAN_F]) + 70, 1] = np.float32("nan")
    p.uvn = np.ascontiguousarray(uvn.reshape(-1))
    return p


# --------------------------------------------------------------------------- the catalogue of ovgpu_triangulate cases
def _b_cases():
    out = []
    for name, options, per_mode in B_CASES:
        for mode, extra in MODES.items():
            out.append(Case(f"B-{name}-{mode}", base, {**options, **extra}, per_mode[mode], group="B"))
    return out


def _shape_cases():
    out = []
    for mode, extra in MODES.items():
        out.append(Case(f"lengths-{mode}", lengths_problem, dict(extra), {(_S, TOO_FEW): 6, (_S, USED): 14}, group="lengths"))
        out.append(Case(f"runs-{mode}", runs_problem, dict(extra), {(_S, USED): 6}, group="runs"))
    for mode, extra in MODES.items():
        if mode != "1d-lin":
            out.append(Case(f"degenerate-{mode}", degenerate_problem, dict(extra), {(_S, TRI_FAILED): 2, (_S, USED): 6}, group="degenerate",
                            named=(ONE_POSE_F, NAN_F)))
    return out


CASES = _b_cases() + _shape_cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


MAX_DROP = 0.02   # a case may leave out this share of its features, none of them one it is named for


def _frozen(d):
    for v in d.values():
        v.setflags(write=False)
    return d


def thin(opts, tr):
    """The features of a traced run that miss one of the two floors."""
    return np.flatnonzero((threshold_margins(opts, tr) < THRESHOLD_FLOOR) | (tr["min_margin"] < DECISION_FLOOR))


@functools.lru_cache(maxsize=None)
def dropped(oracle, cid):
    """The features a case leaves out when it is constructed: those whose oracle run sits within a floor of a threshold or of an LM decision
    (features are independent: leaving one out changes nothing about the others)."""
    case = BY_ID[cid]
    out = thin(case.opts(), oracle.triangulate_trace(case.opts(), capi.Views(case.prob)))
    assert len(out) <= int(MAX_DROP * case.prob.F) and not set(out.tolist()) & set(case.named), (cid, out)
    return tuple(out.tolist())


@functools.lru_cache(maxsize=None)
def problem(oracle, cid):
    """The case's batch as it runs: its stock problem less dropped()."""
    case, out = BY_ID[cid], dropped(oracle, cid)
    return case.prob.subset(np.setdiff1d(np.arange(case.prob.F), out)) if out else case.prob


@functools.lru_cache(maxsize=None)
def oracle_trace(oracle, cid):
    """The oracle's traced triangulation of a case: computed once, shared, never written to."""
    return _frozen(oracle.triangulate_trace(BY_ID[cid].opts(), capi.Views(problem(oracle, cid))))


def count(tr, kind, name, oracle):
    if kind == "status":
        return int((tr["status"] == name).sum())
    code = (oracle.REJECT if kind == "reject" else oracle.EXIT)[name]
    entered = np.isfinite(tr["lam_final"]) if kind == "exit" else np.ones(len(tr["status"]), bool)  # (an exit only of a refinement that ran)
    return int(((tr[kind] == code) & entered).sum())


def threshold_margins(opts, tr):
    """Per feature, the smallest relative distance of a quantity it tested to the threshold it was tested against (inf: tested nothing finite)."""
    F = len(tr["status"])
    out = np.full(F, np.inf)

    def near(q, t):
        ok = np.isfinite(q)
        d = np.full(F, np.inf)
        d[ok] = np.abs(q[ok] - t) / abs(t)
        return d
    for q, t in ((np.abs(tr["condA"]), opts.max_cond_number), (tr["lin_depth"], opts.min_dist), (tr["lin_depth"], opts.max_dist),
                 (tr["gn_depth"], opts.min_dist), (tr["gn_depth"], opts.max_dist), (tr["base_ratio"], opts.max_baseline)):
        out = np.minimum(out, near(q, t))
    return np.minimum(out, tr["min_dx_margin"])


# --------------------------------------------------------------------------- the seeded path (ovgpu_refine)
@functools.lru_cache(maxsize=None)
def linear_seed(oracle):
    """The oracle's linear result on B under default options: seeds (anchor frame), anchors, statuses, global positions."""
    return _frozen(oracle.triangulate(capi.default_options(refine_features=0), capi.Views(base())))


def camera_poses(prob):
    """R_GtoC [K * C, 3, 3] and p_CinG [K * C, 3] of every (camera, clone) pair, pair (k, c) at k * C + c (UpdaterMSCKF.cpp:106-107)."""
    R, p = np.zeros((prob.K * prob.C, 3, 3)), np.zeros((prob.K * prob.C, 3))
    for k in range(prob.K):
        R_ItoC, p_IinC = synth.quat_2_rot(prob.calib_q_p[k, :4]), prob.calib_q_p[k, 4:]
        for c in range(prob.C):
            R[k * prob.C + c] = R_ItoC @ synth.quat_2_rot(prob.clone_q_p[c, :4])
            p[k * prob.C + c] = prob.clone_q_p[c, 4:] - R[k * prob.C + c].T @ p_IinC
    return R, p


@dataclass
class SeedCase:
    id: str
    options: dict
    seed_fn: object              # (oracle) -> (p_FinA [F, 3], anchor_meas [F])
    claims: dict = field(default_factory=dict)
    refused: tuple = ()          # features whose seed anchor lies outside their track
    nan_seed: tuple = ()

    def opts(self):
        return capi.default_options(**self.options)


def _seed_rule(oracle):
    lin = linear_seed(oracle)
    return lin["p_FinA"].copy(), lin["anchor_meas"].copy()


BAD_ANCHOR_F = (10, 57, 119)   # seed anchors -1, m0 - 1 and m1
NAN_SEED_F = 30


def _seed_bad_anchors(oracle):
    pA, an = _seed_rule(oracle)
    off = base().meas_offsets
    # features whose linear seed is healthy, so that the refusal is the anchor's doing
    assert np.isfinite(pA[list(BAD_ANCHOR_F)]).all()
    an[BAD_ANCHOR_F[0]] = -1
    an[BAD_ANCHOR_F[1]] = off[BAD_ANCHOR_F[1]] - 1
    an[BAD_ANCHOR_F[2]] = off[BAD_ANCHOR_F[2] + 1]
    return pA, an


def _seed_nan(oracle):
    pA, an = _seed_rule(oracle)
    assert np.isfinite(pA[NAN_SEED_F]).all()
    pA[NAN_SEED_F, 1] = np.nan
    return pA, an


FIRST_MEAS_EVERY = 8


def _seed_first_measurement(oracle):
    """Every eighth feature anchored on its track's FIRST measurement instead of the rule's: the linear point, moved into that camera's frame."""
    lin, B = linear_seed(oracle), base()
    R, p = camera_poses(B)
    pA, an = lin["p_FinA"].copy(), lin["anchor_meas"].copy()
    f = np.arange(0, B.F, FIRST_MEAS_EVERY)
    an[f] = B.meas_offsets[:-1][f]
    cc = B.cam_idx[an[f]] * B.C + B.clone_idx[an[f]]
    pA[f] = np.einsum("fij,fj->fi", R[cc], lin["p_FinG"][f] - p[cc])
    return pA, an


SEED_CASES = [
    SeedCase("seed-default", {}, _seed_rule, {(_S, USED): 60}),
    SeedCase("seed-min_dist-5.5", dict(min_dist=5.5), _seed_rule, {(_R, "gn_lo"): 40, (_S, USED): 7}),   # gn-lo: reached by nothing else
    SeedCase("seed-max_dist-5", dict(max_dist=5.0), _seed_rule, {(_R, "gn_hi"): 40, (_S, USED): 5}),     # gn-hi from seeds the linear check would have refused
    SeedCase("seed-bad-anchors", {}, _seed_bad_anchors, {(_S, TRI_FAILED): 3, (_S, USED): 60}, refused=BAD_ANCHOR_F),
    SeedCase("seed-first-measurement", {}, _seed_first_measurement, {(_S, USED): 50}),
    SeedCase("seed-nan", {}, _seed_nan, {(_R, "gn_nan"): 1, (_S, USED): 60}, nan_seed=(NAN_SEED_F,)),
]
SEED_BY_ID = {c.id: c for c in SEED_CASES}


@functools.lru_cache(maxsize=None)
def seed_setup(oracle, cid):
    """(problem, seeds, seed anchors, where the case's named features went) of a seeded case: B and the case's seeds less the features that miss a
    floor (at most MAX_DROP of them, none refused or NaN-seeded on purpose); anchors move with their tracks, -1 stays -1."""
    case, B = SEED_BY_ID[cid], base()
    pA, an = case.seed_fn(oracle)
    out = thin(case.opts(), oracle.refine(case.opts(), capi.Views(B), pA, an))
    named = set(case.refused) | set(case.nan_seed)
    assert len(out) <= int(MAX_DROP * B.F) and not set(out.tolist()) & named, (cid, out)
    keep = np.setdiff1d(np.arange(B.F), out)
    prob = B.subset(keep) if len(out) else B
    rel = an[keep] - B.meas_offsets[:-1][keep]
    an2 = np.where(an[keep] == -1, -1, prob.meas_offsets[:-1] + rel).astype(np.int32)
    where = {int(f): int(np.flatnonzero(keep == f)[0]) for f in named}
    pA2 = np.ascontiguousarray(pA[keep])
    pA2.setflags(write=False), an2.setflags(write=False)
    return prob, pA2, an2, where


@functools.lru_cache(maxsize=None)
def oracle_refine(oracle, cid):
    prob, pA, an, _ = seed_setup(oracle, cid)
    return _frozen(oracle.refine(SEED_BY_ID[cid].opts(), capi.Views(prob), pA, an))


# --------------------------------------------------------------------------- the pose table at the LDS limit
LDS_LIMIT = 160 * 1024        # bytes of LDS a workgroup may ask for on gfx950
POSE_BYTES = 96               # 12 doubles per (camera, clone) pair
LDS_C, LDS_SHIFT = 853, 823   # B's 30 clones at 823 .. 852 of an 853-clone table: 2 * 853 * 96 = 163 776 of 163 840 bytes


def embedded_pose_table(C, K, shift=LDS_SHIFT):
    """A C x K pose table with B's clones at shift .. shift + 29 (cameras 0 and 1) and valid poses — identity, origin — everywhere else."""
    B = base()
    Rb, pb = camera_poses(B)
    R = np.tile(np.eye(3).reshape(1, 9), (K * C, 1))
    p = np.zeros((K * C, 3))
    for k in range(B.K):
        R[k * C + shift: k * C + shift + B.C] = Rb[k * B.C:(k + 1) * B.C].reshape(-1, 9)
        p[k * C + shift: k * C + shift + B.C] = pb[k * B.C:(k + 1) * B.C]
    return np.ascontiguousarray(R), np.ascontiguousarray(p)


@functools.lru_cache(maxsize=None)
def shifted_base(shift=LDS_SHIFT):
    q = copy.copy(base())
    q.clone_idx = np.ascontiguousarray(base().clone_idx + shift, dtype=np.int32)
    return q
