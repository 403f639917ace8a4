"""The catalogue of SLAM batches that pin the fused per-feature kernel of UpdaterSLAM::update (csrc/k_slam_y.h, ovgpu_debug_option "slam_fused")
at its representation, track-length, column and dispatch edges: tests/test_slam_shapes_cpu.py checks every batch on the oracle alone,
tests/test_gpu_slam_fused.py runs it on the device.

expected_kernel() restates the eligibility rule FROM ITS DOCUMENTED TERMS (include/ovgpu.h: "slam_fused"), not from the library: the tests
compare what the library reports with it.  Snapshots come from synth.make_slam_problem; tracks are cut with track_shapes' helpers.

A helper module, not a conftest: nothing here is collected.
"""
from __future__ import annotations

import copy
import functools
from dataclasses import dataclass, field

import numpy as np

import track_shapes as ts
from open_vins_amd import capi, synth
from parity_util import GATE_MARGIN

BOUND = 62        # slamy::SLY_MMAX: 2 m + 4 rows of the augmented gate matrix in 8 tile rows
GRAM_MAX_D = 383  # the whitened (Gram) route holds 24 tile columns of [H | r]
SINGLE = capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE
REPS5 = [capi.REP_GLOBAL_3D, capi.REP_GLOBAL_FULL_INVERSE_DEPTH, capi.REP_ANCHORED_3D, capi.REP_ANCHORED_FULL_INVERSE_DEPTH,
         capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH]


def expected_kernel(reps, m_max, D, K, C, switch=1, general=0, gram_route=True):
    """ovgpu_debug_option "last_feature_kernel" after a SLAM update of a batch that observes landmarks of the representations `reps`, longest
    track m_max, D Jacobian columns: 4 (k_slam_y) when the switch is on, no_fast_feature_kernel off, every landmark 3-dof, the track within the
    bound, 16 <= D, K C <= 8192 and the update takes the whitened route (D <= 383, compress_route not TSQR, the prior's factor exists)."""
    ok = switch and not general and all(int(r) != SINGLE for r in reps) and m_max <= BOUND and D >= 16 and K * C <= 8192
    return 4 if (ok and gram_route and D <= GRAM_MAX_D) else 0


def n_columns(C, K, L_dof, pose=1, intr=1):
    return ts.n_columns(C, K, pose, intr) + L_dof


# --------------------------------------------------------------------------- snapshots
def slam(L, reps, seed, C=30, K=2, pose=1, intr=1, **kw):
    reps = np.full(L, reps, np.int32) if np.isscalar(reps) else np.asarray(reps, np.int32)
    if not (pose and intr):
        kw.setdefault("calib_noise", 0.0)  # a calibration error the filter does not model would reject every long track
    p = synth.make_slam_problem(2, L=L, lm_rep=reps, seed=seed, C=C, K=K, **kw)
    p.lm_index = np.arange(L, dtype=np.int32)
    return p


def reordered(p, order):
    q = p.subset(order)
    q.lm_index = np.ascontiguousarray(np.asarray(p.lm_index)[order], dtype=np.int32)
    return q


def without_anchor_clone(p):
    """Every anchored landmark's track without the observations of its anchor clone: the anchor block stands alone in its rows."""
    picks = []
    for f in range(p.F):
        cl = p.clone_idx[int(p.meas_offsets[f]):int(p.meas_offsets[f + 1])]
        keep = np.arange(cl.size)
        if p.lm_anchor_clone is not None and p.lm_anchor_clone[p.lm_index[f]] >= 0:
            keep = np.flatnonzero(cl != p.lm_anchor_clone[p.lm_index[f]])
        picks.append(keep)
    return ts.keep_tracks(p, picks)


def anchor_is_observed(p):
    """per anchored feature: its anchor clone is one of the clones it measures"""
    out = []
    for f in range(p.F):
        l = p.lm_index[f]
        if p.lm_anchor_clone is not None and p.lm_anchor_clone[l] >= 0:
            out.append(bool((p.clone_idx[int(p.meas_offsets[f]):int(p.meas_offsets[f + 1])] == p.lm_anchor_clone[l]).any()))
    return out


LEN_REPS = [capi.REP_GLOBAL_3D, capi.REP_ANCHORED_3D, capi.REP_GLOBAL_FULL_INVERSE_DEPTH, capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH,
            capi.REP_ANCHORED_FULL_INVERSE_DEPTH, capi.REP_GLOBAL_3D]


def length_batch(m_long, long_first, seed):
    """Six landmarks: a track of exactly m_long observations, an EMPTY track, four shorter ones (the 12-observation one a gross outlier from
    m_long >= 12 on), the long one first or last.  Beyond 57 observations the rig is 30 clones x 4 cameras."""
    K = 4 if m_long > 57 else 2
    p = slam(6, LEN_REPS, seed, K=K)
    p = ts.with_lengths(p, [m_long, min(5, m_long), 0, min(12, m_long), min(9, m_long), min(3, m_long)], patterns=("prefix",))
    if m_long >= 12:
        p = ts.make_outlier(p, 3, 15.0, seed)
    return p if long_first else reordered(p, [1, 2, 3, 4, 5, 0])


COLUMN_STATES = {  # D = 6 C + K (6 pose + 8 intr) + 3 L
    63: dict(C=10, K=1, L=1, pose=0, intr=0),
    64: dict(C=5, K=2, L=2),
    128: dict(C=18, K=1, L=2),
    129: dict(C=21, K=1, L=1, pose=0, intr=0),
    # a limit of the synthetic rig (synth has four cameras): with K <= 4, C <= 30 and L <= 12, 6 C + 14 K + 3 L = 256 has no solution (five
    # cameras, 30 clones and 2 landmarks would give it), so the two sides of the two-panel factorisation's threshold are 255 and 257
    255: dict(C=30, K=3, L=11),
    257: dict(C=30, K=4, L=7),
    # the Gram route's last column count and the first Householder one: 60 clones (the rig's four cameras, 30 clones and 12 landmarks end at 272 columns)
    383: dict(C=60, K=1, L=3),
    384: dict(C=60, K=1, L=8, pose=0, intr=0),
}


def column_batch(D, seed):
    st = COLUMN_STATES[D]
    reps = (REPS5 * 3)[:st["L"]]
    p = slam(st["L"], reps, seed, C=st["C"], K=st["K"], pose=st.get("pose", 1), intr=st.get("intr", 1))
    # (three and four cameras see a point up to 120 times: every track within the kernel's bound, every camera kept, the anchor — the first observation — too)
    return ts.with_lengths(p, [min(int(m), 40) for m in np.diff(p.meas_offsets)], patterns=("stride",))


def semi_definite(p):
    """the two newest clones perfectly correlated (tests/test_gpu_parity.py::test_semi_definite_prior_takes_the_householder_route)"""
    q = copy.copy(p)
    A = np.eye(p.N)
    i, j = int(p.clone_cov_id[p.C - 2]), int(p.clone_cov_id[p.C - 1])
    A[j:j + 6, :] = 0.0
    A[j:j + 6, i:i + 6] = np.eye(6)
    P = A @ p.P @ A.T
    q.P = np.ascontiguousarray(0.5 * (P + P.T))
    return q


@dataclass
class Case:
    id: str
    group: str
    build: object                                  # () -> Problem (lm_index set)
    options: dict = field(default_factory=dict)    # capi.default_options keywords on top of chi2_multipler = 1
    sigma: object = None                           # per-feature sigma_pix / chi2_multipler, or None
    mult: object = None
    outliers: bool = False
    m_max: int | None = None                       # the longest track the case is named for (None: whatever the batch holds)
    D: int | None = None                           # the column count the case is named for
    gram_route: bool = True                        # False: the update is known to leave the whitened route (TSQR, a semi-definite prior)
    entry: str = "update"                          # "update" | "compress"

    @functools.cached_property
    def prob(self):
        return self.build()

    def opts(self, **more):
        kw = dict(chi2_multipler=1.0)
        kw.update(self.options)
        kw.update(more)
        return capi.default_options(**kw)

    @property
    def columns(self):
        p = self.prob
        reps = np.asarray(p.lm_rep_each if getattr(p, "lm_rep_each", None) is not None else np.full(len(p.lm_value), p.lm_rep))
        return n_columns(p.C, p.K, int(np.where(reps == SINGLE, 1, 3).sum()), self.options.get("do_calib_camera_pose", 1), self.options.get("do_calib_camera_intrinsics", 1))

    @property
    def longest_track(self):
        return int(np.diff(self.prob.meas_offsets).max())

    @property
    def kernel(self):
        p = self.prob
        reps = np.asarray(p.lm_rep_each if getattr(p, "lm_rep_each", None) is not None else np.full(len(p.lm_value), p.lm_rep))[p.lm_index]
        return expected_kernel(reps, self.longest_track, self.columns, p.K, p.C, 1, self.options.get("no_fast_feature_kernel", 0),
                               self.gram_route and self.entry == "update" and self.options.get("compress_route", capi.COMPRESS_GRAM) != capi.COMPRESS_TSQR)


# seeds: chosen on the CPU (tests/test_slam_shapes_cpu.py holds every case to it) so that the oracle accepts a feature, rejects one where an
# outlier is planted and leaves no statistic within parity_util.GATE_MARGIN of its threshold
MIX10 = (REPS5 * 2)
NOISE_SIGMA = np.linspace(0.7, 2.5, 10)
NOISE_F = 4  # the feature whose multiplier ALONE decides its gate: accepted at its sigma with the multiplier 1, rejected with NOISE_MULT[NOISE_F]
NOISE_MULT = np.array([1.0, 0.8, 3.0, 1.5, 0.02, 2.0, 1.0, 0.6, 4.0, 1.2])
TRACKS = [1, 2, 7, 8, 9, 31, 32, 33, BOUND - 1, BOUND, BOUND + 1]
FIRST_5 = [0, 9, 9, 22, 38, 50]


def nofc(pose, intr):
    return dict(do_calib_camera_pose=pose, do_calib_camera_intrinsics=intr)


def _cases():
    out = []
    for r in REPS5:
        out.append(Case(f"rep-{r}", "rep", functools.partial(slam, 6, r, 40 + r)))
    out.append(Case("rep-mix", "rep", functools.partial(slam, 10, MIX10, 3)))
    out.append(Case("rep-mix-outliers", "rep", functools.partial(slam, 10, MIX10, 7, outlier_frac=0.3), outliers=True))
    out.append(Case("rep-anchor-clone-unobserved", "rep", lambda: without_anchor_clone(slam(9, (REPS5[2:] * 3), 5))))
    # a single-depth landmark RESIDENT (it has its column) but not observed by the batch: the rule is about the landmarks the batch observes
    out.append(Case("rep-single-depth-resident-unobserved", "rep", lambda: reordered(slam(8, [0, 2, 4, SINGLE, 1, 3, 0, 2], 13), [0, 1, 2, 4, 5, 6, 7])))
    out.append(Case("rep-fisheye", "rep", functools.partial(slam, 10, MIX10, 9, fisheye=True)))
    out.append(Case("rep-mix-nofej", "rep", functools.partial(slam, 10, MIX10, 3), options=dict(do_fej=0)))
    for m in TRACKS:
        out.append(Case(f"len-{m}", "len", functools.partial(length_batch, m, True, 11), outliers=m >= 12, m_max=m))
    for m in (9, BOUND, BOUND + 1):
        out.append(Case(f"len-{m}-last", "len", functools.partial(length_batch, m, False, 11), outliers=m >= 12, m_max=m))
    for D, st in COLUMN_STATES.items():
        out.append(Case(f"col-{D}", "col", functools.partial(column_batch, D, 21), options=nofc(st.get("pose", 1), st.get("intr", 1)), D=D))
    out.append(Case("noise", "noise", functools.partial(slam, 10, MIX10, 3), sigma=NOISE_SIGMA, mult=NOISE_MULT))
    # fall-backs: kernel 0, the switch-off context's bits
    out.append(Case("fb-single-depth", "fb", functools.partial(slam, 8, [0, 2, 4, SINGLE, 1, 3, 0, 2], 13)))
    out.append(Case("fb-general", "fb", functools.partial(slam, 8, (REPS5 * 2)[:8], 13), options=dict(no_fast_feature_kernel=1)))
    out.append(Case("fb-tsqr", "fb", functools.partial(slam, 8, (REPS5 * 2)[:8], 13), options=dict(compress_route=capi.COMPRESS_TSQR)))
    out.append(Case("fb-mode-a", "fb", functools.partial(slam, 8, (REPS5 * 2)[:8], 13), entry="compress"))
    out.append(Case("fb-semi-definite", "fb", lambda: semi_definite(slam(8, (REPS5 * 2)[:8], 13)), gram_route=False))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def chunk_problem():
    """L = 50, the six representations in turn (tests/test_gpu_slam_chunked.py's state): chunks of FIRST_5 hold single-depth landmarks"""
    reps6 = [capi.REP_GLOBAL_3D, capi.REP_ANCHORED_3D, capi.REP_GLOBAL_3D, capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, capi.REP_GLOBAL_FULL_INVERSE_DEPTH, SINGLE]
    return slam(50, (reps6 * 9)[:50], 3)


def chunk_problem_3dof():
    """L = 50 of the five 3-dof representations: every chunk is eligible"""
    return slam(50, (REPS5 * 10), 3)


def oracle_run(oracle, case):
    """the oracle's slam_update of a case, cached on it; also the number of features within GATE_MARGIN of their gate"""
    if not hasattr(case, "_ref"):
        ref = oracle.slam_update(case.opts(), capi.Views(case.prob), feat_sigma=case.sigma, feat_chi2mult=case.mult)
        g = np.isfinite(ref["chi2"]) & (ref["chi2_thresh"] > 0)
        ref["near_gate"] = int((np.abs(ref["chi2"][g] / ref["chi2_thresh"][g] - 1.0) < GATE_MARGIN).sum())
        case._ref = ref
    return case._ref
