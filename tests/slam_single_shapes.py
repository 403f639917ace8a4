"""The catalogue of SLAM batches that pin k_slam_y<true> — the fused per-feature kernel of UpdaterSLAM::update with the projection of
single-depth landmarks (csrc/k_slam_y.h, ovgpu_debug_option "slam_fused" = 2) — at its representation, track-length, column and dispatch edges:
tests/test_slam_single_shapes_cpu.py checks every batch on the oracle alone, tests/test_gpu_slam_single.py runs it on the device.

expected_kernel2() restates the level-2 rule FROM ITS DOCUMENTED TERMS (include/ovgpu.h: "slam_fused"), not from the library.  The builders are
slam_shapes' and track_shapes'.

A helper module, not a conftest: nothing here is collected.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import slam_shapes as ss
import track_shapes as ts
from open_vins_amd import capi

SINGLE, BOUND, GRAM_MAX_D = ss.SINGLE, ss.BOUND, ss.GRAM_MAX_D
G3, GI, A3, AI, AM = ss.REPS5  # GLOBAL_3D, GLOBAL_FULL_INVERSE_DEPTH, ANCHORED_3D, ANCHORED_FULL_INVERSE_DEPTH, ANCHORED_MSCKF_INVERSE_DEPTH


def expected_kernel2(reps, m_max, D, K, C, level=2, general=0, gram_route=True):
    """ovgpu_debug_option "last_feature_kernel" after a SLAM update of a batch that observes landmarks of the representations `reps`, longest
    track m_max, D Jacobian columns, with "slam_fused" at `level`: 0 unless the level is 1 or 2, no_fast_feature_kernel is off, the track is
    within the bound, 16 <= D, K C <= 8192 and the update takes the whitened route (D <= 383, compress_route not TSQR, not mode A).  Then 4
    (k_slam_y<false>) for a batch that observes no single-depth landmark; one that does takes 5 (k_slam_y<true>) at level 2 and 0 at level 1."""
    single = any(int(r) == SINGLE for r in reps)
    ok = level >= 1 and not general and m_max <= BOUND and D >= 16 and K * C <= 8192 and gram_route and D <= GRAM_MAX_D
    if not ok or (single and level < 2):
        return 0
    return 5 if single else 4


@dataclass
class Case(ss.Case):
    named: int | None = None      # the feature the case is named for (a single-depth one): its track is m_max observations long
    col: int | None = None        # the Jacobian column the case is named for: the named feature's landmark has it
    rejected: int | None = None   # the single-depth feature the gate must reject (an outlier, a multiplier)

    @property
    def reps_observed(self):
        p = self.prob
        reps = np.asarray(p.lm_rep_each if getattr(p, "lm_rep_each", None) is not None else np.full(len(p.lm_value), p.lm_rep))
        return reps[p.lm_index]

    def kernel_at(self, level):
        p = self.prob
        gram = self.gram_route and self.entry == "update" and self.options.get("compress_route", capi.COMPRESS_GRAM) != capi.COMPRESS_TSQR
        return expected_kernel2(self.reps_observed, self.longest_track, self.columns, p.K, p.C, level, self.options.get("no_fast_feature_kernel", 0), gram)

    @property
    def kernel2(self):
        return self.kernel_at(2)

    def column_of(self, f):
        """first Jacobian column of feature f's landmark: the calibration and clone columns, then the landmarks by covariance id"""
        p = self.prob
        reps = np.asarray(p.lm_rep_each if getattr(p, "lm_rep_each", None) is not None else np.full(len(p.lm_value), p.lm_rep))
        dof = np.where(reps == SINGLE, 1, 3)
        order = np.argsort(p.lm_cov_id, kind="stable")
        before = {int(l): int(dof[order[:k]].sum()) for k, l in enumerate(order)}
        base = ts.n_columns(p.C, p.K, self.options.get("do_calib_camera_pose", 1), self.options.get("do_calib_camera_intrinsics", 1))
        return base + before[int(p.lm_index[f])]


# --------------------------------------------------------------------------- builders
MIX8 = [G3, A3, AM, SINGLE, GI, AI, G3, A3]       # slam_shapes' "fb-single-depth": 8 landmarks, one single
MIX_ANCHOR = [SINGLE, A3, SINGLE, AM, G3, SINGLE, AI, SINGLE]
LEN_REPS = [SINGLE, A3, GI, SINGLE, AI, G3]       # the long track and the 12-observation one (the outlier) are single-depth
LEN_OUTLIER = 3
TRACKS = [1, 2, 3, 6, 7, 8, 9, 31, 32, 33, BOUND - 1, BOUND, BOUND + 1]
LEN_SEED = 11


def length_batch(m_long, long_first, seed):
    """Six landmarks: a single-depth track of exactly m_long observations, an EMPTY track, a single-depth one of 12 (a gross outlier from
    m_long >= 12 on) and three shorter 3-dof ones, none longer than the named one — except at m_long = 1, where the named track is flagged
    OVGPU_FEAT_TOO_FEW_MEAS and the others keep 5 / 4 / 9 / 3 observations so that a single-depth feature is still used.  Beyond 57
    observations the rig is 30 clones x 4 cameras."""
    K = 4 if m_long > 57 else 2
    p = ss.slam(6, LEN_REPS, seed, K=K)
    cap = m_long if m_long >= 2 else 99
    p = ts.with_lengths(p, [m_long, min(5, cap), 0, min(12, cap) if m_long >= 2 else 4, min(9, cap), min(3, cap)], patterns=("prefix",))
    if m_long >= 12:
        p = ts.make_outlier(p, LEN_OUTLIER, 15.0, seed)
    return p if long_first else ss.reordered(p, [1, 2, 3, 4, 5, 0])


# two small states of 10 clones, one camera, no calibration columns: 60 columns, then the landmarks
COLUMN_STATES = {
    # landmark 1 (single) has column 63: the last of the first 64-column block, and column D - 1
    "col-63-last": dict(reps=[G3, SINGLE], named=1, col=63, D=64),
    # landmark 2 (single) has column 64: the first of the second block (landmark 1, single as well, has 63)
    "col-64-first": dict(reps=[G3, SINGLE, SINGLE, A3], named=2, col=64, D=68),
}
COL_SEED = 21


def column_batch(cid, seed):
    st = COLUMN_STATES[cid]
    p = ss.slam(len(st["reps"]), st["reps"], seed, C=10, K=1, pose=0, intr=0)
    return p


NOISE_SIGMA = np.linspace(0.7, 2.5, 8)
MIX_NOISE = [G3, A3, AM, SINGLE, GI, AI, SINGLE, A3]  # two single-depth landmarks: one rejected by its multiplier, one used
NOISE_F = 3  # the first of them: accepted at its sigma with the multiplier 1, rejected by NOISE_MULT[NOISE_F] alone
NOISE_MULT = np.array([1.0, 0.8, 3.0, 0.02, 1.5, 2.0, 1.0, 0.6])
FIRST_5 = ss.FIRST_5


def _cases():
    out = []
    nofc = ss.nofc
    out.append(Case("single-6", "rep", functools.partial(ss.slam, 6, SINGLE, 46)))
    out.append(Case("mix", "rep", functools.partial(ss.slam, 8, MIX8, 13)))
    out.append(Case("mix-nofej", "rep", functools.partial(ss.slam, 8, MIX8, 13), options=dict(do_fej=0)))
    out.append(Case("mix-fisheye", "rep", functools.partial(ss.slam, 8, MIX8, 9, fisheye=True)))
    out.append(Case("mix-outliers", "rep", functools.partial(ss.slam, 8, MIX_ANCHOR, 7, outlier_frac=0.3), outliers=True))
    out.append(Case("anchor-clone-observed", "rep", functools.partial(ss.slam, 8, MIX_ANCHOR, 5)))
    out.append(Case("anchor-clone-unobserved", "rep", lambda: ss.without_anchor_clone(ss.slam(8, MIX_ANCHOR, 5))))
    for m in TRACKS:
        out.append(Case(f"len-{m}", "len", functools.partial(length_batch, m, True, LEN_SEED), outliers=m >= 12, m_max=m, named=0,
                        rejected=LEN_OUTLIER if m >= 12 else None))
    for m in (9, BOUND, BOUND + 1):
        out.append(Case(f"len-{m}-last", "len", functools.partial(length_batch, m, False, LEN_SEED), outliers=m >= 12, m_max=m, named=5,
                        rejected=LEN_OUTLIER - 1 if m >= 12 else None))
    for cid, st in COLUMN_STATES.items():
        out.append(Case(cid, "col", functools.partial(column_batch, cid, COL_SEED), options=nofc(0, 0), D=st["D"], named=st["named"], col=st["col"]))
    out.append(Case("noise", "noise", functools.partial(ss.slam, 8, MIX_NOISE, 13), sigma=NOISE_SIGMA, mult=NOISE_MULT, rejected=NOISE_F))
    # fall-backs at level 2: kernel 0, the level-0 context's bits (the 63-observation tracks are in the "len" group)
    out.append(Case("fb-general", "fb", functools.partial(ss.slam, 8, MIX8, 13), options=dict(no_fast_feature_kernel=1)))
    out.append(Case("fb-tsqr", "fb", functools.partial(ss.slam, 8, MIX8, 13), options=dict(compress_route=capi.COMPRESS_TSQR)))
    out.append(Case("fb-mode-a", "fb", functools.partial(ss.slam, 8, MIX8, 13), entry="compress"))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

oracle_run = ss.oracle_run
chunk_problem = ss.chunk_problem
