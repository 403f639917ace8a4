"""The catalogue of SLAM batches that pin the LONG shape of the fused per-feature kernel of UpdaterSLAM::update — k_slam_y<.., 17, 32, 126>,
tracks of 63 to 126 observations (csrc/k_slam_y.h, ovgpu_debug_option "slam_fused" = 3) — at its track-length, lane, tile-row, column-block and
dispatch edges: tests/test_slam_long_shapes_cpu.py checks every batch on the oracle alone, tests/test_gpu_slam_long.py runs it on the device.

expected_kernel3() restates the level-3 rule FROM ITS DOCUMENTED TERMS (include/ovgpu.h: "slam_fused"), not from the library.  The builders are
slam_shapes' and track_shapes'.  The rig is 32 clones x 4 cameras (a point is seen up to 128 times); the column cases take 51 clones.

A helper module, not a conftest: nothing here is collected.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import slam_shapes as ss
import slam_single_shapes as s2
import track_shapes as ts
from open_vins_amd import capi

SINGLE, BOUND, GRAM_MAX_D = ss.SINGLE, ss.BOUND, ss.GRAM_MAX_D
BOUND_LONG = 126  # slamy::SLY_MMAX_L: 2 m + 4 <= 256 rows of the augmented gate matrix in 16 tile rows
G3, GI, A3, AI, AM = ss.REPS5


def expected_kernel3(reps, m_max, D, K, C, level=3, general=0, gram_route=True):
    """ovgpu_debug_option "last_feature_kernel" after a SLAM update of a batch that observes landmarks of the representations `reps`, longest
    track m_max, D Jacobian columns, with "slam_fused" at `level`: 0 unless the level is at least 1, no_fast_feature_kernel is off, 16 <= D,
    K C <= 8192, the update takes the whitened route (D <= 383, compress_route not TSQR, not mode A, no Householder repeat) and the longest
    track is within the level's bound — 62 at levels 1 and 2, 126 at level 3.  A batch that observes a single-depth landmark needs level 2.
    Then 4 / 5 (without / with a single-depth landmark) up to 62 observations, 6 / 7 from 63 to 126."""
    single = any(int(r) == SINGLE for r in reps)
    bound = BOUND_LONG if level >= 3 else BOUND
    ok = level >= 1 and not general and m_max <= bound and D >= 16 and K * C <= 8192 and gram_route and D <= GRAM_MAX_D
    if not ok or (single and level < 2):
        return 0
    return (6 if m_max > BOUND else 4) + (1 if single else 0)


@dataclass
class Case(s2.Case):
    lengths: tuple | None = None  # the track lengths the case is built with

    def kernel_at(self, level):
        p = self.prob
        gram = self.gram_route and self.entry == "update" and self.options.get("compress_route", capi.COMPRESS_GRAM) != capi.COMPRESS_TSQR
        return expected_kernel3(self.reps_observed, self.longest_track, self.columns, p.K, p.C, level, self.options.get("no_fast_feature_kernel", 0), gram)

    @property
    def kernel3(self):
        return self.kernel_at(3)


# --------------------------------------------------------------------------- builders
RIG = dict(C=32, K=4)
SEED = 11
OUTLIER = 3
LEN_REPS = {"3dof": ss.LEN_REPS, "single": s2.LEN_REPS}  # D = 266 | 262: s2.LEN_REPS has the long track and the 12-observation one single-depth
TRACKS = [63, 64, 65, 72, 73, 95, 96, 97, 125, 126, 127]
BOTH_ENDS = (63, 126, 127)
ALL_LONG = (126, 120, 97, 80, 64, 63)
STRIDE = (100, 90, 70, 64, 30, 2)


def rig_batch(kind, lengths, outlier, patterns=("prefix",), order=None):
    p = ss.slam(6, LEN_REPS[kind], SEED, **RIG)
    p = ts.with_lengths(p, list(lengths), patterns=patterns)
    if outlier is not None:
        p = ts.make_outlier(p, outlier, 15.0, SEED)
    return p if order is None else ss.reordered(p, order)


def length_batch(kind, m_long, long_first):
    """Six landmarks: a track of exactly m_long observations, an EMPTY track, four shorter ones, the 12-observation one a gross outlier"""
    return rig_batch(kind, (m_long, 5, 0, 12, 9, 3), OUTLIER, order=None if long_first else [1, 2, 3, 4, 5, 0])


COL_RIG = dict(C=51, K=4)       # 6 x 51 + 4 x 14 = 362 columns, then the landmarks
COL_SEED = 21
COL_LENGTHS = (126, 126, 20, 12, 9, 5, 3)
COL_REPS = (ss.REPS5 * 2)[:7]   # seven 3-dof landmarks: D = 383, the Gram route's last column count and the sweep's last (12th) column block


def column_batch(D):
    reps = list(COL_REPS) + ([SINGLE] if D == 384 else [])
    p = ss.slam(len(reps), reps, COL_SEED, **COL_RIG)
    return ts.with_lengths(p, list(COL_LENGTHS) + ([7] if D == 384 else []), patterns=("prefix",))


NOISE_SIGMA = np.array([1.3, 1.1, 1.0, 2.5, 1.2, 1.8])
NOISE_MULT = np.array([1.0, 0.8, 3.0, 1.5, 1.0, 2.0])
SHORT = (60, 5, 0, 12, 9, 3)    # a batch the short shapes hold: level 3 must do with it what level 2 does


def _cases():
    out = []
    for kind in ("3dof", "single"):
        named = dict(named=0) if kind == "single" else {}
        for m in TRACKS:
            out.append(Case(f"len-{kind}-{m}", "len", functools.partial(length_batch, kind, m, True), outliers=True, m_max=m, rejected=OUTLIER,
                            lengths=(m, 5, 0, 12, 9, 3), **named))
        for m in BOTH_ENDS:
            out.append(Case(f"len-{kind}-{m}-last", "len", functools.partial(length_batch, kind, m, False), outliers=True, m_max=m, rejected=OUTLIER - 1,
                            lengths=(5, 0, 12, 9, 3, m), **({"named": 5} if kind == "single" else {})))
        # the gross outlier ON the long track: its 252 rows leave the stack
        out.append(Case(f"outlier-long-{kind}", "outlier", functools.partial(rig_batch, kind, (126, 5, 0, 12, 9, 3), 0), outliers=True, m_max=126, rejected=0,
                        lengths=(126, 5, 0, 12, 9, 3), **named))
    out.append(Case("all-long", "mix", functools.partial(rig_batch, "3dof", ALL_LONG, OUTLIER), outliers=True, m_max=126, rejected=OUTLIER, lengths=ALL_LONG))
    out.append(Case("all-long-single", "mix", functools.partial(rig_batch, "single", ALL_LONG, OUTLIER), outliers=True, m_max=126, rejected=OUTLIER,
                    lengths=ALL_LONG, named=0))
    out.append(Case("stride", "mix", functools.partial(rig_batch, "3dof", STRIDE, None, ("stride",)), m_max=100, lengths=STRIDE))
    out.append(Case("stride-single", "mix", functools.partial(rig_batch, "single", STRIDE, None, ("stride",)), m_max=100, lengths=STRIDE, named=0))
    out.append(Case("col-383", "col", functools.partial(column_batch, 383), D=383, m_max=126))
    out.append(Case("col-384", "col", functools.partial(column_batch, 384), D=384, m_max=126))
    out.append(Case("noise", "noise", functools.partial(rig_batch, "single", (126, 70, 0, 12, 9, 3), OUTLIER), sigma=NOISE_SIGMA, mult=NOISE_MULT,
                    outliers=True, m_max=126, rejected=OUTLIER, lengths=(126, 70, 0, 12, 9, 3), named=0))
    for kind in ("3dof", "single"):
        out.append(Case(f"short-{kind}", "short", functools.partial(rig_batch, kind, SHORT, OUTLIER), outliers=True, m_max=60, rejected=OUTLIER, lengths=SHORT,
                        **({"named": 0} if kind == "single" else {})))
    # fall-backs at level 3 with a long batch: kernel 0, the switch-off context's bits
    fb = functools.partial(rig_batch, "single", (100, 5, 0, 12, 9, 3), OUTLIER)
    out.append(Case("fb-general", "fb", fb, options=dict(no_fast_feature_kernel=1), outliers=True))
    out.append(Case("fb-tsqr", "fb", fb, options=dict(compress_route=capi.COMPRESS_TSQR), outliers=True))
    out.append(Case("fb-mode-a", "fb", fb, entry="compress", outliers=True))
    out.append(Case("fb-semi-definite", "fb", lambda: ss.semi_definite(fb()), gram_route=False, outliers=True))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

oracle_run = ss.oracle_run

CHUNK_FIRST = [0, 3, 3, 6]


def chunk_problem():
    """the "all-long-single" batch as a frame of chunks: [0, 3) and [3, 6) hold tracks beyond 62 observations, the first a single-depth landmark too"""
    return BY_ID["all-long-single"].prob
