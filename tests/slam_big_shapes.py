"""The catalogue of SLAM batches that pin the BLOCK-ROW shape of the fused per-feature kernel of UpdaterSLAM::update — k_slam_y_big, tracks of
127 to SLY_MMAX_B observations (csrc/k_slam_y_big.h, ovgpu_debug_option "slam_fused_big" = 1 under "slam_fused" = 3) — at its track-length,
tile-row, pass-count, column-block and dispatch edges: tests/test_slam_big_shapes_cpu.py checks every batch on the oracle alone,
tests/test_gpu_slam_big.py runs it on the device.

expected_kernel_big() restates the rule FROM ITS DOCUMENTED TERMS (include/ovgpu.h: "slam_fused_big"), not from the library.  The builders are
slam_shapes' and track_shapes'.  Rig A is 59 clones x 4 cameras with the calibration columns off (a point is seen up to 236 times, D = 372 / 368
stays on the Gram route); rig B is BASELINE configs[4]'s geometry, 50 clones x 4 cameras with calibration on (D = 374 / 370).

The pass plan is k_feat_y_big's: passes of up to 136 tiles over tile rows that reach from their diagonal tile to the right-hand-side tile column.
A track of m observations has nt = ceil(2 m / 16) tile rows, row i holds nt + 1 - i tiles: n_passes() counts them and PASS_EDGES are the lengths
on both sides of every change (168 | 169: two to three passes, 208 | 209: three to four), derived here and asserted in the CPU file.

A helper module, not a conftest: nothing here is collected.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import slam_long_shapes as s3
import slam_shapes as ss
import slam_single_shapes as s2
import track_shapes as ts
from open_vins_amd import capi

SINGLE, BOUND, GRAM_MAX_D = ss.SINGLE, ss.BOUND, ss.GRAM_MAX_D
BOUND_LONG = s3.BOUND_LONG
BOUND_BIG = 232   # slamy::SLY_MMAX_B: 29 tile rows of the gate matrix
PASS_TILES = 136  # accumulator tiles of a pass: 8 wavefronts x 17


def expected_kernel_big(reps, m_max, D, K, C, level=3, big=1, general=0, gram_route=True, max_d=GRAM_MAX_D):
    """ovgpu_debug_option "last_feature_kernel" after a SLAM update with "slam_fused" at `level` and "slam_fused_big" at `big`: up to 126
    observations what level `level` does (slam_long_shapes.expected_kernel3); 127 to 232 observations 8 / 9 (without / with a single-depth landmark
    observed) when big >= 1 and level >= 3 and the long shape's terms hold — no_fast_feature_kernel off, 16 <= D, K C <= 8192, the whitened route
    (D <= max_d: 383, 511 under "gram_wide") —; 233 and beyond 0."""
    if m_max <= BOUND_LONG:
        return s3.expected_kernel3(reps, m_max, D, K, C, level, general, gram_route)
    single = any(int(r) == SINGLE for r in reps)
    ok = level >= 3 and big >= 1 and not general and m_max <= BOUND_BIG and D >= 16 and K * C <= 8192 and gram_route and D <= max_d
    return (9 if single else 8) if ok else 0


def n_passes(m):
    """passes of the block-row plan for a track of m observations"""
    nt = (2 * m + 15) // 16
    a, passes = 0, 0
    while a < nt:
        b, cnt = a, 0
        while b < nt and cnt + (nt + 1 - b) <= PASS_TILES:
            cnt += nt + 1 - b
            b += 1
        a, passes = b, passes + 1
    return passes


PASS_EDGES = [e for m in range(128, BOUND_BIG + 1) if n_passes(m) != n_passes(m - 1) for e in (m - 1, m)]  # [168, 169, 208, 209]


@dataclass
class Case(s3.Case):
    also_rejected: tuple = ()  # further planted outliers the gate must reject, next to `rejected`

    def kernel_at(self, level, big=1, max_d=GRAM_MAX_D):
        p = self.prob
        gram = self.gram_route and self.entry == "update" and self.options.get("compress_route", capi.COMPRESS_GRAM) != capi.COMPRESS_TSQR
        return expected_kernel_big(self.reps_observed, self.longest_track, self.columns, p.K, p.C, level, big, self.options.get("no_fast_feature_kernel", 0), gram, max_d)

    @property
    def kernel_big(self):
        return self.kernel_at(3, 1)


# --------------------------------------------------------------------------- builders
RIG_A = dict(C=59, K=4, pose=0, intr=0)
RIG_A_OPTS = ss.nofc(0, 0)
RIG_B = dict(C=50, K=4)
SEED = 11
OUTLIER = 3
LEN_REPS = s3.LEN_REPS
TRACKS = [126, 127, 128, 129] + PASS_EDGES + [224, 225, BOUND_BIG, BOUND_BIG + 1]
BOTH_ENDS = (126, 127, BOUND_BIG, BOUND_BIG + 1)
ALL_BIG = (232, 225, 224, 129, 128, 127)
STRIDE = (230, 190, 150, 127, 30, 2)
RIG_B_LENGTHS = (200, 176, 0, 12, 9, 3)


def rig_batch(kind, lengths, outlier, patterns=("prefix",), order=None, rig=None):
    p = ss.slam(6, LEN_REPS[kind], SEED, **(RIG_A if rig is None else rig))
    p = ts.with_lengths(p, list(lengths), patterns=patterns)
    for f in (() if outlier is None else np.atleast_1d(outlier)):
        p = ts.make_outlier(p, int(f), 15.0, SEED)
    return p if order is None else ss.reordered(p, order)


def length_batch(kind, m_long, long_first):
    """Six landmarks: a track of exactly m_long observations, an EMPTY track, four shorter ones, the 12-observation one a gross outlier"""
    return rig_batch(kind, (m_long, 5, 0, 12, 9, 3), OUTLIER, order=None if long_first else [1, 2, 3, 4, 5, 0])


COL_SEED = 21
COL_LENGTHS = (200, 200, 20, 12, 9, 5, 3, 130, 127)
COL_REPS = (ss.REPS5 * 2)[:9]   # nine 3-dof landmarks on rig B's state: D = 356 + 27 = 383, the sweep's twelfth block holds 31 columns


def column_batch(D):
    reps = list(COL_REPS) + ([SINGLE] if D == 384 else [])
    p = ss.slam(len(reps), reps, COL_SEED, **RIG_B)
    return ts.with_lengths(p, list(COL_LENGTHS) + ([7] if D == 384 else []), patterns=("prefix",))


NOISE_SIGMA, NOISE_MULT = s3.NOISE_SIGMA, s3.NOISE_MULT
NOISE_LENGTHS = (200, 140, 0, 12, 9, 3)
SHORT = {60: (60, 5, 0, 12, 9, 3), 100: (100, 5, 0, 12, 9, 3)}  # batches the shapes of level 3 hold: "slam_fused_big" leaves them their bits
FB_LENGTHS = (200, 5, 0, 12, 9, 3)


def _cases():
    out = []
    A = dict(options=RIG_A_OPTS)
    for kind in ("3dof", "single"):
        named = dict(named=0) if kind == "single" else {}
        for m in TRACKS:
            out.append(Case(f"len-{kind}-{m}", "len", functools.partial(length_batch, kind, m, True), outliers=True, m_max=m, rejected=OUTLIER,
                            lengths=(m, 5, 0, 12, 9, 3), **named, **A))
        for m in BOTH_ENDS:
            out.append(Case(f"len-{kind}-{m}-last", "len", functools.partial(length_batch, kind, m, False), outliers=True, m_max=m, rejected=OUTLIER - 1,
                            lengths=(5, 0, 12, 9, 3, m), **({"named": 5} if kind == "single" else {}), **A))
        # the length batch with a second gross outlier ON the 232-observation track: its 464 rows leave the stack
        out.append(Case(f"outlier-big-{kind}", "outlier", functools.partial(rig_batch, kind, (BOUND_BIG, 5, 0, 12, 9, 3), (0, OUTLIER)), outliers=True,
                        m_max=BOUND_BIG, rejected=0, also_rejected=(OUTLIER,), lengths=(BOUND_BIG, 5, 0, 12, 9, 3), **named, **A))
        # 233 observations with a 128-observation track behind them: the batch's longest track decides
        out.append(Case(f"beyond-{kind}", "beyond", functools.partial(rig_batch, kind, (BOUND_BIG + 1, 128, 0, 12, 9, 3), OUTLIER), outliers=True, m_max=BOUND_BIG + 1,
                        rejected=OUTLIER, lengths=(BOUND_BIG + 1, 128, 0, 12, 9, 3), **named, **A))
        out.append(Case(f"all-big-{kind}", "mix", functools.partial(rig_batch, kind, ALL_BIG, OUTLIER), outliers=True, m_max=BOUND_BIG, rejected=OUTLIER,
                        lengths=ALL_BIG, **named, **A))
        out.append(Case(f"stride-{kind}", "mix", functools.partial(rig_batch, kind, STRIDE, None, ("stride",)), m_max=230, lengths=STRIDE, **named, **A))
        out.append(Case(f"rig-b-{kind}", "rigb", functools.partial(rig_batch, kind, RIG_B_LENGTHS, OUTLIER, rig=RIG_B), outliers=True, m_max=200,
                        rejected=OUTLIER, lengths=RIG_B_LENGTHS, **named))
        for m, lengths in SHORT.items():
            out.append(Case(f"short-{m}-{kind}", "short", functools.partial(rig_batch, kind, lengths, OUTLIER), outliers=True, m_max=m, rejected=OUTLIER,
                            lengths=lengths, **named, **A))
    out.append(Case("col-383", "col", functools.partial(column_batch, 383), D=383, m_max=200))
    out.append(Case("col-384", "col", functools.partial(column_batch, 384), D=384, m_max=200))
    out.append(Case("noise", "noise", functools.partial(rig_batch, "single", NOISE_LENGTHS, OUTLIER), sigma=NOISE_SIGMA, mult=NOISE_MULT,
                    outliers=True, m_max=200, rejected=OUTLIER, lengths=NOISE_LENGTHS, named=0, **A))
    # fall-backs with a 200-observation batch: kernel 0, the switch-off context's bits
    fb = functools.partial(rig_batch, "single", FB_LENGTHS, OUTLIER)
    out.append(Case("fb-general", "fb", fb, options=dict(no_fast_feature_kernel=1, **RIG_A_OPTS), outliers=True))
    out.append(Case("fb-tsqr", "fb", fb, options=dict(compress_route=capi.COMPRESS_TSQR, **RIG_A_OPTS), outliers=True))
    out.append(Case("fb-semi-definite", "fb", lambda: ss.semi_definite(fb()), gram_route=False, outliers=True, **A))
    out.append(Case("mode-a-3dof", "modea", functools.partial(rig_batch, "3dof", FB_LENGTHS, OUTLIER), entry="compress", outliers=True, **A))
    out.append(Case("mode-a-single", "modea", fb, entry="compress", outliers=True, **A))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

oracle_run = ss.oracle_run

CHUNK_FIRST = [0, 3, 3, 6]


def chunk_problem():
    """the "all-big-single" batch as a frame of chunks: [0, 3) and [3, 6) hold tracks beyond 126 observations, the first a single-depth landmark too"""
    return BY_ID["all-big-single"].prob
