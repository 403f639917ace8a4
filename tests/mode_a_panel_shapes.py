"""Mode A's pivoted Gram route at 256 .. 383 Jacobian columns on the panelled factor, ovgpu_debug_option "mode_a_panel": the dispatch rule restated
once and the catalogue of batches that pin it (tests/test_mode_a_panel_shapes_cpu.py checks every case on the oracle alone,
tests/test_gpu_mode_a_panel.py runs it on the device).

What the library switches on, restated FROM THE DOCUMENTED RULE (include/ovgpu.h, at ovgpu_msckf_compress, ovgpu_slam_compress and "mode_a_panel"),
not from the library — D Jacobian columns, LD = D + 1 with the residual column, NT = ceil(LD / 16) tile columns:
  * the level in force 0: mode_a_shapes.expected (ovgpu_msckf_compress) and slam_mode_a_shapes.expected_codes (ovgpu_slam_compress) as they stand;
  * the level in force 1 (values above it are taken as it), where the call takes the pivoted Gram route (a float64 context, the whitened stack,
    compress_route not OVGPU_COMPRESS_TSQR, a prior block that factors; ovgpu_slam_compress: "slam_mode_a" in force) and PANEL_MIN_NT <= NT <= 24
    (D = 256 .. 383): the factor is k_pchol_panel + k_pchol_schur (code 3), and at D = 257 .. 383 ovgpu_msckf_compress un-whitens with
    k_unwhiten_blk<24> as ovgpu_slam_compress does (code 6 on the two-panel factorisation's inverse tiles, 7 on k_uinv_tiles'); the Gram kernel
    and every other width — 224 .. 255 columns, 15 and 16 tile columns, among them: the rank-one k_gram_pchol<8> measured no slower there — keep
    their codes;
  * D >= 384: "mode_a_wide" decides, as before.

The MSCKF cases are mode_a_shapes.Case objects (mode_a_shapes.reference serves them), the SLAM cases slam_mode_a_shapes.Case objects
(slam_mode_a_shapes.reference).  slam_mode_a_shapes' fused-single-127 is left out: it puts a noise row at 7.8e-8 of the largest under either
restatement of the factorisation, against the bound of 1e-7.

A helper module, not a conftest: nothing here is collected.
"""
from __future__ import annotations

import functools

import numpy as np

import mode_a_shapes as mas
import mode_a_wide_shapes as maw
import slam_mode_a_shapes as sma
import track_shapes as ts
from open_vins_amd import capi

PANEL_MIN_NT = 17        # the route's lower edge in tile columns of [H | r] (include/ovgpu.h names the library's MODE_A_PANEL_MIN_NT): D = 256
PANEL_MAX_NT = 24        # D = 383; beyond: "mode_a_wide"
PANEL = maw.PANEL        # pivots per launch
FACTOR_PANEL = 3         # "last_factor_kernel"
TOP_LEVEL = 1            # the highest level the library keeps (values above it are taken as it)
MSCKF, SLAM = "msckf", "slam"


# --------------------------------------------------------------------------- the rule
def in_band(D):
    return PANEL_MIN_NT <= mas.n_tiles(D) <= PANEL_MAX_NT


def expected_codes(D, level, entry=MSCKF, *, wide=0, slam_level=1, two_panel=True, unwhiten_blocked=True, single_launch=True,
                   compress_route=capi.COMPRESS_GRAM, fp32=0, whiten=True, prior_ok=True):
    """(ovgpu_last_update_route, "last_gram_kernel", "last_factor_kernel", "last_unwhiten_kernel") after ovgpu_msckf_compress / ovgpu_slam_compress
    at D columns with the level of "mode_a_panel" in force."""
    level = min(level, TOP_LEVEL)
    if entry == SLAM:
        base = sma.expected_codes(D, slam_level, wide, two_panel=two_panel, unwhiten_blocked=unwhiten_blocked, single_launch=single_launch,
                                  compress_route=compress_route, fp32=fp32, whiten=whiten, prior_ok=prior_ok)
    elif D > maw.NARROW_MAX_D:
        base = maw.expected_codes(D, wide if whiten else 0, two_panel=two_panel, unwhiten_blocked=unwhiten_blocked, compress_route=compress_route, fp32=fp32,
                                  prior_ok=prior_ok)
    elif compress_route == capi.COMPRESS_TSQR or fp32 or not whiten or not prior_ok:
        base = sma.HOUSEHOLDER
    else:
        base = mas.codes(mas.expected(D, unwhiten_blocked=unwhiten_blocked, single_launch=single_launch))
    if level < 1 or base[0] != capi.COMPRESS_PCHOLQR or not in_band(D):
        return base
    route, gram, factor, unwhiten = base
    factor = FACTOR_PANEL
    if D > 256:
        unwhiten = sma.UNWHITEN_BLK24_TILES if (two_panel and unwhiten_blocked) else sma.UNWHITEN_BLK24_INVERTED
    return route, gram, factor, unwhiten


def takes_panel(D, level, entry=MSCKF, **kw):
    return expected_codes(D, level, entry, **kw)[2] == FACTOR_PANEL and in_band(D)


def family(codes):
    if codes[0] == capi.COMPRESS_TSQR:
        return "tsqr"
    if codes[2] != FACTOR_PANEL or codes[3] in (maw.UNWHITEN_TILES, maw.UNWHITEN_INVERTED):
        return sma.family(codes)
    fac = "k_pchol_panel"
    gram = {1: "one-pass", 2: "k_gram_blk", 3: "k_gram_wide"}[codes[1]]
    uw = {1: "k_unwhiten_blk<16>", 2: "k_unwhiten<16>", 6: "k_unwhiten_blk<24> on the two-panel tiles", 7: "k_unwhiten_blk<24> on k_uinv_tiles"}[codes[3]]
    return f"{fac} / k_pchol_schur + {gram} + {uw}"


# --------------------------------------------------------------------------- the MSCKF cases
# mode_a_shapes' column cases of 15 .. 24 tile columns: 224 and 254 below the edge (they keep the rank-one factor under the switch), the edge at
# 256, whole panels at 256, 320, 352, a last panel of two pivots at 258, 64-column edges of G at 254 | 256 and 318 | 320, 24 tile columns at 368 and 382
MSCKF_COLUMN_D = (224, 254, 256, 258, 300, 318, 320, 350, 352, 366, 368, 382)
STATE_318 = dict(C=46, K=3)          # 46 clones x 3 cameras, full calibration: LG = 320, five 64-column groups of G full
STATE_300 = dict(C=43, K=3)          # mode_a_shapes.COLUMN_STATES[300]
SEEDS = {"col-318": 31, "slam-col-319": 5}   # chosen on the CPU (tests/test_mode_a_panel_shapes_cpu.py): SLAM seeds 1 .. 4 leave a row inside mode_a_shapes.GAP at 319 columns
# track lengths m per feature, 2 m - 3 rows each: one row; past a 16-row tile; the panel's edge 31 | 32 | 33; past two panels
ROWS_LENGTHS = {1: (2,), 17: (6, 5, 2), 31: (10, 8, 2), 32: (6, 6, 5, 5), 33: (10, 9, 2), 65: (10, 10, 10, 8, 2)}


def col_318_batch():
    return ts._window(STATE_318, mas.F_COLUMN, SEEDS["col-318"])


def rows_batch(R):
    """mode_a_shapes.rank_batch's cut on the state of 300 columns: the first features of an eight-feature window, every track by the widest pick"""
    lens = ROWS_LENGTHS[R]
    assert sum(2 * m - 3 for m in lens) == R
    p = ts._window(STATE_300, 8, 31).subset(np.arange(len(lens)))
    return ts.with_lengths(p, list(lens), patterns=("stride",))


def _msckf_cases():
    out = []
    for D in MSCKF_COLUMN_D:
        out.append(mas.BY_ID[f"col-{D}"] if D != 318 else mas.Case("col-318", "col", 318, STATE_318, col_318_batch))
    for R in ROWS_LENGTHS:
        out.append(mas.Case(f"rank-300-R{R}", "rank", 300, STATE_300, functools.partial(rows_batch, R), R=R))
    out.append(mas.Case("reject-300", "reject", 300, STATE_300, functools.partial(mas.column_batch, 300), options=dict(chi2_multipler=1e-9)))
    return out


MSCKF_CASES = _msckf_cases()
MSCKF_BY_ID = {c.id: c for c in MSCKF_CASES}
MSCKF_IDS = list(MSCKF_BY_ID)
assert len(MSCKF_BY_ID) == len(MSCKF_CASES) and all(c.D == mas.n_columns(c.state) for c in MSCKF_CASES) and mas.COLUMN_STATES[300] == (43, 3)
# what must not move: the widths on either side of the band and the middle link of the hygiene chain
BELOW = mas.BY_ID["col-222"]                     # 14 tile columns: k_gram_pchol_blk<7, 15, 4>  (224 and 254, 15 and 16: among the cases)
ABOVE = maw.BY_ID["col-384"]                     # 25: Householder, or "mode_a_wide"'s panels
NARROW_208 = maw.NARROW[208]
HYGIENE_CHAIN = ("col-382", NARROW_208, "col-300")


# --------------------------------------------------------------------------- the SLAM cases
SLAM_COLUMN_IDS = ("col-224", "col-255", "col-257", "col-300", "col-360", "col-383", "rows-long-272")   # (383: LD = LG = 384, no padding column)
SLAM_STATE_319 = dict(C=43, K=2, a=10, b=3)      # 6 x 43 + 14 x 2 + 3 x 10 + 3: LD = LG = 320, no padding column
SLAM_STATE_300 = sma.COLUMN_STATES[300]
SLAM_ROWS_LENGTHS = {30: (8, 0, 7), 32: (8, 0, 8), 34: (9, 0, 8)}   # 3-dof landmarks (reps_of puts a single-depth one at 1), 2 m rows each
SLAM_BELOW = sma.BY_ID["col-223"]


def _slam_cases():
    out = [sma.BY_ID[i] for i in SLAM_COLUMN_IDS]
    out.append(sma.Case("col-319", "col", functools.partial(sma.state_batch, SLAM_STATE_319, SEEDS["slam-col-319"]), D=319, outlier=sma.OUTLIER))
    for rows, lens in SLAM_ROWS_LENGTHS.items():
        out.append(sma.Case(f"rows-{rows}-300", "rows", functools.partial(sma.state_batch, SLAM_STATE_300, sma.SEEDS["col-300"], lens, None), D=300, rows=rows))
    out.append(sma.Case("reject-300", "reject", functools.partial(sma.state_batch, SLAM_STATE_300, sma.SEEDS["col-300"]), D=300, options=dict(chi2_multipler=1e-9)))
    return out


SLAM_CASES = _slam_cases()
SLAM_BY_ID = {c.id: c for c in SLAM_CASES}
SLAM_IDS = list(SLAM_BY_ID)
assert len(SLAM_BY_ID) == len(SLAM_CASES)


def slam_codes(case, level, **kw):
    """expected_codes for a SLAM case with "slam_mode_a" = 1 (the case's options decide the rest)"""
    return expected_codes(case.columns, level, SLAM, wide=case.wide, compress_route=case.options.get("compress_route", capi.COMPRESS_GRAM),
                          fp32=case.options.get("gram_fp32", 0), whiten=not case.options.get("gram_no_whiten", 0), **kw)


def whitened_gram(P, cols, H, r):
    """[H L | r]^T [H L | r]: what the factorisation is handed (mode_a_shapes.emulate forms the same matrix)"""
    L = np.linalg.cholesky(P[np.ix_(cols, cols)])
    A = np.hstack([H @ L, np.asarray(r)[:, None]])
    return A.T @ A, L
