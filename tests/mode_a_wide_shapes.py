"""Mode A (ovgpu_msckf_compress) on the pivoted Gram route at 384 .. 511 Jacobian columns, ovgpu_debug_option "mode_a_wide" = 1: the dispatch rule
restated once, the catalogue of snapshots that pin it and a numpy restatement of the panelled factorisation (tests/test_mode_a_wide_shapes_cpu.py
checks every case on the oracle alone, tests/test_gpu_mode_a_wide.py runs it on the device).

What the library switches on, restated FROM THE DOCUMENTED RULE (include/ovgpu.h, at ovgpu_msckf_compress and at "mode_a_wide"), not from the
library — D Jacobian columns, LD = D + 1 with the residual column, NT = ceil(LD / 16) tile columns:
  * with the level in force 0, or D <= 383: mode_a_shapes.expected(D) — from 384 columns on the Householder triangle, rows = D;
  * with the level in force 1 on a float64 context (gram_fp32 off) whose compress_route is not OVGPU_COMPRESS_TSQR, 384 <= D <= 511, the prior block
    positive definite: route OVGPU_COMPRESS_PCHOLQR, rows = the numerical rank; Gram matrix k_gram_blk (code 2, four column windows); factor
    k_pchol_panel + k_pchol_schur (code 3); un-whitening k_unwhiten_blk<32> — code 4 on the inverse diagonal tiles the two-panel factorisation of
    the prior block left, code 5 on k_uinv_tiles' when the prior was factored step-wise (options.no_single_launch_cholesky, "chol_wide" = 0) or
    "unwhiten_blocked" is 0;
  * ovgpu_slam_compress keeps the Householder triangle at every width.

The cases: mode_a_shapes.Case objects (mode_a_shapes.reference / emulate serve them as they serve that catalogue) on gram_wide_shapes.MSCKF_STATES.

A helper module, not a conftest: nothing here is collected.
"""
from __future__ import annotations

import functools

import numpy as np

import gram_wide_shapes as gws
import mode_a_shapes as mas
import track_shapes as ts
from open_vins_amd import capi

NARROW_MAX_D = 383
WIDE_MAX_D = 511
PANEL = 32            # pivots per launch of k_pchol_panel (the restatement below is also run at 16)
GRAM_BLK, FACTOR_PANEL, UNWHITEN_TILES, UNWHITEN_INVERTED = 2, 3, 4, 5  # the codes of "last_gram_kernel" / "last_factor_kernel" / "last_unwhiten_kernel"


# --------------------------------------------------------------------------- the rule
def takes_wide_route(D, level, *, compress_route=capi.COMPRESS_GRAM, fp32=0, prior_ok=True, slam=False):
    return bool(level >= 1 and not fp32 and compress_route != capi.COMPRESS_TSQR and prior_ok and not slam and NARROW_MAX_D < D <= WIDE_MAX_D)


def expected_codes(D, level, *, two_panel=True, unwhiten_blocked=True, **route):
    """(ovgpu_last_update_route, "last_gram_kernel", "last_factor_kernel", "last_unwhiten_kernel") after ovgpu_msckf_compress at D columns with the
    level of "mode_a_wide" in force; two_panel: the prior block was factored by the two-panel kernels (the default beyond 256 columns)."""
    if takes_wide_route(D, level, **route):
        return (capi.COMPRESS_PCHOLQR, GRAM_BLK, FACTOR_PANEL, UNWHITEN_TILES if (two_panel and unwhiten_blocked) else UNWHITEN_INVERTED)
    if D > NARROW_MAX_D or route.get("compress_route") == capi.COMPRESS_TSQR or route.get("fp32") or route.get("slam") or not route.get("prior_ok", True):
        return (capi.COMPRESS_TSQR, 0, 0, 0)
    return mas.codes(mas.expected(D))


def family(codes):
    if codes[0] == capi.COMPRESS_TSQR:
        return "tsqr"
    if codes[2] == FACTOR_PANEL:
        return "k_pchol_panel/schur + k_gram_blk + k_unwhiten_blk<32> on " + ("the two-panel tiles" if codes[3] == UNWHITEN_TILES else "k_uinv_tiles")
    return f"narrow route {codes[1:]}"


# --------------------------------------------------------------------------- the cases
F_COLUMN = 24
COLUMN_D = (384, 386, 398, 400, 416, 448, 450, 480, 482, 496, 498, 510)
COLUMN_SEEDS = {448: 41}   # seeds 31 and 36 leave a row inside mode_a_shapes.GAP at 448 columns (so does 36 at 400)
MIX_D = (384, 400, 450, 510)   # gram_wide_shapes' mixed batches (twelve tracks, one a gross outlier): the factor stops inside a panel (a-496: two rows in the gap)
RANK_D = 510
RANK_LENGTHS = {1: (2,), 17: (6, 5, 2), 33: (10, 9, 2)}  # rows 2 m - 3 per feature: one row, past a 16-row panel, past a 32-row panel
REJECT_D = 400


def column_batch(D):
    return ts._window(gws.MSCKF_STATES[D], F_COLUMN, COLUMN_SEEDS.get(D, 31))


def mix_batch(D):
    return gws.msckf_batch(D, gws.msckf_seed(D))


def rank_batch(R):
    """mode_a_shapes.rank_batch's cut on the state of 510 columns: the first features of an eight-feature window, every track by the widest pick"""
    lens = RANK_LENGTHS[R]
    assert sum(2 * m - 3 for m in lens) == R
    p = ts._window(gws.MSCKF_STATES[RANK_D], 8, 31).subset(np.arange(len(lens)))
    return ts.with_lengths(p, list(lens), patterns=("stride",))


def semi_definite_batch(D):
    import slam_shapes as ss
    return ss.semi_definite(column_batch(D))


def _cases():
    out = []
    for D in COLUMN_D:
        out.append(mas.Case(f"col-{D}", "col", D, gws.MSCKF_STATES[D], functools.partial(column_batch, D)))
    for D in MIX_D:
        out.append(mas.Case(f"mix-{D}", "mix", D, gws.MSCKF_STATES[D], functools.partial(mix_batch, D)))
    for R in RANK_LENGTHS:
        out.append(mas.Case(f"rank-{RANK_D}-R{R}", "rank", RANK_D, gws.MSCKF_STATES[RANK_D], functools.partial(rank_batch, R), R=R))
    out.append(mas.Case(f"reject-{REJECT_D}", "reject", REJECT_D, gws.MSCKF_STATES[REJECT_D], functools.partial(column_batch, REJECT_D),
                        options=dict(chi2_multipler=1e-9)))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
CASE_IDS = list(BY_ID)
assert len(BY_ID) == len(CASES)
assert all(c.D == mas.n_columns(c.state) for c in CASES)
# what must not move: the narrow side and the middle link of the hygiene chain
NARROW = {
    382: mas.Case("narrow-382", "col", 382, gws.MSCKF_STATES[382], functools.partial(column_batch, 382)),
    208: mas.Case("narrow-208", "col", 208, ts.SMALL, functools.partial(ts._window, ts.SMALL, F_COLUMN, 31)),
}
HYGIENE_CHAIN = ("col-510", 208, "col-448")


# --------------------------------------------------------------------------- the panelled factorisation, restated in numpy
def chol_pivoted_panelled(M, nfree, tol, nb=PANEL):
    """k_pchol_wide.h in numpy: panels of nb pivots in the manner of LAPACK's dpstrf.  The trailing matrix G is touched once per panel (the Schur
    step); inside a panel row p of G is corrected by the panel's own earlier rows only (lazily), and the pivot comes from `dots` — the starting
    diagonal minus the squares of the rows written so far.  Columns nfree .. are carried: never a pivot, never masked.  Returns (R, pivots)."""
    G = np.array(M, dtype=np.float64)
    n = G.shape[0]
    R = np.zeros_like(G)
    dots = np.diag(G).copy()
    live = np.zeros(n, bool)
    live[:nfree] = True
    pivots, d0, k, stop = [], None, 0, False
    while k < nfree and not stop:
        k0 = k
        for _ in range(nb):
            if k >= nfree:
                break
            p = int(np.argmax(np.where(live, dots, -np.inf)))
            d = dots[p]
            d0 = d if d0 is None else d0
            if not (d > tol * d0 and d > 0.0):
                stop = True
                break
            row = (G[p, :] - R[k0:k, p] @ R[k0:k, :]) / np.sqrt(d)
            row[:nfree][~live[:nfree]] = 0.0
            R[k, :] = row
            dots -= row * row
            live[p] = False
            pivots.append(p)
            k += 1
        if not stop and k < nfree:
            G -= R[k0:k, :].T @ R[k0:k, :]
    return R, pivots


def chol_pivoted_order(M, nfree, tol):
    """The pivot order of tools/dev_mode_a_numerics.chol_pivoted (which returns R alone): its own loop, restated for the order only."""
    M = np.array(M, dtype=np.float64)
    n = M.shape[0]
    done = np.zeros(n, bool)
    done[nfree:] = True
    d0 = np.max(np.diag(M)[:nfree])
    order = []
    for _ in range(nfree):
        p = int(np.argmax(np.where(done, -np.inf, np.diag(M))))
        d = M[p, p]
        if d <= tol * d0:
            break
        row = M[p, :] / np.sqrt(d)
        row[done & (np.arange(n) < nfree)] = 0.0
        M -= np.outer(row, row)
        done[p] = True
        order.append(p)
    return order


def whitened_gram(case, R):
    """[H L | r]^T [H L | r] of the oracle's compressed system: what the factorisation is handed (mode_a_shapes.emulate forms the same matrix)"""
    L = np.linalg.cholesky(case.prob.P[np.ix_(R["cols"], R["cols"])])
    A = np.hstack([R["ref"]["H_comp"] @ L, R["ref"]["r_comp"][:, None]])
    return A.T @ A
