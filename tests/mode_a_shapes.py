"""Mode A's default path (ovgpu_msckf_compress: whitened rows -> Gram matrix -> diagonally pivoted Cholesky -> X = R L^-1) at every tile edge:
the dispatch rule restated once, the catalogue of snapshots that pin it, the float64 emulation they are held to and the rank rule
(tests/test_mode_a_shapes_cpu.py checks every case on the oracle alone, tests/test_gpu_mode_a_shapes.py runs it on the device).

What the library switches on (enqueue_compress_gram, enqueue_gram_factor, enqueue_pipeline_body), restated FROM THE DOCUMENTED RULE (include/ovgpu.h,
at ovgpu_msckf_compress), not from the library — D Jacobian columns, LD = D + 1 with the residual column, NT = ceil(LD / 16) tile columns:
  * route: up to 24 tile columns (D <= 383) the pivoted factor, rows = its numerical rank; from 384 columns on the Householder triangle, rows = D;
  * factor: NT <= 8 k_gram_pchol_blk<4, 9, 2>, NT <= 14 k_gram_pchol_blk<7, 15, 4>, beyond (or with "pchol_blocked" = 0) the rank-one
    k_gram_pchol<NB>, NB = ceil(LD / 32);
  * Gram matrix: NT <= 16 the one-pass kernel launch_gram<T>, T = NT rounded up to even (15 stays 15); NT = 23 k_gram_wide; otherwise k_gram_blk;
  * un-whitening: ceil(D / 16) <= 16 k_unwhiten_blk<16> when the prior block was factored in ONE launch (that factorisation leaves the inverse
    diagonal tiles; it holds up to 256 columns and options.no_single_launch_cholesky turns it off) and "unwhiten_blocked" is on, k_unwhiten<16>
    otherwise; beyond 256 columns k_unwhiten<24>.
The GPU tests compare what ovgpu_last_update_route and ovgpu_debug_option "last_gram_kernel" / "last_factor_kernel" / "last_unwhiten_kernel"
report with expected(); EXPECT in tests/test_mode_a_shapes_cpu.py holds every case's values written out.

A helper module, not a conftest: nothing here is collected.
"""
from __future__ import annotations

import functools
import os
import sys
from collections import namedtuple
from dataclasses import dataclass, field

import numpy as np
import scipy.linalg as sla

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
from dev_mode_a_numerics import chol_pivoted  # noqa: E402  (the numpy restatement of the pivoted factorisation)

from open_vins_amd import capi  # noqa: E402
import track_shapes as ts  # noqa: E402

PIVOT_TOL = 1e-15     # the stop rule of the factorisation: a pivot at or under PIVOT_TOL of the first ends it
RANK_REL = 1e-6       # a row of the un-whitened factor is GENUINE when its 2-norm exceeds RANK_REL of the largest row's
GAP = (1e-7, 1e-5)    # ... and no row of the emulation may lie in between: noise rows stay under GAP[0], genuine ones over GAP[1]
SVD_REL = 1e-9        # the rank of the whitened triangle: singular values over SVD_REL of the largest


# --------------------------------------------------------------------------- the rule
Expect = namedtuple("Expect", "route factor nb gram gram_nt unwhiten")
# route "pchol" / "tsqr"; factor "blk<4,9,2>" / "blk<7,15,4>" / "rank-one" (nb: its NB) / None; gram "one-pass" (gram_nt: its T) / "blk" / "wide" /
# None; unwhiten "blk<16>" / "subst<16>" / "subst<24>" / None


def n_tiles(D):
    return (D + 1 + 15) // 16


def expected(D, blocked=True, *, unwhiten_blocked=None, single_launch=True):
    """What ovgpu_msckf_compress runs at D columns.  blocked: "pchol_blocked" (and "unwhiten_blocked" unless given on its own);
    single_launch: the prior block's factorisation ran as one launch (options.no_single_launch_cholesky = 0; it holds up to 256 columns)."""
    ub = blocked if unwhiten_blocked is None else unwhiten_blocked
    LD = D + 1
    nt = (LD + 15) // 16
    if nt > 24:
        return Expect("tsqr", None, 0, None, 0, None)
    if blocked and nt <= 8:
        factor, nb = "blk<4,9,2>", 0
    elif blocked and nt <= 14:
        factor, nb = "blk<7,15,4>", 0
    else:
        factor, nb = "rank-one", (LD + 31) // 32
    if nt <= 16:
        gram, gnt = "one-pass", (15 if nt == 15 else 2 * ((nt + 1) // 2))
    elif nt == 23:
        gram, gnt = "wide", 0
    else:
        gram, gnt = "blk", 0
    if (D + 15) // 16 <= 16:
        unwhiten = "blk<16>" if (ub and single_launch and D <= 256) else "subst<16>"
    else:
        unwhiten = "subst<24>"
    return Expect("pchol", factor, nb, gram, gnt, unwhiten)


def codes(e):
    """(ovgpu_last_update_route, "last_gram_kernel", "last_factor_kernel", "last_unwhiten_kernel") the library reports for an Expect."""
    route = capi.COMPRESS_PCHOLQR if e.route == "pchol" else capi.COMPRESS_TSQR
    gram = {None: 0, "one-pass": 1, "blk": 2, "wide": 3}[e.gram]
    factor = {None: 0, "blk<4,9,2>": 1, "blk<7,15,4>": 2, "rank-one": 32 + e.nb}[e.factor]
    unwhiten = {None: 0, "blk<16>": 1, "subst<16>": 2, "subst<24>": 3}[e.unwhiten]
    return route, gram, factor, unwhiten


def family(e):
    """The kernel family a run is booked under in the summary of the GPU file."""
    return "tsqr" if e.route == "tsqr" else f"{e.factor} + gram {e.gram} + unwhiten {e.unwhiten}"


# --------------------------------------------------------------------------- the cases
@dataclass
class Case:
    id: str
    group: str                       # "col" / "small" / "rank" / "reject"
    D: int
    state: dict                      # C, K, pose, intr as track_shapes' states
    build: object                    # () -> Problem
    R: int | None = None             # rank cases: the rows of the stack, sum over the features of 2 m - 3
    options: dict = field(default_factory=dict)

    def opts(self, **more):
        s = self.state
        kw = dict(chi2_multipler=1.0, do_calib_camera_pose=s.get("pose", 1), do_calib_camera_intrinsics=s.get("intr", 1))
        kw.update(self.options)
        kw.update(more)
        return capi.default_options(**kw)

    @functools.cached_property
    def prob(self):
        return self.build()


# D = 6 C + 14 K, full calibration
COLUMN_STATES = {126: (14, 3), 128: (19, 1), 222: (30, 3), 224: (28, 4), 254: (33, 4), 256: (38, 2), 258: (36, 3), 300: (43, 3), 320: (44, 4),
                 350: (49, 4), 352: (54, 2), 366: (54, 3), 368: (52, 4), 382: (59, 2), 384: (57, 3)}
COLUMN_SEEDS = {256: 36}  # D: seed where 31 does not meet the conditions of tests/test_mode_a_shapes_cpu.py (256, seed 31: one row at 8.2e-6 of the largest)
F_COLUMN = 24

# states below six tile columns, without extrinsic columns (the calibration estimate is the truth there).  Windows this short have short
# baselines: with one or two cameras the oracle's Gauss-Newton refinement fails on most seeds, four cameras give it enough views (eleven clones do with one)
SMALL_STATES = {
    "D30": dict(C=5, K=4, pose=0, intr=0),    # NT = 2
    "D42": dict(C=7, K=4, pose=0, intr=0),    # NT = 3
    "D48": dict(C=8, K=4, pose=0, intr=0),    # NT = 4, D a multiple of 16: the residual column alone in the last tile column
    "D66": dict(C=11, K=1, pose=0, intr=0),   # NT = 5, two Jacobian columns and the residual in the last tile column
}
SMALL_SEEDS = {"D30": 31, "D42": 31, "D48": 31, "D66": 31}
# (D = 64 = 8 clones + two cameras' intrinsics was tried on seeds 31 .. 69: the distortion coefficients leave rows of 1e-6 .. 1e-5 of the largest,
# inside the gap the rank rule needs empty)

RANK_STATES = {208: dict(C=30, K=2), 126: dict(C=14, K=3), 256: dict(C=38, K=2)}
# track lengths m per feature: rows 2 m - 3 each (1, 3, 5, 7, 9 for m = 2 .. 6)
RANK_LENGTHS = {1: (2,), 3: (3,), 4: (2, 3), 5: (4,), 8: (4, 3), 9: (6,), 16: (6, 5), 17: (6, 5, 2)}
RANK_R = {208: (1, 3, 4, 5, 8, 9, 16, 17), 126: (1, 3, 4, 8), 256: (1, 3, 4, 8, 17)}
RANK_SEEDS = {}         # (D, R): seed where 31 does not do
REJECT_STATE = dict(C=30, K=2)  # D = 208


def n_columns(st):
    return ts.n_columns(st["C"], st["K"], st.get("pose", 1), st.get("intr", 1))


def column_batch(D):
    C, K = COLUMN_STATES[D]
    p = ts._window(dict(C=C, K=K), F_COLUMN, COLUMN_SEEDS.get(D, 31))
    return p


def small_batch(name):
    return ts._window(SMALL_STATES[name], F_COLUMN, SMALL_SEEDS[name])


def rank_batch(D, R):
    """The first features of the window cut to RANK_LENGTHS[R] observations each, every one by the widest pick ("stride": the longest baseline a
    short track can have, so that it triangulates)."""
    lens = RANK_LENGTHS[R]
    assert sum(2 * m - 3 for m in lens) == R
    p = ts._window(RANK_STATES[D], 8, RANK_SEEDS.get((D, R), 31))
    p = p.subset(np.arange(len(lens)))
    return ts.with_lengths(p, list(lens), patterns=("stride",))


def reject_batch():
    return ts._window(REJECT_STATE, 8, 31)


def _cases():
    out = []
    for D, (C, K) in COLUMN_STATES.items():
        out.append(Case(f"col-{D}", "col", D, dict(C=C, K=K), functools.partial(column_batch, D)))
    for name, st in SMALL_STATES.items():
        out.append(Case(f"small-{name}", "small", n_columns(st), st, functools.partial(small_batch, name)))
    for D, Rs in RANK_R.items():
        for R in Rs:
            out.append(Case(f"rank-{D}-R{R}", "rank", D, RANK_STATES[D], functools.partial(rank_batch, D, R), R=R))
    # every feature rejected by the gate: a threshold of 1e-9 of the chi2 quantile
    out.append(Case("reject-208", "reject", 208, REJECT_STATE, reject_batch, options=dict(chi2_multipler=1e-9)))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
CASE_IDS = list(BY_ID)
assert len(BY_ID) == len(CASES)
assert all(c.D == n_columns(c.state) for c in CASES)


# --------------------------------------------------------------------------- the emulation and the rank rule
def row_rel_norms(H):
    """2-norms of the rows of H relative to the largest (an empty or all-zero H: zeros)."""
    H = np.asarray(H, dtype=np.float64)
    if H.shape[0] == 0:
        return np.zeros(0)
    n = np.linalg.norm(H, axis=1)
    return n / n.max() if n.max() > 0 else n


def genuine_rank(H):
    return int((row_rel_norms(H) > RANK_REL).sum())


def emulate(P, cols, H_comp, r_comp):
    """Mode A in float64 numpy, as tests/test_mode_a_numerics.py: the oracle's compressed system times L (P_DD = L L^T), its Gram matrix, the
    diagonally pivoted factor, un-whitened.  Returns (H, r) with every row the factorisation produced (zero rows cut)."""
    D = len(cols)
    if H_comp.shape[0] == 0:
        return np.zeros((0, D)), np.zeros(0)
    L = np.linalg.cholesky(P[np.ix_(cols, cols)])
    A = np.hstack([H_comp @ L, r_comp[:, None]])
    Rw = chol_pivoted(A.T @ A, D, PIVOT_TOL)[:D]
    Rw = Rw[np.abs(Rw).sum(axis=1) > 0]
    H = sla.solve_triangular(L, Rw[:, :D].T, lower=True, trans="T").T
    return np.ascontiguousarray(H), np.ascontiguousarray(Rw[:, D])


def svd_rank(P, cols, H):
    """Rank of the whitened H L at SVD_REL."""
    if H.shape[0] == 0:
        return 0
    sv = np.linalg.svd(H @ np.linalg.cholesky(P[np.ix_(cols, cols)]), compute_uv=False)
    return int((sv > SVD_REL * sv[0]).sum()) if sv[0] > 0 else 0


def reference(oracle, case):
    """What every leg of a case is held to, computed once and cached on the case: the oracle's triangulation and update (with its compressed
    system), G = H^T H and g = H^T r of that system, the emulation's (H, r), its genuine rank and the stack's rows."""
    if not hasattr(case, "_ref"):
        prob, opts = case.prob, case.opts()
        v = capi.Views(prob)
        tri = oracle.triangulate(opts, v)
        ref = oracle.msckf_update(opts, v, want_compressed=True, given=tri)
        cols = oracle.column_map(opts, v)
        Hc, rc = ref["H_comp"], ref["r_comp"]
        He, re = emulate(prob.P, cols, Hc, rc)
        used = ref["feat_status"] == capi.FEAT_USED
        m = np.diff(prob.meas_offsets)
        case._ref = dict(tri=tri, ref=ref, cols=cols, G=Hc.T @ Hc, g=Hc.T @ rc, H_emu=He, r_emu=re, rank=genuine_rank(He),
                         stack_rows=int((2 * m[used] - 3).sum()), n_used=int(used.sum()))
    return case._ref
