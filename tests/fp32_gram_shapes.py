"""The two fp32 Gram kernels of options.gram_fp32 held to a float64 Gram matrix, element by element: the cases, the plan of every case, the
reference, the bound and a numpy emulation of both kernels' arithmetic (tests/test_fp32_gram_shapes_cpu.py checks every case on the oracle and
numpy alone, tests/test_gpu_fp32_gram.py runs it on the device).  Imports no GPU code.

The two device paths (include/ovgpu.h at options.gram_fp32):
  * group A, gram32::k_gram_f32 + k_gram_f32_reduce (k_gram32.h, "last_gram_kernel" 5): the fused per-feature kernels store the whitened stack as
    floats, row stride LDF = 32 ceil(LD / 32), and 8 wavefronts per workgroup hold a part of the triangle of 32 x 32 macro tiles;
  * group B, gram::k_gram_blk<true> (k_gram.h, "last_gram_kernel" 2): a float64 stack on a gram_fp32 context — the general per-feature kernel
    (options.no_fast_feature_kernel) or "featy_big" = 2 — rounded to float stage by stage, 8 x 8-tile blocks of the grid per block pair.

The reference.  A = [H_comp L | r_comp] of the oracle's compressed system (mode_a_wide_shapes.whitened_gram's matrix), G_ref = A^T A in
np.longdouble, n_i = sqrt(G_ref[i, i]) and  e(G) = max over i, j <= D with n_i n_j > 0 of |G_ij - G_ref_ij| / (n_i n_j);  where n_i = 0, row and
column i of G must be exactly zero.  ONE element is not the compressed system's: a stack of more than D rows is compressed to D, and the part
of the residual that no column of H reaches goes with the rows dropped — r_comp^T r_comp is short of r^T r (by 1e-2 of it on these batches), while
the device's G[D, D] is the whole stack's.  G_ref[D, D] is therefore the sum of squares of the projected residuals of the features the oracle
used (uncompressed_stack: its Jacobians, its nullspace projection), and tests/test_fp32_gram_shapes_cpu.py holds that stack's whole Gram matrix
to A^T A at every other element at 1e-12.

The bound, from the arithmetic (u = 2^-24).  Every element of the stack is rounded to float once: a product x_ri x_rj carries 2 u.  Nothing longer
than one stage of 32 rows is summed in single precision: 32 dependent roundings of a partial sum that Cauchy-Schwarz bounds by n_i n_j, 32 u.  The
stages are summed in float64.  k_gram_f32 rounds a workgroup's total to float once more: u.  With sum_r |x_ri x_rj| <= n_i n_j that is
e <= 35 u for k_gram_f32 and e <= 34 u for k_gram_blk<true>; BOUND = 40 u (2.4e-6) is asserted for both — the slack covers the second-order
terms and the reference's own error.  A float64 context must stay under CONTROL = 1 % of it, or the reference is too coarse for the case.

The plan of a case restates the host's rules (enqueue_compress_gram, api_pipeline.inc; the rows of a batch as set_row_layout lays them out: a
track of m >= 2 observations stacks 2 m - 3 rows whatever becomes of the feature, a shorter one none):
  NT = ceil(LD / 16), NTM = ceil(LD / 32), LDF = 32 NTM, P = ceil(NTM (NTM + 1) / 2 / 48) parts,
  Gw = max(1, ceil(rows / 1536), min(ceil(2 CUs / P), ceil(rows / 128))) workgroups per part, each ceil(rows / Gw) rows rounded up to 32;
  k_gram_blk: NB = ceil(NT / 8) windows, nchunks = ceil(rows / 32), Gb = max(1, min(CUs, nchunks)), workgroup w the chunks
  floor(nchunks w / Gb) .. floor(nchunks (w + 1) / Gb) - 1.

A helper module, not a conftest: nothing here is collected.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import track_shapes as ts
from open_vins_amd import capi

U = 2.0 ** -24
BOUND = 40 * U
CONTROL = 0.01 * BOUND
MUTATION_FLOOR = 4 * BOUND          # what every planted fault must exceed in the emulation
MI355X_CUS = 256                    # the plans of the CPU test; the GPU test takes multi_processor_count
STAGE = 32                          # rows per stage of either kernel
G32_NW, G32_MAXT, G32_ROWS_WG = 8, 6, 1536
GB_T = 8                            # tiles per window of k_gram_blk
GK_BLK, GK_F32 = 2, 5               # "last_gram_kernel"
TOL_DX_F32, TOL_P_F32 = 1e-4, 1e-3  # the suite's bounds of an fp32 update (shard_shapes), unchanged


def cdiv(a, b):
    return -(-int(a) // int(b))


# --------------------------------------------------------------------------- the plan
def rows_of(lengths):
    """set_row_layout: the row offsets of a batch of tracks of these lengths (0 .. F)"""
    return np.concatenate([[0], np.cumsum([2 * int(m) - 3 if m >= 2 else 0 for m in lengths])]).astype(np.int64)


@dataclass
class Plan:
    D: int
    rows: int
    cus: int

    @property
    def LD(self):
        return self.D + 1

    @property
    def NT(self):
        return cdiv(self.LD, 16)

    @property
    def LG(self):
        return 16 * self.NT

    # ---- k_gram_f32
    @property
    def NTM(self):
        return cdiv(self.LD, 32)

    @property
    def LDF(self):
        return 32 * self.NTM

    @property
    def tiles(self):
        return self.NTM * (self.NTM + 1) // 2

    @property
    def parts(self):
        return cdiv(self.tiles, G32_NW * G32_MAXT)

    @property
    def Gw(self):
        return max(1, cdiv(self.rows, G32_ROWS_WG), min(cdiv(2 * self.cus, self.parts), cdiv(self.rows, 128)))

    @property
    def rows_wg(self):
        return cdiv(cdiv(self.rows, self.Gw), STAGE) * STAGE

    @property
    def wg_rows(self):
        """the rows of every workgroup of a part, in order (a workgroup past the end holds none)"""
        return [max(0, min(self.rows_wg * (w + 1), self.rows) - self.rows_wg * w) for w in range(self.Gw)]

    @property
    def wg_stages(self):
        return [cdiv(r, STAGE) for r in self.wg_rows]

    @property
    def last_stage_rows(self):
        """rows of the stack's last stage (the one that reads the pad rows unless it is full)"""
        r = [x for x in self.wg_rows if x > 0][-1]
        return r - STAGE * (cdiv(r, STAGE) - 1)

    @property
    def tiles_per_wave(self):
        """tile counts of the 8 wavefronts of every part (gram32_tile_table's deal)"""
        out = []
        for part in range(self.parts):
            n_part = self.tiles * (part + 1) // self.parts - self.tiles * part // self.parts
            out.append([n_part * (w + 1) // G32_NW - n_part * w // G32_NW for w in range(G32_NW)])
        return out

    @property
    def fetch_chunks(self):
        """1 KiB chunks of a 32-row stage (k_gram_f32's DMA fetch)"""
        return STAGE * self.LDF * 4 // 1024

    # ---- k_gram_blk
    @property
    def NB(self):
        return cdiv(self.NT, GB_T)

    @property
    def pairs(self):
        return self.NB * (self.NB + 1) // 2

    @property
    def nchunks(self):
        return cdiv(self.rows, STAGE)

    @property
    def Gb(self):
        return max(1, min(self.cus, self.nchunks))

    @property
    def blk_chunks(self):
        """(first, end) chunk of every workgroup of k_gram_blk"""
        return [(self.nchunks * w // self.Gb, self.nchunks * (w + 1) // self.Gb) for w in range(self.Gb)]


# --------------------------------------------------------------------------- the cases
W3 = ts.REGION_STATES["nt5"]                  # D = 74
W4 = ts.REGION_STATES["D96"]                  # D = 96: LD = 97
W7 = ts.SMALL                                 # D = 208
W9 = dict(C=44, K=1, pose=0, intr=0)          # D = 264
W10 = dict(C=50, K=1, pose=0, intr=0)         # D = 300
W12 = dict(C=59, K=2)                         # D = 382
ROW_STATE = W7                                # the row cases' one width: 30 clones of two cameras triangulate every track


@dataclass
class Case:
    id: str
    group: str                       # "A" k_gram_f32 / "B" k_gram_blk<true>
    state: dict
    lengths: tuple                   # observations per feature, in batch order
    seed: int
    what: str
    options: dict = field(default_factory=dict)   # on top of gram_fp32 = 1
    debug: dict = field(default_factory=dict)
    failed: tuple = (1,)             # features whose injected triangulation status is FEAT_TRI_FAILED (rejected before the gate, rows in the stack)
    outlier: int | None = 3          # the feature moved by a gross pixel offset (rejected by the gate); None: no such feature
    full: bool = False               # full tracks of the window as test_gpu_gram_regions_shapes `deep` takes them (`lengths`: the feature count alone)

    @property
    def D(self):
        s = self.state
        return ts.n_columns(s["C"], s["K"], s.get("pose", 1), s.get("intr", 1))

    def opts(self, fp32=1, **more):
        s = self.state
        kw = dict(chi2_multipler=1.0, gate_always_factor=1, do_calib_camera_pose=s.get("pose", 1), do_calib_camera_intrinsics=s.get("intr", 1),
                  gram_fp32=fp32)
        kw.update(self.options)
        kw.update(more)
        return capi.default_options(**kw)

    @functools.cached_property
    def prob(self):
        if self.full:
            F = len(self.lengths)
            p = ts._window(self.state, F, self.seed)
            p = ts.keep_tracks(p, [np.arange(int(p.meas_offsets[f + 1] - p.meas_offsets[f]))[:1 if f == 0 else None] for f in range(F)])
            return ts.make_outlier(p, self.outlier % F, 15.0, self.seed)
        F = len(self.lengths)
        p = ts.with_lengths(ts._window(self.state, F, self.seed), list(self.lengths), patterns=("stride",))
        got = np.diff(p.meas_offsets)
        assert np.array_equal(got, self.lengths), (self.id, got)
        if self.outlier is not None:
            f = self.outlier % F
            p = ts.make_outlier(p, f, 10.0 if self.lengths[f] < 10 else 15.0, self.seed)
        return p

    @property
    def track_lengths(self):
        return np.diff(self.prob.meas_offsets)

    @property
    def row_off(self):
        return rows_of(self.track_lengths)

    @property
    def rows(self):
        return int(self.row_off[-1])

    def plan(self, cus=MI355X_CUS):
        return Plan(self.D, self.rows, cus)

    @property
    def gram_kernel(self):
        return GK_F32 if self.group == "A" else GK_BLK


def _lens(*runs):
    """feature 0 one observation (no rows), then the lengths given"""
    return (1,) + tuple(runs)


# widths: a dozen tracks of 8 .. 20 observations — a few hundred rows, no multiple of 32
WIDTH_LENGTHS = _lens(9, 8, 20, 11, 14, 17, 10, 19, 12, 16, 13, 18)     # rows 0 + sum(2 m - 3) = 298
W3_LENGTHS = _lens(9, 8, 10, 7, 10, 6, 10, 9, 8, 10, 9, 10)             # ten clones of one camera hold ten observations: 176 rows
W3_SEED = 305   # of the seeds 300 .. 329 one of the few on which the oracle triangulates six of the short window's tracks and the gate rejects the outlier
GENERAL = dict(no_fast_feature_kernel=1)


def _a_cases():
    w = WIDTH_LENGTHS
    return [
        Case("w3", "A", W3, W3_LENGTHS, W3_SEED, "NTM 3, NT 5 odd: the last macro column is clipped to LG = 80 < 96"),
        Case("w4-residual-alone", "A", W4, w, 300, "LD = 97: macro column 3 holds the residual column and 31 pad columns"),
        Case("w7", "A", W7, w, 31, "28 tiles: wavefronts with 3 and 4 tiles"),
        Case("w9", "A", W9, w, 31, "45 of 48 slots, one part, wavefronts with 5 and 6 tiles"),
        Case("w10", "A", W10, w, 31, "55 tiles: the first width with two parts"),
        Case("w12", "A", W12, w, 31, "LD 383, LDF 384, one pad column, 78 tiles in two parts of 39, all 48 fetch chunks, NT 24"),
        # rows, at D = 208
        Case("r29", "A", ROW_STATE, _lens(3, 8, 8), 31, "rows <= 31: one partial stage, one workgroup", outlier=2),
        Case("r128", "A", ROW_STATE, _lens(8, 9, 20, 12, 14, 10), 31, "128 rows: no pad row is multiplied, one workgroup of 4 stages"),
        Case("r129", "A", ROW_STATE, _lens(8, 9, 20, 12, 14, 10, 2), 31, "129 rows: Gw 2 with 96 + 33, the last stage holds ONE row"),
        Case("r304", "A", ROW_STATE, _lens(8, 9, 20, 12, 14, 17, 10, 19, 12, 16, 13, 20), 32, "304 rows: Gw 3 (128 + 128 + 48)"),
        Case("r447", "A", ROW_STATE, _lens(*(WIDTH_LENGTHS[1:] + (15, 20, 11, 20, 16))), 33, "447 rows: Gw 4, the reduction's loop of four without a remainder"),
        Case("r532", "A", ROW_STATE, _lens(*(WIDTH_LENGTHS[1:] + (15, 20, 11, 20, 16, 18, 9, 20))), 34, "532 rows: Gw 5"),
    ]


def _b_cases():
    w = WIDTH_LENGTHS
    return [
        Case("nb1", "B", W3, W3_LENGTHS, W3_SEED, "NT 5: tiles 5 to 7 of the only window lie outside the grid", options=GENERAL),
        Case("nb2", "B", W7, w, 31, "NT 14: three block pairs, partial second window", options=GENERAL),
        Case("nb2-featy-big2", "B", W7, w, 31, "the same through k_feat_y_big<8, 5>, which has no float twin", debug=dict(featy_big=2)),
        Case("nb3-partial", "B", W10, w, 31, "NT 19: six block pairs, partial third window", options=GENERAL),
        Case("nb3-full", "B", W12, w, 31, "NT 24: every window full", options=GENERAL),
        Case("c1", "B", ROW_STATE, _lens(3, 8, 8), 31, "29 rows: one chunk, the reduction with one partial", options=GENERAL, outlier=2),
        Case("c2", "B", ROW_STATE, _lens(3, 8, 8, 10), 31, "46 rows: two partials, the reduction's unrolled pair", options=GENERAL, outlier=2),
        Case("c3", "B", ROW_STATE, _lens(3, 8, 8, 10, 14), 31, "71 rows: three partials, the remainder of the loop of two, a clamped last stage", options=GENERAL,
             outlier=2),
        Case("c4-exact", "B", ROW_STATE, _lens(8, 9, 20, 12, 14, 10), 31, "128 rows = 4 chunks exactly: no partial stage", options=GENERAL),
        Case("deep", "B", ROW_STATE, (0,) * 256, 401, "256 full tracks: every workgroup turns its LDS double buffer over", options=GENERAL, full=True),
    ]


CASES = _a_cases() + _b_cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
A_IDS = [c.id for c in CASES if c.group == "A"]
B_IDS = [c.id for c in CASES if c.group == "B"]
WIDTH_IDS = ["w3", "w4-residual-alone", "w7", "w9", "w10", "w12"]
ROW_IDS = ["r29", "r128", "r129", "r304", "r447", "r532"]

# `stale`, on ONE context: a batch of all-accepted rows first, then a smaller one whose rejected features and tail lie on rows the first left
# non-zero, then (a context takes a state of another size: ovgpu_set_state) one at another NTM, so that the cached tile table is rebuilt
STALE_FIRST = Case("stale-first", "A", ROW_STATE, (20, 20, 20, 20, 20, 20, 20, 20), 35, "296 rows, every feature accepted", failed=(), outlier=None)
STALE_SECOND = Case("stale-second", "A", ROW_STATE, _lens(12, 16, 14, 20, 10, 18), 36, "162 rows: the failed feature on rows 0 .. 20, the outlier on 50 .. 74")
STALE_THIRD = Case("stale-third", "A", W3, W3_LENGTHS, W3_SEED, "w3's batch on the context of D = 208: NTM 7 -> 3")


# --------------------------------------------------------------------------- the reference
def reference(oracle, case):
    """What every leg of a case is held to, computed once and cached on the case: the oracle's triangulation with the case's failures injected,
    its update (with the compressed system), A = [H_comp L | r_comp] and G_ref = A^T A in np.longdouble."""
    if not hasattr(case, "_ref"):
        prob, opts = case.prob, case.opts(fp32=0)
        v = capi.Views(prob)
        tri = oracle.triangulate(opts, v)
        for f in case.failed:   # (a track the oracle did not triangulate anyway keeps its own verdict)
            if tri["status"][f] == capi.FEAT_USED:
                tri["status"][f] = capi.FEAT_TRI_FAILED
        ref = oracle.msckf_update(opts, v, want_compressed=True, given=tri)
        cols = oracle.column_map(opts, v)
        L = np.linalg.cholesky(prob.P[np.ix_(cols, cols)])
        A = np.hstack([ref["H_comp"] @ L, ref["r_comp"][:, None]])
        Al = A.astype(np.longdouble)
        G = Al.T @ Al
        case._ref = dict(tri=tri, ref=ref, cols=cols, L=L, A=A)
        X, off = _uncompressed_stack(oracle, case, case._ref)
        rl = X[:, case.D].astype(np.longdouble)
        G[case.D, case.D] = rl @ rl   # (the compressed system drops the residual's part outside the range of H)
        case._ref.update(G=G, n=np.sqrt(np.diag(G)), X=X, row_off=off)
    return case._ref


def gram_error(G, R):
    """e(G) against the reference R of reference(); G: at least (D + 1) x (D + 1).  Asserts the exact zeros where n_i = 0."""
    n = R["n"]
    ld = n.size
    G = np.asarray(G)[:ld, :ld]
    live = n > 0
    assert not G[~live, :].any() and not G[:, ~live].any(), "a column the reference leaves empty is not exactly zero"
    if not live.any():
        return 0.0
    nn = np.outer(n[live], n[live])
    return float(np.max(np.abs(G[np.ix_(live, live)].astype(np.longdouble) - R["G"][np.ix_(live, live)]) / nn))


def worst_element(G, R):
    n = R["n"]
    ld = n.size
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(np.outer(n, n) > 0, np.abs(np.asarray(G)[:ld, :ld].astype(np.longdouble) - R["G"]) / np.outer(n, n), 0)
    return np.unravel_index(int(np.argmax(e)), e.shape)


def uncompressed_stack(oracle, case):
    R = reference(oracle, case)
    return R["X"], R["row_off"]


def _uncompressed_stack(oracle, case, R):
    """The whitened stack [H_f L | r_f] feature by feature as the device lays it out (rows_of): the oracle's Jacobian of every USED feature,
    projected onto the nullspace of its position block; the rows of every other feature are zero.  (rows x (D + 1), per-feature row offsets)"""
    prob, opts = case.prob, case.opts(fp32=0)
    v = capi.Views(prob)
    off = case.row_off
    X = np.zeros((case.rows, case.D + 1))
    tri, st = R["tri"], R["ref"]["feat_status"]
    for f in range(prob.F):
        if st[f] != capi.FEAT_USED:
            continue
        H_f, H_x, res = oracle.feature_jacobian(opts, v, f, tri["p_FinG"][f], tri["p_FinA"][f], int(tri["anchor_meas"][f]))
        _, Hp, rp = oracle.nullspace_project(H_f, H_x, res)
        assert Hp.shape[0] == off[f + 1] - off[f]
        X[off[f]:off[f + 1], :case.D] = Hp @ R["L"]
        X[off[f]:off[f + 1], case.D] = rp
    return X, off


# --------------------------------------------------------------------------- both kernels' arithmetic in numpy
def _stage_sums(X32, first, stages):
    """float sums of `stages` consecutive 32-row stages from row `first` (X32: float32, padded with zero rows): [stages, n, n] float32"""
    n = X32.shape[1]
    if stages == 0:
        return np.zeros((0, n, n), np.float32)
    blk = X32[first:first + STAGE * stages].reshape(stages, STAGE, n)
    return np.matmul(blk.transpose(0, 2, 1), blk)   # (float32 in, float32 accumulation over the 32 rows of a stage)


def _padded32(X, pad_rows=None):
    n = X.shape[0]
    Xp = np.zeros((cdiv(n, STAGE) * STAGE + STAGE, X.shape[1]), np.float32)
    Xp[:n] = X.astype(np.float32)
    if pad_rows is not None:
        Xp[n:n + pad_rows.shape[0]] = pad_rows
    return Xp


def emulate_f32(X, plan, *, skip_last_stage=False, pad_rows=None, skip_top_column=False, swap_tiles=False):
    """k_gram_f32 + k_gram_f32_reduce on the stack X (rows x LD, float64): the stack rounded to float, per stage 32-row float sums, a workgroup's
    stages summed in float64 and rounded to float once, the workgroups summed in float64.  The keywords plant the faults the cases are named for."""
    Xp = _padded32(X, pad_rows)
    ld = X.shape[1]
    G = np.zeros((ld, ld))
    live = [w for w, r in enumerate(plan.wg_rows) if r > 0]
    for w in live:
        st = plan.wg_stages[w]
        if skip_last_stage and w == live[-1]:
            st -= 1
        S = _stage_sums(Xp, plan.rows_wg * w, st)
        G += S.astype(np.float64).sum(axis=0).astype(np.float32).astype(np.float64)
    return _tile_faults(G, 32, plan.NTM, skip_top_column, swap_tiles)


def emulate_blk(X, plan, *, skip_last_stage=False, pad_rows=None, skip_top_column=False, swap_tiles=False):
    """k_gram_blk<true> + k_gram_blk_reduce: every 32-row chunk rounded to float and summed in float, the chunks of a workgroup and the workgroups
    in float64.  (pad_rows: the kernel never reads behind the stack — the clamped rows are staged as zeros; a fault that staged them instead.)"""
    Xp = _padded32(X, pad_rows)
    ld = X.shape[1]
    G = np.zeros((ld, ld))
    for w, (c0, c1) in enumerate(plan.blk_chunks):
        if skip_last_stage and c1 == plan.nchunks:
            c1 -= 1
        G += _stage_sums(Xp, STAGE * c0, max(0, c1 - c0)).astype(np.float64).sum(axis=0)
    return _tile_faults(G, 16 * GB_T, plan.NB, skip_top_column, swap_tiles)


def _tile_faults(G, width, n, skip_top_column, swap_tiles):
    ld = G.shape[0]
    if skip_top_column:            # the top macro column / window never written
        G[:, width * (n - 1):] = 0
        G[width * (n - 1):, :] = 0
    if swap_tiles and ld > 32:     # two neighbouring tiles of one wavefront's run change places: (0, 0) and (0, 1), 16 x 16 here for either kernel
        a, b = G[:16, :16].copy(), G[:16, 16:32].copy()
        G[:16, :16], G[:16, 16:32] = b, a
        G[16:32, :16] = G[:16, 16:32].T
    return G


def emulate(case, X, plan=None, **faults):
    plan = plan or case.plan()
    return (emulate_f32 if case.group == "A" else emulate_blk)(X, plan, **faults)
