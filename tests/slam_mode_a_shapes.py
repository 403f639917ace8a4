"""Mode A of the SLAM update (ovgpu_slam_compress) on the pivoted Gram route, ovgpu_debug_option "slam_mode_a" = 1: the dispatch rule restated
once, the catalogue of batches that pin it and the reference every batch is held to (tests/test_slam_mode_a_shapes_cpu.py checks every case on
the oracle alone, tests/test_gpu_slam_mode_a.py runs it on the device).

What the library switches on, restated FROM THE DOCUMENTED RULE (include/ovgpu.h, at ovgpu_msckf_compress, ovgpu_slam_compress, "slam_mode_a" and
"mode_a_wide"), not from the library — D Jacobian columns (the active landmarks' included), LD = D + 1, NT = ceil(LD / 16) tile columns:
  * the level in force 0: the Householder triangle at every width, rows = D, codes (TSQR, 0, 0, 0);
  * the level in force 1 on a float64 context (gram_fp32 off, the stack whitened) whose compress_route is not OVGPU_COMPRESS_TSQR and whose prior
    block factors: D <= 383 takes mode_a_shapes.expected(D) — Gram and factor kernels by the column count exactly as the MSCKF entry — with ONE
    difference: at D = 257 .. 383 the un-whitening is k_unwhiten_blk<24>, code 6 on the two-panel factorisation's inverse tiles, 7 on
    k_uinv_tiles' (a step-wise prior, "unwhiten_blocked" = 0);
  * D = 384 .. 511: the Householder triangle, unless "mode_a_wide" = 1 is in force as well: then mode_a_wide_shapes' codes (2, 3, 4 | 5);
  * the per-feature stage: slam_long_shapes.expected_kernel3 with the route's terms ("slam_fused" = 0: the general kernel, 0).
rows_out is the numerical rank: at most the rows of the stack plus noise rows.

Every SLAM feature stacks an EVEN number of rows (2 m for a 3-dof landmark, 2 m - 2 for a single-depth one), so a stack of 15, 17, 31 or 33 rows
does not exist on this entry: the panel edges of k_pchol_panel (32 pivots per launch; 16-row tiles) are bracketed by 14 | 16 | 18 and 30 | 32 | 34.

A helper module, not a conftest: nothing here is collected.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import gram_wide_shapes as gws
import mode_a_shapes as mas
import mode_a_wide_shapes as maw
import slam_long_shapes as s3
import slam_shapes as ss
import track_shapes as ts
from open_vins_amd import capi
from parity_util import GATE_MARGIN

SINGLE = ss.SINGLE
NARROW_MAX_D, WIDE_MAX_D = 383, 511
UNWHITEN_BLK24_TILES, UNWHITEN_BLK24_INVERTED = 6, 7   # "last_unwhiten_kernel": k_unwhiten_blk<24> on the two-panel tiles / on k_uinv_tiles'
HOUSEHOLDER = (capi.COMPRESS_TSQR, 0, 0, 0)


# --------------------------------------------------------------------------- the rule
def takes_route(D, level, wide=0, *, compress_route=capi.COMPRESS_GRAM, fp32=0, whiten=True, prior_ok=True):
    cap = WIDE_MAX_D if (wide >= 1 and not fp32) else NARROW_MAX_D
    return bool(level >= 1 and not fp32 and whiten and compress_route != capi.COMPRESS_TSQR and prior_ok and D <= cap)


def expected_codes(D, level, wide=0, *, two_panel=True, unwhiten_blocked=True, single_launch=True, **route):
    """(ovgpu_last_update_route, "last_gram_kernel", "last_factor_kernel", "last_unwhiten_kernel") after ovgpu_slam_compress at D columns.
    two_panel: beyond 256 columns the prior block was factored by the two-panel kernels; single_launch: up to 256 columns, in one launch."""
    if not takes_route(D, level, wide, **route):
        return HOUSEHOLDER
    if D > NARROW_MAX_D:
        return maw.expected_codes(D, 1, two_panel=two_panel, unwhiten_blocked=unwhiten_blocked)
    route_, gram, factor, unwhiten = mas.codes(mas.expected(D, unwhiten_blocked=unwhiten_blocked, single_launch=single_launch))
    if D > 256:
        unwhiten = UNWHITEN_BLK24_TILES if (two_panel and unwhiten_blocked) else UNWHITEN_BLK24_INVERTED
    return route_, gram, factor, unwhiten


def expected_feature_kernel(reps, m_max, D, K, C, fused, level, wide=0, general=0, **route):
    """"last_feature_kernel" after ovgpu_slam_compress: "slam_fused"'s rule (slam_long_shapes.expected_kernel3) where the call takes the route"""
    return s3.expected_kernel3(reps, m_max, min(D, NARROW_MAX_D), K, C, fused, general, takes_route(D, level, wide, **route))


def family(codes):
    if codes[0] == capi.COMPRESS_TSQR:
        return "tsqr"
    if codes[2] == maw.FACTOR_PANEL:
        return maw.family(codes)
    fac = {1: "k_gram_pchol_blk<4,9,2>", 2: "k_gram_pchol_blk<7,15,4>"}.get(codes[2], "k_gram_pchol<NB>")
    gram = {1: "one-pass", 2: "k_gram_blk", 3: "k_gram_wide"}[codes[1]]
    uw = {1: "k_unwhiten_blk<16>", 2: "k_unwhiten<16>", 3: "k_unwhiten<24>", 6: "k_unwhiten_blk<24> on the two-panel tiles", 7: "k_unwhiten_blk<24> on k_uinv_tiles"}[codes[3]]
    return f"{fac} + {gram} + {uw}"


# --------------------------------------------------------------------------- the cases
@dataclass
class Case:
    id: str
    group: str
    build: object                                  # () -> Problem (lm_index set)
    D: int | None = None                           # the column count the case is named for
    options: dict = field(default_factory=dict)
    sigma: object = None
    mult: object = None
    wide: int = 0                                  # "mode_a_wide" of the case's contexts
    rows: int | None = None                        # the rows of the stack the case is named for
    active: object = None                          # the active landmark set (None: every resident landmark)
    outlier: int | None = None                     # the feature the gate must reject

    @functools.cached_property
    def prob(self):
        return self.build()

    def opts(self, **more):
        kw = dict(chi2_multipler=1.0)
        kw.update(self.options)
        kw.update(more)
        return capi.default_options(**kw)

    @property
    def reps(self):
        p = self.prob
        return np.asarray(p.lm_rep_each if getattr(p, "lm_rep_each", None) is not None else np.full(len(p.lm_value), p.lm_rep))

    @property
    def reps_observed(self):
        return self.reps[self.prob.lm_index]

    @property
    def columns(self):
        p = self.prob
        reps = self.reps if self.active is None else self.reps[np.asarray(self.active, int)]
        return ss.n_columns(p.C, p.K, int(np.where(reps == SINGLE, 1, 3).sum()), self.options.get("do_calib_camera_pose", 1),
                            self.options.get("do_calib_camera_intrinsics", 1))

    @property
    def longest_track(self):
        return int(np.diff(self.prob.meas_offsets).max())

    def codes(self, level=1, **kw):
        return expected_codes(self.columns, level, self.wide, compress_route=self.options.get("compress_route", capi.COMPRESS_GRAM),
                              fp32=self.options.get("gram_fp32", 0), whiten=not self.options.get("gram_no_whiten", 0), **kw)

    def feature_kernel(self, fused, level=1):
        p = self.prob
        return expected_feature_kernel(self.reps_observed, self.longest_track, self.columns, p.K, p.C, fused, level, self.wide,
                                       self.options.get("no_fast_feature_kernel", 0))


# D = 6 C + 14 K + 3 a + b: a 3-dof landmarks of the five representations in turn, b single-depth ones; six to twelve landmarks
COLUMN_STATES = {
    127: dict(C=15, K=1, a=7, b=2),    # 8 tile columns of [H | r]: the last count of k_gram_pchol_blk<4, 9, 2>
    128: dict(C=15, K=1, a=7, b=3),    # 9: k_gram_pchol_blk<7, 15, 4>
    223: dict(C=28, K=2, a=8, b=3),    # 14: its last count
    224: dict(C=28, K=2, a=9, b=1),    # 15: the rank-one k_gram_pchol<8>, the one-pass Gram kernel of 15 tile columns
    255: dict(C=29, K=4, a=8, b=1),    # 16 tile columns, the single-launch prior, k_unwhiten_blk<16>
    257: dict(C=29, K=4, a=8, b=3),    # 17: k_gram_blk, the two-panel prior, k_unwhiten_blk<24>  (256 is unreachable: slam_shapes.COLUMN_STATES)
    300: dict(C=40, K=2, a=10, b=2),   # 19: the middle of the band (the hygiene chain's link)
    360: dict(C=50, K=2, a=10, b=2),   # 23: k_gram_wide
    383: dict(C=54, K=2, a=10, b=1),   # 24 tile columns full: the last count without "mode_a_wide"
}
WIDE_D = (384, 385, 399, 400, 448, 449, 496, 511)   # gram_wide_shapes.SLAM_STATES, with "mode_a_wide" = 1 as well
# case id -> seed, chosen on the CPU (tests/test_slam_mode_a_shapes_cpu.py holds every case to it) so that the oracle uses a feature, rejects the
# planted outlier, leaves no statistic within parity_util.GATE_MARGIN of its threshold and the emulation leaves mode_a_shapes.GAP empty
SEEDS = {"col-64": 1, "col-127": 49, "col-128": 49, "col-223": 2, "col-257": 4, "col-300": 2, "col-383": 3, "wide-399": 1, "wide-400": 1, "wide-448": 7,
         "rep-0": 7, "rep-1": 7, "rep-3": 5, "rep-4": 5, "rep-5": 5, "rep-mix": 1, "rep-mix-nofej": 1, "noise": 2, "single-resident-unobserved": 2,
         "active-120": 6, "fused-3dof": 37, "fused-single-62": 27, "fused-single-63": 27, "fused-single-126": 15, "fused-single-127": 15}
OUTLIER = 2                     # a 3-dof landmark's track (gram_wide_shapes.slam_reps puts the single-depth ones at 1, 4, 7)


def reps_of(a, b):
    reps = (ss.REPS5 * 3)[:a]
    for i in range(b):
        reps.insert(min(1 + 3 * i, len(reps)), SINGLE)
    return reps


def state_batch(st, seed, lengths=None, outlier=OUTLIER, keep=None, cap=40, **kw):
    """every landmark of the state observed once, tracks of at most `cap` observations by the widest pick, one a gross outlier; lengths: the
    track lengths instead; keep: the features that stay in the batch (the others' landmarks stay resident)"""
    reps = reps_of(st["a"], st["b"])
    p = ss.slam(len(reps), reps, seed, C=st["C"], K=st["K"], **kw)
    lens = [min(int(m), cap) for m in np.diff(p.meas_offsets)] if lengths is None else list(lengths) + [0] * (len(reps) - len(lengths))
    p = ts.with_lengths(p, lens, patterns=("stride",))
    if outlier is not None:
        p = ts.make_outlier(p, outlier, 15.0 if lens[outlier] >= 10 else 10.0, seed)
    return p if keep is None else ss.reordered(p, list(keep))


def wide_rows_batch(lens):
    """the state of 511 columns (gram_wide_shapes.SLAM_STATES), the batch cut to the first tracks at `lens` observations: 3-dof landmarks, 2 m rows each"""
    reps = gws.slam_reps(511)
    p = ss.slam(len(reps), reps, gws.SLAM_SEED + 511, C=gws.SLAM_STATES[511]["C"], K=2)
    return ts.with_lengths(p, list(lens) + [0] * (p.F - len(lens)), patterns=("stride",))


def fused_batch(kind, m_long, seed):
    """slam_long_shapes.length_batch on a seed of this catalogue's: six landmarks, a track of exactly m_long observations, an EMPTY track, four
    shorter ones, the 12-observation one a gross outlier; kind "single": the long track and the outlier are single-depth landmarks'"""
    p = ss.slam(6, s3.LEN_REPS[kind], seed, **s3.RIG)
    p = ts.with_lengths(p, [m_long, 5, 0, 12, 9, 3], patterns=("prefix",))
    return ts.make_outlier(p, s3.OUTLIER, 15.0, seed)


def seed_of(cid, default):
    return SEEDS.get(cid, default)


def _cases():
    out = []
    # ---- column edges below 384
    for D in (63, 64):
        st = ss.COLUMN_STATES[D]
        out.append(Case(f"col-{D}", "col", functools.partial(ss.column_batch, D, seed_of(f"col-{D}", 21)), D=D, options=ss.nofc(st.get("pose", 1), st.get("intr", 1))))
    for D, st in COLUMN_STATES.items():
        out.append(Case(f"col-{D}", "col", functools.partial(state_batch, st, seed_of(f"col-{D}", 31 + D)), D=D, outlier=OUTLIER))
    # ---- ... and with "mode_a_wide" = 1 as well
    for D in WIDE_D:
        out.append(Case(f"wide-{D}", "wide", functools.partial(gws.slam_batch, D, seed_of(f"wide-{D}", gws.SEEDS.get(f"b-{D}", gws.SLAM_SEED + D))), D=D, wide=1, outlier=gws.SLAM_OUTLIER))
    # ---- short and long stacks
    s223, s511 = COLUMN_STATES[223], gws.SLAM_STATES[511]
    # one 3-dof landmark with one observation, one single-depth landmark with two: 2 rows each
    out.append(Case("rows-2-3dof", "rows", functools.partial(state_batch, s223, 31, (1,), None, (0,)), D=223, rows=2))
    out.append(Case("rows-2-single", "rows", functools.partial(state_batch, s223, 31, (0, 2), None, (1,)), D=223, rows=2))
    # at 511 columns (k_pchol_panel: 32 pivots per launch): stacks that stop inside, at and just past a 16-row tile and a panel
    for rows, lens in {14: (4, 0, 3), 16: (4, 0, 4), 18: (5, 0, 4), 30: (8, 0, 7), 32: (8, 0, 8), 34: (9, 0, 8)}.items():
        out.append(Case(f"rows-{rows}-511", "rows", functools.partial(wide_rows_batch, lens), D=511, wide=1, rows=rows))
    # a stack longer than D: twelve 3-dof landmarks x 40 observations over 30 clones x 4 cameras, 272 columns, 960 rows
    out.append(Case("rows-long-272", "rows", functools.partial(state_batch, dict(C=30, K=4, a=12, b=0), seed_of("rows-long-272", 31)), D=272, outlier=OUTLIER))
    # ---- representations and options (slam_shapes' and slam_single_shapes' batches)
    for r in ss.REPS5:
        out.append(Case(f"rep-{r}", "rep", functools.partial(ss.slam, 6, r, seed_of(f"rep-{r}", 40 + r))))
    out.append(Case(f"rep-{SINGLE}", "rep", functools.partial(ss.slam, 6, SINGLE, seed_of(f"rep-{SINGLE}", 40 + SINGLE))))
    out.append(Case("rep-mix", "rep", functools.partial(ss.slam, 10, [0, 2, SINGLE, 4, 1, 3, SINGLE, 0, 2, 4], seed_of("rep-mix", 3))))
    out.append(Case("rep-mix-nofej", "rep", functools.partial(ss.slam, 10, ss.MIX10, seed_of("rep-mix-nofej", 3)), options=dict(do_fej=0)))
    out.append(Case("rep-fisheye", "rep", functools.partial(ss.slam, 10, ss.MIX10, 9, fisheye=True)))
    out.append(Case("noise", "noise", functools.partial(ss.slam, 10, ss.MIX10, seed_of("noise", 3)), sigma=ss.NOISE_SIGMA, mult=ss.NOISE_MULT))
    out.append(Case("single-resident-unobserved", "rep", lambda: ss.reordered(ss.slam(8, [0, 2, 4, SINGLE, 1, 3, 0, 2], seed_of("single-resident-unobserved", 13)), [0, 1, 2, 4, 5, 6, 7])))
    # an active set narrower than the resident landmarks: ten resident, the batch's five alone get columns (208 + 15)
    out.append(Case("active-narrow", "active", lambda: ss.reordered(ss.slam(10, ss.MIX10, 36), [0, 2, 4, 6, 9]), active=(0, 2, 4, 6, 9)))
    # 120 resident landmarks, a set of six
    out.append(Case("active-120", "active", lambda: ss.reordered(ss.slam(120, (ss.REPS5 * 24), seed_of("active-120", 5)), [3, 20, 47, 64, 90, 119]), active=(3, 20, 47, 64, 90, 119)))
    # ---- every feature rejected, and only empty tracks
    out.append(Case("reject-223", "reject", functools.partial(state_batch, s223, 31), D=223, options=dict(chi2_multipler=1e-9)))
    out.append(Case("empty-223", "reject", functools.partial(state_batch, s223, 31, (0, 0, 0), None), D=223))
    # ---- the fused per-feature stage: slam_long_shapes' length batches on seeds of their own (32 clones x 4 cameras; D = 266 | 262)
    for kind in ("3dof", "single"):
        for m in (62, 63, 126, 127):
            seed = SEEDS.get(f"fused-{kind}-{m}", SEEDS.get(f"fused-{kind}"))
            out.append(Case(f"fused-{kind}-{m}", "fused", functools.partial(fused_batch, kind, m, seed), outlier=s3.OUTLIER))
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
CASE_IDS = list(BY_ID)
assert len(BY_ID) == len(CASES)
HYGIENE_CHAIN = ("col-383", "col-128", "col-300")


# --------------------------------------------------------------------------- the reference
def used_rows(prob, reps, status):
    """rows each used feature stacks, in batch order: 2 m for a 3-dof landmark, 2 m - 2 for a single-depth one"""
    m = np.diff(prob.meas_offsets)
    dof = np.where(np.asarray(reps)[prob.lm_index] == SINGLE, 1, 3)
    return [int(2 * m[f] - (3 - dof[f])) for f in range(prob.F) if status[f] == capi.FEAT_USED]


def reference(oracle, case):
    """What every run of a case is held to, computed once and cached on the case: the oracle's slam_update with its stack — scaled row by row to the
    context's sigma_pix where the case carries per-feature sigmas —, G = H^T H and g = H^T r of that stack, the float64 emulation of mode A on it
    (mode_a_shapes.emulate), its genuine rank and the number of features within GATE_MARGIN of their gate."""
    if not hasattr(case, "_ref"):
        prob, opts = case.prob, case.opts()
        ref = oracle.slam_update(opts, capi.Views(prob), want_stack=True, feat_sigma=case.sigma, feat_chi2mult=case.mult)
        H, r, cols = ref["H"].copy(), ref["r"].copy(), ref["col_cov_id"]
        if case.active is not None:  # the oracle stacks every resident landmark's columns: the ones outside the active set are zero
            dof = np.where(case.reps == SINGLE, 1, 3)
            lm_cols = np.concatenate([prob.lm_cov_id[l] + np.arange(dof[l]) for l in case.active])
            keep = (cols < prob.lm_cov_id.min()) | np.isin(cols, lm_cols)
            assert not H[:, ~keep].any()
            H, cols = np.ascontiguousarray(H[:, keep]), cols[keep]
        rows = used_rows(prob, case.reps, ref["feat_status"])
        assert sum(rows) == H.shape[0] == ref["rows"], (case.id, sum(rows), H.shape)
        if case.sigma is not None:
            used = np.flatnonzero(ref["feat_status"] == capi.FEAT_USED)
            scale = np.repeat(opts.sigma_pix / np.asarray(case.sigma, float)[used], rows)
            H, r = H * scale[:, None], r * scale
        He, re = mas.emulate(prob.P, cols, H, r)
        g = np.isfinite(ref["chi2"]) & (ref["chi2_thresh"] > 0)
        near = int((np.abs(ref["chi2"][g] / ref["chi2_thresh"][g] - 1.0) < GATE_MARGIN).sum())
        case._ref = dict(ref=ref, cols=cols, H_stack=H, r_stack=r, G=H.T @ H, g=H.T @ r, H_emu=He, r_emu=re, rank=mas.genuine_rank(He),
                         stack_rows=int(H.shape[0]), n_used=int((ref["feat_status"] == capi.FEAT_USED).sum()), near_gate=near)
    return case._ref
