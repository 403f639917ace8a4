"""The catalogue of states and batches that pin the feature-sharded MSCKF update (ovgpu_multi_*, ovgpu_msckf_update_sharded, ovgpu_msckf_local /
_merge_update, ovgpu_msckf_local_gram / _gram_update) at every route, tile, rank-count and shard edge: tests/test_shard_shapes_cpu.py checks every
batch on the oracle and numpy alone, tests/test_gpu_shard_edges.py runs it on the device through the loop-back communicator (ovgpu_multi_create
with a repeated device) and on separate contexts.

The rules below are restated FROM THEIR DOCUMENTED TERMS (include/ovgpu.h, DESIGN.md sections 4.3, 4.4 and 5), not read from the library:
  * the deal of ovgpu_multi_set_features: stable sort by descending track length, round-robin over the ranks, each rank's list ascending;
  * the exchange: Gram matrices iff the context is on OVGPU_COMPRESS_GRAM and NT = ceil((D + 1) / 16) <= 24 ("gram_wide" does not move it),
    triangles otherwise;
  * the merge of G triangles: 16 quads per register array up to 8 tile columns, 28 up to 14, 32 up to 16, 0 (k_qr_append) beyond; one launch
    behind the leaves (2) while NT <= 16 and G - 1 <= CUs and tsqr_no_pipeline is off, level by level (3) otherwise, none (0) for G = 1;
  * the Gram kernel of a rank with rows ("last_gram_kernel"): 5 k_gram_f32 on a gram_fp32 context, 4 k_gram_regions for an unprojected stack,
    3 k_gram_wide at exactly 23 tile columns, 2 k_gram_blk from 17, 1 the one-pass kernels;
  * the replicated factorisation: "chol_wide_factorisations" moves iff D > 256.
States come from synth.make_problem(C=, K=), D = 6 C + 14 K; tracks are cut with track_shapes' helpers; no batch holds more than 64 features.

A helper module, not a conftest: nothing here is collected.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import slam_shapes as ss
import track_shapes as ts
from open_vins_amd import capi, synth

GRAM, TSQR = capi.COMPRESS_GRAM, capi.COMPRESS_TSQR
GRAM_MAX_NT = 24        # the Gram exchange's last tile-column count (383 columns)
LOOP_MAX_RANKS = 8      # ranks of one loop-back communicator
MERGE_RESERVE = 16      # ovgpu_msckf_merge_update reserves max(G, 16) triangles
TREE_NONE, TREE_BEHIND, TREE_LEVELS = 0, 2, 3
GK_ONE_PASS, GK_BLK, GK_WIDE, GK_REGIONS, GK_F32 = 1, 2, 3, 4, 5
# against the oracle and against the single-context update alike
TOL_CHI2, TOL_THR, TOL_DX, TOL_P, TOL_POSE = 1e-8, 1e-12, 1e-8, 1e-9, 1e-9
TOL_DX_F32, TOL_P_F32 = 1e-4, 1e-3   # the fp32 twins' bounds of section 3 (chi2 as in float64)
MIN_GATE_MARGIN = 1e-6               # every verdict of the oracle stands this far (relative) from its threshold


# --------------------------------------------------------------------------- the rules, restated
def tiles(D):
    """tile columns of [H | r]: 16 columns each, the residual column included"""
    return (D + 1 + 15) // 16


def deal(lengths, G):
    """ovgpu_multi_set_features: the caller's feature indices each rank holds, in the rank's own (ascending) order"""
    order = sorted(range(len(lengths)), key=lambda f: -int(lengths[f]))  # (sorted is stable)
    return [sorted(order[g::G]) for g in range(G)]


def exchange_is_gram(route, D):
    return route == GRAM and tiles(D) <= GRAM_MAX_NT


def merge_qh(nt):
    return 16 if nt <= 8 else (28 if nt <= 14 else (32 if nt <= 16 else 0))


def tree_mode(nt, G, num_cu, no_pipeline=0):
    if G <= 1:
        return TREE_NONE
    return TREE_BEHIND if (not no_pipeline and nt <= 16 and G - 1 <= num_cu) else TREE_LEVELS


def gram_kernel(D, raw, fp32=0):
    nt = tiles(D)
    if fp32:
        return GK_F32
    if raw:
        return GK_REGIONS
    return GK_WIDE if nt == 23 else (GK_BLK if nt >= 17 else GK_ONE_PASS)


def chol_is_wide(D):
    return D > 256


def rank_kernel(m_max, gram, options=None):
    """"last_feature_kernel" of a rank whose longest track holds m_max observations: track_shapes.expected_kernel's tile budgets where the Gram
    matrices are exchanged (the fused kernels read the prior block's factor), the general kernel (0) where triangles are"""
    o = options or {}
    return ts.expected_kernel(m_max, o.get("feature_kernel_shape", 0), bool(o.get("no_fast_feature_kernel", 0))) if gram else 0


def rank_raw(D, kernel, gram, options=None):
    """"last_stack_raw" of that rank: DESIGN.md section 4.3's rule (track_shapes.expected_raw) on the Gram exchange, never on the other"""
    return ts.expected_raw(D, kernel, 0, (options or {}).get("gram_fp32", 0)) if gram else 0


# --------------------------------------------------------------------------- states: D -> C, K and, written out, LD and the tile columns
#        D     C   K   LD   NT
STATES = {
    68:  (9,  1, 69,  5),    # the smallest state whose tracks triangulate (44 columns, five clones of one camera 0.4 s apart, give the oracle no feature)
    122: (18, 1, 123, 8),    # the last count on 16 merge quads
    128: (19, 1, 129, 9),    # the first on 28
    208: (30, 2, 209, 14),   # the last on 28; configs[1]'s state
    222: (30, 3, 223, 14),   # the last column count of that tile
    224: (35, 1, 225, 15),   # the first on 32 merge quads
    250: (37, 2, 251, 16),   # the last one-launch tree, the last one-pass Gram kernel
    256: (38, 2, 257, 17),   # k_qr_append level by level, k_gram_blk, the last k_chol_fused
    262: (39, 2, 263, 17),   # chol_wide
    352: (54, 2, 353, 23),   # k_gram_wide
    382: (59, 2, 383, 24),   # the last Gram exchange
    384: (57, 3, 385, 25),   # triangles on a Gram context
}
MORE_RANKS_AT = (128, 250, 256, 382)   # G = 4, 5 and 8
EMPTY_AT = (208, 256, 382)             # group (b)
# (c) two states off the table, for ranks that differ in kind
LONG_STATE = ts.LARGE                                   # D = 360, 23 tile columns: tracks of up to 240 observations
RAW_STATE = dict(C=35, K=4, pose=1, intr=0)             # D = 234, 15 tile columns: tracks of up to 140 observations


def state_of(D):
    C, K, _, _ = STATES[D]
    return dict(C=C, K=K)


# --------------------------------------------------------------------------- batches
# Track lengths in the caller's order: no two neighbours alike and nothing sorted, so that the deal really permutes.  A track is cut to the length
# listed or, where the window gives it fewer observations (five clones of one camera), kept whole; every cut keeps the widest baseline ("stride").
LENGTHS = (9, 33, 5, 17, 40, 8, 25, 16, 12, 6, 21, 29, 7, 36, 11, 19, 38, 10, 27, 14, 13, 4, 23, 31)


def cut(prob, lengths):
    m = np.diff(prob.meas_offsets)
    return ts.with_lengths(prob, [min(int(m[f]), int(lengths[f % len(lengths)])) for f in range(prob.F)], patterns=("stride",))


def plant(prob, outliers, seed):
    for f in outliers:
        m = int(prob.meas_offsets[f + 1] - prob.meas_offsets[f])
        prob = ts.make_outlier(prob, f, 10.0 if m < 10 else 15.0, seed)
    return prob


def batch(state, F, seed, outliers=(), lengths=LENGTHS, fisheye=False):
    """F tracks of the window of `state` cut to `lengths`, the features `outliers` gross outliers"""
    if fisheye:
        p = ts.longest(synth.make_problem(2, C=state["C"], K=state["K"], F=4 * F, seed=seed, fisheye=True), F)
    else:
        p = ts._window(state, F, seed)
    return plant(cut(p, lengths), outliers, seed)


def shard_problem(prob, ids):
    return prob.subset(np.asarray(ids, dtype=np.int64))


def shard_triangulation(prob, tri, ids):
    """the oracle's triangulation of the features `ids`, anchors re-based to the shard's own measurement offsets"""
    ids = np.asarray(ids, dtype=np.int64)
    sub = shard_problem(prob, ids)
    anchor = tri["anchor_meas"][ids] - prob.meas_offsets[ids] + sub.meas_offsets[:-1]
    return dict(p_FinG=tri["p_FinG"][ids], p_FinA=tri["p_FinA"][ids], anchor_meas=anchor.astype(np.int32), status=tri["status"][ids])


@dataclass
class Case:
    id: str
    group: str
    state: dict
    build: object                        # () -> Problem
    G: int
    route: int = GRAM                    # the context's compress_route
    options: dict = field(default_factory=dict)
    debug: dict = field(default_factory=dict)      # ovgpu_debug_option settings of every rank, before the upload
    rejected: tuple = ()                 # the features the gate must reject, and no others
    shards: tuple | None = None          # features per rank, written out
    empty: tuple = ()                    # ranks without a feature
    rowless: tuple = ()                  # ranks with features and no accepted row
    tol_dx: float = TOL_DX
    tol_p: float = TOL_P

    @property
    def D(self):
        s = self.state
        return ts.n_columns(s["C"], s["K"], s.get("pose", 1), s.get("intr", 1))

    @property
    def gram(self):
        return exchange_is_gram(self.route, self.D)

    def opts(self, **more):
        s = self.state
        kw = dict(chi2_multipler=1.0, gate_always_factor=1, do_calib_camera_pose=s.get("pose", 1), do_calib_camera_intrinsics=s.get("intr", 1),
                  compress_route=self.route)
        kw.update(self.options)
        kw.update(more)
        return capi.default_options(**kw)

    @functools.cached_property
    def prob(self):
        return self.build()

    @property
    def lengths(self):
        return np.diff(self.prob.meas_offsets)

    @property
    def deal(self):
        return deal(self.lengths, self.G)

    def rank_m_max(self, g):
        ids = self.deal[g]
        return int(self.lengths[ids].max()) if ids else 0

    def rank_kernel(self, g):
        return rank_kernel(self.rank_m_max(g), self.gram, self.options)

    def rank_raw(self, g):
        return rank_raw(self.D, self.rank_kernel(g), self.gram, self.options)

    def rank_gram_kernel(self, g):
        return gram_kernel(self.D, self.rank_raw(g), self.options.get("gram_fp32", 0)) if self.gram else 0

    @property
    def expected_rejected(self):
        """the planted outliers; "rank 1": every feature the deal hands to rank 1"""
        return tuple(self.deal[1]) if self.rejected == "rank 1" else tuple(self.rejected)

    @property
    def problem_key(self):
        """cases with the same key share one batch and one oracle run"""
        return getattr(self.build, "key", self.id)


def _keyed(key, fn, *a, **kw):
    f = functools.lru_cache(maxsize=None)(functools.partial(fn, *a, **kw))
    f.key = key
    return f


# seeds: chosen on the CPU (tests/test_shard_shapes_cpu.py holds every case to it) so that the oracle uses and rejects exactly the planted features
# and leaves no statistic within MIN_GATE_MARGIN of its threshold.  The default serves all but the ones listed.
SEEDS = {"D68-F6-0": 949, "D68-F4-1": 914, "D128-F40-3.17": 1005, "c-long": 961, "c-raw": 960}
SMALLEST = 68


def seed_of(key, default):
    return SEEDS.get(key, default)


@functools.lru_cache(maxsize=None)
def table_batch(D, F, outliers=(3,)):
    key = f"D{D}-F{F}-{'.'.join(map(str, outliers))}"
    return _keyed(key, batch, state_of(D), F, seed_of(key, 900 + D + F), outliers)


def small_outlier(F):
    return (0,) if F == 6 else (1,)


def shards_of(F, G):
    """features per rank of a round-robin deal"""
    return tuple(len(range(g, F, G)) for g in range(G))


def _a_cases():
    out = []
    for D in STATES:
        plan = [(2, 12), (3, 4)]                     # F = 12 on two ranks; F = G + 1 = 4 on three: shards of 2, 1 and 1
        if D == SMALLEST:
            plan = [(2, 6), (3, 4)]                  # (nine clones of one camera: six tracks of which the oracle uses five)
        if D in MORE_RANKS_AT:
            plan += [(4, 12), (5, 6), (8, 12)]       # F = G + 1 = 6 on five; twelve on eight: four ranks hold two, four hold one
        for G, F in plan:
            outl = small_outlier(F) if D == SMALLEST else ((3,) if F >= 6 else (1,))
            for route, name in ((GRAM, "gram"), (TSQR, "tsqr")):
                out.append(Case(f"a-{D}-G{G}-{name}", "a", state_of(D), table_batch(D, F, outl), G, route, rejected=outl, shards=shards_of(F, G)))
        if D == 384:  # ... and the triangle exchange of a Gram context with "gram_wide" in force
            out.append(Case("a-384-G2-gram-wide1", "a", state_of(D), table_batch(D, 12, (3,)), 2, GRAM, debug=dict(gram_wide=1), rejected=(3,), shards=(6, 6)))
    return out


LONG_LENGTHS = (17, 33, 21, 25, 40, 16)   # (a gross offset on a track of a handful of observations is not always rejected)


def none_batch(D, seed):
    return batch(state_of(D), 4, seed, (0, 1, 2, 3), LONG_LENGTHS)


def rank_rejected_batch(D, seed):
    """six features on two ranks, every feature of rank 1 a gross outlier"""
    p = cut(ts._window(state_of(D), 6, seed), LONG_LENGTHS)
    return plant(p, deal(np.diff(p.meas_offsets), 2)[1], seed)


def _b_cases():
    out = []
    for D in EMPTY_AT:
        for route, name in ((GRAM, "gram"), (TSQR, "tsqr")):
            st = state_of(D)
            out.append(Case(f"b-{D}-F1-G4-{name}", "b", st, table_batch(D, 1, ()), 4, route, shards=(1, 0, 0, 0), empty=(1, 2, 3)))
            out.append(Case(f"b-{D}-F2-G3-{name}", "b", st, table_batch(D, 2, ()), 3, route, shards=(1, 1, 0), empty=(2,)))
            key = f"D{D}-rank-rejected"
            b = _keyed(key, rank_rejected_batch, D, seed_of(key, 950 + D))
            out.append(Case(f"b-{D}-rank-rejected-{name}", "b", st, b, 2, route, rejected="rank 1", shards=(3, 3), rowless=(1,)))
            key = f"D{D}-none"
            b = _keyed(key, none_batch, D, seed_of(key, 970 + D))
            out.append(Case(f"b-{D}-none-{name}", "b", st, b, 2, route, rejected=(0, 1, 2, 3), shards=(2, 2), rowless=(0, 1)))
    return out


LONG_TRACK = 233                           # one observation more than the block-row kernel holds
RAW_TRACK = 127                            # ... and than the one-pass kernels hold
C_LENGTHS = (9, 33, 5, 17, 40, 8, 25, 16)


def long_batch(state, m_long, seed):
    """eight tracks, the third `m_long` observations long (stable sort: it is dealt first, to rank 0), the sixth a gross outlier"""
    lens = list(C_LENGTHS)
    lens[2] = m_long
    return plant(ts.with_lengths(ts._window(state, 8, seed), lens, patterns=("stride",)), (5,), seed)


def _c_cases():
    sm = state_of(208)
    mk = lambda key, fn, *a, **kw: _keyed(key, fn, *a, **kw)  # noqa: E731
    return [
        Case("c-long-track", "c", LONG_STATE, mk("c-long", long_batch, LONG_STATE, LONG_TRACK, seed_of("c-long", 960)), 2, rejected=(5,), shards=(4, 4)),
        Case("c-raw-and-projected", "c", RAW_STATE, mk("c-raw", long_batch, RAW_STATE, RAW_TRACK, seed_of("c-raw", 961)), 2, rejected=(5,), shards=(4, 4)),
        Case("c-fp32", "c", sm, table_batch(208, 12, (3,)), 2, options=dict(gram_fp32=1), rejected=(3,), shards=(6, 6), tol_dx=TOL_DX_F32, tol_p=TOL_P_F32),
        Case("c-anchored", "c", sm, table_batch(208, 12, (3,)), 2, options=dict(feat_rep_msckf=capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH), rejected=(3,),
             shards=(6, 6)),
        Case("c-fisheye", "c", sm, mk("c-fisheye", batch, sm, 12, seed_of("c-fisheye", 962), (3,), LENGTHS, True), 2, rejected=(3,), shards=(6, 6)),
    ]


CASES = _a_cases() + _b_cases() + _c_cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# (d) the life cycle of one set of four ranks: (D, F, outliers); the Householder set runs the first three
LIFE = [(208, 40, (3, 17)), (208, 2, ()), (128, 40, (3, 17)), (384, 20, (3,))]


def life_case(k, route):
    D, F, outl = LIFE[k]
    return Case(f"d-frame{k}-{'gram' if route == GRAM else 'tsqr'}", "d", state_of(D), table_batch(D, F, outl), 4, route, rejected=outl, shards=shards_of(F, 4),
                empty=(2, 3) if F == 2 else ())


FALLS_EMPTY_AT = (250, 256)   # ... and the second frame again where the leaf and Gram kernels are others: k_qr_node | k_qr_append, one-pass | k_gram_blk


def falls_empty_case(D, route):
    return Case(f"d-{D}-F2-{'gram' if route == GRAM else 'tsqr'}", "d", state_of(D), table_batch(D, 2, ()), 4, route, shards=(1, 1, 0, 0), empty=(2, 3))


# (e) building blocks on separate contexts
MERGE_G = (1, 2, 3, 5, 16, 17)             # 16 | 17: the reserve of max(G, 16) triangles
MERGE_D = (128, 256)
MERGE_REAL = 3                             # real shards at most; the triangles beyond are zero triangles
LOCAL_GRAM_D = (SMALLEST, 250, 256, 352, 382)
# (f) the native entry in a world of one
WORLD_OF_ONE_D = (SMALLEST, 256, 262, 382, 384)


def block_case(D, route=GRAM):
    F, outl = (6, small_outlier(6)) if D == SMALLEST else (12, (3,))
    return Case(f"e-{D}", "e", state_of(D), table_batch(D, F, outl), 1, route, rejected=outl)


# (g) a prior block that does not factor (slam_shapes.semi_definite: the builder behind gram_wide_shapes' gram_route = False)
def semi_definite_case(G, route=GRAM):
    b = _keyed("g-semi-definite", lambda: ss.semi_definite(table_batch(208, 12, (3,))()))
    return Case(f"g-semi-definite-G{G}", "g", state_of(208), b, G, route, rejected=None)


# --------------------------------------------------------------------------- the oracle
_ORACLE = {}


def oracle_run(oracle, case):
    """(triangulation, update) of the oracle for a case's batch under the case's filter options: computed once per batch and option set, shared,
    left unchanged.  (The route and the rank count are the device's business: the oracle has neither.)"""
    key = (case.problem_key, tuple(sorted((k, v) for k, v in case.options.items() if k in ("feat_rep_msckf",))), tuple(sorted(case.state.items())))
    if key not in _ORACLE:
        v = capi.Views(case.prob)
        opts = case.opts()
        tri = oracle.triangulate(opts, v)
        _ORACLE[key] = (tri, oracle.msckf_update(opts, v, want_compressed=False, given=tri))
    return _ORACLE[key]


def sharded_oracle(oracle, case, tri, shards=None):
    """the update from the per-shard oracle compressions: every shard's compressed (H, r), stacked, compressed once more, one EKF update"""
    prob, opts = case.prob, case.opts()
    Hs, rs, n_used, n_rows = [], [], 0, 0
    for ids in (case.deal if shards is None else shards):
        if not len(ids):
            continue
        sub = shard_problem(prob, ids)
        loc = oracle.msckf_update(opts, capi.Views(sub), want_compressed=True, given=shard_triangulation(prob, tri, ids))
        n_used += loc["stats"]["n_used"]
        n_rows += loc["stats"]["n_rows"]
        if loc["rows_comp"] > 0:
            Hs.append(loc["H_comp"]), rs.append(loc["r_comp"])
    if not Hs:
        return dict(dx=np.zeros(prob.N), P=prob.P.copy(), n_used=n_used, n_rows=n_rows)
    H, r = oracle.measurement_compress(np.vstack(Hs), np.concatenate(rs))
    cols = oracle.column_map(opts, capi.Views(prob))
    st, P, dx = oracle.ekf_update(prob.P, H, r, cols, float(opts.sigma_pix) ** 2)
    assert st == 0
    return dict(dx=dx, P=P, n_used=n_used, n_rows=n_rows)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))
