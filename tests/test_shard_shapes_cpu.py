"""The batches of tests/test_gpu_shard_edges.py on the oracle and numpy alone (no GPU): every one must hold what it is named for BEFORE it travels —
the column, LD and tile counts written next to its state, the shard sizes the restated deal gives (empty ranks, the rank whose features are all
rejected, the long track on rank 0 only), exactly the planted features rejected with every verdict at least shard_shapes.MIN_GATE_MARGIN from its
threshold, features that differ pairwise in chi2 — and the sharding invariance the device test rests on: the update from the per-shard oracle
compressions, stacked and compressed once more, is the unsharded oracle update.  The worst difference of that comparison is the FLOOR the device
tolerances are read against; test_zz_floors prints it per group (DESIGN.md section 7 quotes it).  Also the restated rules against written-out
tables, one row per edge."""
import numpy as np
import pytest

import shard_shapes as sh
from open_vins_amd import capi

G_, T_ = sh.GRAM, sh.TSQR
FLOOR = {}  # group -> [dx, P]
# the floor must leave the device bounds meaningful: a tenth of them at the most
FLOOR_DX, FLOOR_P = sh.TOL_DX / 10, sh.TOL_P / 10


def test_every_state_is_what_is_written_next_to_it():
    assert sorted(sh.STATES) == [68, 122, 128, 208, 222, 224, 250, 256, 262, 352, 382, 384]
    for D, (C, K, LD, NT) in sh.STATES.items():
        assert D == 6 * C + 14 * K == sh.ts.n_columns(C, K) and LD == D + 1 and NT == -(-LD // 16) == sh.tiles(D), D
    # one row per edge: D -> (tile columns, merge quads, tree of G = 2 on 256 CUs, Gram exchange on a Gram context, Gram kernel of a projected
    # stack, wide factorisation)
    table = {68: (5, 16, 2, True, 1, False), 122: (8, 16, 2, True, 1, False), 128: (9, 28, 2, True, 1, False), 208: (14, 28, 2, True, 1, False),
             222: (14, 28, 2, True, 1, False), 224: (15, 32, 2, True, 1, False), 250: (16, 32, 2, True, 1, False), 256: (17, 0, 3, True, 2, False),
             262: (17, 0, 3, True, 2, True), 352: (23, 0, 3, True, 3, True), 382: (24, 0, 3, True, 2, True), 384: (25, 0, 3, False, 2, True)}
    assert sorted(table) == sorted(sh.STATES)
    for D, want in table.items():
        nt = sh.tiles(D)
        got = (nt, sh.merge_qh(nt), sh.tree_mode(nt, 2, 256), sh.exchange_is_gram(G_, D), sh.gram_kernel(D, 0), sh.chol_is_wide(D))
        assert got == want, (D, got)
        assert not sh.exchange_is_gram(T_, D)
    assert sh.ts.n_columns(**sh.LONG_STATE) == 360 and sh.tiles(360) == 23
    assert sh.ts.n_columns(**sh.RAW_STATE) == 234 and sh.tiles(234) == 15


def test_the_rules_at_their_edges():
    assert [sh.merge_qh(nt) for nt in (1, 8, 9, 14, 15, 16, 17, 25)] == [16, 16, 28, 28, 32, 32, 0, 0]
    # the tree: none for one rank, one launch behind the leaves up to 16 tile columns and G - 1 <= CUs, level by level otherwise
    assert [sh.tree_mode(16, G, 256) for G in (1, 2, 8, 257, 258)] == [0, 2, 2, 2, 3]
    assert sh.tree_mode(17, 2, 256) == 3 and sh.tree_mode(16, 3, 256, no_pipeline=1) == 3 and sh.tree_mode(16, 17, 16) == 2 and sh.tree_mode(16, 18, 16) == 3
    # the exchange: 383 columns are the last (382 the last an MSCKF state reaches), whatever "gram_wide" says; a Householder context never
    assert [sh.exchange_is_gram(G_, D) for D in (382, 383, 384)] == [True, True, False] and not sh.exchange_is_gram(T_, 68)
    # the Gram kernel: fp32 first, then the unprojected stack, then the width
    assert [sh.gram_kernel(D, 0) for D in (254, 255, 256, 351, 352, 367, 368, 383)] == [1, 1, 2, 2, 3, 3, 2, 2]
    assert sh.gram_kernel(208, 1) == 4 and sh.gram_kernel(208, 1, fp32=1) == 5 and sh.gram_kernel(352, 0, fp32=1) == 5
    assert [sh.chol_is_wide(D) for D in (255, 256, 257)] == [False, False, True]
    # the per-rank kernel and stack: the fused kernels on the Gram exchange only, the unprojected stack for 6 .. 15 tile columns under a one-pass kernel
    assert [sh.rank_kernel(m, True) for m in (1, 2, 62, 63, 126, 127, 232, 233)] == [0, 1, 1, 2, 2, 3, 3, 0] and sh.rank_kernel(40, False) == 0
    assert [sh.rank_raw(D, 1, True) for D in (68, 78, 80, 208, 238, 240, 250)] == [0, 0, 1, 1, 1, 0, 0]
    assert sh.rank_raw(208, 3, True) == 0 and sh.rank_raw(208, 0, True) == 0 and sh.rank_raw(208, 1, False) == 0 and sh.rank_raw(208, 1, True, dict(gram_fp32=1)) == 0


def test_the_deal():
    """stable by descending length, round-robin, ascending per rank"""
    assert sh.deal([5, 9, 9, 2, 7], 2) == [[1, 3, 4], [0, 2]]        # order 1 2 4 0 3
    assert sh.deal([5, 9, 9, 2, 7], 3) == [[0, 1], [2, 3], [4]]
    assert sh.deal([4, 4, 4, 4], 2) == [[0, 2], [1, 3]]              # ties keep the caller's order
    assert sh.deal([3], 4) == [[0], [], [], []] and sh.deal([], 2) == [[], []]
    assert sh.deal([1, 2, 3, 4, 5, 6, 7, 8], 8) == [[7 - g] for g in range(8)]
    assert sh.shards_of(12, 8) == (2, 2, 2, 2, 1, 1, 1, 1) and sh.shards_of(6, 5) == (2, 1, 1, 1, 1) and sh.shards_of(4, 3) == (2, 1, 1)


def test_the_catalogue_covers_what_it_claims():
    ids = set(sh.BY_ID)
    for D in sh.STATES:
        for G in (2, 3) + ((4, 5, 8) if D in sh.MORE_RANKS_AT else ()):
            assert {f"a-{D}-G{G}-gram", f"a-{D}-G{G}-tsqr"} <= ids
    assert sh.MORE_RANKS_AT == (128, 250, 256, 382) and "a-384-G2-gram-wide1" in ids
    for D in (208, 256, 382):
        for name in ("gram", "tsqr"):
            assert {f"b-{D}-F1-G4-{name}", f"b-{D}-F2-G3-{name}", f"b-{D}-rank-rejected-{name}", f"b-{D}-none-{name}"} <= ids
    assert {"c-long-track", "c-raw-and-projected", "c-fp32", "c-anchored", "c-fisheye"} <= ids
    assert [(D, F) for D, F, _ in sh.LIFE] == [(208, 40), (208, 2), (128, 40), (384, 20)]
    assert sh.MERGE_G == (1, 2, 3, 5, 16, 17) and sh.MERGE_D == (128, 256) and sh.MERGE_RESERVE == 16
    assert sh.LOCAL_GRAM_D == (68, 250, 256, 352, 382) and sh.WORLD_OF_ONE_D == (68, 256, 262, 382, 384)
    for c in sh.CASES:
        assert (c.G > sh.LOOP_MAX_RANKS) is False and c.gram == (c.route == G_ and c.D <= 383)


def _all_cases():
    return list(sh.CASES) + [sh.life_case(k, G_) for k in range(len(sh.LIFE))] + [sh.falls_empty_case(D, G_) for D in sh.FALLS_EMPTY_AT] + [sh.block_case(D) for D in sorted(set(sh.MERGE_D + sh.LOCAL_GRAM_D + sh.WORLD_OF_ONE_D))]


ALL = {c.id: c for c in _all_cases()}


@pytest.mark.parametrize("cid", list(ALL))
def test_case_is_not_vacuous(oracle, cid):
    case = ALL[cid]
    prob, m = case.prob, case.lengths
    assert prob.F <= 64 and m.max() <= (40 if case.id not in ("c-long-track", "c-raw-and-projected") else 233)
    assert case.D == sh.ts.n_columns(prob.C, prob.K, case.state.get("pose", 1), case.state.get("intr", 1))
    # 1. the shards the restated deal gives are the ones the case names
    shards = case.deal
    assert sorted(f for ids in shards for f in ids) == list(range(prob.F))
    if case.shards is not None:
        assert tuple(len(ids) for ids in shards) == case.shards
    assert tuple(g for g in range(case.G) if not shards[g]) == tuple(case.empty)
    # 2. exactly the planted features are rejected, every other one is used, no verdict near its threshold
    tri, ref = sh.oracle_run(oracle, case)
    st, chi2, thr = ref["feat_status"], ref["chi2"], ref["chi2_thresh"]
    want = np.zeros(prob.F, bool)
    want[list(case.expected_rejected)] = True
    assert ref["stats"]["status"] == 0 and ref["stats"]["D"] == case.D
    assert np.array_equal(st == capi.FEAT_CHI2_REJECTED, want) and np.array_equal(st == capi.FEAT_USED, ~want), st
    gate = np.isfinite(chi2)
    assert gate.all() and np.abs(chi2 / thr - 1.0).min() >= sh.MIN_GATE_MARGIN
    if case.group != "b" and case.rejected:  # (group (b) and the life cycle's two-feature frame say otherwise)
        assert want.any() and (~want).any()
    # 3. ... and the ranks that must contribute nothing do
    for g in range(case.G):
        used = int((st[shards[g]] == capi.FEAT_USED).sum()) if shards[g] else 0
        if case.group == "b":
            assert (used == 0) == (g in case.empty or g in case.rowless), (g, used)
        else:  # (a rank of group (a) that holds the outlier alone has no row either: F = G + 1, twelve features on eight ranks)
            assert used > 0 or len(shards[g]) <= 1, (g, used)
    if case.id.endswith(("none-gram", "none-tsqr")):
        assert ref["stats"]["n_used"] == 0 and not ref["dx"].any() and np.array_equal(ref["P"], prob.P)
    # 4. a permuted feat_of cannot pass: the statistics differ pairwise
    if prob.F > 1:
        sep = np.abs(chi2[:, None] / chi2[None, :] - 1.0) + np.eye(prob.F)
        assert sep.min() > 1e-4
    # 5. the kinds of ranks group (c) is named for
    if case.id == "c-long-track":
        assert m[2] == sh.LONG_TRACK and 2 in shards[0] and case.rank_kernel(0) == 0 and case.rank_kernel(1) == 1 and st[2] == capi.FEAT_USED
        assert max(m[shards[1]]) <= 40
    if case.id == "c-raw-and-projected":
        assert m[2] == sh.RAW_TRACK and 2 in shards[0] and (case.rank_kernel(0), case.rank_raw(0)) == (3, 0) and (case.rank_kernel(1), case.rank_raw(1)) == (1, 1)
        assert (case.rank_gram_kernel(0), case.rank_gram_kernel(1)) == (sh.GK_ONE_PASS, sh.GK_REGIONS)
    if case.id == "c-fisheye":
        assert prob.cam_is_fisheye.all()


def test_the_prior_that_does_not_factor(oracle):
    """group (g): the two newest clones perfectly correlated — six eigenvalues at zero, which the oracle's update (S = H P H^T + R) does not mind"""
    case, plain = sh.semi_definite_case(2), sh.BY_ID["a-208-G2-gram"]
    w, w0 = np.linalg.eigvalsh(case.prob.P), np.linalg.eigvalsh(plain.prob.P)
    assert w[:6].max() < 1e-12 * w[-1] and w0[0] > 0 and case.D == 208
    with pytest.raises(np.linalg.LinAlgError):
        cols = oracle.column_map(case.opts(), capi.Views(case.prob))
        np.linalg.cholesky(case.prob.P[np.ix_(cols, cols)])
    tri, ref = sh.oracle_run(oracle, case)
    st, chi2, thr = ref["feat_status"], ref["chi2"], ref["chi2_thresh"]
    assert ref["stats"]["status"] == 0 and ref["stats"]["n_used"] >= 5 and set(st) <= {capi.FEAT_USED, capi.FEAT_CHI2_REJECTED}
    assert np.abs(chi2 / thr - 1.0).min() >= sh.MIN_GATE_MARGIN
    assert tuple(len(ids) for ids in case.deal) == (6, 6)


@pytest.mark.parametrize("cid", [c.id for c in sh.CASES if c.route == G_ and not c.debug] + [sh.life_case(k, G_).id for k in range(len(sh.LIFE))])
def test_sharding_invariance_on_the_oracle(oracle, cid):
    """per-shard oracle compressions -> stacked -> compressed once more -> one EKF update == the unsharded oracle update"""
    case = ALL[cid]
    tri, ref = sh.oracle_run(oracle, case)
    s = sh.sharded_oracle(oracle, case, tri)
    assert s["n_used"] == ref["stats"]["n_used"] and s["n_rows"] == ref["stats"]["n_rows"]
    if ref["stats"]["n_used"] == 0:
        assert not s["dx"].any() and np.array_equal(s["P"], ref["P"])
        return
    ddx, dP = sh.rel(s["dx"], ref["dx"]), sh.rel(s["P"], ref["P"])
    w = FLOOR.setdefault(case.group, [0.0, 0.0])
    w[0], w[1] = max(w[0], ddx), max(w[1], dP)
    print(f"{cid}: sharded oracle against the oracle  dx {ddx:.3e}  P {dP:.3e}")
    assert ddx < FLOOR_DX and dP < FLOOR_P


def test_zz_floors():
    for grp, (ddx, dP) in sorted(FLOOR.items()):
        print(f"floor ({grp}): dx {ddx:.3e}  P {dP:.3e}")
        assert 5 * ddx < sh.TOL_DX and 5 * dP < sh.TOL_P  # no state's bound has to give way to the reference's own error
