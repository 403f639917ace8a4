"""The systems of tests/test_gpu_tsqr_edges.py on numpy alone (no GPU): every one of them must be what it is named for BEFORE it travels — the
tile count, kernel family, leaf count, last-leaf and last-block rows and merge mode written next to it, both sides of every edge present, the rank
a degenerate input claims, and a reference error (LAPACK's Householder QR under the metric of tsqr_shapes.metric) far enough under the project's
1e-12 cap that the cap never binds because of the input."""
import numpy as np
import pytest

import tsqr_shapes as ts


def test_every_case_is_what_is_written_next_to_it():
    cases = ts.cases(256)
    assert [c.id for c in cases] == ts.CASE_IDS == list(ts.EXPECT_256)
    for c in cases:
        assert c.dispatch(256).astuple() == ts.EXPECT_256[c.id], c.id
        assert c.rows > c.cols and 1 <= c.cols <= 511


def test_the_rule_by_hand():
    """The rule against values worked by hand from the documented thresholds (not from dispatch())."""
    nt = {c: ts.n_tiles(c) for c in ts.A_COLS}
    assert nt == {1: 1, 2: 1, 14: 1, 15: 1, 16: 2, 17: 2, 126: 8, 127: 8, 128: 9, 222: 14, 223: 14, 224: 15, 238: 15, 239: 15, 240: 16, 254: 16,
                  255: 16, 256: 17, 510: 32, 511: 32}
    for t in range(1, 33):
        assert ts.leaf_kernel(t) == (0 if t <= 15 else 1 if t == 16 else 2)
        assert ts.merge_qh(t) == (16 if t <= 8 else 28 if t <= 14 else 32 if t <= 16 else 0)
    # rows per leaf: whole 128-row appends; 128 only while the stack holds at most 256 rows
    assert ts.configure(41, 1, 256) == (128, 1) and ts.configure(129, 256, 256) == (128, 2) and ts.configure(256, 2, 256) == (128, 2)
    assert ts.configure(257, 256, 256) == (256, 2) and ts.configure(257, 1, 256) == (384, 1) and ts.configure(767, 2, 256) == (384, 2)
    assert ts.configure(33025, 0, 256) == (256, 130) and ts.configure(65793, 258, 256) == (256, 258) and ts.configure(100000, 0, 256) == (512, 196)
    assert ts.configure(100000, 0, 304) == (384, 261)
    # merge mode
    assert ts.tree_mode(2, 1, 256) == 0 and ts.tree_mode(2, 128, 256) == 1 and ts.tree_mode(2, 129, 256) == 2
    assert ts.tree_mode(2, 257, 256) == 2 and ts.tree_mode(2, 258, 256) == 3
    assert ts.tree_mode(15, 5, 256) == 1 and ts.tree_mode(16, 5, 256) == 2 and ts.tree_mode(16, 5, 256, overlap=1) == 2 and ts.tree_mode(17, 5, 256) == 3
    assert ts.tree_mode(2, 3, 256, overlap=2) == 2 and ts.tree_mode(2, 200, 256, overlap=1) == 1 and ts.tree_mode(2, 3, 256, no_pipeline=1) == 3
    assert ts.tree_mode(2, 3, 256, no_pipeline=1, overlap=1) == 3
    for cu in (64, 256, 304):
        e = ts.edge_leaves(cu)
        assert [ts.tree_mode(2, e[k], cu) for k in ts.C_EDGE_IDS] == [1, 2, 2, 3]
        for cid, W in e.items():
            c = ts.case(cid, cu)
            assert c.dispatch(cu).W == W and c.dispatch(cu).last_leaf == 1


def test_both_sides_of_every_edge_are_present():
    D = {c.id: c.dispatch(256) for c in ts.cases(256)}
    a = [d for i, d in D.items() if i.startswith("a-")]
    for lo, hi in ts.NT_EDGES:  # column tiles, with one leaf and with a merge on either side
        for merged in (False, True):
            assert {lo, hi} <= {d.NT for d in a if (d.W > 1) == merged}, (lo, hi, merged)
    assert {d.NT for d in a} >= {1, 2, 8, 9, 14, 15, 16, 17, 32}
    assert {(d.leaf, d.qh) for d in D.values()} == {(0, 0), (0, 16), (0, 28), (0, 32), (1, 0), (1, 32), (2, 0)}
    b = {i: d for i, d in D.items() if i.startswith("b-")}
    for cols, leaf in ((40, 0), (230, 0), (250, 1)):  # 128-row leaves: a last leaf of exactly 1, 127 and 128 rows, a last append of 1 and 127 rows in a longer leaf
        mine = [d for i, d in b.items() if i.startswith(f"b-{cols}-")]
        assert {d.leaf for d in mine} == {leaf}
        assert {1, 127, 128} <= {d.last_leaf for d in mine if d.W > 1}
        assert {1, 127} <= {d.last_block for d in mine if d.last_leaf > 128}
        assert {cols + 1, cols + 2} <= {c.rows for c in ts.cases(256) if c.id.startswith(f"b-{cols}-")}
        # both arms of the short-leaf special case: 128-row leaves at 128 < rows <= 256, 256-row leaves just over
        assert any(d.rpn == 128 and d.W == 2 for d in mine) and D[f"b-{cols}-257-w0"].rpn == 256
    b32 = [d for i, d in D.items() if i.startswith("b32-")]
    assert {d.leaf for d in b32} == {2}
    for W in (1, 2):  # 32-row blocks: a last block of 1, 31 and 32 rows with one and with two leaves
        assert {1, 31, 32} <= {d.last_block for d in b32 if d.W == W}
    got = {k: D[k] for k in ts.C_EDGE_IDS}
    assert [got[k].W for k in ts.C_EDGE_IDS] == [128, 129, 257, 258] and [got[k].tree for k in ts.C_EDGE_IDS] == [1, 2, 2, 3]
    assert [D[f"c-W{W}"].W for W in ts.C_W] == ts.C_W
    assert [D[i].tree for i in ts.VARIANT_SETS["W3"]] == [1, 3, 1, 2] and [D[i].tree for i in ts.VARIANT_SETS["W9"]] == [1, 3, 1, 2]
    assert [D[i].tree for i in ts.VARIANT_SETS["238"]] == [1, 1, 2] and [D[i].tree for i in ts.VARIANT_SETS["240"]] == [2, 2, 2]
    assert [D[i].NT for i in ("c-238-W5", "c-240-W5")] == [15, 16]
    for ids in ts.VARIANT_SETS.values():  # variants share one input
        assert len({id(ts.make_input(ts.case(i))[0]) for i in ids}) == 1
    assert sorted({(d.leaf) for i, d in D.items() if i.startswith("d-")}) == [0, 1, 2]
    assert D["d-250-zero_append"].W == 1 and D["d-250-zero_append"].last_leaf == 450 and D["d-300-zero_append"].W == 1
    # a whole zero append with non-zero rows behind it in ONE leaf, in every leaf family (240 rows at 40 columns end inside the zeroed append)
    assert [(D[i].leaf, D[i].W, D[i].last_leaf > 256) for i in ("d-40-zero_append-385", "d-250-zero_append", "d-300-zero_append")] == [(0, 1, True), (1, 1, True), (2, 1, True)]


@pytest.mark.parametrize("cid", [i for i in ts.CASE_IDS if i.startswith("d-")])
def test_degenerate_inputs_have_the_rank_they_claim(cid):
    c = ts.case(cid)
    H, r = ts.make_input(c)
    Hn = H / np.where(np.linalg.norm(H, axis=0) == 0, 1.0, np.linalg.norm(H, axis=0))
    sv = np.linalg.svd(Hn, compute_uv=False)
    rank = int((sv > 1e-10 * max(sv[0], 1e-300)).sum())
    assert rank == ts.claimed_rank(c)
    for k in c.zero_cols:
        assert not H[:, k].any()
    v = c.variant
    assert (not r.any()) == (v == "rzero")
    if v == "Hzero":
        assert not H.any() and r.any()
    if v == "dup_tile":
        assert np.array_equal(H[:, 3], H[:, 7]) and 3 // 16 == 7 // 16
    if v == "dup_tiles":
        assert np.array_equal(H[:, 3], H[:, 20]) and 3 // 16 != 20 // 16
    if v == "zero_append":
        assert not H[128:256].any() and not r[128:256].any() and H[:128].all() and c.workers == 1


@pytest.mark.parametrize("cid", ts.CASE_IDS)
def test_reference_error_is_finite_and_far_under_the_cap(cid):
    """16 e_ref < 1e-12: the bound max(16 e_ref, 256 eps) of the GPU test is never cut by the 1e-12 cap because of the input."""
    c = ts.case(cid)
    H, r = ts.make_input(c)
    assert H.shape == (c.rows, c.cols) and r.shape == (c.rows,) and np.isfinite(H).all()
    if not c.variant:
        n = np.linalg.norm(H, axis=0)
        assert n.min() > 0 and (c.cols < 8 or n.max() / n.min() > 10)  # columns of very different size
    G, n, e_ref = ts.reference(c)
    print(f"{cid}: e_ref {e_ref:.3e}")
    assert np.isfinite(e_ref) and 16 * e_ref < 1e-12
    assert ts.bound(e_ref) == max(16 * e_ref, 256 * ts.EPS)


def test_metric_sees_a_small_column_and_the_last_tile():
    """What the Frobenius-norm assertion cannot see: a relative error of 1e-9 in the SMALLEST column of the compressed system, or in the residual
    column, moves the metric to ~1e-9 while ||Hc^T Hc - G||_F / ||G||_F stays at rounding level."""
    c = ts.case("a-254-w3")
    H, r = ts.make_input(c)
    G, n, e_ref = ts.reference(c)
    Hc, rc = ts.lapack_compress(H, r)
    k = int(np.argmin(np.linalg.norm(H, axis=0)))
    bad = Hc.copy()
    bad[:, k] *= 1 + 1e-9
    Gd = np.asarray(G[:-1, :-1], dtype=np.float64)
    assert np.linalg.norm(bad.T @ bad - Gd) / np.linalg.norm(Gd) < 1e-12
    assert ts.metric(bad, rc, G, n) > 1e-10 > ts.bound(e_ref)
    assert ts.metric(Hc, rc * (1 + 1e-9), G, n) > 1e-10
    assert ts.metric(Hc, rc, G, n) == e_ref
