"""The Householder TSQR's dispatch rule restated once, the catalogue of systems that pin it at every edge, their inputs and the metric
(tests/test_tsqr_shapes_cpu.py checks every case on numpy alone, tests/test_gpu_tsqr_edges.py runs it on the device).

What the library switches on (configure_tsqr, enqueue_compress, enqueue_merge_tree), restated FROM THE DOCUMENTED RULE, not from the library:
  * column tiles NT = ceil((cols + 1) / 16): leaves by the panel-wave kernel up to 15, k_qr_node at 16, k_qr_append (32-row blocks) beyond;
    merges with 16 quads per register array up to 8 tiles, 28 up to 14, 32 up to 16, k_qr_append beyond;
  * rows per leaf: ceil(rows / target) rounded up to whole 128-row appends, target = tsqr_workers or the CU count; a 128-row leaf becomes a 256-row
    one as soon as the stack holds more than 256 rows; W = ceil(rows / rows per leaf) leaves;
  * the merge tree: one launch NEXT TO the leaves while 2 W - 1 <= num_cu and NT <= 15 (tsqr_overlap 1 / 2 force / forbid the first condition),
    one launch behind them while W - 1 <= num_cu and NT <= 16 and tsqr_no_pipeline is off, one launch per level otherwise; none for one leaf.
The GPU tests compare what ovgpu_debug_option reports with dispatch(); EXPECT_256 holds every case's values on 256 CUs, written out.

A helper module, not a conftest: nothing here is collected.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

BLK = 128      # rows per append of the tiled leaves
B_APPEND = 32  # rows per block of k_qr_append
LEAF_PW, LEAF_NODE, LEAF_APPEND = 0, 1, 2
TREE_NONE, TREE_OVERLAP, TREE_PIPELINED, TREE_LEVELS = 0, 1, 2, 3
EPS = float(np.finfo(np.float64).eps)


# --------------------------------------------------------------------------- the rule
def n_tiles(cols):
    return (cols + 1 + 15) // 16


def configure(rows, workers, num_cu):
    """(rows per leaf, leaves) of a stack of `rows` rows: options.tsqr_workers = workers (0: one leaf per CU)."""
    target = max(1, workers if workers > 0 else num_cu)
    rpn = -(-rows // target)
    rpn = max(BLK, -(-rpn // BLK) * BLK)
    if rpn < 2 * BLK and rows > 2 * BLK:
        rpn = 2 * BLK
    return rpn, max(1, -(-rows // rpn))


def leaf_kernel(nt):
    return LEAF_PW if nt <= 15 else (LEAF_NODE if nt == 16 else LEAF_APPEND)


def merge_qh(nt):
    return 16 if nt <= 8 else (28 if nt <= 14 else (32 if nt <= 16 else 0))


def tree_mode(nt, W, num_cu, no_pipeline=0, overlap=0):
    if W <= 1:
        return TREE_NONE
    pipelined = (not no_pipeline) and nt <= 16 and W - 1 <= num_cu
    want = (2 * W - 1 <= num_cu) if overlap == 0 else overlap == 1
    if want and nt <= 15 and pipelined:
        return TREE_OVERLAP
    return TREE_PIPELINED if pipelined else TREE_LEVELS


@dataclass(frozen=True)
class Dispatch:
    NT: int
    leaf: int
    qh: int           # of the merge kernels; 0 where nothing is merged or k_qr_append merges
    W: int
    rpn: int
    last_leaf: int    # rows of the last leaf
    last_block: int   # rows of that leaf's last append (128-row appends) / last block (32-row blocks of k_qr_append)
    tree: int

    def astuple(self):
        return (self.NT, self.leaf, self.qh, self.W, self.last_leaf, self.last_block, self.tree)


def dispatch(rows, cols, workers, num_cu, no_pipeline=0, overlap=0):
    nt = n_tiles(cols)
    rpn, W = configure(rows, workers, num_cu)
    last = rows - (W - 1) * rpn
    blk = B_APPEND if nt > 16 else BLK
    tree = tree_mode(nt, W, num_cu, no_pipeline, overlap)
    return Dispatch(nt, leaf_kernel(nt), merge_qh(nt) if tree != TREE_NONE else 0, W, rpn, last, (last - 1) % blk + 1, tree)


def rows_for_leaves(W):
    """Rows that give exactly W leaves of 256 rows with tsqr_workers = W, the last leaf holding ONE row (W >= 2)."""
    return 256 * (W - 1) + 1


# --------------------------------------------------------------------------- the cases
@dataclass(frozen=True)
class Case:
    id: str
    group: str
    rows: int
    cols: int
    workers: int = 0
    options: tuple = ()        # further capi.default_options keywords, as sorted (name, value) pairs
    variant: str = ""          # degenerate input (group d), see make_input
    inplace: bool = False
    seed_as: str = ""          # cases with the same (rows, cols, seed_as or variant) share one input: the variants of group (c)
    zero_cols: tuple = ()

    @property
    def opts(self):
        return dict(self.options)

    def dispatch(self, num_cu):
        o = self.opts
        return dispatch(self.rows, self.cols, self.workers, num_cu, o.get("tsqr_no_pipeline", 0), o.get("tsqr_overlap", 0))


A_COLS = [1, 2, 14, 15, 16, 17, 126, 127, 128, 222, 223, 224, 238, 239, 240, 254, 255, 256, 510, 511]
NT_EDGES = [(1, 2), (8, 9), (14, 15), (15, 16), (16, 17)]
B_COLS = [40, 230, 250]
B32_ROWS = [301, 319, 320, 321, 300 + 128 + 1]
PASS_THROUGH = [(r, c) for c in (16, 300) for r in (1, c - 1, c)]
C_W = [2, 3, 7, 8, 9]
D_COLS = [40, 250, 300]
D_VARIANTS = ["zero0", "zero15", "zero16", "zerolast", "dup_tile", "dup_tiles", "Hzero", "rzero", "zero_append", "rank3"]
C_EDGE_IDS = ["c-overlap-lo", "c-overlap-hi", "c-pipe-lo", "c-pipe-hi"]


def edge_leaves(num_cu):
    """The leaf counts on either side of the two rule edges in W: the last W with 2 W - 1 <= num_cu and the next, the last with W - 1 <= num_cu and
    the next."""
    w_ov, w_pp = (num_cu + 1) // 2, num_cu + 1
    return dict(zip(C_EDGE_IDS, (w_ov, w_ov + 1, w_pp, w_pp + 1)))


def _o(**kw):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def cases(num_cu=256):
    """Every case, in a fixed order with fixed ids; only the four rule-edge cases of group (c) depend on the CU count."""
    out = []
    for cols in A_COLS:                                   # (a) column tiles
        for w in (1, 3):
            out.append(Case(f"a-{cols}-w{w}", "a", cols + 131, cols, w))
    for cols in B_COLS:                                   # (b) rows of the 128-row leaves
        for rows in (cols + 1, cols + 2, 2 * BLK - 1, 2 * BLK, 2 * BLK + 1, 3 * BLK + 1, 5 * BLK + 127):
            if rows > cols:
                for w in (1, 2, 0):
                    out.append(Case(f"b-{cols}-{rows}-w{w}", "b", rows, cols, w))
    for rows in B32_ROWS:                                 # ... and of the 32-row blocks
        for w in (1, 2):
            out.append(Case(f"b32-300-{rows}-w{w}", "b", rows, 300, w))
    for rows, cols in ((257, 40), (385, 250), (321, 300)):  # in place, rows > cols
        out.append(Case(f"b-{cols}-{rows}-inplace", "b", rows, cols, 0, inplace=True))
    for cid, W in edge_leaves(num_cu).items():            # (c) leaves and tree
        out.append(Case(cid, "c", rows_for_leaves(W), 17, W))
    for W in C_W:
        out.append(Case(f"c-W{W}", "c", rows_for_leaves(W), 17, W, seed_as="c"))
    for W in (3, 9):
        out.append(Case(f"c-W{W}-levels", "c", rows_for_leaves(W), 17, W, _o(tsqr_no_pipeline=1), seed_as="c"))
        out.append(Case(f"c-W{W}-ov1", "c", rows_for_leaves(W), 17, W, _o(tsqr_overlap=1), seed_as="c"))
        out.append(Case(f"c-W{W}-ov2", "c", rows_for_leaves(W), 17, W, _o(tsqr_overlap=2), seed_as="c"))
    for cols in (238, 240):
        out.append(Case(f"c-{cols}-W5", "c", rows_for_leaves(5), cols, 5, seed_as="c"))
        out.append(Case(f"c-{cols}-W5-ov1", "c", rows_for_leaves(5), cols, 5, _o(tsqr_overlap=1), seed_as="c"))
        out.append(Case(f"c-{cols}-W5-ov2", "c", rows_for_leaves(5), cols, 5, _o(tsqr_overlap=2), seed_as="c"))
    for cols in D_COLS:                                   # (d) degenerate columns and rows
        for v in D_VARIANTS:
            zc = dict(zero0=(0,), zero15=(15,), zero16=(16,), zerolast=(cols - 1,), Hzero=tuple(range(cols))).get(v, ())
            out.append(Case(f"d-{cols}-{v}", "d", cols + 200, cols, 1 if v == "zero_append" else 0, variant=v, zero_cols=zc))
    # at 40 columns the 240 rows end inside the zeroed append: the same in a leaf of four appends, where non-zero rows follow the zero ones
    out.append(Case("d-40-zero_append-385", "d", 3 * BLK + 1, 40, 1, variant="zero_append"))
    assert len({c.id for c in out}) == len(out)
    return tuple(out)


CASE_IDS = [c.id for c in cases(256)]
VARIANT_SETS = {  # group (c): variants of ONE input that must agree with each other
    "W3": ["c-W3", "c-W3-levels", "c-W3-ov1", "c-W3-ov2"],
    "W9": ["c-W9", "c-W9-levels", "c-W9-ov1", "c-W9-ov2"],
    "238": ["c-238-W5", "c-238-W5-ov1", "c-238-W5-ov2"],
    "240": ["c-240-W5", "c-240-W5-ov1", "c-240-W5-ov2"],
}


def case(cid, num_cu=256):
    return next(c for c in cases(num_cu) if c.id == cid)


def family(d):
    """The kernel family a dispatch belongs to (DESIGN §3's table): leaf kernel, and the merge kernels' register arrays where a merge runs."""
    return ("pw", "node", "append")[d.leaf] + (f"+qh{d.qh}" if d.qh else ("+append" if d.tree else ""))


# --------------------------------------------------------------------------- inputs
def _seed(c):
    return [c.rows, c.cols, sum(map(ord, c.seed_as or c.variant))]


_inputs = {}


def make_input(c):
    """H = normal(rows, cols) * column scales log-uniform in [1e-3, 1e3], r = normal(rows), seeded by the shape; group (d) degenerates it.
    Built once per (shape, variant) and never modified."""
    key = tuple(_seed(c)) + (c.variant,)
    if key in _inputs:
        return _inputs[key]
    rng = np.random.default_rng(_seed(c))
    rows, cols = c.rows, c.cols
    scale = 10.0 ** rng.uniform(-3.0, 3.0, cols)
    H = rng.normal(size=(rows, cols)) * scale
    r = rng.normal(size=rows)
    v = c.variant
    if c.zero_cols:
        H[:, list(c.zero_cols)] = 0.0
    if v == "dup_tile":       # two identical columns in one tile
        H[:, 7] = H[:, 3]
    elif v == "dup_tiles":    # ... and in two tiles
        H[:, 20] = H[:, 3]
    elif v == "rzero":
        r[:] = 0.0
    elif v == "zero_append":  # rows 128 .. 255 of ONE leaf: a whole 128-row append (four 32-row blocks of k_qr_append) with non-zero rows behind it; at 240 rows the stack ends inside it
        H[BLK:2 * BLK] = 0.0
        r[BLK:2 * BLK] = 0.0
    elif v == "rank3":
        H = (rng.normal(size=(rows, 3)) @ rng.normal(size=(3, cols))) * scale
    H, r = np.ascontiguousarray(H), np.ascontiguousarray(r)
    H.setflags(write=False), r.setflags(write=False)
    _inputs[key] = (H, r)
    return H, r


def claimed_rank(c):
    """Rank of H that a case claims."""
    v = c.variant
    if v == "Hzero":
        return 0
    if v == "rank3":
        return 3
    if v in ("dup_tile", "dup_tiles") or c.zero_cols:
        return c.cols - 1
    return c.cols


# --------------------------------------------------------------------------- the metric
def gram_ref(H, r):
    """G = [H | r]^T [H | r] in np.longdouble, and the column norms n_j (1 for a zero column)."""
    A = np.concatenate([H, r[:, None]], axis=1).astype(np.longdouble)
    G = A.T @ A
    n = np.sqrt(np.diag(G))
    n = np.where(n == 0, np.longdouble(1), n)
    return G, n


def metric(Hc, rc, G, n):
    """max over (i, j) != (cols, cols) of |(M^T M)_ij - G_ij| / (n_i n_j), M = [Hc | rc]: entrywise on the column-normalised Gram matrix, so a
    wrong small column or last tile shows at full size.  The residual's own diagonal entry is left out: a compression keeps H^T H and H^T r, while
    rc^T rc loses the part of r outside the range of H — for LAPACK's factor exactly as for the library's."""
    M = np.concatenate([Hc, rc[:, None]], axis=1).astype(np.longdouble)
    E = np.abs(M.T @ M - G) / np.outer(n, n)
    E[-1, -1] = 0
    return float(E.max())


def lapack_compress(H, r):
    """The first `cols` rows of LAPACK's Householder R of [H | r] (float64), as (Hc, rc)."""
    R = np.linalg.qr(np.concatenate([H, r[:, None]], axis=1), mode="r")
    cols = H.shape[1]
    R = R[:cols] if R.shape[0] >= cols else np.concatenate([R, np.zeros((cols - R.shape[0], cols + 1))])
    return np.ascontiguousarray(R[:, :cols]), np.ascontiguousarray(R[:, cols])


def bound(e_ref):
    """err <= max(16 e_ref, 256 eps), never looser than the project's 1e-12: 16 for the up to nine extra levels of reflections of a TSQR tree and the
    rsq / rcp-with-Newton reflector scalars (a few ulp) LAPACK does not have; the floor for tiny cases where LAPACK is exact by luck."""
    return min(max(16.0 * e_ref, 256.0 * EPS), 1e-12)


_refs = {}


def reference(c):
    """(G, n, e_ref) of a case, computed once."""
    key = tuple(_seed(c)) + (c.variant,)
    if key not in _refs:
        H, r = make_input(c)
        G, n = gram_ref(H, r)
        _refs[key] = (G, n, metric(*lapack_compress(H, r), G, n))
    return _refs[key]


# --------------------------------------------------------------------------- every case on 256 CUs, written out:
# id: (NT, leaf kernel, merge QH, W, rows in the last leaf, rows in its last append / 32-row block, tree)
EXPECT_256 = {
    "a-1-w1": (1, 0, 0, 1, 132, 4, 0),
    "a-1-w3": (1, 0, 16, 2, 4, 4, 1),
    "a-2-w1": (1, 0, 0, 1, 133, 5, 0),
    "a-2-w3": (1, 0, 16, 2, 5, 5, 1),
    "a-14-w1": (1, 0, 0, 1, 145, 17, 0),
    "a-14-w3": (1, 0, 16, 2, 17, 17, 1),
    "a-15-w1": (1, 0, 0, 1, 146, 18, 0),
    "a-15-w3": (1, 0, 16, 2, 18, 18, 1),
    "a-16-w1": (2, 0, 0, 1, 147, 19, 0),
    "a-16-w3": (2, 0, 16, 2, 19, 19, 1),
    "a-17-w1": (2, 0, 0, 1, 148, 20, 0),
    "a-17-w3": (2, 0, 16, 2, 20, 20, 1),
    "a-126-w1": (8, 0, 0, 1, 257, 1, 0),
    "a-126-w3": (8, 0, 16, 2, 1, 1, 1),
    "a-127-w1": (8, 0, 0, 1, 258, 2, 0),
    "a-127-w3": (8, 0, 16, 2, 2, 2, 1),
    "a-128-w1": (9, 0, 0, 1, 259, 3, 0),
    "a-128-w3": (9, 0, 28, 2, 3, 3, 1),
    "a-222-w1": (14, 0, 0, 1, 353, 97, 0),
    "a-222-w3": (14, 0, 28, 2, 97, 97, 1),
    "a-223-w1": (14, 0, 0, 1, 354, 98, 0),
    "a-223-w3": (14, 0, 28, 2, 98, 98, 1),
    "a-224-w1": (15, 0, 0, 1, 355, 99, 0),
    "a-224-w3": (15, 0, 32, 2, 99, 99, 1),
    "a-238-w1": (15, 0, 0, 1, 369, 113, 0),
    "a-238-w3": (15, 0, 32, 2, 113, 113, 1),
    "a-239-w1": (15, 0, 0, 1, 370, 114, 0),
    "a-239-w3": (15, 0, 32, 2, 114, 114, 1),
    "a-240-w1": (16, 1, 0, 1, 371, 115, 0),
    "a-240-w3": (16, 1, 32, 2, 115, 115, 2),
    "a-254-w1": (16, 1, 0, 1, 385, 1, 0),
    "a-254-w3": (16, 1, 32, 2, 129, 1, 2),
    "a-255-w1": (16, 1, 0, 1, 386, 2, 0),
    "a-255-w3": (16, 1, 32, 2, 130, 2, 2),
    "a-256-w1": (17, 2, 0, 1, 387, 3, 0),
    "a-256-w3": (17, 2, 0, 2, 131, 3, 3),
    "a-510-w1": (32, 2, 0, 1, 641, 1, 0),
    "a-510-w3": (32, 2, 0, 3, 129, 1, 3),
    "a-511-w1": (32, 2, 0, 1, 642, 2, 0),
    "a-511-w3": (32, 2, 0, 3, 130, 2, 3),
    "b-40-41-w1": (3, 0, 0, 1, 41, 41, 0),
    "b-40-41-w2": (3, 0, 0, 1, 41, 41, 0),
    "b-40-41-w0": (3, 0, 0, 1, 41, 41, 0),
    "b-40-42-w1": (3, 0, 0, 1, 42, 42, 0),
    "b-40-42-w2": (3, 0, 0, 1, 42, 42, 0),
    "b-40-42-w0": (3, 0, 0, 1, 42, 42, 0),
    "b-40-255-w1": (3, 0, 0, 1, 255, 127, 0),
    "b-40-255-w2": (3, 0, 16, 2, 127, 127, 1),
    "b-40-255-w0": (3, 0, 16, 2, 127, 127, 1),
    "b-40-256-w1": (3, 0, 0, 1, 256, 128, 0),
    "b-40-256-w2": (3, 0, 16, 2, 128, 128, 1),
    "b-40-256-w0": (3, 0, 16, 2, 128, 128, 1),
    "b-40-257-w1": (3, 0, 0, 1, 257, 1, 0),
    "b-40-257-w2": (3, 0, 16, 2, 1, 1, 1),
    "b-40-257-w0": (3, 0, 16, 2, 1, 1, 1),
    "b-40-385-w1": (3, 0, 0, 1, 385, 1, 0),
    "b-40-385-w2": (3, 0, 16, 2, 129, 1, 1),
    "b-40-385-w0": (3, 0, 16, 2, 129, 1, 1),
    "b-40-767-w1": (3, 0, 0, 1, 767, 127, 0),
    "b-40-767-w2": (3, 0, 16, 2, 383, 127, 1),
    "b-40-767-w0": (3, 0, 16, 3, 255, 127, 1),
    "b-230-231-w1": (15, 0, 0, 1, 231, 103, 0),
    "b-230-231-w2": (15, 0, 32, 2, 103, 103, 1),
    "b-230-231-w0": (15, 0, 32, 2, 103, 103, 1),
    "b-230-232-w1": (15, 0, 0, 1, 232, 104, 0),
    "b-230-232-w2": (15, 0, 32, 2, 104, 104, 1),
    "b-230-232-w0": (15, 0, 32, 2, 104, 104, 1),
    "b-230-255-w1": (15, 0, 0, 1, 255, 127, 0),
    "b-230-255-w2": (15, 0, 32, 2, 127, 127, 1),
    "b-230-255-w0": (15, 0, 32, 2, 127, 127, 1),
    "b-230-256-w1": (15, 0, 0, 1, 256, 128, 0),
    "b-230-256-w2": (15, 0, 32, 2, 128, 128, 1),
    "b-230-256-w0": (15, 0, 32, 2, 128, 128, 1),
    "b-230-257-w1": (15, 0, 0, 1, 257, 1, 0),
    "b-230-257-w2": (15, 0, 32, 2, 1, 1, 1),
    "b-230-257-w0": (15, 0, 32, 2, 1, 1, 1),
    "b-230-385-w1": (15, 0, 0, 1, 385, 1, 0),
    "b-230-385-w2": (15, 0, 32, 2, 129, 1, 1),
    "b-230-385-w0": (15, 0, 32, 2, 129, 1, 1),
    "b-230-767-w1": (15, 0, 0, 1, 767, 127, 0),
    "b-230-767-w2": (15, 0, 32, 2, 383, 127, 1),
    "b-230-767-w0": (15, 0, 32, 3, 255, 127, 1),
    "b-250-251-w1": (16, 1, 0, 1, 251, 123, 0),
    "b-250-251-w2": (16, 1, 32, 2, 123, 123, 2),
    "b-250-251-w0": (16, 1, 32, 2, 123, 123, 2),
    "b-250-252-w1": (16, 1, 0, 1, 252, 124, 0),
    "b-250-252-w2": (16, 1, 32, 2, 124, 124, 2),
    "b-250-252-w0": (16, 1, 32, 2, 124, 124, 2),
    "b-250-255-w1": (16, 1, 0, 1, 255, 127, 0),
    "b-250-255-w2": (16, 1, 32, 2, 127, 127, 2),
    "b-250-255-w0": (16, 1, 32, 2, 127, 127, 2),
    "b-250-256-w1": (16, 1, 0, 1, 256, 128, 0),
    "b-250-256-w2": (16, 1, 32, 2, 128, 128, 2),
    "b-250-256-w0": (16, 1, 32, 2, 128, 128, 2),
    "b-250-257-w1": (16, 1, 0, 1, 257, 1, 0),
    "b-250-257-w2": (16, 1, 32, 2, 1, 1, 2),
    "b-250-257-w0": (16, 1, 32, 2, 1, 1, 2),
    "b-250-385-w1": (16, 1, 0, 1, 385, 1, 0),
    "b-250-385-w2": (16, 1, 32, 2, 129, 1, 2),
    "b-250-385-w0": (16, 1, 32, 2, 129, 1, 2),
    "b-250-767-w1": (16, 1, 0, 1, 767, 127, 0),
    "b-250-767-w2": (16, 1, 32, 2, 383, 127, 2),
    "b-250-767-w0": (16, 1, 32, 3, 255, 127, 2),
    "b32-300-301-w1": (19, 2, 0, 1, 301, 13, 0),
    "b32-300-301-w2": (19, 2, 0, 2, 45, 13, 3),
    "b32-300-319-w1": (19, 2, 0, 1, 319, 31, 0),
    "b32-300-319-w2": (19, 2, 0, 2, 63, 31, 3),
    "b32-300-320-w1": (19, 2, 0, 1, 320, 32, 0),
    "b32-300-320-w2": (19, 2, 0, 2, 64, 32, 3),
    "b32-300-321-w1": (19, 2, 0, 1, 321, 1, 0),
    "b32-300-321-w2": (19, 2, 0, 2, 65, 1, 3),
    "b32-300-429-w1": (19, 2, 0, 1, 429, 13, 0),
    "b32-300-429-w2": (19, 2, 0, 2, 173, 13, 3),
    "b-40-257-inplace": (3, 0, 16, 2, 1, 1, 1),
    "b-250-385-inplace": (16, 1, 32, 2, 129, 1, 2),
    "b-300-321-inplace": (19, 2, 0, 2, 65, 1, 3),
    "c-overlap-lo": (2, 0, 16, 128, 1, 1, 1),
    "c-overlap-hi": (2, 0, 16, 129, 1, 1, 2),
    "c-pipe-lo": (2, 0, 16, 257, 1, 1, 2),
    "c-pipe-hi": (2, 0, 16, 258, 1, 1, 3),
    "c-W2": (2, 0, 16, 2, 1, 1, 1),
    "c-W3": (2, 0, 16, 3, 1, 1, 1),
    "c-W7": (2, 0, 16, 7, 1, 1, 1),
    "c-W8": (2, 0, 16, 8, 1, 1, 1),
    "c-W9": (2, 0, 16, 9, 1, 1, 1),
    "c-W3-levels": (2, 0, 16, 3, 1, 1, 3),
    "c-W3-ov1": (2, 0, 16, 3, 1, 1, 1),
    "c-W3-ov2": (2, 0, 16, 3, 1, 1, 2),
    "c-W9-levels": (2, 0, 16, 9, 1, 1, 3),
    "c-W9-ov1": (2, 0, 16, 9, 1, 1, 1),
    "c-W9-ov2": (2, 0, 16, 9, 1, 1, 2),
    "c-238-W5": (15, 0, 32, 5, 1, 1, 1),
    "c-238-W5-ov1": (15, 0, 32, 5, 1, 1, 1),
    "c-238-W5-ov2": (15, 0, 32, 5, 1, 1, 2),
    "c-240-W5": (16, 1, 32, 5, 1, 1, 2),
    "c-240-W5-ov1": (16, 1, 32, 5, 1, 1, 2),
    "c-240-W5-ov2": (16, 1, 32, 5, 1, 1, 2),
    "d-40-zero0": (3, 0, 16, 2, 112, 112, 1),
    "d-40-zero15": (3, 0, 16, 2, 112, 112, 1),
    "d-40-zero16": (3, 0, 16, 2, 112, 112, 1),
    "d-40-zerolast": (3, 0, 16, 2, 112, 112, 1),
    "d-40-dup_tile": (3, 0, 16, 2, 112, 112, 1),
    "d-40-dup_tiles": (3, 0, 16, 2, 112, 112, 1),
    "d-40-Hzero": (3, 0, 16, 2, 112, 112, 1),
    "d-40-rzero": (3, 0, 16, 2, 112, 112, 1),
    "d-40-zero_append": (3, 0, 0, 1, 240, 112, 0),
    "d-40-rank3": (3, 0, 16, 2, 112, 112, 1),
    "d-250-zero0": (16, 1, 32, 2, 194, 66, 2),
    "d-250-zero15": (16, 1, 32, 2, 194, 66, 2),
    "d-250-zero16": (16, 1, 32, 2, 194, 66, 2),
    "d-250-zerolast": (16, 1, 32, 2, 194, 66, 2),
    "d-250-dup_tile": (16, 1, 32, 2, 194, 66, 2),
    "d-250-dup_tiles": (16, 1, 32, 2, 194, 66, 2),
    "d-250-Hzero": (16, 1, 32, 2, 194, 66, 2),
    "d-250-rzero": (16, 1, 32, 2, 194, 66, 2),
    "d-250-zero_append": (16, 1, 0, 1, 450, 66, 0),
    "d-250-rank3": (16, 1, 32, 2, 194, 66, 2),
    "d-300-zero0": (19, 2, 0, 2, 244, 20, 3),
    "d-300-zero15": (19, 2, 0, 2, 244, 20, 3),
    "d-300-zero16": (19, 2, 0, 2, 244, 20, 3),
    "d-300-zerolast": (19, 2, 0, 2, 244, 20, 3),
    "d-300-dup_tile": (19, 2, 0, 2, 244, 20, 3),
    "d-300-dup_tiles": (19, 2, 0, 2, 244, 20, 3),
    "d-300-Hzero": (19, 2, 0, 2, 244, 20, 3),
    "d-300-rzero": (19, 2, 0, 2, 244, 20, 3),
    "d-300-zero_append": (19, 2, 0, 1, 500, 20, 0),
    "d-300-rank3": (19, 2, 0, 2, 244, 20, 3),
    "d-40-zero_append-385": (3, 0, 0, 1, 385, 1, 0),
}
