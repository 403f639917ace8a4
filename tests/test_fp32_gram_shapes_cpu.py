"""The catalogue of tests/fp32_gram_shapes.py without a GPU: (1) the coverage both groups claim, asserted from the plans and the oracle's
verdicts alone; (2) gram32_parts / gram32_tile_table of k_gram32.h, printed by a stand-alone host program (tests/host/gram32_table_main.cpp) for
1 .. 12 macro columns; (3) a numpy emulation of both kernels' arithmetic on the oracle's uncompressed stack of every case — under the bound of
40 u as it stands, and beyond four times the bound with each of the faults the cases are named for planted in it.  (3) is the proof that the
cases can see those faults at the bound the GPU test asserts.

Measured (test_emulation_and_faults prints every figure): the emulation 0.33 u (deep) to 6.9 u (r129); the planted faults, smallest over the
cases each applies to — the least visible accepted row dropped 1.0e4 u, a rejected feature's rows left at accepted rows' values 8.8e4 u, the
partial last stage skipped 5.7e4 u, one pad row non-zero 4.0e4 u (all four on deep; 3.3e5 u and more on every other case), the top macro column
or window skipped 1.7e7 u, two tiles swapped 4.8e7 u — against the 160 u each must exceed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fp32_gram_shapes as fg
from open_vins_amd import capi

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ALL = fg.CASES + [fg.STALE_FIRST, fg.STALE_SECOND, fg.STALE_THIRD]
PLANS = {c.id: c.plan() for c in ALL}


# --------------------------------------------------------------------------- (1) coverage
def test_group_a_widths_reach_their_edges():
    p = PLANS
    assert (p["w3"].D, p["w3"].NTM, p["w3"].NT, p["w3"].LG, p["w3"].LDF) == (74, 3, 5, 80, 96)           # the last macro column clipped
    assert (p["w4-residual-alone"].D, p["w4-residual-alone"].LD, p["w4-residual-alone"].NTM) == (96, 97, 4)  # column 96 = the residual, 31 pad columns
    assert p["w7"].D == 208 and p["w7"].tiles == 28 and set(p["w7"].tiles_per_wave[0]) == {3, 4}
    assert p["w9"].D == 264 and p["w9"].NTM == 9 and p["w9"].tiles == 45 and p["w9"].parts == 1 and set(p["w9"].tiles_per_wave[0]) == {5, 6}
    assert p["w10"].D == 300 and p["w10"].NTM == 10 and p["w10"].tiles == 55 and p["w10"].parts == 2
    w12 = p["w12"]
    assert (w12.D, w12.LD, w12.LDF, w12.NT, w12.tiles, w12.parts, w12.fetch_chunks) == (382, 383, 384, 24, 78, 2, 48)
    assert [sum(t) for t in w12.tiles_per_wave] == [39, 39]
    for cid in fg.A_IDS:
        assert max(max(t) for t in p[cid].tiles_per_wave) <= fg.G32_MAXT
        assert p[cid].NTM <= 12 and p[cid].fetch_chunks <= 48


def test_group_a_rows_reach_their_edges():
    p = PLANS
    assert p["r29"].rows <= 31 and p["r29"].Gw == 1 and p["r29"].wg_stages == [1]
    assert p["r128"].rows % 32 == 0 and p["r128"].Gw == 1
    assert p["r129"].rows == 129 and p["r129"].wg_rows == [96, 33] and p["r129"].last_stage_rows == 1
    assert {p[c].Gw for c in fg.ROW_IDS} >= {1, 2, 3, 4, 5}                      # every remainder of the reduction's loop of four, and none
    assert {p[c].Gw % 4 for c in fg.ROW_IDS} == {0, 1, 2, 3}
    assert any(4 in p[c].wg_stages for c in fg.ROW_IDS)                          # both halves of the double buffer reused
    assert len({fg.BY_ID[c].D for c in fg.ROW_IDS}) == 1
    for cid in fg.A_IDS:                                                          # no workgroup without rows, none beyond the kernel's 48 stages
        assert all(0 < s <= fg.G32_ROWS_WG // 32 for s in p[cid].wg_stages), cid
        assert sum(p[cid].wg_rows) == p[cid].rows
    assert any(p[c].rows % 32 for c in fg.WIDTH_IDS)


def test_group_b_reaches_its_edges():
    p = PLANS
    assert [(p[c].NT, p[c].NB, p[c].pairs) for c in ("nb1", "nb2", "nb2-featy-big2", "nb3-partial", "nb3-full")] == \
        [(5, 1, 1), (14, 2, 3), (14, 2, 3), (19, 3, 6), (24, 3, 6)]
    assert p["nb1"].NT < 8 and p["nb2"].NT % 8 and p["nb3-partial"].NT % 8 and p["nb3-full"].NT == 24
    assert p["c1"].rows < 32 and (p["c1"].nchunks, p["c1"].Gb) == (1, 1)
    assert (p["c2"].nchunks, p["c2"].Gb) == (2, 2)
    assert (p["c3"].nchunks, p["c3"].Gb) == (3, 3) and p["c3"].rows % 32
    assert p["c4-exact"].rows % 32 == 0 and p["c4-exact"].nchunks == p["c4-exact"].rows // 32
    deep = p["deep"]
    assert deep.rows >= 2.5 * 32 * fg.MI355X_CUS and deep.Gb == fg.MI355X_CUS and min(b - a for a, b in deep.blk_chunks) >= 3
    assert fg.BY_ID["nb2-featy-big2"].debug == dict(featy_big=2) and not fg.BY_ID["nb2-featy-big2"].options
    for cid in fg.B_IDS:
        if cid != "nb2-featy-big2":
            assert fg.BY_ID[cid].options == dict(no_fast_feature_kernel=1)
        assert sum(b - a for a, b in p[cid].blk_chunks) == p[cid].nchunks


@pytest.mark.parametrize("cid", [c.id for c in ALL])
def test_the_oracle_rejects_what_the_case_plants(oracle, cid):
    """a feature of one observation (no rows), one rejected before the gate WITH rows, one rejected by the gate, the rest used; the stack the
    plan counts is the one the oracle stacks; the uncompressed stack's Gram matrix is the compressed system's (all but the residual's square)"""
    c = fg.BY_ID.get(cid) or {x.id: x for x in ALL}[cid]
    R = fg.reference(oracle, c)
    st, m = R["ref"]["feat_status"], c.track_lengths
    used = st == capi.FEAT_USED
    assert used.any()
    rows = np.diff(c.row_off)
    assert int(rows[used].sum()) == R["ref"]["stats"]["n_rows"] and R["ref"]["stats"]["n_used"] == int(used.sum())
    if c is fg.STALE_FIRST:
        assert used.all()
    else:
        assert m[0] == 1 and st[0] == capi.FEAT_TOO_FEW_MEAS
        assert (st == capi.FEAT_CHI2_REJECTED).any(), "no feature is rejected by the gate"
        assert ((st == capi.FEAT_TRI_FAILED) & (rows > 0)).any(), "no feature with rows is rejected before the gate"
        assert used[-1], "the tail of the stack holds no accepted row"
    X = R["X"]
    Xl = X.astype(np.longdouble)
    G = Xl.T @ Xl
    A = R["A"].astype(np.longdouble)
    Gc = A.T @ A
    Gc[c.D, c.D] = G[c.D, c.D]
    e = fg.gram_error(np.asarray(G, dtype=np.float64), dict(R, G=Gc))
    short = 1 - float((A[:, c.D] @ A[:, c.D]) / G[c.D, c.D])
    print(f"fp32 gram {cid}: D {c.D} rows {c.rows} accepted {R['ref']['stats']['n_rows']} stack against the compressed system {e:.1e}, r_comp^T r_comp short by {short:.1e}")
    assert e < 1e-12
    assert short > -1e-12 and (short < 1e-12 or R["ref"]["stats"]["n_rows"] > c.D)


def test_stale_sequence(oracle):
    """the second batch is smaller, ends inside a stage, and its rejected features and its tail lie on rows the first batch left non-zero; the
    third changes the macro-column count"""
    a, b, c = fg.STALE_FIRST, fg.STALE_SECOND, fg.STALE_THIRD
    Xa = fg.reference(oracle, a)["X"]
    Rb = fg.reference(oracle, b)
    assert b.rows < a.rows and b.rows % 32 != 0 and cdiv32(b.rows) * 32 + 32 <= a.rows + 32
    stb, off = Rb["ref"]["feat_status"], b.row_off
    kinds = set()
    for f in np.flatnonzero(stb != capi.FEAT_USED):
        if off[f + 1] > off[f]:
            assert np.abs(Xa[off[f]:off[f + 1]]).max(axis=1).min() > 0
            kinds.add(int(stb[f]))
    assert kinds >= {capi.FEAT_TRI_FAILED, capi.FEAT_CHI2_REJECTED}
    assert np.abs(Xa[b.rows:cdiv32(b.rows) * 32]).max(axis=1).min() > 0   # what the partial last stage would read without the pad
    assert a.plan().NTM == b.plan().NTM == 7 and c.plan().NTM == 3


def cdiv32(n):
    return fg.cdiv(n, 32)


def test_header_states_both_paths_and_the_option():
    txt = open(os.path.join(ROOT, "include", "ovgpu.h")).read()
    at = txt.index("int32_t gram_fp32;")
    para = " ".join(ln.strip().strip("/*").strip() for ln in txt[at:txt.index("} ovgpu_options;", at)].splitlines())
    for term in ("k_gram_f32", "v_mfma_f32_32x32x2_f32", "k_gram_blk<true>", "v_mfma_f32_16x16x4_f32", "no_fast_feature_kernel", '"featy_big" = 2',
                 "40 u", "stack_is_f32"):
        assert term in para, term
    at = txt.index('"last_gram_workgroups"')
    para = txt[at:at + 700]
    for term in ("read only", "k_gram_f32", "k_gram_blk", "0 for every other"):
        assert term in para, term


# --------------------------------------------------------------------------- (2) the tile table
@pytest.fixture(scope="module")
def tile_tables(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("no hipcc (k_gram32.h includes the HIP runtime's header)")
    exe = str(tmp_path_factory.mktemp("gram32") / "gram32_table_main")
    build = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter",
                            "-I", os.path.join(ROOT, "open_vins_amd", "csrc"), os.path.join(ROOT, "tests", "host", "gram32_table_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "gram32 table ok" in run.stdout, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    consts = tuple(int(x) for x in lines[0].split()[1:])
    tables, cur = {}, None
    for ln in lines[1:-1]:
        w = ln.split()
        if w[0] == "ntm":
            cur = tables.setdefault(int(w[1]), dict(parts=int(w[3]), rows=[]))
        else:
            cur["rows"].append([int(x) for x in w])
    return consts, tables


def test_tile_table(tile_tables):
    consts, tables = tile_tables
    assert consts == (fg.G32_NW, fg.G32_MAXT, fg.STAGE, fg.G32_ROWS_WG)
    assert sorted(tables) == list(range(1, 13))
    assert tables[9]["parts"] == 1 and tables[10]["parts"] == 2
    for ntm, t in tables.items():
        plan = fg.Plan(32 * ntm - 1, 1, fg.MI355X_CUS)
        assert plan.NTM == ntm and t["parts"] == plan.parts and len(t["rows"]) == t["parts"] * fg.G32_NW
        seen, per_part, per_wave = [], [0] * t["parts"], []
        for k, row in enumerate(t["rows"]):
            part, wave, codes = row[0], row[1], row[2:]
            assert (part, wave) == divmod(k, fg.G32_NW) and len(codes) == fg.G32_MAXT
            live = [x for x in codes if x >= 0]
            assert codes == live + [-1] * (fg.G32_MAXT - len(live))        # a wavefront's tiles first, -1 elsewhere
            assert all(x == -1 for x in codes[len(live):])
            per_part[part] += len(live)
            per_wave.append(len(live))
            seen += [(x & 255, x >> 8) for x in live]
        want = [(i, j) for i in range(ntm) for j in range(i, ntm)]
        assert seen == want                                                   # every tile I <= J exactly once (row by row)
        assert max(per_wave) <= fg.G32_MAXT
        assert max(per_part) - min(per_part) <= 1
        assert [per_wave[fg.G32_NW * q:fg.G32_NW * (q + 1)] for q in range(t["parts"])] == plan.tiles_per_wave


# --------------------------------------------------------------------------- (3) the emulation and the planted faults
def _visibility(X, n):
    """per row r: max over i, j of |x_ri x_rj| / (n_i n_j) — what e(G) moves by when the row goes"""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(n > 0, np.abs(X) / n, 0.0)
    return q.max(axis=1) ** 2


@pytest.mark.parametrize("cid", [c.id for c in ALL])
def test_emulation_and_faults(oracle, cid):
    c = {x.id: x for x in ALL}[cid]
    R = fg.reference(oracle, c)
    X, off = R["X"], R["row_off"]
    plan = c.plan()
    n = R["n"].astype(np.float64)
    st = R["ref"]["feat_status"]
    e0 = fg.gram_error(fg.emulate(c, X, plan), R)
    figs = {}
    # a row dropped: the LEAST visible accepted row of the stack
    vis = _visibility(X, n)
    acc = np.flatnonzero(np.abs(X).max(axis=1) > 0)
    r = int(acc[np.argmin(vis[acc])])
    Xm = X.copy()
    Xm[r] = 0
    figs["row dropped"] = fg.gram_error(fg.emulate(c, Xm, plan), R)
    # a rejected feature's rows left at an earlier batch's values (here: the rows of the accepted features, in order)
    rej = [f for f in range(len(st)) if st[f] != capi.FEAT_USED and off[f + 1] > off[f]]
    if rej:
        f = rej[0]
        Xm = X.copy()
        Xm[off[f]:off[f + 1]] = X[np.resize(acc, off[f + 1] - off[f])]
        figs["stale rows"] = fg.gram_error(fg.emulate(c, Xm, plan), R)
    if c.rows % 32:
        figs["last stage skipped"] = fg.gram_error(fg.emulate(c, X, plan, skip_last_stage=True), R)
        figs["pad row"] = fg.gram_error(fg.emulate(c, X, plan, pad_rows=X[acc[:1]].astype(np.float32)), R)
    else:   # no pad row is ever multiplied: whatever lies there changes no bit
        assert np.array_equal(fg.emulate(c, X, plan, pad_rows=None), fg.emulate(c, X, plan))
    figs["top column skipped"] = fg.gram_error(fg.emulate(c, X, plan, skip_top_column=True), R)
    figs["tiles swapped"] = fg.gram_error(fg.emulate(c, X, plan, swap_tiles=True), R)
    print(f"fp32 gram {cid}: emulation {e0 / fg.U:.2f} u; " + ", ".join(f"{k} {v / fg.U:.3g} u" for k, v in figs.items()))
    assert e0 <= fg.BOUND
    for k, v in figs.items():
        assert v > fg.MUTATION_FLOOR, (k, v / fg.U)
