"""The snapshots of tests/test_gpu_mode_a_shapes.py on the oracle alone (no GPU): every one of them must be what it is named for BEFORE it
travels — the column count, the kernels written next to it, the rows of a rank case's stack, a gate verdict no rounding can turn, a factor
whose genuine rows and noise rows are two decades apart, and an emulated (H, r) that reproduces the oracle's posterior.

The emulation is tests/test_mode_a_numerics.py's (mode_a_shapes.emulate): the oracle's compressed system times L, the diagonally pivoted factor
(tools/dev_mode_a_numerics.chol_pivoted, tolerance 1e-15) of its Gram matrix, un-whitened with solve_triangular.

Measured here (24 full tracks, the seeds of mode_a_shapes): genuine rank D - 13 on every state with full calibration, D - 6 / D - 7 on the states
without calibration columns, R on the rank cases, equal to the SVD rank everywhere; the smallest genuine row 1.3e-5 of the largest (D = 352), the
largest noise row 3.6e-8 (D = 258); the emulation's dx within 4.3e-12 and P' within 8.7e-13 of the oracle's (bounds 1e-8 / 1e-9)."""
import numpy as np
import pytest

import mode_a_shapes as mas
from open_vins_amd import capi
from parity_util import GATE_MARGIN

from test_gpu_parity import TOL_DX, TOL_P  # (importing the module needs no GPU)

# id: (route, factor kernel, NB of the rank-one factor, Gram kernel, T of the one-pass Gram kernel, un-whitening kernel), written out by hand from
# the rule in include/ovgpu.h
EXPECT = {
    "col-126": ("pchol", "blk<4,9,2>", 0, "one-pass", 8, "blk<16>"),      # LD 127: 8 tile columns
    "col-128": ("pchol", "blk<7,15,4>", 0, "one-pass", 10, "blk<16>"),    # LD 129: 9
    "col-222": ("pchol", "blk<7,15,4>", 0, "one-pass", 14, "blk<16>"),    # LD 223: 14
    "col-224": ("pchol", "rank-one", 8, "one-pass", 15, "blk<16>"),       # LD 225: 15
    "col-254": ("pchol", "rank-one", 8, "one-pass", 16, "blk<16>"),       # LD 255: 16
    "col-256": ("pchol", "rank-one", 9, "blk", 0, "blk<16>"),             # LD 257: 17, and exactly 16 un-whitening tile columns
    "col-258": ("pchol", "rank-one", 9, "blk", 0, "subst<24>"),           # 17 un-whitening tile columns
    "col-300": ("pchol", "rank-one", 10, "blk", 0, "subst<24>"),
    "col-320": ("pchol", "rank-one", 11, "blk", 0, "subst<24>"),
    "col-350": ("pchol", "rank-one", 11, "blk", 0, "subst<24>"),          # LD 351: 22
    "col-352": ("pchol", "rank-one", 12, "wide", 0, "subst<24>"),         # LD 353: 23
    "col-366": ("pchol", "rank-one", 12, "wide", 0, "subst<24>"),         # LD 367: 23
    "col-368": ("pchol", "rank-one", 12, "blk", 0, "subst<24>"),          # LD 369: 24
    "col-382": ("pchol", "rank-one", 12, "blk", 0, "subst<24>"),          # LD 383: 24
    "col-384": ("tsqr", None, 0, None, 0, None),                          # LD 385: 25
    "small-D30": ("pchol", "blk<4,9,2>", 0, "one-pass", 2, "blk<16>"),    # LD 31: 2
    "small-D42": ("pchol", "blk<4,9,2>", 0, "one-pass", 4, "blk<16>"),    # LD 43: 3
    "small-D48": ("pchol", "blk<4,9,2>", 0, "one-pass", 4, "blk<16>"),    # LD 49: 4
    "small-D66": ("pchol", "blk<4,9,2>", 0, "one-pass", 6, "blk<16>"),    # LD 67: 5
    "reject-208": ("pchol", "blk<7,15,4>", 0, "one-pass", 14, "blk<16>"),
}
for _R in (1, 3, 4, 5, 8, 9, 16, 17):
    EXPECT[f"rank-208-R{_R}"] = ("pchol", "blk<7,15,4>", 0, "one-pass", 14, "blk<16>")  # LD 209: 14
for _R in (1, 3, 4, 8):
    EXPECT[f"rank-126-R{_R}"] = ("pchol", "blk<4,9,2>", 0, "one-pass", 8, "blk<16>")
for _R in (1, 3, 4, 8, 17):
    EXPECT[f"rank-256-R{_R}"] = ("pchol", "rank-one", 9, "blk", 0, "blk<16>")


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def test_every_case_is_what_is_written_next_to_it():
    assert sorted(mas.CASE_IDS) == sorted(EXPECT)
    for c in mas.CASES:
        assert tuple(mas.expected(c.D)) == EXPECT[c.id], c.id
        assert c.D == 6 * c.state["C"] + c.state["K"] * (6 * c.state.get("pose", 1) + 8 * c.state.get("intr", 1))
    # the column cases of the issue: D = 6 C + 14 K, full calibration, K <= 4
    assert {D: 6 * C + 14 * K for D, (C, K) in mas.COLUMN_STATES.items()} == {D: D for D in mas.COLUMN_STATES}
    assert sorted(mas.COLUMN_STATES) == [126, 128, 222, 224, 254, 256, 258, 300, 320, 350, 352, 366, 368, 382, 384]
    assert all(K <= 4 for _, K in mas.COLUMN_STATES.values())
    # the states below six tile columns: at least three, tile counts in 2 .. 5, one of them a multiple of 16 columns
    small = [c for c in mas.CASES if c.group == "small"]
    assert len(small) >= 3 and all(2 <= mas.n_tiles(c.D) <= 5 for c in small) and any(c.D % 16 == 0 for c in small)
    assert {mas.n_tiles(c.D) for c in small} == {2, 3, 4, 5}
    # the rank cases
    assert mas.RANK_R[208] == (1, 3, 4, 5, 8, 9, 16, 17)
    for D in (126, 256):
        assert set(mas.RANK_R[D]) <= set(mas.RANK_R[208]) and {R % 4 for R in mas.RANK_R[D]} >= {0, 1, 3} and 8 in mas.RANK_R[D]
    assert {R % 8 for R in mas.RANK_R[208]} >= {0, 1, 3}
    assert all(sum(2 * m - 3 for m in lens) == R for R, lens in mas.RANK_LENGTHS.items())


def test_the_rule_by_hand():
    """expected() against values worked by hand from the thresholds of include/ovgpu.h (not from the catalogue)."""
    e = mas.expected
    # route
    assert e(383).route == "pchol" and e(384).route == "tsqr" and e(511).route == "tsqr" and tuple(e(384))[1:] == (None, 0, None, 0, None)
    # factor: 8 | 9 and 14 | 15 tile columns of LD = D + 1
    assert [e(D).factor for D in (15, 127, 128, 223, 224, 383)] == ["blk<4,9,2>", "blk<4,9,2>", "blk<7,15,4>", "blk<7,15,4>", "rank-one", "rank-one"]
    assert [e(D).nb for D in (224, 255, 256, 287, 288, 319, 320, 351, 352, 383)] == [8, 8, 9, 9, 10, 10, 11, 11, 12, 12]
    # ... and with the blocked factor off the rank-one kernel everywhere, NB = ceil((D + 1) / 32)
    assert [(e(D, False).factor, e(D, False).nb) for D in (30, 31, 32, 126, 128, 208, 222)] == [("rank-one", n) for n in (1, 1, 2, 4, 5, 7, 7)]
    # Gram matrix
    assert [(e(D).gram, e(D).gram_nt) for D in (15, 16, 31, 32, 207, 208, 223, 224, 239, 240, 255)] == [("one-pass", t) for t in (2, 2, 2, 4, 14, 14, 14, 15, 15, 16, 16)]
    assert [e(D).gram for D in (256, 351, 352, 367, 368, 383)] == ["blk", "blk", "wide", "wide", "blk", "blk"]
    # un-whitening: 16 | 17 tile columns of D, the switch, and a prior factored step by step (no inverse diagonal tiles)
    assert [e(D).unwhiten for D in (30, 256, 257, 383)] == ["blk<16>", "blk<16>", "subst<24>", "subst<24>"]
    assert e(256, False).unwhiten == "subst<16>" and e(256, True, unwhiten_blocked=False).unwhiten == "subst<16>"
    assert e(256, single_launch=False).unwhiten == "subst<16>" and e(258, single_launch=False).unwhiten == "subst<24>"
    assert e(208, False, unwhiten_blocked=True).unwhiten == "blk<16>" and e(208, False, unwhiten_blocked=True).factor == "rank-one"
    # the library's codes
    assert mas.codes(e(126)) == (capi.COMPRESS_PCHOLQR, 1, 1, 1) and mas.codes(e(208)) == (capi.COMPRESS_PCHOLQR, 1, 2, 1)
    assert mas.codes(e(256)) == (capi.COMPRESS_PCHOLQR, 2, 41, 1) and mas.codes(e(352)) == (capi.COMPRESS_PCHOLQR, 3, 44, 3)
    assert mas.codes(e(126, False)) == (capi.COMPRESS_PCHOLQR, 1, 36, 2) and mas.codes(e(384)) == (capi.COMPRESS_TSQR, 0, 0, 0)


def test_every_kernel_family_and_both_sides_of_every_edge_are_present():
    E = {c.id: mas.expected(c.D) for c in mas.CASES}
    assert {x.factor for x in E.values()} == {"blk<4,9,2>", "blk<7,15,4>", "rank-one", None}
    assert {x.gram for x in E.values()} == {"one-pass", "blk", "wide", None}
    assert {x.unwhiten for x in E.values()} == {"blk<16>", "subst<24>", None}  # (k_unwhiten<16>: the legs with a switch of the GPU file)
    assert {x.nb for x in E.values() if x.factor == "rank-one"} == {8, 9, 10, 11, 12}
    assert {x.gram_nt for x in E.values() if x.gram == "one-pass"} == {2, 4, 6, 8, 10, 14, 15, 16}
    nt = {mas.n_tiles(c.D) for c in mas.CASES}
    assert {2, 3, 4, 5, 8, 9, 14, 15, 16, 17, 22, 23, 24, 25} <= nt
    assert {(c.D + 15) // 16 for c in mas.CASES} >= {16, 17}
    # with the blocked factor off: k_gram_pchol<1 .. 7>
    assert {mas.expected(c.D, False).nb for c in mas.CASES if c.D <= 223} == {1, 2, 3, 4, 5, 7}
    assert sum(c.D % 16 == 0 for c in mas.CASES if c.group in ("col", "small")) >= 8


@pytest.mark.parametrize("cid", mas.CASE_IDS)
def test_case_meets_its_conditions(oracle, cid):
    c = mas.BY_ID[cid]
    R = mas.reference(oracle, c)
    ref, prob = R["ref"], c.prob
    assert ref["D"] == c.D == len(R["cols"]) and prob.F <= 24 and int(np.diff(prob.meas_offsets).max()) <= 240
    # the gate: no verdict within GATE_MARGIN of its threshold
    gate = np.isfinite(ref["chi2"])
    assert gate.any()
    margin = np.abs(ref["chi2"][gate] / ref["chi2_thresh"][gate] - 1.0).min()
    assert margin > GATE_MARGIN
    H, r = R["H_emu"], R["r_emu"]
    rel = mas.row_rel_norms(H)
    if c.group == "reject":
        assert R["n_used"] == 0 and (ref["feat_status"] == capi.FEAT_CHI2_REJECTED).all() and ref["rows_comp"] == 0
        assert H.shape == (0, c.D) and R["rank"] == 0 and not ref["dx"].any() and np.array_equal(ref["P"], prob.P)
        return
    assert R["n_used"] >= 1
    if c.group == "rank":
        assert R["n_used"] == prob.F and R["stack_rows"] == c.R == ref["rows_comp"]
    # the rank gap: genuine rows over 1e-5, noise rows under 1e-7, nothing in between; the genuine rank is the whitened triangle's
    assert not ((rel > mas.GAP[0]) & (rel < mas.GAP[1])).any(), np.sort(rel)[:4]
    rank, sv_rank = R["rank"], mas.svd_rank(prob.P, R["cols"], ref["H_comp"])
    assert rank == sv_rank and 1 <= rank <= min(c.D, R["stack_rows"])
    if c.group == "rank":
        assert rank == c.R == H.shape[0]  # the factor stops after R genuine rows
    # the emulated system through the stock EKFUpdate reproduces the oracle's posterior
    st, P1, dx1 = oracle.ekf_update(prob.P, H, r, R["cols"], 1.0)
    eP, edx = _rel(P1, ref["P"]), _rel(dx1, ref["dx"])
    noise = rel[rel <= mas.RANK_REL]
    print(f"{cid}: D {c.D}, {R['n_used']} of {prob.F} features, {R['stack_rows']} stack rows, emulation {H.shape[0]} rows, genuine rank {rank} = SVD rank, "
          f"smallest genuine row {rel[rel > mas.RANK_REL].min():.1e}, largest noise row {noise.max() if noise.size else 0.0:.1e}, gate margin {margin:.1e}, "
          f"P' {eP:.1e}, dx {edx:.1e}")
    assert st == 0 and eP < TOL_P and edx < TOL_DX


def test_rank_rule_sees_a_lost_and_a_spurious_row():
    """The rule on made-up factors: a genuine row lost, a noise row promoted, and noise rows that must not count."""
    rng = np.random.default_rng(5)
    H = rng.normal(size=(6, 10)) * np.array([1.0, 0.5, 0.1, 1e-3, 3e-5, 2e-8])[:, None]
    assert mas.genuine_rank(H) == 5 and mas.genuine_rank(H[:4]) == 4 and mas.genuine_rank(np.zeros((0, 10))) == 0
    H2 = H.copy()
    H2[5] *= 1e3
    assert mas.genuine_rank(H2) == 6
    assert mas.genuine_rank(np.zeros((3, 10))) == 0


def test_the_bounds_see_a_wrong_factor(oracle):
    """What the GPU file's bounds catch, on the emulation of D = 222: the smallest genuine row lost (a factor that stops one pivot early), one
    row's tile column scaled by 1 + 1e-8 (a rank-4 instalment applied to the wrong tile leaves far more), a residual entry off by 1e-8."""
    c = mas.BY_ID["col-222"]
    R = mas.reference(oracle, c)
    H, r, G, g = R["H_emu"], R["r_emu"], R["G"], R["g"]
    assert _rel(H.T @ H, G) < 1e-13 and _rel(H.T @ r, g) < 1e-12  # the emulation itself: two decades under the bounds
    rel = mas.row_rel_norms(H)
    k = int(np.argmin(np.where(rel > mas.RANK_REL, rel, np.inf)))
    lost = np.delete(H, k, axis=0)
    assert mas.genuine_rank(lost) == R["rank"] - 1  # the rank rule sees it, there is no allowance of one
    bad = H.copy()
    bad[0, 16:32] *= 1 + 1e-8
    assert _rel(bad.T @ bad, G) > 1e-11
    rbad = r.copy()
    rbad[0] *= 1 + 1e-8
    assert _rel(H.T @ rbad, g) > 1e-10
