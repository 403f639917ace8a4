"""The batches of tests/test_gpu_mode_a_panel.py on the oracle alone (no GPU), and the rule of tests/mode_a_panel_shapes.py by hand at its edges.

Every case must be what it is named for BEFORE it travels: the column count, a used feature (or none, where it is named for that), a factor whose
genuine rows and noise rows leave mode_a_shapes.GAP = [1e-7, 1e-5] empty, and an emulated (H, r) that reproduces the oracle's posterior — the
conditions of tests/test_mode_a_wide_shapes_cpu.py::test_case_meets_its_conditions.  Then the panelled factorisation the route runs
(mode_a_wide_shapes.chol_pivoted_panelled at 32 pivots per panel) on the case's whitened Gram matrix: the pivots of the genuine rows are
chol_pivoted_order's, the un-whitened factor leaves the gap empty and keeps the emulation's genuine rank, and its largest noise row stays under
half of GAP[0] — the device's rounding has the other half.
"""
import numpy as np
import pytest
import scipy.linalg as sla

import mode_a_panel_shapes as mps
import mode_a_shapes as mas
import mode_a_wide_shapes as maw
import slam_mode_a_shapes as sma
from open_vins_amd import capi

from test_gpu_parity import TOL_DX, TOL_P  # (importing the module needs no GPU)

PCHOL, TSQR = capi.COMPRESS_PCHOLQR, capi.COMPRESS_TSQR
M, S = mps.MSCKF, mps.SLAM


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def test_the_catalogue_is_what_is_written_next_to_it():
    assert [c.D for c in mps.MSCKF_CASES if c.group == "col"] == [224, 254, 256, 258, 300, 318, 320, 350, 352, 366, 368, 382]
    assert [mps.in_band(c.D) for c in mps.MSCKF_CASES if c.group == "col"] == [False, False] + [True] * 10   # 224 and 254: below the edge
    assert {mas.n_tiles(c.D) for c in mps.MSCKF_CASES} >= {15, 16, 17, 20, 21, 23, 24}
    assert [c.R for c in mps.MSCKF_CASES if c.group == "rank"] == [1, 17, 31, 32, 33, 65]
    assert all(sum(2 * m - 3 for m in lens) == R for R, lens in mps.ROWS_LENGTHS.items())
    assert all(sum(2 * m for m in lens) == R for R, lens in mps.SLAM_ROWS_LENGTHS.items())
    assert [c.columns for c in mps.SLAM_CASES if c.group == "col"] == [224, 255, 257, 300, 360, 383, 319]
    assert all(c.columns == c.D for c in mps.SLAM_CASES if c.D is not None) and mps.SLAM_BY_ID["rows-long-272"].columns == 272
    assert [c.id for c in mps.SLAM_CASES if not mps.in_band(c.columns)] == ["col-224", "col-255"]
    assert all(mps.in_band(c.D) for c in mps.MSCKF_CASES if c.group != "col")
    assert not mps.in_band(mps.BELOW.D) and not mps.in_band(mps.ABOVE.D) and not mps.in_band(mps.SLAM_BELOW.columns) and not mps.in_band(208)
    assert "fused-single-127" not in mps.SLAM_BY_ID


def test_the_rule_by_hand():
    e = mps.expected_codes
    for entry in (M, S):
        # 223 | 224: 14 | 15 tile columns, both below the edge: the switch changes nothing
        assert e(223, 0, entry) == e(223, 1, entry) == e(223, 2, entry) == (PCHOL, 1, 2, 1)
        assert e(224, 0, entry) == e(224, 1, entry) == e(224, 2, entry) == (PCHOL, 1, 40, 1)
        # 255 | 256 | 257: the lower edge, 17 tile columns at 256, where the Gram kernel changes; the un-whitening changes at 257
        assert e(255, 0, entry) == e(255, 1, entry) == e(255, 2, entry) == (PCHOL, 1, 40, 1)
        assert e(256, 0, entry) == (PCHOL, 2, 41, 1) and e(256, 1, entry) == e(256, 2, entry) == (PCHOL, 2, 3, 1)
        assert e(257, 1, entry) == e(257, 2, entry) == (PCHOL, 2, 3, 6)
        assert e(257, 1, entry, two_panel=False) == (PCHOL, 2, 3, 7) and e(257, 2, entry, unwhiten_blocked=False) == (PCHOL, 2, 3, 7)
        assert e(256, 1, entry, single_launch=False) == (PCHOL, 2, 3, 2)
        # 383 | 384: the upper edge; beyond it "mode_a_wide" decides and this switch changes nothing
        assert e(383, 1, entry) == e(383, 2, entry) == (PCHOL, 2, 3, 6)
        for level in (0, 1, 2):
            assert e(384, level, entry) == (TSQR, 0, 0, 0) and e(384, level, entry, wide=1) == (PCHOL, 2, 3, 4)
            assert e(511, level, entry, wide=1) == (PCHOL, 2, 3, 4) and e(384, level, entry, wide=1, two_panel=False) == (PCHOL, 2, 3, 5)
        # values above the top level are taken as it
        assert e(300, 7, entry) == e(300, mps.TOP_LEVEL, entry) == (PCHOL, 2, 3, 6)
        # what stays Householder
        for level in (0, 1, 2):
            assert e(300, level, entry, compress_route=capi.COMPRESS_TSQR) == e(300, level, entry, fp32=1) == e(300, level, entry, prior_ok=False) == (TSQR, 0, 0, 0)
            assert e(300, level, entry, whiten=False) == (TSQR, 0, 0, 0)
    # level 0 is the siblings' rule, entry by entry: the un-whitening at 257 .. 383 columns differs between the entries there
    assert e(257, 0, M) == mas.codes(mas.expected(257)) == (PCHOL, 2, 41, 3) and e(257, 0, S) == sma.expected_codes(257, 1) == (PCHOL, 2, 41, 6)
    assert e(383, 0, M) == (PCHOL, 2, 44, 3) and e(383, 0, S) == (PCHOL, 2, 44, 6) and e(360, 1, M) == (PCHOL, 3, 3, 6)
    # ovgpu_slam_compress without "slam_mode_a": Householder whatever this switch says
    assert e(300, 1, S, slam_level=0) == e(300, 2, S, slam_level=0) == (TSQR, 0, 0, 0)
    assert mps.PANEL_MIN_NT == 17 and mps.PANEL_MAX_NT == 24 and mps.PANEL == 32 and mps.TOP_LEVEL == 1
    assert mps.takes_panel(256, 1) and not mps.takes_panel(255, 1) and not mps.takes_panel(384, 1, wide=1) and not mps.takes_panel(300, 0)


def _panelled(label, P, cols, H_stack, r_stack, rank_emu):
    """the four conditions on chol_pivoted_panelled at 32 pivots per panel"""
    D = len(cols)
    G, L = mps.whitened_gram(P, cols, H_stack, r_stack)
    Rp, piv = maw.chol_pivoted_panelled(G, D, mas.PIVOT_TOL, mps.PANEL)
    order = maw.chol_pivoted_order(G, D, mas.PIVOT_TOL)
    assert piv[:rank_emu] == order[:rank_emu], label                       # the pivots of the genuine rows
    Rw = Rp[:len(piv)]
    H = sla.solve_triangular(L, Rw[:, :D].T, lower=True, trans="T").T
    rel = mas.row_rel_norms(H)
    noise = rel[rel <= mas.RANK_REL]
    big = noise.max() if noise.size else 0.0
    print(f"{label}: D {D}, panelled factor {len(piv)} rows, genuine {mas.genuine_rank(H)} (emulation {rank_emu}), largest noise row {big:.1e}")
    assert not ((rel > mas.GAP[0]) & (rel < mas.GAP[1])).any(), (label, np.sort(rel)[:4])   # the gap stays empty
    assert mas.genuine_rank(H) == rank_emu, label                         # the emulation's genuine rank
    assert big < 0.5 * mas.GAP[0], (label, big)                           # the largest noise row: under half of the bound the device is held to


@pytest.mark.parametrize("cid", mps.MSCKF_IDS)
def test_msckf_case_meets_its_conditions(oracle, cid):
    c = mps.MSCKF_BY_ID[cid]
    R = mas.reference(oracle, c)
    ref, prob = R["ref"], c.prob
    assert ref["D"] == c.D == len(R["cols"]) and prob.F <= 24
    H, r = R["H_emu"], R["r_emu"]
    rel = mas.row_rel_norms(H)
    if c.group == "reject":
        assert R["n_used"] == 0 and (ref["feat_status"] == capi.FEAT_CHI2_REJECTED).all() and ref["rows_comp"] == 0
        assert H.shape == (0, c.D) and R["rank"] == 0
        return
    assert R["n_used"] >= 1
    assert not ((rel > mas.GAP[0]) & (rel < mas.GAP[1])).any(), np.sort(rel)[:4]
    rank = R["rank"]
    assert rank == mas.svd_rank(prob.P, R["cols"], ref["H_comp"]) and 1 <= rank <= min(c.D, R["stack_rows"])
    if c.group == "rank":
        assert R["n_used"] == prob.F and R["stack_rows"] == c.R == ref["rows_comp"] and rank == c.R
    st, P1, dx1 = oracle.ekf_update(prob.P, H, r, R["cols"], 1.0)
    eP, edx = _rel(P1, ref["P"]), _rel(dx1, ref["dx"])
    print(f"{cid}: D {c.D}, {R['n_used']} of {prob.F} features, {R['stack_rows']} stack rows, emulation {H.shape[0]} rows, genuine rank {rank}, P' {eP:.1e}, dx {edx:.1e}")
    assert st == 0 and eP < TOL_P and edx < TOL_DX
    _panelled(cid, prob.P, R["cols"], ref["H_comp"], ref["r_comp"], rank)


@pytest.mark.parametrize("cid", mps.SLAM_IDS)
def test_slam_case_meets_its_conditions(oracle, cid):
    c = mps.SLAM_BY_ID[cid]
    R = sma.reference(oracle, c)
    ref, prob = R["ref"], c.prob
    assert len(R["cols"]) == c.columns and R["near_gate"] == 0
    H, r = R["H_emu"], R["r_emu"]
    rel = mas.row_rel_norms(H)
    if c.group == "reject":
        assert R["n_used"] == 0 and H.shape == (0, c.columns) and R["rank"] == 0
        return
    assert R["n_used"] >= 1
    if c.outlier is not None:
        assert ref["feat_status"][c.outlier] == capi.FEAT_CHI2_REJECTED
    assert not ((rel > mas.GAP[0]) & (rel < mas.GAP[1])).any(), np.sort(rel)[:4]
    rank = R["rank"]
    assert rank == mas.svd_rank(prob.P, R["cols"], R["H_stack"]) and 1 <= rank <= min(c.columns, R["stack_rows"])
    if c.rows is not None:
        assert R["stack_rows"] == c.rows == rank
    st, P1, dx1 = oracle.ekf_update(prob.P, H, r, R["cols"], c.opts().sigma_pix ** 2)
    eP, edx = _rel(P1, ref["P"]), _rel(dx1, ref["dx"])
    print(f"slam {cid}: D {c.columns}, {R['n_used']} of {prob.F} features, {R['stack_rows']} stack rows, emulation {H.shape[0]} rows, genuine rank {rank}, P' {eP:.1e}, dx {edx:.1e}")
    assert st == 0 and eP < TOL_P and edx < TOL_DX
    _panelled(f"slam {cid}", prob.P, R["cols"], R["H_stack"], R["r_stack"], rank)
