"""The snapshots of tests/test_gpu_mode_a_wide.py on the oracle alone (no GPU), and the panelled factorisation of k_pchol_wide.h restated in numpy
against tools/dev_mode_a_numerics.chol_pivoted.

Every case must be what it is named for BEFORE it travels: the column count, the route and kernel codes written next to it, a used feature, a
factor whose genuine rows and noise rows leave mode_a_shapes.GAP = [1e-7, 1e-5] empty, the genuine rank written next to it, and an emulated (H, r)
that reproduces the oracle's posterior.  The restatement (lazy panel rows, the running diagonal, one Schur step per panel) is run on every case's
whitened Gram matrix at 16 and at 32 pivots per panel: the pivot order of chol_pivoted, and R to rounding.
"""
import numpy as np
import pytest

import mode_a_shapes as mas
import mode_a_wide_shapes as maw
from mode_a_shapes import chol_pivoted
from open_vins_amd import capi

from test_gpu_parity import TOL_DX, TOL_P  # (importing the module needs no GPU)

PCHOL, TSQR = capi.COMPRESS_PCHOLQR, capi.COMPRESS_TSQR
# id: (D, genuine rank); the codes of every one of them with the switch on are (PCHOLQR, 2, 3, 4) — written out below
RANKS = {
    "col-384": (384, 371), "col-386": (386, 373), "col-398": (398, 385), "col-400": (400, 387), "col-416": (416, 403), "col-448": (448, 435),
    "col-450": (450, 437), "col-480": (480, 467), "col-482": (482, 469), "col-496": (496, 483), "col-498": (498, 485), "col-510": (510, 497),
    "mix-384": (384, 244), "mix-400": (400, 244), "mix-450": (450, 244), "mix-510": (510, 245),
    "rank-510-R1": (510, 1), "rank-510-R17": (510, 17), "rank-510-R33": (510, 33),
    "reject-400": (400, 0),
}
# the Schur step's relative rounding: the restatement sums a panel's products in another order than the rank-one updates of chol_pivoted; on a
# factor whose pivots span 1e-15 of the first the rows agree to the pivots' own relative accuracy, eps x (first pivot / pivot) — held at the level
# of the whole factor, |R - R'| / |R|, where 1e-9 is six decades over double rounding and far under any wrong row (a lost row: over 1e-5)
R_TOL = 1e-9
TOL_G = 1e-11  # ... and R^T R over the genuine rows at the bound the device's factor is held to against the oracle's Gram matrix (tests/test_gpu_mode_a_wide.py)


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def test_every_case_is_what_is_written_next_to_it():
    assert sorted(maw.CASE_IDS) == sorted(RANKS)
    for c in maw.CASES:
        assert c.D == RANKS[c.id][0] == 6 * c.state["C"] + 14 * c.state["K"], c.id
        assert maw.expected_codes(c.D, 1) == (PCHOL, 2, 3, 4), c.id
        assert maw.expected_codes(c.D, 0) == (TSQR, 0, 0, 0), c.id
    assert [c.D for c in maw.CASES if c.group == "col"] == [384, 386, 398, 400, 416, 448, 450, 480, 482, 496, 498, 510]
    assert {mas.n_tiles(c.D) for c in maw.CASES} == {25, 26, 27, 29, 31, 32}
    assert {(c.D + 15) // 16 for c in maw.CASES} >= {24, 25, 32}            # un-whitening tile columns: 24 at 384 columns
    assert {(c.D + 31) // 32 for c in maw.CASES} >= {12, 13, 16}            # panels of 32 pivots at most
    assert all(sum(2 * m - 3 for m in lens) == R for R, lens in maw.RANK_LENGTHS.items())


def test_the_rule_by_hand():
    e = maw.expected_codes
    # the edges of the switch: 383 | 384 and 511 | 512 columns, level 0 | 1
    assert e(383, 1) == e(383, 0) == mas.codes(mas.expected(383)) == (PCHOL, 2, 44, 3)
    assert e(384, 0) == (TSQR, 0, 0, 0) and e(384, 1) == (PCHOL, 2, 3, 4) and e(511, 1) == (PCHOL, 2, 3, 4) and e(512, 1) == (TSQR, 0, 0, 0)
    assert e(208, 1) == mas.codes(mas.expected(208)) == (PCHOL, 1, 2, 1)
    # the un-whitening's inverse tiles
    assert e(400, 1, two_panel=False) == (PCHOL, 2, 3, 5) and e(400, 1, unwhiten_blocked=False) == (PCHOL, 2, 3, 5)
    # what stays Householder at every width
    assert e(400, 1, compress_route=capi.COMPRESS_TSQR) == e(400, 1, fp32=1) == e(400, 1, slam=True) == e(400, 1, prior_ok=False) == (TSQR, 0, 0, 0)
    assert maw.takes_wide_route(400, 1) and not maw.takes_wide_route(400, 0) and not maw.takes_wide_route(383, 1) and not maw.takes_wide_route(512, 1)


@pytest.mark.parametrize("cid", maw.CASE_IDS)
def test_case_meets_its_conditions(oracle, cid):
    c = maw.BY_ID[cid]
    R = mas.reference(oracle, c)
    ref, prob = R["ref"], c.prob
    assert ref["D"] == c.D == len(R["cols"]) and prob.F <= 24
    H, r = R["H_emu"], R["r_emu"]
    rel = mas.row_rel_norms(H)
    if c.group == "reject":
        assert R["n_used"] == 0 and (ref["feat_status"] == capi.FEAT_CHI2_REJECTED).all() and ref["rows_comp"] == 0
        assert H.shape == (0, c.D) and R["rank"] == 0 == RANKS[cid][1]
        return
    assert R["n_used"] >= 1                                                  # a feature is used
    assert not ((rel > mas.GAP[0]) & (rel < mas.GAP[1])).any(), np.sort(rel)[:4]   # the gap is empty
    rank = R["rank"]
    assert rank == RANKS[cid][1], (cid, rank)                               # the emulation's genuine rank
    assert rank == mas.svd_rank(prob.P, R["cols"], ref["H_comp"]) and 1 <= rank <= min(c.D, R["stack_rows"])
    if c.group == "rank":
        assert R["n_used"] == prob.F and R["stack_rows"] == c.R == ref["rows_comp"] and rank == c.R
    if c.group == "mix":
        assert rank % maw.PANEL != 0 and rank < c.D - maw.PANEL               # the factor stops inside a panel, panels before the last
    st, P1, dx1 = oracle.ekf_update(prob.P, H, r, R["cols"], 1.0)
    eP, edx = _rel(P1, ref["P"]), _rel(dx1, ref["dx"])
    noise = rel[rel <= mas.RANK_REL]
    print(f"{cid}: D {c.D}, {R['n_used']} of {prob.F} features, {R['stack_rows']} stack rows, emulation {H.shape[0]} rows, genuine rank {rank}, "
          f"smallest genuine row {rel[rel > mas.RANK_REL].min():.1e}, largest noise row {noise.max() if noise.size else 0.0:.1e}, P' {eP:.1e}, dx {edx:.1e}")
    assert st == 0 and eP < TOL_P and edx < TOL_DX


@pytest.mark.parametrize("cid", [c.id for c in maw.CASES if c.group != "reject"])
def test_panelled_factorisation_is_the_pivoted_one(oracle, cid):
    """chol_pivoted_panelled at 16 and 32 pivots per panel against chol_pivoted on the case's whitened Gram matrix: the same pivots in the same
    order, the same number of rows, R to rounding, and R^T R = G."""
    c = maw.BY_ID[cid]
    R = mas.reference(oracle, c)
    G = maw.whitened_gram(c, R)
    D = c.D
    ref = chol_pivoted(G, D, mas.PIVOT_TOL)
    order = maw.chol_pivoted_order(G, D, mas.PIVOT_TOL)
    rows = int((np.abs(ref[:D]).sum(axis=1) > 0).sum())
    assert rows == len(order)
    for nb in (16, 32):
        Rp, piv = maw.chol_pivoted_panelled(G, D, mas.PIVOT_TOL, nb)
        # the genuine rows: the same pivots in the same order.  Behind them the pivots are rounding noise (1e-15 of the first and under): their
        # order is no property of the algorithm, so the count of rows may differ by noise rows, as the device's may from the emulation's
        n = R["rank"]
        assert piv[:n] == order[:n], (cid, nb)
        e = _rel(Rp[:n], ref[:n])
        eG = _rel(Rp[:n].T @ Rp[:n], ref[:n].T @ ref[:n])
        print(f"{cid}, panels of {nb}: {len(piv)} rows ({rows} by chol_pivoted), genuine {n}, |R - R'| / |R| {e:.1e}, |R^T R - R'^T R'| {eG:.1e}")
        assert e < R_TOL and eG < TOL_G
        assert (Rp[len(piv):] == 0).all() and len(piv) >= n


def test_the_restatement_sees_a_schur_step_without_its_last_row():
    """A Schur step that leaves out the panel's last row (the mutation the GPU file is run against) is not a rounding matter: on a random
    positive definite matrix the factor is off by far more than R_TOL."""
    rng = np.random.default_rng(7)
    A = rng.normal(size=(200, 97))
    G = A.T @ A
    good, piv = maw.chol_pivoted_panelled(G, 96, mas.PIVOT_TOL, 32)
    assert len(piv) == 96 and _rel((good[:96].T @ good[:96])[:96], G[:96]) < 1e-12  # (the carried column's own diagonal entry is not factored)
    assert _rel(good, chol_pivoted(G, 96, mas.PIVOT_TOL)) < 1e-11
    bad = good.copy()
    bad[31] = 0.0  # what the trailing matrix misses is this row's outer product
    assert _rel((bad[:96].T @ bad[:96])[:96], G[:96]) > 1e-4
