"""The batches of tests/test_gpu_system_edges.py on the oracle alone (no GPU), and the restated LDS carve of the general per-feature kernel against
a table worked by hand from the terms at the top of csrc/k_system.h.

Every batch must hold what it is named for BEFORE it travels: the track lengths as written, the long track triangulated and gated, one gated
feature accepted and one rejected, the long track rejected where it is the planted outlier, and no statistic within 1e-6 of its threshold (the GPU
tests compare accept sets with no excuse).  The lengths of groups (b) and (d) follow the device's LDS limit, so they are checked at 160 KB and at
64 KB."""
import numpy as np
import pytest

import system_shapes as sy
from open_vins_amd import capi

KB = 1024

# (D, stride, limit): g, m_lds_max at g, r, m_lds_max at r - 1 and at r, first refused length
TABLE = [
    (208, 48, 160 * KB, 78, 77, 295, 2, 81, 1709),
    (208, 72, 160 * KB, 73, 72, 209, 2, 84, 1709),
    (511, 72, 160 * KB, 59, 58, 150, 1, 71, 1224),
    (208, 48, 64 * KB, 36, 34, 83, 2, 42, 480),
    (208, 72, 64 * KB, 32, 30, 59, 2, 43, 480),
]


@pytest.mark.parametrize("row", TABLE)
def test_carve_is_the_table(row):
    D, stride, limit, g, at_g, r, below_r, at_r, refused = row
    assert sy.edges(stride, D, limit) == (g, r)
    assert sy.carve(g - 1, stride, D, limit) == (g - 1, False, False)      # everything resident on the near side
    assert sy.carve(g, stride, D, limit) == (at_g, False, False)
    assert sy.carve(r - 1, stride, D, limit) == (below_r, False, False)
    assert sy.carve(r, stride, D, limit) == (at_r, True, False)
    assert sy.carve(refused - 1, stride, D, limit)[1:] == (True, False) and sy.carve(refused, stride, D, limit)[2]


def test_carve_by_hand():
    """D = 208, stride 48, 160 KB, worked out term by term: at m = 78 the fixed part is 2496 + 29952 + 3744 + 512 + 26624 = 63328 bytes, 100512 are
    left; a track of 77 observations needs 8 (154 x 155 / 2 + 616) = 100408 bytes, one of 78 needs 8 (156 x 157 / 2 + 624) = 102960."""
    assert sy.fixed_bytes(78, 48, 208) == 63328 and 8 * sy.gate_doubles(77) == 100408 and 8 * sy.gate_doubles(78) == 102960
    assert sy.lds_bytes(78, 48, 208, 160 * KB) == 63328 + 100408
    # m = 294: 9408 + 112896 + 14112 + 512 + 26624 = 163552 < 163840, 288 bytes left hold the 208 of a 2-observation track, not the 360 of a 3-observation one
    assert sy.fixed_bytes(294, 48, 208) == 163552 and 8 * sy.gate_doubles(2) == 208 and 8 * sy.gate_doubles(3) == 360
    # m = 295: 9440 + 113280 + 14160 + 512 + 26624 = 164016 >= 163840, the records leave: 9440 + 14160 + 512 + 26624 = 50736
    assert sy.fixed_bytes(295, 48, 208) == 164016 and sy.fixed_bytes(295, 48, 208, False) == 50736
    assert sy.carve(0, 48, 208, 160 * KB) == (0, False, False)  # an empty batch is sized as a 1-observation one
    # m_lds_max is not monotonic in the longest track
    assert sy.carve(77, 48, 208, 160 * KB)[0] == 77 > sy.carve(200, 48, 208, 160 * KB)[0] == 50 > sy.carve(294, 48, 208, 160 * KB)[0] == 2 < sy.carve(295, 48, 208, 160 * KB)[0] == 81


def test_panel_blocks():
    assert [sy.panel_blocks(m) for m in (62, 63, 254, 255, 510, 511)] == [("p2",), ("p8",), ("p8",), ("p8-resident", "rest"), ("p8-resident", "rest"),
                                                                           ("p8-resident", "rest", "rest")]
    assert set(sy.A_LENGTHS) >= {2, 3, 7, 8, 9, 61, 62, 63, 64, 65, 254, 255, 256, 257, 510, 511}


@pytest.mark.parametrize("limit", sy.LIMITS)
@pytest.mark.parametrize("cid", [c.id for c in sy.CASES if c.group in "bd"])
def test_role_edges_exist(cid, limit):
    case = sy.BY_ID[cid]
    g, r = sy.edges(case.row_stride, case.D, limit)
    assert g is not None and r is not None and 2 < g - 1 and g + 1 < r - 1
    m = case.length(limit)
    m_lds, rows_global, refused = case.carve(limit)
    assert not refused
    if isinstance(case.role, str):
        assert (m_lds == m, rows_global) == {"g-1": (True, False), "g": (False, False), "g+1": (False, False), "r-1": (False, False), "r": (False, True)}[case.role]
        nxt = sy.carve(m + 1, case.row_stride, case.D, limit)
        if case.role == "g-1":
            assert nxt[0] < m + 1
        if case.role == "r-1":
            assert nxt[1]
    _, prob, f_long = case.batch(limit)
    lens = np.diff(prob.meas_offsets)
    assert lens.max() == m == lens[f_long]
    if case.role == "r-1":  # both homes of S in one batch
        assert (lens == m_lds).any() and (lens == m_lds + 1).any() and m_lds >= 1


def _limits_of(case):
    return sy.LIMITS if isinstance(case.role, str) else sy.LIMITS[:1]


@pytest.mark.parametrize("cid,limit", [(c.id, lim) for c in sy.CASES for lim in _limits_of(c)])
def test_gpu_case_is_not_vacuous(oracle, cid, limit):
    case = sy.BY_ID[cid]
    clean, prob, f_long = case.batch(limit)
    lens = np.diff(prob.meas_offsets)
    assert prob.F <= 12 and np.array_equal(lens, np.diff(clean.meas_offsets))
    assert lens.max() == case.length(limit) == lens[f_long]   # the track lengths are as written
    tri, ref = sy.oracle_run(oracle, case, limit)
    chi2, thr = ref["chi2"], ref["chi2_thresh"]
    gate = np.isfinite(chi2)
    if tri is not None:
        assert tri["status"][f_long] == 0                                                          # the long track is triangulated ...
    assert gate[f_long]                                                                            # ... and gated
    acc = sy.accepted(case, ref)
    assert (gate & acc).any() and (gate & ~acc).any()                                              # one accepted, one rejected
    assert np.array_equal(acc[gate], chi2[gate] <= thr[gate])
    assert acc[f_long] == (not case.long_rejected)
    assert np.abs(chi2[gate] / thr[gate] - 1.0).min() > 1e-6                                       # no verdict on a knife's edge
    assert not gate[lens < 2].any()
    if case.kind == "slam":
        assert ref["D"] == case.D
    else:
        assert ref.get("D", case.D) == case.D


def test_cross_check_and_chain_batches():
    for limit in sy.LIMITS:
        g, r = sy.edges(48, 208, limit)
        alone, under, over = sy.cross_check_batches(limit)
        n = len(sy.X_SHORTS)
        assert np.diff(alone.meas_offsets).tolist() == sy.X_SHORTS
        assert np.diff(under.meas_offsets).tolist() == sy.X_SHORTS + [r - 1] and np.diff(over.meas_offsets).tolist() == sy.X_SHORTS + [r]
        for q in (under, over):  # the common features are the same features
            k = int(alone.meas_offsets[n])
            assert np.array_equal(q.uv[:2 * k], alone.uv) and np.array_equal(q.clone_idx[:k], alone.clone_idx) and np.array_equal(q.cam_idx[:k], alone.cam_idx)
            assert np.array_equal(q.P, alone.P)
        links = sy.chain_links(limit)
        assert [(k, s) for k, _, _, (s, _) in links] == [("msckf", 48), ("slam", 72), ("msckf", 48), ("msckf", 48)]
        for kind, _, prob, (stride, m) in links:
            assert np.diff(prob.meas_offsets).max() == m
        D48 = 110
        assert sy.carve(links[0][3][1], 48, D48, limit)[0] == links[0][3][1] and sy.carve(links[2][3][1], 48, D48, limit)[0] < links[2][3][1]
        assert sy.carve(links[1][3][1], 72, D48 + 18, limit)[1] and links[3][3][1] == 9
