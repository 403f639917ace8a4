"""The batches of tests/test_gpu_track_edges.py on the oracle alone (no GPU): every one of them must hold what it is named for BEFORE it
travels — a longest track of exactly the intended length that the update USES, a gate that rejects where an outlier was planted, and no
statistic so close to its threshold that two float64 evaluations could decide differently (the GPU tests compare accept sets with no excuse).
Also the helper's own rules: the track picks, and the dispatch table the GPU tests assert."""
import numpy as np
import pytest

import track_shapes as ts
from open_vins_amd import capi, synth


@pytest.mark.parametrize("cid", [c.id for c in ts.CASES])
def test_gpu_case_is_not_vacuous(oracle, cid):
    case = ts.BY_ID[cid]
    prob = case.prob
    m = np.diff(prob.meas_offsets)
    assert prob.F <= 12
    assert m.max() == case.longest_track                                     # 1. the longest track, exactly
    tri, ref = ts.oracle_run(oracle, case)
    st, chi2, thr = ref["feat_status"], ref["chi2"], ref["chi2_thresh"]
    assert ((m == m.max()) & (st == capi.FEAT_USED) & np.isfinite(chi2)).any()  # 2. ... and the update uses one of that length
    if case.outliers:
        assert (st == capi.FEAT_CHI2_REJECTED).any()                         # 3. the gate rejects
    gate = np.isfinite(chi2)
    assert np.abs(chi2[gate] / thr[gate] - 1.0).min() > 1e-6                 # 4. no verdict on a knife's edge
    assert np.array_equal(st[m < 2], np.full((m < 2).sum(), capi.FEAT_TOO_FEW_MEAS))


def test_dispatch_rule_is_the_documented_table():
    """expected_kernel (tile budgets 36 / 136 of the gate's 2 m + 4 rows, 29 tile rows of 2 m) against the ranges README and DESIGN §4.2 give."""
    for m in range(2, 300):
        want = 1 if m <= 62 else 2 if m <= 126 else 3 if m <= 232 else 0
        assert ts.expected_kernel(m) == want, m
        assert ts.expected_kernel(m, general=True) == 0
        assert ts.expected_kernel(m, shape=2) == (2 if m <= 126 else 0)
    assert ts.expected_kernel(1) == ts.expected_kernel(0) == 0
    assert {c.m_max for c in ts.CASES if c.group == "a"} == set(ts.SWEEP)
    for c in ts.CASES:  # a track of m % 8 in {0, 7} puts the augmented rows in a tile row of their own
        if c.m_max and c.m_max % 8 in (0, 7):
            assert (2 * c.m_max + 4 + 15) // 16 == (2 * c.m_max + 15) // 16 + 1


def test_region_rule():
    """region_classes / expected_raw on the states of group (f): the widths the group is named for, and the class tables worked by hand."""
    ntf = {k: (ts.n_columns(s["C"], s["K"], s.get("pose", 1), s.get("intr", 1)) + 16) // 16 for k, s in ts.REGION_STATES.items()}
    assert ntf == dict(nt5=5, nt6=6, nt7=7, nt14=14, nt15=15, nt16=16, D96=7, D144=10, K4=12)
    assert ts.n_columns(14, 2, 1, 0) == 96 and ts.n_columns(24, 1, 0, 0) == 144 and ts.n_columns(60, 4, 0, 0) == 360
    assert [ts.expected_raw(ts.n_columns(s["C"], s["K"], s.get("pose", 1), s.get("intr", 1)), 1) for s in ts.REGION_STATES.values()] == [0, 1, 1, 1, 1, 0, 1, 1, 1]
    cls, n = ts.region_classes(34, 1)  # D = 218: regions end at 60, 92, 124, 156, 188 and D; clone c's block ends at 14 + 6 c + 6
    assert n == 6 and cls.tolist() == [0] * 7 + [1] * 6 + [2] * 5 + [3] * 5 + [4] * 6 + [5] * 5
    cls, n = ts.region_classes(20, 4)  # calibration ends at 56: 56 + 6 > 60, the region of 4 tile columns is dropped; 92, 124, 156 and D = 176
    assert n == 4 and cls.tolist() == [0] * 6 + [1] * 5 + [2] * 5 + [3] * 4
    cls, n = ts.region_classes(24, 1, 0, 0)  # no calibration: 60, 92, 124 and D = 144 (10 tile columns, top 10)
    assert n == 4 and cls.tolist() == [0] * 10 + [1] * 5 + [2] * 5 + [3] * 4
    cls, n = ts.region_classes(16, 1)  # 7 tile columns: top rounded to 8, regions of 4 and 6 below it
    assert n == 3 and cls.tolist() == [0] * 7 + [1] * 6 + [2] * 3
    for cid, want in (("f-K4-oldest", {0}), ("f-K4-newest", {3}), ("f-nt14-newest", {5}), ("f-nt15-oldest", {0})):
        case = ts.BY_ID[cid]
        s = case.state
        cls, _ = ts.region_classes(s["C"], s["K"], s.get("pose", 1), s.get("intr", 1))
        assert set(cls[case.prob.clone_idx].tolist()) == want, cid
    for cid in ("f-K4-one_per_class", "f-nt14-one_per_class", "f-nt15-one_per_class"):
        case = ts.BY_ID[cid]
        s = case.state
        cls, n = ts.region_classes(s["C"], s["K"], s.get("pose", 1), s.get("intr", 1))
        for f in range(case.prob.F):
            a, b = case.prob.meas_offsets[f], case.prob.meas_offsets[f + 1]
            assert sorted(cls[case.prob.clone_idx[a:b]].tolist()) == list(range(n)), (cid, f)


def test_track_picks():
    prob = ts.longest(synth.make_problem(2, C=12, K=2, F=20), 5)
    m0 = np.diff(prob.meas_offsets)
    code = prob.cam_idx.astype(np.int64) * 1000 + prob.clone_idx

    def codes(q, f):
        return (q.cam_idx.astype(np.int64) * 1000 + q.clone_idx)[q.meas_offsets[f]:q.meas_offsets[f + 1]]

    def own(f):
        return code[prob.meas_offsets[f]:prob.meas_offsets[f + 1]]

    q = ts.exact_length(prob, 7, n=4)
    assert np.diff(q.meas_offsets).tolist() == [7, 7, 7, 7, m0[4]]
    assert np.array_equal(codes(q, 0), own(0)[:7]) and np.array_equal(codes(q, 1), own(1)[-7:])       # prefix, suffix
    k = (m0[2] - 1) // 6
    assert np.array_equal(codes(q, 2), own(2)[::k][:7]) and k >= 1                                      # every k-th, from the first on
    assert len(set((codes(q, 3) // 1000).tolist())) == 1                                                 # one camera
    assert np.array_equal(codes(q, 4), own(4))                                                           # untouched
    for f in range(4):  # order kept: camera groups descending, clones ascending inside a group
        c = codes(q, f)
        assert np.all(np.diff(c // 1000) <= 0) and np.all(np.diff(c)[np.diff(c // 1000) == 0] > 0)
    # data travel with the indices
    a = prob.meas_offsets[1] + m0[1] - 7
    assert np.array_equal(q.uv.reshape(-1, 2)[7:14], prob.uv.reshape(-1, 2)[a:a + 7]) and np.array_equal(q.uvn.reshape(-1, 2)[7:14], prob.uvn.reshape(-1, 2)[a:a + 7])
    # beyond the rig: every distinct (camera, clone) pair first, repetition only tops up
    big = ts.exact_length(prob, 40, n=1)
    c = codes(big, 0)
    assert len(c) == 40 > m0[0] and np.array_equal(c[:m0[0]], own(0)) and np.array_equal(c[m0[0]:], np.resize(own(0), 40 - m0[0]))
    # clone ranges
    r = ts.clone_range(prob, 3, 6)
    assert set(r.clone_idx.tolist()) <= {3, 4, 5} and r.M == int(((prob.clone_idx >= 3) & (prob.clone_idx < 6)).sum())
    r = ts.exact_length(prob, 4, clones=(prob.C - 3, prob.C))
    assert r.clone_idx.min() >= prob.C - 3 and np.diff(r.meas_offsets).tolist() == [4] * 5
    # empty and single-observation tracks, and an outlier that moves one track only
    e = ts.with_lengths(prob, [5, 1, 0, None, 2])
    assert np.diff(e.meas_offsets).tolist() == [5, 1, 0, m0[3], 2]
    o = ts.make_outlier(prob, 2, 15.0)
    moved = np.abs(o.uv - prob.uv).reshape(-1, 2).max(axis=1) > 1
    assert moved[prob.meas_offsets[2]:prob.meas_offsets[3]].all() and moved.sum() == m0[2]
    assert (np.abs(o.uvn - prob.uvn).reshape(-1, 2).max(axis=1) > 1e-3)[prob.meas_offsets[2]:prob.meas_offsets[3]].all()
    assert np.array_equal(prob.uv, ts.longest(synth.make_problem(2, C=12, K=2, F=20), 5).uv)  # the source is never modified
