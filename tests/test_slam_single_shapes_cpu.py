"""The batches of tests/test_gpu_slam_single.py on the oracle alone (no GPU): every one of them must hold what it is named for BEFORE it
travels — a single-depth feature the update uses, a single-depth feature the gate rejects where an outlier or a multiplier was planted, the
track length and the column position in its name — and no statistic within parity_util.GATE_MARGIN of its threshold, so that the GPU file
compares accept sets with no excuse.  Also the level-2 rule of "slam_fused" restated in slam_single_shapes against a written-out table, and
include/ovgpu.h."""
import os

import numpy as np
import pytest

import slam_single_shapes as s2
from open_vins_amd import capi

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SINGLE = s2.SINGLE


@pytest.mark.parametrize("cid", [c.id for c in s2.CASES if c.entry == "update"])
def test_gpu_case_is_not_vacuous(oracle, cid):
    case = s2.BY_ID[cid]
    prob = case.prob
    m = np.diff(prob.meas_offsets)
    single = case.reps_observed == SINGLE
    assert prob.F <= 10 and prob.C <= 30
    ref = s2.oracle_run(oracle, case)
    st = ref["feat_status"]
    assert ref["stats"]["status"] == 0
    assert single.any() and ((st == capi.FEAT_USED) & single).any()             # 1. a single-depth feature is used
    if case.outliers or case.rejected is not None:                               # 2. the gate rejects a SINGLE-DEPTH feature where one was planted
        assert ((st == capi.FEAT_CHI2_REJECTED) & single).any()
    if case.rejected is not None:
        assert single[case.rejected] and st[case.rejected] == capi.FEAT_CHI2_REJECTED and (st == capi.FEAT_CHI2_REJECTED).sum() == 1
    assert ref["near_gate"] == 0                                                 # 3. no verdict within GATE_MARGIN of its threshold
    # a single-depth track of fewer than two observations has no row to give; a 3-dof one of one observation has two
    few = np.where(single, m < 2, m < 1)
    assert np.array_equal(st == capi.FEAT_TOO_FEW_MEAS, few)
    used = st == capi.FEAT_USED
    assert ref["stats"]["n_rows"] == int(np.where(single, 2 * m - 2, 2 * m)[used].sum())  # the projection takes two rows of every single-depth feature
    if case.m_max is not None:                                                   # 4. the named track: single-depth, exactly m_max observations
        f = case.named
        assert single[f] and m[f] == case.m_max
        assert st[f] == (capi.FEAT_USED if case.m_max >= 2 else capi.FEAT_TOO_FEW_MEAS)
        if case.m_max >= 2:
            assert m.max() == case.m_max
    if case.col is not None:                                                     # 5. the named column
        assert single[case.named] and case.column_of(case.named) == case.col
    if case.D is not None:
        assert case.columns == case.D
    assert prob.K * prob.C <= 8192 and case.columns >= 16


def test_what_the_cases_are_named_for(oracle):
    by = s2.BY_ID
    assert (by["single-6"].reps_observed == SINGLE).all() and by["single-6"].prob.F == 6
    assert by["mix"].reps_observed.tolist() == s2.MIX8 and (by["mix"].reps_observed == SINGLE).sum() == 1
    assert by["mix-nofej"].opts().do_fej == 0 and by["mix"].opts().do_fej == 1
    assert by["mix-fisheye"].prob.cam_is_fisheye.all() and not by["mix"].prob.cam_is_fisheye.any()
    # anchors of the single-depth landmarks: observed by their own feature (the anchor block ADDS to the measurement's clone block), and not
    for cid, want in (("anchor-clone-observed", True), ("anchor-clone-unobserved", False)):
        p = by[cid].prob
        assert (by[cid].reps_observed == SINGLE).sum() == 4
        for f in np.flatnonzero(by[cid].reps_observed == SINGLE):
            cl = p.clone_idx[int(p.meas_offsets[f]):int(p.meas_offsets[f + 1])]
            assert bool((cl == p.lm_anchor_clone[p.lm_index[f]]).any()) == want, (cid, f)
    # track lengths: TOO_FEW_MEAS, two stack rows, the gate's "augmented rows share the last tile" edge (6 | 7: 2 m + 4 = 16 | 18), the 16-row
    # tile edge (8 | 9), the 64-row lane edge (32), the bound
    assert s2.TRACKS == [1, 2, 3, 6, 7, 8, 9, 31, 32, 33, 61, 62, 63] and s2.BOUND == 62
    for m in s2.TRACKS:
        c = by[f"len-{m}"]
        lens = np.diff(c.prob.meas_offsets)
        assert lens[0] == m and (lens == 0).sum() == 1 and c.reps_observed[0] == SINGLE
        assert c.kernel2 == (5 if m <= s2.BOUND else 0)
        assert (c.rejected is not None) == (m >= 12)
    for m in (9, 62, 63):
        c = by[f"len-{m}-last"]
        assert np.diff(c.prob.meas_offsets)[-1] == m and c.reps_observed[-1] == SINGLE
    ref = s2.oracle_run(oracle, by["len-62"])
    assert sorted(set(ref["feat_status"].tolist())) == [capi.FEAT_USED, capi.FEAT_TOO_FEW_MEAS, capi.FEAT_CHI2_REJECTED]
    assert s2.oracle_run(oracle, by["len-2"])["stats"]["n_rows"] == 2 + 3 * 4 + 2  # the named track gives two rows
    # columns: the last of a 64-column block (and D - 1), the first of the next
    a, b = by["col-63-last"], by["col-64-first"]
    assert a.column_of(a.named) == 63 == a.columns - 1 and b.column_of(b.named) == 64 and b.columns == 68
    assert a.prob.C == b.prob.C == 10 and a.prob.K == b.prob.K == 1 and a.opts().do_calib_camera_pose == 0 and a.opts().do_calib_camera_intrinsics == 0
    # noise: the options differ between features, and the single-depth feature is rejected by its multiplier alone
    c = by["noise"]
    assert len(set(c.sigma.tolist())) == 8 and len(set(c.mult.tolist())) > 5 and c.reps_observed[s2.NOISE_F] == SINGLE
    ref = s2.oracle_run(oracle, c)
    ones = c.mult.copy()
    ones[s2.NOISE_F] = 1.0
    alt = oracle.slam_update(c.opts(), capi.Views(c.prob), feat_sigma=c.sigma, feat_chi2mult=ones)
    assert ref["feat_status"][s2.NOISE_F] == capi.FEAT_CHI2_REJECTED and alt["feat_status"][s2.NOISE_F] == capi.FEAT_USED
    assert ref["chi2"][s2.NOISE_F] == alt["chi2"][s2.NOISE_F]
    # fall-backs
    for cid in ("fb-general", "fb-tsqr", "fb-mode-a", "len-63", "len-63-last"):
        assert by[cid].kernel2 == 0 and (by[cid].reps_observed == SINGLE).any(), cid
    # chunks: FIRST_5 on the six representations in turn puts a single-depth landmark in every non-empty chunk
    reps = s2.chunk_problem().lm_rep_each
    for k in range(5):
        a, b = s2.FIRST_5[k], s2.FIRST_5[k + 1]
        assert a == b or (reps[a:b] == SINGLE).any()


def test_level_two_rule_is_the_documented_table():
    """expected_kernel2 against the terms include/ovgpu.h lists for "slam_fused", written out"""
    R5, S = s2.ss.REPS5, SINGLE
    table = [  # reps, m_max, D, K, C, level, general, gram_route -> kernel
        (R5 + [S], 60, 238, 2, 30, 2, 0, True, 5),
        ([S], 60, 238, 2, 30, 2, 0, True, 5),
        (R5, 60, 238, 2, 30, 2, 0, True, 4),          # no single-depth landmark observed: k_slam_y<false> at either level
        (R5, 60, 238, 2, 30, 1, 0, True, 4),
        (R5 + [S], 60, 238, 2, 30, 1, 0, True, 0),    # level 1: the whole batch stays
        (R5 + [S], 60, 238, 2, 30, 0, 0, True, 0),    # off
        (R5, 60, 238, 2, 30, 0, 0, True, 0),
        (R5 + [S], 62, 238, 2, 30, 2, 0, True, 5),
        (R5 + [S], 63, 238, 2, 30, 2, 0, True, 0),    # the bound
        ([S], 1, 238, 2, 30, 2, 0, True, 5),
        (R5 + [S], 60, 238, 2, 30, 2, 1, True, 0),    # no_fast_feature_kernel
        (R5 + [S], 60, 238, 2, 30, 2, 0, False, 0),   # TSQR / mode A / the Householder repeat
        ([S], 10, 15, 1, 2, 2, 0, True, 0),           # D >= 16
        ([S], 10, 16, 1, 2, 2, 0, True, 5),
        (R5 + [S], 40, 383, 1, 60, 2, 0, True, 5),
        (R5 + [S], 40, 384, 1, 60, 2, 0, True, 0),    # beyond the Gram route
        (R5 + [S], 40, 300, 9, 1000, 2, 0, True, 0),  # K C <= 8192
        (R5 + [S], 40, 300, 8, 1024, 2, 0, True, 5),
    ]
    for reps, m, D, K, C, level, gen, gram, want in table:
        assert s2.expected_kernel2(reps, m, D, K, C, level, gen, gram) == want, (m, D, K, C, level, gen, gram)
    assert {c.kernel2 for c in s2.CASES if c.group in ("rep", "col", "noise")} == {5}
    assert {c.kernel_at(1) for c in s2.CASES} == {0} and {c.kernel_at(0) for c in s2.CASES} == {0}
    assert {c.kernel2 for c in s2.CASES if c.group == "fb"} == {0}
    # at level 1 the rule is slam_shapes' own
    for c in s2.ss.CASES:
        p = c.prob
        reps = np.asarray(p.lm_rep_each if getattr(p, "lm_rep_each", None) is not None else np.full(len(p.lm_value), p.lm_rep))[p.lm_index]
        gram = c.gram_route and c.entry == "update" and c.options.get("compress_route", capi.COMPRESS_GRAM) != capi.COMPRESS_TSQR
        assert s2.expected_kernel2(reps, c.longest_track, c.columns, p.K, p.C, 1, c.options.get("no_fast_feature_kernel", 0), gram) == c.kernel, c.id


def test_header_documents_the_levels_and_kernel_five():
    txt = open(os.path.join(ROOT, "include", "ovgpu.h")).read()
    at = txt.index('"slam_fused"              (default 0)')
    para = txt[at:txt.index('"slam_fused_batches"', at)]
    for term in ("level", "1:", "2:", "k_slam_y<true>", "single-depth", "62", "16 <= D", "K C <= 8192", "no_fast_feature_kernel", "whitened"):
        assert term in para, term
    at = txt.index('"last_feature_kernel"     (read only)')
    assert "5 " in txt[at:at + 600] and "k_slam_y<true>" in txt[at:at + 600]
