"""The batches of tests/test_gpu_slam_long.py on the oracle alone (no GPU): every one of them must hold what it is named for BEFORE it
travels — a feature the update uses, the planted outlier rejected, the track length and the column count in its name — and no statistic within
parity_util.GATE_MARGIN of its threshold, so that the GPU file compares accept sets with no excuse.  Also the level-3 rule of "slam_fused"
restated in slam_long_shapes against a written-out table, and include/ovgpu.h."""
import os

import numpy as np
import pytest

import slam_long_shapes as s3
from open_vins_amd import capi

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SINGLE = s3.SINGLE


@pytest.mark.parametrize("cid", [c.id for c in s3.CASES if c.entry == "update"])
def test_gpu_case_is_not_vacuous(oracle, cid):
    case = s3.BY_ID[cid]
    prob = case.prob
    m = np.diff(prob.meas_offsets)
    single = case.reps_observed == SINGLE
    assert prob.F <= 8
    ref = s3.oracle_run(oracle, case)
    st = ref["feat_status"]
    assert ref["stats"]["status"] == 0
    assert (st == capi.FEAT_USED).any()                                          # 1. a feature is used
    if case.rejected is not None:                                                # 2. the planted outlier, and nothing else, is rejected
        assert st[case.rejected] == capi.FEAT_CHI2_REJECTED and (st == capi.FEAT_CHI2_REJECTED).sum() == 1
    elif not case.outliers:
        assert not (st == capi.FEAT_CHI2_REJECTED).any()
    assert ref["near_gate"] == 0                                                 # 3. no verdict within GATE_MARGIN of its threshold
    few = np.where(single, m < 2, m < 1)
    assert np.array_equal(st == capi.FEAT_TOO_FEW_MEAS, few)
    used = st == capi.FEAT_USED
    assert ref["stats"]["n_rows"] == int(np.where(single, 2 * m - 2, 2 * m)[used].sum())
    if case.lengths is not None:                                                 # 4. the track lengths the case is built with
        assert m.tolist() == list(case.lengths)
    if case.m_max is not None:
        assert m.max() == case.m_max == case.longest_track
    if case.named is not None:                                                   # ... the longest track on a single-depth landmark
        assert single[case.named] and m[case.named] == case.m_max
    if case.D is not None:                                                       # 5. the named column count
        assert case.columns == case.D
    assert prob.K * prob.C <= 8192 and case.columns >= 16


def test_what_the_cases_are_named_for(oracle):
    by = s3.BY_ID
    # the first long length, the lane edge (64 measurements = 128 rows: the second row of 64-lane passes), the tile-row edges (8 measurements per
    # tile row: 72 | 73, 96 | 97), the bound and one beyond it
    assert s3.TRACKS == [63, 64, 65, 72, 73, 95, 96, 97, 125, 126, 127] and s3.BOUND_LONG == 126 and s3.BOUND == 62
    assert by["len-3dof-126"].columns == 266 and by["len-single-126"].columns == 262
    for kind in ("3dof", "single"):
        for m in s3.TRACKS:
            c = by[f"len-{kind}-{m}"]
            lens = np.diff(c.prob.meas_offsets)
            assert lens[0] == m and (lens == 0).sum() == 1
            assert (c.reps_observed[0] == SINGLE) == (kind == "single") and (c.reps_observed == SINGLE).sum() == (2 if kind == "single" else 0)
            assert c.kernel3 == ((7 if kind == "single" else 6) if m <= 126 else 0) and c.kernel_at(2) == 0
        for m in s3.BOTH_ENDS:
            c = by[f"len-{kind}-{m}-last"]
            assert np.diff(c.prob.meas_offsets)[-1] == m and (c.reps_observed[-1] == SINGLE) == (kind == "single")
        c = by[f"outlier-long-{kind}"]
        ref = s3.oracle_run(oracle, c)
        assert ref["feat_status"][0] == capi.FEAT_CHI2_REJECTED and ref["chi2"][0] > 20 * ref["chi2_thresh"][0]
        assert np.diff(c.prob.meas_offsets)[0] == 126
    ref = s3.oracle_run(oracle, by["len-3dof-126"])
    assert sorted(set(ref["feat_status"].tolist())) == [capi.FEAT_USED, capi.FEAT_TOO_FEW_MEAS, capi.FEAT_CHI2_REJECTED]
    assert min(by["all-long"].lengths) == 63 and by["all-long"].kernel3 == 6 and by["all-long-single"].kernel3 == 7
    assert min(by["stride"].lengths) == 2 and max(by["stride"].lengths) == 100 and by["stride"].kernel3 == 6 and by["stride-single"].kernel3 == 7
    # columns: 383 = 12 blocks of 32 with one column short of the last; 384 leaves the Gram route
    assert by["col-383"].columns == 383 and by["col-383"].kernel3 == 6 and not (by["col-383"].reps_observed == SINGLE).any()
    assert by["col-384"].columns == 384 and by["col-384"].kernel3 == 0
    assert (np.diff(by["col-383"].prob.meas_offsets) == 126).sum() == 2
    c = by["noise"]
    assert len(set(c.sigma.tolist())) == 6 and len(set(c.mult.tolist())) >= 5 and c.kernel3 == 7
    assert by["short-3dof"].kernel3 == by["short-3dof"].kernel_at(2) == 4 and by["short-single"].kernel3 == by["short-single"].kernel_at(2) == 5
    for cid in ("fb-general", "fb-tsqr", "fb-mode-a", "fb-semi-definite"):
        assert by[cid].kernel3 == 0 and by[cid].longest_track == 100, cid
    # chunks: both non-empty chunks hold a track beyond 62 observations
    lens = np.diff(s3.chunk_problem().meas_offsets)
    assert lens[0:3].max() > 62 and lens[3:6].max() > 62 and s3.CHUNK_FIRST == [0, 3, 3, 6]


def test_level_three_rule_is_the_documented_table():
    """expected_kernel3 against the terms include/ovgpu.h lists for "slam_fused", written out"""
    R5, S = s3.ss.REPS5, SINGLE
    table = [  # reps, m_max, D, K, C, level, general, gram_route -> kernel
        (R5, 62, 266, 4, 32, 3, 0, True, 4),          # up to 62: the shapes of level 2
        (R5 + [S], 62, 266, 4, 32, 3, 0, True, 5),
        (R5, 63, 266, 4, 32, 3, 0, True, 6),          # the first long track
        (R5 + [S], 63, 266, 4, 32, 3, 0, True, 7),
        (R5, 126, 266, 4, 32, 3, 0, True, 6),         # the bound
        (R5 + [S], 126, 266, 4, 32, 3, 0, True, 7),
        (R5, 127, 266, 4, 32, 3, 0, True, 0),         # beyond it
        (R5 + [S], 127, 266, 4, 32, 3, 0, True, 0),
        (R5, 63, 266, 4, 32, 2, 0, True, 0),          # level 2 at 63
        (R5 + [S], 63, 266, 4, 32, 2, 0, True, 0),
        (R5, 63, 266, 4, 32, 1, 0, True, 0),
        (R5, 126, 266, 4, 32, 0, 0, True, 0),         # off
        (R5, 60, 266, 4, 32, 2, 0, True, 4),          # levels 1 and 2 keep their meaning
        (R5 + [S], 60, 266, 4, 32, 2, 0, True, 5),
        (R5 + [S], 60, 266, 4, 32, 1, 0, True, 0),
        (R5, 60, 266, 4, 32, 1, 0, True, 4),
        (R5, 100, 266, 4, 32, 3, 1, True, 0),         # no_fast_feature_kernel
        (R5, 100, 266, 4, 32, 3, 0, False, 0),        # TSQR / mode A / the Householder repeat
        ([S], 100, 15, 1, 2, 3, 0, True, 0),          # D >= 16
        ([S], 100, 16, 1, 2, 3, 0, True, 7),
        (R5, 126, 383, 4, 51, 3, 0, True, 6),
        (R5 + [S], 126, 384, 4, 51, 3, 0, True, 0),   # beyond the Gram route
        (R5, 100, 300, 9, 1000, 3, 0, True, 0),       # K C <= 8192
        (R5, 100, 300, 8, 1024, 3, 0, True, 6),
    ]
    for reps, m, D, K, C, level, gen, gram, want in table:
        assert s3.expected_kernel3(reps, m, D, K, C, level, gen, gram) == want, (m, D, K, C, level, gen, gram)
    # at levels 0, 1 and 2 the rule is slam_single_shapes' own, on its catalogue and on slam_shapes'
    for c in s3.s2.CASES:
        gram = c.gram_route and c.entry == "update" and c.options.get("compress_route", capi.COMPRESS_GRAM) != capi.COMPRESS_TSQR
        for level in (0, 1, 2):
            assert s3.expected_kernel3(c.reps_observed, c.longest_track, c.columns, c.prob.K, c.prob.C, level, c.options.get("no_fast_feature_kernel", 0), gram) == c.kernel_at(level), c.id
    assert {c.kernel_at(2) for c in s3.CASES if c.group != "short"} == {0}


def test_header_documents_level_three_and_the_long_kernels():
    txt = open(os.path.join(ROOT, "include", "ovgpu.h")).read()
    at = txt.index('"slam_fused"              (default 0)')
    para = txt[at:txt.index('"slam_fused_batches"', at)]
    for term in ("level", "1:", "2:", "3:", "values above 3 are taken as 3", "126", "63", "62", "k_slam_y<true>", "single-depth", "16 <= D", "K C <= 8192",
                 "no_fast_feature_kernel", "whitened"):
        assert term in para, term
    at = txt.index('"last_feature_kernel"     (read only)')
    para = txt[at:txt.index('"sys_lds_limit"', at)]
    for term in ("5 ", "6 ", "7 ", "k_slam_y<true>", "126"):
        assert term in para, term
