"""The batches of tests/test_gpu_slam_fused.py on the oracle alone (no GPU): every one of them must hold what it is named for BEFORE it
travels — a feature the update uses, a rejection where an outlier was planted, the track length / column count / anchor pattern in its name —
and no statistic within parity_util.GATE_MARGIN of its threshold, so that the GPU file compares accept sets with no excuse.  Also the
eligibility rule of the fused kernel restated in slam_shapes against a written-out table, and include/ovgpu.h."""
import hashlib
import os
import re

import numpy as np
import pytest

import slam_shapes as ss
from open_vins_amd import capi

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.parametrize("cid", [c.id for c in ss.CASES])
def test_gpu_case_is_not_vacuous(oracle, cid):
    case = ss.BY_ID[cid]
    prob = case.prob
    m = np.diff(prob.meas_offsets)
    assert prob.F <= 12 and prob.C <= (60 if case.D in (383, 384) else 30)
    ref = ss.oracle_run(oracle, case)
    st = ref["feat_status"]
    assert ref["stats"]["status"] == 0
    assert (st == capi.FEAT_USED).any()                                   # 1. a feature is accepted
    if case.outliers:
        assert (st == capi.FEAT_CHI2_REJECTED).any()                      # 2. the gate rejects where an outlier was planted
    assert ref["near_gate"] == 0                                          # 3. no verdict within GATE_MARGIN of its threshold
    assert np.array_equal(st[m == 0], np.full((m == 0).sum(), capi.FEAT_TOO_FEW_MEAS))
    if case.m_max is not None:                                            # 4. the longest track, exactly, and the update uses it
        assert m.max() == case.m_max and ((m == m.max()) & (st == capi.FEAT_USED)).any()
    if case.D is not None:
        assert case.columns == case.D
    assert prob.K * prob.C <= 8192 and case.columns >= 16


def test_what_the_cases_are_named_for(oracle):
    by = ss.BY_ID
    # anchors: observed by their own feature in the representation cases (the anchor block ADDS to the measurement's clone block), never in the other
    for cid in ("rep-2", "rep-3", "rep-4", "rep-mix"):
        obs = ss.anchor_is_observed(by[cid].prob)
        assert obs and all(obs), cid
    obs = ss.anchor_is_observed(by["rep-anchor-clone-unobserved"].prob)
    assert len(obs) == 9 and not any(obs)
    c = by["rep-single-depth-resident-unobserved"]
    assert (c.prob.lm_rep_each == ss.SINGLE).sum() == 1 and not (c.prob.lm_rep_each[c.prob.lm_index] == ss.SINGLE).any() and c.columns == 208 + 3 * 7 + 1
    assert by["rep-fisheye"].prob.cam_is_fisheye.all() and not by["rep-mix"].prob.cam_is_fisheye.any()
    assert by["rep-mix-nofej"].opts().do_fej == 0 and by["rep-mix"].opts().do_fej == 1
    assert sorted(set(by["rep-mix"].prob.lm_rep_each.tolist())) == sorted(ss.REPS5)
    # track lengths: both sides of every 16-row tile edge (8 measurements), of the 64-row lane edge (32) and of the bound
    assert ss.TRACKS == [1, 2, 7, 8, 9, 31, 32, 33, 61, 62, 63] and ss.BOUND == 62
    for m in ss.TRACKS:
        c = by[f"len-{m}"]
        lens = np.diff(c.prob.meas_offsets)
        assert lens[0] == m and (lens == 0).sum() == 1 and c.kernel == (4 if m <= ss.BOUND else 0)
    for m in (9, 62, 63):
        assert np.diff(by[f"len-{m}-last"].prob.meas_offsets)[-1] == m
    ref = ss.oracle_run(oracle, by["len-62"])
    assert sorted(set(ref["feat_status"].tolist())) == [capi.FEAT_USED, capi.FEAT_TOO_FEW_MEAS, capi.FEAT_CHI2_REJECTED]
    # columns
    assert [D % 16 for D in (63, 64, 128, 129)] == [15, 0, 0, 1] and set(ss.COLUMN_STATES) == {63, 64, 128, 129, 255, 257, 383, 384}
    assert by["col-383"].kernel == 4 and by["col-384"].kernel == 0
    # noise: the options differ between features, and ONE feature is rejected by its multiplier alone
    c = by["noise"]
    assert len(set(c.sigma.tolist())) == 10 and len(set(c.mult.tolist())) > 5
    ref = ss.oracle_run(oracle, c)
    ones = c.mult.copy()
    ones[ss.NOISE_F] = 1.0
    alt = oracle.slam_update(c.opts(), capi.Views(c.prob), feat_sigma=c.sigma, feat_chi2mult=ones)
    assert ref["feat_status"][ss.NOISE_F] == capi.FEAT_CHI2_REJECTED and alt["feat_status"][ss.NOISE_F] == capi.FEAT_USED
    assert ref["chi2"][ss.NOISE_F] == alt["chi2"][ss.NOISE_F]
    # fall-backs
    for cid in ("fb-single-depth", "fb-general", "fb-tsqr", "fb-mode-a", "fb-semi-definite"):
        assert by[cid].kernel == 0 and by[cid].longest_track <= ss.BOUND, cid
    assert (by["fb-single-depth"].prob.lm_rep_each == ss.SINGLE).sum() == 1
    P = by["fb-semi-definite"].prob.P
    assert np.linalg.eigvalsh(P).min() > -1e-12 * np.abs(P).max() and np.linalg.matrix_rank(P, tol=1e-13 * np.abs(P).max()) == P.shape[0] - 6
    # chunks: FIRST_5 on the six representations in turn puts a single-depth landmark in every non-empty chunk; on the five 3-dof ones in none
    reps = ss.chunk_problem().lm_rep_each
    for k in range(5):
        a, b = ss.FIRST_5[k], ss.FIRST_5[k + 1]
        assert a == b or (reps[a:b] == ss.SINGLE).any()
    assert not (ss.chunk_problem_3dof().lm_rep_each == ss.SINGLE).any()


def test_eligibility_rule_is_the_documented_table():
    """expected_kernel against the terms include/ovgpu.h lists for "slam_fused", written out"""
    R5, S = ss.REPS5, ss.SINGLE
    table = [  # reps, m_max, D, K, C, switch, general, gram_route -> kernel
        (R5, 60, 238, 2, 30, 1, 0, True, 4),
        (R5, 62, 238, 2, 30, 1, 0, True, 4),
        (R5, 63, 238, 2, 30, 1, 0, True, 0),          # the bound
        (R5, 1, 238, 2, 30, 1, 0, True, 4),
        (R5, 0, 238, 2, 30, 1, 0, True, 4),           # a batch of empty tracks still takes the branch
        (R5 + [S], 60, 238, 2, 30, 1, 0, True, 0),    # one single-depth landmark: the whole batch stays
        ([S], 60, 238, 2, 30, 1, 0, True, 0),
        (R5, 60, 238, 2, 30, 0, 0, True, 0),          # the switch
        (R5, 60, 238, 2, 30, 1, 1, True, 0),          # no_fast_feature_kernel
        (R5, 60, 238, 2, 30, 1, 0, False, 0),         # TSQR / mode A / the Householder repeat
        (R5, 10, 15, 1, 2, 1, 0, True, 0),            # D >= 16
        (R5, 10, 16, 1, 2, 1, 0, True, 4),
        (R5, 40, 383, 1, 60, 1, 0, True, 4),
        (R5, 40, 384, 1, 60, 1, 0, True, 0),          # beyond the Gram route
        (R5, 40, 300, 9, 1000, 1, 0, True, 0),        # K C <= 8192
        (R5, 40, 300, 8, 1024, 1, 0, True, 4),
    ]
    for reps, m, D, K, C, sw, gen, gram, want in table:
        assert ss.expected_kernel(reps, m, D, K, C, sw, gen, gram) == want, (m, D, K, C, sw, gen, gram)
    assert {c.kernel for c in ss.CASES if c.group in ("rep", "noise")} == {4}
    assert {c.kernel for c in ss.CASES if c.group == "fb"} == {0}


def test_header_names_the_switch_and_exports_nothing_new():
    txt = open(os.path.join(ROOT, "include", "ovgpu.h")).read()
    for name in ('"slam_fused"', '"slam_fused_batches"', '"last_feature_kernel"'):
        assert name in txt, name
    assert re.search(r'"last_feature_kernel".*?\n.*4 the fused kernel of the SLAM update', txt)
    assert "#define OVGPU_ABI_VERSION 10" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = sorted(set(re.findall(r"\b(ovgpu_[a-z0-9_]+)\s*\(", code)))
    # the export list of ABI 10 as it stood before the switch: a debug option is a string, not a symbol
    assert len(names) == 89
    assert hashlib.sha256("\n".join(names).encode()).hexdigest() == "c40493705335313fa5fa8dc7ec8ab7cd82e84766e5b0cb96dabab1d01a74051f"
    assert "ovgpu_slam_update_fused" not in code and not any("slam_fused" in n for n in names)
