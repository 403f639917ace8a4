"""The batches of tests/test_gpu_gram_wide.py on the oracle alone (no GPU): every one of them must hold what it is named for BEFORE it travels —
the column count, the tile, window and block counts and the longest track in its name, a feature the update uses and the planted outlier
rejected — and no statistic within parity_util.GATE_MARGIN of its threshold, so that the GPU file compares accept sets with no excuse.  Also
the rules restated in gram_wide_shapes against written-out tables, the clone window beyond 64 poses, and include/ovgpu.h."""
import os

import numpy as np
import pytest

import gram_wide_shapes as gw
from open_vins_amd import capi, synth
from parity_util import GATE_MARGIN

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SINGLE = gw.SINGLE
G, T = capi.COMPRESS_GRAM, capi.COMPRESS_TSQR


def test_the_clone_window_holds_85_poses():
    """states of up to 85 clones: the window beyond 64 poses continues the fixture's at 10 Hz"""
    short, long_ = synth.load_traj_window(), synth.load_traj_window(85)
    assert short.shape == (64, 8) and long_.shape == (85, 8)
    assert np.abs(long_[:64] - short).max() < 1e-8          # (the fixture is the same rows printed to nine decimals)
    assert np.abs(np.diff(long_[:, 0]) - 0.1).max() < 2e-3
    assert np.abs(np.linalg.norm(long_[:, 4:8], axis=1) - 1.0).max() < 1e-6
    assert max(st["C"] for st in list(gw.MSCKF_STATES.values()) + list(gw.KERNEL_STATES.values()) + list(gw.SLAM_STATES.values())) <= 85


# --------------------------------------------------------------------------- the MSCKF batches
@pytest.mark.parametrize("cid", [c.id for c in gw.MSCKF_CASES])
def test_msckf_case_is_not_vacuous(oracle, cid):
    case = gw.MSCKF_BY_ID[cid]
    prob = case.prob
    m = np.diff(prob.meas_offsets)
    assert prob.F <= 12
    assert case.D == gw.ts.n_columns(prob.C, prob.K, case.state.get("pose", 1), case.state.get("intr", 1))  # 1. the column count
    assert m.max() == case.longest_track == case.m_max                                                               # 2. the longest track
    if case.group != "c":
        assert m.max() <= 40
    if case.lengths is not None:
        assert m.tolist() == list(case.lengths)
    tri, ref = gw.msckf_oracle_run(oracle, case)
    st, chi2, thr = ref["feat_status"], ref["chi2"], ref["chi2_thresh"]
    assert ref["stats"]["status"] == 0 and ref["stats"]["D"] == case.D
    assert ((m == m.max()) & (st == capi.FEAT_USED)).any()                                                           # 3. ... is used
    assert st[case.rejected] == capi.FEAT_CHI2_REJECTED and (st == capi.FEAT_CHI2_REJECTED).sum() == 1               # 4. the planted outlier alone is rejected
    gate = np.isfinite(chi2)
    assert gate.sum() >= 5 and np.abs(chi2[gate] / thr[gate] - 1.0).min() > GATE_MARGIN                              # 5. no verdict near its threshold
    assert np.array_equal(st[m < 2], np.full((m < 2).sum(), capi.FEAT_TOO_FEW_MEAS))


def test_msckf_cases_are_what_they_are_named_for():
    by = gw.MSCKF_BY_ID
    # D -> (tile columns, windows, tiles of the fourth window, blocks of 64, columns of the last, blocks of 32, columns of the last)
    table = {382: (24, 3, 0, 6, 62, 12, 30), 384: (25, 4, 1, 6, 64, 12, 32), 386: (25, 4, 1, 7, 2, 13, 2), 398: (25, 4, 1, 7, 14, 13, 14),
             400: (26, 4, 2, 7, 16, 13, 16), 416: (27, 4, 3, 7, 32, 13, 32), 448: (29, 4, 5, 7, 64, 14, 32), 450: (29, 4, 5, 8, 2, 15, 2),
             480: (31, 4, 7, 8, 32, 15, 32), 482: (31, 4, 7, 8, 34, 16, 2), 496: (32, 4, 8, 8, 48, 16, 16), 498: (32, 4, 8, 8, 50, 16, 18),
             510: (32, 4, 8, 8, 62, 16, 30)}
    assert sorted(table) == sorted(gw.MSCKF_STATES)
    for D, want in table.items():
        c = by[f"a-{D}"]
        got = (gw.tiles(D), gw.windows(D), gw.fourth_window_tiles(D), gw.blocks(D, 64), gw.last_block_columns(D, 64), gw.blocks(D, 32), gw.last_block_columns(D, 32))
        assert c.D == D and got == want, (D, got)
        assert c.kernel_at(1) == 1 and c.kernel_at(0) == (1 if D <= 383 else 0)
        assert c.gram_at(1) and c.gram_at(0) == (D <= 383) and c.wide_at(1) == (D >= 384) and not c.wide_at(0)
    for D in (384, 510):
        for m, k in gw.KERNEL_TRACKS.items():
            c = by[f"c-{D}-{m}"]
            assert c.D == D and c.prob.K == 4 and c.kernel_at(1) == k and c.kernel_at(0) == 0
        assert by[f"c-{D}-general"].kernel_at(1) == 0 and by[f"c-{D}-general"].wide_at(1)
    assert gw.KERNEL_TRACKS == {62: 1, 63: 2, 126: 2, 127: 3}
    # what must not move: off the wide route with the switch on; the step-wise Cholesky stays on it
    for cid in ("d-tsqr-400", "d-fp32-400", "d-compress-384", "d-semi-definite-400"):
        assert not by[cid].wide_at(1) and not by[cid].gram_at(1) and by[cid].kernel_at(1) == 0, cid
    assert by["d-stepwise-400"].wide_at(1) and by["d-stepwise-400"].kernel_at(1) == 1
    P = by["d-semi-definite-400"].prob.P
    assert np.linalg.eigvalsh(P)[:6].max() < 1e-12 * np.linalg.eigvalsh(P)[-1] and np.linalg.eigvalsh(by["a-400"].prob.P)[0] > 0
    assert [by[c].D for c in gw.HYGIENE_CHAIN] == [510, 208, 448]


# --------------------------------------------------------------------------- the SLAM batches
@pytest.mark.parametrize("cid", [c.id for c in gw.SLAM_CASES if c.entry == "update"])
def test_slam_case_is_not_vacuous(oracle, cid):
    case = gw.SLAM_BY_ID[cid]
    prob = case.prob
    m = np.diff(prob.meas_offsets)
    assert prob.F <= 12 and case.columns == case.D                                # 1. the column count
    if case.m_max is not None:                                                    # 2. the long track, on a 3-dof landmark
        assert m.max() == case.m_max == m[0] and case.reps_observed[0] != SINGLE and (m[1:] <= 40).all()
    else:
        assert m.max() <= 40
    ref = gw.slam_oracle_run(oracle, case)
    st = ref["feat_status"]
    assert ref["stats"]["status"] == 0 and ref["stats"]["D"] == case.D
    assert (st == capi.FEAT_USED).any() and ref["near_gate"] == 0                 # 3. a feature is used, no verdict near its threshold
    if case.rejected is not None:                                                 # 4. the planted outlier alone is rejected
        assert st[case.rejected] == capi.FEAT_CHI2_REJECTED and (st == capi.FEAT_CHI2_REJECTED).sum() == 1 and case.reps_observed[case.rejected] != SINGLE
    single = case.reps_observed == SINGLE
    used = st == capi.FEAT_USED
    assert ref["stats"]["n_rows"] == int(np.where(single, 2 * m - 2, 2 * m)[used].sum())


def test_slam_cases_are_what_they_are_named_for():
    by = gw.SLAM_BY_ID
    # D -> (tile columns, tiles of the fourth window, blocks of 64, columns of the last, blocks of 32, columns of the last)
    table = {384: (25, 1, 6, 64, 12, 32), 385: (25, 1, 7, 1, 13, 1), 399: (25, 1, 7, 15, 13, 15), 400: (26, 2, 7, 16, 13, 16), 401: (26, 2, 7, 17, 13, 17),
             447: (28, 4, 7, 63, 14, 31), 448: (29, 5, 7, 64, 14, 32), 449: (29, 5, 8, 1, 15, 1), 495: (31, 7, 8, 47, 16, 15), 496: (32, 8, 8, 48, 16, 16),
             497: (32, 8, 8, 49, 16, 17), 510: (32, 8, 8, 62, 16, 30), 511: (32, 8, 8, 63, 16, 31)}
    assert sorted(table) == sorted(gw.SLAM_STATES)
    for D, want in table.items():
        c = by[f"b-{D}"]
        got = (gw.tiles(D), gw.fourth_window_tiles(D), gw.blocks(D, 64), gw.last_block_columns(D, 64), gw.blocks(D, 32), gw.last_block_columns(D, 32))
        assert c.columns == D and got == want, (D, got)
        assert (c.reps_observed == SINGLE).sum() == gw.SLAM_STATES[D]["b"] >= 1
        assert c.kernel_wide(1) == 0 and c.wide_at(1) and not c.gram_at(0)       # "slam_fused" = 0: k_system_t with L
    assert gw.FUSED_D == {385: 63, 449: 100, 511: 126}
    for D, m in gw.FUSED_D.items():
        want = {"fused-single": 5, "fused-3dof": 4, "long-single": 7, "long-3dof": 6}
        for tag, k in want.items():
            c = by[f"b-{D}-{tag}"]
            assert c.columns == D and c.kernel_wide(1) == k and c.kernel_wide(0) == 0, (D, tag)
            assert (c.reps_observed == SINGLE).any() == tag.endswith("single")
            assert c.longest_track == (m if tag.startswith("long") else min(40, c.longest_track))
    assert by["d-383"].columns == 383 and by["d-383"].gram_at(0) and by["d-383"].gram_at(1) and not by["d-383"].wide_at(1)
    assert not by["d-compress-384"].gram_at(1)
    p = gw.over_the_bound()
    reps = np.asarray(p.lm_rep_each)
    assert gw.ts.n_columns(p.C, p.K) + int(np.where(reps == SINGLE, 1, 3).sum()) == 512
    full, per_chunk = gw.chunk_columns()
    assert full == 444 and per_chunk == [422, 422, 424] and gw.CHUNK_FIRST == [0, 4, 8, 12]
    q = gw.chunk_problem()
    assert q.F == 12 and np.diff(q.meas_offsets).max() <= 40


def test_chunks_on_the_oracle(oracle):
    """the three chunks chained on the oracle: features used in every chunk, nothing near its threshold"""
    import test_gpu_slam_chunked as sc
    q = gw.chunk_problem()
    q.lm_index = np.arange(q.F, dtype=np.int32)
    ref = sc.oracle_chain(oracle, capi.default_options(chi2_multipler=1.0), q, gw.CHUNK_FIRST)
    assert ref["near_gate"] == 0 and min(ref["n_used"]) >= 2


# --------------------------------------------------------------------------- the rules against written-out tables
def test_route_rule_is_the_documented_table():
    table = [  # D, wide, compress_route, fp32, prior_ok, entry -> (Gram route, counted by "gram_wide_updates")
        (383, 0, G, 0, True, "update", True, False), (383, 1, G, 0, True, "update", True, False),
        (384, 0, G, 0, True, "update", False, False), (384, 1, G, 0, True, "update", True, True),
        (511, 1, G, 0, True, "update", True, True), (511, 0, G, 0, True, "update", False, False),
        (512, 1, G, 0, True, "update", False, False),
        (400, 1, T, 0, True, "update", False, False), (208, 1, T, 0, True, "update", False, False),
        (400, 1, G, 1, True, "update", False, False), (300, 1, G, 1, True, "update", True, False),   # gram_fp32: the switch is ignored
        (400, 1, G, 0, False, "update", False, False),                                                   # the Householder repeat
        (400, 1, G, 0, True, "compress", False, False), (208, 1, G, 0, True, "compress", False, False),  # mode A is not the update's route
    ]
    for D, wide, route, fp32, prior, entry, gram, counted in table:
        kw = dict(compress_route=route, fp32=fp32, prior_ok=prior, entry=entry)
        assert gw.takes_gram_route(D, wide, **kw) == gram and gw.takes_wide_route(D, wide, **kw) == counted, (D, wide, route, fp32, prior, entry)
    assert gw.tiles(383) == 24 and gw.tiles(384) == 25 and gw.tiles(511) == 32 and gw.windows(383) == 3 and gw.windows(384) == 4
    assert [gw.fourth_window_tiles(D) for D in (383, 384, 399, 400, 495, 496, 511)] == [0, 1, 1, 2, 7, 8, 8]


def test_kernel_rules_are_the_documented_tables():
    for m in (2, 62, 63, 126, 127, 232, 233):
        for D in (208, 383):
            assert gw.expected_msckf_kernel(m, D, 0) == gw.expected_msckf_kernel(m, D, 1) == gw.ts.expected_kernel(m)
        for D in (384, 510):
            assert gw.expected_msckf_kernel(m, D, 0) == 0 and gw.expected_msckf_kernel(m, D, 1) == gw.ts.expected_kernel(m)
            assert gw.expected_msckf_kernel(m, D, 1, general=1) == 0 and gw.expected_msckf_kernel(m, D, 1, compress_route=T) == 0
    R5, S = gw.ss.REPS5, SINGLE
    table = [  # reps, m_max, D, level, wide -> kernel
        (R5, 40, 383, 3, 0, 4), (R5, 40, 384, 3, 0, 0), (R5, 40, 384, 3, 1, 4), (R5 + [S], 40, 385, 3, 1, 5), (R5 + [S], 40, 385, 1, 1, 0),
        (R5, 63, 449, 3, 1, 6), (R5 + [S], 126, 511, 3, 1, 7), (R5 + [S], 127, 511, 3, 1, 0), (R5, 63, 449, 2, 1, 0), (R5, 40, 511, 0, 1, 0),
        (R5, 40, 512, 3, 1, 0),
    ]
    for reps, m, D, level, wide, want in table:
        assert gw.expected_slam_kernel(reps, m, D, 2, 60, level, wide) == want, (m, D, level, wide)
    # without the switch the rule is slam_long_shapes' own, on its catalogue
    for c in gw.s3.CASES:
        gram = c.gram_route and c.entry == "update" and c.options.get("compress_route", G) != T
        for level in (0, 1, 2, 3):
            got = gw.expected_slam_kernel(c.reps_observed, c.longest_track, c.columns, c.prob.K, c.prob.C, level, 0, c.options.get("no_fast_feature_kernel", 0),
                                          compress_route=c.options.get("compress_route", G), prior_ok=c.gram_route, entry=c.entry)
            assert got == gw.s3.expected_kernel3(c.reps_observed, c.longest_track, c.columns, c.prob.K, c.prob.C, level, c.options.get("no_fast_feature_kernel", 0), gram), c.id


def test_header_documents_the_switch():
    txt = open(os.path.join(ROOT, "include", "ovgpu.h")).read()
    at = txt.index('"gram_wide"               (default 0)')
    para = txt[at:txt.index('"gram_wide_updates"', at)]
    for term in ("default 0", "384", "511", "float64", "OVGPU_COMPRESS_GRAM", "gram_fp32", "ovgpu_set_features"):
        assert term in para, term
    at = txt.index('"gram_wide_updates"')
    assert "read only" in txt[at:at + 400] and "once per update" in txt[at:at + 400]
    at = txt.index("OVGPU_COMPRESS_GRAM = 0")
    assert "gram_wide" in txt[at:at + 3000]
