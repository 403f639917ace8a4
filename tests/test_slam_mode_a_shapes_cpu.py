"""The batches of tests/test_gpu_slam_mode_a.py on the oracle alone (no GPU): every one must hold what it is named for BEFORE it travels — a
feature the update uses (except where every feature is to be rejected), the planted outlier rejected, no statistic within
parity_util.GATE_MARGIN of its threshold, the column count and the rows of the stack in its name — and the float64 emulation of mode A on the
oracle's stack (mode_a_shapes.emulate) must leave mode_a_shapes.GAP empty: no row of the un-whitened factor between 1e-7 and 1e-5 of the largest.
That is what keeps the GPU file's rank assertion honest: the genuine rank written out below is a property of the batch, not of a kernel.
Also the dispatch rule restated in slam_mode_a_shapes against written-out tables, and include/ovgpu.h."""
import hashlib
import os
import re

import numpy as np
import pytest

import mode_a_shapes as mas
import slam_mode_a_shapes as sma
from open_vins_amd import capi

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
T, P = capi.COMPRESS_TSQR, capi.COMPRESS_PCHOLQR

# case id -> (columns, rows of the oracle's stack, genuine rank of the emulation): written out, from the oracle alone
EXPECT = {
    "col-63": (63, 20, 20),
    "col-64": (64, 36, 36),
    "col-127": (127, 202, 111),
    "col-128": (128, 230, 112),
    "col-223": (223, 746, 207),
    "col-224": (224, 618, 208),
    "col-255": (255, 638, 229),
    "col-257": (257, 794, 233),
    "col-300": (300, 836, 273),
    "col-360": (360, 860, 310),
    "col-383": (383, 786, 328),
    "wide-384": (384, 542, 240),
    "wide-385": (385, 480, 331),
    "wide-399": (399, 456, 292),
    "wide-400": (400, 534, 293),
    "wide-448": (448, 586, 361),
    "wide-449": (449, 638, 273),
    "wide-496": (496, 640, 392),
    "wide-511": (511, 794, 341),
    "rows-2-3dof": (223, 2, 2),
    "rows-2-single": (223, 2, 2),
    "rows-14-511": (511, 14, 14),
    "rows-16-511": (511, 16, 16),
    "rows-18-511": (511, 18, 18),
    "rows-30-511": (511, 30, 30),
    "rows-32-511": (511, 32, 32),
    "rows-34-511": (511, 34, 34),
    "rows-long-272": (272, 872, 231),
    "rep-0": (226, 638, 213),
    "rep-1": (226, 638, 213),
    "rep-2": (226, 692, 213),
    "rep-3": (226, 510, 213),
    "rep-4": (226, 510, 213),
    "rep-5": (214, 498, 201),
    "rep-mix": (234, 932, 221),
    "rep-mix-nofej": (238, 936, 225),
    "rep-fisheye": (238, 1056, 225),
    "noise": (238, 990, 222),
    "single-resident-unobserved": (230, 770, 216),
    "active-narrow": (223, 574, 210),
    "active-120": (226, 716, 213),
    "reject-223": (223, 0, 0),
    "empty-223": (223, 0, 0),
    "fused-3dof-62": (266, 158, 74),
    "fused-3dof-63": (266, 160, 74),
    "fused-3dof-126": (266, 286, 74),
    "fused-3dof-127": (266, 288, 74),
    "fused-single-62": (262, 156, 138),
    "fused-single-63": (262, 158, 139),
    "fused-single-126": (262, 284, 169),
    "fused-single-127": (262, 286, 169),
}


@pytest.mark.parametrize("cid", sma.CASE_IDS)
def test_gpu_case_is_not_vacuous(oracle, cid):
    case = sma.BY_ID[cid]
    prob = case.prob
    m = np.diff(prob.meas_offsets)
    R = sma.reference(oracle, case)
    ref, st = R["ref"], R["ref"]["feat_status"]
    rel = mas.row_rel_norms(R["H_emu"])
    gap = rel[(rel > mas.GAP[0]) & (rel < mas.GAP[1])]
    print(f'    "{cid}": ({case.columns}, {R["stack_rows"]}, {R["rank"]}),   # used {R["n_used"]} of {prob.F}, emulation rows {R["H_emu"].shape[0]}, '
          f'in the gap {gap.size}, near a gate {R["near_gate"]}')
    assert ref["stats"]["status"] == 0
    assert prob.F <= 12 and m.max() <= (40 if case.group in ("col", "wide", "rows", "reject") else (127 if case.group == "fused" else 62))
    if case.D is not None:
        assert case.columns == case.D
    assert R["cols"].size == case.columns
    if case.group == "reject":
        assert R["n_used"] == 0 and R["stack_rows"] == 0 and R["rank"] == 0
    else:
        assert R["n_used"] >= 1                                                # a feature is used
    if case.outlier is not None:
        assert st[case.outlier] == capi.FEAT_CHI2_REJECTED                     # the planted outlier is rejected
    assert R["near_gate"] == 0                                                 # no verdict within GATE_MARGIN of its threshold
    assert np.array_equal(st[m == 0], np.full((m == 0).sum(), capi.FEAT_TOO_FEW_MEAS))
    assert gap.size == 0, (cid, gap)                                           # the rank rule's gap is empty
    assert R["rank"] <= min(R["stack_rows"], case.columns)
    if case.rows is not None:
        assert R["stack_rows"] == case.rows
    assert EXPECT[cid] == (case.columns, R["stack_rows"], R["rank"])


def test_what_the_cases_are_named_for(oracle):
    by = sma.BY_ID
    # six to twelve landmarks, one gross outlier, tracks of at most 40 observations at every column edge
    for c in sma.CASES:
        if c.group in ("col", "wide") and c.D not in (63, 64):
            assert 6 <= len(c.prob.lm_value) <= 12 and c.outlier is not None, c.id
    # both sides of every dispatch edge: tile columns of [H | r]
    nt = {D: mas.n_tiles(D) for D in (63, 64, 127, 128, 223, 224, 255, 257, 360, 383)}
    assert nt == {63: 4, 64: 5, 127: 8, 128: 9, 223: 14, 224: 15, 255: 16, 257: 17, 360: 23, 383: 24}
    assert [mas.n_tiles(D) for D in sma.WIDE_D] == [25, 25, 25, 26, 29, 29, 32, 32]
    # short stacks: 2 rows from one 3-dof landmark with one observation, and from one single-depth landmark with two
    c = by["rows-2-3dof"]
    assert c.prob.F == 1 and np.diff(c.prob.meas_offsets).tolist() == [1] and c.reps_observed[0] != sma.SINGLE
    c = by["rows-2-single"]
    assert c.prob.F == 1 and np.diff(c.prob.meas_offsets).tolist() == [2] and c.reps_observed[0] == sma.SINGLE
    # every SLAM feature stacks an even number of rows: the panel and tile edges are bracketed by even counts
    for rows in (14, 16, 18, 30, 32, 34):
        c = by[f"rows-{rows}-511"]
        R = sma.reference(oracle, c)
        seen = np.diff(c.prob.meas_offsets) > 0   # the two tracks with observations are 3-dof landmarks' (2 m rows each)
        assert c.columns == 511 and R["stack_rows"] == rows == R["rank"] and seen.sum() == 2 and not (c.reps_observed[seen] == sma.SINGLE).any()
    R = sma.reference(oracle, by["rows-long-272"])
    assert R["stack_rows"] > 272 and len(by["rows-long-272"].prob.lm_value) == 12
    # representations and options
    assert {int(by[f"rep-{r}"].reps[0]) for r in sma.ss.REPS5 + [sma.SINGLE]} == set(sma.ss.REPS5) | {sma.SINGLE}
    assert (by["rep-mix"].reps == sma.SINGLE).sum() == 2 and by["rep-mix-nofej"].opts().do_fej == 0
    assert by["rep-fisheye"].prob.cam_is_fisheye.all()
    c = by["single-resident-unobserved"]
    assert (c.reps == sma.SINGLE).sum() == 1 and not (c.reps_observed == sma.SINGLE).any() and c.columns == 208 + 3 * 7 + 1
    c = by["active-narrow"]
    assert len(c.prob.lm_value) == 10 and c.columns == 208 + 15
    c = by["active-120"]
    assert len(c.prob.lm_value) == 120 and c.columns == 208 + 18
    c = by["noise"]
    assert len(set(np.asarray(c.sigma).tolist())) == 10
    R = sma.reference(oracle, c)
    assert not np.array_equal(R["H_stack"], R["ref"]["H"])   # the reference stack is the oracle's scaled to sigma_pix
    # the fused stage: both sides of both bounds, without and with a single-depth landmark observed
    for kind, single in (("3dof", False), ("single", True)):
        for m in (62, 63, 126, 127):
            c = by[f"fused-{kind}-{m}"]
            assert c.longest_track == m and bool((c.reps_observed == sma.SINGLE).any()) == single


def test_the_rule_is_the_documented_table():
    """expected_codes against values worked by hand from include/ovgpu.h (not from the catalogue): (route, Gram, factor, un-whitening)"""
    table = [  # D, level, wide, keywords -> codes
        (63, 1, 0, {}, (P, 1, 1, 1)),
        (127, 1, 0, {}, (P, 1, 1, 1)),            # 8 tile columns: k_gram_pchol_blk<4, 9, 2>
        (128, 1, 0, {}, (P, 1, 2, 1)),            # 9: <7, 15, 4>
        (223, 1, 0, {}, (P, 1, 2, 1)),
        (224, 1, 0, {}, (P, 1, 32 + 8, 1)),       # 15: the rank-one factor, NB = ceil(225 / 32)
        (255, 1, 0, {}, (P, 1, 32 + 8, 1)),
        (255, 1, 0, dict(single_launch=False), (P, 1, 32 + 8, 2)),
        (257, 1, 0, {}, (P, 2, 32 + 9, 6)),       # 17: k_gram_blk, k_unwhiten_blk<24> on the two-panel tiles
        (257, 1, 0, dict(two_panel=False), (P, 2, 32 + 9, 7)),
        (257, 1, 0, dict(unwhiten_blocked=False), (P, 2, 32 + 9, 7)),
        (300, 1, 0, {}, (P, 2, 32 + 10, 6)),
        (360, 1, 0, {}, (P, 3, 32 + 12, 6)),      # 23: k_gram_wide
        (383, 1, 0, {}, (P, 2, 32 + 12, 6)),
        (383, 1, 0, dict(two_panel=False), (P, 2, 32 + 12, 7)),
        (383, 0, 0, {}, (T, 0, 0, 0)),            # the switch
        (383, 0, 1, {}, (T, 0, 0, 0)),
        (383, 1, 0, dict(compress_route=T), (T, 0, 0, 0)),
        (383, 1, 0, dict(fp32=1), (T, 0, 0, 0)),
        (383, 1, 0, dict(whiten=False), (T, 0, 0, 0)),
        (383, 1, 0, dict(prior_ok=False), (T, 0, 0, 0)),
        (384, 1, 0, {}, (T, 0, 0, 0)),            # beyond 383 columns "mode_a_wide" has to be in force as well
        (384, 1, 1, {}, (P, 2, 3, 4)),
        (384, 0, 1, {}, (T, 0, 0, 0)),
        (511, 1, 1, {}, (P, 2, 3, 4)),
        (511, 1, 1, dict(two_panel=False), (P, 2, 3, 5)),
        (511, 1, 1, dict(fp32=1), (T, 0, 0, 0)),
    ]
    for D, level, wide, kw, want in table:
        assert sma.expected_codes(D, level, wide, **kw) == want, (D, level, wide, kw)
    R5, S = sma.ss.REPS5, sma.SINGLE
    kernels = [  # reps, m_max, D, fused, level, wide -> "last_feature_kernel"
        (R5, 40, 300, 0, 1, 0, 0), (R5, 40, 300, 1, 1, 0, 4), (R5, 40, 300, 1, 0, 0, 0), (R5 + [S], 40, 300, 1, 1, 0, 0), (R5 + [S], 40, 300, 2, 1, 0, 5),
        (R5, 62, 266, 3, 1, 0, 4), (R5, 63, 266, 2, 1, 0, 0), (R5, 63, 266, 3, 1, 0, 6), (R5 + [S], 126, 262, 3, 1, 0, 7), (R5, 127, 266, 3, 1, 0, 0),
        (R5, 40, 400, 1, 1, 0, 0), (R5, 40, 400, 1, 1, 1, 4),
    ]
    for reps, m, D, fused, level, wide, want in kernels:
        assert sma.expected_feature_kernel(reps, m, D, 4, 30, fused, level, wide) == want, (m, D, fused, level, wide)


def test_header_names_the_switch_and_exports_nothing_new():
    txt = open(os.path.join(ROOT, "include", "ovgpu.h")).read()
    for name in ('"slam_mode_a"', '"slam_mode_a_compressions"', "k_unwhiten_blk<24>", 'Likewise the debug option "slam_mode_a"'):
        assert name in txt, name
    at = txt.index(' *   "slam_mode_a" ')
    assert "default 0" in txt[at:at + 200] and "values above 1 are taken as 1" in txt[at:at + 200]
    at = txt.index(' *   "slam_mode_a_compressions"')
    assert "read only" in txt[at:at + 200]
    assert re.search(r"6 k_unwhiten_blk<24> on the\s+\*\s+two-panel factorisation's inverse tiles, 7 k_unwhiten_blk<24> on k_uinv_tiles'", txt)
    assert "#define OVGPU_ABI_VERSION 10" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = sorted(set(re.findall(r"\b(ovgpu_[a-z0-9_]+)\s*\(", code)))
    assert len(names) == 89   # the export list of ABI 10 as it stood: a debug option is a string, not a symbol
    assert hashlib.sha256("\n".join(names).encode()).hexdigest() == "c40493705335313fa5fa8dc7ec8ab7cd82e84766e5b0cb96dabab1d01a74051f"
