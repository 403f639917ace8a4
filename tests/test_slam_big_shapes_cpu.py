"""The batches of tests/test_gpu_slam_big.py on the oracle alone (no GPU): every one of them must hold what it is named for BEFORE it travels — a
feature the update uses, the planted outlier rejected, the track length and the column count in its name — and no statistic within
parity_util.GATE_MARGIN of its threshold, so that the GPU file compares accept sets with no excuse.  Also the rule of "slam_fused_big" restated in
slam_big_shapes against a written-out table, the pass plan's edges, the kernel's LDS carve (csrc/k_slam_y_big.h) compiled into a stand-alone
host program, and include/ovgpu.h."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import slam_big_shapes as sb
from open_vins_amd import capi

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SINGLE = sb.SINGLE
LDS_LIMIT = 163840


@pytest.mark.parametrize("cid", [c.id for c in sb.CASES if c.entry == "update"])
def test_gpu_case_is_not_vacuous(oracle, cid):
    case = sb.BY_ID[cid]
    prob = case.prob
    m = np.diff(prob.meas_offsets)
    single = case.reps_observed == SINGLE
    assert prob.F <= 10
    ref = sb.oracle_run(oracle, case)
    st = ref["feat_status"]
    assert ref["stats"]["status"] == 0
    assert (st == capi.FEAT_USED).any()                                          # 1. a feature is used
    if case.rejected is not None:                                                # 2. the planted outlier, and nothing else, is rejected
        planted = sorted((case.rejected,) + tuple(case.also_rejected))
        assert np.flatnonzero(st == capi.FEAT_CHI2_REJECTED).tolist() == planted
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
    by = sb.BY_ID
    # 126: level 3's bound; 127: the first big track; 128: 256 rows, a full last tile; 129: two live rows in the last tile; both sides of every change
    # in the number of passes; the 28th | 29th tile row; the bound and one beyond it
    assert sb.PASS_EDGES == [168, 169, 208, 209]
    assert sb.TRACKS == [126, 127, 128, 129, 168, 169, 208, 209, 224, 225, 232, 233] and sb.BOUND_BIG == 232 and sb.BOUND_LONG == 126
    assert [sb.n_passes(m) for m in (127, 168, 169, 208, 209, 232)] == [2, 2, 3, 3, 4, 4]
    assert sb.n_passes(120) == 1 and sb.n_passes(121) == 2 and sb.n_passes(5) == 1   # a short track of a big batch: one pass up to 15 tile rows
    assert (2 * 224 + 15) // 16 == 28 and (2 * 225 + 15) // 16 == 29 and (2 * 232 + 15) // 16 == 29 and (2 * 233 + 15) // 16 == 30
    assert by["len-3dof-232"].columns == 372 and by["len-single-232"].columns == 368          # rig A: calibration columns off
    assert by["rig-b-3dof"].columns == 374 and by["rig-b-single"].columns == 370              # rig B: configs[4]'s 50 x 4 with calibration
    for kind in ("3dof", "single"):
        want = 9 if kind == "single" else 8
        for m in sb.TRACKS:
            c = by[f"len-{kind}-{m}"]
            lens = np.diff(c.prob.meas_offsets)
            assert lens[0] == m and (lens == 0).sum() == 1
            assert (c.reps_observed[0] == SINGLE) == (kind == "single") and (c.reps_observed == SINGLE).sum() == (2 if kind == "single" else 0)
            assert c.kernel_big == ((want - 2) if m <= 126 else (want if m <= 232 else 0))
            assert c.kernel_at(3, 0) == ((want - 2) if m <= 126 else 0) and c.kernel_at(2, 1) == 0
        for m in sb.BOTH_ENDS:
            c = by[f"len-{kind}-{m}-last"]
            assert np.diff(c.prob.meas_offsets)[-1] == m and (c.reps_observed[-1] == SINGLE) == (kind == "single")
        c = by[f"outlier-big-{kind}"]
        ref = sb.oracle_run(oracle, c)
        assert ref["feat_status"][0] == capi.FEAT_CHI2_REJECTED and ref["chi2"][0] > 20 * ref["chi2_thresh"][0]
        assert np.diff(c.prob.meas_offsets)[0] == 232 and c.kernel_big == want
        c = by[f"beyond-{kind}"]
        assert np.diff(c.prob.meas_offsets).tolist()[:2] == [233, 128] and c.kernel_big == 0
        assert min(by[f"all-big-{kind}"].lengths) == 127 and by[f"all-big-{kind}"].kernel_big == want
        assert min(by[f"stride-{kind}"].lengths) == 2 and max(by[f"stride-{kind}"].lengths) == 230 and by[f"stride-{kind}"].kernel_big == want
        assert by[f"rig-b-{kind}"].kernel_big == want and by[f"rig-b-{kind}"].prob.C == 50 and by[f"rig-b-{kind}"].prob.K == 4
        assert by[f"short-60-{kind}"].kernel_big == want - 4 and by[f"short-100-{kind}"].kernel_big == want - 2
    ref = sb.oracle_run(oracle, by["len-3dof-232"])
    assert sorted(set(ref["feat_status"].tolist())) == [capi.FEAT_USED, capi.FEAT_TOO_FEW_MEAS, capi.FEAT_CHI2_REJECTED]
    # columns: 383 = 12 blocks of 32 with one column short of the last; 384 leaves the Gram route unless "gram_wide" is on
    assert by["col-383"].columns == 383 and by["col-383"].kernel_big == 8 and not (by["col-383"].reps_observed == SINGLE).any()
    assert by["col-384"].columns == 384 and by["col-384"].kernel_big == 0 and by["col-384"].kernel_at(3, 1, max_d=511) == 9
    assert (np.diff(by["col-383"].prob.meas_offsets) == 200).sum() == 2 and by["col-383"].prob.F == 9
    c = by["noise"]
    assert len(set(c.sigma.tolist())) == 6 and len(set(c.mult.tolist())) >= 5 and c.kernel_big == 9
    for cid in ("fb-general", "fb-tsqr", "fb-semi-definite", "mode-a-3dof", "mode-a-single"):
        assert by[cid].kernel_big == 0 and by[cid].longest_track == 200, cid
    lens = np.diff(sb.chunk_problem().meas_offsets)
    assert lens[0:3].min() > 126 and lens[3:6].min() > 126 and sb.CHUNK_FIRST == [0, 3, 3, 6]


def test_rule_is_the_documented_table():
    """expected_kernel_big against the terms include/ovgpu.h lists for "slam_fused_big", written out"""
    R5, S = sb.ss.REPS5, SINGLE
    table = [  # reps, m_max, D, K, C, level, big, general, gram_route -> kernel
        (R5, 126, 372, 4, 59, 3, 1, 0, True, 6),          # up to 126: level 3's shapes
        (R5 + [S], 126, 372, 4, 59, 3, 1, 0, True, 7),
        (R5, 127, 372, 4, 59, 3, 1, 0, True, 8),          # the first big track
        (R5 + [S], 127, 372, 4, 59, 3, 1, 0, True, 9),
        (R5, 232, 372, 4, 59, 3, 1, 0, True, 8),          # the bound
        (R5 + [S], 232, 372, 4, 59, 3, 1, 0, True, 9),
        (R5, 233, 372, 4, 59, 3, 1, 0, True, 0),          # beyond it
        (R5 + [S], 233, 372, 4, 59, 3, 1, 0, True, 0),
        (R5, 127, 372, 4, 59, 3, 0, 0, True, 0),          # big = 0 at 127
        (R5 + [S], 127, 372, 4, 59, 3, 0, 0, True, 0),
        (R5, 127, 372, 4, 59, 2, 1, 0, True, 0),          # level 2 with big = 1 at 127
        (R5 + [S], 127, 372, 4, 59, 2, 1, 0, True, 0),
        (R5, 127, 372, 4, 59, 0, 1, 0, True, 0),
        (R5, 127, 372, 4, 59, 3, 9, 0, True, 8),          # every value above 1 is taken as 1
        (R5, 60, 372, 4, 59, 3, 1, 0, True, 4),           # the lower levels keep their meaning
        (R5 + [S], 60, 372, 4, 59, 3, 1, 0, True, 5),
        (R5, 100, 372, 4, 59, 2, 1, 0, True, 0),
        (R5, 200, 372, 4, 59, 3, 1, 1, True, 0),          # no_fast_feature_kernel
        (R5, 200, 372, 4, 59, 3, 1, 0, False, 0),         # TSQR / mode A without "slam_mode_a" / the Householder repeat
        ([S], 200, 15, 1, 2, 3, 1, 0, True, 0),           # D >= 16
        ([S], 200, 16, 1, 2, 3, 1, 0, True, 9),
        (R5, 200, 383, 4, 50, 3, 1, 0, True, 8),
        (R5 + [S], 200, 384, 4, 50, 3, 1, 0, True, 0),    # beyond the Gram route
        (R5, 200, 300, 9, 1000, 3, 1, 0, True, 0),        # K C <= 8192
        (R5, 200, 300, 8, 1024, 3, 1, 0, True, 8),
    ]
    for reps, m, D, K, C, level, big, gen, gram, want in table:
        assert sb.expected_kernel_big(reps, m, D, K, C, level, big, gen, gram) == want, (m, D, K, C, level, big, gen, gram)
    assert sb.expected_kernel_big(R5 + [S], 200, 384, 4, 50, 3, 1, 0, True, max_d=511) == 9
    # with the switch off, and on every batch of at most 126 observations, the rule is slam_long_shapes' own on its catalogue
    for c in sb.s3.CASES:
        gram = c.gram_route and c.entry == "update" and c.options.get("compress_route", capi.COMPRESS_GRAM) != capi.COMPRESS_TSQR
        for level in (0, 1, 2, 3):
            for big in (0, 1):
                got = sb.expected_kernel_big(c.reps_observed, c.longest_track, c.columns, c.prob.K, c.prob.C, level, big, c.options.get("no_fast_feature_kernel", 0), gram)
                if c.longest_track <= 126 or not (big and level >= 3):
                    assert got == c.kernel_at(level), (c.id, level, big)


# --------------------------------------------------------------------------- the carve
@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("no hipcc (k_slam_y_big.h includes the HIP runtime's header)")
    exe = str(tmp_path_factory.mktemp("slamyb") / "slamyb_layout_main")
    build = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-Wno-unused-variable",
                            "-Wno-pass-failed", "-I", os.path.join(ROOT, "open_vins_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tests", "host", "slamyb_layout_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "slamyb layout ok" in run.stdout, run.stdout + run.stderr
    out = dict(carve={}, parts={})
    for ln in run.stdout.splitlines():
        w = ln.split()
        if w[0] == "consts":
            out["consts"] = tuple(int(x) for x in w[1:])
        elif w[0] == "carve":
            out["carve"][(int(w[1]), int(w[2]))] = dict(nt=int(w[3]), total=int(w[4]), holds=int(w[5]))
        elif w[0] == "parts":
            out["parts"][int(w[1])] = [int(x) for x in w[2:]]
        elif w[0] == "ws":
            out["ws"] = (int(w[1]), int(w[2]))
    return out


def test_carve_fits_at_the_bound_and_the_tile_rows_stop_the_next_length(layout):
    mmax, nt_b, tpw, nw, pf = layout["consts"]
    assert mmax == sb.BOUND_BIG >= 200 and nt_b == (2 * mmax + 15) // 16 and nw * tpw == sb.PASS_TILES
    for proj in (0, 1):
        at = layout["carve"][(mmax, proj)]
        assert at["nt"] == nt_b and at["total"] <= LDS_LIMIT and at["holds"] == 1
        assert layout["carve"][(200, proj)]["holds"] == 1 and layout["carve"][(127, proj)]["holds"] == 1
        over = layout["carve"][(mmax + 1, proj)]   # over the limit, or one tile row more than a fetched panel's prefetch registers hold
        assert over["holds"] == 0 and (over["total"] > LDS_LIMIT or over["nt"] > nt_b)
        assert (over["nt"] + 1) * 256 > pf * 64 * nw or over["total"] > LDS_LIMIT
    assert (nt_b + 1) * 256 <= pf * 64 * nw
    # by hand: the block of Y 16 x 29 x 34 doubles, V[:, 0:2] 16 x 29 x 2, the stage 4096, the right-hand sides 16 x 29 x 4, the instance lists
    # 29 x 32 ints, hq 512, 64 bytes of flags
    for proj, vl in ((0, 0), (1, 16 * 29 * 2 * 8)):
        yb, vlo, wpart, rhs, inst, hq, misc, total = layout["parts"][proj]
        assert (yb, vlo, wpart - vlo) == (0, 126208, vl)
        assert (rhs - wpart, inst - rhs, hq - inst, misc - hq, total - misc) == (4096, 14848, 3712, 512, 64)
        assert total == 149440 + vl and total % 16 == 0 and all(o % 16 == 0 for o in (vlo, wpart, rhs, inst, hq, misc))
    assert layout["ws"] == (29, 29 * 30 * 256)
    for (m, proj), at in layout["carve"].items():   # monotone in the track length: the host's check of the longest track covers the shorter ones
        assert at["total"] <= layout["carve"][(mmax + 1, proj)]["total"]


def test_header_documents_the_switch_and_the_kernel_codes():
    txt = open(os.path.join(ROOT, "include", "ovgpu.h")).read()
    at = txt.index('"slam_fused_big"          (default 0)')
    para = txt[at:txt.index('"slam_fused_batches"      counter', at)]
    for term in ("level", "1 and every value above is taken as 1", '"slam_fused" is at 3', "127 to 232", "SLY_MMAX_B", "k_slam_y_big", "16 <= D", "K C <= 8192",
                 "no_fast_feature_kernel", "whitened", "8 without, 9 with", "126", "233", "ovgpu_slam_update_chunked", '"slam_mode_a"', '"gram_wide"',
                 "ovgpu_set_features"):
        assert term in para, term
    at = txt.index('"slam_fused"              (default 0)')
    assert "values above 3 are taken as 3" in txt[at:txt.index('"slam_fused_big"', at)]
    at = txt.index('"last_feature_kernel"     (read only)')
    para = txt[at:txt.index('"sys_lds_limit"', at)]
    for term in ("8 / 9", "k_slam_y_big<true>", "232", '"slam_fused_big" = 1'):
        assert term in para, term
    hdr = open(os.path.join(ROOT, "open_vins_amd", "csrc", "k_slam_y_big.h")).read()
    assert "constexpr int SLY_MMAX_B = 232;" in hdr
