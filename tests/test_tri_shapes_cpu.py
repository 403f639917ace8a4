"""The cases of tests/test_gpu_tri_edges.py on the oracle alone (no GPU): every case of tests/tri_shapes.py must reach the rejection clause, the
loop exit or the stride-loop trip it is named for BEFORE it travels, and nothing in it may sit within round-off of a decision — no tested quantity
within THRESHOLD_FLOOR = 1e-6 (relative) of a threshold in force, no counted LM decision margin below DECISION_FLOOR = 1e-10 — so that the GPU file
compares statuses for every feature with no excuse.  oracle.triangulate_trace must give triangulate()'s arrays bit for bit."""
import numpy as np
import pytest

import tri_shapes as t
from open_vins_amd import capi


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _floors(opts, tr, who):
    thr, dec = t.threshold_margins(opts, tr), tr["min_margin"]
    print(f"margins {who}: threshold {thr.min():.2e} decision {dec.min():.2e} structural ties {int(tr['n_structural'].sum())} other exact ties {int(tr['n_exact'].sum())}")
    assert thr.min() >= t.THRESHOLD_FLOOR, (who, int(thr.argmin()), thr.min())
    assert dec.min() >= t.DECISION_FLOOR, (who, int(dec.argmin()), dec.min())
    assert tr["n_exact"].sum() == 0


@pytest.mark.parametrize("cid", [c.id for c in t.CASES])
def test_case_reaches_what_it_is_named_for(oracle, cid):
    case = t.BY_ID[cid]
    out = t.dropped(oracle, cid)  # asserts: at most 2 % of the features, none the case is named for
    prob = t.problem(oracle, cid)
    assert prob.F == case.prob.F - len(out) and prob.F <= 120
    tr = t.oracle_trace(oracle, cid)
    ref = oracle.triangulate(case.opts(), capi.Views(prob))
    for k in ("p_FinA", "p_FinG", "anchor_meas", "status"):
        assert _bits(tr[k], ref[k]), k
    for (kind, name), least in case.claims.items():
        got = t.count(tr, kind, name, oracle)
        print(f"claim {cid}: {kind} {name} {got} (at least {least})")
        assert got >= least, (kind, name, got, least)
    _floors(case.opts(), tr, cid)
    # the trace agrees with the statuses it came with
    rej, st = tr["reject"], tr["status"]
    lin = np.isin(rej, [oracle.REJECT[k] for k in ("cond", "lin_lo", "lin_hi", "lin_nan")])
    gn = np.isin(rej, [oracle.REJECT[k] for k in ("gn_lo", "gn_hi", "baseline", "gn_nan")])
    assert np.array_equal(st == t.TRI_FAILED, lin) and np.array_equal(st == t.GN_FAILED, gn)
    assert np.array_equal(st == t.TOO_FEW, np.diff(prob.meas_offsets) < 2)
    if not case.opts().refine_features:
        assert not gn.any() and not np.isfinite(tr["lam_final"]).any()
    else:  # every refinement that ran is bounded: at most max_runs accepted steps, lam below max_lamda x lam_mult
        ran = np.isfinite(tr["lam_final"])
        assert np.array_equal(ran, (st == t.USED) | (st == t.GN_FAILED))
        assert (tr["n_accept"][ran] <= case.opts().max_runs + 1).all() and (tr["lam_final"][ran] <= case.opts().max_lamda * case.opts().lam_mult).all()


def test_b_is_the_problem_the_cases_say():
    B = t.base()
    m = np.diff(B.meas_offsets)
    assert (B.C, B.K, B.F) == (30, 2, 120) and m.min() >= 5 and m.max() <= 60
    assert all(c.opts().lam_mult > 1 for c in t.CASES)  # every loop the cases enter ends: a NaN cost only multiplies lam up to max_lamda


def test_every_mode_of_every_option_is_a_case(oracle):
    ids = {c.id for c in t.CASES}
    for name, _, per_mode in t.B_CASES:
        assert set(per_mode) == set(t.MODES)
        assert all(f"B-{name}-{mode}" in ids for mode in t.MODES)
    # a moved threshold that the 1-D routine does not have changes nothing there
    a, b = t.oracle_trace(oracle, "B-default-1d-lin"), t.oracle_trace(oracle, "B-max_cond-2000-1d-lin")
    assert _bits(a["p_FinG"], b["p_FinG"]) and _bits(a["status"], b["status"])


def test_loop_exit_cases_in_detail(oracle):
    tr = t.oracle_trace(oracle, "B-max_runs-1-full")
    assert (tr["exit"] == oracle.EXIT["runs"]).all() and (tr["n_accept"] == 1).all()
    tr = t.oracle_trace(oracle, "B-max_lamda-10-full")
    lam = tr["exit"] == oracle.EXIT["lam"]
    assert (tr["n_reject"][lam] >= 1).all() and (tr["lam_final"][lam] >= 10.0).all()  # left after rejected steps, lam at the bound
    tr = t.oracle_trace(oracle, "B-max_lamda-init-full")
    assert (tr["exit"] == oracle.EXIT["not_entered"]).all() and (tr["n_accept"] + tr["n_reject"] == 0).all() and (tr["status"] == t.USED).all()
    lin = t.oracle_trace(oracle, "B-max_lamda-init-lin")
    np.testing.assert_allclose(tr["p_FinA"], lin["p_FinA"], rtol=1e-15)  # a refinement that never steps returns (x / z) / (1 / z), .., 1 / (1 / z): the linear point to an ulp or two
    tr, dflt = t.oracle_trace(oracle, "B-min_dcost-1e-2-full"), t.oracle_trace(oracle, "B-default-full")
    assert (tr["exit"] == oracle.EXIT["dcost"]).all() and (tr["n_accept"] <= dflt["n_accept"]).all()
    assert (tr["n_accept"] < dflt["n_accept"]).sum() >= 60  # the coarser test fires an accepted step earlier than the default one
    # no default-option run ever takes the two exits the cases above are for
    tr = t.oracle_trace(oracle, "B-default-full")
    assert not np.isin(tr["exit"], [oracle.EXIT["runs"], oracle.EXIT["lam"]]).any()


def test_track_lengths(oracle):
    p = t.lengths_problem()
    m = np.diff(p.meas_offsets)
    assert sorted(set(m.tolist())) == t.LENGTHS and m[0] == 0 and m[-1] == 0 and (m[1:-1] == 0).sum() >= 3
    assert p.K == 4 and p.C == 30
    for f in range(p.F):  # every camera's observations contiguous
        cams = [c for c, _, _ in t.camera_runs(p, f)]
        assert len(cams) == len(set(cams))
    for mode in t.MODES:
        st = t.oracle_trace(oracle, f"lengths-{mode}")["status"]
        assert (st[m < 2] == t.TOO_FEW).all() and (st[m >= 2] != t.TOO_FEW).all()
        assert (st[m >= 63] == t.USED).all()  # every trip count of the stride loop — 1, 2, 3 and 4 — ends in an accepted point
        assert st[m == 2][0] != t.TRI_FAILED and st[m == 3][0] == t.USED
    assert {(x + 63) // 64 for x in m.tolist()} == {0, 1, 2, 3, 4}


def test_anchor_rule(oracle):
    p = t.runs_problem()
    assert [tuple(n for _, _, n in t.camera_runs(p, f)) for f in range(p.F)] == t.RUNS
    want = [t.rule_anchor(p, f) for f in range(p.F)]
    for mode in t.MODES:
        assert t.oracle_trace(oracle, f"runs-{mode}")["anchor_meas"].tolist() == want
    off = p.meas_offsets
    rel = [w - int(off[f]) for f, w in enumerate(want)]
    # equal runs: the first; a longer later run: that one; runs that start in one 64-measurement chunk and end in the next, or two chunks on
    assert rel == [2, 6, 6, 0, 129, 69, 63, 127, 128, 73]
    lp = t.lengths_problem()
    tr = t.oracle_trace(oracle, "lengths-full")
    long = np.diff(lp.meas_offsets) >= 2  # (a track of fewer than two observations is refused before an anchor is picked: -1)
    assert tr["anchor_meas"][long].tolist() == [t.rule_anchor(lp, f) for f in np.flatnonzero(long)] and (tr["anchor_meas"][~long] == -1).all()


def test_degenerate_inputs(oracle):
    p = t.degenerate_problem()
    a = int(p.meas_offsets[t.ONE_POSE_F])
    assert len(set(zip(p.cam_idx[a:a + 5].tolist(), p.clone_idx[a:a + 5].tolist()))) == 1 and p.meas_offsets[t.ONE_POSE_F + 1] - a == 5
    n = int(p.meas_offsets[t.NAN_F])
    assert p.meas_offsets[t.NAN_F + 1] - n == 120 and np.isnan(p.uvn.reshape(-1, 2)[n:n + 120]).sum() == 1
    for mode in ("full", "1d", "lin"):
        tr = t.oracle_trace(oracle, f"degenerate-{mode}")
        assert tr["status"][t.ONE_POSE_F] == t.TRI_FAILED
        assert tr["status"][t.NAN_F] == t.TRI_FAILED and tr["reject"][t.NAN_F] == oracle.REJECT["lin_nan"]  # only the isnan clause can reject it
        assert tr["anchor_meas"][t.NAN_F] != n + 70
        others = np.setdiff1d(np.arange(p.F), [t.ONE_POSE_F, t.NAN_F])
        assert (tr["status"][others] == t.USED).all()  # healthy neighbours on both sides


@pytest.mark.parametrize("cid", [c.id for c in t.SEED_CASES])
def test_seeded_case(oracle, cid):
    case = t.SEED_BY_ID[cid]
    prob, pA, an, where = t.seed_setup(oracle, cid)
    ref = t.oracle_refine(oracle, cid)
    for (kind, name), least in case.claims.items():
        got = t.count(ref, kind, name, oracle)
        print(f"claim {cid}: {kind} {name} {got} (at least {least})")
        assert got >= least
    _floors(case.opts(), ref, cid)
    off = prob.meas_offsets
    for f in case.refused:
        g = where[f]
        assert not (off[g] <= an[g] < off[g + 1])
        assert ref["status"][g] == t.TRI_FAILED and ref["anchor_meas"][g] == -1 and np.isnan(ref["p_FinA"][g]).all() and np.isnan(ref["p_FinG"][g]).all()
    for f in case.nan_seed:
        assert ref["status"][where[f]] == t.GN_FAILED and ref["reject"][where[f]] == oracle.REJECT["gn_nan"]
    ok = ref["status"] == t.USED
    assert np.isfinite(ref["p_FinA"][ok]).all() and np.isnan(ref["p_FinA"][~ok]).all() and np.isnan(ref["p_FinG"][~ok]).all()
    accepted_anchor = np.setdiff1d(np.arange(prob.F), [where[f] for f in case.refused])
    assert np.array_equal(ref["anchor_meas"][accepted_anchor], an[accepted_anchor])


def test_seeded_refinement_is_the_second_half_of_triangulation(oracle):
    """Seeded with the linear result and the rule's anchors under default options, refine() gives triangulate()'s accepted points bit for bit."""
    prob, pA, an, _ = t.seed_setup(oracle, "seed-default")
    ref = t.oracle_refine(oracle, "seed-default")
    full = oracle.triangulate(capi.default_options(), capi.Views(prob))
    lin_ok = np.isfinite(pA).all(axis=1)
    assert np.array_equal(ref["status"][lin_ok], full["status"][lin_ok])
    ok = lin_ok & (full["status"] == t.USED)
    assert ok.sum() >= 60 and _bits(ref["p_FinA"][ok], full["p_FinA"][ok]) and _bits(ref["p_FinG"][ok], full["p_FinG"][ok])
    # the first-measurement case really anchors elsewhere
    _, _, an1, _ = t.seed_setup(oracle, "seed-first-measurement")
    prob1 = t.seed_setup(oracle, "seed-first-measurement")[0]
    rule = np.array([t.rule_anchor(prob1, f) for f in range(prob1.F)])
    moved = np.arange(prob1.F) % t.FIRST_MEAS_EVERY == 0
    assert (an1[moved] != rule[moved]).all() and np.array_equal(an1[moved], prob1.meas_offsets[:-1][moved]) and np.array_equal(an1[~moved], rule[~moved])
    assert prob1.F == t.base().F
    # too few measurements: refused before the anchor is looked at
    short = t.lengths_problem()
    r = oracle.refine(capi.default_options(), capi.Views(short), np.ones((short.F, 3)), short.meas_offsets[:-1].astype(np.int32))
    assert (r["status"][np.diff(short.meas_offsets) < 2] == t.TOO_FEW).all()


def test_pose_table_sits_on_the_lds_limit():
    assert 2 * t.LDS_C * t.POSE_BYTES == 163776 <= t.LDS_LIMIT == 163840 < 2 * (t.LDS_C + 1) * t.POSE_BYTES
    assert t.LDS_SHIFT + t.base().C == t.LDS_C
    R, p = t.embedded_pose_table(t.LDS_C, 2)
    Rb, pb = t.camera_poses(t.base())
    assert R.shape == (2 * t.LDS_C, 9) and np.array_equal(R[t.LDS_C + t.LDS_SHIFT + 3].reshape(3, 3), Rb[30 + 3]) and np.array_equal(p[t.LDS_SHIFT], pb[0])
    Rm = R.reshape(-1, 3, 3)
    assert np.abs(Rm @ Rm.transpose(0, 2, 1) - np.eye(3)).max() < 1e-12  # valid rotations everywhere
    q = t.shifted_base()
    assert q.clone_idx.min() >= t.LDS_SHIFT and q.clone_idx.max() < t.LDS_C
