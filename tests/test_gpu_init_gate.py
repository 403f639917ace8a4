"""GPU tests (`-m gpu`) of level 2 of ovgpu_debug_option "delayed_init_fused" (csrc/k_init_fused.h): ovgpu_slam_delayed_init_fused with the
gate-free k_init_rows as the step's first launch and the gate decided in k_initf_tail_gate, from the residual the step's own factorisation
carries.  Every batch of tests/init_gate_shapes.py runs at level 2 against

  (a) the oracle's slam_delayed_init,
  (b) a second context of the same library at level 1 (the default: k_system_t decides the gate ahead of the step),

both through tests/test_gpu_delayed_init_fused.py's _check, imported with its bounds: chi2 1e-7, chi2_thresh 1e-12, values 1e-8 / 1e-10, FEJ
1e-12, dx_seq 1e-6, P 1e-7, P symmetric to 1e-13 of its largest entry, poses 1e-9; feat_status, lm_cov_id, N, anchors and landmark slots identical
across the three.  tests/test_init_gate_shapes_cpu.py holds every batch, on the oracle alone, further than GATE_MARGIN from every threshold
(asserted again in _oracle) and to the planted outliers being the only rejections.  "delayed_init_rows_steps" counts the candidates that took the
level-2 step: every case asserts it, so every case fails on a library without the level.

Worst deviations over the catalogue, measured on the MI355X (every case prints its own, test_zz_worst_deviations the maxima): against the oracle
chi2 8.9e-14, dx_seq 5.5e-13, P 4.9e-14, values 1.3e-12, poses 1.7e-13; against the level-1 context chi2 2.4e-12, dx_seq 1.7e-13, P 1.5e-14, values
3.4e-13, poses 1.7e-13 ("The delayed initialisation's gate from the chain's own factor").
"""
import numpy as np
import pytest

import init_gate_shapes as g
from open_vins_amd import capi
from test_gpu_delayed_init_fused import _check, _oracle, _run, _rel, Case, GATE_MARGIN, M_MAX, SINGLE

pytestmark = pytest.mark.gpu

OUT_KEYS = ("feat_status", "chi2", "chi2_thresh", "lm_cov_id", "lm_value", "lm_fej", "anchor_cam", "anchor_clone", "dx_seq", "P")
STATE_KEYS = ("P", "clone_q_p", "calib_q_p", "intrinsics")
WORST = {}  # (comparator, quantity) -> the largest deviation over the cases run so far
L2 = {"delayed_init_fused": 2}


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _run2(Updater, case, tri, fused=True, debug=L2):
    """_run with the level-2 counter next to the other two: (context, out, post, landmarks, (fused, chain, rows))."""
    dbg = dict(debug or {})
    dbg["delayed_init_rows_steps"] = 0
    up, out, post, lm, steps = _run(Updater, case, tri, fused, debug=dbg)
    return up, out, post, lm, steps + (up.debug_option("delayed_init_rows_steps"),)


def _note(tag, out, ref, post, ref_post, gate):
    acc = ref["lm_cov_id"] >= 0
    d = {"chi2": float(np.abs(out["chi2"][gate] / ref["chi2"][gate] - 1.0).max(initial=0.0)),
         "dx_seq": _rel(out["dx_seq"], ref["dx_seq"]) if ref["dx_seq"].any() else float(np.abs(out["dx_seq"]).max(initial=0.0)),
         "P": _rel(out["P"], ref["P"]),
         "values": float(np.abs(out["lm_value"][acc] - ref["lm_value"][acc]).max(initial=0.0)),
         "poses": max(float(np.abs(post[k] - ref_post[k]).max()) for k in ("clone_q_p", "calib_q_p", "intrinsics"))}
    for k, v in d.items():
        WORST[(tag, k)] = max(WORST.get((tag, k), 0.0), v)
    print(f"{tag}: " + "  ".join(f"{k} {v:.3e}" for k, v in d.items()))


def _three2(Updater, oracle, shape, want=None, keep=False, debug=L2):
    """(a) the oracle, (b) level 1, (c) level 2 and every comparison of the module's docstring.  want: (fused, chain, rows) steps of (c), default
    every candidate with two measurements or more on the level-2 step."""
    case = shape.case
    tri, ref = _oracle(g.oracle_for(oracle, shape), case)
    b = _run2(Updater, case, tri, debug=None)
    c = _run2(Updater, case, tri, debug=debug)
    (up_b, out_b, post_b, lm_b, steps_b), (up_c, out_c, post_c, lm_c, steps_c) = b, c
    try:
        gate = np.isfinite(ref["chi2"])
        acc = ref["lm_cov_id"] >= 0
        # ---- the planted outliers, and nothing else, are rejected: on the device as on the oracle
        assert np.flatnonzero(out_c["feat_status"] == capi.FEAT_CHI2_REJECTED).tolist() == sorted(shape.planted)
        # ---- identical across the three
        for k in ("feat_status", "lm_cov_id", "anchor_cam", "anchor_clone"):
            assert np.array_equal(out_b[k], out_c[k]), k
        assert out_b["N"] == out_c["N"] == ref["N"]
        for k in ("cov_id", "anchor_cam", "anchor_clone", "feat_rep"):
            assert np.array_equal(lm_b[k], lm_c[k]), k
        assert len(lm_c["cov_id"]) == case.L0 + acc.sum() and np.array_equal(lm_c["cov_id"][case.L0:], ref["lm_cov_id"][acc])
        # ---- (c) against (a), (c) against (b)
        _note("(c)-(a)", out_c, ref, post_c, ref, gate)
        _note("(c)-(b)", out_c, out_b, post_c, post_b, gate)
        _check(out_c, ref, post_c, ref, gate, "(c)-(a)")
        _check(out_c, out_b, post_c, post_b, gate, "(c)-(b)")
        if case.L0:
            np.testing.assert_allclose(lm_c["value"][:case.L0], ref["landmarks_existing"], rtol=1e-8, atol=1e-10)
            np.testing.assert_allclose(lm_c["value"][:case.L0], lm_b["value"][:case.L0], rtol=1e-8, atol=1e-10)
        # ---- the resident state is what the call returned
        assert post_c["P"].shape == out_c["P"].shape and np.array_equal(post_c["P"], out_c["P"])
        assert np.array_equal(lm_c["value"][case.L0:], out_c["lm_value"][acc]) and np.array_equal(lm_c["fej"][case.L0:], out_c["lm_fej"][acc])
        # ---- which step the candidates took
        m = np.diff(case.prob.meas_offsets)
        n2, n_held = int((m >= 2).sum()), int(((m >= 2) & (m <= M_MAX)).sum())
        assert steps_c == ((n_held, n2 - n_held, n_held) if want is None else want)
        assert steps_b == (n_held, n2 - n_held, 0)  # level 1 takes the fused step and never the level-2 one
    finally:
        if not keep:
            up_b.close(), up_c.close()
    return ref, b, c


# --------------------------------------------------------------------------- the option and the counter
def test_option_reads_back_the_level(Updater):
    up = Updater(capi.default_options())
    try:
        assert up.debug_option("delayed_init_fused") == 1  # the default
        assert up.debug_option("delayed_init_fused", 2) == 1 and up.debug_option("delayed_init_fused") == 2
        assert up.debug_option("delayed_init_fused", 9) == 2 and up.debug_option("delayed_init_fused") == 2  # above 2: taken as 2
        assert up.debug_option("delayed_init_fused", 0) == 2 and up.debug_option("delayed_init_fused") == 0
        assert up.debug_option("delayed_init_fused", 1) == 0 and up.debug_option("delayed_init_fused") == 1
        assert up.debug_option("delayed_init_rows_steps") == 0
        assert up.debug_option("delayed_init_rows_steps", 7) == 0 and up.debug_option("delayed_init_rows_steps") == 7
    finally:
        up.close()


def test_counter_counts_the_candidates_the_step_holds(Updater, oracle):
    """One, two and twelve measurements in one batch: the candidate with one is skipped, the others take the level-2 step; at level 1 and at
    level 0 the counter stays 0."""
    import track_shapes as ts
    from open_vins_amd import synth
    lengths = [12, 1, 2, 12, 2, 1, 12, 2]
    case = Case(ts.with_lengths(synth.make_problem(2, C=12, F=8, seed=32), lengths, patterns=("stride",)), capi.REP_ANCHORED_3D)
    tri, ref = _oracle(oracle, case)
    for level, want in ((2, (6, 0, 6)), (1, (6, 0, 0)), (0, (0, 6, 0))):
        up, out, _, _, steps = _run2(Updater, case, tri, debug={"delayed_init_fused": level})
        up.close()
        assert steps == want and np.array_equal(out["feat_status"], ref["feat_status"]), level


# --------------------------------------------------------------------------- track length at the tile edges
@pytest.mark.parametrize("m", g.TRACKS + [M_MAX])
def test_track_length_at_the_tile_edges(Updater, oracle, m):
    """m = 2: r = 1, a one-row factorisation and a one-term statistic.  m = 3.  m = 8: r + 3 = 16, W's rows fill one tile.  m = 9, 10: r = 15, 17 on
    either side of 16 (the statistic's lane-strided sum, the factorisation's first tile edge).  m = 64: r = 125, r + 3 = 128, the bound."""
    shape = g.BY_ID[f"len-{m}"]
    assert np.diff(shape.case.prob.meas_offsets).max() == m
    ref, _, _ = _three2(Updater, oracle, shape)
    assert (ref["lm_cov_id"] >= 0).sum() >= 3


def test_track_beyond_the_bound_takes_the_chain_step_in_place(Updater, oracle):
    """m = 65 between two shorter candidates: it alone takes the chain's step (k_system_t's gate), where it stands."""
    ref, _, _ = _three2(Updater, oracle, g.BY_ID[f"len-{M_MAX + 1}"], want=(2, 1, 2))
    assert (ref["lm_cov_id"] >= 0).all()


# --------------------------------------------------------------------------- representations and flags
@pytest.mark.parametrize("flags", range(len(g.FLAG_SETS)))
@pytest.mark.parametrize("rep", g.REPS6)
def test_representations_and_flags(Updater, oracle, rep, flags):
    """Every representation the entry accepts under the four flag sets (FEJ, K = 1 / 2, calibration of pose / intrinsics; the mono sets are
    fisheye), a planted outlier among the candidates.  The single depth gates at 2m - 2: chi2_thresh to 1e-12 of the oracle's (in _check)."""
    shape = g.BY_ID[f"rep{rep}-flags{flags}"]
    ref, _, (_, out_c, _, _, _) = _three2(Updater, oracle, shape)
    gate = np.isfinite(ref["chi2"])
    acc = ref["lm_cov_id"] >= 0
    assert acc.sum() >= 3 and ref["N"] == shape.case.prob.N + (1 if rep == SINGLE else 3) * acc.sum()
    np.testing.assert_allclose(out_c["chi2_thresh"][gate], ref["chi2_thresh"][gate], rtol=1e-12)
    do_fej, K, pose, intr = g.FLAG_SETS[flags]
    assert out_c["stats"]["D"] == 6 * 10 + K * (6 * pose + 8 * intr)


# --------------------------------------------------------------------------- where the decision moved
@pytest.mark.parametrize("sid", ["out-first", "out-middle", "out-last", "out-pair"])
def test_gross_outlier_first_middle_last_and_two_in_a_row(Updater, oracle, sid):
    shape = g.BY_ID[sid]
    ref, _, (_, out_c, _, lm_c, _) = _three2(Updater, oracle, shape)
    acc = ref["lm_cov_id"] >= 0
    assert not out_c["dx_seq"][list(shape.planted)].any() and (out_c["lm_cov_id"][list(shape.planted)] == -1).all()
    # the accepted candidate behind a rejected one receives the covariance id and the slot the rejected one would have had
    N0, ids = shape.case.prob.N, out_c["lm_cov_id"]
    assert np.array_equal(ids[acc], N0 + 3 * np.arange(acc.sum())) and np.array_equal(lm_c["cov_id"], ids[acc])
    if sid == "out-first":
        assert ids[0] == -1 and ids[np.flatnonzero(acc)[0]] == N0


def test_every_candidate_rejected_leaves_the_state_bit_for_bit(Updater, oracle):
    shape = g.BY_ID["out-all"]
    prob = shape.case.prob
    ref, _, (up_c, out_c, post_c, lm_c, _) = _three2(Updater, oracle, shape)
    assert not (ref["lm_cov_id"] >= 0).any() and (out_c["feat_status"] == capi.FEAT_CHI2_REJECTED).all()
    assert out_c["N"] == prob.N and np.array_equal(out_c["P"], prob.P) and np.array_equal(post_c["P"], prob.P)
    assert not out_c["dx_seq"].any() and len(lm_c["cov_id"]) == 0
    assert np.array_equal(post_c["clone_q_p"], prob.clone_q_p) and np.array_equal(post_c["calib_q_p"], prob.calib_q_p)
    assert np.array_equal(post_c["intrinsics"], prob.intrinsics)


def test_failed_triangulation_between_two_accepted_keeps_its_status(Updater, oracle):
    """Candidate 5 arrives OVGPU_FEAT_TRI_FAILED through ovgpu_set_triangulation: k_init_rows switches the step off, nobody writes its chi2 — the
    level-1 context's value, bit for bit (the caller sees NaN from both) — and the chain goes on."""
    shape = g.BY_ID["tri-failed"]
    (f, code), = shape.tri_failed.items()
    ref, (_, out_b, _, _, _), (_, out_c, _, _, _) = _three2(Updater, oracle, shape)
    assert out_c["feat_status"][f] == code and out_c["lm_cov_id"][f] == -1 and not out_c["dx_seq"][f].any()
    assert np.array_equal(out_c["chi2"][[f]], out_b["chi2"][[f]], equal_nan=True)
    acc = ref["lm_cov_id"] >= 0
    assert acc[:f].any() and acc[f + 1:].any()


# --------------------------------------------------------------------------- the covariance dimension at a tile edge
@pytest.mark.parametrize("mod", g.EDGES)
def test_covariance_dimension_crosses_a_tile_edge(Updater, oracle, mod):
    """N at entry 16k + 14, 16k + 15, 16k with 3-dof candidates: the tail's workgroups straddle id, and every one of them decides the gate alike."""
    shape = g.BY_ID[f"edge-{mod}"]
    assert shape.case.prob.N % 16 == mod
    ref, _, _ = _three2(Updater, oracle, shape)
    assert (ref["lm_cov_id"] >= 0).sum() >= 6 and ref["N"] // 16 > shape.case.prob.N // 16


# --------------------------------------------------------------------------- per-feature sigma and multiplier
@pytest.mark.parametrize("rep", ["global", "single"])
def test_per_feature_sigma_and_multiplier(Updater, oracle, rep):
    """sigma_f and the multiplier per candidate.  The rows leave k_init_rows scaled by oscale = sigma / sigma_f; the same sigma_f under a context
    sigma of 3 scales S by 9 and res2 by 3: chi2 must not move (the project's bound on chi2, 1e-7)."""
    a, b = g.BY_ID[f"sigma-{rep}"], g.BY_ID[f"sigma-{rep}-ctx3"]
    ref, _, (_, out_a, _, _, _) = _three2(Updater, oracle, a)
    _, _, (_, out_b, _, _, _) = _three2(Updater, oracle, b)
    gate = np.isfinite(ref["chi2"])
    tag, _, _ = g.sigma_arrays()
    acc = ref["lm_cov_id"] >= 0
    assert (acc & tag).any() and (acc & ~tag).any()
    print(f"chi2 under sigma 3 against sigma 1: {np.abs(out_b['chi2'][gate] / out_a['chi2'][gate] - 1.0).max():.3e}")
    np.testing.assert_allclose(out_b["chi2"][gate], out_a["chi2"][gate], rtol=1e-7)
    assert np.array_equal(out_b["feat_status"], out_a["feat_status"])


# --------------------------------------------------------------------------- resident landmarks, then the SLAM update on the grown state
def test_resident_landmarks_follow_every_step_then_slam_update(Updater, oracle):
    shape = g.BY_ID["resident"]
    case = shape.case
    ref, b, c = _three2(Updater, oracle, shape, keep=True)
    try:
        assert (ref["lm_cov_id"] >= 0).sum() >= 3
        assert np.abs(c[3]["value"][:6] - case.prob.lm_value).max() > 0  # they moved
        outs = []
        for up, out, post, lm, _ in (b, c):
            nxt = g.resident_state()  # the six landmarks' own tracks
            nxt.N, nxt.P, nxt.clone_q_p, nxt.calib_q_p, nxt.intrinsics = out["N"], post["P"], post["clone_q_p"], post["calib_q_p"], post["intrinsics"]
            nxt.lm_value, nxt.lm_fej, nxt.lm_cov_id = lm["value"], lm["fej"], lm["cov_id"]
            nxt.lm_anchor_cam, nxt.lm_anchor_clone, nxt.lm_rep_each = lm["anchor_cam"], lm["anchor_clone"], lm["feat_rep"]
            nxt.lm_index = np.arange(6, dtype=np.int32)
            up.set_active_landmarks(None)
            up.set_features(nxt)
            outs.append(up.slam_update(lm_index=nxt.lm_index))
        u_b, u_c = outs
        assert np.array_equal(u_b["feat_status"], u_c["feat_status"]) and (u_c["feat_status"] == capi.FEAT_USED).sum() >= 3
        print(f"follow-up (c)-(b): dx {_rel(u_c['dx'], u_b['dx']):.3e}  P {_rel(u_c['P'], u_b['P']):.3e}")
        assert _rel(u_c["dx"], u_b["dx"]) < 1e-6 and _rel(u_c["P"], u_b["P"]) < 1e-7
        np.testing.assert_allclose(u_c["landmarks"], u_b["landmarks"], rtol=1e-8, atol=1e-10)
    finally:
        b[0].close(), c[0].close()


# --------------------------------------------------------------------------- every tail workgroup decides alike
def _run_from_reset(Updater, case, tri):
    """A level-2 run that starts from ovgpu_reset_state: the state as ovgpu_set_state left it, the batch laid out again."""
    up = Updater(case.opts)
    up.debug_option("delayed_init_fused", 2)
    up.set_problem(case.prob)
    up.reset_state()
    up.set_features(case.prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    out = up.delayed_init(case.rep, feat_rep_each=case.each, fused=True)
    steps = tuple(up.debug_option(k) for k in ("delayed_init_fused_steps", "delayed_init_chain_steps", "delayed_init_rows_steps"))
    return up, out, up.get_state(P=True), up.get_landmarks(), steps


def test_two_runs_return_the_same_bits(Updater, oracle):
    """Twelve candidates, two of them rejected, twice from ovgpu_reset_state: every output bit for bit.  A tail workgroup that decided the gate
    differently from its neighbours would leave a partly written P; one that summed in another order could differ in the last bit of chi2."""
    shape = g.BY_ID["two-rejected"]
    case = shape.case
    tri, ref = _oracle(oracle, case)
    runs = [_run_from_reset(Updater, case, tri) for _ in range(2)]
    try:
        (_, out_1, post_1, lm_1, steps_1), (_, out_2, post_2, lm_2, steps_2) = runs
        assert steps_1 == steps_2 == (12, 0, 12)
        assert np.flatnonzero(out_1["feat_status"] == capi.FEAT_CHI2_REJECTED).tolist() == sorted(shape.planted)
        for k in OUT_KEYS:
            assert np.array_equal(out_1[k], out_2[k], equal_nan=out_1[k].dtype.kind == "f"), k
        assert out_1["N"] == out_2["N"]
        for k in STATE_KEYS:
            assert np.array_equal(post_1[k], post_2[k]), k
        for k in lm_1:
            assert np.array_equal(lm_1[k], lm_2[k]), k
    finally:
        for r in runs:
            r[0].close()


# --------------------------------------------------------------------------- nothing else moved
def _equal_bits(a, b):
    (_, out_a, post_a, lm_a, _), (_, out_b, post_b, lm_b, _) = a, b
    for k in OUT_KEYS:
        assert np.array_equal(out_a[k], out_b[k], equal_nan=out_a[k].dtype.kind == "f"), k
    assert out_a["N"] == out_b["N"]
    for k in STATE_KEYS:
        assert np.array_equal(post_a[k], post_b[k]), k
    for k in lm_a:
        assert np.array_equal(lm_a[k], lm_b[k]), k


def test_level_one_and_an_untouched_context_return_equal_bits(Updater, oracle):
    case = g.BY_ID["out-middle"].case
    tri, _ = _oracle(oracle, case)
    a = _run(Updater, case, tri, fused=True)
    b = _run(Updater, case, tri, fused=True, debug={"delayed_init_fused": 1})
    try:
        assert a[0].debug_option("delayed_init_fused") == 1 and a[0].debug_option("delayed_init_rows_steps") == 0
        _equal_bits(a, b)
    finally:
        a[0].close(), b[0].close()


def test_the_chain_entry_keeps_its_bits_at_level_two(Updater, oracle):
    """ovgpu_slam_delayed_init with the option at 2 and at 1."""
    case = g.BY_ID["out-middle"].case
    tri, _ = _oracle(oracle, case)
    a = _run2(Updater, case, tri, fused=False, debug={"delayed_init_fused": 1})
    b = _run2(Updater, case, tri, fused=False, debug=L2)
    try:
        assert a[4] == b[4] == (0, 0, 0)
        _equal_bits(a, b)
    finally:
        a[0].close(), b[0].close()


def test_mode_a_keeps_its_bits_at_level_two(Updater, oracle):
    """ovgpu_slam_init_systems: its export needs the pre-gate system from k_system_t, at every level."""
    case = g.BY_ID["out-middle"].case
    tri, _ = _oracle(oracle, case)
    outs = []
    for level in (1, 2):
        up = Updater(case.opts)
        try:
            up.debug_option("delayed_init_fused", level)
            up.set_problem(case.prob)
            up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
            outs.append((up.init_systems(case.rep), up.get_state(P=True), up.debug_option("delayed_init_rows_steps")))
        finally:
            up.close()
    (sys_1, post_1, rows_1), (sys_2, post_2, rows_2) = outs
    assert rows_1 == rows_2 == 0 and len(sys_1) == len(sys_2) == case.prob.F
    assert sum(s["status"] == capi.FEAT_CHI2_REJECTED for s in sys_2) == 1
    for s1, s2 in zip(sys_1, sys_2):
        for k in s1:
            if isinstance(s1[k], np.ndarray):
                assert np.array_equal(s1[k], s2[k], equal_nan=True), k
            elif isinstance(s1[k], float):
                assert s1[k] == s2[k] or (np.isnan(s1[k]) and np.isnan(s2[k])), k
            else:
                assert s1[k] == s2[k], k
    for k in STATE_KEYS:
        assert np.array_equal(post_1[k], post_2[k]), k


def test_no_single_launch_cholesky_returns_level_zero_bits(Updater, oracle):
    base = g.BY_ID["out-middle"].case
    case = Case(base.prob, base.rep, opts=capi.default_options(chi2_multipler=1.0, no_single_launch_cholesky=1))
    tri, _ = _oracle(oracle, case)
    a = _run2(Updater, case, tri, debug={"delayed_init_fused": 0})
    b = _run2(Updater, case, tri, debug=L2)
    try:
        n2 = int((np.diff(case.prob.meas_offsets) >= 2).sum())
        assert a[4] == b[4] == (0, n2, 0)
        _equal_bits(a, b)
    finally:
        a[0].close(), b[0].close()


def test_zz_worst_deviations():
    """Prints the largest deviations over the cases of this run (-s shows them); holds nothing the cases did not hold already."""
    for (tag, k), v in sorted(WORST.items()):
        print(f"worst {tag} {k}: {v:.3e}")
    assert WORST, "no case ran before this one"
