"""GPU tests (`-m gpu`) of ovgpu_debug_option "delayed_init_fused_long" (csrc/k_init_fused.h): ovgpu_slam_delayed_init_fused with the fused step
for candidates of 65 .. 232 measurements — k_init_rows' carve beyond 64 KB, and from 130 measurements on (r = 2m - 3 > 256) the two panels of
k_chol_wide.h under the step.  Every batch of tests/init_long_shapes.py runs with the switch on, at level 1 and at level 2 of
"delayed_init_fused", against

  (a) the oracle's slam_delayed_init,
  (b) a second context of the same library with the switch off, at the same level,

both through tests/test_gpu_delayed_init_fused.py's _check, imported with its bounds: chi2 1e-7, chi2_thresh 1e-12, values 1e-8 / 1e-10, FEJ
1e-12, dx_seq 1e-6, P 1e-7, P symmetric to 1e-13 of its largest entry, poses 1e-9; feat_status, lm_cov_id, N, anchors and landmark slots identical
across the three.  tests/test_init_long_shapes_cpu.py holds every batch, on the oracle alone, further than GATE_MARGIN from every threshold
(asserted again in _oracle) and to the planted rejections being the only ones.  Every case asserts the counters — "delayed_init_long_steps" equal
to the number of candidates with 65 .. 232 measurements — and that the switch reads back 1: every case fails on a library without the switch.

Worst deviations over the catalogue, measured on the MI355X (every case prints its own, test_zz_worst_deviations the maxima): against the oracle,
at either level, chi2 2.6e-13, dx_seq 1.2e-12, P 3.8e-14, values 1.7e-13, poses 1.0e-12; against the switch-off context at level 1 chi2 0,
dx_seq 2.4e-15, P 8.5e-17, values 4.4e-15, poses 0, at level 2 chi2 7.3e-15, dx_seq 1.8e-14, P 6.1e-16, values 6.2e-15, poses 5.7e-14 (DESIGN.md
section 7, "The fused delayed-initialisation step for tracks of 65 to 232 measurements").
"""
import numpy as np
import pytest

import init_gate_shapes as g
import init_long_shapes as ls
from open_vins_amd import capi
from test_gpu_delayed_init_fused import _check, _oracle, _run, Case, M_MAX
from test_gpu_init_gate import _note, _equal_bits, WORST, STATE_KEYS

pytestmark = pytest.mark.gpu

COUNTERS = ("delayed_init_fused_steps", "delayed_init_chain_steps", "delayed_init_rows_steps", "delayed_init_long_steps")
_REF = {}  # shape id -> (triangulation, oracle result): computed once, shared by the levels, never modified


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _ref(oracle, shape):
    if shape.id not in _REF:
        _REF[shape.id] = _oracle(g.oracle_for(oracle, shape), shape.case)
    return _REF[shape.id]


def _run_long(Updater, case, tri, level, long=1, fused=True, more=None):
    """_run at `level` with the switch at `long`; (context, out, post, landmarks, (fused, chain, rows, long) steps)."""
    dbg = {"delayed_init_fused": level, "delayed_init_rows_steps": 0}
    if long is not None:  # (None: a context that never hears of the switch)
        dbg.update({"delayed_init_fused_long": long, "delayed_init_long_steps": 0})
    dbg.update(more or {})
    up, out, post, lm, _ = _run(Updater, case, tri, fused, debug=dbg)
    return up, out, post, lm, tuple(up.debug_option(k) for k in COUNTERS)


def _want_steps(m, level, bound):
    n2, held = int((m >= 2).sum()), int(((m >= 2) & (m <= bound)).sum())
    return held, n2 - held, held if level >= 2 else 0, int(((m > M_MAX) & (m <= bound)).sum())


def _three_long(Updater, oracle, shape, level, keep=False):
    """(a) the oracle, (b) the switch off, (c) the switch on, and every comparison of the module's docstring."""
    case = shape.case
    tri, ref = _ref(oracle, shape)
    b = _run_long(Updater, case, tri, level, long=0)
    c = _run_long(Updater, case, tri, level, long=1)
    (up_b, out_b, post_b, lm_b, steps_b), (up_c, out_c, post_c, lm_c, steps_c) = b, c
    try:
        assert up_c.debug_option("delayed_init_fused_long") == 1 and up_b.debug_option("delayed_init_fused_long") == 0
        gate = np.isfinite(ref["chi2"])
        acc = ref["lm_cov_id"] >= 0
        # ---- the planted rejections, and nothing else, are rejected: on the device as on the oracle
        assert np.flatnonzero(out_c["feat_status"] == capi.FEAT_CHI2_REJECTED).tolist() == sorted(shape.planted)
        # ---- identical across the three
        for k in ("feat_status", "lm_cov_id", "anchor_cam", "anchor_clone"):
            assert np.array_equal(out_b[k], out_c[k]), k
        assert out_b["N"] == out_c["N"] == ref["N"]
        for k in ("cov_id", "anchor_cam", "anchor_clone", "feat_rep"):
            assert np.array_equal(lm_b[k], lm_c[k]), k
        assert len(lm_c["cov_id"]) == case.L0 + acc.sum() and np.array_equal(lm_c["cov_id"][case.L0:], ref["lm_cov_id"][acc])
        # ---- (c) against (a), (c) against (b)
        _note(f"L{level} (c)-(a)", out_c, ref, post_c, ref, gate)
        _note(f"L{level} (c)-(b)", out_c, out_b, post_c, post_b, gate)
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
        assert steps_c == _want_steps(m, level, ls.M_LONG) and steps_c[3] == ls.n_long(shape) >= 1
        assert steps_b == _want_steps(m, level, M_MAX) and steps_b[3] == 0
    finally:
        if not keep:
            up_b.close(), up_c.close()
    return ref, b, c


# --------------------------------------------------------------------------- the option and the counter
def test_option_and_counter_read_back(Updater):
    up = Updater(capi.default_options())
    try:
        assert up.debug_option("delayed_init_fused_long") == 0  # the default
        assert up.debug_option("delayed_init_fused_long", 1) == 0 and up.debug_option("delayed_init_fused_long") == 1
        assert up.debug_option("delayed_init_fused_long", 0) == 1 and up.debug_option("delayed_init_fused_long") == 0
        assert up.debug_option("delayed_init_fused") == 1  # the level is its own
        assert up.debug_option("delayed_init_long_steps") == 0
        assert up.debug_option("delayed_init_long_steps", 7) == 0 and up.debug_option("delayed_init_long_steps") == 7
    finally:
        up.close()


# --------------------------------------------------------------------------- the catalogue, at both levels
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("sid", [s.id for s in ls.SHAPES])
def test_catalogue(Updater, oracle, sid, level):
    """stereo-64-65: 64 unchanged, 65 the first long one.  panel-*: r = 253, 255 (the last single panel), 257 (the first two-panel one).
    bound-*: 231, 232 on the step, 233 on the chain's, in place.  long-first / -last / -alone: the carve and the step words before and after
    short steps.  resident, sigma, out-*, uncalibrated-232, tri-failed-130: as named in tests/init_long_shapes.py."""
    shape = ls.BY_ID[sid]
    ref, _, (_, out_c, _, _, _) = _three_long(Updater, oracle, shape, level)
    for f in shape.planted:
        assert not out_c["dx_seq"][f].any() and out_c["lm_cov_id"][f] == -1
    for f, code in shape.tri_failed.items():
        assert out_c["feat_status"][f] == code and out_c["lm_cov_id"][f] == -1 and not out_c["dx_seq"][f].any()


# --------------------------------------------------------------------------- nothing else moved
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("sid", ["out-middle", "len-64"])
def test_short_batch_keeps_its_bits_under_the_switch(Updater, oracle, sid, level):
    """Tracks of 64 measurements at most: the switch-off outputs and resident state, bit for bit, and the same counters."""
    shape = g.BY_ID[sid]
    assert np.diff(shape.case.prob.meas_offsets).max() <= M_MAX
    tri, _ = _oracle(g.oracle_for(oracle, shape), shape.case)
    a = _run_long(Updater, shape.case, tri, level, long=None)
    b = _run_long(Updater, shape.case, tri, level, long=1)
    try:
        assert b[0].debug_option("delayed_init_fused_long") == 1
        assert a[4] == b[4] and b[4][3] == 0 and b[4][1] == 0
        _equal_bits(a, b)
    finally:
        a[0].close(), b[0].close()


def test_level_zero_returns_the_chain_entry_bits_under_the_switch(Updater, oracle):
    """"delayed_init_fused" = 0 with the switch on: ovgpu_slam_delayed_init's bits, every candidate counted on the chain's step."""
    shape = ls.BY_ID["panel-rep0"]
    tri, _ = _ref(oracle, shape)
    a = _run_long(Updater, shape.case, tri, 1, long=None, fused=False)
    b = _run_long(Updater, shape.case, tri, 0, long=1)
    try:
        assert a[4] == (0, 0, 0, 0) and b[4] == (0, shape.case.prob.F, 0, 0)
        _equal_bits(a, b)
    finally:
        a[0].close(), b[0].close()


@pytest.mark.parametrize("sid", ["out-130", "uncalibrated-232"])
def test_long_rejection_at_level_two_leaves_what_a_batch_without_it_leaves(Updater, oracle, sid):
    """The rejected long candidate ran k_init_rows, both products and the two-panel factorisation, and its tail wrote chi2 and the status alone:
    P, the poses, the landmarks and the device counters (N, the landmark slots) behind it are, bit for bit, those of the batch without it."""
    shape = ls.BY_ID[sid]
    case = shape.case
    (f,) = shape.planted
    keep = [k for k in range(case.prob.F) if k != f]
    tri, ref = _ref(oracle, shape)
    short = Case(case.prob.subset(keep), case.rep, opts=case.opts)
    tri_s, _ = _oracle(oracle, short)  # (a feature's triangulation reads its own track and the clone poses at entry: the same bits)
    assert np.array_equal(np.asarray(tri_s["p_FinG"]).reshape(-1, 3), np.asarray(tri["p_FinG"]).reshape(-1, 3)[keep])
    a = _run_long(Updater, case, tri, 2)
    b = _run_long(Updater, short, tri_s, 2)
    try:
        (_, out_a, post_a, lm_a, steps_a), (_, out_b, post_b, lm_b, steps_b) = a, b
        assert out_a["feat_status"][f] == capi.FEAT_CHI2_REJECTED and np.isfinite(out_a["chi2"][f]) and out_a["chi2"][f] > out_a["chi2_thresh"][f]
        assert steps_a == _want_steps(np.diff(case.prob.meas_offsets), 2, ls.M_LONG) and steps_a[1] == 0
        assert steps_b == _want_steps(np.diff(short.prob.meas_offsets), 2, ls.M_LONG) and steps_b[0] == steps_a[0] - 1
        assert out_a["N"] == out_b["N"] == ref["N"]
        for k in ("feat_status", "chi2", "chi2_thresh", "lm_cov_id", "lm_value", "lm_fej", "anchor_cam", "anchor_clone"):
            assert np.array_equal(out_a[k][keep], out_b[k]), k
        assert np.array_equal(out_a["dx_seq"][keep][:, :out_a["N"]], out_b["dx_seq"][:, :out_b["N"]])
        for k in STATE_KEYS:
            assert np.array_equal(post_a[k], post_b[k]), k
        for k in lm_a:
            assert np.array_equal(lm_a[k], lm_b[k]), k
    finally:
        a[0].close(), b[0].close()


@pytest.mark.parametrize("level", [1, 2])
def test_without_the_two_panel_factorisation_130_takes_the_chain_step(Updater, oracle, level):
    """"chol_wide" = 0: r = 257 has no factorisation the step can use.  That candidate takes the chain's step in place and is counted there;
    128 and 129 (one panel) stay on the fused step."""
    shape = ls.BY_ID["panel-rep0"]
    case = shape.case
    tri, ref = _ref(oracle, shape)
    up, out, post, lm, steps = _run_long(Updater, case, tri, level, more={"chol_wide": 0, "chol_wide_factorisations": 0})
    try:
        assert steps == (4, 1, 4 if level == 2 else 0, 2) and up.debug_option("chol_wide_factorisations") == 0
        _check(out, ref, post, ref, np.isfinite(ref["chi2"]), "chol_wide = 0 against the oracle")
    finally:
        up.close()
    up, _, _, _, steps = _run_long(Updater, case, tri, level, more={"chol_wide_factorisations": 0})
    try:
        assert steps == (5, 0, 5 if level == 2 else 0, 3) and up.debug_option("chol_wide_factorisations") == 1
    finally:
        up.close()


def test_zz_worst_deviations():
    """Prints the largest deviations over the cases of this run (-s shows them); holds nothing the cases did not hold already."""
    mine = {k: v for k, v in WORST.items() if k[0].startswith("L")}
    for (tag, k), v in sorted(mine.items()):
        print(f"worst {tag} {k}: {v:.3e}")
    assert mine, "no case ran before this one"
