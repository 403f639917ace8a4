"""The general per-feature kernel (csrc/k_system.h: k_system_t<false> / <true>) at its LDS-carve, panel and loop edges (run with `-m gpu` on an
MI355X).

Everything that is not on a fused fast path runs on this kernel: every SLAM update and delayed initialisation of a default context, batches with
per-feature noise, anchored MSCKF batches under "anchored_fast" = 0, tracks beyond 232 observations, everything under no_fast_feature_kernel.
tests/system_shapes.py builds batches ON its internal edges — the gate's panel routine (2 m + 4 = 128 | 129, 512 | 513, 1024 | 1025 rows), the
strided loops (m = 64 | 65, 256 | 257, m % 8, D = 255 | 256 | 257), the LDS carve's two role edges g (the longest track's own gate matrix leaves
LDS) and r (the Jacobian records leave LDS, the other instantiation) at both record strides, and the row modes (MSCKF, 3-dof and single-depth
SLAM landmarks, the delayed initialisation, per-feature noise) — and tests/test_system_shapes_cpu.py shows every batch non-vacuous on the oracle
alone.  Here every case runs on a context of its own with the oracle's positions injected and is held to the ORACLE: accept sets identical with
no excuse, thresholds 1e-12, chi2 1e-8, dx 1e-8, P' 1e-9 and exactly symmetric, poses 1e-9 (tracks beyond 232 observations: dx 1e-7, P' 1e-8,
the bounds of test_gpu_parity.test_tracks_beyond_254_observations_are_gated), n_rows / n_used the oracle's.  The kernel must be the general one
and the carve the library reports ("sys_m_lds_max", "sys_rows_global", "sys_row_stride", "sys_lds_bytes") must be system_shapes.carve's at the
limit it reports ("sys_lds_limit"): the role lengths are computed from that limit at run time.

Each case prints one line `sys ...` with its deviations; test_zz_worst_deviations the maxima per group (DESIGN.md section 3 quotes them)."""
import numpy as np
import pytest

import system_shapes as sy
from open_vins_amd import capi
from parity_util import assert_chi2

pytestmark = pytest.mark.gpu

TOL_CHI2, TOL_THR, TOL_DX, TOL_P, TOL_POSE = 1e-8, 1e-12, 1e-8, 1e-9, 1e-9
TOL_DX_LONG, TOL_P_LONG = 1e-7, 1e-8  # tracks beyond 232 observations
STATE_KEYS = ("clone_q_p", "calib_q_p", "intrinsics")
WORST = {}  # (group, quantity) -> largest deviation so far


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


@pytest.fixture(scope="module")
def limit(Updater):
    up = Updater(capi.default_options())
    lim = up.debug_option("sys_lds_limit")
    up.close()
    assert 32 * 1024 <= lim <= 160 * 1024
    return lim


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def note(group, **dev):
    for k, v in dev.items():
        WORST[(group, k)] = max(WORST.get((group, k), 0.0), float(v))


def carve_of(up):
    return dict(m_lds_max=up.debug_option("sys_m_lds_max"), rows_global=up.debug_option("sys_rows_global"), row_stride=up.debug_option("sys_row_stride"),
                lds_bytes=up.debug_option("sys_lds_bytes"), kernel=up.debug_option("last_feature_kernel"))


def run(Updater, kind, opts, prob, tri=None, debug=None, rep=0, sigma=None, mult=None, up=None, keep=False):
    """one batch on a context of its own (or on `up`): the outputs, the state behind them and the carve the library reports"""
    up = Updater(opts) if up is None else up
    for name, val in (debug or {}).items():
        up.debug_option(name, val)
    if kind == "slam":
        up.set_slam_problem(prob)
        if sigma is not None or mult is not None:
            up.set_feature_options(sigma_pix=sigma, chi2_multipler=mult)
        out = up.slam_update(prob.lm_index)
        out.update(up.get_state(P=False))
    else:
        up.set_problem(prob)
        if tri is not None:
            up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
        if kind == "msckf":
            out = up.update()
        else:
            out = up.delayed_init(rep)
            out.update(up.get_state(P=False))
    out["carve"] = carve_of(up)
    if keep:
        return out, up
    up.close()
    return out


def run_case(Updater, case, limit, oracle):
    tri, ref = sy.oracle_run(oracle, case, limit)
    _, prob, _ = case.batch(limit)
    return run(Updater, case.kind, case.opts(), prob, tri, case.debug, case.rep, case.sigma, case.mult), ref


def hold_to_the_oracle(case, out, ref, limit):
    m = case.length(limit)
    m_lds, rows_global, refused = case.carve(limit)
    gate = np.isfinite(ref["chi2"])
    dx_key = "dx_seq" if case.kind == "init" else "dx"
    dev = dict(chi2=np.abs(out["chi2"][gate] / ref["chi2"][gate] - 1.0).max(), dx=_rel(out[dx_key], ref[dx_key]), P=_rel(out["P"], ref["P"]),
               poses=max(np.abs(out[k] - ref[k]).max() for k in STATE_KEYS[:2]))
    if case.kind == "slam":
        dev["landmarks"] = np.abs(out["landmarks"] - ref["landmarks"]).max()
    print(f"sys {case.id} m_max {m} D {case.D} carve {out['carve']} gated {int(gate.sum())}: " + "  ".join(f"{k} {v:.2e}" for k, v in dev.items()))
    note(case.group, **dev)
    # ---- the dispatch the library reports against the restated rule
    assert not refused
    assert out["carve"]["kernel"] == 0
    assert out["carve"]["row_stride"] == case.row_stride
    assert (out["carve"]["m_lds_max"], out["carve"]["rows_global"]) == (m_lds, int(rows_global))
    assert out["carve"]["lds_bytes"] == sy.lds_bytes(m, case.row_stride, case.D, limit) <= limit
    # ---- accept sets, no excuse; statistic and threshold
    assert np.array_equal(out["feat_status"], ref["feat_status"]), (out["feat_status"], ref["feat_status"])
    assert_chi2(out, ref, TOL_CHI2, strict=True)
    assert np.isnan(out["chi2"][~gate]).all()
    np.testing.assert_allclose(out["chi2_thresh"][gate], ref["chi2_thresh"][gate], rtol=TOL_THR)
    # ---- the rows of rejected and untriangulated features leave no trace
    if case.kind == "init":
        assert out["N"] == ref["N"] and np.array_equal(out["lm_cov_id"], ref["lm_cov_id"])
        acc = ref["lm_cov_id"] >= 0
        assert not out["dx_seq"][~acc].any() and np.isnan(out["lm_value"][~acc]).all()
        np.testing.assert_allclose(out["lm_value"][acc], ref["lm_value"][acc], rtol=1e-8, atol=1e-10)
    else:
        assert out["stats"]["n_used"] == ref["stats"]["n_used"] and out["stats"]["n_rows"] == ref["stats"]["n_rows"]
        assert out["stats"]["D"] == case.D
    long_track = m > sy.FUSED_MAX
    assert dev["dx"] < (TOL_DX_LONG if long_track else TOL_DX)
    assert dev["P"] < (TOL_P_LONG if long_track else TOL_P)
    assert np.array_equal(out["P"], out["P"].T)
    assert dev["poses"] < TOL_POSE and np.abs(out["intrinsics"] - ref["intrinsics"]).max() < 1e-8
    if case.kind == "slam":
        assert dev["landmarks"] < 1e-9


@pytest.mark.parametrize("cid", [c.id for c in sy.CASES])
def test_system_edge(Updater, oracle, limit, cid):
    case = sy.BY_ID[cid]
    out, ref = run_case(Updater, case, limit, oracle)
    hold_to_the_oracle(case, out, ref, limit)
    _, _, f_long = case.batch(limit)
    acc = sy.accepted(case, ref)
    assert bool(acc[f_long]) == (not case.long_rejected) and np.isfinite(out["chi2"][f_long])


# --------------------------------------------------------------------------- the two cross-checks
GENERAL = dict(chi2_multipler=1.0, gate_always_factor=1, no_fast_feature_kernel=1)


def _cross(Updater, oracle, limit):
    alone, under, over = sy.cross_check_batches(limit)
    opts = capi.default_options(**GENERAL)
    tri = oracle.triangulate(opts, capi.Views(over))
    n = alone.F
    cut = lambda k: {key: np.ascontiguousarray(val[:k]) for key, val in tri.items() if isinstance(val, np.ndarray)}
    assert (tri["status"][:n] == 0).all()
    return [run(Updater, "msckf", opts, p, cut(p.F)) for p in (alone, under, over)], n


def test_gate_matrix_home_does_not_change_a_bit(Updater, oracle, limit):
    """The same short tracks alone (every gate matrix in LDS) and with one track of r - 1 observations appended (m_lds_max below every one of them:
    every gate matrix in the global workspace), both on k_system_t<false>: the common features' chi2 must be the same BITS.  A difference means a
    gate read or wrote outside its matrix."""
    (alone, under, _), n = _cross(Updater, oracle, limit)
    _, r = sy.edges(48, 208, limit)
    assert alone["carve"]["kernel"] == under["carve"]["kernel"] == 0 and alone["carve"]["rows_global"] == under["carve"]["rows_global"] == 0
    assert alone["carve"]["m_lds_max"] == max(sy.X_SHORTS) and under["carve"]["m_lds_max"] == sy.carve(r - 1, 48, 208, limit)[0] < min(sy.X_SHORTS)
    assert np.isfinite(alone["chi2"]).all() and np.isfinite(under["chi2"][n])
    assert np.array_equal(alone["chi2"], under["chi2"][:n]), np.abs(alone["chi2"] / under["chi2"][:n] - 1.0).max()
    assert np.array_equal(alone["chi2_thresh"], under["chi2_thresh"][:n]) and np.array_equal(alone["feat_status"], under["feat_status"][:n])


def test_records_in_lds_against_records_in_the_workspace(Updater, oracle, limit):
    """k_system_t<false> (the short tracks alone) against k_system_t<true> (the same with a track of r observations appended): two instantiations,
    so the common features' chi2 is held to the bound, not to the bits.  Measured on the MI355X: see DESIGN.md section 3."""
    (alone, _, over), n = _cross(Updater, oracle, limit)
    assert alone["carve"]["rows_global"] == 0 and over["carve"]["rows_global"] == 1 and over["carve"]["m_lds_max"] >= max(sy.X_SHORTS)
    d = np.abs(over["chi2"][:n] / alone["chi2"] - 1.0).max()
    print(f"sys cross-check k_system_t<false> against <true>: chi2 {d:.3e}, identical bits: {np.array_equal(over['chi2'][:n], alone['chi2'])}")
    note("x", chi2_false_true=d)
    assert d < TOL_CHI2 and np.array_equal(alone["feat_status"], over["feat_status"][:n])


# --------------------------------------------------------------------------- (e) what a batch leaves behind on its context
def _same_bits(a, b, what):
    for k in ("feat_status", "chi2", "chi2_thresh", "dx", "P") + STATE_KEYS + (("landmarks",) if "landmarks" in b else ()):
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)
    assert a["carve"] == b["carve"], what
    for k in ("n_used", "n_rows", "D"):
        assert a["stats"][k] == b["stats"][k], (what, k)


def test_chain_across_the_edges_equals_fresh_contexts(Updater, limit):
    """One context: stride 48 at g - 1, stride 72 at r (a SLAM batch of anchored landmarks, records in the workspace), stride 48 at g + 1 (gate
    matrix in the workspace), a 9-observation batch.  Every link must be what a fresh context gives, bit for bit: the carve and both workspaces
    follow the batch in force, nothing of the batch before is left."""
    links = sy.chain_links(limit)
    up, seen = None, []
    for i, (kind, o, prob, (stride, m)) in enumerate(links):
        opts = capi.default_options(**o)
        fresh = run(Updater, kind, opts, prob)
        if up is None:
            up = Updater(opts)
        out, up = run(Updater, kind, opts, prob, up=up, keep=True)
        _same_bits(out, fresh, f"link {i}")
        assert fresh["carve"]["row_stride"] == stride and fresh["carve"]["kernel"] == 0 and fresh["stats"]["n_used"] >= 2
        seen.append((fresh["carve"]["m_lds_max"] == m, fresh["carve"]["rows_global"]))
    up.close()
    assert seen[0] == (True, 0) and seen[1][1] == 1 and seen[2] == (False, 0) and seen[3] == (True, 0)


def test_msckf_update_after_a_delayed_initialisation_that_switched_the_stride(Updater, oracle, limit):
    """ovgpu_slam_delayed_init in an anchored representation moves a 48-double context to 72-double records (begin_init_chain); the MSCKF batch
    uploaded behind it (a new state: 48 again, gate matrix of the longest track in the workspace) must be a fresh context's, bit for bit."""
    init = sy.BY_ID[f"d-init-rep{capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH}-g"]
    tri, _ = sy.oracle_run(oracle, init, limit)
    _, prob, _ = init.batch(limit)
    first, up = run(Updater, "init", init.opts(), prob, tri, rep=init.rep, keep=True)
    assert first["carve"]["row_stride"] == 72 and (first["lm_cov_id"] >= 0).any()
    kind, o, nxt, (stride, m) = sy.chain_links(limit)[2]
    out, up = run(Updater, kind, init.opts(), nxt, up=up, keep=True)
    up.close()
    fresh = run(Updater, kind, init.opts(), nxt)
    assert fresh["carve"]["row_stride"] == 48 and fresh["carve"]["m_lds_max"] < m and fresh["stats"]["n_used"] >= 2
    _same_bits(out, fresh, "the MSCKF update behind the delayed initialisation")


def test_zz_worst_deviations():
    """prints what the cases of this file measured (DESIGN.md section 3 quotes the figures)"""
    for (group, k), v in sorted(WORST.items()):
        print(f"sys group {group}: worst {k} {v:.3e}")
