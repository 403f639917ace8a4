"""GPU tests (`-m gpu`) of the Cholesky-with-carry beyond 256 columns: two panels of k_chol_fused around k_chol_schur, four launches
(csrc/k_chol_wide.h, enqueue_chol_wide) where the library used to run one launch of k_ekf_chol_step per 16 rows.  All through the C ABI.

Shapes: D2 = D - 256 is 1, just under / at / over a tile (15, 16, 17), 44 and 255: D in {257, 271, 272, 273, 300, 511}.

Bounds.  Against float64 numpy and the oracle: the suite's own (dx 1e-8, P' 1e-9 relative for the dense update, TOL_DX / TOL_P of
tests/test_gpu_parity.py for the feature updates, ten times that for SLAM as tests/test_gpu_slam_chunked.py has it).  Against the step-wise kernels of
the same library (`"chol_wide"` = 0 on a second context): dx 1e-10, P' 1e-11 relative — U is unique and the carried columns are the same sums in
another order.  Measured on the MI355X, worst over the six D: dx 1.3e-15, P' 3.9e-16 against the step-wise result.  Every context here sets
ovgpu_debug_option "chol_wide" to what it wants, whatever the library's default.

Every test reads ovgpu_debug_option("chol_wide_factorisations"), a name the library did not know before this path existed."""
import numpy as np
import pytest

from open_vins_amd import capi, synth
from parity_util import GATE_MARGIN
from test_gpu_parity import TOL_CHI2, TOL_DX, TOL_P

pytestmark = pytest.mark.gpu

WIDE_D = [257, 271, 272, 273, 300, 511]
COUNTER = "chol_wide_factorisations"


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


# --------------------------------------------------------------------------- 1, 2, 6: ovgpu_ekf_update
_dense = {}


def dense_case(D):
    """20 clones and padding rows of P up to N = D + 40, a random SPD P (eigenvalues 1e-3 .. 1: condition 1e3), H with D + 8 rows over a shuffled
    subset of the covariance's columns, sigma^2 = 1; expected dx and P' in float64 numpy.  Built once per D and never modified."""
    if D not in _dense:
        rng = np.random.default_rng(1000 + D)
        prob = synth.make_problem(1, C=20, K=1, F=4, seed=7)
        N = D + 40
        assert N > prob.N
        Q, _ = np.linalg.qr(rng.normal(size=(N, N)))
        P = (Q * np.logspace(-3, 0, N)) @ Q.T
        prob.N, prob.P = N, np.ascontiguousarray(0.5 * (P + P.T))
        cols = rng.permutation(N)[:D].astype(np.int32)
        H = rng.normal(size=(D + 8, D)) / np.sqrt(D)
        r = rng.normal(size=D + 8) * 0.01
        S = H @ prob.P[np.ix_(cols, cols)] @ H.T + np.eye(D + 8)
        K = np.linalg.solve(S, H @ prob.P[cols, :]).T  # P_c H^T S^-1 (S symmetric)
        _dense[D] = dict(prob=prob, cols=cols, H=H, r=r, dx=K @ r, P=prob.P - K @ H @ prob.P[cols, :])
        for v in _dense[D].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _dense[D]


def dense_run(Updater, D, wide=1, **opts):
    c = dense_case(D)
    up = Updater(capi.default_options(**opts))
    up.set_problem(c["prob"])
    up.debug_option("chol_wide", wide)
    assert up.debug_option(COUNTER) == 0
    dx, P = up.ekf_update(c["H"], c["r"], c["cols"], 1.0)
    n = up.debug_option(COUNTER)
    up.close()
    return dx, P, n


@pytest.mark.parametrize("D", WIDE_D)
def test_ekf_update_against_numpy_and_the_stepwise_kernels(Updater, D):
    c = dense_case(D)
    dx, P, n = dense_run(Updater, D)
    print(f"D {D} against numpy: dx {_rel(dx, c['dx']):.3e}  P {_rel(P, c['P']):.3e}")
    assert n == 1
    assert _rel(dx, c["dx"]) < 1e-8 and _rel(P, c["P"]) < 1e-9
    assert np.array_equal(P, P.T)
    dx0, P0, n0 = dense_run(Updater, D, wide=0)
    print(f"D {D} against the step-wise kernels: dx {_rel(dx, dx0):.3e}  P {_rel(P, P0):.3e}")
    assert n0 == 0
    assert _rel(dx0, c["dx"]) < 1e-8 and _rel(P0, c["P"]) < 1e-9
    assert _rel(dx, dx0) < 1e-10 and _rel(P, P0) < 1e-11


def test_no_single_launch_cholesky_selects_the_stepwise_kernels(Updater):
    dx, P, n = dense_run(Updater, 300, no_single_launch_cholesky=1)
    dx0, P0, n0 = dense_run(Updater, 300, wide=0)
    assert n == 0 and n0 == 0
    assert _rel(dx, dx0) < 1e-10 and _rel(P, P0) < 1e-11


@pytest.mark.parametrize("D", [240, 256])
def test_up_to_256_columns_nothing_changes(Updater, D):
    dx, P, n = dense_run(Updater, D)
    dx0, P0, n0 = dense_run(Updater, D, wide=0)
    assert n == 0 and n0 == 0
    assert np.array_equal(dx, dx0) and np.array_equal(P, P0)
    c = dense_case(D)
    assert _rel(dx, c["dx"]) < 1e-8 and _rel(P, c["P"]) < 1e-9


# --------------------------------------------------------------------------- 3, 5: the Gram route of ovgpu_msckf_update at D = 266
C_MSCKF = 42  # x 1 camera with online extrinsics and intrinsics: 14 + 6 * 42 = 266 columns, clone c at columns 14 + 6 c (calibration first)
_msckf = {}


def msckf_case(oracle, singular=None):
    """48 tracks over 42 clones; singular = (i, j): clone j's rows and columns of P are a copy of clone i's (positive semi-definite, rank N - 6)"""
    if singular not in _msckf:
        prob = synth.make_problem(1, C=C_MSCKF, K=1, F=48, seed=11)
        assert prob.Dmax == 266
        if singular:
            A = np.eye(prob.N)
            i, j = int(prob.clone_cov_id[singular[0]]), int(prob.clone_cov_id[singular[1]])
            A[j:j + 6, :] = 0.0
            A[j:j + 6, i:i + 6] = np.eye(6)
            prob.P = A @ prob.P @ A.T
        opts = capi.default_options(chi2_multipler=1.0)
        v = capi.Views(prob)
        tri = oracle.triangulate(opts, v)
        ref = oracle.msckf_update(opts, v, given=tri)
        gate = np.isfinite(ref["chi2"]) & (ref["chi2_thresh"] > 0)
        assert ref["stats"]["status"] == 0 and ref["stats"]["n_used"] >= 20
        # the oracle alone leaves nothing within the excuse's margin of its gate: accept sets are compared as they are
        assert np.abs(ref["chi2"][gate] / ref["chi2_thresh"][gate] - 1.0).min() > GATE_MARGIN
        _msckf[singular] = (prob, opts, tri, ref)
    return _msckf[singular]


def msckf_up(Updater, case):
    prob, opts, tri, ref = case
    up = Updater(opts)
    up.debug_option("chol_wide", 1)
    up.set_problem(prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    return up


def test_msckf_gram_route_both_factorisations(Updater, oracle):
    case = msckf_case(oracle)
    ref = case[3]
    up = msckf_up(Updater, case)
    out = up.update()
    print(f"MSCKF D 266: used {out['stats']['n_used']}  dx {_rel(out['dx'], ref['dx']):.3e}  P {_rel(out['P'], ref['P']):.3e}")
    assert out["route"] == capi.COMPRESS_GRAM and up.debug_option(COUNTER) == 2
    assert np.array_equal(out["feat_status"], ref["feat_status"])
    assert _rel(out["dx"], ref["dx"]) < TOL_DX and _rel(out["P"], ref["P"]) < TOL_P
    assert np.abs(out["clone_q_p"] - ref["clone_q_p"]).max() < 1e-9
    up.close()


@pytest.mark.parametrize("pair", [(28, 29), (40, 41)], ids=["first_panel", "second_panel"])
def test_semi_definite_prior_repeats_through_householder(Updater, oracle, pair):
    """Clone 29 (columns 188 .. 193) a copy of clone 28: the pivot fails in the FIRST panel; the Schur step, the second panel and the place step do
    nothing.  Clone 41 (columns 260 .. 265) a copy of clone 40: the first 256 columns are positive definite, the pivot fails in the SECOND panel.
    Either way flags[0] is what the host sees, and the call repeats through the Householder route (whose own factorisation is two panels again)."""
    case = msckf_case(oracle, pair)
    ref = case[3]
    up = msckf_up(Updater, case)
    out = up.update()
    print(f"semi-definite {pair}: dx {_rel(out['dx'], ref['dx']):.3e}  P {_rel(out['P'], ref['P']):.3e}  wide factorisations {up.debug_option(COUNTER)}")
    assert out["stats"]["status"] == 0 and out["route"] == capi.COMPRESS_TSQR
    assert np.array_equal(out["feat_status"], ref["feat_status"])
    assert _rel(out["dx"], ref["dx"]) < 1e-7 and _rel(out["P"], ref["P"]) < 1e-8  # (tests/test_gpu_parity.py's bounds for this prior)
    assert np.abs(out["clone_q_p"] - ref["clone_q_p"]).max() < 1e-9
    assert up.debug_option(COUNTER) == 3  # the Gram attempt's two and the Householder route's one
    up.close()


def test_follower_timeout_repeats_with_the_stepwise_kernels(Updater, oracle):
    """"chol_follow_spin_limit" = 0: every follower of the first panel gives up, nothing behind it runs, the state stays untouched and the call
    repeats with c->no_chol_pipe, which must reach k_ekf_chol_step: the result IS the step-wise one, and the counter holds the first attempt only
    (its two factorisations were both enqueued before the host saw the flag)."""
    case = msckf_case(oracle)
    prob, ref = case[0], case[3]
    steps = msckf_up(Updater, case)
    steps.debug_option("chol_wide", 0)
    want = steps.update()
    assert steps.debug_option(COUNTER) == 0
    steps.close()
    up = msckf_up(Updater, case)
    assert up.debug_option("chol_follow_spin_limit", 0) == 1 << 22
    up.update_async()
    with pytest.raises(capi.OvgpuError):
        up.synchronize()
    st = up.get_state()
    assert np.array_equal(st["P"], prob.P) and np.array_equal(st["clone_q_p"], prob.clone_q_p)
    assert up.debug_option(COUNTER, 0) == 2
    out = up.update()
    assert up.debug_option("chol_timeouts") == 1 and up.debug_option(COUNTER) == 2
    assert np.array_equal(out["feat_status"], ref["feat_status"])
    assert np.array_equal(out["dx"], want["dx"]) and np.array_equal(out["P"], want["P"])
    up.debug_option("chol_follow_spin_limit", 1 << 22)
    up.reset_state()
    again = up.update()
    assert up.debug_option("chol_timeouts") == 1 and up.debug_option(COUNTER) == 4
    assert _rel(again["dx"], want["dx"]) < 1e-10 and _rel(again["P"], want["P"]) < 1e-11
    up.close()


# --------------------------------------------------------------------------- 4: SLAM, 30 clones stereo (208 columns) and global landmarks
def slam_batch(L, F, seed):
    prob = synth.make_slam_problem(2, L=L, lm_rep=capi.REP_GLOBAL_3D, seed=seed)
    q = prob.subset(np.arange(F))
    q.lm_index = np.ascontiguousarray(np.arange(F), dtype=np.int32)
    return q


def test_slam_update_against_the_oracle(Updater, oracle):
    """20 landmarks, all with columns: D = 208 + 60 = 268; a batch of 12 features"""
    q = slam_batch(20, 12, 3)
    opts = capi.default_options(chi2_multipler=1.0)
    ref = oracle.slam_update(opts, capi.Views(q))
    gate = np.isfinite(ref["chi2"]) & (ref["chi2_thresh"] > 0)
    assert np.abs(ref["chi2"][gate] / ref["chi2_thresh"][gate] - 1.0).min() > GATE_MARGIN and ref["stats"]["n_used"] >= 6
    up = Updater(opts)
    up.debug_option("chol_wide", 1)
    up.set_slam_problem(q)
    out = up.slam_update()
    print(f"SLAM D 268: used {out['stats']['n_used']}  dx {_rel(out['dx'], ref['dx']):.3e}  P {_rel(out['P'], ref['P']):.3e}")
    assert up.debug_option(COUNTER) >= 1
    assert np.array_equal(out["feat_status"], ref["feat_status"])
    np.testing.assert_allclose(out["chi2"][gate], ref["chi2"][gate], rtol=TOL_CHI2)
    assert out["stats"]["n_used"] == ref["stats"]["n_used"]
    assert _rel(out["dx"], ref["dx"]) < 10 * TOL_DX
    assert _rel(out["P"], ref["P"]) < 10 * TOL_P and np.array_equal(out["P"], out["P"].T)
    assert np.abs(out["landmarks"] - ref["landmarks"]).max() < 1e-9
    up.close()


def test_slam_chunks_equal_the_chain(Updater):
    """ovgpu_slam_update_chunked in two chunks against ovgpu_set_active_landmarks / ovgpu_set_features / ovgpu_slam_update per chunk on a second
    context, for equality.  A chunk's landmarks alone get columns, so the chunks hold 20 landmarks each (40 resident): D = 268 in both."""
    import test_gpu_slam_chunked as sc
    q = slam_batch(40, 40, 5)
    opts = capi.default_options(chi2_multipler=1.0)
    first = [0, 20, 40]

    def wide(o):
        u = Updater(o)
        u.debug_option("chol_wide", 1)
        return u

    out, up = sc.chunked(wide, opts, q, first, keep=True)
    ref, upc = sc.chain(wide, opts, q, first, keep=True)
    n, nc = up.debug_option(COUNTER), upc.debug_option(COUNTER)
    up.close(), upc.close()
    assert n >= 2 and nc == n and up is not upc
    assert sum(s["n_used"] for s in out["stats"]) >= 12
    sc.assert_equal_outputs(out, ref, "two chunks of 20 landmarks")
