"""GPU tests (`-m gpu`) of ovgpu_slam_update_chunked: every chunk of a frame's SLAM update (the reference calls UpdaterSLAM::update once per
max_slam_in_update features, VioManager.cpp:529-547, chunk k + 1 linearised at the state chunk k left) in one device pass.

Three comparators:
 1. the documented chain — ovgpu_set_active_landmarks / ovgpu_set_features / ovgpu_slam_update per chunk — on a second context of the same
    library: statuses, chi2, thresholds, every chunk's dx, P', the clone / calibration / intrinsic values and all landmarks are compared for
    EQUALITY (the entry enqueues the same kernels on the same inputs; measured on the MI355X: every difference is 0);
 2. the oracle's slam_update chained chunk by chunk, with the bounds of tests/test_gpu_parity.py's test_slam_update_parity* (10 TOL_DX on dx,
    10 TOL_P on P', TOL_CHI2, 1e-9 on the landmarks; imported).  The gate excuse (parity_util.GATE_MARGIN) is not needed: for the seeds used the
    ORACLE ALONE leaves 0 features within GATE_MARGIN of a threshold in any chunk — counted on the CPU when the seeds were chosen and asserted
    again here on the oracle's own numbers — so accept and reject sets are compared as they are;
 3. n_chunks = 1 against one ovgpu_slam_update under the batch's active set, for equality.
States: synth.make_slam_problem, 30 clones, stereo."""
import copy

import numpy as np
import pytest

from open_vins_amd import capi, synth
from parity_util import GATE_MARGIN
from test_gpu_parity import TOL_CHI2, TOL_DX, TOL_P

pytestmark = pytest.mark.gpu

REPS6 = [capi.REP_GLOBAL_3D, capi.REP_ANCHORED_3D, capi.REP_GLOBAL_3D, capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, capi.REP_GLOBAL_FULL_INVERSE_DEPTH,
         capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE]
D0 = 208  # 30 clones, 2 cameras with extrinsics and intrinsics
OUT_KEYS = ("feat_status", "chi2", "chi2_thresh", "dx_seq", "P", "landmarks", "clone_q_p", "calib_q_p", "intrinsics")


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    assert hasattr(capi.load(), "ovgpu_slam_update_chunked"), "the library does not export ovgpu_slam_update_chunked"
    return UpdaterMSCKF


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def mixed(L):
    return np.array((REPS6 * ((L + 5) // 6))[:L], np.int32)


def problem(L, seed, reps=None, **kw):
    return synth.make_slam_problem(2, L=L, lm_rep=mixed(L) if reps is None else reps, seed=seed, **kw)


def batch_of(prob, ids):
    q = prob.subset(ids)
    q.lm_index = np.ascontiguousarray(ids, dtype=np.int32)
    return q


def chunked(Updater, opts, q, first, sigma=None, mult=None, keep=False, fail_chunk=None):
    up = Updater(opts)
    up.set_slam_problem(q)
    if sigma is not None or mult is not None:
        up.set_feature_options(sigma_pix=sigma, chi2_multipler=mult)
    if fail_chunk is not None:
        up.debug_option("slam_chunked_fail_chunk", fail_chunk)
    out = up.slam_update_chunked(q.lm_index, first)
    out.update(up.get_state(P=False))
    if keep:
        return out, up
    up.close()
    return out


def chain(Updater, opts, q, first, sigma=None, mult=None, keep=False):
    """the documented chain on a context of its own; empty chunks do nothing"""
    up = Updater(opts)
    up.set_slam_problem(q)
    F, n = q.F, len(first) - 1
    out = dict(feat_status=np.zeros(F, np.int32), chi2=np.zeros(F), chi2_thresh=np.zeros(F), dx_seq=np.zeros((n, q.N)), stats=[None] * n,
               P=np.array(q.P, dtype=np.float64), landmarks=np.array(q.lm_value, dtype=np.float64), p_FinG=np.zeros((F, 3)), p_FinA=np.zeros((F, 3)))
    for k in range(n):
        a, b = int(first[k]), int(first[k + 1])
        if a == b:
            continue
        qk = q.subset(np.arange(a, b))
        lm = np.ascontiguousarray(q.lm_index[a:b], dtype=np.int32)
        up.set_active_landmarks(np.unique(lm))
        up.set_features(qk)
        if sigma is not None or mult is not None:
            up.set_feature_options(sigma_pix=None if sigma is None else sigma[a:b], chi2_multipler=None if mult is None else mult[a:b])
        o = up.slam_update(lm)
        for key in ("feat_status", "chi2", "chi2_thresh"):
            out[key][a:b] = o[key]
        out["dx_seq"][k], out["P"], out["landmarks"], out["stats"][k] = o["dx"], o["P"], o["landmarks"], o["stats"]
        tri = up.get_triangulation()
        out["p_FinG"][a:b], out["p_FinA"][a:b] = tri["p_FinG"], tri["p_FinA"]
    out.update(up.get_state(P=False))
    if keep:
        return out, up
    up.close()
    return out


def oracle_chain(oracle, opts, q, first, sigma=None, mult=None):
    """the oracle's slam_update chunk by chunk on a state carried along; also the number of features within GATE_MARGIN of their gate"""
    F, n = q.F, len(first) - 1
    cur = copy.copy(q)
    out = dict(feat_status=np.zeros(F, np.int32), chi2=np.full(F, np.nan), chi2_thresh=np.full(F, np.nan), dx_seq=np.zeros((n, q.N)), n_used=[0] * n)
    for k in range(n):
        a, b = int(first[k]), int(first[k + 1])
        if a == b:
            continue
        qk = cur.subset(np.arange(a, b))
        qk.lm_index = np.ascontiguousarray(q.lm_index[a:b], dtype=np.int32)
        v = capi.Views(qk)
        ref = oracle.slam_update(opts, v, feat_sigma=None if sigma is None else sigma[a:b], feat_chi2mult=None if mult is None else mult[a:b])
        post = oracle.apply_dx(opts, v, ref["dx"])
        for key in ("feat_status", "chi2", "chi2_thresh"):
            out[key][a:b] = ref[key]
        out["dx_seq"][k], out["n_used"][k] = ref["dx"], ref["stats"]["n_used"]
        cur = copy.copy(cur)
        cur.P, cur.lm_value = ref["P"], ref["landmarks"]
        cur.clone_q_p, cur.calib_q_p, cur.intrinsics = post["clone_q_p"], post["calib_q_p"], post["intrinsics"]
    out["P"], out["landmarks"] = np.asarray(cur.P), np.asarray(cur.lm_value)
    out["clone_q_p"], out["calib_q_p"], out["intrinsics"] = cur.clone_q_p, cur.calib_q_p, cur.intrinsics
    g = np.isfinite(out["chi2"]) & (out["chi2_thresh"] > 0)
    out["near_gate"] = int((np.abs(out["chi2"][g] / out["chi2_thresh"][g] - 1.0) < GATE_MARGIN).sum())
    return out


def assert_equal_outputs(a, b, what, keys=OUT_KEYS):
    """prints the largest difference per output, then asserts equality"""
    worst = {}
    for k in keys:
        x, y = np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)
        assert x.shape == y.shape, k
        both = np.isfinite(x) & np.isfinite(y)
        assert np.array_equal(np.isfinite(x), np.isfinite(y)), k
        worst[k] = float(np.abs(x[both] - y[both]).max()) if both.any() else 0.0
    print(what + ": " + "  ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k, worst[k])


def assert_oracle(out, ref, what):
    assert ref["near_gate"] == 0  # the excuse cannot hide a failure: the oracle alone leaves nothing in the margin
    assert np.array_equal(out["feat_status"], ref["feat_status"]), what
    gate = np.isfinite(ref["chi2"])
    np.testing.assert_allclose(out["chi2"][gate], ref["chi2"][gate], rtol=TOL_CHI2)
    np.testing.assert_allclose(out["chi2_thresh"][gate], ref["chi2_thresh"][gate], rtol=1e-12)
    assert np.isnan(out["chi2"][~gate]).all()
    live = [k for k in range(ref["dx_seq"].shape[0]) if ref["n_used"][k] > 0]
    edx = max(_rel(out["dx_seq"][k], ref["dx_seq"][k]) for k in live)
    print(f"{what} against the oracle's chain: dx {edx:.3e}  P {_rel(out['P'], ref['P']):.3e}  landmarks {np.abs(out['landmarks'] - ref['landmarks']).max():.3e}")
    assert [s["n_used"] if s else 0 for s in out["stats"]] == ref["n_used"]
    assert edx < 10 * TOL_DX
    assert _rel(out["P"], ref["P"]) < 10 * TOL_P and np.array_equal(out["P"], out["P"].T)
    assert np.abs(out["landmarks"] - ref["landmarks"]).max() < 1e-9
    for k in ("clone_q_p", "calib_q_p", "intrinsics"):
        assert np.abs(out[k] - ref[k]).max() < 1e-9


FIRST_5 = [0, 9, 9, 22, 38, 50]  # five chunks of unequal size, the second empty


# --------------------------------------------------------------------------- L = 50, the whole batch in 1, 2 and 5 chunks
@pytest.mark.parametrize("first", [[0, 50], [0, 18, 50], FIRST_5], ids=["1", "2", "5"])
def test_chunks_equal_the_chain(Updater, first):
    opts = capi.default_options(chi2_multipler=1.0)
    q = batch_of(problem(50, 3), np.arange(50))
    out = chunked(Updater, opts, q, first)
    ref = chain(Updater, opts, q, first)
    assert_equal_outputs(out, ref, f"{len(first) - 1} chunk(s) against the chain")
    assert sum(s["n_used"] for s in out["stats"]) >= 30
    for k in range(len(first) - 1):
        if first[k] == first[k + 1]:
            assert not out["dx_seq"][k].any() and out["stats"][k]["n_used"] == 0 and out["stats"][k]["D"] == 0
            continue
        for key in ("n_used", "n_rows", "D", "n_rows_comp", "status", "n_gate_bound"):
            assert out["stats"][k][key] == ref["stats"][k][key], (k, key)
        assert out["stats"][k]["D"] < D0 + 3 * (first[k + 1] - first[k]) + 1


def test_five_chunks_against_the_oracle(Updater, oracle):
    """oracle alone, seed 3, chunks 9 / 0 / 13 / 16 / 12: 0 features within GATE_MARGIN of their gate"""
    opts = capi.default_options(chi2_multipler=1.0)
    q = batch_of(problem(50, 3), np.arange(50))
    assert_oracle(chunked(Updater, opts, q, FIRST_5), oracle_chain(oracle, opts, q, FIRST_5), "five chunks")


def test_one_chunk_is_the_single_call(Updater):
    opts = capi.default_options(chi2_multipler=1.0)
    q = batch_of(problem(50, 3), np.arange(50))
    out = chunked(Updater, opts, q, [0, 50])
    up = Updater(opts)
    up.set_slam_problem(q)
    up.set_active_landmarks(np.unique(q.lm_index))
    up.set_features(q)
    one = up.slam_update()
    one.update(up.get_state(P=False))
    up.close()
    one["dx_seq"] = one["dx"][None, :]
    assert_equal_outputs(out, one, "n_chunks = 1 against ovgpu_slam_update")
    assert out["stats"][0]["D"] == one["stats"]["D"] and out["stats"][0]["n_rows"] == one["stats"]["n_rows"]


# --------------------------------------------------------------------------- representations
@pytest.mark.parametrize("rep", list(range(6)) + ["mix"])
def test_representations(Updater, rep):
    """each representation alone, and 3-dof global landmarks next to single-depth ones (rows per feature follow the landmark)"""
    L = 18
    reps = np.full(L, rep, np.int32) if rep != "mix" else np.array([capi.REP_GLOBAL_3D, capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE] * (L // 2), np.int32)
    opts = capi.default_options(chi2_multipler=1.0)
    q = batch_of(problem(L, 11, reps=reps), np.arange(L))
    first = [0, 5, 12, 18]
    out, ref = chunked(Updater, opts, q, first), chain(Updater, opts, q, first)
    assert_equal_outputs(out, ref, f"representation {rep}")
    assert sum(s["n_used"] for s in out["stats"]) >= 9


# --------------------------------------------------------------------------- per-feature options that differ between chunks
def test_feature_options_per_chunk(Updater):
    opts = capi.default_options(chi2_multipler=1.0)
    q = batch_of(problem(50, 3), np.arange(50))
    first = [0, 15, 35, 50]
    sigma = np.concatenate([np.full(15, 1.0), np.full(20, 2.5), np.full(15, 0.7)])
    mult = np.concatenate([np.full(15, 1.0), np.full(20, 0.25), np.full(15, 4.0)])
    out, ref = chunked(Updater, opts, q, first, sigma, mult), chain(Updater, opts, q, first, sigma, mult)
    assert_equal_outputs(out, ref, "per-feature options")
    plain = chunked(Updater, opts, q, first)
    assert not np.array_equal(plain["chi2_thresh"][15:35], out["chi2_thresh"][15:35])  # the multiplier reached the middle chunk
    assert not np.array_equal(plain["P"], out["P"])


# --------------------------------------------------------------------------- outliers: rejections in the middle chunks
def test_outliers_rejected_in_the_middle_chunks(Updater, oracle):
    """oracle alone, seed 7, L = 30, outlier_frac 0.3, chunks of 10: 0 features within GATE_MARGIN of their gate"""
    opts = capi.default_options(chi2_multipler=1.0)
    q = batch_of(problem(30, 7, outlier_frac=0.3), np.arange(30))
    first = [0, 10, 20, 30]
    out, ref = chunked(Updater, opts, q, first), chain(Updater, opts, q, first)
    assert_equal_outputs(out, ref, "outliers")
    assert (out["feat_status"][10:20] == capi.FEAT_CHI2_REJECTED).any() and (out["feat_status"][10:20] == capi.FEAT_USED).any()
    assert_oracle(out, oracle_chain(oracle, opts, q, first), "outliers")


# --------------------------------------------------------------------------- L = 100: all columns exceed 383, every chunk stays small
def test_100_landmarks_in_chunks_of_25(Updater):
    opts = capi.default_options(chi2_multipler=1.0)
    q = batch_of(problem(100, 5), np.arange(100))
    dof = int(np.where(mixed(100) == capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE, 1, 3).sum())
    assert 383 < D0 + dof <= 511
    first = [0, 25, 50, 75, 100]
    out, ref = chunked(Updater, opts, q, first), chain(Updater, opts, q, first)
    assert_equal_outputs(out, ref, "L = 100")
    assert all(s["D"] <= D0 + 75 for s in out["stats"]) and sum(s["n_used"] for s in out["stats"]) >= 60


def test_100_landmarks_against_the_oracle(Updater, oracle):
    """oracle alone, seed 5, the first 30 tracks of 100 landmarks in chunks of 10: 0 features within GATE_MARGIN of their gate"""
    opts = capi.default_options(chi2_multipler=1.0)
    q = batch_of(problem(100, 5), np.arange(30))
    first = [0, 10, 20, 30]
    assert_oracle(chunked(Updater, opts, q, first), oracle_chain(oracle, opts, q, first), "L = 100")


# --------------------------------------------------------------------------- what the call leaves behind
def test_state_left_behind(Updater):
    opts = capi.default_options(chi2_multipler=1.0)
    q = batch_of(problem(50, 3), np.arange(50))
    first = [0, 18, 50]
    out, up = chunked(Updater, opts, q, first, keep=True)
    ref, up2 = chain(Updater, opts, q, first, keep=True)
    assert np.array_equal(up.get_landmarks()["value"], out["landmarks"])
    post = up.get_state(P=True)
    assert np.array_equal(post["P"], out["P"])
    tri = up.get_triangulation()  # the whole batch: every chunk's positions as its gather left them
    # (k_slam_gather writes the position where the representation keeps it: the global frame, or the anchor camera's)
    anchored = mixed(50)[q.lm_index] >= capi.REP_ANCHORED_3D
    assert tri["p_FinG"].shape == (50, 3) and anchored.any() and (~anchored).any()
    assert np.array_equal(tri["p_FinG"][~anchored], ref["p_FinG"][~anchored]) and np.array_equal(tri["p_FinA"][anchored], ref["p_FinA"][anchored])
    assert np.abs(tri["p_FinG"][~anchored]).max() > 0 and np.abs(tri["p_FinA"][anchored]).max() > 0
    # the active set in force is "all": the batch has to be handed over again, as after ovgpu_set_active_landmarks(n < 0) ...
    with pytest.raises(capi.OvgpuError) as err:
        up.slam_update(q.lm_index)
    assert err.value.code == capi.ERR_NO_STATE
    # ... and then a following update and a batched marginalisation do what they do after the chain
    up2.set_active_landmarks(None)
    nxt = []
    for u in (up, up2):
        u.set_features(q)
        o = u.slam_update(q.lm_index)
        assert o["stats"]["D"] == D0 + int(np.where(mixed(50) == capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE, 1, 3).sum())
        lm = u.get_landmarks()
        free = [l for l in range(50) if lm["feat_rep"][l] < capi.REP_ANCHORED_3D][:4]
        u.state_marginalize_many([int(lm["cov_id"][l]) for l in free], [3] * len(free))
        o.update(u.get_state(P=True))
        o["lm_after"] = u.get_landmarks()["value"]
        nxt.append(o)
    for k in ("feat_status", "chi2", "dx", "P", "clone_q_p", "lm_after"):
        assert np.array_equal(nxt[0][k], nxt[1][k], equal_nan=True), k
    up.close(), up2.close()


# --------------------------------------------------------------------------- checks: codes, and nothing changes
def test_refused_calls_change_nothing(Updater):
    opts = capi.default_options(chi2_multipler=1.0)
    q = batch_of(problem(50, 3), np.arange(50))
    up = Updater(opts)
    F, N, L = q.F, q.N, 50
    st, x2, thr, P, lm = np.zeros(F, np.int32), np.zeros(F), np.zeros(F), np.zeros((N, N)), np.zeros((L, 3))
    i = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(capi.c_int32_p)
    d = lambda a: a.ctypes.data_as(capi.c_double_p)

    def rc(n, first, lm_index):
        first = None if first is None else np.ascontiguousarray(first, dtype=np.int32)
        lmi = None if lm_index is None else np.ascontiguousarray(lm_index, dtype=np.int32)
        return up.lib.ovgpu_slam_update_chunked(up._ctx, n, i(first), i(lmi), st.ctypes.data_as(capi.c_int32_p), d(x2), d(thr), None, d(P), d(lm), None)

    assert up.lib.ovgpu_slam_update_chunked(None, 1, i([0, F]), i(q.lm_index), None, None, None, None, None, None, None) == capi.ERR_INVALID
    assert rc(1, [0, F], q.lm_index) == capi.ERR_NO_STATE  # no state
    up.set_slam_problem(q)
    before = up.get_state(P=True)
    lm_before = up.get_landmarks()["value"]
    bad = q.lm_index.copy()
    bad[7] = L
    neg = q.lm_index.copy()
    neg[0] = -1
    for n, first, lmi in [(2, None, q.lm_index), (0, [0], q.lm_index), (2, [0, 30, 20], q.lm_index), (2, [0, 60, F], q.lm_index), (2, [1, 20, F], q.lm_index),
                          (2, [0, 20, F - 1], q.lm_index), (2, [0, 20, F], None), (2, [0, 20, F], bad), (2, [0, 20, F], neg)]:
        assert rc(n, first, lmi) == capi.ERR_INVALID, (n, first)
    after = up.get_state(P=True)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert np.array_equal(up.get_landmarks()["value"], lm_before)
    out = up.slam_update_chunked(q.lm_index, [0, 20, F])  # the refused calls left the batch resident
    assert sum(s["n_used"] for s in out["stats"]) >= 30
    # no batch (the call above ended with the all-landmarks map: the batch has to be handed over again)
    assert rc(2, [0, 20, F], q.lm_index) == capi.ERR_NO_STATE
    up.close()
    # no landmarks
    up = Updater(opts)
    up.set_problem(synth.make_problem(2, F=F, seed=3))
    assert rc(1, [0, F], q.lm_index) == capi.ERR_NO_STATE
    up.close()


def test_a_chunk_of_more_than_511_columns_is_refused_before_any_work(Updater):
    opts = capi.default_options(chi2_multipler=1.0)
    L = 120
    q = batch_of(problem(L, 3), np.arange(L))
    up = Updater(opts)
    up.set_slam_problem(q)
    before, lm_before = up.get_state(P=True), up.get_landmarks()["value"]
    with pytest.raises(capi.OvgpuError) as err:
        up.slam_update_chunked(q.lm_index, [0, 2, L])  # chunk 1: 118 landmarks of 314 dof next to the 208 other columns
    assert err.value.code == capi.ERR_CAPACITY and "chunk 1" in str(err.value)
    after = up.get_state(P=True)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert np.array_equal(up.get_landmarks()["value"], lm_before)
    out = up.slam_update_chunked(q.lm_index, [0, 30, 60, 90, L])  # the same batch in chunks that fit
    assert sum(s["n_used"] for s in out["stats"]) >= 70
    up.close()


# --------------------------------------------------------------------------- the restore-and-chain path
def test_a_failed_chunk_restores_the_entry_state_and_runs_the_chain(Updater):
    opts = capi.default_options(chi2_multipler=1.0)
    q = batch_of(problem(50, 3), np.arange(50))
    first = [0, 18, 30, 50]
    out, up = chunked(Updater, opts, q, first, keep=True, fail_chunk=1)
    assert up.debug_option("slam_chunked_fallbacks") == 1
    assert up.debug_option("slam_chunked_fail_chunk") == -1  # one-shot
    ref = chain(Updater, opts, q, first)
    assert_equal_outputs(out, ref, "restore-and-chain path")
    up.close()
    out, up = chunked(Updater, opts, q, first, keep=True)
    assert up.debug_option("slam_chunked_fallbacks") == 0
    assert_equal_outputs(out, ref, "the pass itself")
    up.close()


# --------------------------------------------------------------------------- a batch that outgrows every buffer a chunk's batch pointed into
@pytest.mark.parametrize("fail_chunk", [None, 0], ids=["the_pass", "restore_and_chain"])
def test_a_larger_batch_after_a_chunked_call(Updater, fail_chunk):
    """The tracks of landmarks 0..5 in chunks of 2 / 0 / 4 through the chunked entry (fail_chunk = 0: through its restore-and-chain path) and through
    the chain, then all twelve tracks with per-feature options on both contexts: F and M above anything either context has held, so every batch
    array and per-feature option buffer reallocates behind the chunks' batches.  Equality throughout; both contexts close."""
    opts = capi.default_options(chi2_multipler=1.0)
    p = problem(12, 3)
    q6, q12 = batch_of(p, np.arange(6)), batch_of(p, np.arange(12))
    assert q12.F > q6.F and q12.M > q6.M
    first = [0, 2, 2, 6]
    out, up = chunked(Updater, opts, q6, first, keep=True, fail_chunk=fail_chunk)
    ref, up2 = chain(Updater, opts, q6, first, keep=True)
    assert up.debug_option("slam_chunked_fallbacks") == (0 if fail_chunk is None else 1)
    assert_equal_outputs(out, ref, "the first batch")
    assert sum(s["n_used"] for s in out["stats"] if s) >= 3
    sigma, mult = np.linspace(0.8, 2.0, q12.F), np.linspace(0.5, 3.0, q12.F)
    up2.set_active_landmarks(None)  # (the chunked call left "all" in force itself)
    nxt = []
    for u in (up, up2):
        u.set_features(q12)
        u.set_feature_options(sigma_pix=sigma, chi2_multipler=mult)
        o = u.slam_update(q12.lm_index)
        o.update(u.get_state(P=False))
        nxt.append(o)
    assert_equal_outputs(nxt[0], nxt[1], "the larger batch", keys=("feat_status", "chi2", "chi2_thresh", "dx", "P", "landmarks", "clone_q_p", "calib_q_p", "intrinsics"))
    assert nxt[0]["stats"]["n_used"] >= 6
    up.close(), up2.close()
