"""GPU tests (`-m gpu`): the resident window against the oracle on states whose clones and landmarks INTERLEAVE in covariance order, the order a
running filter produces (StateHelper::clone appends every clone behind the landmarks already resident, delayed initialisation appends landmarks
behind that clone, a long-lived landmark ends up in front of every clone) and synth.make_slam_problem never does.  The orders, the reordering and
the batches: tests/window_order.py; tests/test_window_order_cpu.py holds every batch of this file to the oracle alone (equivariance of the
oracle within 1e-12, a feature used, the planted outlier rejected, nothing within parity_util.GATE_MARGIN of its gate), which is what lets the
accept sets be compared as they are.

Every entry runs on the reordered state against the oracle ON THE SAME STATE, with the bounds of the entry's existing test:
  ovgpu_slam_update, every "slam_fused" level      tests/test_gpu_slam_fused.py::check_oracle (test_gpu_parity.py::test_slam_update_parity's: chi2 TOL_CHI2,
                                                   dx 10 TOL_DX = 1e-7, P' 10 TOL_P = 1e-8 and exactly symmetric, landmarks and poses 1e-9)
  ovgpu_slam_update_chunked                        tests/test_gpu_slam_chunked.py::assert_oracle, and assert_equal_outputs against the chain of single calls
  ovgpu_slam_compress, Householder route           tests/test_gpu_parity.py::test_slam_mode_a_compressed_system (P' 1e-8, dx 1e-7 through the stock ekf_update)
  ovgpu_slam_compress, "slam_mode_a" = 1           tests/test_gpu_slam_mode_a.py::check (P' TOL_P = 1e-9, dx TOL_DX = 1e-8)
  ovgpu_msckf_update_lm, ovgpu_msckf_update        tests/test_gpu_msckf_lm.py::check_oracle (dx 1e-7, P' 1e-8, poses 1e-9), check_landmarks (value + dx, exactly)
  ovgpu_slam_delayed_init(_fused)                  tests/test_gpu_delayed_init_fused.py::_check
  ovgpu_slam_change_anchor(s_batched)              tests/test_gpu_anchor_batch.py::check_against (P' 1e-12, values rtol 1e-12 / atol 1e-13)
  ovgpu_state_marginalize_batched                  bit for bit against np.delete (tests/test_gpu_marginalize_batch.py)
  "gram_wide" = 1                                  tests/test_gpu_gram_wide.py::hold (chi2 1e-8, dx 1e-8, P' 1e-9, landmarks and poses 1e-9)
  the life cycle's covariance steps                tests/test_gpu_parity.py::test_state_propagate_clone_marginalize_parity (propagate 1e-14, augment_clone
                                                   1e-15, marginalize bit for bit)
Every fused case asserts "last_feature_kernel" against the restated rule (window_order.Case.kernel): a silent fall-back to the general kernel fails.
"""
import copy
import ctypes

import numpy as np
import pytest

import test_gpu_anchor_batch as aab
import test_gpu_slam_chunked as sc
import window_order as wo
from open_vins_amd import capi
from test_gpu_parity import TOL_CHI2, TOL_DX, TOL_P

pytestmark = pytest.mark.gpu

STATE_KEYS = ("clone_q_p", "calib_q_p", "intrinsics")
WORST = {}    # entry -> {quantity: largest deviation against the oracle}
KERNELS = {}  # fused case -> the kernel the library reported


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def context(Updater, opts, **debug):
    """a context with its switches set before anything is uploaded"""
    up = Updater(opts)
    for name, val in debug.items():
        up.debug_option(name, val)
    return up


def note(entry, what, **dev):
    print(f"{what}: " + "  ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    w = WORST.setdefault(entry, {})
    for k, v in dev.items():
        w[k] = max(w.get(k, 0.0), float(v))


def hold_slam(entry, oracle, opts, prob, out, ref, what, tol_dx=10 * TOL_DX, tol_p=10 * TOL_P, symmetric=True):
    """tests/test_gpu_slam_fused.py::check_oracle; out carries the pose tables read back after the call.  symmetric = False: the prior is not
    symmetric bit for bit (EKFPropagation leaves Phi P Phi^T as computed, in the reference too), and the update keeps what it finds below the diagonal
    where the reference mirrors the upper triangle (StateHelper.cpp:166-167): a difference of the prior's own asymmetry, ~1e-20 here."""
    assert wo.near_gate(ref) == 0
    assert np.array_equal(out["feat_status"], ref["feat_status"]), what
    gate = np.isfinite(ref["chi2"])
    post = oracle.apply_dx(opts, capi.Views(prob), ref["dx"])
    dev = dict(chi2=np.abs(out["chi2"][gate] / ref["chi2"][gate] - 1.0).max(), dx=_rel(out["dx"], ref["dx"]), P=_rel(out["P"], ref["P"]),
               landmarks=np.abs(out["landmarks"] - ref["landmarks"]).max(), poses=max(np.abs(out[k] - post[k]).max() for k in STATE_KEYS))
    note(entry, what, **dev)
    np.testing.assert_allclose(out["chi2"][gate], ref["chi2"][gate], rtol=TOL_CHI2)
    np.testing.assert_allclose(out["chi2_thresh"][gate], ref["chi2_thresh"][gate], rtol=1e-12)
    assert np.isnan(out["chi2"][~gate]).all()
    assert out["stats"]["n_used"] == ref["stats"]["n_used"] and out["stats"]["n_rows"] == ref["stats"]["n_rows"]
    assert dev["dx"] < tol_dx
    assert dev["P"] < tol_p and (np.array_equal(out["P"], out["P"].T) or not symmetric)
    assert dev["landmarks"] < 1e-9 and dev["poses"] < 1e-9


def slam_update(up, prob, active=None):
    up.set_slam_problem(prob)
    if active is not None:
        up.set_active_landmarks(active)
        up.set_features(prob)
    out = up.slam_update(prob.lm_index)
    out.update(up.get_state(P=False))
    return out


# --------------------------------------------------------------------------- ovgpu_slam_update: the general kernel and every fused level
@pytest.mark.parametrize("cid", [c.id for c in wo.CASES])
def test_slam_update(Updater, oracle, cid):
    case = wo.BY_ID[cid]
    p, opts = case.prob, case.opts()
    ref, app = wo.oracle_pair(oracle, case)
    assert ref["feat_status"][case.rejected] == capi.FEAT_CHI2_REJECTED and (ref["feat_status"] == capi.FEAT_USED).any()
    up = context(Updater, opts, **({"slam_fused": case.fused} if case.fused else {}))
    out = slam_update(up, p)
    kernel, batches = up.debug_option("last_feature_kernel"), up.debug_option("slam_fused_batches")
    lm = up.get_landmarks()
    up.close()
    assert kernel == case.kernel, (cid, kernel, case.kernel)  # a silent fall-back to the general kernel fails here
    if case.fused:
        assert kernel in (4, 5, 6, 7) and batches == 1
        KERNELS[cid] = kernel
    else:
        assert kernel == 0 and batches == 0
    hold_slam("ovgpu_slam_update" + (f', "slam_fused" = {case.fused}' if case.fused else ", general kernel"), oracle, opts, p, out, ref, f"{cid} (kernel {kernel})")
    # every landmark is corrected by ITS rows of dx (one float64 add of the returned dx: exact), wherever they lie among the clones' rows
    assert np.array_equal(out["landmarks"], wo.corrected(p, out["dx"]))
    assert np.array_equal(lm["value"], out["landmarks"]) and np.array_equal(lm["cov_id"], p.lm_cov_id)
    # ... and the appended state's result, permuted, within the same bounds (the oracle's own floor is 1e-12)
    assert _rel(out["dx"], app["dx"]) < 10 * TOL_DX and _rel(out["P"], app["P"]) < 10 * TOL_P


# --------------------------------------------------------------------------- ovgpu_slam_update_chunked
@pytest.mark.parametrize("level", [0, 2], ids=["general", "fused2"])
def test_chunks_from_different_landmark_groups(Updater, oracle, level):
    """Two chunks whose active sets are the first and the last landmark group of `steady`: against the oracle's chain of single updates, and
    bit for bit against the documented chain of single calls."""
    q, first = wo.chunk_batch()
    opts = capi.default_options(chi2_multipler=1.0)
    make = (lambda o: context(Updater, o, slam_fused=level)) if level else Updater
    ref = sc.oracle_chain(oracle, opts, q, first)
    assert all(n >= 1 for n in ref["n_used"])
    out, up = sc.chunked(make, opts, q, first, keep=True)
    kernel = up.debug_option("last_feature_kernel")
    up.close()
    sc.assert_oracle(out, ref, f"two chunks on steady, slam_fused {level} (kernel {kernel})")
    note("ovgpu_slam_update_chunked", f"two chunks, slam_fused {level}", dx=max(_rel(out["dx_seq"][k], ref["dx_seq"][k]) for k in (0, 1)),
         P=_rel(out["P"], ref["P"]), landmarks=np.abs(out["landmarks"] - ref["landmarks"]).max())
    sc.assert_equal_outputs(out, sc.chain(make, opts, q, first), "two chunks against the chain of single calls")
    reps = wo.lm_reps(q)
    sets = [np.unique(q.lm_index[a:b]) for a, b in zip(first[:-1], first[1:])]
    assert not set(sets[0]) & set(sets[1]) and q.lm_cov_id[sets[0]].max() < q.clone_cov_id.max() < q.lm_cov_id[sets[1]].min()
    if level:  # the last chunk decides what is reported: 5 with a single-depth landmark in it, 4 without
        assert kernel == (5 if (reps[sets[1]] == wo.SINGLE).any() else 4)
        KERNELS[f"chunked-fused{level}-steady"] = kernel


# --------------------------------------------------------------------------- ovgpu_slam_compress
@pytest.mark.parametrize("route", ["householder", "slam_mode_a"])
@pytest.mark.parametrize("order", ["steady", "straddle"])
def test_compress(Updater, oracle, order, route):
    case = wo.BY_ID[f"general-{order}"]
    p, opts = case.prob, case.opts()
    ref, _ = wo.oracle_pair(oracle, case)
    up = context(Updater, opts, **({"slam_mode_a": 1} if route == "slam_mode_a" else {}))
    up.set_slam_problem(p)
    cmp = up.slam_compress()
    P_after, lm_after = up.get_state()["P"], up.get_landmarks()
    count = up.debug_option("slam_mode_a_compressions") if route == "slam_mode_a" else None
    up.close()
    cols = wo.col_cov_ids(p)
    assert cmp["D"] == cols.size and np.array_equal(cmp["col_cov_id"], cols) and np.all(np.diff(cmp["col_cov_id"]) > 0)
    assert np.array_equal(cmp["col_cov_id"], ref["col_cov_id"])
    assert np.array_equal(cmp["feat_status"], ref["feat_status"])
    assert 0 < cmp["rows"] <= cmp["D"]
    st, P1, dx1 = oracle.ekf_update(p.P, cmp["H"], cmp["r"], cmp["col_cov_id"], opts.sigma_pix ** 2)
    dev = dict(P=_rel(P1, ref["P"]), dx=_rel(dx1, ref["dx"]))
    note(f"ovgpu_slam_compress, {route}", f"{order}", **dev)
    tol_p, tol_dx = (TOL_P, TOL_DX) if route == "slam_mode_a" else (1e-8, 1e-7)
    assert st == 0 and dev["P"] < tol_p and dev["dx"] < tol_dx
    assert np.array_equal(P_after, p.P) and np.array_equal(lm_after["value"], p.lm_value)  # mode A does not touch the state
    if route == "slam_mode_a":
        assert count == 1  # the whitened route ran, not the Householder one behind the switch's back


# --------------------------------------------------------------------------- ovgpu_msckf_update_lm / ovgpu_msckf_update
def check_msckf(out, ref, what):
    """tests/test_gpu_msckf_lm.py::check_oracle"""
    note("ovgpu_msckf_update(_lm)", what, dx=_rel(out["dx"], ref["dx"]), P=_rel(out["P"], ref["P"]), poses=max(np.abs(out[k] - ref[k]).max() for k in ("clone_q_p", "calib_q_p")))
    assert np.array_equal(out["feat_status"], ref["feat_status"]) and (ref["feat_status"] == capi.FEAT_USED).sum() >= 10
    assert _rel(out["dx"], ref["dx"]) < 1e-7 and _rel(out["P"], ref["P"]) < 1e-8
    for k in ("clone_q_p", "calib_q_p"):
        assert np.abs(out[k] - ref[k]).max() < 1e-9


def hand_over(up, prob, active):
    up.set_slam_state(prob)
    up.set_active_landmarks(active)
    up.set_features(prob)


def two_from_different_groups(tokens):
    gr = wo.groups(tokens)
    return [int(gr[0][1][0]), int(gr[-1][1][0])]


def test_msckf_update_with_interleaved_landmarks(Updater, oracle):
    """The MSCKF update on `steady`: every clone column has landmark rows of P between it and the next.  Under the empty set ovgpu_msckf_update_lm
    takes the landmark-free route (fused kernel, unprojected stack, a column map with gaps in its covariance ids) and corrects EVERY resident
    landmark by dx[lm_cov_id]; ovgpu_msckf_update leaves them alone.  Under a set of two landmarks from different groups ovgpu_msckf_update
    gives those two their (zero) columns and computes the same update; ovgpu_msckf_update_lm refuses the batch, as documented."""
    p, _, tokens, _ = wo.steady_mixed()
    msckf, plain = wo.msckf_on(p)
    opts = capi.default_options(chi2_multipler=1.0)
    ref = oracle.msckf_update(opts, capi.Views(plain))
    # ---- ovgpu_msckf_update_lm, the empty set
    up = Updater(opts)
    hand_over(up, msckf, [])
    out = up.update_lm()
    check_msckf(out, ref, "ovgpu_msckf_update_lm, empty set")
    assert out["route"] == capi.COMPRESS_GRAM and up.debug_option("last_feature_kernel") in (1, 2) and up.debug_option("last_stack_raw") == 1
    want = wo.corrected(msckf, out["dx"])
    assert np.abs(want - msckf.lm_value).max(axis=1).min() > 0 and np.abs(out["dx"][msckf.lm_cov_id]).min() > 0  # the correction reaches every one
    got = up.get_landmarks()
    assert np.array_equal(out["landmarks"], want) and np.array_equal(got["value"], want)
    assert np.array_equal(got["fej"], msckf.lm_fej) and np.array_equal(got["cov_id"], msckf.lm_cov_id)
    up.close()
    # ---- ovgpu_msckf_update, the empty set and a set of two
    for active in ([], two_from_different_groups(tokens)):
        up = Updater(opts)
        hand_over(up, msckf, active)
        out = up.update()
        check_msckf(out, ref, f"ovgpu_msckf_update, active set {active}")
        lm = up.get_landmarks()
        assert np.array_equal(lm["value"], msckf.lm_value) and np.abs(out["dx"][msckf.lm_cov_id]).min() > 0
        if active:
            lm_out = up.update_lm(check=False)  # laid out with landmark columns: refused, nothing written
            assert lm_out["rc"] == capi.ERR_INVALID and not lm_out["dx"].any()
            assert np.array_equal(up.get_landmarks()["value"], msckf.lm_value)
        up.close()


def test_slam_update_under_a_set_of_two_landmarks_from_different_groups(Updater, oracle):
    """Two of the nine landmarks have columns; the other seven — in front of, between and behind them in covariance order — are corrected through
    dx[lm_cov_id] all the same."""
    p, _, tokens, _ = wo.steady_mixed()
    two = two_from_different_groups(tokens)
    q = wo.only_features(p, [int(np.flatnonzero(p.lm_index == l)[0]) for l in two])
    opts = capi.default_options(chi2_multipler=1.0)
    ref = oracle.slam_update(opts, capi.Views(q))
    assert (ref["feat_status"] == capi.FEAT_USED).all()
    up = Updater(opts)
    out = slam_update(up, q, two)
    up.close()
    assert out["stats"]["D"] == wo.col_cov_ids(q, active=two).size
    hold_slam("ovgpu_slam_update, active set of two", oracle, opts, q, out, ref, f"active set {two}")
    assert np.array_equal(out["landmarks"], wo.corrected(q, out["dx"])) and np.abs(out["landmarks"] - q.lm_value).max(axis=1).min() > 0


# --------------------------------------------------------------------------- ovgpu_slam_delayed_init(_fused)
@pytest.mark.parametrize("entry", ["chain", "fused1", "fused2"])
def test_delayed_init_behind_interleaved_landmarks(Updater, oracle, entry):
    """New landmarks get the ids from the current N upward — behind the newest clone's group — and the next SLAM update, on old and new landmarks
    together, matches the oracle on the state read back."""
    state, batch, reps, opts = wo.init_batch()
    v = capi.Views(batch)
    tri = oracle.triangulate(opts, v)
    ref = oracle.slam_delayed_init(opts, v, feat_rep=0, tri=tri, feat_rep_each=reps)
    acc = ref["lm_cov_id"] >= 0
    gate = np.isfinite(ref["chi2"])
    assert ref["rc"] == 0 and acc.sum() >= 3
    up = context(Updater, opts, **({"delayed_init_fused": 2} if entry == "fused2" else {}))
    up.set_slam_problem(batch)
    up.set_active_landmarks([])
    up.set_features(batch)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    out = up.delayed_init(0, feat_rep_each=reps, fused=entry != "chain")
    post, lm = up.get_state(P=True), up.get_landmarks()
    L0 = len(state.lm_cov_id)
    # tests/test_gpu_delayed_init_fused.py::_check
    assert np.array_equal(out["feat_status"], ref["feat_status"]) and out["N"] == ref["N"] and np.array_equal(out["lm_cov_id"], ref["lm_cov_id"])
    dof = np.where(reps == wo.SINGLE, 1, 3)
    assert np.array_equal(out["lm_cov_id"][acc], state.N + np.concatenate([[0], np.cumsum(dof[acc])[:-1]]))
    np.testing.assert_allclose(out["chi2"][gate], ref["chi2"][gate], rtol=1e-7)
    dev = dict(dx_seq=_rel(out["dx_seq"], ref["dx_seq"]), P=_rel(out["P"], ref["P"]), values=np.abs(out["lm_value"][acc] - ref["lm_value"][acc]).max(),
               existing=np.abs(lm["value"][:L0] - ref["landmarks_existing"]).max(), poses=max(np.abs(post[k] - ref[k]).max() for k in STATE_KEYS))
    note("ovgpu_slam_delayed_init" + ("" if entry == "chain" else f"_fused, level {entry[-1]}"), entry, **dev)
    np.testing.assert_allclose(out["lm_value"][acc], ref["lm_value"][acc], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(out["lm_fej"][acc], ref["lm_fej"][acc], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(lm["value"][:L0], ref["landmarks_existing"], rtol=1e-8, atol=1e-10)
    assert dev["dx_seq"] < 1e-6 and not out["dx_seq"][~acc].any() and dev["P"] < 1e-7 and dev["poses"] < 1e-9
    assert np.array_equal(post["P"], out["P"]) and np.array_equal(lm["cov_id"], np.concatenate([state.lm_cov_id, ref["lm_cov_id"][acc]]))
    assert np.abs(lm["value"][:L0] - state.lm_value).max(axis=1).min() > 0  # every resident landmark moved with the chain's corrections
    # ---- the next SLAM update on the state read back: the nine old landmarks and the new ones
    nxt = wo.after_init(state, batch, post, lm, acc)
    ref2 = oracle.slam_update(opts, capi.Views(nxt))
    assert wo.near_gate(ref2) == 0 and (ref2["feat_status"] == capi.FEAT_USED).sum() >= 3
    up.set_active_landmarks(None)
    up.set_features(nxt)
    out2 = up.slam_update(nxt.lm_index)
    out2.update(up.get_state(P=False))
    up.close()
    hold_slam("ovgpu_slam_update behind the delayed initialisation", oracle, opts, nxt, out2, ref2, f"SLAM update behind {entry}")


# --------------------------------------------------------------------------- ovgpu_slam_change_anchor(s_batched), ovgpu_state_marginalize_batched
def read_back(up, like):
    """the resident state as a snapshot: the covariance, pose tables and landmarks of the device; ids, first estimates of the clones and the batch of `like`"""
    st, lm = up.get_state(P=True), up.get_landmarks()
    q = copy.copy(like)
    q.P, q.clone_q_p, q.calib_q_p, q.intrinsics = st["P"], st["clone_q_p"], st["calib_q_p"], st["intrinsics"]
    q.lm_value, q.lm_fej, q.lm_cov_id = lm["value"], lm["fej"], lm["cov_id"]
    anchored = lm["feat_rep"] >= wo.A3  # (the anchors of the global ones are not read)
    q.lm_anchor_cam, q.lm_anchor_clone = np.where(anchored, lm["anchor_cam"], -1).astype(np.int32), np.where(anchored, lm["anchor_clone"], -1).astype(np.int32)
    q.lm_rep_each = lm["feat_rep"]
    return q


def check_anchors(lm, P, ref, what, symmetric):
    """tests/test_gpu_anchor_batch.py::check_against; the chain of single calls leaves each landmark's Phi P Phi^T as computed (the reference's
    EKFPropagation does), the batched entry a covariance that is symmetric bit for bit"""
    if symmetric:
        return aab.check_against(lm, P, ref, what)
    np.testing.assert_allclose(lm["value"], ref.lm_value, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(lm["fej"], ref.lm_fej, rtol=1e-12, atol=1e-13)
    anchored = ref.lm_anchor_clone >= 0
    np.testing.assert_array_equal(lm["anchor_clone"][anchored], ref.lm_anchor_clone[anchored])
    np.testing.assert_array_equal(lm["anchor_cam"][anchored], ref.lm_anchor_cam[anchored])
    assert _rel(P, ref.P) < 1e-12


@pytest.mark.parametrize("entry", ["batched", "single"])
@pytest.mark.parametrize("order", ["steady", "front"])
def test_anchor_change_then_marginalize_then_update(Updater, oracle, order, entry):
    """The landmarks anchored in the oldest clone move to the newest: Phi over (old clone, extrinsics, new clone, landmark) — ids that are not
    ascending by kind once landmarks lie in front of clones.  Then the oldest clone and one landmark of the middle group leave in one pass, and
    the SLAM update on the shifted window matches the oracle."""
    q, _, tokens, _ = wo.anchor_state(order)
    moved = wo.moving(q, 0)
    assert len(moved) >= 3
    opts = capi.default_options(chi2_multipler=1.0)
    up = Updater(opts)
    up.set_slam_problem(q)
    if entry == "batched":
        assert up.change_anchors_batched(0, q.C - 1) == len(moved)
    else:
        for l in moved:
            up.change_anchor(int(l), int(q.lm_anchor_cam[l]), q.C - 1)
    ref = aab.oracle_chain(oracle, opts, q, moved)
    P1, lm1 = up.get_state(P=True)["P"], up.get_landmarks()
    check_anchors(lm1, P1, ref, f"{entry} on {order}, {len(moved)} moved", symmetric=entry == "batched")
    note(f"ovgpu_slam_change_anchor{'s_batched' if entry == 'batched' else ''}", f"{order}", P=_rel(P1, ref.P), values=np.abs(lm1["value"] - ref.lm_value).max())
    assert np.array_equal(lm1["cov_id"], q.lm_cov_id)
    # ---- the oldest clone and a landmark from the middle of the covariance leave together
    cur = read_back(up, q)
    gone = wo.middle_landmark(tokens)
    exp, rows = wo.drop_blocks(cur, clones=[0], landmarks=[gone])
    up.state_marginalize_many([int(cur.lm_cov_id[gone]), int(cur.clone_cov_id[0])], [int(wo.lm_dof(cur)[gone]), 6])
    got = read_back(up, exp)
    assert up.N == exp.N and up.Cn == exp.C
    assert np.array_equal(got.P, exp.P)  # np.delete on the covariance read back: a selection, bit for bit
    for k in ("clone_q_p", "lm_value", "lm_fej", "lm_cov_id", "lm_anchor_cam", "lm_anchor_clone", "lm_rep_each"):
        assert np.array_equal(getattr(got, k), getattr(exp, k)), k
    # ---- the SLAM update on the shifted window (tests/test_gpu_parity.py::test_change_anchors_parity_then_marginalize: dx 1e-7, P' 1e-8)
    ref_u = oracle.slam_update(opts, capi.Views(got))
    assert wo.near_gate(ref_u) == 0 and (ref_u["feat_status"] == capi.FEAT_USED).sum() >= 3
    up.set_features(got)
    out = up.slam_update(got.lm_index)
    out.update(up.get_state(P=False))
    up.close()
    hold_slam("ovgpu_slam_update behind the marginalisation", oracle, opts, got, out, ref_u, f"{entry} on {order}: update on the shifted window", symmetric=entry == "batched")


# --------------------------------------------------------------------------- "gram_wide" = 1
def test_gram_wide_on_steady(Updater, oracle):
    """gram_wide_shapes' "b-385" (56 clones, stereo, nine landmarks: 385 columns, the first count with a seventh block of 64) in the `steady` order"""
    p, perm, opts, ref, app = wo.wide_case(oracle)
    up = context(Updater, opts, gram_wide=1)
    out = slam_update(up, p)
    route, wide = up.lib.ovgpu_last_update_route(up._ctx), up.debug_option("gram_wide_updates")
    up.close()
    assert out["stats"]["D"] == 385 and route == capi.COMPRESS_GRAM and wide == 1
    hold_slam('"gram_wide" = 1', oracle, opts, p, out, ref, "b-385 on steady", tol_dx=TOL_DX, tol_p=TOL_P)  # tests/test_gpu_gram_wide.py::hold
    assert np.array_equal(out["landmarks"], wo.corrected(p, out["dx"]))


# --------------------------------------------------------------------------- one life cycle through the real calls
class Device:
    """what window_order.Life drives next to the oracle: one long-lived context"""

    def __init__(self, Updater, opts):
        self.up = Updater(opts)

    def start(self, p):  # an MSCKF-only ovgpu_set_state
        up = self.up
        up._views = capi.Views(p)
        capi.check(up.lib.ovgpu_set_state(up._ctx, ctypes.byref(up._views.state)), "ovgpu_set_state")
        up.N, up.Cn, up.K, up.F = p.N, p.C, p.K, 0

    def read_back(self, exp):
        up = self.up
        up._refresh_dims()
        st = up.get_state(P=True)
        q = copy.copy(exp)
        q.N, q.C = up.N, up.Cn
        q.P, q.clone_q_p, q.calib_q_p, q.intrinsics = st["P"], st["clone_q_p"], st["calib_q_p"], st["intrinsics"]
        if exp.lm_value is not None:
            lm = up.get_landmarks()
            anchored = lm["feat_rep"] >= wo.A3
            q.lm_value, q.lm_fej, q.lm_cov_id, q.lm_rep_each = lm["value"], lm["fej"], lm["cov_id"], lm["feat_rep"]
            q.lm_anchor_cam = np.where(anchored, lm["anchor_cam"], -1).astype(np.int32)
            q.lm_anchor_clone = np.where(anchored, lm["anchor_clone"], -1).astype(np.int32)
        return q

    def reset_returns_the_state_left(self, what):
        """after a structural call ovgpu_reset_state goes back to exactly the state that call left"""
        up = self.up
        up._refresh_dims()
        before = up.get_state(P=True)
        up.reset_state()
        after = up.get_state(P=True)
        for k in before:
            assert np.array_equal(before[k], after[k]), (what, k)

    def delayed_init(self, batch, tri, reps, entry, L):
        up = self.up
        if L:
            up.set_active_landmarks([])
        up.set_features(batch)
        up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
        out = up.delayed_init(0, feat_rep_each=reps, fused=entry == "fused")
        self.reset_returns_the_state_left("ovgpu_slam_delayed_init")
        return out

    def augment_clone(self, q, qf, dnc):
        nid = self.up.state_augment_clone(0, q, qf, dt_cov_id=15, dnc_dt=dnc)
        self.reset_returns_the_state_left("ovgpu_state_augment_clone")
        return nid

    def propagate(self, new_id, old_ids, Phi, Q):
        self.up.state_propagate(new_id, old_ids, Phi, Q)

    def slam_update(self, batch, tracked):
        up = self.up
        up.set_active_landmarks(tracked)
        up.set_features(batch)
        return up.slam_update(batch.lm_index)

    def change_anchor(self, l, cam, clone):
        self.up.change_anchor(l, cam, clone)

    def change_anchors_batched(self, marg, new):
        return self.up.change_anchors_batched(marg, new)

    def marginalize(self, ids, sizes):
        self.up.state_marginalize_many(ids, sizes)
        self.reset_returns_the_state_left("ovgpu_state_marginalize_batched")


def test_life_cycle_through_the_real_calls(Updater, oracle):
    """Three turns of the window from an MSCKF-only ovgpu_set_state (window_order.Life): every step against the oracle step applied to the state
    read back before it.  Then a fresh context is handed the read-back state through ovgpu_set_state + ovgpu_set_landmarks: on the same batch it
    must return the long-lived context's BITS — which holds every host mirror (the clones', landmarks' and calibration's covariance ids, the
    anchors, the active set that followed the landmarks' indices) to the device without any tolerance."""
    life = wo.Life(oracle, Device(Updater, capi.default_options(**wo.LIFE_OPTS))).run()
    for turn, step, dev in life.log:
        note(f"life cycle: {step.split(' (')[0]}", f"turn {turn} {step}", **dev)
    cur, up = life.cur, life.dev.up
    assert cur.lm_cov_id.min() < cur.clone_cov_id.max() and cur.lm_cov_id.max() > cur.clone_cov_id.min()
    batch = life.final_batch()
    L = life.L

    def run(u):
        u.set_features(batch)
        out = u.slam_update(batch.lm_index)
        out.update(u.get_state(P=False))
        out["lm"] = u.get_landmarks()
        return out

    a = run(up)
    up.close()
    fresh = Updater(life.opts)
    fresh.set_slam_state(cur)
    fresh.set_active_landmarks(np.arange(L))
    b = run(fresh)
    fresh.close()
    assert a["stats"]["n_used"] >= 3 and a["stats"]["n_used"] == b["stats"]["n_used"] and a["stats"]["D"] == b["stats"]["D"] == wo.col_cov_ids(cur).size
    for k in ("feat_status", "chi2", "chi2_thresh", "dx", "P", "landmarks") + STATE_KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    for k in ("value", "fej", "cov_id", "feat_rep"):
        assert np.array_equal(a["lm"][k], b["lm"][k]), k
    ref = oracle.slam_update(life.opts, capi.Views(batch))
    hold_slam("life cycle: the update behind the last turn", oracle, life.opts, batch, a, ref, "long-lived context against the oracle", symmetric=False)


def test_zz_worst_deviations():
    """prints what this file measured against the oracle, per entry, and the kernel every fused case reported (DESIGN.md quotes the figures)"""
    for entry, w in sorted(WORST.items()):
        print(f"{entry}: worst " + "  ".join(f"{k} {v:.2e}" for k, v in w.items()))
    print("kernels reported: " + "  ".join(f"{k} {v}" for k, v in sorted(KERNELS.items())))
