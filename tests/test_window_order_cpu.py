"""CPU tests of tests/window_order.py: what lets tests/test_gpu_window_order.py compare accept sets exactly and trust its reordered states.

For every case the GPU test runs: the oracle on the reordered state equals the permuted oracle result of the appended one (identical accept sets;
dx, P', chi2 and landmarks within window_order.FLOOR = 1e-12 relative — measured 6e-14), a feature is used, the planted outlier is rejected, no
statistic lies within parity_util.GATE_MARGIN of its threshold, and the order has the property it is named for.
"""
import numpy as np
import pytest

import window_order as wo
from open_vins_amd import capi


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


# --------------------------------------------------------------------------- reorder() itself
def test_reorder_moves_the_covariance_and_nothing_else():
    b = wo.small_batch(wo.MIX9, 5)
    q, perm = wo.reorder(b, wo.order_steady(b))
    blk_b, blk_q = wo.blocks(b), wo.blocks(q)
    for t, (i, size) in blk_b.items():
        j = blk_q[t][0]
        assert blk_q[t][1] == size
        for u, (i2, size2) in blk_b.items():
            j2 = blk_q[u][0]
            assert np.array_equal(q.P[j:j + size, j2:j2 + size2], b.P[i:i + size, i2:i2 + size2])
    front = int(b.clone_cov_id[0])
    assert np.array_equal(perm[:front], np.arange(front)) and np.array_equal(q.P[:front, :front], b.P[:front, :front])
    assert np.array_equal(q.calib_cov_id, b.calib_cov_id) and np.array_equal(q.intr_cov_id, b.intr_cov_id)
    for k in ("clone_q_p", "clone_q_p_fej", "lm_value", "lm_fej", "lm_index", "lm_anchor_clone", "lm_anchor_cam", "uv", "clone_idx", "meas_offsets"):
        assert np.array_equal(getattr(q, k), getattr(b, k)), k
    q.P[0, 0] = -1.0  # a deep copy
    assert b.P[0, 0] > 0
    same, perm0 = wo.reorder(b, wo.order_appended(b))
    assert np.array_equal(perm0, np.arange(b.N)) and np.array_equal(same.P, b.P) and np.array_equal(same.lm_cov_id, b.lm_cov_id)


def test_an_id_of_minus_one_stays():
    b = wo.small_batch(wo.MIX9, 5)
    b.intr_cov_id = np.array([-1, int(b.intr_cov_id[1])], dtype=np.int32)
    q, _ = wo.reorder(b, wo.order_front(b))
    assert q.intr_cov_id[0] == -1 and q.intr_cov_id[1] == b.intr_cov_id[1]
    assert [c[0] for c in wo.columns(q)].count("k") == 1


def test_columns_follow_the_covariance_ids():
    b = wo.small_batch(wo.MIX9, 5)
    cols = wo.columns(b)
    assert [c[0] for c in cols] == ["x", "k"] * 2 + ["c"] * 10 + ["l"] * 9  # the appended order: calibration, clones, landmarks
    assert cols[-1][4] + cols[-1][3] == 6 * 10 + 28 + 7 * 3 + 2
    assert np.array_equal(wo.col_cov_ids(b), np.arange(16, b.N))
    q, _ = wo.reorder(b, wo.order_steady(b))
    ids = wo.col_cov_ids(q, active=[0, 4])
    assert np.all(np.diff(ids) > 0) and ids.size == 28 + 60 + 6
    assert [c[0] for c in wo.columns(q, pose=0, intr=0)][:4] == ["c", "c", "c", "l"] and wo.columns(q, pose=0, intr=0)[0][4] == 0


# --------------------------------------------------------------------------- the orders have the properties they are named for
@pytest.mark.parametrize("cid", [c.id for c in wo.CASES])
def test_order_has_its_property(cid):
    case = wo.BY_ID[cid]
    p, b = case.prob, case.base
    cl, lm = p.clone_cov_id, p.lm_cov_id
    assert np.all(np.diff(cl) > 0), "clones run oldest to newest"
    front = int(b.clone_cov_id[0])
    assert np.array_equal(p.calib_cov_id, b.calib_cov_id) and max(p.calib_cov_id.max(), p.intr_cov_id.max()) < front
    ids = wo.col_cov_ids(p)
    assert np.all(np.diff(ids) > 0) and ids.size == p.N - 16
    if case.order in ("steady", "straddle"):
        assert wo.interleaved(p, case.tokens)
        assert not wo.interleaved(b, wo.order_appended(b))
    if case.order == "front":
        assert lm.max() < cl.min() and lm.min() == front
    if case.order == "straddle":
        assert wo.crossings(p) == (True, True)
        # (the appended order of the same state has no landmark in front of a clone at all)
        assert wo.crossings(b)[1] is False


# --------------------------------------------------------------------------- the oracle is equivariant, the batches decide away from the gate
WORST = {}


@pytest.mark.parametrize("cid", [c.id for c in wo.CASES])
def test_oracle_on_the_reordered_state_is_the_permuted_oracle(oracle, cid):
    case = wo.BY_ID[cid]
    ref, app = wo.oracle_pair(oracle, case)
    assert ref["near_gate"] == 0 and app["near_gate"] == 0
    assert np.array_equal(ref["feat_status"], app["feat_status"])
    assert (ref["feat_status"] == capi.FEAT_USED).sum() >= 1
    assert ref["feat_status"][case.rejected] == capi.FEAT_CHI2_REJECTED
    gate = np.isfinite(ref["chi2"])
    assert np.array_equal(gate, np.isfinite(app["chi2"]))
    dev = dict(chi2=np.abs(ref["chi2"][gate] / app["chi2"][gate] - 1.0).max(), dx=_rel(ref["dx"], app["dx"]), P=_rel(ref["P"], app["P"]),
               landmarks=_rel(ref["landmarks"], app["landmarks"]))
    print(f"{cid}: the oracle against its permuted self: " + "  ".join(f"{k} {v:.2e}" for k, v in dev.items()))
    for k, v in dev.items():
        WORST[k] = max(WORST.get(k, 0.0), float(v))
        assert v < wo.FLOOR, (k, v)
    assert np.array_equal(ref["chi2_thresh"][gate], app["chi2_thresh"][gate])
    assert np.array_equal(ref["col_cov_id"], wo.col_cov_ids(case.prob))  # the oracle's own column order is the documented one
    assert np.abs(ref["dx"][case.prob.lm_cov_id]).min() > 0  # every landmark moves: a correction read from the wrong row would show


# --------------------------------------------------------------------------- the batches of the other entries
def test_chunks_come_from_different_groups_and_decide_away_from_the_gate(oracle):
    import test_gpu_slam_chunked as sc
    q, first = wo.chunk_batch()
    ref = sc.oracle_chain(oracle, capi.default_options(chi2_multipler=1.0), q, first)
    assert ref["near_gate"] == 0 and all(n >= 1 for n in ref["n_used"]) and len(first) == 3
    a, b = np.unique(q.lm_index[first[0]:first[1]]), np.unique(q.lm_index[first[1]:first[2]])
    assert not set(a) & set(b) and q.lm_cov_id[a].max() < q.clone_cov_id.max() < q.lm_cov_id[b].min()


def test_msckf_batch_on_the_interleaved_state(oracle):
    p, _, tokens, _ = wo.steady_mixed()
    msckf, plain = wo.msckf_on(p)
    opts = capi.default_options(chi2_multipler=1.0)
    ref = oracle.msckf_update(opts, capi.Views(plain))
    assert (ref["feat_status"] == capi.FEAT_USED).sum() >= 10 and wo.near_gate(ref) == 0
    assert np.abs(ref["dx"][p.lm_cov_id]).min() > 0  # every landmark, wherever it lies, gets a correction through its cross-covariance
    # the landmark-free twin on the APPENDED covariance gives the permuted result: the oracle's MSCKF update is equivariant as well
    base = wo.BY_ID["general-steady"]
    _, plain0 = wo.msckf_on(base.base)
    ref0 = wo.permuted(oracle.msckf_update(opts, capi.Views(plain0)), base.perm)
    assert np.array_equal(ref["feat_status"], ref0["feat_status"])
    assert _rel(ref["dx"], ref0["dx"]) < wo.FLOOR and _rel(ref["P"], ref0["P"]) < wo.FLOOR
    # the column map of the empty set has gaps in its covariance ids where the landmarks lie
    ids = wo.col_cov_ids(p, active=[])
    assert ids.size == 28 + 6 * p.C and (np.diff(ids) > 1).sum() >= 2


def test_two_landmarks_from_different_groups(oracle):
    p, _, tokens, _ = wo.steady_mixed()
    gr = wo.groups(tokens)
    two = [int(gr[0][1][0]), int(gr[-1][1][0])]
    q = wo.only_features(p, [int(np.flatnonzero(p.lm_index == l)[0]) for l in two])
    ref = oracle.slam_update(capi.default_options(chi2_multipler=1.0), capi.Views(q))
    assert (ref["feat_status"] == capi.FEAT_USED).all() and wo.near_gate(ref) == 0
    assert np.abs(ref["landmarks"] - q.lm_value).max(axis=1).min() > 0  # the seven without columns move too
    assert p.lm_cov_id[two[0]] < p.clone_cov_id.max() < p.lm_cov_id[two[1]]


def test_delayed_init_batch(oracle):
    state, batch, reps, opts = wo.init_batch()
    v = capi.Views(batch)
    tri = oracle.triangulate(opts, v)
    ref = oracle.slam_delayed_init(opts, v, feat_rep=0, tri=tri, feat_rep_each=reps)
    acc = ref["lm_cov_id"] >= 0
    gate = np.isfinite(ref["chi2"]) & (ref["chi2_thresh"] > 0)
    assert ref["rc"] == 0 and acc.sum() >= 3
    assert (np.abs(ref["chi2"][gate] / ref["chi2_thresh"][gate] - 1.0) > 1e-6).all()  # tests/test_gpu_delayed_init_fused.py's margin
    assert (reps[acc] == wo.SINGLE).any() and (reps[acc] != wo.SINGLE).any()
    assert ref["lm_cov_id"][acc].min() == state.N > state.clone_cov_id.max()
    post, lm = wo.init_as_read_back(state, ref, reps, acc)
    nxt = wo.after_init(state, batch, post, lm, acc)
    assert nxt.F == state.F + acc.sum() and nxt.M == state.M + int(np.diff(batch.meas_offsets)[acc].sum())
    ref2 = oracle.slam_update(opts, capi.Views(nxt))
    assert wo.near_gate(ref2) == 0 and (ref2["feat_status"] == capi.FEAT_USED).sum() >= 3
    assert (ref2["feat_status"][state.F:] == capi.FEAT_USED).any() and (ref2["feat_status"][:state.F] == capi.FEAT_USED).any()


@pytest.mark.parametrize("order", ["steady", "front"])
def test_anchor_change_batch(oracle, order):
    import test_gpu_anchor_batch as aab
    q, perm, tokens, b = wo.anchor_state(order)
    moved = wo.moving(q, 0)
    assert len(moved) >= 3 and (wo.lm_reps(q)[moved] == wo.SINGLE).any() and (wo.lm_reps(q)[moved] != wo.SINGLE).any()
    opts = capi.default_options(chi2_multipler=1.0)
    ref = aab.oracle_chain(oracle, opts, q, moved)
    ref0 = aab.oracle_chain(oracle, opts, b, moved)  # the appended state: the permuted result
    assert _rel(ref.P, ref0.P[np.ix_(perm, perm)]) < wo.FLOOR and np.abs(ref.lm_value - ref0.lm_value).max() < 1e-12
    # the ids of one landmark's Phi columns — old clone, extrinsics, new clone, landmark — are not ascending by kind
    l = int(moved[0])
    ids = [int(q.clone_cov_id[0]), int(q.calib_cov_id[q.lm_anchor_cam[l]]), int(q.clone_cov_id[-1]), int(q.lm_cov_id[l])]
    assert any(q.lm_cov_id[m] < q.clone_cov_id[-1] for m in moved), ids
    gone = wo.middle_landmark(tokens)
    assert q.lm_cov_id.min() < q.lm_cov_id[gone] < q.lm_cov_id.max()
    win, rows = wo.drop_blocks(ref, clones=[0], landmarks=[gone])
    assert rows.size == 6 + wo.lm_dof(q)[gone] and win.N == q.N - rows.size and win.C == q.C - 1
    assert np.array_equal(win.P, ref.P[np.ix_(np.setdiff1d(np.arange(q.N), rows), np.setdiff1d(np.arange(q.N), rows))])
    ref_u = oracle.slam_update(opts, capi.Views(win))
    assert wo.near_gate(ref_u) == 0 and (ref_u["feat_status"] == capi.FEAT_USED).sum() >= 3


def test_wide_case(oracle):
    p, perm, opts, ref, app = wo.wide_case(oracle)
    assert sum(c[3] for c in wo.columns(p)) == 385 and wo.interleaved(p, wo.order_steady(p))
    assert wo.near_gate(ref) == 0 and np.array_equal(ref["feat_status"], app["feat_status"]) and (ref["feat_status"] == capi.FEAT_USED).any()
    assert (ref["feat_status"] == capi.FEAT_CHI2_REJECTED).sum() >= 1
    assert _rel(ref["dx"], app["dx"]) < wo.FLOOR and _rel(ref["P"], app["P"]) < wo.FLOOR


def test_drop_blocks_is_a_selection():
    p = wo.steady_mixed()[0]
    q, rows = wo.drop_blocks(p, clones=[2, 4], landmarks=[3])
    keep = np.setdiff1d(np.arange(p.N), rows)
    assert np.array_equal(q.P, p.P[np.ix_(keep, keep)]) and q.N == p.N - 15 and q.C == p.C - 2
    new_of = {int(o): n for n, o in enumerate(keep)}
    kept_clones = [c for c in range(p.C) if c not in (2, 4)]
    assert [new_of[int(p.clone_cov_id[c])] for c in kept_clones] == q.clone_cov_id.tolist()
    assert [new_of[int(p.lm_cov_id[l])] for l in range(9) if l != 3] == q.lm_cov_id.tolist()
    assert q.F == p.F - 1 and q.clone_idx.max() == q.C - 1 and set(q.lm_index) == set(range(8))
    assert not np.isin(p.clone_idx[np.isin(p.clone_idx, (2, 4))], kept_clones).any()


# --------------------------------------------------------------------------- the life cycle, on the oracle alone
def test_life_cycle_on_the_oracle(oracle):
    life = wo.Life(oracle).run()
    steps = {}
    for turn, step, facts in life.log:
        steps.setdefault(step.split(" (")[0], []).append(facts)
    assert [len(v) for v in steps.values()] == [3] * 7, steps.keys()
    assert all(3 <= f["accepted"] <= 4 and f["near_gate"] == 0 for f in steps["delayed_init"])
    assert all(f["landmarks_in_front"] >= 3 for f in steps["augment_clone"])  # the clone lands behind resident landmarks, every turn
    assert all(f["used"] >= 2 and f["near_gate"] == 0 and f["interleaved"] for f in steps["slam_update"])
    assert all(f["moved"] >= 1 for f in steps["change_anchors_batched"])
    assert all(f["landmark_between_clones"] for f in steps["marginalize_batched"])
    cur = life.cur
    assert cur.C == wo.LIFE["C"] and len(cur.lm_cov_id) >= 6
    # after three turns: landmark blocks alternate with clone blocks
    kinds = "".join(k for k, *_ in wo.columns(cur) if k in "cl")
    assert kinds.count("cl") >= 3 and kinds.count("lc") >= 3, kinds
    ref = oracle.slam_update(life.opts, capi.Views(life.final_batch()))
    assert wo.near_gate(ref) == 0 and (ref["feat_status"] == capi.FEAT_USED).sum() >= 3


def test_zz_equivariance_floor():
    print("the oracle's equivariance floor over the cases: " + "  ".join(f"{k} {v:.2e}" for k, v in sorted(WORST.items())))
