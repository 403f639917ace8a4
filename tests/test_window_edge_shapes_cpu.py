"""CPU tests of tests/window_edge_shapes.py: every case tests/test_gpu_window_edges.py runs has the property it is named for, the oracle and the
plain numpy restatement agree on it, and the updates behind the structural cases decide away from their gates."""
import copy

import numpy as np
import pytest

import window_edge_shapes as we
import window_order as wo
from open_vins_amd import capi


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def test_states_have_their_dimension_and_landmarks_between_clones():
    for N in we.DIMENSIONS:
        p = we.state_of_dimension(N)
        assert p.N == N and p.P.shape == (N, N) and wo.interleaved(p, wo.order_steady(p))
        assert np.array_equal(p.P, p.P.T)  # symmetric bit for bit: a marginalisation is then a selection


@pytest.mark.parametrize("cid", [c.id for c in we.PROPAGATE])
def test_propagate_case(oracle, cid):
    c = we.PROPAGATE_BY_ID[cid]
    p = c.prob
    n, ids, blk = c.n_new, c.old_ids, set(range(c.new_id, c.new_id + c.n_new))
    assert c.Phi.shape == (n, ids.size) and c.Q.shape == (n, n) and 0 <= c.new_id and c.new_id + n <= p.N and ids.min() >= 0 and ids.max() < p.N
    rc, ref = oracle.propagate(p.P, c.new_id, ids, c.Phi, c.Q)
    assert rc == 0 and _rel(ref, we.numpy_propagate(p.P, c.new_id, ids, c.Phi, c.Q)) < 1e-14
    assert _rel(ref, p.P) > 1e-6  # the case does something
    runs = 1 + int((np.diff(ids) != 1).sum())
    named = {
        "n_new-1": n == 1, "n_new-3-scattered": n == 3 and ids.size == 27 and runs == 5 and not np.all(np.diff(ids) > 0),
        "n_new-6": n == 6, "n_new-15": n == 15 and ids.size == 15,
        "n_old-more-two-runs": ids.size > n and runs == 2, "old-ids-descending": np.all(np.diff(ids) == -1),
        "old-ids-outside": not (set(ids.tolist()) & blk), "ends-at-the-last-row": c.new_id + n == p.N,
        "grid-512": p.N * n == 512, "grid-513": p.N * n == 513,
        "Q-lower-garbage": n > 1 and np.abs(c.Q[np.tril_indices(n, -1)]).min(initial=np.inf) > 1e20,
    }
    assert named[cid], cid
    if cid == "Q-lower-garbage":  # ... and is ignored: the clean Q gives the same covariance
        assert np.array_equal(ref, oracle.propagate(p.P, c.new_id, ids, c.Phi, np.triu(c.Q))[1])


def test_negative_diagonal_outside_the_block(oracle):
    p, c, j = we.negative_outside()
    assert p.P[j, j] < 0 and j >= c.new_id + c.n_new
    rc, ref = oracle.propagate(p.P, c.new_id, c.old_ids, c.Phi, c.Q)
    assert rc == capi.ERR_NEGATIVE_DIAGONAL and (np.diag(ref)[:c.n_new] > 0).all() and (np.diag(ref) < 0).sum() == 1


@pytest.mark.parametrize("cid", [c.id for c in we.AUGMENT])
def test_augment_case(oracle, cid):
    c = we.AUGMENT_BY_ID[cid]
    p = c.prob
    src = c.src_id(p)
    assert (src == 0) == (c.src == "imu") and (c.src == "imu" or src in p.clone_cov_id.tolist())
    assert {"grid-256": p.N + 36 == 256, "grid-257": p.N + 36 == 257}.get(cid, True)
    assert (p.lm_cov_id < p.clone_cov_id.max()).any()  # landmarks resident in front of where the clone lands, and behind other clones
    dnc = we.rng_of(cid).normal(size=6)
    ref = oracle.augment_clone(p.P, src, 6, dt_id=15 if c.dt else -1, dnc_dt=dnc if c.dt else None)
    N = p.N
    want = np.zeros((N + 6, N + 6))
    want[:N, :N] = p.P
    want[:N, N:], want[N:, :N], want[N:, N:] = p.P[:, src:src + 6], p.P[src:src + 6, :], p.P[src:src + 6, src:src + 6]
    if c.dt:
        want[:, N:] += np.outer(want[:, 15], dnc)
        want[N:, :] += np.outer(dnc, want[15, :])
    assert _rel(ref, want) < 1e-15


def test_marginal_index_lists():
    N = 127
    sizes = {name: we.marginal_indices(name, N).size for name in we.MARGINAL}
    assert sizes == {"n-1": 1, "n-16": 16, "n-17": 17, "n-1024": 1024, "repeated": 6, "permuted": N}
    assert len(set(we.marginal_indices("repeated", N).tolist())) < 6 and sorted(we.marginal_indices("permuted", N).tolist()) == list(range(N))
    assert not np.all(np.diff(we.marginal_indices("permuted", N)) > 0)
    for name in we.MARGINAL:
        i = we.marginal_indices(name, N)
        assert i.min() >= 0 and i.max() < N


@pytest.mark.parametrize("name", we.MARGINALIZE)
def test_marginalize_case(oracle, name):
    p = we.state_of_dimension(127)
    cov_id, size = we.marginalize_block(name, p)
    msckf, plain = wo.msckf_on(p)
    exp = we.after_block(msckf, cov_id, size)
    assert np.array_equal(exp.P, oracle.marginalize(p.P, cov_id, size))  # np.delete and StateHelper::marginalize: the same selection, bit for bit
    named = {
        "time-offset": size == 1 and cov_id == 15, "extrinsics": size == 6 and (exp.calib_cov_id == -1).sum() == 1,
        "intrinsics": size == 8 and (exp.intr_cov_id == -1).sum() == 1, "last-rows": cov_id + size == p.N and len(exp.lm_cov_id) == 8,
        "middle-landmark": p.clone_cov_id.min() < cov_id < p.clone_cov_id.max() and len(exp.lm_cov_id) == 8,
    }
    assert named[name]
    assert exp.N == p.N - size and exp.F == msckf.F
    ids = [int(i) for i in np.concatenate([exp.clone_cov_id, exp.calib_cov_id, exp.intr_cov_id, exp.lm_cov_id]) if i >= 0]
    assert len(set(ids)) == len(ids) and max(ids) < exp.N
    twin = copy.copy(plain)
    twin.N, twin.P, twin.clone_cov_id, twin.calib_cov_id, twin.intr_cov_id = exp.N, exp.P, exp.clone_cov_id, exp.calib_cov_id, exp.intr_cov_id
    ref = oracle.msckf_update(capi.default_options(chi2_multipler=1.0), capi.Views(twin))
    assert (ref["feat_status"] == capi.FEAT_USED).sum() >= 10 and wo.near_gate(ref) == 0
    assert ref["D"] == 28 + 6 * p.C - (size if name in ("extrinsics", "intrinsics") else 0)


@pytest.mark.parametrize("cid", [c.id for c in we.AUGMENT])
def test_update_behind_the_augmented_window(oracle, cid):
    """the oracle's side of the update tests/test_gpu_window_edges.py::test_augment_clone runs behind its clones: enough features, none on its gate"""
    c = we.AUGMENT_BY_ID[cid]
    p = c.prob
    from open_vins_amd import synth
    rng = we.rng_of(cid)
    P, clones, fej, src = p.P, p.clone_q_p, p.clone_q_p_fej, c.src_id(p)
    for k in range(c.times):
        dnc = rng.normal(size=6) if c.dt else None
        q, qf = synth.boxplus_pose(clones[-1], 0.01 * rng.normal(size=6)), synth.boxplus_pose(fej[-1], 0.01 * rng.normal(size=6))
        P = oracle.augment_clone(P, src, 6, dt_id=15 if c.dt else -1, dnc_dt=dnc)
        clones, fej = np.vstack([clones, q[None]]), np.vstack([fej, qf[None]])
    _, plain = wo.msckf_on(p)
    plain.N, plain.C, plain.P, plain.clone_q_p, plain.clone_q_p_fej = P.shape[0], clones.shape[0], P, clones, fej
    plain.clone_cov_id = np.concatenate([p.clone_cov_id, p.N + 6 * np.arange(c.times)]).astype(np.int32)
    ref = oracle.msckf_update(capi.default_options(chi2_multipler=1.0), capi.Views(plain))
    assert (ref["feat_status"] == capi.FEAT_USED).sum() >= 10 and wo.near_gate(ref) == 0
