"""The shapes at which the window kernels of csrc/k_slam.h (k_cov_propagate, k_cov_clone, k_cov_dt, k_cov_gather, k_cov_remove, k_cov_copy) and
their entries are held to the oracle, ON A STATE THAT HAS LANDMARKS between its clones (window_order's `steady` order): tests/test_window_order_cpu.py
shows every case has the property it is named for, tests/test_gpu_window_edges.py runs it on the device.

Before this table the kernels met the oracle at one shape: a 15 x 15 Phi over the contiguous ids 0 .. 14 of a landmark-free state.  Other callers
pass other shapes — the anchor change a 3 x 27 Phi over scattered ids, the propagation with IMU intrinsics n_old > n_new.

A helper module, not a conftest: nothing here is collected.
"""
from __future__ import annotations

import copy
import functools
import zlib
from dataclasses import dataclass

import numpy as np

import slam_shapes as ss
import window_order as wo

G3, GI, A3, AI, AM = ss.REPS5
SINGLE = wo.SINGLE


@functools.lru_cache(maxsize=None)
def state(C=10, reps=tuple(wo.MIX9), seed=5):
    """C clones x two cameras and the landmarks `reps` in the `steady` order: N = 44 + 6 C + the landmarks' dof"""
    b = ss.slam(len(reps), list(reps), seed, C=C, K=2)
    return wo.reorder(b, wo.order_steady(b))[0]


def state_of_dimension(N):
    """a `steady` state whose covariance has exactly N rows (the grid edges of the kernels are stated in N)"""
    return state(*DIMENSIONS[N])


# N = 44 + 6 C + 3 a + b: a 3-dof landmarks, b single-depth ones
DIMENSIONS = {
    127: (10, tuple(wo.MIX9)),                    # the file's default state
    128: (10, (G3, A3, AM, GI, AI, G3, A3, AM)),  # N n_new = 512 at n_new = 4
    171: (18, (G3, A3, AM, GI, AI, G3, SINGLE)),  # N n_new = 513 at n_new = 3
    220: (28, (G3, SINGLE, A3, SINGLE)),          # N + 36 = 256: k_cov_clone's corner ends with the first workgroup
    221: (28, (G3, A3, AM)),                      # N + 36 = 257: one corner entry falls into a second workgroup
}


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


# --------------------------------------------------------------------------- ovgpu_state_propagate
@dataclass
class Propagate:
    id: str
    N: int
    new_id: int
    old_ids: np.ndarray
    Phi: np.ndarray
    Q: np.ndarray  # as handed over: only its upper triangle may be read

    @property
    def n_new(self):
        return self.Phi.shape[0]

    @property
    def prob(self):
        return state_of_dimension(self.N)


def numpy_propagate(P, new_id, old_ids, Phi, Q):
    """StateHelper::EKFPropagation in plain numpy: P(new, :) = Phi P(old, :), P(new, new) = Phi P(old, old) Phi^T + Q.selfadjointView<Upper>()"""
    n = Phi.shape[0]
    W = P[:, old_ids] @ Phi.T
    Qs = np.triu(Q) + np.triu(Q, 1).T
    out = P.copy()
    out[new_id:new_id + n, :], out[:, new_id:new_id + n] = W.T, W
    out[new_id:new_id + n, new_id:new_id + n] = Phi @ W[old_ids, :] + Qs
    return out


def _prop(name, N, new_id, old_ids, n_new, identity=True, garbage=False):
    rng = rng_of(name)
    old_ids = np.asarray(old_ids, dtype=np.int32)
    Phi = 0.05 * rng.normal(size=(n_new, old_ids.size))
    if identity:  # the block's own columns carry the identity: a transition, not a projection
        for a in range(n_new):
            Phi[a, np.flatnonzero(old_ids == new_id + a)] += 1.0
    Q = np.diag(rng.uniform(1e-8, 1e-6, n_new))
    if n_new > 1:
        Q[0, n_new - 1] = 1e-9
    if garbage:
        Q[np.tril_indices(n_new, -1)] = 1e30 * rng.normal(size=n_new * (n_new - 1) // 2)
    return Propagate(name, N, int(new_id), old_ids, np.ascontiguousarray(Phi), np.ascontiguousarray(Q))


def _propagate_cases():
    p = state_of_dimension(127)
    cl, lm, dof = p.clone_cov_id, p.lm_cov_id, wo.lm_dof(p)
    three = [l for l in range(len(lm)) if dof[l] == 3]
    mid = next(l for l in three if cl[0] < lm[l] < cl[-1])           # a 3-dof landmark between two clones
    last = int(np.argmax(lm))                                         # the variable at the last rows of P
    r = lambda i, n: list(range(int(i), int(i) + n))
    out = [
        _prop("n_new-1", 127, 15, [15], 1),                                                                   # the time offset alone
        # the anchor change's widest shape: 3 x 27 over the old clone, the old camera's extrinsics, the new clone, the new camera's extrinsics and the
        # landmark — five runs of ids that are not ascending
        _prop("n_new-3-scattered", 127, lm[mid], r(cl[0], 6) + r(p.calib_cov_id[1], 6) + r(cl[-1], 6) + r(p.calib_cov_id[0], 6) + r(lm[mid], 3), 3),
        _prop("n_new-6", 127, cl[3], r(cl[3], 6), 6),                                                         # one clone on itself
        _prop("n_new-15", 127, 0, r(0, 15), 15),                                                              # the IMU block, dense
        _prop("n_old-more-two-runs", 127, 0, r(0, 15) + r(30, 9), 15),                                        # n_old = 24 > n_new = 15: ids 0 .. 14 and 30 .. 38
        _prop("old-ids-descending", 127, 0, r(0, 15)[::-1], 15),
        _prop("old-ids-outside", 127, lm[mid], r(cl[5], 6), 3, identity=False),                               # nothing of the block's own rows is read
        _prop("ends-at-the-last-row", 127, lm[last], r(cl[2], 6) + r(lm[last], int(dof[last])), int(dof[last])),
        _prop("grid-512", 128, 22, r(22, 4) + r(50, 6), 4),                                                   # N n_new = 2 x 256
        _prop("grid-513", 171, 16, r(16, 3) + r(60, 6), 3),                                                   # N n_new = 2 x 256 + 1
        _prop("Q-lower-garbage", 127, 0, r(0, 15), 15, garbage=True),
    ]
    assert dof[last] == 3 and lm[last] + 3 == 127
    return out


PROPAGATE = _propagate_cases()
PROPAGATE_BY_ID = {c.id: c for c in PROPAGATE}


def negative_outside():
    """the default state with one NEGATIVE diagonal entry outside the propagated block (a landmark's row), and the IMU block's case: the reference
    and the oracle scan the whole diagonal (StateHelper.cpp:101-113)"""
    p = copy.copy(state_of_dimension(127))
    P = p.P.copy()
    j = int(p.lm_cov_id[0])
    P[j, j] = -1e-6
    p.P = np.ascontiguousarray(P)
    return p, PROPAGATE_BY_ID["n_new-15"], j


# --------------------------------------------------------------------------- ovgpu_state_augment_clone
@dataclass
class Augment:
    id: str
    N: int
    src: str            # "imu": the IMU pose at id 0, or "clone": a window clone's pose
    dt: bool            # with the time-offset Jacobian (dt_cov_id = 15)
    times: int = 1      # clones in a row

    @property
    def prob(self):
        return state_of_dimension(self.N)

    def src_id(self, p):
        return 0 if self.src == "imu" else int(p.clone_cov_id[4])


AUGMENT = [
    Augment("no-dt", 127, "imu", False),
    Augment("dt", 127, "imu", True),
    Augment("source-is-a-window-clone", 127, "clone", True),
    Augment("five-in-a-row", 127, "imu", True, times=5),   # ten clones of seven doubles grow to fifteen: the record buffers regrow
    Augment("grid-256", 220, "imu", True),
    Augment("grid-257", 221, "clone", True),
]
AUGMENT_BY_ID = {c.id: c for c in AUGMENT}


# --------------------------------------------------------------------------- ovgpu_state_marginal_covariance
def marginal_indices(name, N):
    rng = rng_of("marginal-" + name)
    return {
        "n-1": np.array([N - 1]),
        "n-16": rng.permutation(N)[:16],
        "n-17": rng.permutation(N)[:17],
        "n-1024": rng.integers(0, N, 1024),            # the bound: every row many times over
        "repeated": np.array([5, 5, 90, 5, 126, 90]),
        "permuted": rng.permutation(N),
    }[name].astype(np.int32)


MARGINAL = ["n-1", "n-16", "n-17", "n-1024", "repeated", "permuted"]


# --------------------------------------------------------------------------- ovgpu_state_marginalize
def marginalize_block(name, p):
    """(covariance id, size) of the block the case removes from the default state"""
    lm, dof = p.lm_cov_id, wo.lm_dof(p)
    last = int(np.argmax(lm))
    mid = wo.middle_landmark(wo.order_steady(p))
    return {
        "time-offset": (15, 1),
        "extrinsics": (int(p.calib_cov_id[1]), 6),
        "intrinsics": (int(p.intr_cov_id[0]), 8),
        "last-rows": (int(lm[last]), int(dof[last])),
        "middle-landmark": (int(lm[mid]), int(dof[mid])),
    }[name]


MARGINALIZE = ["time-offset", "extrinsics", "intrinsics", "last-rows", "middle-landmark"]


def after_block(p, cov_id, size):
    """the snapshot after ovgpu_state_marginalize of [cov_id, cov_id + size): a landmark or clone that starts there leaves (window_order.drop_blocks),
    a calibration variable stops being estimated (its id becomes -1), anything else only shifts the ids behind it"""
    lm_hit = [l for l in range(len(p.lm_cov_id)) if p.lm_cov_id[l] == cov_id]
    cl_hit = [c for c in range(p.C) if p.clone_cov_id[c] == cov_id]
    if lm_hit or cl_hit:
        return wo.drop_blocks(p, clones=cl_hit, landmarks=lm_hit)[0]
    rows = np.arange(cov_id, cov_id + size)
    q = copy.copy(p)
    q.P = np.ascontiguousarray(np.delete(np.delete(p.P, rows, axis=0), rows, axis=1))
    q.N = p.N - size
    shift = lambda i: -1 if (i < 0 or i == cov_id) else (int(i) - size if i > cov_id else int(i))
    for k in ("clone_cov_id", "calib_cov_id", "intr_cov_id", "lm_cov_id"):
        setattr(q, k, np.asarray([shift(int(i)) for i in getattr(p, k)], dtype=np.int32))
    return q
