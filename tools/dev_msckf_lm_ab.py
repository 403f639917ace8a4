"""What ovgpu_msckf_update_lm is worth in the resident frame loop once the state carries SLAM landmarks: three legs of one frame's MSCKF update on one box.

    time [--reps 30] [--rounds 3] [--features 2000] [--lib-a PATH] [--tag NAME] [--out FILE.jsonl]
                    configs[2]: 2000 features, 30 clones, stereo, online camera / IMU calibration (N = 248), with L = 25 and L = 50 global landmarks
                    behind the clones (N = 248 + 3 L).  Per frame the state (and the landmarks, and the empty active set) are uploaded and the stream
                    drained, not timed; then, timed host to host, from handing the MSCKF batch over to the point where the posterior AND current
                    landmarks are resident:
                      A  ovgpu_set_features, ovgpu_msckf_update with the landmarks declared, the landmarks corrected on the host from the dx read
                         back, ovgpu_set_landmarks, ovgpu_synchronize — what a resident caller had to do before the entry existed; on the library
                         --lib-a names (the parent commit's build; default: the tree's, whose ovgpu_msckf_update is that code)
                      B  ovgpu_set_features, ovgpu_msckf_update_lm
                      C  ovgpu_set_features, ovgpu_msckf_update with the landmarks undeclared at the same N: the fast route's own time
                    The legs take turns frame by frame, `rounds` repetitions of `reps` frames; a row per (L, leg) with the median of every round, the
                    median of those and their spread (max - min): the yardstick for a difference between two legs.
    trace [--L 50] [--leg B] [--calls 10] [--features 2000]
                    the frames of one leg alone, for a rocprofv3 --kernel-trace --stats run of its own (which per-feature kernels run)"""
import argparse
import copy
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def problems(synth, L, F, seed=11):
    """(with landmarks, landmark-free twin): configs[2]'s state grown by L global landmarks whose rows of P are correlated with every other variable
    (P_big = [[P, P W], [W^T P, W^T P W + s^2 I]]: positive definite by its Schur complement), and the same N and P with the landmarks undeclared"""
    base = synth.make_problem(3, F=F, imu_intrinsics=True)
    pts = synth.make_problem(3, F=L, seed=seed).p_FinG_true
    rng = np.random.default_rng([seed, 9])
    N0, n = base.N, 3 * L
    W = rng.normal(0, 0.3 / np.sqrt(N0), (N0, n))
    PW = base.P @ W
    P = np.zeros((N0 + n, N0 + n))
    P[:N0, :N0], P[:N0, N0:], P[N0:, :N0] = base.P, PW, PW.T
    P[N0:, N0:] = W.T @ PW + 0.1 ** 2 * np.eye(n)
    plain = copy.copy(base)
    plain.N, plain.P = N0 + n, np.ascontiguousarray(0.5 * (P + P.T))
    lm = copy.copy(plain)
    lm.lm_value = np.ascontiguousarray(pts + rng.normal(0, 0.05, (L, 3)))
    lm.lm_fej = np.ascontiguousarray(lm.lm_value + rng.normal(0, 0.01, (L, 3)))
    lm.lm_cov_id = (N0 + 3 * np.arange(L)).astype(np.int32)
    lm.lm_index = np.zeros(0, np.int32)
    lm.lm_rep = 0
    return lm, plain


def bind(capi, path):
    """a library by path with the handful of entries the legs call (the parent commit's build does not export ovgpu_msckf_update_lm: capi.declare would refuse it)"""
    if path is None:
        return capi.load()
    lib = C.CDLL(os.path.abspath(path))
    ip, dp, ctx, st = capi.c_int32_p, capi.c_double_p, C.c_void_p, C.POINTER(capi.UpdateStats)
    sig = {"ovgpu_create": [C.POINTER(capi.Options), C.c_int, C.POINTER(ctx)], "ovgpu_destroy": [ctx], "ovgpu_set_state": [ctx, C.POINTER(capi.StateView)],
           "ovgpu_set_landmarks": [ctx, C.POINTER(capi.LandmarksView)], "ovgpu_set_active_landmarks": [ctx, C.c_int32, ip],
           "ovgpu_set_features": [ctx, C.POINTER(capi.FeaturesView)], "ovgpu_msckf_update": [ctx, ip, dp, dp, dp, dp, dp, st], "ovgpu_synchronize": [ctx],
           "ovgpu_last_update_route": [ctx]}
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, (None if name == "ovgpu_destroy" else C.c_int)
    lib.ovgpu_last_error.restype = C.c_char_p
    return lib


class Leg:
    """one context and the closures of its frame: prepare() is not timed, frame() is"""

    def __init__(self, capi, lib, opts, prob, kind):
        self.lib, self.kind, self.ctx = lib, kind, C.c_void_p()
        assert lib.ovgpu_create(C.byref(opts), 0, C.byref(self.ctx)) == 0
        self.v = capi.Views(prob)
        F, N = self.v.features.F, prob.N
        self.L = 0 if kind == "C" else int(prob.lm_cov_id.shape[0])
        self.st, self.x2, self.thr, self.pg = np.zeros(F, np.int32), np.zeros(F), np.zeros(F), np.zeros((F, 3))
        self.dx, self.P, self.lm = np.zeros(N), np.zeros((N, N)), np.zeros((max(self.L, 1), 3))
        self.stats = capi.UpdateStats()
        self.ip = lambda a: a.ctypes.data_as(capi.c_int32_p)
        self.dp = lambda a: a.ctypes.data_as(capi.c_double_p)
        if kind == "A":  # the landmark view of the corrected values
            self.val = np.array(self.v.lm_value, copy=True)
            self.lv2 = capi.LandmarksView()
            C.memmove(C.byref(self.lv2), C.byref(self.v.landmarks), C.sizeof(capi.LandmarksView))
            self.lv2.p_value = self.dp(self.val)
            self.ids = np.asarray(self.v.lm_cov_id, np.int64)[:, None] + np.arange(3)[None, :]

    def ok(self, rc, where):
        if rc != 0:
            raise RuntimeError(f"leg {self.kind}: {where} returned {rc}: {self.lib.ovgpu_last_error()}")

    def prepare(self):
        lib, ctx = self.lib, self.ctx
        self.ok(lib.ovgpu_set_state(ctx, C.byref(self.v.state)), "ovgpu_set_state")
        if self.kind != "C":
            self.ok(lib.ovgpu_set_landmarks(ctx, C.byref(self.v.landmarks)), "ovgpu_set_landmarks")
            self.ok(lib.ovgpu_set_active_landmarks(ctx, 0, None), "ovgpu_set_active_landmarks")
        self.ok(lib.ovgpu_synchronize(ctx), "ovgpu_synchronize")

    def frame(self):
        lib, ctx, ip, dp = self.lib, self.ctx, self.ip, self.dp
        self.ok(lib.ovgpu_set_features(ctx, C.byref(self.v.features)), "ovgpu_set_features")
        if self.kind == "B":
            self.ok(lib.ovgpu_msckf_update_lm(ctx, ip(self.st), dp(self.x2), dp(self.thr), dp(self.pg), dp(self.dx), dp(self.P), dp(self.lm), C.byref(self.stats)),
                    "ovgpu_msckf_update_lm")
            return
        self.ok(lib.ovgpu_msckf_update(ctx, ip(self.st), dp(self.x2), dp(self.thr), dp(self.pg), dp(self.dx), dp(self.P), C.byref(self.stats)), "ovgpu_msckf_update")
        if self.kind == "A":
            np.add(self.v.lm_value, self.dx[self.ids], out=self.val)  # Landmark::update on the host (global landmarks: 3 dof each)
            self.ok(lib.ovgpu_set_landmarks(ctx, C.byref(self.lv2)), "ovgpu_set_landmarks")
            self.ok(lib.ovgpu_synchronize(ctx), "ovgpu_synchronize")

    def close(self):
        self.lib.ovgpu_destroy(self.ctx)


def legs_for(capi, synth, a, L, which="ABC"):
    opts = capi.default_options()
    lm, plain = problems(synth, L, a.features)
    lib, lib_a = capi.load(), bind(capi, getattr(a, "lib_a", None))
    return {k: Leg(capi, lib_a if k == "A" else lib, opts, plain if k == "C" else lm, k) for k in which}, lm


def timed(a):
    import torch  # noqa: F401  (capi.load: torch's HIP runtime first)
    from open_vins_amd import capi, synth
    rows = []
    for L in (25, 50):
        legs, lm = legs_for(capi, synth, a, L)
        med = {k: [] for k in legs}
        for rnd in range(a.rounds):
            t = {k: [] for k in legs}
            for i in range(a.reps + 3):
                for k, leg in legs.items():  # interleaved frame by frame
                    leg.prepare()
                    t0 = time.perf_counter()
                    leg.frame()
                    t1 = time.perf_counter()
                    if i >= 3:
                        t[k].append((t1 - t0) * 1e3)
            for k in legs:
                med[k].append(float(np.median(t[k])))
        # the three legs computed one update: A and C through their own kernels, B the bits of C; B's landmarks are A's
        A, B, Cc = legs["A"], legs["B"], legs["C"]
        same = dict(B_returns_C_bits=bool(np.array_equal(B.st, Cc.st) and np.array_equal(B.dx, Cc.dx) and np.array_equal(B.P, Cc.P)),
                    A_accepts_what_B_accepts=bool(np.array_equal(A.st, B.st)), A_dx_rel_to_B=float(np.abs(A.dx - B.dx).max() / np.abs(B.dx).max()),
                    B_landmarks_are_value_plus_dx=bool(np.array_equal(B.lm[:L], lm.lm_value + B.dx[A.ids])), A_landmarks_max_abs_to_B=float(np.abs(A.val - B.lm[:L]).max()))
        for k, leg in legs.items():
            row = dict(case="msckf_lm", leg=k, L=L, features=int(a.features), n_used=int(leg.stats.n_used), N=int(lm.N), D=int(leg.stats.D), clones=int(lm.C),
                       cameras=int(lm.K), route=int(leg.lib.ovgpu_last_update_route(leg.ctx)), build=(a.tag_a if k == "A" else a.tag), reps=a.reps,
                       ms_round_medians=med[k], ms_median=float(np.median(med[k])), ms_spread=float(np.max(med[k]) - np.min(med[k])))
            rows.append(row)
            print(json.dumps(row), flush=True)
            leg.close()
        mA, mB, mC = (float(np.median(med[k])) for k in "ABC")
        spread = max(float(np.max(med[k]) - np.min(med[k])) for k in "ABC")
        row = dict(case="msckf_lm_summary", L=L, features=int(a.features), A_minus_B_ms=mA - mB, B_minus_C_ms=mB - mC, largest_spread_ms=spread,
                   B_faster_than_A_by_more_than_the_spread=bool(mA - mB > spread), **same)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


def trace(a):
    import torch  # noqa: F401
    from open_vins_amd import capi, synth
    legs, lm = legs_for(capi, synth, a, a.L, which=a.leg)
    leg = legs[a.leg]
    for _ in range(a.calls):
        leg.prepare()
        leg.frame()
    print(f"{a.calls} frames of leg {a.leg}, {a.features} features, L = {a.L}, {leg.stats.n_used} used, route {leg.lib.ovgpu_last_update_route(leg.ctx)}")
    leg.close()


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--reps", type=int, default=30)
    t.add_argument("--rounds", type=int, default=3)
    t.add_argument("--features", type=int, default=2000)
    t.add_argument("--lib-a", default=None)
    t.add_argument("--tag", default="tree")
    t.add_argument("--tag-a", default="parent")
    t.add_argument("--out", default=None)
    r = sub.add_parser("trace")
    r.add_argument("--L", type=int, default=50)
    r.add_argument("--leg", choices=("A", "B", "C"), default="B")
    r.add_argument("--calls", type=int, default=10)
    r.add_argument("--features", type=int, default=2000)
    a = ap.parse_args()
    {"time": timed, "trace": trace}[a.cmd](a)


if __name__ == "__main__":
    main()
