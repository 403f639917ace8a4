"""What the fused per-feature kernels are worth to a filter configured with an anchored feat_rep_msckf: four legs of one frame's MSCKF update on one box.

    time [--reps 30] [--rounds 3] [--features 2000] [--rep 4] [--lib-a PATH] [--tag NAME] [--out FILE.jsonl]
                    configs[2]: 2000 features, 30 clones, stereo, online camera / IMU calibration (N = 248).  Per frame the state is uploaded and the
                    stream drained, not timed; then, timed host to host, ovgpu_set_features and ovgpu_msckf_update (triangulation on the device):
                      A   feat_rep_msckf = --rep on the library --lib-a names (the parent commit's build: the general kernel, 72-double records;
                          default: the tree's library with "anchored_fast" = 0, which is that routing)
                      A'  the tree's library, "anchored_fast" = 0
                      B   the tree's library as it comes: k_feat_rows_anchored and the fused kernels
                      C   the same problem under GLOBAL_3D: the fused kernels' own time
                    The legs take turns frame by frame, `rounds` repetitions of `reps` frames; a row per leg with the median of every round, the
                    median of those and their spread (max - min): the yardstick for a difference between two legs.
    trace [--leg B] [--calls 10] [--features 2000] [--rep 4]
                    the frames of one leg alone, for a rocprofv3 --kernel-trace --stats run of its own (which per-feature kernels run)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bind(capi, path):
    """a library by path with the handful of entries the legs call"""
    if path is None:
        return capi.load()
    lib = C.CDLL(os.path.abspath(path))
    ip, dp, ctx, st = capi.c_int32_p, capi.c_double_p, C.c_void_p, C.POINTER(capi.UpdateStats)
    sig = {"ovgpu_create": [C.POINTER(capi.Options), C.c_int, C.POINTER(ctx)], "ovgpu_destroy": [ctx], "ovgpu_set_state": [ctx, C.POINTER(capi.StateView)],
           "ovgpu_set_features": [ctx, C.POINTER(capi.FeaturesView)], "ovgpu_msckf_update": [ctx, ip, dp, dp, dp, dp, dp, st], "ovgpu_synchronize": [ctx],
           "ovgpu_last_update_route": [ctx], "ovgpu_debug_option": [ctx, C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]}
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, (None if name == "ovgpu_destroy" else C.c_int)
    lib.ovgpu_last_error.restype = C.c_char_p
    return lib


class Leg:
    """one context and the closures of its frame: prepare() is not timed, frame() is"""

    def __init__(self, capi, lib, opts, prob, kind, switch_off):
        self.lib, self.kind, self.ctx = lib, kind, C.c_void_p()
        assert lib.ovgpu_create(C.byref(opts), 0, C.byref(self.ctx)) == 0
        if switch_off:
            self.ok(lib.ovgpu_debug_option(self.ctx, b"anchored_fast", 0, None), "ovgpu_debug_option anchored_fast")
        self.v = capi.Views(prob)
        F, N = self.v.features.F, prob.N
        self.st, self.x2, self.thr, self.pg = np.zeros(F, np.int32), np.zeros(F), np.zeros(F), np.zeros((F, 3))
        self.dx, self.P = np.zeros(N), np.zeros((N, N))
        self.stats = capi.UpdateStats()
        self.ip = lambda a: a.ctypes.data_as(capi.c_int32_p)
        self.dp = lambda a: a.ctypes.data_as(capi.c_double_p)

    def ok(self, rc, where):
        if rc != 0:
            raise RuntimeError(f"leg {self.kind}: {where} returned {rc}: {self.lib.ovgpu_last_error()}")

    def kernel(self):
        old = C.c_int64(-1)
        self.ok(self.lib.ovgpu_debug_option(self.ctx, b"last_feature_kernel", -1, C.byref(old)), "ovgpu_debug_option last_feature_kernel")
        return int(old.value)

    def prepare(self):
        self.ok(self.lib.ovgpu_set_state(self.ctx, C.byref(self.v.state)), "ovgpu_set_state")
        self.ok(self.lib.ovgpu_synchronize(self.ctx), "ovgpu_synchronize")

    def frame(self):
        lib, ctx, ip, dp = self.lib, self.ctx, self.ip, self.dp
        self.ok(lib.ovgpu_set_features(ctx, C.byref(self.v.features)), "ovgpu_set_features")
        self.ok(lib.ovgpu_msckf_update(ctx, ip(self.st), dp(self.x2), dp(self.thr), dp(self.pg), dp(self.dx), dp(self.P), C.byref(self.stats)), "ovgpu_msckf_update")

    def close(self):
        self.lib.ovgpu_destroy(self.ctx)


LEGS = ("A", "A'", "B", "C")


def legs_for(capi, synth, a, which=LEGS):
    prob = synth.make_problem(3, F=a.features, imu_intrinsics=True)
    lib, lib_a = capi.load(), bind(capi, getattr(a, "lib_a", None))
    anchored, glob = capi.default_options(feat_rep_msckf=a.rep), capi.default_options()
    legs = {}
    for k in which:
        # (the parent commit's library does not know the switch and needs none; without --lib-a leg A is leg A' on a context of its own)
        off = k == "A'" or (k == "A" and getattr(a, "lib_a", None) is None)
        legs[k] = Leg(capi, lib_a if k == "A" else lib, glob if k == "C" else anchored, prob, k, off)
    return legs, prob


def _rel(x, y):
    return float(np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-300))


def timed(a):
    import torch  # noqa: F401  (capi.load: torch's HIP runtime first)
    from open_vins_amd import capi, synth
    legs, prob = legs_for(capi, synth, a)
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
    rows = []
    B = legs["B"]
    for k, leg in legs.items():
        row = dict(case="anchored_fast", leg=k, feat_rep_msckf=0 if k == "C" else int(a.rep), features=int(a.features), n_used=int(leg.stats.n_used), N=int(prob.N),
                   D=int(leg.stats.D), clones=int(prob.C), cameras=int(prob.K), route=int(leg.lib.ovgpu_last_update_route(leg.ctx)), feature_kernel=leg.kernel(),
                   build=(a.tag_a if k == "A" and a.lib_a else a.tag), reps=a.reps, ms_round_medians=med[k], ms_median=float(np.median(med[k])),
                   ms_spread=float(np.max(med[k]) - np.min(med[k])), same_accept_set_as_B=bool(np.array_equal(leg.st, B.st)), dx_rel_to_B=_rel(leg.dx, B.dx),
                   P_rel_to_B=_rel(leg.P, B.P))
        rows.append(row)
        print(json.dumps(row), flush=True)
    m = {k: float(np.median(med[k])) for k in legs}
    spread = max(float(np.max(med[k]) - np.min(med[k])) for k in legs)
    row = dict(case="anchored_fast_summary", feat_rep_msckf=int(a.rep), features=int(a.features), A_minus_B_ms=m["A"] - m["B"], Ap_minus_B_ms=m["A'"] - m["B"],
               B_minus_C_ms=m["B"] - m["C"], largest_spread_ms=spread, B_faster_than_A_by_more_than_the_spread=bool(m["A"] - m["B"] > spread),
               B_within_the_spread_of_C=bool(abs(m["B"] - m["C"]) <= spread))
    rows.append(row)
    print(json.dumps(row), flush=True)
    for leg in legs.values():
        leg.close()
    if a.out:
        with open(a.out, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


def trace(a):
    import torch  # noqa: F401
    from open_vins_amd import capi, synth
    legs, prob = legs_for(capi, synth, a, which=(a.leg,))
    leg = legs[a.leg]
    for _ in range(a.calls):
        leg.prepare()
        leg.frame()
    print(f"{a.calls} frames of leg {a.leg}, {a.features} features, feat_rep_msckf {0 if a.leg == 'C' else a.rep}, {leg.stats.n_used} used, "
          f"route {leg.lib.ovgpu_last_update_route(leg.ctx)}, last_feature_kernel {leg.kernel()}")
    leg.close()


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--reps", type=int, default=30)
    t.add_argument("--rounds", type=int, default=3)
    t.add_argument("--features", type=int, default=2000)
    t.add_argument("--rep", type=int, default=4)
    t.add_argument("--lib-a", default=None)
    t.add_argument("--tag", default="tree")
    t.add_argument("--tag-a", default="parent")
    t.add_argument("--out", default=None)
    r = sub.add_parser("trace")
    r.add_argument("--leg", choices=LEGS, default="B")
    r.add_argument("--calls", type=int, default=10)
    r.add_argument("--features", type=int, default=2000)
    r.add_argument("--rep", type=int, default=4)
    a = ap.parse_args()
    {"time": timed, "trace": trace}[a.cmd](a)


if __name__ == "__main__":
    main()
