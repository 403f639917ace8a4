"""What the fused per-feature kernel of the SLAM update (csrc/k_slam_y.h, ovgpu_debug_option "slam_fused") is worth: the tree's library against
another build of it on one box.

    time [--reps 30] [--rounds 3] [--lib-a PATH] [--tag NAME] [--tag-a NAME] [--cases slam,chunked] [--state 3dof|mixed|long|big] [--level-a N] [--level-a1 0] [--level-b 1] [--big-b 0] [--out FILE.jsonl]
                    leg A runs on the library --lib-a names (the parent commit's build; without it: the tree's with the switch untouched), leg A' on
                    the tree's with "slam_fused" = --level-a1 (0), leg B on the tree's with "slam_fused" = --level-b (1): the switch is a level, an
                    integer.  A leg whose count of fused pipelines ("slam_fused_batches") is not what its level and the state say — some at level 1
                    on the 3-dof state and at level 2 on either, none otherwise — is an error, not a row.  Cases, timed host to host:
                      slam     ovgpu_slam_update, 30 clones stereo, L = 50 landmarks of the five 3-dof representations in turn, a batch of 25 features
                               under their own active set (D = 283); ovgpu_set_active_landmarks / ovgpu_set_features are part of the frame, the state
                               upload is not; ms_total of the last frame is recorded next to the host-to-host time
                      chunked  ovgpu_slam_update_chunked, L = 100, a batch of 100 in four chunks of 25 (ovgpu_set_features is part of the frame)
                    (DESIGN.md section 7's rows hold a single-depth landmark in every sixth place; at level 1 a batch that holds one keeps the general
                    kernel as a whole, so the landmarks of --state 3dof are the five 3-dof representations: 3 more columns per former single-depth
                    landmark.  --state mixed is the table's own state, the six representations in turn: --level-a1 1 --level-b 2 times the parent's
                    library, this one at level 1 — k_system_t, as the parent — and this one at level 2, k_slam_y<true>.
                    --state long is the four-camera rig: 30 clones x 4 cameras, the six representations in turn, every track as the rig sees it, up
                    to 120 observations (D = 303 for a batch of 25).  --level-a1 2 --level-b 3 times the parent's library, this one at level 2 —
                    k_system_t for every batch whose longest track exceeds 62 — and this one at level 3, the long shapes of k_slam_y.
                    --state big is BASELINE configs[4]'s rig: 50 clones x 4 cameras, the six representations in turn, every track as the rig sees
                    it, up to 200 observations (D = 423 for a batch of 25: every leg runs with "gram_wide" = 1, the Gram route for 384 .. 511
                    columns).  --level-a 3 --level-a1 3 --level-b 3 --big-b 1 times the parent's library at level 3 (--level-a sets "slam_fused" on
                    leg A too, for a parent that knows the name), this one at level 3 with "slam_fused_big" = 0 — k_system_t for every batch whose
                    longest track exceeds 126, as the parent — and this one with "slam_fused_big" = 1, the block-row shapes k_slam_y_big
                    (csrc/k_slam_y_big.h).)
                    The legs take turns frame by frame, `rounds` repetitions of `reps` frames; a row per (case, leg) with the median of every
                    round, the median of those and their spread (max - min), and a summary row: A' against A's spread, A - B against the largest spread.
    trace [--case slam] [--leg B] [--calls 10] [--lib-a PATH] [--state 3dof|mixed|long|big] [--level-a N] [--level-a1 0] [--level-b 1] [--big-b 0]
                    the frames of one leg alone, for a rocprofv3 --kernel-trace --stats run of its own"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEGS = ("A", "A'", "B")


def bind(capi, path):
    """a library by path with the entries the legs call"""
    if path is None:
        return capi.load()
    lib = C.CDLL(os.path.abspath(path))
    ip, dp, ctx, st = capi.c_int32_p, capi.c_double_p, C.c_void_p, C.POINTER(capi.UpdateStats)
    sig = {"ovgpu_create": [C.POINTER(capi.Options), C.c_int, C.POINTER(ctx)], "ovgpu_destroy": [ctx], "ovgpu_set_state": [ctx, C.POINTER(capi.StateView)],
           "ovgpu_set_landmarks": [ctx, C.POINTER(capi.LandmarksView)], "ovgpu_set_active_landmarks": [ctx, C.c_int32, ip],
           "ovgpu_set_features": [ctx, C.POINTER(capi.FeaturesView)], "ovgpu_slam_update": [ctx, ip, ip, dp, dp, dp, dp, dp, st], "ovgpu_synchronize": [ctx],
           "ovgpu_slam_update_chunked": [ctx, C.c_int32, ip, ip, ip, dp, dp, dp, dp, dp, st], "ovgpu_debug_option": [ctx, C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]}
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, (None if name == "ovgpu_destroy" else C.c_int)
    lib.ovgpu_last_error.restype = C.c_char_p
    return lib


class Leg:
    """one context and its frame: prepare() is not timed, frame() is"""

    def __init__(self, capi, synth, lib, case, kind, fused, state="3dof", big=0):
        """fused: an integer sets "slam_fused" to that level, None leaves the library alone (another build, which may not know the name);
        big: a level above 0 sets "slam_fused_big" (leg B only: no other build knows the name)"""
        self.lib, self.kind, self.case, self.ctx = lib, kind, case, C.c_void_p()
        opts = capi.default_options(chi2_multipler=1.0)
        assert lib.ovgpu_create(C.byref(opts), 0, C.byref(self.ctx)) == 0
        self.knows = fused is not None
        self.expect_fused = fused is not None and (fused >= 2 or (fused >= 1 and state == "3dof"))
        if state == "long":  # every batch holds a 120-observation track: fused at level 3 alone
            self.expect_fused = fused is not None and fused >= 3
        if fused is not None:
            self.ok(lib.ovgpu_debug_option(self.ctx, b"slam_fused", int(fused), None), "ovgpu_debug_option")
        if big:
            self.ok(lib.ovgpu_debug_option(self.ctx, b"slam_fused_big", int(big), None), "ovgpu_debug_option")
        if state == "big":  # D = 423: the Gram route for 384 .. 511 columns, on every leg
            self.ok(lib.ovgpu_debug_option(self.ctx, b"gram_wide", 1, None), "ovgpu_debug_option")
        self.ip = lambda a: a.ctypes.data_as(capi.c_int32_p)
        self.dp = lambda a: a.ctypes.data_as(capi.c_double_p)
        L, F = (50, 25) if case == "slam" else (100, 100)
        reps5 = [capi.REP_GLOBAL_3D, capi.REP_ANCHORED_3D, capi.REP_GLOBAL_FULL_INVERSE_DEPTH, capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, capi.REP_ANCHORED_FULL_INVERSE_DEPTH]
        reps6 = [capi.REP_GLOBAL_3D, capi.REP_ANCHORED_3D, capi.REP_GLOBAL_3D, capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, capi.REP_GLOBAL_FULL_INVERSE_DEPTH,
                 capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE]  # DESIGN.md section 7's rows (tools/dev_chol_wide_ab.py, tools/dev_slam_chunked_ab.py)
        reps = np.array((reps5 * ((L + 4) // 5))[:L] if state == "3dof" else (reps6 * ((L + 5) // 6))[:L], np.int32)
        if state in ("long", "big"):
            reps = np.array((reps6 * ((L + 5) // 6))[:L], np.int32)
        full = synth.make_slam_problem(2, L=L, lm_rep=reps, seed=3, **({"long": dict(C=30, K=4), "big": dict(C=50, K=4)}.get(state, {})))
        prob = full.subset(np.arange(F))
        prob.lm_index = np.ascontiguousarray(np.arange(F), dtype=np.int32)
        self.lm = prob.lm_index
        self.m_max = int(np.diff(prob.meas_offsets).max())
        self.first = np.arange(0, F + 1, 25, dtype=np.int32)
        if state == "big":  # a pipeline is fused when its batch's longest track is within the bound of the shapes the leg's switches allow
            lens = np.diff(prob.meas_offsets)
            bound = 0 if fused is None or fused < 3 else (232 if big else 126)
            self.expect_fused = any(int(lens[a:b].max()) <= bound for a, b in zip(self.first[:-1], self.first[1:]))
        n = len(self.first) - 1
        self.st, self.x2, self.thr, self.lmo = np.zeros(F, np.int32), np.zeros(F), np.zeros(F), np.zeros((L, 3))
        self.dxs = np.zeros((n, prob.N))
        self.stats = capi.UpdateStats() if case == "slam" else (capi.UpdateStats * n)()
        self.v = capi.Views(prob)
        self.dx, self.P = np.zeros(prob.N), np.zeros((prob.N, prob.N))

    def ok(self, rc, where):
        if rc != 0:
            raise RuntimeError(f"leg {self.kind}: {where} returned {rc}: {self.lib.ovgpu_last_error()}")

    def prepare(self):
        lib, ctx = self.lib, self.ctx
        self.ok(lib.ovgpu_set_state(ctx, C.byref(self.v.state)), "ovgpu_set_state")
        self.ok(lib.ovgpu_set_landmarks(ctx, C.byref(self.v.landmarks)), "ovgpu_set_landmarks")
        self.ok(lib.ovgpu_synchronize(ctx), "ovgpu_synchronize")

    def frame(self):
        lib, ctx, ip, dp = self.lib, self.ctx, self.ip, self.dp
        if self.case == "slam":
            self.ok(lib.ovgpu_set_active_landmarks(ctx, len(self.lm), ip(self.lm)), "ovgpu_set_active_landmarks")
            self.ok(lib.ovgpu_set_features(ctx, C.byref(self.v.features)), "ovgpu_set_features")
            self.ok(lib.ovgpu_slam_update(ctx, ip(self.lm), ip(self.st), dp(self.x2), dp(self.thr), dp(self.dx), dp(self.P), dp(self.lmo), C.byref(self.stats)),
                    "ovgpu_slam_update")
        else:
            self.ok(lib.ovgpu_set_features(ctx, C.byref(self.v.features)), "ovgpu_set_features")
            self.ok(lib.ovgpu_slam_update_chunked(ctx, len(self.first) - 1, ip(self.first), ip(self.lm), ip(self.st), dp(self.x2), dp(self.thr), dp(self.dxs),
                                                  dp(self.P), dp(self.lmo), self.stats), "ovgpu_slam_update_chunked")
            self.dx = self.dxs[-1]

    @property
    def D(self):
        """Jacobian columns of the last frame (of its first chunk), as the library reports them"""
        return int(self.stats.D if self.case == "slam" else self.stats[0].D)

    def fused_count(self):
        if not self.knows:
            return 0
        n = C.c_int64(0)
        self.ok(self.lib.ovgpu_debug_option(self.ctx, b"slam_fused_batches", -1, C.byref(n)), "ovgpu_debug_option")
        return int(n.value)

    def close(self):
        self.lib.ovgpu_destroy(self.ctx)


def make_legs(a, case, which=LEGS):
    import torch  # noqa: F401  (capi.load: torch's HIP runtime first)
    from open_vins_amd import capi, synth
    lib, lib_a = capi.load(), bind(capi, a.lib_a)
    return {k: Leg(capi, synth, lib_a if k == "A" else lib, case, k, fused={"A": a.level_a, "A'": a.level_a1, "B": a.level_b}[k], state=a.state, big=(a.big_b if k == "B" else 0)) for k in which}


def spread(v):
    return float(np.max(v) - np.min(v))


def timed(a):
    rows = []
    for case in a.cases.split(","):
        legs = make_legs(a, case)
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
        A, A1, B = legs["A"], legs["A'"], legs["B"]
        counts = {k: leg.fused_count() for k, leg in legs.items()}
        if any((counts[k] > 0) != leg.expect_fused for k, leg in legs.items()):
            raise RuntimeError(f"case {case}: fused pipelines per leg {counts} — nothing was compared")
        for k, leg in legs.items():
            row = dict(case=case, state=a.state, m_max=leg.m_max, leg=k, level=({"A": a.level_a, "A'": a.level_a1, "B": a.level_b}[k]), big=(a.big_b if k == "B" else 0), D=leg.D, build=(a.tag_a if k == "A" else a.tag), reps=a.reps, ms_round_medians=med[k],
                       ms_median=float(np.median(med[k])), ms_spread=spread(med[k]), fused_pipelines=counts[k])
            if case == "slam":
                row["ms_total_device"], row["n_used"] = float(leg.stats.ms_total), int(leg.stats.n_used)
            else:
                row["n_used"] = int(sum(s.n_used for s in leg.stats))
            rows.append(row)
            print(json.dumps(row), flush=True)
        mA, mA1, mB = (float(np.median(med[k])) for k in LEGS)
        big = max(spread(med["A"]), spread(med["B"]))
        row = dict(case=case + "_summary", state=a.state, D=B.D, A_minus_A1_ms=mA - mA1, spread_of_A_ms=spread(med["A"]), A1_within_the_spread_of_A=bool(abs(mA - mA1) <= spread(med["A"])),
                   A_minus_B_ms=mA - mB, largest_spread_of_A_and_B_ms=big, B_faster_than_A_by_more_than_the_spread=bool(mA - mB > big),
                   dx_rel_A_to_B=float(np.linalg.norm(A.dx - B.dx) / max(np.linalg.norm(B.dx), 1e-300)), P_rel_A_to_B=float(np.linalg.norm(A.P - B.P) / np.linalg.norm(B.P)),
                   A1_equals_A_bitwise=bool(np.array_equal(A.dx, A1.dx) and np.array_equal(A.P, A1.P)))
        rows.append(row)
        print(json.dumps(row), flush=True)
        for leg in legs.values():
            leg.close()
    if a.out:
        with open(a.out, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


def trace(a):
    leg = make_legs(a, a.case, which=(a.leg,))[a.leg]
    for _ in range(a.calls):
        leg.prepare()
        leg.frame()
    n = leg.fused_count()
    if (n > 0) != leg.expect_fused:
        raise RuntimeError(f"leg {a.leg} counted {n} fused pipelines")
    print(f"{a.calls} frames of leg {a.leg}, case {a.case}, D = {leg.D}, {n} fused pipelines")
    leg.close()


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--reps", type=int, default=30)
    t.add_argument("--rounds", type=int, default=3)
    t.add_argument("--cases", default="slam,chunked")
    t.add_argument("--lib-a", default=None)
    t.add_argument("--tag", default="tree")
    t.add_argument("--tag-a", default="parent")
    t.add_argument("--out", default=None)
    r = sub.add_parser("trace")
    r.add_argument("--case", default="slam")
    r.add_argument("--leg", choices=LEGS, default="B")
    r.add_argument("--calls", type=int, default=10)
    r.add_argument("--lib-a", default=None)
    for q in (t, r):
        q.add_argument("--state", choices=("3dof", "mixed", "long", "big"), default="3dof")
        q.add_argument("--level-a", type=int, default=None)
        q.add_argument("--big-b", type=int, default=0)
        q.add_argument("--level-a1", type=int, default=0)
        q.add_argument("--level-b", type=int, default=1)
    a = ap.parse_args()
    {"time": timed, "trace": trace}[a.cmd](a)


if __name__ == "__main__":
    main()
