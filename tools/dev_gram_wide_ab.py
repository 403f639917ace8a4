"""What the whitened Gram route is worth at 384 .. 511 Jacobian columns (ovgpu_debug_option "gram_wide"): three legs on one MI355X.

    time [--reps 30] [--rounds 3] [--lib-a PATH] [--control] [--cases slam476,msckf448,msckf384,msckf510] [--out FILE.jsonl]
                    leg A  runs on the library --lib-a names (the parent commit's build, which does not know the switch); without --lib-a the leg is left out
                    leg A' on the tree's library with "gram_wide" = 0 (the Householder route, as the parent takes it)
                    leg B  on the tree's library with "gram_wide" = 1
                    leg A2 (--control) a SECOND context on leg A's library, behind leg B in every frame: what two contexts of one build differ by
                    One context per leg.  The legs take turns frame by frame, `rounds` rounds of `reps` frames (three more warm each round up); a row per
                    (case, leg) with the median of every round, the median of those and their spread (max - min), and a summary row per case:
                    A' - A and A' - B against the largest spread.  A case whose leg B counted no "gram_wide_updates" is an error, not a row.
                    Cases, timed host to host:
                      slam476   ovgpu_slam_update, 30 clones stereo, L = 100 landmarks of the six representations in turn, ALL with columns
                                (D = 476), a batch of 25 features; ovgpu_set_features is part of the frame, the state and landmark upload is not
                      msckfD    ovgpu_set_features + ovgpu_msckf_update on a stereo state with calibration of D = 6 C + 28 columns:
                                msckf448 (70 clones) with F = 800 features, msckf384 is 57 clones x 3 cameras (6 C + 42) and msckf510 78 clones x 3
                                cameras, F = 100 each; any other msckfD with D = 6 C + 28 takes F = 100 (--features overrides; msckfD:F names its own)
                    ms_total of the last frame (the device time between the update's events) is recorded next to the host-to-host time.
    trace [--case msckf448] [--leg B] [--calls 10] [--lib-a PATH]
                    the frames of one leg alone, for a rocprofv3 --kernel-trace --stats run of its own"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.dev_chol_wide_ab import bind  # noqa: E402  (a library by path with the entries the legs call)

MSCKF = {448: dict(C=70, K=2, F=800), 384: dict(C=57, K=3, F=100), 510: dict(C=78, K=3, F=100)}


class Leg:
    """one context and its frame: prepare() is not timed, frame() is"""

    def __init__(self, capi, synth, lib, case, kind, wide, features=None):
        """wide: 1 / 0 sets "gram_wide" (the tree's library), None leaves the library alone (another build, which does not know the name)"""
        self.lib, self.kind, self.case, self.ctx = lib, kind, case, C.c_void_p()
        opts = capi.default_options(chi2_multipler=1.0)
        assert lib.ovgpu_create(C.byref(opts), 0, C.byref(self.ctx)) == 0
        if wide is not None:
            self.ok(lib.ovgpu_debug_option(self.ctx, b"gram_wide", int(wide), None), "ovgpu_debug_option")
        self.ip = lambda a: a.ctypes.data_as(capi.c_int32_p)
        self.dp = lambda a: a.ctypes.data_as(capi.c_double_p)
        if case.startswith("msckf"):
            D, _, f_own = case[5:].partition(":")  # msckfD or msckfD:F
            D = int(D)
            st = MSCKF.get(D) or dict(C=(D - 28) // 6, K=2, F=100)
            assert 6 * st["C"] + 14 * st["K"] == D, f"no state of {D} columns"
            prob = synth.make_problem(2, C=st["C"], K=st["K"], F=int(f_own) if f_own else (features or st["F"]), seed=5)
            F, self.D = prob.F, prob.Dmax
            self.st, self.x2, self.thr, self.pg = np.zeros(F, np.int32), np.zeros(F), np.zeros(F), np.zeros((F, 3))
        elif case == "slam476":
            L, F = 100, 25
            reps6 = [capi.REP_GLOBAL_3D, capi.REP_ANCHORED_3D, capi.REP_GLOBAL_3D, capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, capi.REP_GLOBAL_FULL_INVERSE_DEPTH,
                     capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE]
            reps = np.array((reps6 * ((L + 5) // 6))[:L], np.int32)
            full = synth.make_slam_problem(2, L=L, lm_rep=reps, seed=3)
            prob = full.subset(np.arange(F))
            prob.lm_index = np.ascontiguousarray(np.arange(F), dtype=np.int32)
            self.lm = prob.lm_index
            self.D = 208 + int(np.where(reps == capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE, 1, 3).sum())
            self.st, self.x2, self.thr, self.lmo = np.zeros(F, np.int32), np.zeros(F), np.zeros(F), np.zeros((L, 3))
        else:
            raise SystemExit(f"unknown case {case}")
        self.stats = capi.UpdateStats()
        self.v = capi.Views(prob)
        self.dx, self.P = np.zeros(prob.N), np.zeros((prob.N, prob.N))

    def ok(self, rc, where):
        if rc != 0:
            raise RuntimeError(f"leg {self.kind}: {where} returned {rc}: {self.lib.ovgpu_last_error()}")

    def prepare(self):
        lib, ctx = self.lib, self.ctx
        self.ok(lib.ovgpu_set_state(ctx, C.byref(self.v.state)), "ovgpu_set_state")
        if self.case == "slam476":
            self.ok(lib.ovgpu_set_landmarks(ctx, C.byref(self.v.landmarks)), "ovgpu_set_landmarks")
        self.ok(lib.ovgpu_synchronize(ctx), "ovgpu_synchronize")

    def frame(self):
        lib, ctx, ip, dp = self.lib, self.ctx, self.ip, self.dp
        self.ok(lib.ovgpu_set_features(ctx, C.byref(self.v.features)), "ovgpu_set_features")
        if self.case == "slam476":
            self.ok(lib.ovgpu_slam_update(ctx, ip(self.lm), ip(self.st), dp(self.x2), dp(self.thr), dp(self.dx), dp(self.P), dp(self.lmo), C.byref(self.stats)),
                    "ovgpu_slam_update")
        else:
            self.ok(lib.ovgpu_msckf_update(ctx, ip(self.st), dp(self.x2), dp(self.thr), dp(self.pg), dp(self.dx), dp(self.P), C.byref(self.stats)), "ovgpu_msckf_update")

    def counter(self, name):
        n = C.c_int64(0)
        self.ok(self.lib.ovgpu_debug_option(self.ctx, name.encode(), -1, C.byref(n)), "ovgpu_debug_option")
        return int(n.value)

    def close(self):
        self.lib.ovgpu_destroy(self.ctx)


LEGS = {"A": None, "A'": 0, "B": 1, "A2": None}


def make_legs(a, case, which=None):
    import torch  # noqa: F401  (capi.load: torch's HIP runtime first)
    from open_vins_amd import capi, synth
    lib, lib_a = capi.load(), (bind(capi, a.lib_a) if a.lib_a else None)
    which = which or [k for k in LEGS if (k != "A" or lib_a is not None) and (k != "A2" or (lib_a is not None and getattr(a, "control", False)))]
    if ("A" in which or "A2" in which) and lib_a is None:
        raise SystemExit("legs A and A2 need --lib-a")
    return {k: Leg(capi, synth, lib_a if k in ("A", "A2") else lib, case, k, LEGS[k], getattr(a, "features", None)) for k in which}


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
        B, A1 = legs["B"], legs["A'"]
        n_wide = B.counter("gram_wide_updates")
        if n_wide == 0:
            raise RuntimeError(f"case {case}: leg B counted no gram_wide_updates — nothing was compared")
        if A1.counter("gram_wide_updates") != 0:
            raise RuntimeError(f"case {case}: leg A' took the wide route")
        for k, leg in legs.items():
            row = dict(case=case, leg=k, D=leg.D, F=int(leg.v.features.F), reps=a.reps, ms_round_medians=med[k], ms_median=float(np.median(med[k])),
                       ms_spread=float(np.max(med[k]) - np.min(med[k])), ms_total_device=float(leg.stats.ms_total), n_used=int(leg.stats.n_used))
            if k in ("A'", "B"):
                row["last_feature_kernel"], row["last_gram_kernel"] = leg.counter("last_feature_kernel"), leg.counter("last_gram_kernel")
            rows.append(row)
            print(json.dumps(row), flush=True)
        m = {k: float(np.median(med[k])) for k in legs}
        spread = max(float(np.max(med[k]) - np.min(med[k])) for k in legs)
        row = dict(case=case + "_summary", D=B.D, F=int(B.v.features.F), largest_spread_ms=spread, Aprime_minus_B_ms=m["A'"] - m["B"],
                   B_faster_than_Aprime_by_more_than_the_spread=bool(m["A'"] - m["B"] > spread), speedup_Aprime_over_B=m["A'"] / m["B"],
                   gram_wide_updates_of_B=n_wide, dx_rel_Aprime_to_B=float(np.linalg.norm(A1.dx - B.dx) / max(np.linalg.norm(B.dx), 1e-300)),
                   P_rel_Aprime_to_B=float(np.linalg.norm(A1.P - B.P) / np.linalg.norm(B.P)))
        if "A" in legs:
            row["Aprime_minus_A_ms"] = m["A'"] - m["A"]
            row["Aprime_equals_A_within_the_spread"] = bool(abs(m["A'"] - m["A"]) <= spread)
            row["A_and_Aprime_same_bits"] = bool(np.array_equal(legs["A"].dx, A1.dx) and np.array_equal(legs["A"].P, A1.P))
        if "A2" in legs:  # the control: two contexts of ONE build
            row["A2_minus_A_ms"] = m["A2"] - m["A"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        for leg in legs.values():
            leg.close()
    if a.out:
        with open(a.out, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


def trace(a):
    leg = make_legs(a, a.case, which=[a.leg])[a.leg]
    for _ in range(a.calls):
        leg.prepare()
        leg.frame()
    n = leg.counter("gram_wide_updates") if a.leg != "A" else 0
    if (n > 0) != (a.leg == "B"):
        raise RuntimeError(f"leg {a.leg} counted {n} gram_wide_updates")
    print(f"{a.calls} frames of leg {a.leg}, case {a.case}, D = {leg.D}, F = {leg.v.features.F}, {n} gram_wide_updates")
    leg.close()


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--reps", type=int, default=30)
    t.add_argument("--rounds", type=int, default=3)
    t.add_argument("--cases", default="slam476,msckf448,msckf384,msckf510")
    t.add_argument("--features", type=int, default=None)
    t.add_argument("--lib-a", default=None)
    t.add_argument("--control", action="store_true")
    t.add_argument("--out", default=None)
    r = sub.add_parser("trace")
    r.add_argument("--case", default="msckf448")
    r.add_argument("--leg", choices=("A", "A'", "B"), default="B")
    r.add_argument("--calls", type=int, default=10)
    r.add_argument("--features", type=int, default=None)
    r.add_argument("--lib-a", default=None)
    a = ap.parse_args()
    {"time": timed, "trace": trace}[a.cmd](a)


if __name__ == "__main__":
    main()
