"""What the pivoted Gram route is worth to mode A of the SLAM update (ovgpu_slam_compress under ovgpu_debug_option "slam_mode_a"): five legs on one
MI355X, after tools/dev_mode_a_wide_ab.py.

    time [--reps 30] [--rounds 3] [--lib-a PATH] [--control] [--lib-b2 PATH] [--cases slam283,slam358,slam476,slam223] [--out FILE.jsonl]
                    leg A   runs on the library --lib-a names (the parent commit's build, which does not know the switch); without --lib-a it is left out
                    leg A'  on the tree's library with "slam_mode_a" = 0 (the Householder route, as the parent takes it)
                    leg B   on the tree's library with "slam_mode_a" = 1 (and "mode_a_wide" = 1 beyond 383 columns)
                    leg B+f leg B with "slam_fused" = 3: the per-feature stage as k_slam_y
                    leg B2  (--lib-b2) leg B on another build of this tree (a scratch build with another un-whitening shape in the 257 .. 383 band)
                    leg A2  (--control) a SECOND context on leg A's library, behind the others in every frame: what two contexts of one build differ by
                    One context per leg.  The legs take turns frame by frame, `rounds` rounds of `reps` frames (three more warm each round up); a row per
                    (case, leg) with the median of every round, the median of those and their spread (max - min), and a summary row per case:
                    A' - A against the larger of the spread and |A2 - A|, A' - B and A' - B+f against the largest spread.  A case whose leg B counted
                    no "slam_mode_a_compressions" is an error, not a row.
                    Cases, timed host to host (ovgpu_set_features + ovgpu_slam_compress; the state and landmark upload is not), 30 clones x 2 cameras
                    with full calibration (208 columns) and every resident landmark with columns:
                      slam283  25 3-dof landmarks, a batch of 25        slam358  50 3-dof landmarks, a batch of 50
                      slam223  5 3-dof landmarks, a batch of 5          slam476  100 landmarks of the six representations in turn, a batch of 25
    trace [--case slam358] [--leg B] [--calls 10] [--lib-a PATH] [--lib-b2 PATH]
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

COUNTER = "slam_mode_a_compressions"
CASES = {"slam283": (25, 25, False), "slam358": (50, 50, False), "slam223": (5, 5, False), "slam476": (100, 25, True)}  # landmarks, batch, six representations


class Leg:
    """one context and its frame: prepare() is not timed, frame() is"""

    def __init__(self, capi, synth, lib, case, kind, level, fused=0):
        """level: 1 / 0 sets "slam_mode_a" (a build of this tree), None leaves the library alone (another build, which does not know the name)"""
        self.lib, self.kind, self.case, self.ctx = lib, kind, case, C.c_void_p()
        ip, dp, st = capi.c_int32_p, capi.c_double_p, C.POINTER(capi.UpdateStats)
        lib.ovgpu_slam_compress.argtypes = [C.c_void_p, ip, ip, dp, dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), ip, dp, dp, st]
        lib.ovgpu_slam_compress.restype = C.c_int
        opts = capi.default_options(chi2_multipler=1.0)
        assert lib.ovgpu_create(C.byref(opts), 0, C.byref(self.ctx)) == 0
        L, F, six = CASES[case]
        r5 = [capi.REP_GLOBAL_3D, capi.REP_ANCHORED_3D, capi.REP_GLOBAL_FULL_INVERSE_DEPTH, capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, capi.REP_ANCHORED_FULL_INVERSE_DEPTH]
        r6 = [capi.REP_GLOBAL_3D, capi.REP_ANCHORED_3D, capi.REP_GLOBAL_3D, capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, capi.REP_GLOBAL_FULL_INVERSE_DEPTH,
              capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE]
        reps = np.array(((r6 if six else r5) * (L // 5 + 1))[:L], np.int32)
        self.D = 208 + int(np.where(reps == capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE, 1, 3).sum())
        if level is not None:
            self.ok(lib.ovgpu_debug_option(self.ctx, b"slam_mode_a", int(level), None), "ovgpu_debug_option")
            if level >= 1 and self.D > 383:
                self.ok(lib.ovgpu_debug_option(self.ctx, b"mode_a_wide", 1, None), "ovgpu_debug_option")
            if fused:
                self.ok(lib.ovgpu_debug_option(self.ctx, b"slam_fused", int(fused), None), "ovgpu_debug_option")
        self.ip = lambda a: a.ctypes.data_as(ip)
        self.dp = lambda a: a.ctypes.data_as(dp)
        full = synth.make_slam_problem(2, L=L, lm_rep=reps, seed=3)
        prob = full.subset(np.arange(F))
        prob.lm_index = np.ascontiguousarray(np.arange(F), dtype=np.int32)
        self.lm = prob.lm_index
        self.st, self.x2, self.thr = np.zeros(F, np.int32), np.zeros(F), np.zeros(F)
        self.H, self.r, self.cols = np.zeros((self.D, self.D)), np.zeros(self.D), np.zeros(self.D, np.int32)
        self.D_out, self.rows = C.c_int32(0), C.c_int32(0)
        self.stats = capi.UpdateStats()
        self.v = capi.Views(prob)

    def ok(self, rc, where):
        if rc != 0:
            raise RuntimeError(f"leg {self.kind}: {where} returned {rc}: {self.lib.ovgpu_last_error()}")

    def prepare(self):
        self.ok(self.lib.ovgpu_set_state(self.ctx, C.byref(self.v.state)), "ovgpu_set_state")
        self.ok(self.lib.ovgpu_set_landmarks(self.ctx, C.byref(self.v.landmarks)), "ovgpu_set_landmarks")
        self.ok(self.lib.ovgpu_synchronize(self.ctx), "ovgpu_synchronize")

    def frame(self):
        lib, ctx, ip, dp = self.lib, self.ctx, self.ip, self.dp
        self.ok(lib.ovgpu_set_features(ctx, C.byref(self.v.features)), "ovgpu_set_features")
        self.ok(lib.ovgpu_slam_compress(ctx, ip(self.lm), ip(self.st), dp(self.x2), dp(self.thr), C.byref(self.D_out), C.byref(self.rows), ip(self.cols),
                                        dp(self.H), dp(self.r), C.byref(self.stats)), "ovgpu_slam_compress")

    def gram(self):
        """H^T H and H^T r of the rows the last frame returned: what two routes must agree on"""
        n = int(self.rows.value)
        H = self.H.reshape(-1)[: n * self.D].reshape(n, self.D)
        return H.T @ H, H.T @ self.r[:n]

    def counter(self, name):
        n = C.c_int64(0)
        self.ok(self.lib.ovgpu_debug_option(self.ctx, name.encode(), -1, C.byref(n)), "ovgpu_debug_option")
        return int(n.value)

    def close(self):
        self.lib.ovgpu_destroy(self.ctx)


LEGS = {"A": (None, 0), "A'": (0, 0), "B": (1, 0), "B+f": (1, 3), "B2": (1, 0), "A2": (None, 0)}


def make_legs(a, case, which=None):
    import torch  # noqa: F401  (capi.load: torch's HIP runtime first)
    from open_vins_amd import capi, synth
    lib, lib_a, lib_b2 = capi.load(), (bind(capi, a.lib_a) if a.lib_a else None), (bind(capi, a.lib_b2) if a.lib_b2 else None)
    which = which or [k for k in LEGS if (k != "A" or lib_a is not None) and (k != "A2" or (lib_a is not None and getattr(a, "control", False)))
                      and (k != "B2" or lib_b2 is not None)]
    if ("A" in which or "A2" in which) and lib_a is None:
        raise SystemExit("legs A and A2 need --lib-a")
    if "B2" in which and lib_b2 is None:
        raise SystemExit("leg B2 needs --lib-b2")
    pick = {"A": lib_a, "A2": lib_a, "B2": lib_b2}
    return {k: Leg(capi, synth, pick.get(k, lib), case, k, *LEGS[k]) for k in which}


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
        n_new = B.counter(COUNTER)
        if n_new == 0:
            raise RuntimeError(f"case {case}: leg B counted no {COUNTER} — nothing was compared")
        if A1.counter(COUNTER) != 0:
            raise RuntimeError(f"case {case}: leg A' took the pivoted route")
        for k, leg in legs.items():
            row = dict(case=case, leg=k, D=leg.D, F=int(leg.v.features.F), reps=a.reps, ms_round_medians=med[k], ms_median=float(np.median(med[k])),
                       ms_spread=float(np.max(med[k]) - np.min(med[k])), rows=int(leg.rows.value), n_used=int(leg.stats.n_used))
            if k not in ("A", "A2"):
                for name in ("last_feature_kernel", "last_gram_kernel", "last_factor_kernel", "last_unwhiten_kernel"):
                    row[name] = leg.counter(name)
            rows.append(row)
            print(json.dumps(row), flush=True)
        m = {k: float(np.median(med[k])) for k in legs}
        spread = max(float(np.max(med[k]) - np.min(med[k])) for k in legs)
        (Ga, ga), (Gb, gb) = A1.gram(), B.gram()
        row = dict(case=case + "_summary", D=B.D, F=int(B.v.features.F), largest_spread_ms=spread, Aprime_minus_B_ms=m["A'"] - m["B"],
                   B_faster_than_Aprime_by_more_than_the_spread=bool(m["A'"] - m["B"] > spread), speedup_Aprime_over_B=m["A'"] / m["B"],
                   Aprime_minus_Bf_ms=m["A'"] - m["B+f"], Bf_faster_than_Aprime_by_more_than_the_spread=bool(m["A'"] - m["B+f"] > spread),
                   speedup_Aprime_over_Bf=m["A'"] / m["B+f"], rows_Aprime=int(A1.rows.value), rows_B=int(B.rows.value),
                   slam_mode_a_compressions_of_B=n_new, HtH_rel_Aprime_to_B=float(np.linalg.norm(Ga - Gb) / max(np.linalg.norm(Gb), 1e-300)),
                   Htr_rel_Aprime_to_B=float(np.linalg.norm(ga - gb) / max(np.linalg.norm(gb), 1e-300)))
        if "B2" in legs:
            row["B2_minus_B_ms"] = m["B2"] - m["B"]
            row["B2_and_B_same_bits"] = bool(np.array_equal(legs["B2"].H, B.H) and np.array_equal(legs["B2"].r, B.r))
        if "A" in legs:
            row["Aprime_minus_A_ms"] = m["A'"] - m["A"]
            row["A_and_Aprime_same_bits"] = bool(np.array_equal(legs["A"].H, A1.H) and np.array_equal(legs["A"].r, A1.r))
            margin = spread
            if "A2" in legs:  # the control: two contexts of ONE build
                row["A2_minus_A_ms"] = m["A2"] - m["A"]
                margin = max(spread, abs(m["A2"] - m["A"]))
            row["Aprime_equals_A_within_the_margin"] = bool(abs(m["A'"] - m["A"]) <= margin)
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
    n = leg.counter(COUNTER) if a.leg not in ("A", "A2") else 0
    if (n > 0) != (a.leg in ("B", "B+f", "B2")):
        raise RuntimeError(f"leg {a.leg} counted {n} {COUNTER}")
    print(f"{a.calls} frames of leg {a.leg}, case {a.case}, D = {leg.D}, F = {leg.v.features.F}, {n} {COUNTER}, rows {leg.rows.value}")
    leg.close()


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--reps", type=int, default=30)
    t.add_argument("--rounds", type=int, default=3)
    t.add_argument("--cases", default="slam283,slam358,slam476,slam223")
    t.add_argument("--lib-a", default=None)
    t.add_argument("--lib-b2", default=None)
    t.add_argument("--control", action="store_true")
    t.add_argument("--out", default=None)
    r = sub.add_parser("trace")
    r.add_argument("--case", default="slam358")
    r.add_argument("--leg", choices=tuple(LEGS), default="B")
    r.add_argument("--calls", type=int, default=10)
    r.add_argument("--lib-a", default=None)
    r.add_argument("--lib-b2", default=None)
    a = ap.parse_args()
    {"time": timed, "trace": trace}[a.cmd](a)


if __name__ == "__main__":
    main()
