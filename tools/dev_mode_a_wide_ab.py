"""What mode A's pivoted Gram route is worth at 384 .. 511 Jacobian columns (ovgpu_debug_option "mode_a_wide"): three legs on one MI355X, after
tools/dev_gram_wide_ab.py.

    time [--reps 30] [--rounds 3] [--lib-a PATH] [--control] [--cases modeA448,modeA448:100,modeA384,modeA510] [--out FILE.jsonl]
                    leg A  runs on the library --lib-a names (the parent commit's build, which does not know the switch); without --lib-a the leg is left out
                    leg A' on the tree's library with "mode_a_wide" = 0 (the Householder route, as the parent takes it)
                    leg B  on the tree's library with "mode_a_wide" = 1
                    leg A2 (--control) a SECOND context on leg A's library, behind leg B in every frame: what two contexts of one build differ by
                    One context per leg.  The legs take turns frame by frame, `rounds` rounds of `reps` frames (three more warm each round up); a row per
                    (case, leg) with the median of every round, the median of those and their spread (max - min), and a summary row per case:
                    A' - A and A' - B against the largest spread.  A case whose leg B counted no "mode_a_wide_compressions" is an error, not a row.
                    Cases, timed host to host: modeAD[:F] is ovgpu_set_features + ovgpu_msckf_compress on a state with full calibration of
                    D = 6 C + 14 K columns — modeA448 70 clones x 2 cameras with F = 800 features, modeA384 57 clones x 3 cameras and modeA510
                    78 clones x 3 cameras with F = 100; :F names another feature count.
    trace [--case modeA448] [--leg B] [--calls 10] [--lib-a PATH]
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

STATES = {448: dict(C=70, K=2, F=800), 384: dict(C=57, K=3, F=100), 510: dict(C=78, K=3, F=100)}
COUNTER = "mode_a_wide_compressions"


class Leg:
    """one context and its frame: prepare() is not timed, frame() is"""

    def __init__(self, capi, synth, lib, case, kind, level):
        """level: 1 / 0 sets "mode_a_wide" (the tree's library), None leaves the library alone (another build, which does not know the name)"""
        self.lib, self.kind, self.case, self.ctx = lib, kind, case, C.c_void_p()
        ip, dp, st = capi.c_int32_p, capi.c_double_p, C.POINTER(capi.UpdateStats)
        lib.ovgpu_msckf_compress.argtypes = [C.c_void_p, ip, dp, dp, dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), ip, dp, dp, st]
        lib.ovgpu_msckf_compress.restype = C.c_int
        opts = capi.default_options(chi2_multipler=1.0)
        assert lib.ovgpu_create(C.byref(opts), 0, C.byref(self.ctx)) == 0
        if level is not None:
            self.ok(lib.ovgpu_debug_option(self.ctx, b"mode_a_wide", int(level), None), "ovgpu_debug_option")
        self.ip = lambda a: a.ctypes.data_as(ip)
        self.dp = lambda a: a.ctypes.data_as(dp)
        D, _, f_own = case[5:].partition(":")  # modeAD or modeAD:F
        s = STATES[int(D)]
        prob = synth.make_problem(2, C=s["C"], K=s["K"], F=int(f_own) if f_own else s["F"], seed=5)
        F, self.D = prob.F, prob.Dmax
        assert self.D == int(D)
        self.st, self.x2, self.thr, self.pg = np.zeros(F, np.int32), np.zeros(F), np.zeros(F), np.zeros((F, 3))
        self.H, self.r, self.cols = np.zeros((self.D, self.D)), np.zeros(self.D), np.zeros(self.D, np.int32)
        self.D_out, self.rows = C.c_int32(0), C.c_int32(0)
        self.stats = capi.UpdateStats()
        self.v = capi.Views(prob)

    def ok(self, rc, where):
        if rc != 0:
            raise RuntimeError(f"leg {self.kind}: {where} returned {rc}: {self.lib.ovgpu_last_error()}")

    def prepare(self):
        self.ok(self.lib.ovgpu_set_state(self.ctx, C.byref(self.v.state)), "ovgpu_set_state")
        self.ok(self.lib.ovgpu_synchronize(self.ctx), "ovgpu_synchronize")

    def frame(self):
        lib, ctx, ip, dp = self.lib, self.ctx, self.ip, self.dp
        self.ok(lib.ovgpu_set_features(ctx, C.byref(self.v.features)), "ovgpu_set_features")
        self.ok(lib.ovgpu_msckf_compress(ctx, ip(self.st), dp(self.x2), dp(self.thr), dp(self.pg), C.byref(self.D_out), C.byref(self.rows), ip(self.cols),
                                         dp(self.H), dp(self.r), C.byref(self.stats)), "ovgpu_msckf_compress")

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


LEGS = {"A": None, "A'": 0, "B": 1, "A2": None}


def make_legs(a, case, which=None):
    import torch  # noqa: F401  (capi.load: torch's HIP runtime first)
    from open_vins_amd import capi, synth
    lib, lib_a = capi.load(), (bind(capi, a.lib_a) if a.lib_a else None)
    which = which or [k for k in LEGS if (k != "A" or lib_a is not None) and (k != "A2" or (lib_a is not None and getattr(a, "control", False)))]
    if ("A" in which or "A2" in which) and lib_a is None:
        raise SystemExit("legs A and A2 need --lib-a")
    return {k: Leg(capi, synth, lib_a if k in ("A", "A2") else lib, case, k, LEGS[k]) for k in which}


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
        n_wide = B.counter(COUNTER)
        if n_wide == 0:
            raise RuntimeError(f"case {case}: leg B counted no {COUNTER} — nothing was compared")
        if A1.counter(COUNTER) != 0:
            raise RuntimeError(f"case {case}: leg A' took the wide route")
        for k, leg in legs.items():
            row = dict(case=case, leg=k, D=leg.D, F=int(leg.v.features.F), reps=a.reps, ms_round_medians=med[k], ms_median=float(np.median(med[k])),
                       ms_spread=float(np.max(med[k]) - np.min(med[k])), rows=int(leg.rows.value), n_used=int(leg.stats.n_used))
            if k in ("A'", "B"):
                row["last_factor_kernel"], row["last_unwhiten_kernel"] = leg.counter("last_factor_kernel"), leg.counter("last_unwhiten_kernel")
            rows.append(row)
            print(json.dumps(row), flush=True)
        m = {k: float(np.median(med[k])) for k in legs}
        spread = max(float(np.max(med[k]) - np.min(med[k])) for k in legs)
        (Ga, ga), (Gb, gb) = A1.gram(), B.gram()
        row = dict(case=case + "_summary", D=B.D, F=int(B.v.features.F), largest_spread_ms=spread, Aprime_minus_B_ms=m["A'"] - m["B"],
                   B_faster_than_Aprime_by_more_than_the_spread=bool(m["A'"] - m["B"] > spread), speedup_Aprime_over_B=m["A'"] / m["B"],
                   mode_a_wide_compressions_of_B=n_wide, HtH_rel_Aprime_to_B=float(np.linalg.norm(Ga - Gb) / max(np.linalg.norm(Gb), 1e-300)),
                   Htr_rel_Aprime_to_B=float(np.linalg.norm(ga - gb) / max(np.linalg.norm(gb), 1e-300)))
        if "A" in legs:
            row["Aprime_minus_A_ms"] = m["A'"] - m["A"]
            row["Aprime_equals_A_within_the_spread"] = bool(abs(m["A'"] - m["A"]) <= spread)
            row["A_and_Aprime_same_bits"] = bool(np.array_equal(legs["A"].H, A1.H) and np.array_equal(legs["A"].r, A1.r))
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
    n = leg.counter(COUNTER) if a.leg != "A" else 0
    if (n > 0) != (a.leg == "B"):
        raise RuntimeError(f"leg {a.leg} counted {n} {COUNTER}")
    print(f"{a.calls} frames of leg {a.leg}, case {a.case}, D = {leg.D}, F = {leg.v.features.F}, {n} {COUNTER}, rows {leg.rows.value}")
    leg.close()


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--reps", type=int, default=30)
    t.add_argument("--rounds", type=int, default=3)
    t.add_argument("--cases", default="modeA448,modeA448:100,modeA384,modeA510")
    t.add_argument("--lib-a", default=None)
    t.add_argument("--control", action="store_true")
    t.add_argument("--out", default=None)
    r = sub.add_parser("trace")
    r.add_argument("--case", default="modeA448")
    r.add_argument("--leg", choices=("A", "A'", "B"), default="B")
    r.add_argument("--calls", type=int, default=10)
    r.add_argument("--lib-a", default=None)
    a = ap.parse_args()
    {"time": timed, "trace": trace}[a.cmd](a)


if __name__ == "__main__":
    main()
