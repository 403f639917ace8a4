"""What the panelled pivoted factor is worth to mode A at 256 .. 383 Jacobian columns (ovgpu_debug_option "mode_a_panel"): the legs on one MI355X,
after tools/dev_slam_mode_a_ab.py.

    time [--reps 30] [--rounds 3] [--lib-a PATH] [--control] [--cases slam283,slam358,msckf236,msckf356,msckf224,msckf254] [--out FILE.jsonl]
                    leg A   runs on the library --lib-a names (the parent commit's build, which does not know the switch); without --lib-a it is left out
                    leg A'  on the tree's library with "mode_a_panel" = 0 (the rank-one k_gram_pchol<NB>, as the parent takes it)
                    leg B1  on the tree's library with "mode_a_panel" = 1 (k_pchol_panel / k_pchol_schur)
                    (profiles/r33_mode_a_panel_ab.jsonl also holds a leg B2: level 2 of the attempt DESIGN.md section 7 describes, which is not in the tree)
                    leg A2  (--control) a SECOND context on leg A's library, behind the others in every frame: what two contexts of one build differ by
                    One context per leg.  The legs take turns frame by frame, `rounds` rounds of `reps` frames (three more warm each round up); a row per
                    (case, leg) with the median of every round, the median of those and their spread (max - min), and a summary row per case:
                    A' - A against the larger of the spread and |A2 - A|, A' - B1 against the largest spread.  Below the route's lower edge (224
                    and 254 columns) leg B1 runs what leg A' runs; from the edge on a leg B1 that counted no "mode_a_panel_compressions" is an
                    error, not a row.
                    Cases, timed host to host from ovgpu_set_features (the state and landmark upload is not timed):
                      slam283 / slam358   ovgpu_slam_compress, 30 clones x 2 cameras with full calibration and 25 / 50 3-dof landmarks, every one observed;
                                          "slam_mode_a" = 1 and "slam_fused" = 3 on EVERY leg
                      msckf236 / msckf356 ovgpu_msckf_compress at BASELINE configs[3] / configs[4] (30 / 50 clones x 4 cameras), 800 features
                      msckf224 / msckf254 ... at 28 / 33 clones x 4 cameras: 15 and 16 tile columns, below the route's lower edge of 17
    trace [--case slam358] [--leg B1] [--calls 10] [--lib-a PATH]
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

COUNTER = "mode_a_panel_compressions"
SLAM_CASES = {"slam283": 25, "slam358": 50}                                                           # 3-dof landmarks, every one in the batch
MSCKF_CASES = {"msckf236": dict(cfg=4), "msckf356": dict(cfg=5), "msckf224": dict(cfg=2, C=28, K=4), "msckf254": dict(cfg=2, C=33, K=4)}  # (synth.CONFIGS counts from 1)
MSCKF_F = 800
LEGS = {"A": None, "A'": 0, "B1": 1, "A2": None}
EDGE_D = 256  # the route's lower edge in Jacobian columns (17 tile columns of [H | r])


class Leg:
    """one context and its frame: prepare() is not timed, frame() is"""

    def __init__(self, capi, synth, lib, case, kind, level):
        """level: 0 / 1 sets "mode_a_panel" (the tree's library), None leaves the name alone (another build, which does not know it)"""
        self.lib, self.kind, self.case, self.ctx, self.slam = lib, kind, case, C.c_void_p(), case in SLAM_CASES
        ip, dp, st = capi.c_int32_p, capi.c_double_p, C.POINTER(capi.UpdateStats)
        lib.ovgpu_slam_compress.argtypes = [C.c_void_p, ip, ip, dp, dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), ip, dp, dp, st]
        lib.ovgpu_msckf_compress.argtypes = [C.c_void_p, ip, dp, dp, dp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), ip, dp, dp, st]
        lib.ovgpu_slam_compress.restype = lib.ovgpu_msckf_compress.restype = C.c_int
        opts = capi.default_options(chi2_multipler=1.0)
        assert lib.ovgpu_create(C.byref(opts), 0, C.byref(self.ctx)) == 0
        if level is not None:
            self.ok(lib.ovgpu_debug_option(self.ctx, b"mode_a_panel", int(level), None), "ovgpu_debug_option")
        self.ip = lambda a: a.ctypes.data_as(ip)
        self.dp = lambda a: a.ctypes.data_as(dp)
        if self.slam:
            for name, val in ((b"slam_mode_a", 1), (b"slam_fused", 3)):  # (every leg: the parent's build knows both)
                self.ok(lib.ovgpu_debug_option(self.ctx, name, val, None), "ovgpu_debug_option")
            L = SLAM_CASES[case]
            r5 = [capi.REP_GLOBAL_3D, capi.REP_ANCHORED_3D, capi.REP_GLOBAL_FULL_INVERSE_DEPTH, capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, capi.REP_ANCHORED_FULL_INVERSE_DEPTH]
            reps = np.array((r5 * (L // 5 + 1))[:L], np.int32)
            self.D = 208 + 3 * L
            prob = synth.make_slam_problem(2, L=L, lm_rep=reps, seed=3).subset(np.arange(L))
            prob.lm_index = np.ascontiguousarray(np.arange(L), dtype=np.int32)
            self.lm = prob.lm_index
        else:
            kw = dict(MSCKF_CASES[case])
            prob = synth.make_problem(kw.pop("cfg"), F=MSCKF_F, seed=5, **kw)
            self.D = prob.Dmax
        assert self.D == int(case[-3:]), (case, self.D)
        F = prob.F
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
        if self.slam:
            self.ok(self.lib.ovgpu_set_landmarks(self.ctx, C.byref(self.v.landmarks)), "ovgpu_set_landmarks")
        self.ok(self.lib.ovgpu_synchronize(self.ctx), "ovgpu_synchronize")

    def frame(self):
        lib, ctx, ip, dp = self.lib, self.ctx, self.ip, self.dp
        self.ok(lib.ovgpu_set_features(ctx, C.byref(self.v.features)), "ovgpu_set_features")
        if self.slam:
            self.ok(lib.ovgpu_slam_compress(ctx, ip(self.lm), ip(self.st), dp(self.x2), dp(self.thr), C.byref(self.D_out), C.byref(self.rows), ip(self.cols),
                                            dp(self.H), dp(self.r), C.byref(self.stats)), "ovgpu_slam_compress")
        else:
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


def make_legs(a, case, which=None):
    import torch  # noqa: F401  (capi.load: torch's HIP runtime first)
    from open_vins_amd import capi, synth
    lib, lib_a = capi.load(), (bind(capi, a.lib_a) if a.lib_a else None)
    which = which or [k for k in LEGS if (k != "A" or lib_a is not None) and (k != "A2" or (lib_a is not None and getattr(a, "control", False)))]
    if ("A" in which or "A2" in which) and lib_a is None:
        raise SystemExit("legs A and A2 need --lib-a")
    return {k: Leg(capi, synth, lib_a if k in ("A", "A2") else lib, case, k, LEGS[k]) for k in which}


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


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
        A1, B1 = legs["A'"], legs["B1"]
        if (B1.counter(COUNTER) > 0) != (B1.D >= EDGE_D):
            raise RuntimeError(f"case {case}: leg B1 counted {B1.counter(COUNTER)} {COUNTER} at {B1.D} columns")
        if A1.counter(COUNTER) != 0:
            raise RuntimeError(f"case {case}: leg A' took the panelled factor")
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
        (Ga, ga), (Gb, gb) = A1.gram(), B1.gram()
        row = dict(case=case + "_summary", D=B1.D, F=int(B1.v.features.F), largest_spread_ms=spread,
                   Aprime_minus_B1_ms=m["A'"] - m["B1"], B1_faster_than_Aprime_by_more_than_the_spread=bool(m["A'"] - m["B1"] > spread), speedup_Aprime_over_B1=m["A'"] / m["B1"],
                   B1_and_Aprime_same_bits=bool(np.array_equal(B1.H, A1.H) and np.array_equal(B1.r, A1.r) and B1.rows.value == A1.rows.value),
                   rows_Aprime=int(A1.rows.value), rows_B1=int(B1.rows.value), HtH_rel_Aprime_to_B1=_rel(Ga, Gb), Htr_rel_Aprime_to_B1=_rel(ga, gb))
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
    if (n > 0) != (a.leg == "B1" and leg.D >= EDGE_D):
        raise RuntimeError(f"leg {a.leg} counted {n} {COUNTER}")
    print(f"{a.calls} frames of leg {a.leg}, case {a.case}, D = {leg.D}, F = {leg.v.features.F}, {n} {COUNTER}, rows {leg.rows.value}")
    leg.close()


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--reps", type=int, default=30)
    t.add_argument("--rounds", type=int, default=3)
    t.add_argument("--cases", default="slam283,slam358,msckf236,msckf356,msckf224,msckf254")
    t.add_argument("--lib-a", default=None)
    t.add_argument("--control", action="store_true")
    t.add_argument("--out", default=None)
    r = sub.add_parser("trace")
    r.add_argument("--case", default="slam358")
    r.add_argument("--leg", choices=tuple(LEGS), default="B1")
    r.add_argument("--calls", type=int, default=10)
    r.add_argument("--lib-a", default=None)
    a = ap.parse_args()
    {"time": timed, "trace": trace}[a.cmd](a)


if __name__ == "__main__":
    main()
