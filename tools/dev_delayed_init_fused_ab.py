"""What the fused step of the delayed initialisation (ovgpu_slam_delayed_init_fused, csrc/k_init_fused.h: five launches per candidate) is worth
next to the chain of single launches (ovgpu_slam_delayed_init): an A/B of the two entries of ONE build on one box, on the same seeded inputs.

    time [--reps 30] [--rounds 3] [--tag NAME] [--out FILE.jsonl]
                    DESIGN.md §2's rows: 30 clones, stereo, online calibration, L = 50 resident landmarks of the six representations in turn,
                    the empty active set, F = 1, 5 and 30 candidates initialised in those representations in turn.  Per frame, timed host to
                    host: ovgpu_set_state, ovgpu_set_landmarks, ovgpu_set_active_landmarks(0), ovgpu_set_features, ovgpu_set_feature_reps and
                    the entry, whose read-back ends it (the device triangulates).  The two entries take turns frame by frame, `rounds`
                    repetitions of `reps` frames each; a row per (case, entry) with the median of every round, the median of those and their
                    spread (max - min): the yardstick for a difference between the two.
    time --legs [--lib-a PATH] [--level-a 1] [--level-b 2] [--tag-a NAME] [--outlier-frac 0.2]
                    three legs of the FUSED entry, interleaved frame by frame on the same inputs: A on the library --lib-a names (the parent
                    commit's build, its options untouched; without --lib-a: the tree's), A' on the tree's with "delayed_init_fused" = --level-a,
                    B on the tree's with "delayed_init_fused" = --level-b (the switch is a level: 1 the step behind k_system_t's gate, 2 behind
                    k_init_rows with the gate in the tail).  A row per (F, leg); bits_equal_A: the leg's N, covariance ids, values, dx_seq and P
                    are leg A's bit for bit.  --outlier-frac 1: every candidate a gross outlier (the all-rejected frame).
    time --long [--clones 30 50]
                    the long-track rows of "delayed_init_fused_long" (tracks of 65 .. 232 measurements on the fused step): `clones` x 4 cameras with
                    online calibration, no resident landmarks, F = 1, 5 and 30 candidates at the window's full length (120 / 200 measurements,
                    GLOBAL_3D), three legs of the fused entry on the tree's library, interleaved frame by frame on the same inputs: "off-1" the
                    switch off at level 1 (every candidate on the chain's step), "on-1" the switch on at level 1, "on-2" the switch on at level 2.
                    A row per (clones, F, leg); the on legs are held to the off leg within the bounds of tests/test_gpu_delayed_init_fused.py's
                    _check (verdicts identical, values 1e-8 / 1e-10, dx_seq 1e-6, P 1e-7) before their row is written.
    trace [--F 30] [--calls 10] [--entry fused|chain] [--lib-a PATH] [--level N] [--long CLONES]
                    the frames alone, for a rocprofv3 --kernel-trace --stats run of its own (the kernels per candidate); --lib-a: on that
                    library; --level: "delayed_init_fused" set to it first; --long CLONES: the long-track frame of `time --long` at that many
                    clones with the switch on (--F 1: the per-kernel times of ONE long candidate)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPS6 = [0, 2, 0, 3, 1, 5]
L_RESIDENT = 50


def problem(synth, F, seed=3, outlier_frac=0.2):
    L = L_RESIDENT
    prob = synth.make_slam_problem(2, L=L, lm_rep=np.array((REPS6 * ((L + 5) // 6))[:L], np.int32), seed=seed)
    tracks = synth.make_problem(2, F=F, seed=seed, outlier_frac=outlier_frac)
    for k in ("meas_offsets", "uv", "uvn", "clone_idx", "cam_idx", "p_FinG_true"):
        setattr(prob, k, getattr(tracks, k))
    return prob


def problem_long(synth, C, F, seed=3):
    """F candidates at the full length of the C x 4 window (the longest F of 4 F: C * 4 measurements each where the point is seen throughout),
    online calibration, no resident landmarks, no planted outliers"""
    prob = synth.make_problem(2, C=C, K=4, F=4 * F, seed=seed)
    m = np.diff(prob.meas_offsets)
    return prob.subset(np.sort(np.argsort(-m, kind="stable")[:F]))


def forms(up, capi, prob):
    """one frame through either entry, as closures over prebuilt views (no marshalling inside the timed region)"""
    lib, ctx = up.lib, up._ctx
    v = capi.Views(prob)
    F, N = v.features.F, prob.N
    reps = np.array((REPS6 * ((F + 5) // 6))[:F], np.int32)
    Nmax = N + int(np.where(reps == capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE, 1, 3).sum())
    st, cov = np.zeros(F, np.int32), np.zeros(F, np.int32)
    val, fej, dx, P = np.zeros((F, 3)), np.zeros((F, 3)), np.zeros((F, Nmax)), np.zeros(Nmax * Nmax)
    ip = lambda a: a.ctypes.data_as(capi.c_int32_p)
    dp = lambda a: a.ctypes.data_as(capi.c_double_p)
    N_out, stats = C.c_int32(0), capi.UpdateStats()
    got = {}

    def frame(name, key):
        entry = getattr(lib, name)

        def run():
            capi.check(lib.ovgpu_set_state(ctx, C.byref(v.state)), "ovgpu_set_state")
            capi.check(lib.ovgpu_set_landmarks(ctx, C.byref(v.landmarks)), "ovgpu_set_landmarks")
            capi.check(lib.ovgpu_set_active_landmarks(ctx, 0, None), "ovgpu_set_active_landmarks")
            capi.check(lib.ovgpu_set_features(ctx, C.byref(v.features)), "ovgpu_set_features")
            capi.check(lib.ovgpu_set_feature_reps(ctx, ip(reps)), "ovgpu_set_feature_reps")
            capi.check(entry(ctx, 0, ip(st), None, None, ip(cov), dp(val), dp(fej), None, None, dp(dx), C.byref(N_out), dp(P), C.byref(stats)), name)
            got[key] = (N_out.value, cov.copy(), val.copy())
        return run

    return dict(chain=frame("ovgpu_slam_delayed_init", "chain"), fused=frame("ovgpu_slam_delayed_init_fused", "fused")), got, v


def bind(capi, path):
    """a library by path with the entries a leg calls (another build: it may not know this tree's option names)"""
    if path is None:
        return capi.load()
    lib = C.CDLL(os.path.abspath(path))
    ip, dp, ctx, st = capi.c_int32_p, capi.c_double_p, C.c_void_p, C.POINTER(capi.UpdateStats)
    sig = {"ovgpu_create": [C.POINTER(capi.Options), C.c_int, C.POINTER(ctx)], "ovgpu_destroy": [ctx], "ovgpu_set_state": [ctx, C.POINTER(capi.StateView)],
           "ovgpu_set_landmarks": [ctx, C.POINTER(capi.LandmarksView)], "ovgpu_set_active_landmarks": [ctx, C.c_int32, ip],
           "ovgpu_set_features": [ctx, C.POINTER(capi.FeaturesView)], "ovgpu_set_feature_reps": [ctx, ip], "ovgpu_synchronize": [ctx],
           "ovgpu_slam_delayed_init_fused": [ctx, C.c_int32, ip, dp, dp, ip, dp, dp, ip, ip, dp, ip, dp, st],
           "ovgpu_debug_option": [ctx, C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]}
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, (None if name == "ovgpu_destroy" else C.c_int)
    lib.ovgpu_last_error.restype = C.c_char_p
    return lib


class Leg:
    """one context of `lib` and its frame through the fused entry; level: "delayed_init_fused" is set to it, None leaves the library alone"""

    def __init__(self, capi, lib, prob, kind, level, debug=None, reps=None):
        self.capi, self.lib, self.kind, self.level, self.ctx = capi, lib, kind, level, C.c_void_p()
        opts = capi.default_options(chi2_multipler=1.0)
        self.ok(lib.ovgpu_create(C.byref(opts), 0, C.byref(self.ctx)), "ovgpu_create")
        if level is not None:
            self.ok(lib.ovgpu_debug_option(self.ctx, b"delayed_init_fused", int(level), None), "ovgpu_debug_option")
        for name, value in (debug or {}).items():  # further options of the tree's library
            self.ok(lib.ovgpu_debug_option(self.ctx, name.encode(), int(value), None), "ovgpu_debug_option")
        self.v = capi.Views(prob)
        F, N = self.v.features.F, prob.N
        self.reps = np.array((REPS6 * ((F + 5) // 6))[:F], np.int32) if reps is None else np.full(F, reps, np.int32)
        Nmax = N + int(np.where(self.reps == capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE, 1, 3).sum())
        self.st, self.cov = np.zeros(F, np.int32), np.zeros(F, np.int32)
        self.val, self.fej, self.dx, self.P = np.zeros((F, 3)), np.zeros((F, 3)), np.zeros((F, Nmax)), np.zeros(Nmax * Nmax)
        self.N_out, self.stats = C.c_int32(0), capi.UpdateStats()

    def ok(self, rc, where):
        if rc != 0:
            raise RuntimeError(f"leg {self.kind}: {where} returned {rc}: {self.lib.ovgpu_last_error()}")

    def frame(self):
        lib, ctx, v = self.lib, self.ctx, self.v
        ip = lambda a: a.ctypes.data_as(self.capi.c_int32_p)
        dp = lambda a: a.ctypes.data_as(self.capi.c_double_p)
        self.ok(lib.ovgpu_set_state(ctx, C.byref(v.state)), "ovgpu_set_state")
        if v.landmarks is not None:  # (the long-track rows have no resident landmarks)
            self.ok(lib.ovgpu_set_landmarks(ctx, C.byref(v.landmarks)), "ovgpu_set_landmarks")
            self.ok(lib.ovgpu_set_active_landmarks(ctx, 0, None), "ovgpu_set_active_landmarks")
        self.ok(lib.ovgpu_set_features(ctx, C.byref(v.features)), "ovgpu_set_features")
        self.ok(lib.ovgpu_set_feature_reps(ctx, ip(self.reps)), "ovgpu_set_feature_reps")
        self.ok(lib.ovgpu_slam_delayed_init_fused(ctx, 0, ip(self.st), None, None, ip(self.cov), dp(self.val), dp(self.fej), None, None, dp(self.dx),
                                                  C.byref(self.N_out), dp(self.P), C.byref(self.stats)), "ovgpu_slam_delayed_init_fused")

    def outputs(self):
        n = self.N_out.value
        return n, self.st.copy(), self.cov.copy(), self.val.copy(), self.dx.copy(), self.P[: n * n].copy()

    def counter(self, name):
        if self.level is None:
            return -1
        n = C.c_int64(0)
        self.ok(self.lib.ovgpu_debug_option(self.ctx, name.encode(), -1, C.byref(n)), "ovgpu_debug_option")
        return int(n.value)

    def close(self):
        self.lib.ovgpu_destroy(self.ctx)


def bits_equal(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[1:], b[1:]))


def timed_legs(a):
    import torch  # noqa: F401  (capi.load: torch's HIP runtime first)
    from open_vins_amd import capi, synth
    lib, lib_a = capi.load(), bind(capi, a.lib_a)
    rows = []
    for F in (1, 5, 30):
        prob = problem(synth, F, outlier_frac=a.outlier_frac)
        legs = {"A": Leg(capi, lib_a, prob, "A", None), "A'": Leg(capi, lib, prob, "A'", a.level_a), "B": Leg(capi, lib, prob, "B", a.level_b)}
        med = {k: [] for k in legs}
        for rnd in range(a.rounds):
            t = {k: [] for k in legs}
            for i in range(a.reps + 3):
                for k, leg in legs.items():  # interleaved frame by frame
                    leg.ok(leg.lib.ovgpu_synchronize(leg.ctx), "ovgpu_synchronize")
                    t0 = time.perf_counter()
                    leg.frame()
                    t1 = time.perf_counter()
                    if i >= 3:
                        t[k].append((t1 - t0) * 1e3)
            for k in legs:
                med[k].append(float(np.median(t[k])))
        ref = legs["A"].outputs()
        for k, leg in legs.items():
            o = leg.outputs()
            assert o[0] == ref[0] and np.array_equal(o[1], ref[1]) and np.array_equal(o[2], ref[2]), f"leg {k}: verdicts differ from leg A's"
            row = dict(case="delayed_init_gate", leg=k, level=leg.level, F=F, L=L_RESIDENT, outlier_frac=a.outlier_frac, n_accepted=int((o[2] >= 0).sum()),
                       n_rejected=int((o[1] == capi.FEAT_CHI2_REJECTED).sum()), N=int(prob.N), N_out=int(o[0]), clones=int(prob.C), cameras=int(prob.K),
                       build=(a.tag_a if k == "A" else a.tag), reps=a.reps, ms_round_medians=med[k], ms_median=float(np.median(med[k])),
                       ms_spread=float(np.max(med[k]) - np.min(med[k])), bits_equal_A=bool(bits_equal(o, ref)),
                       fused_steps=leg.counter("delayed_init_fused_steps"), rows_steps=(leg.counter("delayed_init_rows_steps") if k != "A" or a.lib_a is None else -1))
            rows.append(row)
            print(json.dumps(row), flush=True)
        for leg in legs.values():
            leg.close()
    if a.out:
        with open(a.out, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


LONG_LEGS = (("off-1", 1, 0), ("on-1", 1, 1), ("on-2", 2, 1))  # (leg, "delayed_init_fused", "delayed_init_fused_long")


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def timed_long(a):
    import torch  # noqa: F401  (capi.load: torch's HIP runtime first)
    from open_vins_amd import capi, synth
    lib = capi.load()
    rows = []
    for C_ in a.clones:
        for F in (1, 5, 30):
            prob = problem_long(synth, C_, F)
            m = np.diff(prob.meas_offsets)
            legs = {k: Leg(capi, lib, prob, k, level, debug={"delayed_init_fused_long": on}, reps=capi.REP_GLOBAL_3D) for k, level, on in LONG_LEGS}
            med = {k: [] for k in legs}
            for rnd in range(a.rounds):
                t = {k: [] for k in legs}
                for i in range(a.reps + 3):
                    for k, leg in legs.items():  # interleaved frame by frame
                        leg.ok(leg.lib.ovgpu_synchronize(leg.ctx), "ovgpu_synchronize")
                        t0 = time.perf_counter()
                        leg.frame()
                        t1 = time.perf_counter()
                        if i >= 3:
                            t[k].append((t1 - t0) * 1e3)
                for k in legs:
                    med[k].append(float(np.median(t[k])))
            ref = legs["off-1"].outputs()
            calls = a.rounds * (a.reps + 3)
            for k, leg in legs.items():
                o = leg.outputs()
                acc = ref[2] >= 0
                d_val = float(np.abs(o[3][acc] - ref[3][acc]).max(initial=0.0))
                d_dx, d_P = rel(o[4], ref[4]), rel(o[5], ref[5])
                # the on legs against the off leg, within the bounds of tests/test_gpu_delayed_init_fused.py::_check
                assert o[0] == ref[0] and np.array_equal(o[1], ref[1]) and np.array_equal(o[2], ref[2]), f"leg {k}: verdicts differ from the off leg's"
                assert np.allclose(o[3][acc], ref[3][acc], rtol=1e-8, atol=1e-10) and d_dx < 1e-6 and d_P < 1e-7, f"leg {k}: {d_val} {d_dx} {d_P}"
                row = dict(case="delayed_init_long", leg=k, level=leg.level, long=int(k != "off-1"), F=F, L=0, clones=int(prob.C), cameras=int(prob.K),
                           m_min=int(m.min()), m_max=int(m.max()), N=int(prob.N), N_out=int(o[0]), n_accepted=int(acc.sum()),
                           n_rejected=int((o[1] == capi.FEAT_CHI2_REJECTED).sum()), build=a.tag, reps=a.reps, ms_round_medians=med[k],
                           ms_median=float(np.median(med[k])), ms_spread=float(np.max(med[k]) - np.min(med[k])),
                           fused_steps_per_call=leg.counter("delayed_init_fused_steps") / calls, long_steps_per_call=leg.counter("delayed_init_long_steps") / calls,
                           chain_steps_per_call=leg.counter("delayed_init_chain_steps") / calls, d_values_off=d_val, d_dx_seq_off=d_dx, d_P_off=d_P)
                rows.append(row)
                print(json.dumps(row), flush=True)
            for leg in legs.values():
                leg.close()
    if a.out:
        with open(a.out, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


def same(got):
    (n0, c0, v0), (n1, c1, v1) = got["chain"], got["fused"]
    acc = c0 >= 0
    return n0 == n1 and np.array_equal(c0, c1) and np.allclose(v0[acc], v1[acc], rtol=1e-8, atol=1e-10)


def timed(a):
    if a.long:
        return timed_long(a)
    if a.legs:
        return timed_legs(a)
    import torch  # noqa: F401  (capi.load: torch's HIP runtime first)
    from open_vins_amd import capi, synth
    from open_vins_amd.updater import UpdaterMSCKF
    opts = capi.default_options(chi2_multipler=1.0)
    rows = []
    for F in (1, 5, 30):
        prob = problem(synth, F)
        up = UpdaterMSCKF(opts)
        fns, got, keep_alive = forms(up, capi, prob)
        med = {k: [] for k in fns}
        for rnd in range(a.rounds):
            t = {k: [] for k in fns}
            for i in range(a.reps + 3):
                for name, fn in fns.items():  # interleaved frame by frame
                    capi.check(up.lib.ovgpu_synchronize(up._ctx), "ovgpu_synchronize")
                    t0 = time.perf_counter()
                    fn()
                    t1 = time.perf_counter()
                    if i >= 3:
                        t[name].append((t1 - t0) * 1e3)
                assert same(got)
            for k in fns:
                med[k].append(float(np.median(t[k])))
        steps = (up.debug_option("delayed_init_fused_steps"), up.debug_option("delayed_init_chain_steps"))
        for k in fns:
            row = dict(case="delayed_init_fused", entry=k, F=F, L=L_RESIDENT, n_accepted=int((got[k][1] >= 0).sum()), N=int(prob.N), N_out=int(got[k][0]),
                       clones=int(prob.C), cameras=int(prob.K), build=a.tag, reps=a.reps, ms_round_medians=med[k], ms_median=float(np.median(med[k])),
                       ms_spread=float(np.max(med[k]) - np.min(med[k])), fused_steps=int(steps[0]), chain_steps=int(steps[1]))
            rows.append(row)
            print(json.dumps(row), flush=True)
        up.close()
    if a.out:
        with open(a.out, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


def trace(a):
    import torch  # noqa: F401
    from open_vins_amd import capi, synth
    from open_vins_amd.updater import UpdaterMSCKF
    if a.long is not None:  # the long-track frame with the switch on, at --level (default 1)
        prob = problem_long(synth, a.long, a.F)
        level = 1 if a.level is None else a.level
        leg = Leg(capi, capi.load(), prob, "trace", level, debug={"delayed_init_fused_long": 1}, reps=capi.REP_GLOBAL_3D)
        for _ in range(a.calls):
            leg.frame()
        o = leg.outputs()
        n_long = leg.counter("delayed_init_long_steps")
        leg.close()
        print(f"{a.calls} frames of the fused entry with the long bound at level {level}: {a.long} clones x 4 cameras, {a.F} candidates of "
              f"{int(np.diff(prob.meas_offsets).min())} .. {int(np.diff(prob.meas_offsets).max())} measurements ({int((o[2] >= 0).sum())} accepted), {n_long} long steps")
        return
    prob = problem(synth, a.F, outlier_frac=a.outlier_frac)
    if a.lib_a is not None or a.level is not None:  # the fused entry on a library by path and / or at a level
        leg = Leg(capi, bind(capi, a.lib_a), prob, "trace", a.level)
        for _ in range(a.calls):
            leg.frame()
        o = leg.outputs()
        leg.close()
        print(f"{a.calls} frames of the fused entry (library {a.lib_a or 'of the tree'}, level {a.level}), {a.F} candidates ({int((o[2] >= 0).sum())} accepted), L = {L_RESIDENT}")
        return
    up = UpdaterMSCKF(capi.default_options(chi2_multipler=1.0))
    fns, got, keep_alive = forms(up, capi, prob)
    for _ in range(a.calls):
        fns[a.entry]()
    up.close()
    print(f"{a.calls} frames of the {a.entry} entry, {a.F} candidates ({int((got[a.entry][1] >= 0).sum())} accepted), L = {L_RESIDENT}")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--reps", type=int, default=30)
    t.add_argument("--rounds", type=int, default=3)
    t.add_argument("--tag", default="tree")
    t.add_argument("--out", default=None)
    t.add_argument("--legs", action="store_true")
    t.add_argument("--lib-a", default=None)
    t.add_argument("--tag-a", default="parent")
    t.add_argument("--level-a", type=int, default=1)
    t.add_argument("--level-b", type=int, default=2)
    t.add_argument("--outlier-frac", type=float, default=0.2)
    t.add_argument("--long", action="store_true")
    t.add_argument("--clones", type=int, nargs="+", default=[30, 50])
    r = sub.add_parser("trace")
    r.add_argument("--F", type=int, default=30)
    r.add_argument("--calls", type=int, default=10)
    r.add_argument("--entry", choices=("fused", "chain"), default="fused")
    r.add_argument("--lib-a", default=None)
    r.add_argument("--level", type=int, default=None)
    r.add_argument("--outlier-frac", type=float, default=0.2)
    r.add_argument("--long", type=int, default=None)
    a = ap.parse_args()
    {"time": timed, "trace": trace}[a.cmd](a)


if __name__ == "__main__":
    main()
