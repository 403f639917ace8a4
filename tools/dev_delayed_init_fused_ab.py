"""What the fused step of the delayed initialisation (ovgpu_slam_delayed_init_fused, csrc/k_init_fused.h: five launches per candidate) is worth
next to the chain of single launches (ovgpu_slam_delayed_init): an A/B of the two entries of ONE build on one box, on the same seeded inputs.

    time [--reps 30] [--rounds 3] [--tag NAME] [--out FILE.jsonl]
                    DESIGN.md §2's rows: 30 clones, stereo, online calibration, L = 50 resident landmarks of the six representations in turn,
                    the empty active set, F = 1, 5 and 30 candidates initialised in those representations in turn.  Per frame, timed host to
                    host: ovgpu_set_state, ovgpu_set_landmarks, ovgpu_set_active_landmarks(0), ovgpu_set_features, ovgpu_set_feature_reps and
                    the entry, whose read-back ends it (the device triangulates).  The two entries take turns frame by frame, `rounds`
                    repetitions of `reps` frames each; a row per (case, entry) with the median of every round, the median of those and their
                    spread (max - min): the yardstick for a difference between the two.
    trace [--F 30] [--calls 10] [--entry fused|chain]
                    the frames alone, for a rocprofv3 --kernel-trace --stats run of its own (the kernels per candidate)"""
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


def problem(synth, F, seed=3):
    L = L_RESIDENT
    prob = synth.make_slam_problem(2, L=L, lm_rep=np.array((REPS6 * ((L + 5) // 6))[:L], np.int32), seed=seed)
    tracks = synth.make_problem(2, F=F, seed=seed, outlier_frac=0.2)
    for k in ("meas_offsets", "uv", "uvn", "clone_idx", "cam_idx", "p_FinG_true"):
        setattr(prob, k, getattr(tracks, k))
    return prob


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


def same(got):
    (n0, c0, v0), (n1, c1, v1) = got["chain"], got["fused"]
    acc = c0 >= 0
    return n0 == n1 and np.array_equal(c0, c1) and np.allclose(v0[acc], v1[acc], rtol=1e-8, atol=1e-10)


def timed(a):
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
    prob = problem(synth, a.F)
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
    r = sub.add_parser("trace")
    r.add_argument("--F", type=int, default=30)
    r.add_argument("--calls", type=int, default=10)
    r.add_argument("--entry", choices=("fused", "chain"), default="fused")
    a = ap.parse_args()
    {"time": timed, "trace": trace}[a.cmd](a)


if __name__ == "__main__":
    main()
