"""What the batched anchor change (ovgpu_slam_change_anchors_batched) is worth next to the per-landmark chain (ovgpu_slam_change_anchors), and
what the mode-A export (ovgpu_slam_anchor_systems) costs: an A/B of the entries of ONE build on one box.

    time [--reps 30] [--rounds 3] [--tag NAME] [--out FILE.jsonl]
                    50 anchored landmarks (the four anchored representations) on 30 clones, stereo, online calibration, N as it comes;
                    n = 1, 7, 25, 50 of them anchored in the clone that leaves.  Per call: the state and the landmarks are uploaded and the
                    stream drained (not timed), then the entry and the synchronisation that ends it are timed host to host (the export
                    synchronises itself).  The three entries take turns call by call, `rounds` repetitions of `reps` calls each; a row per
                    (n, entry) with the median of every round, the median of those and their spread (max - min): the yardstick for a
                    difference between two entries.
    trace [--n 50] [--calls 10] [--entry batched|sequential|export]
                    the calls alone, for a rocprofv3 --kernel-trace --stats run of its own (the kernel count per call)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ANCHORED = [2, 3, 4, 5]
L = 50


def problem(synth, n):
    """n of the 50 landmarks anchored in clone 0, the others spread over the clones that stay (the anchors are reassigned as
    tests/test_gpu_active_landmarks.py::test_change_anchors_with_120_landmarks reassigns them)"""
    reps = np.array((ANCHORED * ((L + 3) // 4))[:L], np.int32)
    prob = synth.make_slam_problem(2, L=L, lm_rep=reps, seed=3)
    move = np.round(np.linspace(0, L - 1, n)).astype(int)
    idx = np.arange(L)
    prob.lm_anchor_clone[:] = np.where(np.isin(idx, move), 0, 1 + idx % (prob.C - 2)).astype(np.int32)
    return prob


def entries(up, capi, prob):
    lib, ctx, new = up.lib, up._ctx, prob.C - 1
    n = C.c_int32(0)

    def sequential():
        capi.check(lib.ovgpu_slam_change_anchors(ctx, 0, new, C.byref(n)), "ovgpu_slam_change_anchors")
        capi.check(lib.ovgpu_synchronize(ctx), "ovgpu_synchronize")
        return n.value

    def batched():
        capi.check(lib.ovgpu_slam_change_anchors_batched(ctx, 0, new, C.byref(n)), "ovgpu_slam_change_anchors_batched")
        capi.check(lib.ovgpu_synchronize(ctx), "ovgpu_synchronize")
        return n.value

    def export():
        return len(up.anchor_systems(0, new))

    return dict(sequential=sequential, batched=batched, export=export)


def upload(up, capi, v):
    capi.check(up.lib.ovgpu_set_state(up._ctx, C.byref(v.state)), "ovgpu_set_state")
    capi.check(up.lib.ovgpu_set_landmarks(up._ctx, C.byref(v.landmarks)), "ovgpu_set_landmarks")
    capi.check(up.lib.ovgpu_set_active_landmarks(up._ctx, 0, None), "ovgpu_set_active_landmarks")
    capi.check(up.lib.ovgpu_synchronize(up._ctx), "ovgpu_synchronize")


def timed(a):
    import torch  # noqa: F401  (capi.load: torch's HIP runtime first)
    from open_vins_amd import capi, synth
    from open_vins_amd.updater import UpdaterMSCKF
    opts = capi.default_options(chi2_multipler=1.0)
    rows = []
    for n in (1, 7, 25, 50):
        prob = problem(synth, n)
        v = capi.Views(prob)
        up = UpdaterMSCKF(opts)
        up.N, up.Cn, up.K = v.state.N, v.state.C, v.state.K
        fns = entries(up, capi, prob)
        med = {k: [] for k in fns}
        for rnd in range(a.rounds):
            t = {k: [] for k in fns}
            for i in range(a.reps + 3):
                for name, fn in fns.items():  # interleaved call by call
                    upload(up, capi, v)
                    t0 = time.perf_counter()
                    moved = fn()
                    t1 = time.perf_counter()
                    assert moved == n
                    if i >= 3:
                        t[name].append((t1 - t0) * 1e3)
            for k in fns:
                med[k].append(float(np.median(t[k])))
        for k in fns:
            row = dict(case="change_anchors", entry=k, n_moving=n, L=L, N=int(prob.N), clones=int(prob.C), cameras=int(prob.K), build=a.tag, reps=a.reps,
                       ms_round_medians=med[k], ms_median=float(np.median(med[k])), ms_spread=float(np.max(med[k]) - np.min(med[k])))
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
    prob = problem(synth, a.n)
    v = capi.Views(prob)
    up = UpdaterMSCKF(capi.default_options(chi2_multipler=1.0))
    up.N, up.Cn, up.K = v.state.N, v.state.C, v.state.K
    fn = entries(up, capi, prob)[a.entry]
    for _ in range(a.calls):
        upload(up, capi, v)
        assert fn() == a.n
    up.close()
    print(f"{a.calls} calls of the {a.entry} entry, {a.n} moving landmarks each")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--reps", type=int, default=30)
    t.add_argument("--rounds", type=int, default=3)
    t.add_argument("--tag", default="tree")
    t.add_argument("--out", default=None)
    r = sub.add_parser("trace")
    r.add_argument("--n", type=int, default=50)
    r.add_argument("--calls", type=int, default=10)
    r.add_argument("--entry", choices=("batched", "sequential", "export"), default="batched")
    a = ap.parse_args()
    {"time": timed, "trace": trace}[a.cmd](a)


if __name__ == "__main__":
    main()
