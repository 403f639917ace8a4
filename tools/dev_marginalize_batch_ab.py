"""What the batched marginalisation (ovgpu_state_marginalize_batched) is worth next to the chain of single calls (ovgpu_state_marginalize, one
per block, highest id first): an A/B of the two entries of ONE build on one box.

    time [--reps 30] [--rounds 3] [--tag NAME] [--out FILE.jsonl]
                    the state of tools/dev_anchor_batch_ab.py (50 anchored landmarks of the four anchored representations on 30 clones, stereo,
                    online calibration, N = 350; no landmark anchored in clone 0, so that the oldest clone may leave).  Sets: n = 1, 5, 10, 25
                    landmarks, and 10 landmarks plus the oldest clone.  Per call: the state and the landmarks are uploaded and the stream
                    drained (not timed), then the entry and the synchronisation that ends it are timed host to host.  The two entries take
                    turns call by call, `rounds` repetitions of `reps` calls each; a row per (set, entry) with the median of every round, the
                    median of those and their spread (max - min): the yardstick for a difference between two entries.
    trace [--n 25] [--calls 10] [--entry batched|chain]
                    the calls alone, for a rocprofv3 --kernel-trace --stats run of its own (the kernel count per call)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dev_anchor_batch_ab import L, problem, upload  # noqa: E402  (the same state, the same untimed upload)


def blocks_of(prob, n, with_clone):
    """n landmarks spread over the 50 (ids of the covariance at entry), and the oldest clone"""
    reps = np.asarray(prob.lm_rep_each)
    ls = np.round(np.linspace(1, L - 2, n)).astype(int)
    b = [(int(prob.lm_cov_id[l]), 1 if reps[l] == 5 else 3) for l in ls]
    return b + ([(int(prob.clone_cov_id[0]), 6)] if with_clone else [])


def entries(up, capi, blocks):
    lib, ctx = up.lib, up._ctx
    desc = sorted(blocks, reverse=True)  # highest id first: the ids of the others are still the entry's
    ids, sz = np.array([b[0] for b in blocks], np.int32), np.array([b[1] for b in blocks], np.int32)
    pi, ps = ids.ctypes.data_as(capi.c_int32_p), sz.ctypes.data_as(capi.c_int32_p)

    def chain():
        for i, s in desc:
            capi.check(lib.ovgpu_state_marginalize(ctx, i, s), "ovgpu_state_marginalize")
        capi.check(lib.ovgpu_synchronize(ctx), "ovgpu_synchronize")

    def batched():
        capi.check(lib.ovgpu_state_marginalize_batched(ctx, len(blocks), pi, ps), "ovgpu_state_marginalize_batched")
        capi.check(lib.ovgpu_synchronize(ctx), "ovgpu_synchronize")

    return dict(chain=chain, batched=batched), (ids, sz)


def dims(up, capi):
    n, c = C.c_int32(0), C.c_int32(0)
    capi.check(up.lib.ovgpu_state_dims(up._ctx, C.byref(n), C.byref(c)), "ovgpu_state_dims")
    return n.value, c.value


def timed(a):
    import torch  # noqa: F401  (capi.load: torch's HIP runtime first)
    from open_vins_amd import capi, synth
    from open_vins_amd.updater import UpdaterMSCKF
    opts = capi.default_options(chi2_multipler=1.0)
    prob = problem(synth, 0)
    v = capi.Views(prob)
    rows = []
    for n, with_clone in ((1, False), (5, False), (10, False), (25, False), (10, True)):
        blocks = blocks_of(prob, n, with_clone)
        gone = sum(s for _, s in blocks)
        up = UpdaterMSCKF(opts)
        up.N, up.Cn, up.K = v.state.N, v.state.C, v.state.K
        fns, keep_alive = entries(up, capi, blocks)
        med = {k: [] for k in fns}
        for rnd in range(a.rounds):
            t = {k: [] for k in fns}
            for i in range(a.reps + 3):
                for name, fn in fns.items():  # interleaved call by call
                    upload(up, capi, v)
                    t0 = time.perf_counter()
                    fn()
                    t1 = time.perf_counter()
                    assert dims(up, capi) == (prob.N - gone, prob.C - int(with_clone))
                    if i >= 3:
                        t[name].append((t1 - t0) * 1e3)
            for k in fns:
                med[k].append(float(np.median(t[k])))
        for k in fns:
            row = dict(case="marginalize", entry=k, n_landmarks=n, oldest_clone=with_clone, blocks=len(blocks), rows_removed=gone, L=L, N=int(prob.N),
                       clones=int(prob.C), cameras=int(prob.K), build=a.tag, reps=a.reps, ms_round_medians=med[k], ms_median=float(np.median(med[k])),
                       ms_spread=float(np.max(med[k]) - np.min(med[k])))
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
    prob = problem(synth, 0)
    v = capi.Views(prob)
    up = UpdaterMSCKF(capi.default_options(chi2_multipler=1.0))
    up.N, up.Cn, up.K = v.state.N, v.state.C, v.state.K
    blocks = blocks_of(prob, a.n, False)
    fns, keep_alive = entries(up, capi, blocks)
    for _ in range(a.calls):
        upload(up, capi, v)
        fns[a.entry]()
    up.close()
    print(f"{a.calls} calls of the {a.entry} entry, {a.n} landmarks each")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--reps", type=int, default=30)
    t.add_argument("--rounds", type=int, default=3)
    t.add_argument("--tag", default="tree")
    t.add_argument("--out", default=None)
    r = sub.add_parser("trace")
    r.add_argument("--n", type=int, default=25)
    r.add_argument("--calls", type=int, default=10)
    r.add_argument("--entry", choices=("batched", "chain"), default="batched")
    a = ap.parse_args()
    {"time": timed, "trace": trace}[a.cmd](a)


if __name__ == "__main__":
    main()
