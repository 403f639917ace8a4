"""What one device pass over the chunks of a frame's SLAM update (ovgpu_slam_update_chunked) is worth next to the chain of single calls
(ovgpu_set_active_landmarks / ovgpu_set_features / ovgpu_slam_update per chunk): an A/B of the two forms of ONE build on one box.

    time [--reps 30] [--rounds 3] [--tag NAME] [--out FILE.jsonl]
                    30 clones, stereo, online calibration, landmarks of the six representations in turn; L = 50 and L = 100 resident landmarks;
                    batches of 25, 50 and 100 tracks (where L allows) in chunks of 25.  Per frame: the state and the landmarks are uploaded and
                    the stream drained (not timed); then, timed host to host, everything from the first call of the frame's SLAM update to the
                    synchronisation that ends it — the chain: per chunk its three calls, the last read-back ends it; the chunked entry:
                    ovgpu_set_features with the whole batch and the entry, whose one read-back ends it.  The two forms take turns frame by
                    frame, `rounds` repetitions of `reps` frames each; a row per (case, form) with the median of every round, the median of
                    those and their spread (max - min): the yardstick for a difference between the two.
    trace [--L 50] [--batch 50] [--calls 10] [--entry chunked|chain]
                    the frames alone, for a rocprofv3 --kernel-trace --stats run of its own (the kernel count per frame)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHUNK = 25
REPS6 = [0, 2, 0, 3, 1, 5]


def problem(synth, L, seed=3):
    return synth.make_slam_problem(2, L=L, lm_rep=np.array((REPS6 * ((L + 5) // 6))[:L], np.int32), seed=seed)


def forms(up, capi, prob, batch):
    """the two forms of one frame's SLAM update over the first `batch` tracks, as closures over prebuilt views (no marshalling inside the timed region)"""
    lib, ctx = up.lib, up._ctx
    N, L = prob.N, int(prob.lm_cov_id.shape[0])
    q = prob.subset(np.arange(batch))
    q.lm_index = np.arange(batch, dtype=np.int32)
    first = np.array(list(range(0, batch, CHUNK)) + [batch], np.int32)
    n = len(first) - 1
    whole = capi.Views(q)
    parts = []
    for k in range(n):
        qk = q.subset(np.arange(first[k], first[k + 1]))
        qk.lm_index = np.ascontiguousarray(q.lm_index[first[k]:first[k + 1]])
        parts.append((capi.Views(qk), np.unique(qk.lm_index).astype(np.int32), qk.lm_index))
    st, x2, thr = np.zeros(batch, np.int32), np.zeros(batch), np.zeros(batch)
    dx, P, lm = np.zeros((n, N)), np.zeros((N, N)), np.zeros((L, 3))
    ip = lambda a: a.ctypes.data_as(capi.c_int32_p)
    dp = lambda a: a.ctypes.data_as(capi.c_double_p)
    stats = (capi.UpdateStats * n)()
    used = {}

    def chain():
        tot = 0
        for k, (v, ids, lmi) in enumerate(parts):
            a = int(first[k])
            capi.check(lib.ovgpu_set_active_landmarks(ctx, int(ids.size), ip(ids)), "ovgpu_set_active_landmarks")
            capi.check(lib.ovgpu_set_features(ctx, C.byref(v.features)), "ovgpu_set_features")
            capi.check(lib.ovgpu_slam_update(ctx, ip(lmi), ip(st[a:]), dp(x2[a:]), dp(thr[a:]), dp(dx[k]), dp(P), dp(lm), C.byref(stats[k])), "ovgpu_slam_update")
            tot += stats[k].n_used
        used["chain"] = tot

    def chunked():
        capi.check(lib.ovgpu_set_features(ctx, C.byref(whole.features)), "ovgpu_set_features")
        capi.check(lib.ovgpu_slam_update_chunked(ctx, n, ip(first), ip(q.lm_index), ip(st), dp(x2), dp(thr), dp(dx), dp(P), dp(lm), stats), "ovgpu_slam_update_chunked")
        used["chunked"] = sum(s.n_used for s in stats)

    return dict(chain=chain, chunked=chunked), n, used, (whole, parts, q)


def upload(up, capi, v):
    """the frame's state and landmarks, and a drained stream: not timed"""
    capi.check(up.lib.ovgpu_set_state(up._ctx, C.byref(v.state)), "ovgpu_set_state")
    capi.check(up.lib.ovgpu_set_landmarks(up._ctx, C.byref(v.landmarks)), "ovgpu_set_landmarks")
    capi.check(up.lib.ovgpu_synchronize(up._ctx), "ovgpu_synchronize")


def timed(a):
    import torch  # noqa: F401  (capi.load: torch's HIP runtime first)
    from open_vins_amd import capi, synth
    from open_vins_amd.updater import UpdaterMSCKF
    opts = capi.default_options(chi2_multipler=1.0)
    rows = []
    for L in (50, 100):
        prob = problem(synth, L)
        v = capi.Views(prob)
        for batch in (25, 50, 100):
            if batch > L:
                continue
            up = UpdaterMSCKF(opts)
            fns, n, used, keep_alive = forms(up, capi, prob, batch)
            med = {k: [] for k in fns}
            for rnd in range(a.rounds):
                t = {k: [] for k in fns}
                for i in range(a.reps + 3):
                    for name, fn in fns.items():  # interleaved frame by frame
                        upload(up, capi, v)
                        t0 = time.perf_counter()
                        fn()
                        t1 = time.perf_counter()
                        if i >= 3:
                            t[name].append((t1 - t0) * 1e3)
                    assert used["chain"] == used["chunked"] > 0
                for k in fns:
                    med[k].append(float(np.median(t[k])))
            for k in fns:
                row = dict(case="slam_chunked", entry=k, L=L, batch=batch, chunks=n, chunk=CHUNK, n_used=int(used[k]), N=int(prob.N), clones=int(prob.C),
                           cameras=int(prob.K), build=a.tag, reps=a.reps, ms_round_medians=med[k], ms_median=float(np.median(med[k])),
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
    prob = problem(synth, a.L)
    v = capi.Views(prob)
    up = UpdaterMSCKF(capi.default_options(chi2_multipler=1.0))
    fns, n, used, keep_alive = forms(up, capi, prob, a.batch)
    for _ in range(a.calls):
        upload(up, capi, v)
        fns[a.entry]()
    up.close()
    print(f"{a.calls} frames of the {a.entry} form, {a.batch} tracks in {n} chunks, L = {a.L}")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("time")
    t.add_argument("--reps", type=int, default=30)
    t.add_argument("--rounds", type=int, default=3)
    t.add_argument("--tag", default="tree")
    t.add_argument("--out", default=None)
    r = sub.add_parser("trace")
    r.add_argument("--L", type=int, default=50)
    r.add_argument("--batch", type=int, default=50)
    r.add_argument("--calls", type=int, default=10)
    r.add_argument("--entry", choices=("chunked", "chain"), default="chunked")
    a = ap.parse_args()
    {"time": timed, "trace": trace}[a.cmd](a)


if __name__ == "__main__":
    main()
