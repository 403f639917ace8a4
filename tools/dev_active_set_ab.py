"""What the active landmark set (ovgpu_set_active_landmarks) is worth, and that the default path is untouched: an A/B of two builds of
libovgpu.so on one box.

    dump OUT.npz [--lib FILE]       every output of ovgpu_slam_update (L = 40: a batch of 25 and a batch of all 40) and of
                                    ovgpu_slam_delayed_init (L = 40, 30 candidates) WITHOUT a named set, through the library FILE (default:
                                    the tree's)
    compare A.npz B.npz             bit for bit, as tools/dev_bitcompare.py does
    time --variant all|active [--lib FILE] [--tag NAME] [--reps 30] [--out FILE.jsonl]
                                    ovgpu_slam_update with a batch of 25 at L = 50 and L = 100 resident landmarks, and the 30-candidate chain of
                                    ovgpu_slam_delayed_init at L = 50 (30 clones, stereo, online calibration, landmarks of mixed
                                    representations).  `frame` is host to host from ovgpu_set_state to the end of the SLAM call (what a filter
                                    pays per frame: the uploads, the set, the call and its one synchronisation), `call` the SLAM call alone,
                                    `device` ovgpu_update_stats::ms_total, `kernel` ovgpu_kernel_times (compress + update).  One process per
                                    (build, variant); the caller interleaves the processes and repeats them: the spread between the
                                    repetitions of one configuration is the yardstick for a difference between two.

A library without the entry (the parent build) runs `all` only."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPS6 = [0, 2, 0, 4, 1, 5]  # global, anchored 3d, global, anchored MSCKF inverse depth, global full inverse depth, single depth


def load(path):
    import torch  # noqa: F401  (capi.load: torch's HIP runtime first)
    from open_vins_amd import capi
    if path:
        lib = C.CDLL(os.path.abspath(path))
        if not hasattr(lib, "ovgpu_set_active_landmarks"):
            lib.ovgpu_set_active_landmarks = lib["ovgpu_abi_version"]  # never called: keeps capi.declare whole
        capi.declare(lib)
        capi._lib = lib
    return capi


def slam_problem(synth, L, seed, candidates=0):
    reps = np.array((REPS6 * ((L + 5) // 6))[:L], np.int32)
    prob = synth.make_slam_problem(2, L=L, lm_rep=reps, seed=seed)
    if candidates:
        tracks = synth.make_problem(2, F=candidates, seed=seed, outlier_frac=0.2)
        for k in ("meas_offsets", "uv", "uvn", "clone_idx", "cam_idx", "p_FinG_true"):
            setattr(prob, k, getattr(tracks, k))
    return prob


def batch(prob, n, seed=0):
    L = len(prob.lm_cov_id)
    ids = np.sort(np.random.default_rng(seed).choice(L, n, replace=False)).astype(np.int32)
    q = prob.subset(ids)
    q.lm_index = ids
    return q


def dump(a):
    capi = load(a.lib)
    from open_vins_amd import synth
    from open_vins_amd.updater import UpdaterMSCKF
    opts = capi.default_options(chi2_multipler=1.0)
    out = {}
    for name, q in (("batch25", batch(slam_problem(synth, 40, 3), 25)), ("batch40", slam_problem(synth, 40, 4))):
        up = UpdaterMSCKF(opts)
        up.set_slam_problem(q)
        r = up.slam_update()
        for k in ("feat_status", "chi2", "chi2_thresh", "dx", "P", "landmarks"):
            out[f"slam_update_{name}_{k}"] = r[k]
        up.close()
    prob = slam_problem(synth, 40, 5, candidates=30)
    up = UpdaterMSCKF(opts)
    up.set_slam_problem(prob)
    r = up.delayed_init(0)
    for k in ("feat_status", "chi2", "lm_cov_id", "lm_value", "lm_fej", "dx_seq", "P"):
        out[f"delayed_init_{k}"] = r[k]
    out["delayed_init_resident"] = up.get_landmarks()["value"]
    up.close()
    np.savez(a.out, **out)
    print(f"{len(out)} arrays -> {a.out}")


def compare(a):
    x, y = np.load(a.a), np.load(a.b)
    assert sorted(x.files) == sorted(y.files)
    bad = 0
    for k in sorted(x.files):
        same = x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes()
        bad += not same
        print(f"{'same bits' if same else 'DIFFERENT'}  {k} {x[k].shape}")
    print(f"{len(x.files) - bad} of {len(x.files)} arrays bit-identical")
    sys.exit(1 if bad else 0)


def timed(a):
    capi = load(a.lib)
    from open_vins_amd import synth
    from open_vins_amd.updater import UpdaterMSCKF, _ip
    opts = capi.default_options(chi2_multipler=1.0)
    active = a.variant == "active"
    rows = []
    cases = [("slam_update", 50, 0), ("slam_update", 100, 0), ("delayed_init", 50, 30)]
    for case, L, cand in cases:
        prob = slam_problem(synth, L, 3, candidates=cand)
        q = prob if cand else batch(prob, 25)
        v = capi.Views(q)
        up = UpdaterMSCKF(opts)
        lib, ctx = up.lib, up._ctx
        tri = None
        if cand:  # the entry triangulation once, on a context of its own; every repetition starts from it (ovgpu_set_triangulation)
            up0 = UpdaterMSCKF(opts)
            up0.set_problem(q)
            tri = up0.triangulate()
            up0.close()
        ids = np.zeros(0, np.int32) if cand else q.lm_index
        t_frame, t_call, t_dev, t_kern = [], [], [], []
        D = 0
        for i in range(a.reps + 3):
            up.kernel_times(reset=True)
            t0 = time.perf_counter()
            capi.check(lib.ovgpu_set_state(ctx, C.byref(v.state)), "ovgpu_set_state")
            capi.check(lib.ovgpu_set_landmarks(ctx, C.byref(v.landmarks)), "ovgpu_set_landmarks")
            if active:
                capi.check(lib.ovgpu_set_active_landmarks(ctx, int(ids.size), _ip(ids)), "ovgpu_set_active_landmarks")
            capi.check(lib.ovgpu_set_features(ctx, C.byref(v.features)), "ovgpu_set_features")
            up._views, up.F, up.N, up.Cn, up.K = v, v.features.F, v.state.N, v.state.C, v.state.K
            if cand:
                up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
            t1 = time.perf_counter()
            r = up.delayed_init(0) if cand else up.slam_update()
            t2 = time.perf_counter()
            kt = up.kernel_times(reset=True)
            D = r["stats"]["D"]
            if i >= 3:
                t_frame.append((t2 - t0) * 1e3), t_call.append((t2 - t1) * 1e3), t_dev.append(r["stats"]["ms_total"])
                t_kern.append(kt["ms_compress"] + kt["ms_update"])
        row = dict(case=case, L=L, candidates=cand, batch=int(v.features.F), build=a.tag, variant=a.variant, D=int(D), reps=a.reps)
        for name, t in (("frame", t_frame), ("call", t_call), ("device", t_dev), ("kernel", t_kern)):
            row[f"ms_{name}_median"], row[f"ms_{name}_min"], row[f"ms_{name}_max"] = float(np.median(t)), float(np.min(t)), float(np.max(t))
        rows.append(row)
        print(json.dumps(row))
        up.close()
    if a.out:
        with open(a.out, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump")
    d.add_argument("out")
    d.add_argument("--lib", default=None)
    c = sub.add_parser("compare")
    c.add_argument("a")
    c.add_argument("b")
    t = sub.add_parser("time")
    t.add_argument("--variant", choices=("all", "active"), required=True)
    t.add_argument("--lib", default=None)
    t.add_argument("--tag", default="tree")
    t.add_argument("--reps", type=int, default=30)
    t.add_argument("--out", default=None)
    a = ap.parse_args()
    {"dump": dump, "compare": compare, "time": timed}[a.cmd](a)


if __name__ == "__main__":
    main()
