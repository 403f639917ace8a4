"""What ovgpu_debug_option "feat_classes" (a per-feature kernel per length class, csrc/feat_classes.h) is worth on batches of mixed track lengths:
ONE process per (workload, leg), so that the legs can be interleaved on one box by the caller (a shell loop: leg parent, level0, level1, three
times over); a row of JSON per run.

    time WORKLOAD --leg parent|level0|level1 [--lib PATH] [--steps K] [--warmup W] [--loops 5] [--out FILE.jsonl] [--dump FILE.npz]
                    the timed loop of bench.py: ovgpu_reset_state + ovgpu_msckf_update_async per step over the resident batch with
                    "layout_every_update" = 1 (a step costs what a frame's tables cost), `loops` loops of `steps` steps between two
                    synchronisations; ms per update = the median loop / steps.  --lib: the parent commit's build (leg parent: no option of this
                    change is named).  --dump: the posterior of the last step and the per-feature outputs of one blocking update, for a
                    bit comparison between legs.
    trace WORKLOAD --leg ... [--steps 20]
                    the steps alone, for a rocprofv3 --kernel-trace --stats run of its own (the per-class kernel times)

Workloads:
    ragged3   configs[3] geometry, ragged tracks: C = 30, K = 4, F = 10000, track = "ragged"
    ragged2   configs[2] geometry, ragged tracks: C = 30, K = 2, F = 2000 (one class expected: level 1 must equal level 0)
    mixed233  the LARGE state of tests/track_shapes.py (60 x 4, no calibration, D = 360), F = 800 ragged tracks and ONE track of 233 observations
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workload(name):
    from open_vins_amd import capi, synth
    if name == "ragged3":
        return synth.make_problem(4, C=30, K=4, F=10000, track="ragged"), capi.default_options()
    if name == "ragged2":
        return synth.make_problem(3, C=30, K=2, F=2000, track="ragged"), capi.default_options()
    if name == "mixed233":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import track_shapes as ts
        st = ts.LARGE
        p = synth.make_problem(5, C=st["C"], K=st["K"], F=800, track="ragged", calib_noise=0.0)
        m = np.diff(p.meas_offsets)
        f = int(np.argmax(m))
        p = ts.with_lengths(p, [233 if g == f else (None if m[g] <= 232 else 232) for g in range(p.F)])
        return p, capi.default_options(do_calib_camera_pose=0, do_calib_camera_intrinsics=0)
    raise SystemExit(f"unknown workload {name}")


def class_sizes(lengths):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import class_shapes as cs
    return {str(k): b - a for k, a, b, _ in cs.expected_partition(lengths)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["time", "trace"])
    ap.add_argument("workload")
    ap.add_argument("--leg", choices=["parent", "level0", "level1"], required=True)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loops", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--dump", default=None)
    a = ap.parse_args()
    from open_vins_amd import capi
    if a.lib:
        capi.LIB_PATH = os.path.abspath(a.lib)
    from open_vins_amd.updater import UpdaterMSCKF
    prob, opts = workload(a.workload)
    up = UpdaterMSCKF(opts)
    up.debug_option("layout_every_update", 1)
    if a.leg != "parent":
        up.debug_option("feat_classes", 1 if a.leg == "level1" else 0)
    up.set_problem(prob)

    def step():
        up.reset_state()
        up.update_async()

    for _ in range(a.warmup):
        step()
    up.synchronize()
    if a.mode == "trace":
        for _ in range(a.steps):
            step()
        up.synchronize()
        return
    loops = []
    for _ in range(a.loops):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        up.synchronize()
        loops.append((time.perf_counter() - t0) / a.steps * 1e3)
    m = np.diff(prob.meas_offsets)
    row = dict(workload=a.workload, leg=a.leg, build="parent" if a.lib else "tree", F=int(prob.F), M=int(prob.M), m_max=int(m.max()), D=None, steps=a.steps,
               ms_loops=loops, ms_per_update=float(np.median(loops)), ms_spread=float(max(loops) - min(loops)), class_sizes=class_sizes(m),
               last_feature_kernel=int(up.debug_option("last_feature_kernel")), last_stack_raw=int(up.debug_option("last_stack_raw")))
    if a.leg != "parent":
        row["last_feature_classes"] = int(up.debug_option("last_feature_classes"))
        row["class_features"] = [int(up.debug_option(f"last_class_features_{k}")) for k in range(4)]
    if a.dump:
        post = up.get_state()
        up.reset_state()
        out = up.update()
        row["D"] = int(out["stats"]["D"])
        np.savez(a.dump, P_async=post["P"], clone_async=post["clone_q_p"], **{k: out[k] for k in ("feat_status", "chi2", "chi2_thresh", "p_FinG", "dx", "P", "clone_q_p", "calib_q_p", "intrinsics")})
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")
    up.close()


if __name__ == "__main__":
    main()
