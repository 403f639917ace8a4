"""Call time of ovgpu_slam_init_systems (mode A of UpdaterSLAM::delayed_init) next to ovgpu_slam_delayed_init (mode B) on the same
inputs: 16 and 50 candidates on a 30-clone stereo state (N = 223).  Each call is timed host to host (the entry's own single
synchronisation included); the state, the batch and the triangulation are uploaded again before every call and are not timed.
The host-side replay through the stock StateHelper::initialize is not part of this number.

    python tools/dev_init_systems_time.py [--reps 30] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from open_vins_amd import capi, synth  # noqa: E402
from open_vins_amd.updater import UpdaterMSCKF  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for F in (16, 50):
        prob = synth.make_problem(2, F=F, seed=7, outlier_frac=0.2)
        opts = capi.default_options(chi2_multipler=1.0)
        up = UpdaterMSCKF(opts)
        up.set_problem(prob)
        tri = up.triangulate()
        t = {"mode_a_init_systems": [], "mode_b_delayed_init": []}
        for i in range(a.reps + 3):
            for name in t:
                up.set_problem(prob)
                up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
                t0 = time.perf_counter()
                if name == "mode_a_init_systems":
                    out = up.init_systems(capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH)
                    n_acc = sum(s["status"] == capi.FEAT_USED for s in out)
                else:
                    n_acc = int((up.delayed_init(capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH)["lm_cov_id"] >= 0).sum())
                dt = (time.perf_counter() - t0) * 1e3
                if i >= 3:
                    t[name].append(dt)
        for name, v in t.items():
            rows.append(dict(candidates=F, N=int(prob.N), call=name, accepted=n_acc, ms_median=float(np.median(v)), ms_min=float(np.min(v)),
                             ms_max=float(np.max(v)), reps=len(v)))
            print(json.dumps(rows[-1]))
        up.close()
    if a.out:
        with open(a.out, "w") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
