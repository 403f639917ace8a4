"""Where k_system_t's time goes for ONE candidate of the delayed initialisation (init mode): its SYS_PROFILE phase counters (csrc/k_system.h,
a -DSYS_PROFILE build of the library, named by --lib) after one frame of ovgpu_slam_delayed_init_fused on tools/dev_delayed_init_fused_ab.py's
state.  The counters are those of the frame's LAST launch of the kernel, i.e. of candidate F - 1: pick F so that it triangulates.

    python tools/dev_init_system_phases.py --lib PATH [--F 30]

Slot i holds the cycles that ended at the kernel's i-th SYS_T mark: 1 the representation Jacobian (a0), 2 the measurement rows (a), 9 T = H P,
3 S0 = T H^T, 4 the right-hand sides and the trailing updates, 0 the panel factorisations (and the set-up ahead of (a0)), 5 + 6 the statistic,
7 the reflectors (b), 8 the stack (d).  The gate (c) is 9 + 3 + 4 + 0 + 5 + 6."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dev_delayed_init_fused_ab as ab  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--F", type=int, default=30)
    a = ap.parse_args()
    import torch  # noqa: F401  (torch's HIP runtime first)
    from open_vins_amd import capi, synth
    lib = ab.bind(capi, a.lib)
    lib.ovgpu_debug_cycles.argtypes, lib.ovgpu_debug_cycles.restype = [C.c_void_p, C.c_int, C.POINTER(C.c_longlong)], C.c_int
    prob = ab.problem(synth, a.F)
    leg = ab.Leg(capi, lib, prob, "phases", None)
    leg.frame()  # (allocations, first-launch costs)
    leg.ok(lib.ovgpu_debug_cycles(leg.ctx, 1, None), "ovgpu_debug_cycles")
    leg.frame()
    buf = (C.c_longlong * 512)()
    leg.ok(lib.ovgpu_debug_cycles(leg.ctx, 1, buf), "ovgpu_debug_cycles")
    t = np.array(buf[100:110], dtype=np.float64)
    m = int(np.diff(prob.meas_offsets)[a.F - 1])
    gate = t[9] + t[3] + t[4] + t[0] + t[5] + t[6]
    row = dict(case="k_system_t_init_phases", F=a.F, candidate=a.F - 1, m=m, status=int(leg.st[a.F - 1]), cycles=t.tolist(), total=float(t.sum()),
               gate_share=float(gate / max(t.sum(), 1.0)), tp_share=float(t[9] / max(t.sum(), 1.0)), s0_share=float(t[3] / max(t.sum(), 1.0)),
               factor_share=float((t[4] + t[0]) / max(t.sum(), 1.0)), rows_share=float((t[1] + t[2]) / max(t.sum(), 1.0)),
               reflectors_share=float(t[7] / max(t.sum(), 1.0)), stack_share=float(t[8] / max(t.sum(), 1.0)))
    print(json.dumps(row))
    leg.close()


if __name__ == "__main__":
    main()
