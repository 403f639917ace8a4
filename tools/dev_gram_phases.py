"""Developer probe (GPU, developer build with -DOVG_GRAM_PROF: EXTRA=-DOVG_GRAM_PROF tools/build_dev_lib.sh): where a workgroup of k_gram_regions
spends its time, region by region, and how long the workgroups of a region idle until the slowest one of the launch ends.
usage: dev_gram_phases.py [config = 3] [gram_read_ahead = 1] [gram_waves = 8] [raw_work_const: the library's]"""
import sys, os, ctypes as C
import numpy as np
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from open_vins_amd import capi, synth
from open_vins_amd.updater import UpdaterMSCKF
cfg = int(sys.argv[1]) if len(sys.argv) > 1 else 3
ahead = int(sys.argv[2]) if len(sys.argv) > 2 else 1
waves = int(sys.argv[3]) if len(sys.argv) > 3 and ahead else 8 if ahead else 4  # (without the reads ahead the kernel has four)
prob = synth.make_problem(cfg)
up = UpdaterMSCKF(capi.default_options(chi2_multipler=1.0))
up.debug_option("gram_read_ahead", ahead)
up.debug_option("gram_waves", waves)
if len(sys.argv) > 4:
    up.debug_option("raw_work_const", int(sys.argv[4]))
work_const = up.debug_option("raw_work_const")
up.set_problem(prob)
for _ in range(5):
    up.reset_state(); up.update_async()
up.synchronize()
n = 1024
up.lib.ovgpu_debug_gram_phases.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
buf = (C.c_longlong * (64 * n))()
launched = C.c_int(0)
capi.check(up.lib.ovgpu_debug_gram_phases(up._ctx, buf, C.c_int(n), C.byref(launched)), "ovgpu_debug_gram_phases")
a = np.array(buf, dtype=np.float64).reshape(n, 8, 8)[:min(launched.value, n), :waves]  # the workgroups of the LAST launch (the counters wrap at 1024)
t0, t1 = a[:, :, 0].min(), a[:, :, 1].max()
print(f"# k_gram_regions phase counters, configs[{cfg - 1}], gram_read_ahead = {ahead}, gram_waves = {waves}, raw_work_const = {work_const}: {len(a)} workgroups, launch {10 * (t1 - t0) / 1e3:.1f} us by the 100 MHz counter")
print("# shader cycles of the SLOWEST wavefront of a workgroup, mean over the workgroups of a group; groups = workgroups of equal stage-loop length (one region each, +-3 %)")
print("#  wgs  start_us  end_us  idle_us |  zero   fills+bar  loop    (op.wait  barrier)   put  |  share of the workgroup's cycles: zero+fills  loop-wait-bar  wait  bar  put")
slow = a[np.arange(len(a)), a[:, :, 4].argmax(axis=1)]  # the wavefront with the longest stage loop
order = np.argsort(slow[:, 4])
groups, cur = [], [order[0]]
for i in order[1:]:
    if slow[i, 4] > 1.06 * slow[cur[0], 4]:
        groups.append(cur); cur = [i]
    else:
        cur.append(i)
groups.append(cur)
for g in groups:
    s = slow[g]
    m = s.mean(axis=0)
    tot = m[2] + m[3] + m[4] + m[7]
    st, en = 10 * (a[g][:, :, 0].min(axis=1) - t0).mean() / 1e3, 10 * (a[g][:, :, 1].max(axis=1) - t0).mean() / 1e3
    idle = 10 * (t1 - a[g][:, :, 1].max(axis=1)).mean() / 1e3
    print(f"  {len(g):4d}  {st:7.1f}  {en:6.1f}  {idle:6.1f} | {m[2]:6.0f}  {m[3]:8.0f}  {m[4]:7.0f}  ({m[5]:7.0f}  {m[6]:7.0f})  {m[7]:6.0f} |"
          f"  {100 * (m[2] + m[3]) / tot:5.1f}  {100 * (m[4] - m[5] - m[6]) / tot:5.1f}  {100 * m[5] / tot:5.1f}  {100 * m[6] / tot:5.1f}  {100 * m[7] / tot:5.1f}")
m = slow.mean(axis=0)
tot = m[2] + m[3] + m[4] + m[7]
idle = 10 * (t1 - a[:, :, 1].max(axis=1)).mean() / 1e3
print(f"# all: zero+fills {100 * (m[2] + m[3]) / tot:.1f} %, loop without waits {100 * (m[4] - m[5] - m[6]) / tot:.1f} %, operand wait {100 * m[5] / tot:.1f} %, stage barrier {100 * m[6] / tot:.1f} %, "
      f"tile stores {100 * m[7] / tot:.1f} %; mean idle until the launch ends {idle:.1f} us of {10 * (t1 - t0) / 1e3:.1f}")
up.close()
