"""CPU tests of the fused delayed initialisation at the boundary: ovgpu_slam_delayed_init_fused is declared by include/ovgpu.h with the argument
list of ovgpu_slam_delayed_init, exported by the library and bound by the ctypes mirror and the updater, under the ABI number its library already
had (callers find it by symbol).  tests/fake_ovgpu does not have the entry, so every CPU drop-in leg runs the chain it ran before; the shim
reaches the entry through a weak reference only.  What the entry computes is tests/test_gpu_delayed_init_fused.py's."""
import ctypes as C
import os
import re

import numpy as np

from open_vins_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ovgpu_slam_delayed_init_fused"
OLD = "ovgpu_slam_delayed_init"


def _code(path):
    txt = open(path).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def _args(code, name):
    decl = re.search(rf"\bint {name}\s*\(([^)]*)\)", code)
    assert decl, name
    return [re.sub(r"\s+", " ", a).strip() for a in decl.group(1).split(",")]


def test_entry_is_declared_exported_and_bound_under_abi_10():
    path = os.path.join(ROOT, "include", "ovgpu.h")
    txt, code = open(path).read(), _code(path)
    assert int(re.search(r"#define OVGPU_ABI_VERSION (\d+)", txt).group(1)) == 10
    args = _args(code, NAME)
    assert args == _args(code, OLD)  # the exact argument list of the existing entry
    assert args == ["ovgpu_ctx *ctx", "int32_t feat_rep", "int32_t *feat_status", "double *chi2", "double *chi2_thresh", "int32_t *lm_cov_id",
                    "double *lm_value", "double *lm_fej", "int32_t *anchor_cam", "int32_t *anchor_clone", "double *dx_seq", "int32_t *N_out",
                    "double *P_out", "ovgpu_update_stats *stats"]
    assert NAME in txt[:txt.index("#define OVGPU_ABI_VERSION")]  # the history comment names it
    for opt in ('"delayed_init_fused"', '"delayed_init_fused_steps"', '"delayed_init_chain_steps"'):
        assert opt in txt  # the switches are named next to the others
    lib = capi.load()
    assert lib.ovgpu_abi_version() == 10
    assert hasattr(lib, NAME) and NAME in capi.declare(lib) and OLD in capi.declare(lib)
    assert getattr(lib, NAME).argtypes == getattr(lib, OLD).argtypes
    ip, dp = capi.c_int32_p, capi.c_double_p
    assert getattr(lib, NAME).argtypes == [C.c_void_p, C.c_int32, ip, dp, dp, ip, dp, dp, ip, ip, dp, ip, dp, C.POINTER(capi.UpdateStats)]


def test_entry_refuses_a_null_context_without_a_device():
    lib = capi.load()
    assert getattr(lib, NAME)(None, 0, None, None, None, None, None, None, None, None, None, None, None, None) == capi.ERR_INVALID


def test_fake_library_does_not_have_the_entry():
    assert NAME not in open(os.path.join(ROOT, "tests", "fake_ovgpu", "fake_ovgpu.cpp")).read()


def test_shim_names_the_entry_only_behind_a_weak_reference():
    shim = os.path.join(ROOT, "open_vins_amd", "shim")
    users = [f for f in sorted(os.listdir(shim)) if f.endswith((".cpp", ".h")) and NAME in _code(os.path.join(shim, f))]
    assert users == ["UpdaterSLAM_delayed_init.cpp"]
    code = _code(os.path.join(shim, users[0]))
    assert re.search(rf"#pragma weak {NAME}\b", code)
    uses = [m.start() for m in re.finditer(rf"\b{NAME}\b", code)]
    assert len(uses) == 3  # the pragma, the test of the address, the value taken when it is there
    assert re.search(rf"{NAME}\s*\?\s*{NAME}\s*:\s*{OLD}\b", code)  # ... with the existing entry as the other branch
    assert code.index("#pragma weak " + NAME) < uses[1]


class _Lib:
    """records the call; stands for a library so that the updater's marshalling runs without a device"""

    def __init__(self):
        self.calls = []

    def _entry(self, name, ctx, rep, st, x2, thr, cov, val, fej, acam, aclone, dx_seq, N_out, P, stats):
        self.calls.append((name, rep))
        n = 9
        N_out._obj.value = n
        for i in range(n * n):
            P[i] = float(i)
        st[1], cov[0], dx_seq[12] = 4, 6, 2.5
        stats._obj.n_used = 1
        return 0

    def ovgpu_slam_delayed_init(self, *a):
        return self._entry(OLD, *a)

    def ovgpu_slam_delayed_init_fused(self, *a):
        return self._entry(NAME, *a)

    def ovgpu_set_feature_reps(self, ctx, reps):
        self.calls.append(("ovgpu_set_feature_reps", [reps[i] for i in range(2)]))
        return 0


def _updater(F, N):
    from open_vins_amd.updater import UpdaterMSCKF
    up = UpdaterMSCKF.__new__(UpdaterMSCKF)
    up.lib, up._ctx, up.F, up.N = _Lib(), None, F, N
    return up


def test_updater_marshals_to_the_new_symbol():
    up = _updater(F=2, N=6)
    out = up.delayed_init(3, fused=True)
    assert up.lib.calls == [(NAME, 3)]
    assert out["N"] == 9 and up.N == 9 and out["P"].shape == (9, 9) and out["P"][1, 2] == 11.0
    assert out["dx_seq"].shape == (2, 12) and out["dx_seq"][1, 0] == 2.5  # N + 3 F columns a row
    assert out["feat_status"].tolist() == [0, 4] and out["lm_cov_id"].tolist() == [6, 0] and out["stats"]["n_used"] == 1
    assert set(out) == {"feat_status", "chi2", "chi2_thresh", "lm_cov_id", "lm_value", "lm_fej", "anchor_cam", "anchor_clone", "dx_seq", "rc", "N", "P", "stats"}
    up = _updater(F=2, N=6)
    same = up.delayed_init(3)  # the default stays the existing entry, the dictionary is the same
    assert up.lib.calls == [(OLD, 3)] and set(same) == set(out)
    up = _updater(F=2, N=6)
    each = np.array([0, 5], np.int32)
    out = up.delayed_init(0, feat_rep_each=each, fused=True)
    assert up.lib.calls == [("ovgpu_set_feature_reps", [0, 5]), (NAME, 0)] and out["dx_seq"].shape == (2, 6 + 3 + 1)
