"""CPU tests of ovgpu_msckf_update_lm at the boundary: include/ovgpu.h declares it, the library exports it and the ctypes mirror and the updater bind
it, under the ABI number the library already had (callers find it by symbol).  tests/fake_ovgpu and the shims do not have the entry — the shims upload
the state with every call, so their landmarks never go stale.  What needs no device is checked here: the signature, the refusal of a null context and
the updater's marshalling.  What the entry computes is tests/test_gpu_msckf_lm.py's."""
import ctypes as C
import os
import re

import numpy as np

from open_vins_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ovgpu_msckf_update_lm"


def _code(path):
    txt = open(path).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_entry_is_declared_exported_and_bound_under_abi_10():
    txt = open(os.path.join(ROOT, "include", "ovgpu.h")).read()
    assert int(re.search(r"#define OVGPU_ABI_VERSION (\d+)", txt).group(1)) == 10
    decl = re.search(rf"\bint {NAME}\s*\(([^)]*)\)", _code(os.path.join(ROOT, "include", "ovgpu.h")))
    assert decl
    args = [re.sub(r"\s+", " ", a).strip() for a in decl.group(1).split(",")]
    assert args == ["ovgpu_ctx *ctx", "int32_t *feat_status", "double *chi2", "double *chi2_thresh", "double *p_FinG", "double *dx", "double *P_out",
                    "double *lm_out", "ovgpu_update_stats *stats"]
    assert NAME in txt[:txt.index("#define OVGPU_ABI_VERSION")]  # the history comment names it
    lib = capi.load()
    assert lib.ovgpu_abi_version() == 10
    assert hasattr(lib, NAME) and NAME in capi.declare(lib)
    ip, dp = capi.c_int32_p, capi.c_double_p
    fn = getattr(lib, NAME)
    assert fn.restype == C.c_int and fn.argtypes == [C.c_void_p, ip, dp, dp, dp, dp, dp, dp, C.POINTER(capi.UpdateStats)]
    # ovgpu_msckf_update keeps its own shape: the new entry is that one with lm_out in front of stats
    assert lib.ovgpu_msckf_update.argtypes == fn.argtypes[:7] + fn.argtypes[8:]


def test_entry_refuses_a_null_context_without_a_device():
    lib = capi.load()
    assert lib.ovgpu_msckf_update_lm(None, None, None, None, None, None, None, None, None) == capi.ERR_INVALID
    assert b"null" in lib.ovgpu_last_error()


def test_fake_library_and_shims_do_not_have_the_entry():
    assert NAME not in open(os.path.join(ROOT, "tests", "fake_ovgpu", "fake_ovgpu.cpp")).read()
    assert NAME not in open(os.path.join(ROOT, "open_vins_amd", "shim", "UpdaterMSCKF.cpp")).read()


class _Lib:
    """records the call; stands for a library so that the updater's marshalling runs without a device"""

    def __init__(self, L):
        self.L, self.lm_was_null = L, None

    def ovgpu_get_landmarks(self, ctx, L_out, *rest):
        L_out._obj.value = self.L
        return 0

    def ovgpu_msckf_update_lm(self, ctx, st, x2, thr, pg, dx, P, lm, stats):
        self.lm_was_null = lm is None
        st[0], dx[1] = 4, 0.5
        if lm is not None:
            lm[3 * self.L - 1] = 7.0
        stats._obj.n_used = 3
        return 0

    def ovgpu_last_update_route(self, ctx):
        return capi.COMPRESS_GRAM

    def ovgpu_get_state(self, ctx, P, clone, calib, intr):
        return 0


def _updater(F, N, L):
    from open_vins_amd.updater import UpdaterMSCKF
    up = UpdaterMSCKF.__new__(UpdaterMSCKF)
    up.lib, up._ctx, up.F, up.N, up.Cn, up.K = _Lib(L), None, F, N, 3, 1
    return up


def test_updater_returns_the_landmarks_next_to_the_update():
    up = _updater(F=5, N=9, L=2)
    out = up.update_lm()
    assert out["landmarks"].shape == (2, 3) and out["landmarks"][1, 2] == 7.0 and not up.lib.lm_was_null
    assert out["feat_status"][0] == 4 and out["dx"][1] == 0.5 and out["P"].shape == (9, 9) and out["stats"]["n_used"] == 3
    assert out["rc"] == 0 and out["route"] == capi.COMPRESS_GRAM and out["clone_q_p"].shape == (3, 7)
    up = _updater(F=5, N=9, L=0)  # no landmark: an empty array, and the library is not handed a pointer to nothing
    out = up.update_lm()
    assert out["landmarks"].shape == (0, 3) and up.lib.lm_was_null
