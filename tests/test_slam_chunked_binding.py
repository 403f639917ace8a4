"""CPU tests of the chunked SLAM update at the boundary: ovgpu_slam_update_chunked is declared by include/ovgpu.h, exported by the library and bound by
the ctypes mirror and the updater, under the ABI number its library already had (callers find it by symbol).  tests/fake_ovgpu does not have the
entry — the shim does not call it: the reference's chunking lives in VioManager, outside the drop-in units —, so what needs no device is checked
here: the signature, the refusal of a null context, and the updater's own argument checks.  What the entry computes is
tests/test_gpu_slam_chunked.py's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from open_vins_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ovgpu_slam_update_chunked"


def _code(path):
    txt = open(path).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_entry_is_declared_exported_and_bound_under_abi_10():
    txt = open(os.path.join(ROOT, "include", "ovgpu.h")).read()
    assert int(re.search(r"#define OVGPU_ABI_VERSION (\d+)", txt).group(1)) == 10
    decl = re.search(rf"\bint {NAME}\s*\(([^)]*)\)", _code(os.path.join(ROOT, "include", "ovgpu.h")))
    assert decl
    args = [re.sub(r"\s+", " ", a).strip() for a in decl.group(1).split(",")]
    assert args == ["ovgpu_ctx *ctx", "int32_t n_chunks", "const int32_t *chunk_first", "const int32_t *lm_index", "int32_t *feat_status", "double *chi2",
                    "double *chi2_thresh", "double *dx_seq", "double *P_out", "double *lm_out", "ovgpu_update_stats *stats"]
    assert NAME in txt[:txt.index("#define OVGPU_ABI_VERSION")]  # the history comment names it
    lib = capi.load()
    assert lib.ovgpu_abi_version() == 10
    assert hasattr(lib, NAME) and NAME in capi.declare(lib)
    ip, dp = capi.c_int32_p, capi.c_double_p
    assert getattr(lib, NAME).argtypes == [C.c_void_p, C.c_int32, ip, ip, ip, dp, dp, dp, dp, dp, C.POINTER(capi.UpdateStats)]
    assert "ovgpu_slam_update" in capi.declare(lib)  # the single entry is still there


def test_entry_refuses_a_null_context_without_a_device():
    lib = capi.load()
    first = (C.c_int32 * 2)(0, 0)
    assert lib.ovgpu_slam_update_chunked(None, 1, first, None, None, None, None, None, None, None, None) == capi.ERR_INVALID


def test_fake_library_does_not_have_the_entry():
    assert NAME not in open(os.path.join(ROOT, "tests", "fake_ovgpu", "fake_ovgpu.cpp")).read()
    assert NAME not in open(os.path.join(ROOT, "open_vins_amd", "shim", "UpdaterSLAM_update.cpp")).read()


class _Lib:
    """records the call; stands for a library so that the updater's marshalling runs without a device"""

    def __init__(self, L):
        self.L, self.call = L, None

    def ovgpu_get_landmarks(self, ctx, L_out, *rest):
        L_out._obj.value = self.L
        return 0

    def ovgpu_slam_update_chunked(self, ctx, n, first, lm_index, st, x2, thr, dx_seq, P, lm, stats):
        self.call = dict(n=n, first=[first[i] for i in range(n + 1)], lm_index=[lm_index[i] for i in range(first[n])], n_stats=len(stats))
        for k in range(n):
            stats[k].n_used, stats[k].D = k + 1, 200 + k
            dx_seq[k * 7] = float(k + 1)
        return 0


def _updater(F, N, L):
    from open_vins_amd.updater import UpdaterMSCKF
    up = UpdaterMSCKF.__new__(UpdaterMSCKF)
    up.lib, up._ctx, up.F, up.N = _Lib(L), None, F, N
    up._views = type("V", (), dict(lm_index=np.arange(F, dtype=np.int32)))()
    return up


def test_updater_marshals_chunks_indices_and_outputs():
    up = _updater(F=6, N=7, L=4)
    out = up.slam_update_chunked(lm_index=[3, 0, 1, 1, 2, 0], chunk_first=[0, 2, 2, 6])
    assert up.lib.call == dict(n=3, first=[0, 2, 2, 6], lm_index=[3, 0, 1, 1, 2, 0], n_stats=3)
    assert out["dx_seq"].shape == (3, 7) and out["dx_seq"][:, 0].tolist() == [1.0, 2.0, 3.0]
    assert out["P"].shape == (7, 7) and out["landmarks"].shape == (4, 3) and out["feat_status"].shape == (6,)
    assert [s["n_used"] for s in out["stats"]] == [1, 2, 3] and [s["D"] for s in out["stats"]] == [200, 201, 202]
    one = up.slam_update_chunked()  # the snapshot's lm_index, one chunk
    assert up.lib.call["n"] == 1 and up.lib.call["first"] == [0, 6] and one["dx_seq"].shape == (1, 7)


def test_updater_checks_its_arguments():
    up = _updater(F=6, N=7, L=4)
    with pytest.raises(ValueError):
        up.slam_update_chunked(lm_index=[0, 1, 2], chunk_first=[0, 6])
    with pytest.raises(ValueError):
        up.slam_update_chunked(chunk_first=[0])
