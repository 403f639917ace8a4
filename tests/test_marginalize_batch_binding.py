"""CPU tests of the batched marginalisation at the boundary: ovgpu_state_marginalize_batched is declared by include/ovgpu.h, exported by the
library and bound by the ctypes mirror and the updater, under the ABI number its library already had (callers find it by symbol); the
resident-covariance StateHelper reaches it only through a weak reference, so that the drop-in still loads — and runs its host path — next to a
library without the entry (tests/fake_ovgpu is one: tests/test_dropin_build.py).  What the entry computes is tests/test_gpu_marginalize_batch.py's."""
import ctypes as C
import os
import re

from open_vins_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ovgpu_state_marginalize_batched"


def _code(path):
    txt = open(path).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_entry_is_declared_exported_and_bound_under_abi_10():
    txt = open(os.path.join(ROOT, "include", "ovgpu.h")).read()
    assert int(re.search(r"#define OVGPU_ABI_VERSION (\d+)", txt).group(1)) == 10
    assert re.search(rf"\bint {NAME}\s*\(\s*ovgpu_ctx \*ctx,\s*int32_t n,\s*const int32_t \*cov_id,\s*const int32_t \*size\)", _code(os.path.join(ROOT, "include", "ovgpu.h")))
    assert NAME in txt[:txt.index("#define OVGPU_ABI_VERSION")]  # the history comment names it
    lib = capi.load()
    assert lib.ovgpu_abi_version() == 10
    assert hasattr(lib, NAME) and NAME in capi.declare(lib)
    assert getattr(lib, NAME).argtypes == [C.c_void_p, C.c_int32, capi.c_int32_p, capi.c_int32_p]
    assert "ovgpu_state_marginalize" in capi.declare(lib)  # the single entry is still there


def test_entry_checks_its_arguments_without_a_device():
    lib = capi.load()
    one = (C.c_int32 * 1)(0)
    assert lib.ovgpu_state_marginalize_batched(None, 1, one, one) == capi.ERR_INVALID
    assert lib.ovgpu_state_marginalize_batched(None, 0, None, None) == capi.ERR_INVALID  # (a null context is refused before n is looked at)


def test_updater_binding_has_the_method():
    from open_vins_amd.updater import UpdaterMSCKF
    assert callable(getattr(UpdaterMSCKF, "state_marginalize_many")) and callable(getattr(UpdaterMSCKF, "state_marginalize"))


def test_fake_library_does_not_have_the_entry():
    """the CPU legs of tests/test_dropin_build.py link tests/fake_ovgpu: there the weak symbol stays null and they run the host path"""
    assert NAME not in open(os.path.join(ROOT, "tests", "fake_ovgpu", "fake_ovgpu.cpp")).read()


def test_resident_state_helper_reaches_the_entry_through_a_weak_reference_only():
    code = _code(os.path.join(ROOT, "open_vins_amd", "shim", "StateHelper_resident.cpp"))
    assert f"#pragma weak {NAME}" in code
    calls = [m.start() for m in re.finditer(rf"{NAME}\s*\(", code)]
    assert len(calls) == 1
    body = code[code.index("void StateHelper::marginalize_slam("):]
    null_test = re.search(rf"if \(\s*{NAME}\s*&&", body)
    assert null_test and code.index("void StateHelper::marginalize_slam(") + null_test.start() < calls[0]
    # the path of a library without the entry is still there, behind it: every flagged landmark through the reference's own marginalize
    assert body.index("StateHelperHost::marginalize(state, lm)") > body.index(f"{NAME}(")
    # marginalize_old_clone keeps the single entry
    old = code[code.index("void StateHelper::marginalize_old_clone("):code.index("void StateHelper::marginalize_slam(")]
    assert "StateHelper::marginalize(state," in old and NAME not in old
