"""CPU tests of ovgpu_set_active_landmarks at the boundary: exported by the library, declared by the ctypes mirror, refuses a null context
without a device, and the drop-in units name their set where include/ovgpu.h says it goes (after ovgpu_set_landmarks, before ovgpu_set_features).
That the units compile and run is covered by tests/test_shim*.py and tests/test_dropin_build.py, which build them as they are."""
import ctypes as C
import os
import re

from open_vins_amd import capi

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SHIM = os.path.join(ROOT, "open_vins_amd", "shim")


def _code(path):
    """the unit without its comments: a call named in a comment is no call"""
    txt = open(path).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_entry_is_exported_and_declared():
    lib = capi.load()
    assert hasattr(lib, "ovgpu_set_active_landmarks")
    assert "ovgpu_set_active_landmarks" in set(capi.declare(lib))
    assert lib.ovgpu_set_active_landmarks.argtypes == [C.c_void_p, C.c_int32, capi.c_int32_p]
    assert lib.ovgpu_set_active_landmarks(None, 0, None) == capi.ERR_INVALID and b"null ctx" in lib.ovgpu_last_error()


def test_abi_version_is_the_headers():
    txt = open(os.path.join(ROOT, "include", "ovgpu.h")).read()
    ver = int(re.search(r"#define OVGPU_ABI_VERSION (\d+)", txt).group(1))
    assert ver >= 9 and capi.load().ovgpu_abi_version() == ver


def test_updater_binding_has_the_method():
    from open_vins_amd.updater import UpdaterMSCKF
    assert callable(getattr(UpdaterMSCKF, "set_active_landmarks"))


def test_dropin_units_name_their_set_between_landmarks_and_features():
    common = open(os.path.join(SHIM, "ovgpu_shim_common.h")).read()
    assert "#pragma weak ovgpu_set_active_landmarks" in common  # the drop-in still loads next to a library without the entry
    for unit in ("UpdaterSLAM_update.cpp", "UpdaterSLAM_delayed_init.cpp", "ovgpu_delayed_init_a.h"):
        txt = _code(os.path.join(SHIM, unit))
        a, b, c = txt.index("ovgpu_set_landmarks("), txt.index("set_active_landmarks("), txt.index("ovgpu_set_features(")
        assert a < b < c, unit
    for unit in ("UpdaterSLAM_delayed_init.cpp", "ovgpu_delayed_init_a.h"):
        assert "set_active_landmarks(ctx, 0, nullptr)" in _code(os.path.join(SHIM, unit)), unit  # the empty set
    txt = _code(os.path.join(SHIM, "UpdaterSLAM_change_anchors.cpp"))
    assert txt.index("ovgpu_set_landmarks(") < txt.index("set_active_landmarks(") < txt.index("ovgpu_slam_change_anchors(")
