"""CPU tests of the batched anchor change at the boundary (ABI 10): ovgpu_slam_change_anchors_batched and ovgpu_slam_anchor_systems(_len) are
declared by include/ovgpu.h, exported by the library and bound by the ctypes mirror and the updater; both bodies of
open_vins_amd/shim/UpdaterSLAM_change_anchors.cpp compile against the reference's declarations (tests/shim_mock; the mode-A body against the
UNPATCHED ones, with StateHelper::EKFPropagation from tests/shim_mock_ca in front) and the mode-A body uses nothing of the friend line.
What the entries compute is tests/test_gpu_anchor_batch.py's."""
import ctypes as C
import os
import re
import subprocess

from open_vins_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "open_vins_amd", "shim")
MOCK = os.path.join(ROOT, "tests", "shim_mock")
MOCK_CA = os.path.join(ROOT, "tests", "shim_mock_ca")
NEW = ("ovgpu_slam_change_anchors_batched", "ovgpu_slam_anchor_systems_len", "ovgpu_slam_anchor_systems")


def _code(path):
    txt = open(path).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def _compile(*defs):
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", *[f"-D{d}" for d in defs], f"-I{MOCK_CA}", f"-I{MOCK}", f"-I{MOCK}/update",
           f"-I{MOCK}/feat", f"-I{ROOT}/include", f"-I{SHIM}", os.path.join(SHIM, "UpdaterSLAM_change_anchors.cpp")]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_abi_version_is_10():
    txt = open(os.path.join(ROOT, "include", "ovgpu.h")).read()
    assert int(re.search(r"#define OVGPU_ABI_VERSION (\d+)", txt).group(1)) == 10
    assert capi.load().ovgpu_abi_version() == 10


def test_entries_are_declared_exported_and_bound():
    hdr = _code(os.path.join(ROOT, "include", "ovgpu.h"))
    lib = capi.load()
    bound = set(capi.declare(lib))
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", hdr), name
        assert hasattr(lib, name) and name in bound, name
    assert lib.ovgpu_slam_change_anchors_batched.argtypes == [C.c_void_p, C.c_int32, C.c_int32, capi.c_int32_p]
    # the sequential entries are still there
    assert "ovgpu_slam_change_anchors" in bound and "ovgpu_slam_change_anchor" in bound


def test_entries_refuse_a_null_context_without_a_device():
    lib = capi.load()
    n = C.c_int32(7)
    assert lib.ovgpu_slam_change_anchors_batched(None, 0, 1, C.byref(n)) == capi.ERR_INVALID and n.value == 0
    sz = capi.AnchorSizes(5, 5, 5)
    assert lib.ovgpu_slam_anchor_systems_len(None, 0, 1, C.byref(sz)) == capi.ERR_INVALID
    assert lib.ovgpu_slam_anchor_systems(None, 0, 1, C.byref(sz), None, None, None, None, None, None) == capi.ERR_INVALID


def test_struct_layouts_match_header(tmp_path):
    structs = {"ovgpu_anchor_sizes": capi.AnchorSizes, "ovgpu_anchor_system": capi.AnchorSystem}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ovgpu.h"', 'int main(void) {']
    for cname, cls in structs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"{cname}.{fname}"


def test_updater_binding_has_the_methods():
    from open_vins_amd.updater import UpdaterMSCKF
    assert callable(getattr(UpdaterMSCKF, "change_anchors_batched")) and callable(getattr(UpdaterMSCKF, "anchor_systems"))


def test_mode_b_body_compiles_and_prefers_the_batched_entry():
    r = _compile("OVGPU_SHIM_MODE_B")
    assert r.returncode == 0, r.stderr[-3000:]
    txt = _code(os.path.join(SHIM, "UpdaterSLAM_change_anchors.cpp"))
    assert "#pragma weak ovgpu_slam_change_anchors_batched" in txt  # the drop-in still loads next to a library without the entry ...
    a, b = txt.index("ovgpu_slam_change_anchors_batched("), txt.index("ovgpu_slam_change_anchors(")
    assert txt.index("set_active_landmarks(") < a < b  # ... and then falls back to the per-landmark one


def test_mode_a_body_compiles_without_the_friend_line():
    r = _compile("OVGPU_SHIM_CHANGE_ANCHORS_A")
    assert r.returncode == 0, r.stderr[-3000:]


def test_mode_a_body_uses_no_state_access():
    code = _code(os.path.join(SHIM, "ovgpu_change_anchors_a.h"))
    assert "StateAccess" not in code and "ovgpu_state_access.h" not in code and "_Cov" not in code and "_variables" not in code
    assert "StateHelper::EKFPropagation(" in code and "ovgpu_slam_anchor_systems(" in code
    assert code.index("ovgpu_set_landmarks(") < code.index("set_active_landmarks(ctx, 0, nullptr)") < code.index("ovgpu_slam_anchor_systems_len(")


def test_default_build_of_the_unit_is_still_mode_b():
    """Without the macros the unit is the mode-B body: it needs the friend line (private State::_Cov) as before."""
    r = _compile()
    assert r.returncode != 0 and "private" in r.stderr
