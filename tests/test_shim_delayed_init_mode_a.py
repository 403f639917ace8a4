"""CPU tests of the mode-A form of UpdaterSLAM::delayed_init (open_vins_amd/shim/ovgpu_delayed_init_a.h, selected by
-DOVGPU_SHIM_DELAYED_INIT_A in UpdaterSLAM_delayed_init.cpp): it compiles against the UNPATCHED reference declarations (tests/shim_mock,
with StateHelper::initialize from tests/shim_mock_a in front) and uses nothing of the friend line's StateAccess."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "open_vins_amd", "shim")
MOCK = os.path.join(ROOT, "tests", "shim_mock")
MOCK_A = os.path.join(ROOT, "tests", "shim_mock_a")


def _compile(*defs):
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", *[f"-D{d}" for d in defs], f"-I{MOCK_A}", f"-I{MOCK}", f"-I{MOCK}/update",
           f"-I{MOCK}/feat", f"-I{ROOT}/include", f"-I{SHIM}", os.path.join(SHIM, "UpdaterSLAM_delayed_init.cpp")]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_mode_a_delayed_init_compiles_without_the_friend_line():
    r = _compile("OVGPU_SHIM_DELAYED_INIT_A")
    assert r.returncode == 0, r.stderr[-3000:]


def test_mode_a_delayed_init_uses_no_state_access():
    src = open(os.path.join(SHIM, "ovgpu_delayed_init_a.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "StateAccess" not in code and "ovgpu_state_access.h" not in code and "_Cov" not in code and "_variables" not in code
    assert "StateHelper::initialize(" in code and "ovgpu_slam_init_systems(" in code


def test_default_build_of_the_unit_is_still_mode_b():
    """Without the macro the unit is the mode-B body: it needs the friend line (private State::_Cov) as before."""
    r = _compile()
    assert r.returncode != 0 and "private" in r.stderr
    assert _compile("OVGPU_SHIM_MODE_B").returncode == 0
