"""The upload arena and the landing zone of the host side (open_vins_amd/csrc/host_link.h) without a GPU: tests/host/host_link_main.cpp
instantiates Uplink / Landing with a port whose copies and launches run only when its fake stream is synchronised, and is built here as a
stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer — so a source that died before its copy ran, an arena or a zone freed
under copies in flight, or a landing beyond the reservation ends the program with a non-zero status."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_uplink_and_landing_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ or clang++) on PATH")
    exe = str(tmp_path / "host_link_main")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "open_vins_amd", "csrc"), os.path.join(ROOT, "tests", "host", "host_link_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0 and "host_link ok" in run.stdout, run.stdout + run.stderr
