"""The owning buffer type of the host side (open_vins_amd/csrc/dev_buf.h) without a GPU: tests/host/dev_buf_main.cpp instantiates it with a
counting malloc / free policy and is built here as a stand-alone program with AddressSanitizer and UndefinedBehaviorSanitizer, so a double free, a
leak (LeakSanitizer runs at exit), a use after a move or an uncounted allocation ends the program with a non-zero status."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_owned_buf_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ or clang++) on PATH")
    exe = str(tmp_path / "dev_buf_main")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "open_vins_amd", "csrc"), os.path.join(ROOT, "tests", "host", "dev_buf_main.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0 and "dev_buf ok" in run.stdout, run.stdout + run.stderr
