"""open_vins_amd/csrc/feat_classes.h — the partition of an MSCKF batch into length classes, plain C++ — compiled with g++ under the address and
undefined-behaviour sanitizers into a stand-alone program (tests/host/feat_classes_main.cpp, its own main) and held to the Python restatement of
the rule (class_shapes.expected_partition).  Nothing is loaded into this process and nothing is preloaded: the sanitizers' runtime is the
program's own (as tests/test_dev_buf_host.py builds its program)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import class_shapes as cs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

EDGES = [62, 63, 126, 127, 232, 233]


def _batches():
    out = [(c.id, [int(x) for x in c.lengths]) for c in cs.CASES]
    out.append(("all-empty", [0, 0, 0, 0]))
    out.append(("no-feature", []))
    out.append(("short-only", [1, 0, 1]))
    out.append(("F1", [9]))
    out.append(("F1-empty", [0]))
    out.append(("F1-general", [400]))
    for m in EDGES:
        out.append((f"equal-{m}", [m] * 5))
        out.append((f"equal-{m}-with-stubs", [0, m, 1, m]))
    out.append(("every-length", list(range(0, 300))))
    out.append(("unsorted-edges", [1, 233, 62, 0, 127, 63, 232, 126, 2]))
    return out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile the partition header on its own"
    exe = str(tmp_path_factory.mktemp("feat_classes") / "feat_classes_host")
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "open_vins_amd", "csrc"), os.path.join(ROOT, "tests", "host", "feat_classes_main.cpp"), "-o", exe])
    return exe


def test_partition_header_against_the_rule(program):
    batches = _batches()
    text = "".join(" ".join(str(m) for m in lengths) + "\n" for _, lengths in batches)
    res = subprocess.run([program], input=text, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=60)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    assert len(lines) == len(batches)
    for (name, lengths), line in zip(batches, lines):
        w = [int(x) for x in line.split()]
        got = [tuple(w[1 + 4 * k:5 + 4 * k]) for k in range(w[0])]
        assert len(w) == 1 + 4 * w[0], name
        assert got == cs.expected_partition(lengths), (name, got)
        assert sum(b - a for _, a, b, _ in got) == len(lengths), name
    # the documented table, per track
    by_len = dict(zip((n for n, _ in batches), lines))
    for m, k in zip(EDGES, [1, 2, 2, 3, 3, 0]):
        assert by_len[f"equal-{m}"] == f"1 {k} 0 5 {m}"
    assert by_len["all-empty"] == "1 0 0 4 0" and by_len["no-feature"] == "0" and by_len["F1"] == "1 1 0 1 9"
    assert np.array_equal([int(x) for x in by_len["unsorted-edges"].split()], [4, 0, 0, 1, 233, 3, 1, 3, 232, 2, 3, 5, 126, 1, 5, 9, 62])
