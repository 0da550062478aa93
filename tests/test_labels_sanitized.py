"""td_crown_labels under AddressSanitizer + UndefinedBehaviorSanitizer in a program of its own
(treedetection_amd/csrc/checks/labels_check.cpp, ``make -C treedetection_amd/csrc labels-check``): crafted and overlapping rings with
known pixel sets drawn into exact-size heap buffers, rings off every side of the raster and 1e300 away, a 1 x 1 raster, rings of
0 - 2 vertices, starts outside xy, non-finite coordinates, malformed calls. The program links the sanitizers' runtimes statically;
nothing is preloaded and nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_crown_labels_in_a_sanitized_program_of_its_own():
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    lib = subprocess.run(["g++", "-print-file-name=libasan.a"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(lib) or not os.path.exists(lib):
        pytest.skip("libasan not installed")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "treedetection_amd", "csrc"), "labels-check"], capture_output=True, text=True,
                       timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "labels_check: ok" in r.stdout and "ERROR: AddressSanitizer" not in tail and "runtime error" not in tail
