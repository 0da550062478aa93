"""td_treetops under AddressSanitizer + UndefinedBehaviorSanitizer in a program of its own
(treedetection_amd/csrc/checks/treetops_check.cpp, ``make -C treedetection_amd/csrc treetops-check``): random, plateau and non-finite
rasters in exact-size heap buffers against a restatement of the rule, 1 x 1 rasters and rasters narrower than the radius, windows
wider than the raster, crafted spikes, malformed calls. The program links the sanitizers' runtimes statically; nothing is preloaded
and nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_treetops_in_a_sanitized_program_of_its_own():
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    lib = subprocess.run(["g++", "-print-file-name=libasan.a"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(lib) or not os.path.exists(lib):
        pytest.skip("libasan not installed")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "treedetection_amd", "csrc"), "treetops-check"], capture_output=True, text=True,
                       timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "treetops_check: ok" in r.stdout and "ERROR: AddressSanitizer" not in tail and "runtime error" not in tail
