"""td_box_pairs_ab and td_match_greedy under AddressSanitizer + UndefinedBehaviorSanitizer in a program of its own
(treedetection_amd/csrc/checks/evaluation_check.cpp, ``make -C treedetection_amd/csrc evaluation-check``): random and degenerate box
sets against the pair rule over all pairs, random and malformed sparse IoU matrices against a dense restatement of the reference's
matching loop, in exact-size heap buffers. The program links the sanitizers' runtimes statically; nothing is preloaded and nothing is
loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_evaluation_host_code_in_a_sanitized_program_of_its_own():
    import treedetection_amd.evaluation  # noqa: F401  (the stage under test exists)
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    lib = subprocess.run(["g++", "-print-file-name=libasan.a"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(lib) or not os.path.exists(lib):
        pytest.skip("libasan not installed")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "treedetection_amd", "csrc"), "evaluation-check"], capture_output=True, text=True,
                       timeout=300)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert "evaluation_check: ok" in r.stdout and "ERROR: AddressSanitizer" not in tail and "runtime error" not in tail
