"""The LM controller (csrc/lm_controller.hpp: the decisions of Optimizer.cpp:834-1097 that vb_optimize and the
multi-process controllers run) without a GPU: tests/cpp/lm_check.cpp is compiled once as host code under
AddressSanitizer and UBSan and drives lmRun, and the plain-C table behind vb_lm_run, with scripted primitives.
Each case compares the exact sequence of primitive calls, the damping passed to every iteration, the step
factors and the final summary with values written out by hand in the program; a difference is printed and the
program exits 1."""
from __future__ import annotations

import functools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# host code only, and the sanitizers on the host side only (-Xarch_host): nothing here is built for or run on a GPU
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
FLAGS = ["-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", *SANITIZE]

CASES = ["tolerances", "max_iterations", "hold_off", "troubled", "damping_max", "rescale_first", "rescale_sub_step",
         "rescale_all_fail", "negative_model_reduction", "errors"]


@functools.lru_cache(maxsize=None)
def checker():
    os.makedirs(REF, exist_ok=True)
    obj, exe = os.path.join(REF, "lm_check.o"), os.path.join(REF, "lm_check")
    subprocess.check_call([HIPCC, *FLAGS, "-c", os.path.join(ROOT, "tests", "cpp", "lm_check.cpp"), "-o", obj])
    subprocess.check_call([HIPCC, *SANITIZE, "-o", exe, obj])
    return exe


@pytest.mark.parametrize("case", CASES)
def test_lm_controller_case(case):
    r = subprocess.run([checker(), case], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_unknown_case_is_an_error():
    """(a misspelt case name must not pass as an empty check)"""
    assert subprocess.run([checker(), "no_such_case"], capture_output=True).returncode == 2
