"""The engine's resource owner (csrc/devmem.hpp: device buffers, pinned memory, events and streams, released by
lifetime group) without a GPU: tests/cpp/devmem_check.cpp is compiled once as host code under AddressSanitizer
and UBSan and drives DevOwnerT over a counting fake backend (malloc memory, a k-th call that fails, an abort on
a double or unknown free).  And a source check: no other file of csrc/ reaches the runtime's allocate / create /
free / destroy entries."""
from __future__ import annotations

import functools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
CSRC = os.path.join(ROOT, "visual_inertial_bundle_adjustment_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# host code only, and the sanitizers on the host side only (-Xarch_host): nothing here is built for or run on a GPU
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
FLAGS = ["-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", *SANITIZE]

CASES = ["scope_exit", "release", "zero_length", "failure_sweep", "two_owners"]
OWNED_CALLS = ["hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree", "hipEventCreate", "hipEventCreateWithFlags",
               "hipEventDestroy", "hipStreamCreateWithFlags", "hipStreamDestroy"]


@functools.lru_cache(maxsize=None)
def checker():
    os.makedirs(REF, exist_ok=True)
    obj, exe = os.path.join(REF, "devmem_check.o"), os.path.join(REF, "devmem_check")
    subprocess.check_call([HIPCC, *FLAGS, "-c", os.path.join(ROOT, "tests", "cpp", "devmem_check.cpp"), "-o", obj])
    subprocess.check_call([HIPCC, *SANITIZE, "-o", exe, obj])
    return exe


@pytest.mark.parametrize("case", CASES)
def test_owner_case(case):
    r = subprocess.run([checker(), case], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_unknown_case_is_an_error():
    """(a misspelt case name must not pass as an empty check)"""
    assert subprocess.run([checker(), "no_such_case"], capture_output=True).returncode == 2


def test_only_the_owner_calls_the_runtimes_allocators():
    call = re.compile(r"\b(" + "|".join(OWNED_CALLS) + r")\s*\(")
    found = []
    for name in sorted(os.listdir(CSRC)):
        if name == "devmem.hpp" or not name.endswith((".hip", ".hpp", ".h", ".cpp")):
            continue
        with open(os.path.join(CSRC, name), encoding="utf-8") as fh:
            for no, line in enumerate(fh, 1):
                if call.search(line):
                    found.append(f"{name}:{no}: {line.strip()}")
    assert not found, "\n".join(found)
    with open(os.path.join(CSRC, "devmem.hpp"), encoding="utf-8") as fh:
        assert len(call.findall(fh.read())) >= len(set(OWNED_CALLS)) - 2  # (the check does see calls where they are)
