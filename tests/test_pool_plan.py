"""The launch planner of paxisim_step (paxi_amd/csrc/pool_plan.h) is a pure host
header.  tests/pool_plan_check.cpp is a stand-alone program around it - built here with the host
compiler and the address and undefined-behaviour sanitizers, and run as its own process - that
checks, over a grid of (t, nsteps, S, pipe_max, cmp_every, late_until) that includes the headline
shape (S=20, pipe_max=4, cmp_every=60, calls of 400) and odd call lengths (1, 19, 61, 137):
both pools end every call at t + nsteps; no launch crosses a due compaction of its pool or exceeds
pipe_max chunks; one pool reproduces the loop paxisim_step ran before pools, restated directly;
and the pools' compactions stay one chunk apart."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if cxx and shutil.which(cxx):
            return cxx
    return None


def test_pool_plan_program(tmp_path):
    cxx = _compiler()
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path / "pool_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "paxi_amd", "csrc"),
           "-o", exe, os.path.join(ROOT, "tests", "pool_plan_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "pool_plan OK" in r.stdout
