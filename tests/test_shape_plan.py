"""Which handles run the fixed-shape unit (paxi_amd/csrc/shape_plan.h) is decided on
the host.  tests/shape_plan_check.cpp is a stand-alone program around that header and the create
plan - built here for the host only, with the address and undefined-behaviour sanitizers, and run as
its own process - that checks: the headline's exact config fits; every single departure from it, one
case per pinned field (N, Z, window, q1, q2, thrifty, ephemeral_leader, reply_when_commit, kv, a
scripted fault, a late worker, max_requests, each non-uniform distribution, locality, moving keys,
PAXISIM_SERIAL=0, PAXISIM_SHAPE=0), does not, names that field, and shows in the Params that
fill_params writes; and PAXISIM_SHAPE reads 1 / 0 and refuses anything else."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_shape_plan_program(tmp_path):
    assert shutil.which(HIPCC), f"no HIP compiler at {HIPCC}"
    exe = str(tmp_path / "shape_plan_check")
    cmd = [HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-Wall",
           "-Wextra", "-Werror", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "paxi_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "shape_plan_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    env = {k: v for k, v in os.environ.items() if not k.startswith("PAXISIM_")}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "shape_plan OK" in r.stdout


def test_shape_header_is_host_only():
    """shape_plan.h takes the C ABI's structs and nothing of HIP, as pool_plan.h."""
    text = open(os.path.join(ROOT, "paxi_amd", "csrc", "shape_plan.h")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<stdint.h>", '"../../include/paxisim.h"']


def test_paxisim_h_unchanged_and_symbol_listed():
    from paxi_amd import abi, sim
    assert "paxisim_step_unit" in sim.EXPORTED
    assert callable(getattr(sim.Simulation, "step_unit", None))
    hdr = open(os.path.join(ROOT, "include", "paxisim_shape.h")).read()
    assert "PAXISIM_UNIT_GENERIC      = %d" % abi.UNIT_GENERIC in hdr
    assert "PAXISIM_UNIT_FIXED_PAXOS5 = %d" % abi.UNIT_FIXED_PAXOS5 in hdr
    assert "paxisim_step_unit" not in open(os.path.join(ROOT, "include", "paxisim.h")).read()
    assert abi.ABI_VERSION == 14
