"""What paxisim_create decides before it touches the device (paxi_amd/csrc/create_plan.h, DESIGN.md
§5) is pure host arithmetic.  tests/create_plan_check.cpp is a stand-alone program around it - built
here with the HIP compiler in host-only mode (paxisim_dev.h needs HIP's vector types) and the address
and undefined-behaviour sanitizers, and run as its own process, no GPU - that runs the plan on every
case of tests/golden/create_plan.txt, recorded from the library before paxisim_create was split, and
compares every recorded output (each Params scalar, each arena offset, the schedule, the pools) or
the refusal's code and message; then checks the plan's invariants on those cases and on a denser
grid of shapes: arena regions aligned, disjoint and inside the arena with rec last at zero_bytes,
the sizing and binding passes equal, G * lds_bytes within the LDS, C a multiple of 64 * G, the
co-located WPaxos block's strides, one pool whenever the handle cannot run two."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_create_plan_program(tmp_path):
    assert shutil.which(HIPCC), f"no HIP compiler at {HIPCC}"
    exe = str(tmp_path / "create_plan_check")
    cmd = [HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-Wall",
           "-Wextra", "-Werror", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "paxi_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "create_plan_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "create_plan.txt")], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "create_plan OK" in r.stdout
