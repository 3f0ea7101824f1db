"""The host side of snapshot / restore / fork (paxi_amd/csrc/snapshot_plan.h) is
pure host arithmetic.  tests/snapshot_plan_check.cpp is a stand-alone program around it - built here
with the HIP compiler in host-only mode and the address and undefined-behaviour sanitizers, run as
its own process, no GPU.  The other tests pin the documented blob format: a header built here with
struct.pack from the layout in include/paxisim_snapshot.h is what paxisim_snapshot_info of
libpaxisim.so reads, with no device."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from paxi_amd import abi, sim, snapshot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SYMBOLS = ["paxisim_snapshot_size", "paxisim_snapshot", "paxisim_restore", "paxisim_fork", "paxisim_snapshot_info"]


def test_snapshot_plan_program(tmp_path):
    assert shutil.which(HIPCC), f"no HIP compiler at {HIPCC}"
    exe = str(tmp_path / "snapshot_plan_check")
    cmd = [HIPCC, "--offload-arch=gfx950", "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-Wall",
           "-Wextra", "-Werror", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "paxi_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "snapshot_plan_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "snapshot_plan OK" in r.stdout


def header(sections, *, magic=b"PXSSNAP\0", version=1, header_bytes=256, build=b"feedfacecafebeef", plan_hash=0x1122334455667788,
           total=None, protocol=abi.WPAXOS, n=9, clusters=1000, base=4096, step=37, records=None, lat=64, ch=0, mv=8,
           tr=(0, 0, 0, 0), faults=2, pools=1, words=None):
    """The 256-byte header, field by field as include/paxisim_snapshot.h documents it."""
    sections = list(sections)
    total = header_bytes + sum(sections) if total is None else total
    records = sections[4] // 16 if records is None else records
    words = sections[0] // 8 if words is None else words
    recorders = (1 if lat else 0) | (2 if ch else 0) | (4 if mv else 0) | (8 if tr[0] else 0)
    h = struct.pack("<8sII32sQQIIQQIIQ9Q10I40s", magic, version, header_bytes, build, plan_hash, total, protocol, n,
                    clusters, base, step, recorders, records, *sections, lat, ch, mv, tr[0], tr[1], tr[2], tr[3],
                    faults, pools, words, b"")
    assert len(h) == 256
    return h


SECTIONS = (8 * 90, 2 * 48, 48, 4096, 16 * 123, 1000, 0, 64, 0)


def blob_of(h, sections=SECTIONS):
    return np.frombuffer(h + bytes(sum(sections)), dtype=np.uint8)


def test_info_reads_the_documented_header_without_a_device():
    i = snapshot.info(blob_of(header(SECTIONS)))
    assert i["version"] == 1 and i["protocol"] == abi.WPAXOS and i["N"] == 9 and i["clusters"] == 1000
    assert i["cluster_base"] == 4096 and i["step"] == 37 and i["build_id"] == "feedfacecafebeef"
    assert i["plan_hash"] == 0x1122334455667788 and i["mailbox_records"] == 123 and i["faults"] == 2
    assert i["recorders"] == {"latency": True, "client_history": False, "multiversion": True, "trace": False}
    assert i["sections"] == dict(zip(abi.SNAPSHOT_SECTIONS, SECTIONS))
    assert i["total_bytes"] == 256 + sum(SECTIONS)
    assert list(abi.SNAPSHOT_SECTIONS) == ["plan", "faults", "pools", "arena", "mailbox", "lat", "chist", "mv", "trace"]


@pytest.mark.parametrize("kw, msg", [
    (dict(magic=b"PXSSNAQ\0"), "bad magic"),
    (dict(version=2), "snapshot version 2, this library reads version 1"),
    (dict(header_bytes=512), "header_bytes"),
    (dict(total=256 + sum(SECTIONS) + 1), "add up"),
    (dict(records=122), "section mailbox"),
    (dict(words=89), "section plan"),
    (dict(faults=3), "section faults"),
    (dict(pools=2), "section pools"),
    (dict(pools=0), "section pools"),
    (dict(lat=0), "recorders word"),
    (dict(build=b"x" * 32), "not terminated"),
])
def test_info_refuses(kw, msg):
    h = header(SECTIONS, **kw)
    if "lat" in kw:   # the sizes say "no latency recorder", the recorders word says there is one
        h = h[:92] + struct.pack("<I", 5) + h[96:]
    with pytest.raises(sim.PaxisimError, match=msg):
        snapshot.info(blob_of(h))


def test_info_refuses_truncation_and_excess():
    b = blob_of(header(SECTIONS))
    for n in (0, 1, 255, 256, 257, len(b) - 1):
        with pytest.raises(sim.PaxisimError, match="truncated"):
            snapshot.info(b[:n].copy())
    with pytest.raises(sim.PaxisimError, match="add up"):
        snapshot.info(np.concatenate([b, np.zeros(1, np.uint8)]))
    with pytest.raises(sim.PaxisimError, match="null argument"):
        sim._check(sim.load_library().paxisim_snapshot_info(None, 0, C.byref(abi.SnapshotInfo())))
    with pytest.raises(sim.PaxisimError, match="null argument"):
        sim._check(sim.load_library().paxisim_snapshot_info(b.ctypes.data_as(C.c_void_p), len(b), None))


def test_save_and_load_are_the_raw_blob(tmp_path):
    b = blob_of(header(SECTIONS))
    p = str(tmp_path / "s.snap")
    snapshot.save(p, b)
    assert open(p, "rb").read() == b.tobytes()
    assert (snapshot.load(p) == b).all() and snapshot.load(p).dtype == np.uint8


def test_header_file_python_and_library_agree(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "paxisim_snapshot.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", sim.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in exported and name in sim.EXPORTED, name
    assert {n for n in abi.PROTOTYPES if re.search(r"(?m)^int %s\(" % n, hdr)} == set(SYMBOLS)   # the declarations
    assert "#define PAXISIM_SNAPSHOT_SECTIONS %d" % len(abi.SNAPSHOT_SECTIONS) in hdr
    assert "#define PAXISIM_SNAPSHOT_HEADER   %d" % abi.SNAPSHOT_HEADER in hdr
    # the ABI version and paxisim.h itself are the parent's: the step units and the guard's pinned header stay as they are
    assert sim.load_library().paxisim_abi_version() == 14
    # plain C takes the header (the info struct is a tag, the parser a function of the same name) and
    # lays the struct out as ctypes does
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "paxisim_snapshot.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(struct paxisim_snapshot_info), '
                   'offsetof(struct paxisim_snapshot_info, mailbox_records), '
                   'offsetof(struct paxisim_snapshot_info, section_bytes), '
                   'offsetof(struct paxisim_snapshot_info, build_id)); return 0; }\n')
    exe = str(tmp_path / "probe")
    b = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    S = abi.SnapshotInfo
    assert got == [C.sizeof(S), S.mailbox_records.offset, S.section_bytes.offset, S.build_id.offset]
