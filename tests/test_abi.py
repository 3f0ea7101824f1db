"""CPU-side checks of the C-ABI boundary: the HIP library loads and exports
every symbol include/paxisim.h declares (no compute calls without a GPU)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "paxisim.h")).read()
    return sorted(set(re.findall(r"\b(paxisim_[a-z_]+)\s*\(", hdr)))


def test_header_declares_api():
    syms = declared_symbols()
    for s in ["paxisim_create", "paxisim_step", "paxisim_stats_get", "paxisim_read_state",
              "paxisim_check", "paxisim_destroy", "paxisim_last_error", "paxisim_fault_add"]:
        assert s in syms


def test_library_exports_all_declared():
    from paxi_amd import sim
    lib = os.path.join(ROOT, "paxi_amd", "libpaxisim.so")
    assert os.path.exists(lib), "build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (paxisim_\w+)", out))
    missing = [s for s in declared_symbols() if s not in exported]
    assert not missing, missing
    assert set(sim.EXPORTED) <= exported


def test_library_loads_and_reports_version():
    from paxi_amd import abi, sim
    L = sim.load_library()
    assert L.paxisim_abi_version() == abi.ABI_VERSION


# the ABI structs: C name -> ctypes class (include/paxisim.h, paxisim_snapshot.h)
def abi_structs():
    from paxi_amd import abi
    return {"paxisim_config": abi.Config, "paxisim_workload": abi.Workload, "paxisim_fault_process": abi.FaultProcess,
            "paxisim_fault": abi.Fault, "paxisim_replica_state": abi.ReplicaState,
            "paxisim_instance_state": abi.InstanceState, "paxisim_log_entry": abi.LogEntry,
            "paxisim_inbox_record": abi.InboxRecord, "paxisim_trace_record": abi.TraceRecord,
            "paxisim_worker_state": abi.WorkerState, "paxisim_latency": abi.Latency,
            "paxisim_latency_stat": abi.LatencyStat, "paxisim_stats": abi.Stats,
            "paxisim_snapshot_info": abi.SnapshotInfo}


HEADERS = ["include/paxisim.h", "include/paxisim_snapshot.h", "include/paxisim_verdict.h", "include/paxisim_shape.h",
           "oracle/oracle.h"]


def header_prototypes():
    """{name: (return type, [parameter types])} of every paxisim_* / oracle_* function the headers
    declare, as C type strings without `const`, `struct`, blanks and parameter names."""
    def ctype(words, name_last):
        words = [w for w in words.replace("*", " * ").split() if w not in ("const", "struct")]
        if name_last:                                   # `uint64_t counts[32]` is the type uint64_t[32]
            dim = re.search(r"\[\d+\]$", words[-1])
            words[-1] = dim.group(0) if dim else ""
        return "".join(words)
    found = {}
    for h in HEADERS:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(os.path.join(ROOT, h)).read(), flags=re.S)
        for ret, name, params in re.findall(r"([\w \t*]+?)\b((?:paxisim|oracle)_\w+)\s*\(([^()]*)\)\s*;", text):
            assert name not in found, name
            params = [] if params.strip() == "void" else [ctype(p, True) for p in params.split(",")]
            found[name] = (ctype(ret, False), params)
    return found


def test_table_matches_every_header_declaration():
    """abi.PROTOTYPES, the binding's single source, against the headers: the same 60 + 25 names, and
    for each the return type and every parameter type under one fixed map of C types to ctypes."""
    from paxi_amd import abi, sim
    P = ctypes.POINTER
    handles = ("paxisim", "paxisim_dist", "oracle_sim")
    cmap = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
            "double": ctypes.c_double, "char*": ctypes.c_char_p, "void*": ctypes.c_void_p,
            "uint32_t*": P(ctypes.c_uint32), "uint64_t*": P(ctypes.c_uint64), "int64_t*": P(ctypes.c_int64),
            "double*": P(ctypes.c_double), "int*": P(ctypes.c_int),
            "unsignedchar[128]": ctypes.c_char_p, "uint64_t[32]": P(ctypes.c_uint64)}
    cmap.update({h + "*": ctypes.c_void_p for h in handles})
    cmap.update({h + "**": P(ctypes.c_void_p) for h in handles})
    cmap.update({c + "*": P(cls) for c, cls in abi_structs().items()})
    declared = header_prototypes()
    assert set(declared) == set(abi.PROTOTYPES)
    assert len([n for n in declared if n.startswith("paxisim_")]) == 60 and len(declared) == 85
    assert sorted(sim.EXPORTED) == sorted(n for n in declared if n.startswith("paxisim_"))
    for name, (ret, params) in declared.items():
        res, args = abi.PROTOTYPES[name]
        assert res is cmap[ret], name
        assert args == [cmap[p] for p in params], (name, params)
    assert not set(abi.DEBUG_PROTOTYPES) & set(declared)


def test_loaded_libraries_carry_the_table():
    """Every call of the table is bound on the library that has it, under the table's types."""
    import oracle_lib
    from paxi_amd import abi, sim
    for L, prefix in ((sim.load_library(), "paxisim_"), (oracle_lib.lib(), "oracle_")):
        assert L.missing == []
        names = [n for n in abi.PROTOTYPES if n.startswith(prefix)]
        assert len(names) == {"paxisim_": 60, "oracle_": 25}[prefix]
        for name in names:
            fn = getattr(L, name)
            assert fn.restype is abi.PROTOTYPES[name][0] and fn.argtypes == abi.PROTOTYPES[name][1], name
            assert getattr(L, name[len(prefix):]) is fn
    # abi.declare: the same prototypes on a ctypes library the caller keeps
    raw = ctypes.CDLL(oracle_lib.ORACLE_SO)
    assert abi.declare(raw, "oracle") is raw
    for name in names:
        assert getattr(raw, name).argtypes == abi.PROTOTYPES[name][1], name
    with pytest.raises(AttributeError):
        raw.oracle_no_such_call


def test_struct_layout_matches_header(tmp_path):
    """Compile a C probe generated from the _fields_ lists against the headers and compare sizeof of all
    14 structs, and offsetof and the size of every field, with ctypes."""
    structs = abi_structs()
    lines, want = [], []
    for cname, cls in structs.items():
        t = ("struct " if cname == "paxisim_snapshot_info" else "") + cname
        lines.append(f'printf("%zu\\n", sizeof({t}));')
        want.append(ctypes.sizeof(cls))
        for field, _ in cls._fields_:
            lines.append(f'printf("%zu %zu\\n", offsetof({t}, {field}), sizeof((({t}*)0)->{field}));')
            want += [getattr(cls, field).offset, getattr(cls, field).size]
    assert len(structs) == 14 and len(want) == 314
    src = tmp_path / "p.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "paxisim.h"\n#include "paxisim_snapshot.h"\n'
                   "int main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "p"), str(src)], check=True)
    out = subprocess.run([str(tmp_path / "p")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == want


STUB = r"""
#include "paxisim.h"
int paxisim_abi_version(void) { return PAXISIM_ABI_VERSION; }
const char* paxisim_last_error(void) { return ""; }
const char* paxisim_build_id(void) { return "stub"; }
int paxisim_create(const paxisim_config* cfg, const paxisim_workload* wl, const paxisim_fault_process* fp,
                   paxisim** out) { (void)cfg; (void)wl; (void)fp; (void)out; return PAXISIM_EDEVICE; }
"""
STUB_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import pytest
from paxi_amd import abi, sim
L = sim.load_library()
assert sim.LIB_PATH == sys.argv[2] and len(L.missing) == 56 and len(sim.EXPORTED) == 60
assert sim.build_id() == "stub"
with pytest.raises(sim.PaxisimError, match="error -3"):
    sim.Simulation(abi.make_config(clusters=4), abi.make_workload())
s = object.__new__(sim.Simulation)
s.h = None
for call, name in ((lambda: sim.select_words([1], 1), "paxisim_select_words"),
                   (s.latency_reset, "paxisim_latency_reset"), (s.check, "paxisim_check"),
                   (lambda: s.step(1), "paxisim_step"), (lambda: sim.quorum(abi.make_config(), 0, 1), "paxisim_quorum")):
    with pytest.raises(sim.PaxisimError) as e:
        call()
    assert str(e.value) == f"{sys.argv[2]} was built without {name}", str(e.value)
with pytest.raises(AttributeError):
    L.paxisim_no_such_call
print("stub ok")
"""


def test_a_library_without_a_call_raises_where_it_is_looked_up(tmp_path):
    """A library built from older sources lacks the newer calls (the miscompile guard's pinned
    reproducers): it loads, and a call through a missing name raises PaxisimError naming the library and the call."""
    import sys
    (tmp_path / "stub.c").write_text(STUB)
    lib = str(tmp_path / "libstub.so")
    subprocess.run(["gcc", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), "-o", lib, str(tmp_path / "stub.c")],
                   check=True)
    out = subprocess.run([sys.executable, "-c", STUB_CHILD, ROOT, lib], env=dict(os.environ, PAXISIM_LIB=lib),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("stub ok"), out.stderr[-2000:]


def test_create_without_gpu_fails_loudly():
    """No device here: the product path must refuse, never fall back to the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from paxi_amd import abi, sim
    with pytest.raises(sim.PaxisimError):
        sim.Simulation(abi.make_config(clusters=4), abi.make_workload())


def test_quorum_predicates_match_the_oracle():
    """paxisim_quorum (the kernels' own predicate, built for the host) equals the
    oracle's restatement of quorum.go:55-119 for every kind, mask and layout."""
    import oracle_lib as ol
    from paxi_amd import abi, sim
    for npz in ([3], [5], [2, 2], [3, 3, 3], [2, 3, 4], [4, 4, 4, 4]):
        for fz in (0, 1, 2):
            cfg = abi.make_config(npz=npz, fz=fz)
            n = sum(npz)
            masks = range(1 << n) if n <= 9 else range(0, 1 << n, 37)
            for kind in range(8):
                for m in masks:
                    assert sim.quorum(cfg, kind, m) == ol.quorum(kind, npz, m, fz), (npz, fz, kind, m)
