"""The device message trace without a device: the yardstick tests/trace_ref.py
against paxi_amd.trace.capture, trace.from_rows against the yardstick, the library's new symbols,
and self-checks that the shapes of tests/test_trace_device_gpu.py contain what they are meant to
exercise."""
import ctypes as C
import os
import re
import subprocess

import pytest

import oracle_lib
import trace_ref
from paxi_amd import abi, trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["paxisim_trace_enable", "paxisim_trace_read", "paxisim_trace_totals"]


@pytest.mark.parametrize("case", ["paxos", "wpaxos", "abd", "m2paxos", "kpaxos", "epaxos", "crash"])
def test_capture_many_equals_capture(case):
    """Message for message what trace.capture records for each cluster on a fresh handle."""
    steps = 100
    r = trace_ref.ref(case, trace_ref.PROTO_TRACED, (steps,))
    for c in trace_ref.PROTO_TRACED[1:3]:
        cfg, wl, fp, faults = trace_ref.CASES[case]()
        o = oracle_lib.OracleSim(cfg, wl, fp, faults)
        tr = trace.capture(o, c, steps)
        o.close()
        assert len(tr["msgs"]) > 100
        assert tr["msgs"] == r.msgs[c], f"{case}: cluster {c}"
    assert not r.poisoned


@pytest.mark.parametrize("case", ["paxos", "epaxos", "crash"])
def test_from_rows_reproduces_the_yardstick(case):
    steps = 100
    r = trace_ref.ref(case, trace_ref.PROTO_TRACED, (steps,))
    N = abi.n_replicas(trace_ref.CASES[case]()[0])
    for c in trace_ref.PROTO_TRACED:
        rows = trace_ref.rows_of(r.msgs[c], N)
        for row in rows:                                       # the order paxisim_trace_read promises
            assert [x[:2] for x in row] == sorted(x[:2] for x in row)
        got = trace.from_rows(N, [(row, 0) for row in rows], 0, steps)
        assert got == {"N": N, "t0": 0, "steps": steps, "msgs": r.msgs[c]}
        # a window: the yardstick filtered to those steps
        got = trace.from_rows(N, [(row, 0) for row in rows], 40, 50)
        assert got["msgs"] == [m for m in r.msgs[c] if 40 <= m[0] < 90]
        # a row cut to 16 records is no whole trace
        assert all(len(row) > 16 for row in rows)
        cut = [(row[:16], len(row) - 16) for row in rows]
        with pytest.raises(trace.TraceError):
            trace.from_rows(N, cut, 0, steps)
        part = trace.from_rows(N, cut, 0, steps, truncated=True)
        assert sum(len(m[3]) for m in part["msgs"]) == 16 * N
        flat = [(m[0], m[2], rec) for m in r.msgs[c] for rec in m[3]]
        assert all((m[0], m[2], rec) in flat for m in part["msgs"] for rec in m[3])


def test_library_exports_the_trace_symbols():
    lib = os.path.join(ROOT, "paxi_amd", "libpaxisim.so")
    assert os.path.exists(lib), "build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (paxisim_\w+)", out))
    assert set(SYMBOLS) <= exported
    from paxi_amd import sim
    assert set(SYMBOLS) <= set(sim.EXPORTED)
    hdr = open(os.path.join(ROOT, "include", "paxisim.h")).read()
    assert int(re.search(r"#define PAXISIM_TRACE_MAX_CLUSTERS \(1u << (\d+)\)", hdr).group(1)) == \
        abi.TRACE_MAX_CLUSTERS.bit_length() - 1
    assert int(re.search(r"#define PAXISIM_TRACE_MAX_RECORDS  \(1u << (\d+)\)", hdr).group(1)) == \
        abi.TRACE_MAX_RECORDS.bit_length() - 1
    assert C.sizeof(abi.TraceRecord) == 24
    assert re.search(r"#define PAXISIM_ABI_VERSION\s+14\b", hdr) and abi.ABI_VERSION == 14


def test_trace_calls_refuse_a_null_handle():
    """No device is needed: the argument checks come first."""
    from paxi_amd import sim
    L = sim.load_library()
    ids = (C.c_uint64 * 1)(0)
    n, d = C.c_uint32(), C.c_uint32()
    k, lost = C.c_uint64(), C.c_uint64()
    assert L.paxisim_trace_enable(None, ids, 1, 16, 0, 10) == abi.EINVAL
    assert b"null" in L.paxisim_last_error()
    assert L.paxisim_trace_read(None, 0, 0, None, 0, C.byref(n), C.byref(d)) == abi.EINVAL
    assert L.paxisim_trace_totals(None, C.byref(k), C.byref(lost)) == abi.EINVAL


# ---- input self-checks: the GPU tests cannot pass vacuously -------------------------------------
def test_the_paxos_shape_fills_every_traced_row():
    """Test 1's shape in its step() calls; with records_per_replica = 16 (test 4) every row overflows."""
    r = trace_ref.ref("paxos", trace_ref.TILE_EDGE, trace_ref.CHUNKS)
    for c in trace_ref.TILE_EDGE:
        rows = trace_ref.rows_of(r.msgs[c], 5)
        assert all(len(row) > 16 for row in rows), [len(row) for row in rows]
        fwd = [m for m in r.msgs[c] if m[1] < 5 and (m[3][0][1] & 0xFF) == trace.T_REQUEST]   # replica to leader
        assert fwd, "no forwarded request"
    edges = [c for c in trace_ref.TILE_EDGE if {40, 89, 90} <= {m[0] for m in r.msgs[c]}]
    assert len(edges) >= 4, edges                              # test 5's window has records at both edges
    assert r.stats["dropped"] > 0, "no Drop window opened"


def test_the_crash_shape_has_p1b_payloads_crashed_inboxes_and_a_queued_late_start():
    r = trace_ref.ref("crash", trace_ref.CRASH_TRACED, trace_ref.CHUNKS)
    N, late = 5, trace_ref.LATE_AT
    p1b = crashed = behind = 0
    for c in trace_ref.CRASH_TRACED:
        for (t, src, dst, recs) in r.msgs[c]:
            p1b += (recs[0][1] & 0xFF) == trace.T_P1B and len(recs) > 1
            crashed += dst == 0 and src < N and trace_ref.CRASH_FROM <= t < trace_ref.CRASH_TO
        q = [m[3][0][4] for m in r.msgs[c] if m[0] == late and m[2] == 1 and m[1] == N]
        behind += len(q) >= 2 and q[-1] == 3 and q[0] != 3      # worker 2's first command id is 3
    assert p1b > 0, "no P1b with payload records"
    assert crashed > 0, "no record at the crashed replica"
    assert behind > 0, "the late worker's request is never behind a queued one"
    assert sum(s[12] for s in r.states) > 0, "nothing was discarded at Recv"


def test_the_multi_record_shapes_have_multi_record_messages():
    r = trace_ref.ref("epaxos", trace_ref.PROTO_TRACED, trace_ref.PROTO_STEPS)
    assert any(len(m[3]) > 1 for c in trace_ref.PROTO_TRACED for m in r.msgs[c])
    assert r.stats["dropped"] > 0
