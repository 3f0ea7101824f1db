"""Message traces recorded on the device (trace_kernel.h) against the oracle-derived
yardstick of tests/trace_ref.py: every traced cluster's trace message for message, in every kernel
form and for every protocol, and the replica states, stats, latencies and client histories those of
a run without tracing and of the oracle."""
import pytest

import client_history_ref
import latency_ref
import mv_ref
import oracle_lib
import trace_ref
from paxi_amd import abi, trace
from paxi_amd.sim import PaxisimError, Simulation

pytestmark = pytest.mark.gpu
EINVAL, ERANGE = r"error -1:", r"error -5:"
BINS, CHIST, CAP = 64, 128, 8192
KEEP = lambda t: t[:11] + t[12:14] + t[15:]   # replica state minus dropped and replies (a replay drops every send)


def _has_chist(cfg):
    return cfg.protocol == abi.ABD or bool(cfg.kv)


def _sim(shape, traced=None, cap=CAP, window=(), chist=True):
    cfg, wl, fp, faults = shape
    g = Simulation(cfg, wl, fp, faults)
    g.latency_enable(BINS)
    if chist and _has_chist(cfg):
        g.client_history_enable(CHIST)
    if traced is not None:
        g.trace_enable(traced, cap, *window)
    return g


def _observe(g, traced):
    workers = [None] + list(range(g.wl.outstanding))
    return ([s.as_tuple() for s in g.read_state()], g.stats().as_dict(), [g.latency(w) for w in workers],
            [g.client_history(c) for c in traced] if _has_chist(g.cfg) else None)


def _expected(r, wl, cfg, traced):
    workers = [None] + list(range(wl.outstanding))
    return (r.states, r.stats, [latency_ref.expected(r, BINS, w) for w in workers],
            [(client_history_ref.canonical(r.hist[c]), 0) for c in traced] if _has_chist(cfg) else None)


def _same(got, want, ctx):
    for k, what in enumerate(("replica states", "stats", "latencies", "client histories")):
        assert got[k] == want[k], f"{ctx}: {what} differ"


def _check_case(name, traced, chunks):
    """Trace `traced` of shape `name` over the step() calls `chunks`; returns the yardstick."""
    r = trace_ref.ref(name, traced, chunks)
    shape = trace_ref.CASES[name]()
    cfg, wl = shape[0], shape[1]
    with _sim(shape) as g:                                    # tracing off
        for n in chunks:
            g.step(n)
        plain = _observe(g, traced)
    with _sim(trace_ref.CASES[name](), traced) as g:
        for n in chunks:
            g.step(n)
        for c in traced:
            got = trace.from_device(g, c)
            assert got["steps"] == sum(chunks) and got["N"] == g.N
            assert len(r.msgs[c]) > 20
            assert got["msgs"] == r.msgs[c], f"{name}: trace of cluster {c}"
        kept, dropped = g.trace_totals()
        assert dropped == 0 and kept == sum(len(m[3]) for c in traced for m in r.msgs[c])
        seen = _observe(g, traced)
    _same(seen, plain, f"{name}: tracing on against off")
    _same(plain, _expected(r, wl, cfg, traced), f"{name}: against the oracle")
    return r


# ---- 1. Multi-Paxos N=5 in every kernel form ---------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"PAXISIM_SERIAL": "0"}, {"PAXISIM_PIPE": "1"}],
                         ids=["default", "serial0", "pipe1"])
def test_paxos5_every_kernel_form(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _check_case("paxos", trace_ref.TILE_EDGE, trace_ref.CHUNKS)


def test_paxos5_two_pools(monkeypatch):
    monkeypatch.setenv("PAXISIM_POOLS", "1")
    with _sim(trace_ref.paxos_pools_case()) as g:
        for n in trace_ref.CHUNKS:
            g.step(n)
        g.sync()
        one = g.kernel_time()[1]
    monkeypatch.setenv("PAXISIM_POOLS", "2")
    monkeypatch.setenv("PAXISIM_PHASE_SORT", "1")
    _check_case("pools", trace_ref.POOLS_TRACED, trace_ref.CHUNKS)
    with _sim(trace_ref.paxos_pools_case(), trace_ref.POOLS_TRACED) as g:
        for n in trace_ref.CHUNKS:
            g.step(n)
        g.sync()
        assert g.kernel_time()[1] > one                      # both pools launched


# ---- 2. Crash, P1b payloads, a late worker ------------------------------------------------------
def test_crash_p1b_payloads_and_a_late_worker():
    r = _check_case("crash", trace_ref.CRASH_TRACED, trace_ref.CHUNKS)
    late = [m for c in trace_ref.CRASH_TRACED for m in r.msgs[c]
            if m[0] == trace_ref.LATE_AT and m[1] == 5 and m[3][0][4] == 3]
    assert len(late) == len(trace_ref.CRASH_TRACED)           # the late worker's first request, in every trace


# ---- 3. Every protocol ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wpaxos", "abd", "epaxos", "m2paxos", "kpaxos"])
def test_every_protocol(name):
    r = _check_case(name, trace_ref.PROTO_TRACED, trace_ref.PROTO_STEPS)
    if name == "epaxos":
        assert any(len(m[3]) > 1 for c in trace_ref.PROTO_TRACED for m in r.msgs[c])


# ---- 4. Overflow -----------------------------------------------------------------------------------
def test_overflow_counts_and_drops():
    traced, chunks, cap = trace_ref.TILE_EDGE, trace_ref.CHUNKS, 16
    r = trace_ref.ref("paxos", traced, chunks)
    with _sim(trace_ref.paxos_case()) as g:
        for n in chunks:
            g.step(n)
        plain = _observe(g, traced)
    with _sim(trace_ref.paxos_case(), traced, cap) as g:
        for n in chunks:
            g.step(n)
        kept = lost = 0
        for c in traced:
            for dst, row in enumerate(trace_ref.rows_of(r.msgs[c], 5)):
                assert len(row) > cap
                assert g.trace_read(c, dst) == (row[:cap], len(row) - cap), f"cluster {c} replica {dst}"
                kept += cap
                lost += len(row) - cap
            with pytest.raises(trace.TraceError):
                trace.from_device(g, c)
            part = trace.from_device(g, c, truncated=True)
            assert sum(len(m[3]) for m in part["msgs"]) == 5 * cap
        assert g.trace_totals() == (kept, lost)
        _same(_observe(g, traced), plain, "16 records per replica against tracing off")   # no flag is raised
    assert plain[0] == r.states


# ---- 5. Step window --------------------------------------------------------------------------------
def test_step_window():
    traced, chunks = trace_ref.TILE_EDGE, trace_ref.CHUNKS
    r = trace_ref.ref("paxos", traced, chunks)
    with _sim(trace_ref.paxos_case(), traced, CAP, (40, 90)) as g:
        for n in chunks:
            g.step(n)
        edges = 0
        for c in traced:
            want = [m for m in r.msgs[c] if 40 <= m[0] < 90]
            got = trace.from_device(g, c)["msgs"]
            assert got == want, f"cluster {c}"
            assert not any(m[0] >= 90 or m[0] < 40 for m in got)
            edges += any(m[0] == 40 for m in got) and any(m[0] == 89 for m in got) and \
                any(m[0] == 90 for m in r.msgs[c])
        assert edges >= 4                                      # a record delivered at step 40, none of those at 90
        assert [s.as_tuple() for s in g.read_state()] == r.states


# ---- 6. Compaction and wake ------------------------------------------------------------------------
def test_compaction_and_wake_leave_the_rows_with_their_cluster(monkeypatch):
    monkeypatch.setenv("PAXISIM_COMPACT_EVERY", "16")
    make = mv_ref.SHAPES["paxos3_freeze"][0]
    N = 3
    with _sim(make()) as g:                                   # which clusters freeze: a run without tracing
        g.step(100)
        frozen = [c for c, a in enumerate(g.activity()) if a is not None]
    cfg, wl, fp, faults = make()
    assert frozen
    live = [c for c in range(cfg.clusters) if c not in frozen]
    traced = frozen[::max(1, len(frozen) // 6)][:6] + live[:2]       # two more are traced and left asleep
    if not live:
        traced += frozen[1:3]
    o = oracle_lib.OracleSim(cfg, wl, fp, faults)
    woken, cid = {}, 1 << 22
    for c in traced[:6]:
        while not o.command(c, cid)[1]:
            cid += 1
        woken[c] = cid
        cid += 1

    def inject(sim):
        for c, x in woken.items():
            sim.inject(c, c % N, x)

    r = trace_ref.capture_many(o, traced, [100, 60], before={100: inject})
    o.close()
    with _sim(make(), traced) as g:
        g.step(100)
        act = g.activity()
        assert g.active_clusters() < cfg.clusters and any(act[c] is not None for c in traced), \
            "no traced cluster froze: the row move is not exercised"
        inject(g)
        g.step(60)
        for c in traced:
            got = trace.from_device(g, c)["msgs"]
            assert got == r.msgs[c], f"cluster {c}"             # by cluster id, after rows have moved
            if c in woken:                                      # the write wakes the cluster at step 100
                assert (100, N, c % N, [(N, trace.T_REQUEST, 0, 0, woken[c])]) in got
        _same(_observe(g, traced), _expected(r, wl, cfg, traced), "after the wake, against the oracle")


# ---- 7. Inject and deliver -------------------------------------------------------------------------
def test_inject_and_deliver_between_steps():
    traced, T = trace_ref.PROTO_TRACED, 30
    base = trace_ref.ref("paxos", traced, (100,))
    N = 5
    # a P3 replica 1 has already received is delivered to it again, from the same source
    p3 = {c: [m for m in base.msgs[c] if m[2] == 1 and m[0] < T and (m[3][0][1] & 0xFF) == trace.T_P3][-1]
          for c in traced}

    def stage(sim):
        for c in traced:
            sim.deliver(c, 1, p3[c][1], p3[c][3])
            sim.inject(c, 1, (1 << 22) + c)

    shape = trace_ref.paxos_case(clusters=70)
    o = oracle_lib.OracleSim(*shape)
    r = trace_ref.capture_many(o, list(traced), [T, 40], before={T: stage})
    o.close()
    queued = 0
    with _sim(trace_ref.paxos_case(clusters=70), traced) as g:
        g.step(T)
        stage(g)
        g.step(40)
        for c in traced:
            got = trace.from_device(g, c)["msgs"]
            assert got == r.msgs[c], f"cluster {c}"
            link = [m[3] for m in got if m[0] == T and m[2] == 1 and m[1] == p3[c][1]]
            client = [m[3] for m in got if m[0] == T and m[2] == 1 and m[1] == N]
            assert link[-1] == p3[c][3] and client[-1] == [(N, trace.T_REQUEST, 0, 0, (1 << 22) + c)]
            queued += (len(link) > 1) + (len(client) > 1)
        assert [s.as_tuple() for s in g.read_state()] == r.states
    assert queued, "nothing was queued in front of the staged records"


# ---- 8. POISON ---------------------------------------------------------------------------------------
def _poison_promise(at, cluster):
    """A (replica, key) of `cluster` for which a Promise delivered before step `at` raises POISON at
    that step on the oracle: the replica never initialised the key."""
    for r in range(9):
        for key in range(6):
            o = oracle_lib.OracleSim(*trace_ref.wpaxos_case())
            if at:
                o.step(at)
            rec = [((r + 1) % 9, trace.T_P1B | (key << 16), (1 << 4) | r, 0, 0)]
            o.deliver(cluster, r, (r + 1) % 9, rec)
            o.step(1)
            hit = any(s.flags & abi.F_POISON for s in o.read_state(cluster, 1))
            o.close()
            if hit:
                return r, rec
    raise AssertionError("every replica initialised every key")


def test_poison_ends_the_trace():
    traced, T, rest = trace_ref.PROTO_TRACED, 1, 39      # by step 2 every replica has initialised every key
    stage0 = (63, *_poison_promise(0, 63))
    stageT = (64, *_poison_promise(T, 64))

    def deliver(st):
        c, rep, rec = st
        return lambda sim: sim.deliver(c, rep, rec[0][0], rec)

    o = oracle_lib.OracleSim(*trace_ref.wpaxos_case())
    r = trace_ref.capture_many(o, list(traced), [T, rest], before={0: deliver(stage0), T: deliver(stageT)})
    o.close()
    assert r.poisoned == {63: 0, 64: T}
    with _sim(trace_ref.wpaxos_case(), traced) as g:
        deliver(stage0)(g)
        g.step(T)
        deliver(stageT)(g)
        g.step(rest)
        for c in traced:
            got = trace.from_device(g, c)["msgs"]
            assert got == r.msgs[c], f"cluster {c}"
        for c, at in r.poisoned.items():
            got = trace.from_device(g, c)["msgs"]
            assert max(m[0] for m in got) == at                 # nothing after the poison step
            assert len({m[2] for m in got if m[0] == at}) > 1   # the poison step's inboxes of the other replicas too
        assert max(m[0] for m in trace.from_device(g, 62)["msgs"]) == T + rest - 1
        assert [s.as_tuple() for s in g.read_state()] == r.states
        assert g.stats().as_dict() == r.stats


# ---- 9. End to end ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["paxos", "epaxos"])
def test_device_trace_exports_imports_and_replays(name):
    cluster, steps = 64, 100
    make = trace_ref.CASES[name]
    with _sim(make(), [cluster]) as a:
        a.step(steps)
        tr = trace.from_device(a, cluster)
        streams, sched = trace.export(a, cluster, tr)
        tr2 = trace.import_streams(a, cluster, streams, sched)
        key = lambda m: (m[0], m[1], m[2], m[3])
        assert sorted(tr2["msgs"], key=key) == sorted(tr["msgs"], key=key)
        sa = [KEEP(s.as_tuple()) for s in a.read_state(cluster, 1)]
    cfg2, wl2, _, _ = make(clusters=1, base=cluster)
    faults = trace.replay_setup(wl2, abi.n_replicas(cfg2))
    with Simulation(cfg2, wl2, None, faults) as b:
        trace.replay(b, 0, tr2)
        sb = [KEEP(s.as_tuple()) for s in b.read_state(0, 1)]
    assert sa == sb
    cfg, wl, fp, faults = make()
    o = oracle_lib.OracleSim(cfg, wl, fp, faults)
    otr = trace.capture(o, cluster, steps)
    ostreams, _ = trace.export(o, cluster, otr)
    assert [KEEP(s.as_tuple()) for s in o.read_state(cluster, 1)] == sa
    o.close()
    assert len(streams) >= 4 and ostreams == streams             # the same bytes on every link


# ---- 10. Second pass on failures -------------------------------------------------------------------
def test_second_pass_traces_the_failing_clusters():
    make, schedule = mv_ref.SHAPES["epaxos5"]
    with _sim(make(), chist=False) as g:                      # pass 1: which clusters fail Consensus
        g.multiversion_enable(128)
        for n in schedule:
            g.step(n)
        masks = g.consensus_failed()
    failing = [c for c, m in enumerate(masks) if m]
    cfg, wl, fp, faults = make()
    assert 0 < len(failing) < cfg.clusters
    o = oracle_lib.OracleSim(cfg, wl, fp, faults)
    r = trace_ref.capture_many(o, failing, list(schedule), clients=False)
    o.close()
    with _sim(make(), failing, chist=False) as g:             # pass 2: a new handle traces exactly those
        g.multiversion_enable(128)
        for n in schedule:
            g.step(n)
        assert g.consensus_failed() == masks
        for c in failing:
            assert trace.from_device(g, c)["msgs"] == r.msgs[c], f"cluster {c}"
        assert [s.as_tuple() for s in g.read_state()] == r.states


# ---- 11. Errors ------------------------------------------------------------------------------------
def test_errors():
    shape = lambda: trace_ref.paxos_case(clusters=70)
    with Simulation(*shape()) as g:
        with pytest.raises(PaxisimError, match=EINVAL):
            g.trace_enable([0], 16)                            # needs the recording units
    with _sim(shape()) as g:
        for call in (lambda: g.trace_read(0, 0), g.trace_totals):
            with pytest.raises(PaxisimError, match=EINVAL):
                call()                                         # every readout before enable
        for bad in ([], list(range(abi.TRACE_MAX_CLUSTERS + 1))):
            with pytest.raises(PaxisimError, match=EINVAL):
                g.trace_enable(bad, 16)                        # n_clusters of 0 or above the maximum
        with pytest.raises(PaxisimError, match=EINVAL):
            g.trace_enable([3, 5, 3], 16)                      # a repeated cluster
        for cap in (0, abi.TRACE_MAX_RECORDS + 1):
            with pytest.raises(PaxisimError, match=EINVAL):
                g.trace_enable([0], cap)
        for window in ((5, 5), (6, 5)):
            with pytest.raises(PaxisimError, match=EINVAL):
                g.trace_enable([0], 16, *window)               # step_from >= step_to
        with pytest.raises(PaxisimError, match=ERANGE):
            g.trace_enable([0, 70], 16)                        # a cluster outside the handle
        before = g.device_bytes()
        g.trace_enable([69, 0], 16)
        table = g.device_bytes() - before - 2 * 5 * (16 * 32 + 4)   # 4 bytes per allocated cluster lane
        assert 4 * 70 <= table <= 4 * 1024 and table % 256 == 0
        with pytest.raises(PaxisimError, match=EINVAL):
            g.trace_enable([1], 16)                            # only once
        assert g.trace_read(69, 4) == ([], 0) and g.trace_totals() == (0, 0)
        for cluster, replica in ((1, 0), (70, 0), (0, 5)):
            with pytest.raises(PaxisimError, match=EINVAL):
                g.trace_read(cluster, replica)                 # not traced, outside the handle, no such replica
    with _sim(shape()) as g:
        g.step(1)
        with pytest.raises(PaxisimError, match=EINVAL):
            g.trace_enable([0], 16)                            # only before the first step


# ---- tools/trace_cli.py capture --device ---------------------------------------------------------
@pytest.mark.parametrize("config", [2, 4, 5])
def test_trace_cli_device_capture_writes_the_same_files(config, tmp_path):
    """One step(n) through the recorder writes the gob files and schedule the step-by-step capture
    writes, and they replay."""
    import argparse
    import filecmp
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import trace_cli
    a, b = str(tmp_path / "host"), str(tmp_path / "device")
    ns = dict(config=config, cluster=65, clusters=70, steps=120, crash_step=40)
    trace_cli.capture(argparse.Namespace(out=a, **ns))
    trace_cli.capture(argparse.Namespace(out=b, device=True, **ns))
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and len(names) > 5
    match, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert not mismatch and not errors, (mismatch, errors)
    assert trace_cli.replay(argparse.Namespace(dir=b))
