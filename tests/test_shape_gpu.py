"""The fixed-shape unit (k_paxos5f.hip) is invisible: a handle of the headline's shape
runs it, and every replica state, instance, log entry, statistic and flag word equals the oracle's
and the same run's on the generic unit (PAXISIM_SHAPE=0).  Config 2's shape at small sizes: 20-step
chunks, compaction and phase binning on.  Simulation.step_unit says which unit ran."""
import functools

import pytest

from paxi_amd import abi
import oracle_lib as ol

pytestmark = pytest.mark.gpu
FIXED, GENERIC = abi.UNIT_FIXED_PAXOS5, abi.UNIT_GENERIC


def _shape(clusters, ppm=5000, seed=11, **over):
    """Config 2's shape; ppm: the Drop/Slow process (5000: windows overflow, ghosts appear and clusters
    die within 400 steps, so compaction moves slots)."""
    kw = dict(npz=[5], clusters=clusters, seed=seed, window=16, mbox_cap=32, max_delay=4, steps_per_launch=20, kv=1)
    kw.update(over)
    cfg = abi.make_config(**kw)
    wl = abi.make_workload(outstanding=8, target=0)
    fp = abi.make_fault_process(drop_ppm=ppm, drop_len=20, slow_ppm=ppm, slow_len=20, slow_min=1, slow_max=4)
    return cfg, wl, fp


def _logs(s, states, clusters):
    """The window entries from each replica's execute on, of a spread of clusters."""
    n = s.N
    out = []
    for c in sorted({0, 1, clusters // 3, clusters // 2, clusters - 2, clusters - 1}):
        for r in range(n):
            lo = max(0, states[c * n + r][2])
            out.append((c, r, [e.as_tuple() for e in s.read_log(c, r, lo, s.cfg.window)]))
    return out


def _snap(s):
    """read_state (the flag words in it), read_instances, read_log, stats (flagged[] in it), check."""
    states = [x.as_tuple() for x in s.read_state()]
    return (states, [x.as_tuple() for x in s.read_instances()], _logs(s, states, s.cfg.clusters),
            s.stats().as_dict(), s.check())


def _same(a, b, ctx):
    for k, what in enumerate(("states", "instances", "logs", "stats", "check")):
        assert a[k] == b[k], f"{ctx}: {what} differ"


def _flag_words(states, n):
    return [functools.reduce(lambda f, s: f | s[4], states[c * n:(c + 1) * n], 0) for c in range(len(states) // n)]


def _env(monkeypatch, shape, pools=1, slots=None):
    monkeypatch.setenv("PAXISIM_SHAPE", str(shape))
    monkeypatch.setenv("PAXISIM_POOLS", str(pools))
    monkeypatch.setenv("PAXISIM_PHASE_SORT", "1")
    if slots:
        monkeypatch.setenv("PAXISIM_PIPE_SLOTS", str(slots))
    else:
        monkeypatch.delenv("PAXISIM_PIPE_SLOTS", raising=False)


def _gpu(monkeypatch, shape, args, calls, unit, pools=1, slots=None, faults=()):
    from paxi_amd.sim import Simulation
    _env(monkeypatch, shape, pools, slots)
    g = Simulation(*args, faults)
    assert g.step_unit() == unit, f"PAXISIM_SHAPE={shape}: unit {g.step_unit()}"
    for n in calls:
        g.step(n)
    snap = _snap(g)
    active = g.active_clusters()
    assert g.step_unit() == unit
    g.close()
    return snap, active


def _oracle(args, calls, faults=()):
    o = ol.OracleSim(*args, faults)
    o.step(sum(calls))
    snap = _snap(o)
    o.close()
    return snap


def _both(monkeypatch, args, calls, ctx, **kw):
    """The run on the fixed-shape unit, against the oracle and against the generic unit."""
    want = _oracle(args, calls)
    fixed, a1 = _gpu(monkeypatch, 1, args, calls, FIXED, **kw)
    _same(fixed, want, f"{ctx}: fixed-shape unit against the oracle")
    generic, a0 = _gpu(monkeypatch, 0, args, calls, GENERIC, **kw)
    _same(fixed, generic, f"{ctx}: fixed-shape unit against the generic unit")
    assert a1 == a0, (a1, a0)
    return want, a1


def test_partial_tile_and_odd_calls(monkeypatch):
    """64 + 5 clusters (a partial tile), 300 steps in calls of odd lengths: single-chunk sim_serial
    launches beside the pipelined ones."""
    _both(monkeypatch, _shape(64 + 5), (1, 19, 61, 137, 82), "69 clusters")


def test_two_pools_looping_waves(monkeypatch):
    """2,048 + 37 clusters in two pools on a persistent grid of 8 waves: every wave loops over many
    tickets, and both region kernels run."""
    args = _shape(2048 + 37)
    _, active = _both(monkeypatch, args, (200, 200), "2085 clusters", pools=2, slots=8)
    assert active < args[0].clusters


def test_overflow_ghost_and_dead_clusters(monkeypatch):
    """A fault process heavy enough that the oracle alone shows window overflows, ghosts and dead
    clusters (replica states, message counts included, that no longer change) within the run."""
    args = _shape(640, ppm=8000)
    n = 5
    o = ol.OracleSim(*args)
    o.step(200)
    mid = [x.as_tuple() for x in o.read_state()]
    o.step(200)
    end = [x.as_tuple() for x in o.read_state()]
    o.close()
    words = _flag_words(end, n)
    dead = {c for c in range(640) if mid[c * n:(c + 1) * n] == end[c * n:(c + 1) * n]}
    assert sum(1 for w in words if w & abi.F_WOVF) > 50 and sum(1 for w in words if w & abi.F_GHOST) > 50
    assert len(dead) > 50
    want, active = _both(monkeypatch, args, (200, 200), "heavy faults", pools=2)
    assert _flag_words(want[0], n) == words
    assert want[3]["flagged"][:2] == [sum(1 for w in words if w & abi.F_WOVF), sum(1 for w in words if w & abi.F_GHOST)]
    assert active < 640 - 50, active                     # the dead clusters were compacted away


def test_wake_of_frozen_clusters_in_both_regions(monkeypatch):
    """Clusters die (every worker waits for a reply that was dropped) and both regions freeze slots; a
    request injected into a frozen cluster of each region wakes it, on either unit."""
    from paxi_amd.sim import Simulation
    args = _shape(640, ppm=8000)
    snaps = []
    for shape, unit in ((1, FIXED), (0, GENERIC)):
        _env(monkeypatch, shape, pools=2)
        g, o = Simulation(*args), ol.OracleSim(*args)
        assert g.step_unit() == unit
        g.step(200)
        o.step(200)
        act = g.activity()
        # no compaction moves a cluster across the split, so cluster c sits in region c >= 512
        frozen = [[c for c in rng if act[c] is not None] for rng in (range(0, 512), range(512, 640))]
        assert frozen[0] and frozen[1], (len(frozen[0]), len(frozen[1]))
        woken = [frozen[0][0], frozen[0][-1], frozen[1][0], frozen[1][-1]]
        for k, c in enumerate(woken):
            g.inject(c, c % 5, (1 << 22) + k)
            o.inject(c, c % 5, (1 << 22) + k)
        act = g.activity()
        assert all(act[c] is None for c in woken), [act[c] for c in woken]
        for n in (60, 140):
            g.step(n)
            o.step(n)
        snaps.append(_snap(g))
        _same(snaps[-1], _snap(o), f"PAXISIM_SHAPE={shape}: after the wake, against the oracle")
        g.close()
        o.close()
    _same(snaps[0], snaps[1], "after the wake: fixed-shape unit against the generic unit")


def test_recording_twin(monkeypatch):
    """Latency enabled and a trace of two clusters: the recording twin of the fixed-shape unit against
    the generic recording unit, and its states against the oracle."""
    from paxi_amd.sim import Simulation
    args = _shape(512 + 64 + 5)
    traced = (3, 512 + 64 + 4)
    got = []
    for shape, unit in ((1, FIXED), (0, GENERIC)):
        _env(monkeypatch, shape, pools=2)
        g = Simulation(*args)
        g.latency_enable(64)
        g.trace_enable(traced, 256, 0, 120)
        assert g.step_unit() == unit
        before = g.stats().replies
        for n in (200, 200):
            g.step(n)
        lat = g.latency()
        assert lat.count == g.stats().replies - before > 0
        per_worker = [g.latency(w) for w in range(8)]
        hists = [(h.count, h.sum, h.overflow, h.min, h.max, [int(x) for x in h.counts]) for h in [lat] + per_worker]
        traces = [g.trace_read(c, r) for c in traced for r in range(5)]
        assert all(t[0] for t in traces)
        got.append((_snap(g), hists, traces, g.trace_totals()))
        g.close()
    _same(got[0][0], _oracle(args, (200, 200)), "recording twin against the oracle")
    _same(got[0][0], got[1][0], "recording twin against the generic recording unit")
    assert got[0][1] == got[1][1], "latency histograms differ"
    assert got[0][2] == got[1][2] and got[0][3] == got[1][3], "traces differ"


@pytest.mark.parametrize("first", [1, 0])
def test_snapshot_crosses_units(monkeypatch, first):
    """A snapshot taken under one PAXISIM_SHAPE value restores into a handle created under the other;
    100 more steps end in the state of the straight run."""
    from paxi_amd.sim import Simulation
    args = _shape(512 + 64 + 5)
    units = {1: FIXED, 0: GENERIC}
    _env(monkeypatch, first, pools=2)
    a = Simulation(*args)
    assert a.step_unit() == units[first]
    a.step(100)
    blob = a.snapshot()
    a.close()
    _env(monkeypatch, 1 - first, pools=2)
    b = Simulation(*args)
    assert b.step_unit() == units[1 - first]
    b.restore(blob)
    assert b.step_unit() == units[1 - first]               # the unit is the handle's, not the snapshot's
    b.step(100)
    snap = _snap(b)
    b.close()
    _same(snap, _oracle(args, (200,)), f"snapshot under PAXISIM_SHAPE={first}, restored under {1 - first}")


def test_snapshot_carries_a_fault_out_of_the_shape(monkeypatch):
    """The scripted-fault count is the one pinned field that changes after create: a restored snapshot
    that brings a fault moves a fixed-shape handle to the generic unit, and one without moves it back."""
    from paxi_amd.sim import Simulation
    _env(monkeypatch, 1)
    args = _shape(64 + 5)
    fault = abi.make_fault(abi.FAULT_DROP, 1, step_from=10, step_to=60)
    plain, faulty = Simulation(*args), Simulation(*args)
    assert plain.step_unit() == FIXED and faulty.step_unit() == FIXED
    faulty.fault(fault)
    assert faulty.step_unit() == GENERIC
    plain.step(20)
    faulty.step(20)
    blob_plain, blob_faulty = plain.snapshot(), faulty.snapshot()
    plain.restore(blob_faulty)
    assert plain.step_unit() == GENERIC
    plain.step(80)
    o = ol.OracleSim(*args, [fault])
    o.step(100)
    _same(_snap(plain), _snap(o), "restored with a fault, against the oracle")
    faulty.restore(blob_plain)
    assert faulty.step_unit() == FIXED
    f = faulty.fork()
    assert f.step_unit() == FIXED
    for s in (faulty, f):
        s.step(80)
    want = _oracle(args, (100,))
    _same(_snap(faulty), want, "restored without a fault, against the oracle")
    _same(_snap(f), want, "its fork, against the oracle")
    for s in (plain, faulty, f):
        s.close()
    o.close()


@pytest.mark.parametrize("name", ["thrifty", "window32", "scripted_fault"])
def test_one_field_off_the_shape_runs_the_generic_unit(monkeypatch, name):
    over = {"thrifty": dict(thrifty=1), "window32": dict(window=32), "scripted_fault": {}}[name]
    faults = [abi.make_fault(abi.FAULT_CRASH, 2, step_from=90)] if name == "scripted_fault" else []
    args = _shape(512 + 64 + 5, **over)
    calls = (137, 63)
    got, _ = _gpu(monkeypatch, 1, args, calls, GENERIC, pools=2, faults=faults)
    _same(got, _oracle(args, calls, faults), f"{name} against the oracle")
