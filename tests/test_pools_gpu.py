"""Two cluster pools per handle (PAXISIM_POOLS=2) are invisible: each pool steps,
compacts and phase-bins its own slot region on its own stream, and every replica state, instance
and statistic equals the oracle's and the one-pool run's.  The launch count shows both pools
launched; a handle of one tile degrades to one pool.  20-step chunks, two calls of 200 steps."""
import functools

import pytest

from paxi_amd import abi
import oracle_lib as ol
from test_parity_gpu import assert_same

pytestmark = pytest.mark.gpu
STEPS = (200, 200)


def _paxos5(clusters):
    """The fault process of test_pipeline_gpu: clusters die and compaction moves slots."""
    cfg = abi.make_config(npz=[5], clusters=clusters, seed=11, window=16, mbox_cap=32, max_delay=4,
                          steps_per_launch=20)
    wl = abi.make_workload(outstanding=8, target=0)
    fp = abi.make_fault_process(drop_ppm=5000, drop_len=20, slow_ppm=5000, slow_len=20, slow_min=1, slow_max=4)
    return cfg, wl, fp, []


def _paxos9(clusters=1024 + 9, crash=150):
    """The config-4 workload: FGrid 3x3, the leader crashes and a second set of clients re-elects."""
    cfg = abi.make_config(npz=[3, 3, 3], clusters=clusters, seed=42, q1=abi.Q_FGRID_Q1, q2=abi.Q_FGRID_Q2, fz=1,
                          ephemeral_leader=1, window=16, mbox_cap=32, max_delay=0, steps_per_launch=20)
    wl = abi.make_workload(outstanding=8, target=[0, 0, 0, 0, 3, 3, 3, 3],
                           start_step=[0, 0, 0, 0, crash, crash, crash, crash])
    return cfg, wl, None, [abi.make_fault(abi.FAULT_CRASH, 0, step_from=crash)]


def _paxos3(clusters=640):
    cfg = abi.make_config(npz=[3], clusters=clusters, seed=31, window=16, mbox_cap=16, max_delay=3,
                          steps_per_launch=20)
    wl = abi.make_workload(outstanding=3, target=[0, 1, 2])
    fp = abi.make_fault_process(drop_ppm=5000, drop_len=20, slow_ppm=5000, slow_len=20, slow_min=1, slow_max=3)
    return cfg, wl, fp, []


SHAPES = {"p5_64": lambda: _paxos5(64), "p5_581": lambda: _paxos5(512 + 64 + 5),
          "p5_2085": lambda: _paxos5(2048 + 37), "p9": _paxos9, "p3": _paxos3}


def _snap(s):
    return ([x.as_tuple() for x in s.read_state()], [x.as_tuple() for x in s.read_instances()],
            s.stats().as_dict(), s.check())


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(states, instances, stats, check) of the oracle after both calls: computed once per shape."""
    cfg, wl, fp, faults = SHAPES[name]()
    o = ol.OracleSim(cfg, wl, fp, faults)
    o.step(sum(STEPS))
    snap = _snap(o)
    o.close()
    return snap


def _gpu(monkeypatch, name, pools, env=()):
    from paxi_amd.sim import Simulation
    monkeypatch.setenv("PAXISIM_POOLS", str(pools))
    monkeypatch.setenv("PAXISIM_PHASE_SORT", "1")
    for k, v in env:
        monkeypatch.setenv(k, v)
    cfg, wl, fp, faults = SHAPES[name]()
    g = Simulation(cfg, wl, fp, faults)
    for n in STEPS:
        g.step(n)
    g.sync()
    _, launches = g.kernel_time()
    snap = _snap(g)
    active = g.active_clusters()
    g.close()
    return snap, launches, active


def _same(a, b, ctx):
    for k, what in enumerate(("states", "instances", "stats", "check")):
        assert a[k] == b[k], f"{ctx}: {what} differ"


def test_one_tile_runs_one_pool(monkeypatch):
    s2, k2, _ = _gpu(monkeypatch, "p5_64", 2)
    s1, k1, _ = _gpu(monkeypatch, "p5_64", 1)
    _same(s2, _oracle("p5_64"), "64 clusters against the oracle")
    _same(s2, s1, "64 clusters against one pool")
    assert k2 == k1, (k2, k1)


@pytest.mark.parametrize("name", ["p5_581", "p5_2085"])
def test_paxos5_two_pools_match_oracle_and_one_pool(monkeypatch, name):
    s2, k2, a2 = _gpu(monkeypatch, name, 2)
    s1, k1, a1 = _gpu(monkeypatch, name, 1)
    _same(s2, _oracle(name), f"{name} against the oracle")
    _same(s2, s1, f"{name} against one pool")
    assert k2 > k1, (k2, k1)                       # both pools launched
    clusters = SHAPES[name]()[0].clusters
    assert a2 < clusters and a1 < clusters, (a2, a1)   # clusters died and were compacted away in both


def test_looping_waves(monkeypatch):
    """A persistent grid of 8 waves: every wave loops over many tickets, two such kernels at once."""
    s2, k2, _ = _gpu(monkeypatch, "p5_2085", 2, env=[("PAXISIM_PIPE_SLOTS", "8")])
    _same(s2, _oracle("p5_2085"), "8 slots against the oracle")
    s1, k1, _ = _gpu(monkeypatch, "p5_2085", 1, env=[("PAXISIM_PIPE_SLOTS", "8")])
    _same(s1, _oracle("p5_2085"), "8 slots, one pool, against the oracle")
    assert k2 > k1, (k2, k1)


def test_paxos9_plane_unit_with_idle_skip(monkeypatch):
    s2, k2, _ = _gpu(monkeypatch, "p9", 2)
    s1, k1, _ = _gpu(monkeypatch, "p9", 1)
    _same(s2, _oracle("p9"), "N=9 against the oracle")
    _same(s2, s1, "N=9 against one pool")
    assert k2 > k1, (k2, k1)


def test_paxos3_generic_packed_unit(monkeypatch):
    s2, k2, _ = _gpu(monkeypatch, "p3", 2)
    s1, k1, _ = _gpu(monkeypatch, "p3", 1)
    _same(s2, _oracle("p3"), "N=3 against the oracle")
    _same(s2, s1, "N=3 against one pool")
    assert k2 > k1, (k2, k1)


def test_wake_in_both_regions(monkeypatch):
    """Workers stop after max_requests, every cluster goes quiet and both regions freeze slots; a
    request injected into a frozen cluster of each region wakes it (as in test_compaction_gpu)."""
    from paxi_amd.sim import Simulation
    monkeypatch.setenv("PAXISIM_POOLS", "2")
    monkeypatch.setenv("PAXISIM_PHASE_SORT", "1")
    cfg = abi.make_config(npz=[3], clusters=640, seed=31, window=16, mbox_cap=16, max_delay=3,
                          ephemeral_leader=1, steps_per_launch=20)
    wl = abi.make_workload(outstanding=3, target=[0, 1, 2], max_requests=6)
    fp = abi.make_fault_process(drop_ppm=8000, drop_len=20, slow_ppm=8000, slow_len=20, slow_min=1, slow_max=3)
    g, o = Simulation(cfg, wl, fp), ol.OracleSim(cfg, wl, fp)
    g.step(200)
    o.step(200)
    assert_same(g, o, "quiet")
    act = g.activity()
    # no compaction has moved a cluster across the split, so cluster c sits in region c >= 512
    frozen = [[c for c in rng if act[c] is not None] for rng in (range(0, 512), range(512, 640))]
    assert frozen[0] and frozen[1], (len(frozen[0]), len(frozen[1]))
    woken = [frozen[0][0], frozen[0][-1], frozen[1][0], frozen[1][-1]]
    cid = 1 << 22
    for c in woken:
        g.inject(c, c % 3, cid)
        o.inject(c, c % 3, cid)
        cid += 1
    act = g.activity()
    assert all(act[c] is None for c in woken), [act[c] for c in woken]
    for n in STEPS:
        g.step(n)
        o.step(n)
    assert_same(g, o, "after the wake")
    g.close()


def test_interleaved_readouts_join_the_pools(monkeypatch):
    """stats(), read_state() and check() between step calls wait for both pools' streams."""
    from paxi_amd.sim import Simulation
    monkeypatch.setenv("PAXISIM_POOLS", "2")
    monkeypatch.setenv("PAXISIM_PHASE_SORT", "1")
    cfg, wl, fp, faults = SHAPES["p5_581"]()
    g, o = Simulation(cfg, wl, fp, faults), ol.OracleSim(cfg, wl, fp, faults)
    for k, n in enumerate((60, 20, 137, 1, 182)):          # 400 steps in all: ends at the shared oracle's state
        g.step(n)
        o.step(n)
        assert g.stats().as_dict() == o.stats().as_dict(), f"stats after call {k}"
        assert [x.as_tuple() for x in g.read_state()] == [x.as_tuple() for x in o.read_state()], f"states after call {k}"
        assert g.check() == o.check()
    _same(_snap(g), _oracle("p5_581"), "after the interleaved calls")
    g.close()


def test_latency_recording_twin(monkeypatch):
    """The latency-recording kernels (lat_kernel.h) under two pools: one sample per reply."""
    from paxi_amd.sim import Simulation
    monkeypatch.setenv("PAXISIM_POOLS", "2")
    monkeypatch.setenv("PAXISIM_PHASE_SORT", "1")
    cfg, wl, fp, faults = SHAPES["p5_581"]()
    g = Simulation(cfg, wl, fp, faults)
    g.latency_enable(64)
    before = g.stats().replies
    for n in STEPS:
        g.step(n)
    assert g.latency().count == g.stats().replies - before > 0
    _, launches = g.kernel_time()
    assert launches > sum(STEPS) // 60 + 2                 # more launches than one pool makes
    _same(_snap(g), _oracle("p5_581"), "latency twin against the oracle")
    g.close()
