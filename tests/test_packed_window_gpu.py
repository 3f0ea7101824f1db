"""The Multi-Paxos log window of the serial kernels: one 16-B entry {ballot,
cmd|flags, acks, request} per slot in HBM, with the committed bits of the
window kept beside the pending count.

Every case runs against the CPU oracle: replica states and totals
(assert_same), and the window itself, which read_state does not show - read_log
of the whole held window [execute, execute + W) of every replica of the first
64 clusters, `request` included.  Each case first checks on the oracle's own
statistics that its inputs reach the paths it is there for."""
import functools

import pytest

from paxi_amd import abi
import oracle_lib as ol
from test_parity_gpu import assert_same

pytestmark = pytest.mark.gpu

WOVF, GHOST, MBOX_OVF, PEND_OVF, UNFAITHFUL, POISON = range(6)   # bit numbers of Stats.flagged
LOG_CLUSTERS = 64


def _gpu(cfg, wl, fp=None, faults=()):
    from paxi_amd.sim import Simulation
    return Simulation(cfg, wl, fp, faults)


def _windows(sim, cfg, states=None):
    """The held window of every replica of the first LOG_CLUSTERS clusters, as tuples."""
    N, n = abi.n_replicas(cfg), min(LOG_CLUSTERS, cfg.clusters)
    states = states or sim.read_state(0, n)
    return [[e.as_tuple() for e in sim.read_log(c, r, states[c * N + r].execute, cfg.window)]
            for c in range(n) for r in range(N)]


def _assert_windows(g, o, cfg, ctx):
    N, n = abi.n_replicas(cfg), min(LOG_CLUSTERS, cfg.clusters)
    states = o.read_state(0, n)            # assert_same has shown the GPU's equal
    a, b = _windows(g, cfg, states), _windows(o, cfg, states)
    held = 0
    for k, (x, y) in enumerate(zip(a, b)):
        assert x == y, f"{ctx}: window of cluster {k // N} replica {k % N}\n gpu={x}\n cpu={y}"
        held += sum(1 for e in y if e[3] & abi.LOG_EXISTS)
    assert held > 0, f"{ctx}: no entry held in any window read"


def _run(cfg, wl, fp, faults, chunks, oracle, ctx):
    g = _gpu(cfg, wl, fp, faults)
    for n in chunks:
        g.step(n)
    st = assert_same(g, oracle, ctx)
    _assert_windows(g, oracle, cfg, ctx)
    return g, st


# ---------------------------------------------------------------------------
# 1: the config-2 shape (N = 5, W = 16, Drop/Slow), shared by cases 1, 6 and 7
# ---------------------------------------------------------------------------
def _case1():
    cfg = abi.make_config(npz=[5], clusters=192, seed=31, window=16, mbox_cap=32, max_delay=4,
                          steps_per_launch=20, kv=1)
    wl = abi.make_workload(outstanding=8, target=0)
    fp = abi.make_fault_process(drop_ppm=5000, drop_len=20, slow_ppm=5000, slow_len=20, slow_min=1, slow_max=4)
    return cfg, wl, fp


@functools.lru_cache(maxsize=None)
def _oracle1():
    """Case 1 after its 400 steps on the oracle (read only: shared)."""
    cfg, wl, fp = _case1()
    o = ol.OracleSim(cfg, wl, fp)
    o.step(400)
    st = o.stats().as_dict()
    assert st["flagged"][WOVF] == 170 and st["flagged"][GHOST] == 88, st
    assert st["dropped"] == 124462 and st["commits"] == 134912, st
    return o


def test_config2_shape():
    cfg, wl, fp = _case1()
    _run(cfg, wl, fp, (), (200, 200), _oracle1(), "config-2 shape")


# ---------------------------------------------------------------------------
# 2: W = 8 - the committed bits wrap with the ring - at three unit sizes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("npz,clusters,wovf,mbox", [([3], 192, 129, 113), ([5], 192, 144, 137),
                                                   ([3, 3, 3], 128, 110, 105)])
def test_tight_window(npz, clusters, wovf, mbox):
    cfg = abi.make_config(npz=npz, clusters=clusters, seed=32, window=8, mbox_cap=8, max_delay=6, kv=1)
    wl = abi.make_workload(outstanding=8, target=0)
    fp = abi.make_fault_process(drop_ppm=5000, drop_len=40, slow_ppm=8000, slow_len=30, slow_min=2, slow_max=6)
    o = ol.OracleSim(cfg, wl, fp)
    o.step(400)
    st = o.stats().as_dict()
    assert st["flagged"][WOVF] == wovf and st["flagged"][MBOX_OVF] == mbox and st["flagged"][UNFAITHFUL] > 0, st
    _run(cfg, wl, fp, (), (400,), o, f"tight npz={npz}")


# ---------------------------------------------------------------------------
# 3: entries that carry requests at a deposed leader
# ---------------------------------------------------------------------------
def test_requests_at_deposed_leader():
    cfg = abi.make_config(npz=[3, 3, 3], clusters=128, seed=5, q1=abi.Q_FGRID_Q1, q2=abi.Q_FGRID_Q2, fz=1,
                          ephemeral_leader=1, mbox_cap=24, max_delay=0, kv=1)
    wl = abi.make_workload(outstanding=8, target=[0, 0, 0, 0, 3, 3, 3, 3], start_step=[0, 0, 0, 0, 60, 60, 60, 60])
    faults = [abi.make_fault(abi.FAULT_CRASH, 0, step_from=60)]
    o = ol.OracleSim(cfg, wl, None, faults)
    o.step(300)
    st = o.stats().as_dict()
    assert st["discarded"] == 86144 and st["commits"] == 50688, st
    _run(cfg, wl, None, faults, (300,), o, "deposed leader")


# ---------------------------------------------------------------------------
# 4: external requests - the entry's request word is used
# ---------------------------------------------------------------------------
def test_external_requests_forwarding():
    cfg = abi.make_config(npz=[5], clusters=128, seed=21, kv=1)
    wl = abi.make_workload(outstanding=6, target=[0, 1, 2, 3, 4, 2])
    fp = abi.make_fault_process(drop_ppm=2000, drop_len=15, slow_ppm=2000, slow_len=15, slow_min=1, slow_max=4)
    o = ol.OracleSim(cfg, wl, fp)
    o.step(300)
    st = o.stats().as_dict()
    assert st["delivered"]["Request"] == 21546 and st["delivered"]["Reply"] == 21182, st
    assert st["flagged"][WOVF] == 117 and st["flagged"][GHOST] == 42, st
    _run(cfg, wl, fp, (), (300,), o, "forwarding")


def test_external_requests_ephemeral_leaders():
    cfg = abi.make_config(npz=[3, 3, 3], clusters=128, seed=21, ephemeral_leader=1, kv=1)
    wl = abi.make_workload(outstanding=6, target=[0, 4, 8, 0, 4, 8])
    fp = abi.make_fault_process(drop_ppm=2000, drop_len=15, slow_ppm=2000, slow_len=15, slow_min=1, slow_max=3)
    o = ol.OracleSim(cfg, wl, fp)
    o.step(300)
    st = o.stats().as_dict()
    assert st["flagged"][GHOST] == 128 and st["flagged"][POISON] == 9 and st["flagged"][MBOX_OVF] == 10, st
    _run(cfg, wl, fp, (), (300,), o, "ephemeral leaders")


# ---------------------------------------------------------------------------
# 5: reply_when_commit and thrifty
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("opt,seed", [("reply_when_commit", 22), ("thrifty", 23)])
def test_options(opt, seed):
    cfg = abi.make_config(npz=[5], clusters=128, seed=seed, kv=1, **{opt: 1})
    wl = abi.make_workload(outstanding=8, target=0)
    fp = abi.make_fault_process(drop_ppm=5000, drop_len=20, slow_ppm=5000, slow_len=20, slow_min=1, slow_max=4)
    o = ol.OracleSim(cfg, wl, fp)
    o.step(300)
    st = o.stats().as_dict()
    assert st["commits"] > 0 and st["dropped"] > 0 and st["replies"] > 0, st
    _run(cfg, wl, fp, (), (300,), o, opt)


# ---------------------------------------------------------------------------
# 6: compaction moves the packed array with the rest of a cluster's state
# ---------------------------------------------------------------------------
def test_compaction_moves_the_windows(monkeypatch):
    cfg, wl, fp = _case1()
    chunks = (60, 60, 60, 60, 60, 100)
    g1, _ = _run(cfg, wl, fp, (), chunks, _oracle1(), "compaction on")
    assert g1.active_clusters() < cfg.clusters      # clusters were frozen: slots have been swapped
    monkeypatch.setenv("PAXISIM_COMPACT", "0")
    g0, _ = _run(cfg, wl, fp, (), chunks, _oracle1(), "compaction off")
    assert [s.as_tuple() for s in g1.read_state()] == [s.as_tuple() for s in g0.read_state()]
    assert _windows(g1, cfg) == _windows(g0, cfg)


# ---------------------------------------------------------------------------
# 7: the plane layout of the replica-per-wave kernel still works
# ---------------------------------------------------------------------------
def test_plane_layout_kernel(monkeypatch):
    monkeypatch.setenv("PAXISIM_SERIAL", "0")
    cfg, wl, fp = _case1()
    _run(cfg, wl, fp, (), (200, 200), _oracle1(), "PAXISIM_SERIAL=0")
