"""The Multi-Paxos kernels against the map-based model of tests/paxos_model.py: the
recording build's own trace of the pinned clusters of a shape, replayed through replicas that keep
unbounded maps, and the end of the run - read_state, the window by read_log, the flags - checked
against them.  The shapes and their pinned flag words are those of tests/test_paxos_model.py."""
import pytest

import paxos_model as pm
from paxi_amd import trace
from paxi_amd.sim import Simulation

pytestmark = pytest.mark.gpu
CAP = 1 << 13                       # records per traced replica; the longest row seen on the oracle is 3428


def device_against_model(name):
    sh = pm.SHAPES[name]()
    with Simulation(sh.cfg, sh.wl, sh.fp, sh.faults) as g:
        g.latency_enable(64)
        g.trace_enable(list(sh.traced), CAP)
        g.step(sh.steps)
        assert g.trace_totals()[1] == 0
        assert pm.flag_counts(g) == pm.FLAG_COUNTS[name]
        res = {c: pm.replay_cluster(g, sh, c, trace.from_device(g, c)["msgs"]) for c in sh.traced}
    assert {c: word for c, (_, word) in res.items()} == sh.traced
    assert sum(rp.matched for rp, _ in res.values()) > 500
    assert {c for c, (rp, _) in res.items() if rp.panics} == {c for c, w in sh.traced.items() if w & pm.POISON}
    reps = [m.paxos for rp, _ in res.values() for m in rp.replicas]
    if name in pm.WRAPS:
        for c, (rp, _) in res.items():
            assert max(m.paxos.slot for m in rp.replicas) >= 4 * sh.cfg.window, f"cluster {c}"
    if name in pm.OUT_OF_WINDOW:
        assert sum(p.below for p in reps) > 0 and sum(p.above for p in reps) > 0
    return res


@pytest.mark.parametrize("name", list(pm.SHAPES))
def test_device_trace_against_model(name):
    device_against_model(name)


def test_a_p2b_for_a_committed_ghost_is_ignored():
    """The commit bit of a ghost, which only a transport that hands a P3 and a P2b in reaches
    (tests/test_paxos_model.py has the scenario): the device against the model, from its own trace."""
    sh, deliveries = pm.committed_ghost_case()
    with Simulation(sh.cfg, sh.wl) as g:
        g.latency_enable(64)
        g.trace_enable([0], 256)
        at = 0
        for t, args in sorted(deliveries.items()):
            g.step(t - at)
            g.deliver(*args)
            at = t
        g.step(sh.steps - at)
        seen = {(t, src, dst, tuple(recs[0][1:])) for t, (_, dst, src, recs) in deliveries.items()}
        rp, word = pm.replay_cluster(g, sh, 0, trace.from_device(g, 0)["msgs"], delivered_in=seen)
    a = rp.replicas[0].paxos
    assert word == sh.traced[0] and sum(rp.delivered.values()) == rp.matched + 2
    assert a.log[0].commit and (a.ballot, a.active, a.execute) == ((1 << 4) | 0, True, 3)


@pytest.mark.parametrize("env", [{"PAXISIM_SERIAL": "0"}, {"PAXISIM_POOLS": "1"}], ids=["serial0", "pools1"])
def test_kernel_forms_against_model(monkeypatch, env):
    """The replica-per-wave kernel and the single-pool form on the wrap shape."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    device_against_model("wrap")
