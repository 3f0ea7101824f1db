"""EPaxos on the device at the edges of its shape space.

D1: the recording build of the EPaxos kernel against the map-based model of tests/epaxos_model.py -
the device's own trace replayed through replicas that keep unbounded maps, at shapes where the ring
wraps, the payloads fill five records, Drop faults leave gaps and reply_when_commit is on.
D2: the plain kernels against the oracle, bit-exact, at N = 8, 9, 10, even N, N = 1, a ring and a
mailbox that overflow, reply_when_commit, every kernel form and every launch shape."""
import pytest

import epaxos_model as em
import oracle_lib as ol
from paxi_amd import abi, trace
from paxi_amd.sim import PaxisimError, Simulation
from test_parity_wpaxos_gpu import run_and_compare

pytestmark = pytest.mark.gpu
CAP = 1 << 13                       # records per traced replica; the oracle's longest row is 6621 (wrap10)


# ---- D1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wrap5", "wrap10", "drop10", "rwc5"])
def test_device_trace_against_model(name):
    sh = em.SHAPES[name]()
    with Simulation(sh.cfg, sh.wl, sh.fp) as g:
        g.latency_enable(64)
        g.trace_enable(list(em.TRACED), CAP)
        g.step(sh.steps)
        assert g.trace_totals()[1] == 0
        rps = {c: em.replay_cluster(g, sh, c, trace.from_device(g, c)["msgs"]) for c in em.TRACED}
    assert sum(rp.matched for rp in rps.values()) > 500
    if name.startswith("wrap"):
        for c, rp in rps.items():
            for r, m in enumerate(rp.replicas):
                assert m.slot[r] >= 4 * sh.cfg.window, f"cluster {c} replica {r}"
    if name == "wrap10":
        assert sum(rp.delivered[em.T_ACCEPT] for rp in rps.values()) > 0
    if sh.drains:
        assert sum(em.reexecutions(rp) for rp in rps.values()) > 0


# ---- D2 ------------------------------------------------------------------------------------------
def ep(npz, keys, W=32, M=32, D=3, clusters=130, **kw):
    return abi.make_config(protocol=abi.EPAXOS, npz=list(npz), clusters=clusters, seed=11, keys=keys, window=W,
                           mbox_cap=M, max_delay=D, **kw)


def workers(cfg, **kw):
    N = abi.n_replicas(cfg)
    return abi.make_workload(outstanding=N, target=list(range(N)), **kw)


def usual_faults(D=3):
    """The fault process of test_epaxos.py::test_gpu_parity and its crash of replica 1 over [60, 90)."""
    return (abi.make_fault_process(drop_ppm=1500, drop_len=10, slow_ppm=3000, slow_len=20, slow_min=1,
                                   slow_max=min(3, D)),
            [abi.make_fault(abi.FAULT_CRASH, 1, step_from=60, step_to=90)])


def parity(cfg, chunks=(70, 53), faults=True):
    fp, sc = usual_faults(cfg.max_delay) if faults else (None, [])
    return run_and_compare(cfg, workers(cfg), fp, sc, chunks=chunks)


@pytest.mark.parametrize("npz,keys,kw,wovf", [
    ((10,), 4, dict(M=64), False), ((3, 3, 4), 8, dict(M=64), True),
    ((3, 3, 3), 8, dict(M=64, D=2), False), ((8,), 2, dict(M=48, D=2), False),
    ((2, 2), 2, dict(W=16, D=2), False), ((2,), 1, dict(W=16, M=16, D=1), False)],
    ids=["n10", "n10_zones", "n9", "n8", "n4", "n2"])
def test_parity_at_every_n(npz, keys, kw, wovf):
    st = parity(ep(npz, keys, **kw))
    assert st["commits"] > 0
    if wovf:                                  # 3 clusters on the oracle: the flag agrees (run_and_compare)
        assert st["flagged"][0] > 0


def test_a_single_replica():
    """N = 1: PreAccept goes to nobody, no reply ever arrives, nothing commits."""
    st = parity(ep((1,), 1, W=16, M=16, D=0), chunks=(10,), faults=False)
    assert st["delivered_total"] == 0 and st["commits"] == 0 and st["client_requests"] == 130


def test_ring_overflow():
    st = parity(ep((5,), 2, W=8))
    assert st["flagged"][0] > 0 and st["commits"] > 0


@pytest.mark.parametrize("npz,M", [((5,), 8), ((7,), 12)])
def test_mailbox_overflow(npz, M):
    """A multi-record message that does not fit is dropped whole and counted once."""
    st = parity(ep(npz, 4, M=M))
    assert st["flagged"][2] > 0 and st["commits"] > 0


def test_reply_when_commit():
    a = parity(ep((5,), 4, reply_when_commit=1))
    b = parity(ep((5,), 4, reply_when_commit=1, kv=1))
    assert a["replies"] == b["replies"] > 0


@pytest.mark.parametrize("env", [{"PAXISIM_SERIAL": "0"}, {"PAXISIM_PIPE": "1"}], ids=["serial0", "pipe1"])
@pytest.mark.parametrize("npz,M", [((5,), 32), ((10,), 64)], ids=["n5", "n10"])
def test_kernel_forms(monkeypatch, env, npz, M):
    default = parity(ep(npz, 4, M=M))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert parity(ep(npz, 4, M=M)) == default


def _states(cfg, chunks):
    fp, sc = usual_faults(cfg.max_delay)
    with Simulation(cfg, workers(cfg), fp, sc) as g:
        for n in chunks:
            g.step(n)
        return [s.as_tuple() for s in g.read_state()], [i.as_tuple() for i in g.read_instances()]


def test_steps_per_launch_invariance():
    res = [_states(ep((5,), 4, steps_per_launch=S), (100, 57)) for S in (1, 7, 64)]
    assert res[0] == res[1] == res[2]
    o = ol.OracleSim(ep((5,), 4), workers(ep((5,), 4)), *usual_faults())
    o.step(157)
    assert res[0][0] == [s.as_tuple() for s in o.read_state()]


def test_sharding_by_cluster_base():
    whole = _states(ep((5,), 4, clusters=200), (150,))
    a = _states(ep((5,), 4, clusters=77), (150,))
    b = _states(ep((5,), 4, clusters=123, cluster_base=77), (150,))
    assert whole[0] == a[0] + b[0] and whole[1] == a[1] + b[1]


@pytest.mark.parametrize("clusters", [1, 65])
def test_single_cluster_and_ragged_tail(clusters):
    assert parity(ep((5,), 4, clusters=clusters))["commits"] > 0


def test_a_redelivered_commit_recommits_in_place():
    """The re-commit branch of ep_handle_commit, which only a transport that hands a Commit in
    twice reaches (tests/test_epaxos_model.py has the scenario): the device against the model,
    from its own trace, and against the oracle."""
    sh, at, args, seen = em.redelivery_case()
    o = ol.OracleSim(sh.cfg, sh.wl)
    with Simulation(sh.cfg, sh.wl) as g:
        g.latency_enable(64)
        g.trace_enable([0], 256)
        for sim in (g, o):
            sim.step(at)
            sim.deliver(*args)
            sim.step(sh.steps - at)
        rp = em.replay_cluster(g, sh, 0, trace.from_device(g, 0)["msgs"], {seen})
        assert rp.replicas[2].log[2][0].seq == 10
        assert [s.as_tuple() for s in g.read_state()] == [s.as_tuple() for s in o.read_state()]
        assert [i.as_tuple() for i in g.read_instances()] == [i.as_tuple() for i in o.read_instances()]


# ---- E -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("proto", [abi.EPAXOS, abi.ABD])
def test_read_log_is_refused(proto):
    """EPaxos and ABD images hold no Paxos window: read_log fails on the host, before any launch."""
    cfg = abi.make_config(protocol=proto, npz=[3], clusters=2, keys=2, window=16, mbox_cap=16, max_delay=1)
    with Simulation(cfg, abi.make_workload(outstanding=1)) as g:
        g.step(5)
        with pytest.raises(PaxisimError, match=r"error -4:"):
            g.read_log(0, 0, 0, 4)
