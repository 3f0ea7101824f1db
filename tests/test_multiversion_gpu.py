"""The multi-version Database recorded on the device (mv_kernel.h) against the
oracle-derived histories of tests/mv_ref.py: every (cluster, replica, key) history value for value,
the Consensus scan against the reference's predicate over the same histories, and the replica
states, stats, latencies and client histories those of a run without it."""
import contextlib

import pytest

import mv_ref
from paxi_amd import abi
from paxi_amd.sim import PaxisimError, Simulation

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPP, ERANGE = r"error -1:", r"error -4:", r"error -5:"


def _sim(name, H, bins=32, chist=0):
    cfg, wl, fp, faults = mv_ref.SHAPES[name][0]()
    g = Simulation(cfg, wl, fp, faults)
    if bins:
        g.latency_enable(bins)
    if chist:
        g.client_history_enable(chist)
    if H:
        g.multiversion_enable(H)
    return g


def _run(g, name):
    for n in mv_ref.SHAPES[name][1]:
        g.step(n)


def _assert_histories(g, hist, H):
    """Every row is the yardstick's first H values, the rest counted as dropped."""
    for (c, r, k), want in hist.items():
        got = g.kv_history(c, r, k)
        assert got == (want[:H], max(0, len(want) - H)), f"cluster {c} replica {r} key {k}"


def _yardstick(name, H):
    cfg = mv_ref.SHAPES[name][0]()[0]
    r = mv_ref.ref(name)
    return cfg, r, mv_ref.verdict(r.hist, cfg.clusters, abi.n_replicas(cfg), cfg.keys, H)


def _observables(g, cfg):
    return ([s.as_tuple() for s in g.read_state()], g.stats().as_dict(),
            [g.latency(w) for w in [None] + list(range(g.wl.outstanding))],
            [g.client_history(c) for c in range(0, cfg.clusters, 7)])


@pytest.mark.parametrize("env", [{}, {"PAXISIM_SERIAL": "0"}, {"PAXISIM_PIPE": "1"}],
                         ids=["default", "serial0", "pipe1"])
def test_paxos5_every_kernel_form(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    name, H = "paxos5", 64
    cfg, r, v = _yardstick(name, H)
    assert v.dropped == 0 and v.failed == 0 and 0 < v.longest <= H and v.versions == r.executed_writes
    with _sim(name, 0, chist=128) as g:                  # latency and the client history, no multiversion
        _run(g, name)
        plain = _observables(g, cfg)
    with _sim(name, H, chist=128) as g:
        _run(g, name)
        _assert_histories(g, r.hist, H)
        assert g.consensus() == (0, r.executed_writes, 0)
        assert sum(s.executed_writes for s in g.read_state()) == r.executed_writes
        assert g.consensus_failed() == [0] * cfg.clusters
        assert _observables(g, cfg) == plain
        assert plain[0] == r.states, "replica states differ from the oracle"


def _write_cid(s, cluster, start):
    cid = start
    while not s.command(cluster, cid)[1]:
        cid += 1
    return cid


def test_compaction_and_wake_leave_the_rows_with_their_cluster(monkeypatch):
    monkeypatch.setenv("PAXISIM_COMPACT_EVERY", "16")
    name, H = "paxos3_freeze", 64
    cfg, wl, fp, faults = mv_ref.SHAPES[name][0]()
    s = mv_ref.Slices(cfg, wl, fp, faults)
    with _sim(name, H) as g:
        g.step(100)
        s.step(100)
        act = g.activity()
        frozen = [c for c, a in enumerate(act) if a is not None]
        assert g.active_clusters() < cfg.clusters and frozen, "no cluster was frozen: the row move is not exercised"
        woken, cid = {}, 1 << 22
        for c in frozen[::5][:12]:                       # a write into a frozen cluster, on both backends
            cid = _write_cid(s, c, cid)
            assert g.commands(c, [cid]) == [s.command(c, cid)]
            g.inject(c, c % 3, cid)
            s.inject(c, c % 3, cid)
            woken[c] = cid
            cid += 1
        g.step(60)
        s.step(60)
        hist = s.histories()
        v = mv_ref.verdict(hist, cfg.clusters, 3, cfg.keys, H)
        assert v.dropped == 0 and v.longest <= H
        # injected writes were executed and put (a request the fault process drops is never retried)
        put = [c for c, cid in woken.items() if any(cid in hist[(c, r, s.command(c, cid)[0])] for r in range(3))]
        assert len(put) > len(woken) // 2, "the injected writes were not executed"
        _assert_histories(g, hist, H)                    # by cluster id, after rows have moved
        assert g.consensus() == (v.failed, s.executed_writes(), 0)
        assert g.consensus_failed() == v.masks
        assert [x.as_tuple() for x in g.read_state()] == s.read_state()
    s.close()


@contextlib.contextmanager
def _epaxos(H):
    name = "epaxos5"
    cfg, r, v = _yardstick(name, H)
    pairs = cfg.clusters * cfg.keys
    with _sim(name, H) as g:
        _run(g, name)
        yield cfg, r, v, pairs, g


def test_epaxos_reexecutions_and_a_mix_of_verdicts():
    """H = 128: the longest history of the 80 clusters has 69 values (one row; the next has 44),
    so 64 would drop 5 and the verdict would not be the reference's for every key."""
    H = 128
    with _epaxos(H) as (cfg, r, v, pairs, g):
        assert 0 < v.failed < pairs and v.dropped == 0 and v.longest <= H
        # re-executed writes: some history holds a value twice
        assert any(len(set(h)) < len(h) for h in r.hist.values())
        _assert_histories(g, r.hist, H)
        failed, versions, dropped = g.consensus()
        print("epaxos5: failed", failed, "of", pairs, "versions", versions, "longest", v.longest)
        assert (failed, versions, dropped) == (v.failed, r.executed_writes, 0)
        assert g.consensus_failed() == v.masks
        assert g.consensus_failed(70, 10) == v.masks[70:] and g.consensus_failed(80, 0) == []
        for (c, k), i in v.first.items():
            assert g.consensus_of(c, k) == (False, i)
        ok = [(c, k) for c in range(0, cfg.clusters, 9) for k in range(cfg.keys) if (c, k) not in v.first]
        assert ok and all(g.consensus_of(c, k) == (True, None) for c, k in ok)
        assert [s.as_tuple() for s in g.read_state()] == r.states


def test_overflow_counts_and_drops():
    H = 16
    with _sim("epaxos5", 0) as g:
        _run(g, "epaxos5")
        plain = ([s.as_tuple() for s in g.read_state()], g.stats().as_dict())
    with _epaxos(H) as (cfg, r, v, pairs, g):
        assert v.dropped > 0 and v.longest > H
        _assert_histories(g, r.hist, H)                  # each row holds the first 16 values
        print("epaxos5 H=16: failed", v.failed, "dropped", v.dropped)
        assert g.consensus() == (v.failed, r.executed_writes, v.dropped)
        assert g.consensus_failed() == v.masks           # Consensus over the 16-prefixes
        assert ([s.as_tuple() for s in g.read_state()], g.stats().as_dict()) == plain   # no flag is raised
        assert plain[0] == r.states


@pytest.mark.parametrize("name", ["wpaxos9", "kpaxos3"])
def test_per_key_protocols(name):
    H = 64
    cfg, r, v = _yardstick(name, H)
    assert v.failed == 0 and v.dropped == 0 and 0 < v.longest <= H
    with _sim(name, H) as g:
        _run(g, name)
        _assert_histories(g, r.hist, H)
        assert g.consensus() == (0, r.executed_writes, 0)
        assert [s.as_tuple() for s in g.read_state()] == r.states


def test_staged_violation():
    """Replicas 1 and 2 of every cluster receive a P3 for slot 0 with different writes of one key
    (paxos.go:313-343), and execute them: Consensus of that key fails at index 0."""
    from paxi_amd import trace
    clusters, N, K = 70, 5, 8
    cfg = abi.make_config(npz=[N], clusters=clusters, seed=5, kv=1, keys=K, window=16, mbox_cap=32, max_delay=0)
    wl = abi.make_workload(outstanding=1, target=[0], write_ppm=600000)
    faults = trace.replay_setup(wl, N)
    s = mv_ref.Slices(cfg, wl, None, faults)
    with Simulation(cfg, wl, None, faults) as g:
        g.latency_enable(32)
        g.multiversion_enable(8)
        staged = {}
        for c in range(clusters):
            cids = list(range(100, 164))
            cmds = g.commands(c, cids)
            assert cmds == [s.command(c, cid) for cid in cids]
            a = next(i for i, (k, w) in enumerate(cmds) if w)
            b = next(i for i, (k, w) in enumerate(cmds) if w and k == cmds[a][0] and i != a)
            staged[c] = (cmds[a][0], cids[a], cids[b])
            for sim in (g, s):
                sim.deliver(c, 1, 0, [(0, abi.MSG_P3, 0, 0, cids[a])])
                sim.deliver(c, 2, 0, [(0, abi.MSG_P3, 0, 0, cids[b])])
        g.step(1)
        s.step(1)
        hist = s.histories()
        v = mv_ref.verdict(hist, clusters, N, K, 8)
        assert v.failed == clusters and v.versions == 2 * clusters
        assert g.consensus() == (70, 140, 0)
        for c, (key, a, b) in staged.items():
            assert hist[(c, 1, key)] == [a] and hist[(c, 2, key)] == [b]
            assert g.kv_history(c, 1, key) == ([a], 0) and g.kv_history(c, 2, key) == ([b], 0)
            assert g.kv_history(c, 0, key) == ([], 0)
            for k in range(K):
                assert g.consensus_of(c, k) == ((False, 0) if k == key else (True, None))
        assert g.consensus_failed() == [1 << staged[c][0] for c in range(clusters)] == v.masks
        assert [x.as_tuple() for x in g.read_state()] == s.read_state()
    s.close()


def test_errors():
    with _sim("paxos5", 0, bins=0) as g:
        with pytest.raises(PaxisimError, match=EINVAL):
            g.multiversion_enable(64)                    # needs the recording units
    with _sim("paxos5", 0) as g:
        for call in (lambda: g.kv_history(0, 0, 0), g.consensus, g.consensus_failed, lambda: g.consensus_of(0, 0)):
            with pytest.raises(PaxisimError, match=EINVAL):
                call()                                   # every readout before enable
        for H in (0, abi.MV_MAX + 1):
            with pytest.raises(PaxisimError, match=EINVAL):
                g.multiversion_enable(H)
        g.multiversion_enable(4)
        with pytest.raises(PaxisimError, match=EINVAL):
            g.multiversion_enable(4)                     # only once
        assert g.kv_history(199, 4, 7) == ([], 0)
        with pytest.raises(PaxisimError, match=ERANGE):
            g.kv_history(200, 0, 0)
        with pytest.raises(PaxisimError, match=ERANGE):
            g.consensus_failed(190, 11)
        with pytest.raises(PaxisimError, match=EINVAL):
            g.kv_history(0, 5, 0)
        with pytest.raises(PaxisimError, match=EINVAL):
            g.kv_history(0, 0, 8)
    with _sim("paxos5", 0) as g:
        g.step(1)
        with pytest.raises(PaxisimError, match=EINVAL):
            g.multiversion_enable(64)                    # only before the first step
    cfg, wl, fp, faults = mv_ref.SHAPES["paxos5"][0]()
    cfg.kv = 0
    with Simulation(cfg, wl, fp, faults) as g:
        g.latency_enable(32)
        with pytest.raises(PaxisimError, match=EUNSUPP):
            g.multiversion_enable(64)                    # no Database
    cfg = abi.make_config(npz=(5,), protocol=abi.ABD, clusters=70, seed=5, keys=8, mbox_cap=32, max_delay=3)
    with Simulation(cfg, abi.make_workload(outstanding=4, target=[0, 1, 2, 3], write_ppm=600000)) as g:
        g.latency_enable(32)
        with pytest.raises(PaxisimError, match=EUNSUPP):
            g.multiversion_enable(64)                    # ABD keeps no put order
