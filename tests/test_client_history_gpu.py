"""The client-side op history recorded on the device (chist_kernel.h) against
the oracle-derived histories of client_history_ref: every cluster's history op for op in
canonical order, the on-device linearizability count against oracle_lib.linearizable over the
same partitions, and the replica states still the oracle's with recording on - in every kernel
form and for every protocol."""
import numpy as np
import pytest

import client_history_ref as chr_
from paxi_amd import abi
from paxi_amd.sim import PaxisimError, Simulation

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPP = r"error -1:", r"error -4:"


def _sim(name, cap, bins=32, history=0):
    cfg, wl, fp, faults = chr_.SHAPES[name]()
    cfg.history = history
    g = Simulation(cfg, wl, fp, faults)
    if bins:
        g.latency_enable(bins)
    if cap:
        g.client_history_enable(cap)
    return g


def _assert_histories(g, r, cap=None):
    """Every cluster's history equals the yardstick's op for op (cap: each worker's first `cap`
    ops, the rest dropped); returns the yardstick's per-cluster op lists."""
    want = [chr_.canonical(h, cap) for h in r.hist]
    dropped = 0
    for c, w in enumerate(want):
        ops, d = g.client_history(c)
        assert ops == w, f"cluster {c}: history differs from the yardstick"
        assert d == sum(len(x) for x in r.hist[c]) - len(w), f"cluster {c}: dropped"
        dropped += d
    return want, dropped


def _check(name, cap, schedule=(150, 150)):
    r = chr_.ref(name, sum(schedule))
    with _sim(name, cap) as g:
        for n in schedule:
            g.step(n)
        want, dropped = _assert_histories(g, r)
        assert dropped == 0
        anomalies, ops, largest = chr_.check(want)
        got = g.client_linearizable()
        print(name, "anomalies, ops, skipped", got, "yardstick", (anomalies, ops), "largest partition", largest)
        assert got == (anomalies, ops, 0) and ops == r.replies == g.stats().replies
        assert [s.as_tuple() for s in g.read_state()] == r.states, "replica states differ from the oracle"
        return anomalies, largest


@pytest.mark.parametrize("env", [{}, {"PAXISIM_SERIAL": "0"}, {"PAXISIM_PIPE": "1"}],
                         ids=["default", "serial0", "pipe1"])
def test_paxos5_partial_tile_every_kernel_form(monkeypatch, env):
    """130 clusters (a partial tile), workers on replicas 0, 1, 2: replicas 1 and 2 forward."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    anomalies, _ = _check("paxos5", 128)
    assert anomalies == 0


def test_compaction_leaves_the_history_with_its_cluster():
    name, schedule = "paxos5_compaction", (75, 75, 75, 75)
    r = chr_.ref(name)
    with _sim(name, 128) as g:
        for n in schedule[:3]:
            g.step(n)
        active, replies = g.active_clusters(), g.stats().replies
        assert active < 192, "no cluster was frozen: the row move is not exercised"
        g.step(schedule[3])
        assert g.stats().replies > replies, "no reply after the compaction"
        want, dropped = _assert_histories(g, r)          # by cluster id, after rows have moved
        assert dropped == 0
        assert g.client_linearizable() == chr_.check(want)[:2] + (0,)
        assert [s.as_tuple() for s in g.read_state()] == r.states


def test_late_workers_start_is_no_op():
    """The 9-replica idle-skip unit; workers 2 and 3 start at steps 40 and 41."""
    _check("paxos9_late", 128)
    r = chr_.ref("paxos9_late")
    assert all(cl[2][0][3] == 40 and cl[3][0][3] == 41 for cl in r.hist)


def test_finished_worker_keeps_its_last_op():
    _check("paxos3_max_requests", 16)
    assert all([len(ops) for ops in cl] == [10, 10] for cl in chr_.ref("paxos3_max_requests").hist)


def test_epaxos_anomalies_register_path():
    anomalies, largest = _check("epaxos5_keys4", 128)
    assert anomalies > 0 and largest <= 128, "every partition is meant to fit the register checker"


def test_epaxos_one_key_big_path():
    """Partitions of about 300 ops: lin_big_kernel reads the stage the client instance wrote."""
    assert max(len(ops) for cl in chr_.ref("epaxos5_keys1").hist for ops in cl) <= 64
    anomalies, largest = _check("epaxos5_keys1", 64)
    assert anomalies > 0 and largest > 128


def test_abd_client_side_and_replica_side_histories():
    anomalies, _ = _check("abd5", 128)
    assert anomalies > 0
    with _sim("abd5", 0, bins=0, history=128) as g:      # the replica-side history alone
        g.step(300)
        alone = g.linearizable()
    with _sim("abd5", 128, history=128) as g:
        g.step(300)
        assert g.linearizable() == alone and alone[1] > 0
        assert g.client_linearizable()[0] == anomalies


def test_wpaxos9_colocated_blocks():
    _check("wpaxos9", 128)


def test_overflow_counts_and_drops():
    name, cap = "paxos5", 8
    r = chr_.ref(name)
    with _sim(name, cap) as g:
        g.step(150)
        g.step(150)
        want, dropped = _assert_histories(g, r, cap)     # each worker's first 8 ops
        assert all(len(w) == 3 * cap for w in want)
        assert dropped == r.replies - sum(len(w) for w in want) > 0
        assert g.client_linearizable() == chr_.check(want)[:2] + (0,)
        assert g.stats().as_dict() == r.stats            # no flag is raised
        assert [s.as_tuple() for s in g.read_state()] == r.states


def _deal(ops, workers):
    """ops dealt round-robin over `workers` workers; returns ([worker] -> ops, the canonical order)."""
    rows = [ops[w::workers] for w in range(workers)]
    return rows, [op for row in rows for op in row]


def _random_ops(rng, n, keys, t0=10):
    """n ops over `keys` keys: writes of fresh values; reads return the latest, an older or no write of the key."""
    ops, written, t, nextv = [], {k: [0] for k in range(keys)}, t0, 1000
    for _ in range(n):
        k = int(rng.integers(keys))
        start = t + int(rng.integers(3))
        end = start + 1 + int(rng.integers(6))
        t += int(rng.integers(2))
        if rng.integers(2):
            ops.append((k, 1, nextv, start, end))
            written[k].append(nextv)
            nextv += 1
        else:
            vals = written[k]
            v = vals[-1] if rng.integers(4) else vals[int(rng.integers(len(vals)))]
            ops.append((k, 0, v, start, end))
    return ops


def test_load_32_workers_and_both_checker_paths():
    """A handle with 32 workers, never stepped.  The history is dealt over all 32 workers: a
    length array of 16 entries (the replicas' bound) would lose workers 16-31."""
    WK, cap = 32, 64
    cfg = abi.make_config(npz=(5,), clusters=3, seed=11, keys=4, kv=1, mbox_cap=32)
    wl = abi.make_workload(outstanding=WK, target=0, write_ppm=500000)
    rng = np.random.default_rng(17)
    with Simulation(cfg, wl) as g:
        g.latency_enable(32)
        g.client_history_enable(cap)
        # cluster 0: the stale read and 300 random ops on 4 keys (partitions of about 75: registers)
        rows0, can0 = _deal(chr_.STALE_READ + _random_ops(rng, 300, 4), WK)
        # cluster 1: exactly 128 ops on key 0 (the register checker's largest) and 129 on key 1 (the big path)
        a = [(0,) + op[1:] for op in _random_ops(rng, 128, 1)]
        b = [(1,) + op[1:] for op in _random_ops(rng, 129, 1)]
        mixed = [op for pair in zip(a, b) for op in pair] + [b[-1]]
        rows1, can1 = _deal(mixed, WK)
        for c, rows in ((0, rows0), (1, rows1)):
            for w, row in enumerate(rows):
                g.client_history_load(c, w, row)
        assert g.client_history(0) == (can0, 0) and g.client_history(1) == (can1, 0)
        assert g.client_history(2) == ([], 0)
        want = chr_.check([can0, can1])
        parts1 = {k: len(v) for k, v in chr_.partitions(can1).items()}
        assert parts1 == {0: 128, 1: 129}
        per_key = {k: chr_.check([[op for op in can1 if op[0] == k]])[0] for k in (0, 1)}
        print("anomalies", want, "cluster 1 per key", per_key)
        assert chr_.check([can0])[0] >= 1 and per_key[0] > 0 and per_key[1] > 0
        assert g.client_linearizable() == want[:2] + (0,)
        # each path alone: cluster 1 reduced to one key
        for k in (0, 1):
            for w, row in enumerate(rows1):
                g.client_history_load(1, w, [op for op in row if op[0] == k])
            for w in range(WK):
                g.client_history_load(0, w, [])
            assert g.client_linearizable() == (per_key[k], parts1[k], 0)
        with pytest.raises(PaxisimError, match=EINVAL):
            g.client_history_load(0, 0, [(4, 0, 1, 0, 1)])          # keys = 4
        with pytest.raises(PaxisimError, match=EINVAL):
            g.client_history_load(0, 0, [(0, 2, 1, 0, 1)])          # is_write is 0 or 1
        with pytest.raises(PaxisimError, match=EINVAL):
            g.client_history_load(0, 0, [(0, 0, 1, 0, 1)] * (cap + 1))
        with pytest.raises(PaxisimError):
            g.client_history_load(0, WK, [])


def test_identity_and_errors():
    r = chr_.ref("paxos5")
    with _sim("paxos5", 0) as g:                         # latency only
        with pytest.raises(PaxisimError, match=EINVAL):
            g.client_history(0)                          # readout before enable
        with pytest.raises(PaxisimError, match=EINVAL):
            g.client_linearizable()
        with pytest.raises(PaxisimError, match=EINVAL):
            g.client_history_load(0, 0, [])
        with pytest.raises(PaxisimError, match=EINVAL):
            g.client_history_enable(0)
        g.step(150)
        g.step(150)
        with pytest.raises(PaxisimError, match=EINVAL):
            g.client_history_enable(64)                  # only before the first step
        stats = g.stats().as_dict()
        lat = [g.latency(w) for w in [None, 0, 1, 2]]
    with _sim("paxos5", 64) as g:
        with pytest.raises(PaxisimError, match=EINVAL):
            g.client_history_enable(64)                  # only once
        g.step(150)
        g.latency_reset()                                # leaves the history alone
        g.step(150)
        assert g.stats().as_dict() == stats == r.stats
        ops, dropped = g.client_history(129)
        assert ops == chr_.canonical(r.hist[129], 64) and len(ops) + dropped == sum(len(x) for x in r.hist[129])
    with _sim("paxos5", 64) as g:                        # the histograms with recording on
        g.step(150)
        g.step(150)
        assert [g.latency(w) for w in [None, 0, 1, 2]] == lat
    with _sim("paxos5", 0, bins=0) as g:
        with pytest.raises(PaxisimError, match=EINVAL):
            g.client_history_enable(64)                  # needs the recording units and the stamps
    cfg, wl, fp, faults = chr_.SHAPES["paxos5"]()
    cfg.kv = 0
    with Simulation(cfg, wl, fp, faults) as g:
        g.latency_enable(32)
        with pytest.raises(PaxisimError, match=EUNSUPP):
            g.client_history_enable(64)                  # replies carry no read values
