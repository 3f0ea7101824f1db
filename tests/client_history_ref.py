"""Expected client-side op histories, derived from the CPU oracle as it stands.

The oracle is stepped one step at a time, as latency_ref.derive does.  A change
of a worker's (cid, issued) pair during step t is a reply accepted at t: the op
of the answered command, (key, is_write) = oracle.command(cluster, cid) with a
key beyond the key space taken as the last index (key_fit), value = the cid for
a write and the worker's new reply_value for a read (0: a read of nil), start =
the step the request was issued (start_step for the first one), end = t.  A
change from cid == 0 is a late worker's start, not an op.  The derived op count
must equal the oracle's own stats().replies.

A cluster's history is worker 0's ops in completion order, then worker 1's, ...
(the canonical order); the anomaly count is the sum of oracle_lib.linearizable
over the (cluster, key) partitions in that order.

The shapes are latency_ref's with a Database (kv = 1, except ABD) and half the
commands writes; each is derived once per process.
"""
import collections

import latency_ref
import oracle_lib
from paxi_amd import abi

# hist: [cluster][worker] -> [(key, is_write, value, start, end)]
Ref = collections.namedtuple("Ref", "hist replies states stats")


def derive(cfg, wl, fp=None, faults=(), steps=300):
    o = oracle_lib.OracleSim(cfg, wl, fp, faults)
    workers = range(wl.outstanding)
    prev = {c: [s[:2] for s in o.read_client(c)] for c in range(cfg.clusters)}
    issued_at = {c: [wl.start_step[w] for w in workers] for c in range(cfg.clusters)}
    hist = [[[] for _ in workers] for _ in range(cfg.clusters)]
    for t in range(steps):
        o.step(1)
        for c in range(cfg.clusters):
            full = o.read_client(c)
            now = [s[:2] for s in full]
            for w in workers:
                if now[w] != prev[c][w]:
                    cid = prev[c][w][0]
                    if cid != 0:
                        key, is_write = o.command(c, cid)
                        key = min(key, cfg.keys - 1)
                        hist[c][w].append((key, int(is_write), cid if is_write else full[w][2], issued_at[c][w], t))
                    issued_at[c][w] = t
            prev[c] = now
    replies = o.stats().replies
    assert sum(len(ops) for cl in hist for ops in cl) == replies
    states = [s.as_tuple() for s in o.read_state()]
    stats = o.stats().as_dict()
    o.close()
    return Ref(hist, replies, states, stats)


def canonical(cluster_hist, cap=None):
    """A cluster's ops in canonical order; cap: only each worker's first `cap` ops."""
    return [op for ops in cluster_hist for op in (ops if cap is None else ops[:cap])]


def partitions(ops):
    """{key: [(input, output, start, end)]} of ops in the given order (a write has an input, a read an output)."""
    parts = {}
    for key, is_write, value, start, end in ops:
        parts.setdefault(key, []).append((value, None, start, end) if is_write else (None, value, start, end))
    return parts


def check(histories):
    """(anomalies, ops, largest partition) of a list of per-cluster op lists."""
    anomalies = ops = largest = 0
    for h in histories:
        for part in partitions(h).values():
            anomalies += oracle_lib.linearizable(part)
            ops += len(part)
            largest = max(largest, len(part))
    return anomalies, ops, largest


def _with(shape, keys=None, kv=1, **cfg_kw):
    cfg, wl, fp, faults = shape(**cfg_kw)
    if keys is not None:
        cfg.keys = keys
    if cfg.protocol != abi.ABD:
        cfg.kv = kv
    wl.write_ppm = 500000
    return cfg, wl, fp, faults


SHAPES = {
    # 130 clusters: a partial tile; workers on replicas 0, 1, 2, so replicas 1 and 2 forward to the leader
    "paxos5": lambda: _with(latency_ref.paxos5, keys=4),
    "paxos5_compaction": lambda: _with(latency_ref.paxos5_compaction),
    "paxos9_late": lambda: _with(latency_ref.paxos9_late),
    "paxos3_max_requests": lambda: _with(latency_ref.paxos3_max_requests),
    "epaxos5_keys4": lambda: _with(latency_ref.epaxos5, keys=4),
    "epaxos5_keys1": lambda: _with(latency_ref.epaxos5, keys=1),
    "abd5": lambda: _with(latency_ref.abd5, keys=4),
    "wpaxos9": lambda: _with(latency_ref.wpaxos9),
}
_refs = {}


def ref(name, steps=300):
    """The oracle-derived client histories and final replica states of a shape after `steps` steps."""
    if (name, steps) not in _refs:
        _refs[(name, steps)] = derive(*SHAPES[name](), steps=steps)
    return _refs[(name, steps)]


# A read that returns a value overwritten before it started: w(1) [0,1], w(2) [2,3], r -> 1 [4,5].
STALE_READ = [(0, 1, 1, 0, 1), (0, 1, 2, 2, 3), (0, 0, 1, 4, 5)]
