"""Expected client request latencies, derived from the CPU oracle as it stands.

A closed-loop worker has one request in flight and a reply issues the next
request in the same step, so the oracle needs no latency code of its own: step
it one step at a time and watch read_client.  A change of a worker's
(cid, issued) pair during step t is a reply accepted at t, with latency t minus
the step the answered request was issued at (start_step for the first one).  A
change from cid == 0 is a late worker's start, not a sample.  The derived sample
count must equal the oracle's own stats().replies.

The shapes are shared by the CPU and GPU tests; each is run once per process.
"""
import collections

import numpy as np

import oracle_lib
from paxi_amd import abi
from paxi_amd.latency import Histogram

Ref = collections.namedtuple("Ref", "samples replies states")   # samples: {worker: [(reply step, latency)]}


def derive(cfg, wl, fp=None, faults=(), steps=300):
    o = oracle_lib.OracleSim(cfg, wl, fp, faults)
    workers = range(wl.outstanding)
    prev = {c: [s[:2] for s in o.read_client(c)] for c in range(cfg.clusters)}
    issued_at = {c: [wl.start_step[w] for w in workers] for c in range(cfg.clusters)}
    samples = {w: [] for w in workers}
    for t in range(steps):
        o.step(1)
        for c in range(cfg.clusters):
            now = [s[:2] for s in o.read_client(c)]
            for w in workers:
                if now[w] != prev[c][w]:
                    if prev[c][w][0] != 0:
                        samples[w].append((t, t - issued_at[c][w]))
                    issued_at[c][w] = t
            prev[c] = now
    replies = o.stats().replies
    assert sum(len(v) for v in samples.values()) == replies
    states = [s.as_tuple() for s in o.read_state()]
    o.close()
    return Ref(samples, replies, states)


def paxos5(clusters=130, **cfg):
    return (abi.make_config(npz=(5,), clusters=clusters, seed=7, **cfg),
            abi.make_workload(outstanding=3, target=[0, 1, 2]), None, ())


def paxos5_faulted():
    cfg, wl, _, _ = paxos5(max_delay=8)
    fp = abi.make_fault_process(slow_ppm=20000, slow_len=20, slow_min=1, slow_max=8)
    return cfg, wl, fp, (abi.make_fault(abi.FAULT_FLAKY, 0, param=50000, step_from=50, step_to=150),)


def paxos9_late():
    return (abi.make_config(npz=(3, 3, 3), clusters=70, seed=7),
            abi.make_workload(outstanding=4, target=[0, 1, 2, 3], start_step=[0, 0, 40, 41]), None, ())


def paxos3_max_requests():
    return (abi.make_config(npz=(3,), clusters=66, seed=5),
            abi.make_workload(outstanding=2, target=[0, 1], start_step=[0, 40], max_requests=10), None, ())


# Clusters [0, 64) and [128, 192) lose replica 0 - the target of both workers and so the leader - for
# good at step CRASH_AT: it discards what it receives and nothing it sends arrives, no other replica
# has anything to send (Paxi has no timers), so those clusters' mailboxes drain and compaction freezes
# them, while [64, 128) keeps running and its rows move to the front.
CRASH_AT = 30


def paxos5_compaction():
    cfg = abi.make_config(npz=(5,), clusters=192, seed=7)
    wl = abi.make_workload(outstanding=2, target=0)
    faults = tuple(abi.make_fault(abi.FAULT_CRASH, 0, cluster_lo=lo, cluster_hi=lo + 64, step_from=CRASH_AT)
                   for lo in (0, 128))
    return cfg, wl, None, faults


def abd5():
    return (abi.make_config(npz=(5,), protocol=abi.ABD, clusters=70, seed=3),
            abi.make_workload(outstanding=4, target=[0, 1, 2, 3], write_ppm=500000), None, ())


def wpaxos9():
    return (abi.make_config(npz=(3, 3, 3), protocol=abi.WPAXOS, clusters=70, seed=3, keys=8, window=8),
            abi.make_workload(outstanding=9, target=list(range(9)), locality_ppm=700000, keys=8), None, ())


def epaxos5():
    return (abi.make_config(npz=(5,), protocol=abi.EPAXOS, clusters=70, seed=3),
            abi.make_workload(outstanding=5, target=list(range(5))), None, ())


SHAPES = {f.__name__: f for f in (paxos5, paxos5_faulted, paxos9_late, paxos3_max_requests, paxos5_compaction,
                                  abd5, wpaxos9, epaxos5)}
_refs = {}


def ref(name, steps=300):
    """The oracle's samples and final replica states of a shape after `steps` steps."""
    if (name, steps) not in _refs:
        _refs[(name, steps)] = derive(*SHAPES[name](), steps=steps)
    return _refs[(name, steps)]


def expected(r, bins, worker=None, since=0):
    """The Histogram of a worker's (None: every worker's) samples whose reply step is >= since."""
    ws = r.samples if worker is None else [worker]
    return Histogram.from_samples(np.array([lat for w in ws for t, lat in r.samples[w] if t >= since], dtype=np.int64),
                                  bins)
