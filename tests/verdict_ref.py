"""The yardstick of the per-cluster verdict words, built on the CPU oracle as it stands.

  flags       the OR of read_state's flags over the cluster's replicas
  AGREE       one oracle per cluster (clusters = 1, cluster_base = c, the same delivers), then check()
  CONSENSUS   mv_ref.verdict(...).masks
  LIN         the oracle's history(c) split by key through oracle_lib.linearizable
  CLIENT_LIN  client_history_ref
  WAITING     read_client: some worker's command id is non-zero
  QUIET at T  step the oracle max_delay + 2 more steps: the cluster is quiet when no replica's
              delivered[], client_requests, discarded or sent changed.  Every record in a mailbox at T
              is due within max_delay + 1 steps and is delivered or discarded when due, so the
              counters move iff some bucket holds a record.  Exact for clusters without POISON (a
              POISON cluster is frozen with its mailboxes as they were); those are reported apart.
"""
import collections

import client_history_ref
import mv_ref
import oracle_lib
from paxi_amd import abi


# ---- the shapes shared by the CPU and GPU suites (mv_ref's: seed 5, its fault process, mbox_cap 32,
# max_delay 3, 8 keys) -------------------------------------------------------------------------------
def paxos3(clusters=200, **kw):
    """Multi-Paxos N = 3, 3 workers of 6 requests each: with Drop faults some clusters stall."""
    return mv_ref._shape((3,), clusters, max_requests=6, **kw)


def wpaxos9(clusters, **kw):
    """WPaxos 3x3, W = 8, 9 workers of 6 requests each."""
    return mv_ref._shape((3, 3, 3), clusters, protocol=abi.WPAXOS, window=8, max_requests=6, **kw)


def abd3(clusters=200):
    """ABD N = 3, 4 keys, history 256, half writes, 3 workers."""
    cfg = abi.make_config(protocol=abi.ABD, npz=(3,), clusters=clusters, seed=5, mbox_cap=32, max_delay=3, keys=4,
                          history=256)
    wl = abi.make_workload(outstanding=3, target=[0, 1, 2], write_ppm=500000)
    return cfg, wl, mv_ref._fp(), ()


PAXOS3_STEP, WPAXOS9_STEP, WPAXOS9_AGREE_STEP, ABD3_STEP = 33, 34, 100, 150
WPAXOS9_AGREE_SET = [181]   # of wpaxos9(200) at step 100
# paxos3's workers run almost in lockstep: at step 20 a sixth reply has arrived in 198 of the 200
# clusters, so client-history rows of 5 ops overflow in those and not in the other two
CHIST_STEP, CHIST_CAP = 20, 5

Words = collections.namedtuple("Words", "words poison late_only")


def _activity(o, N):
    st = o.read_state()
    return [tuple((tuple(st[c * N + r].delivered), st[c * N + r].client_requests, st[c * N + r].discarded,
                   st[c * N + r].sent) for r in range(N)) for c in range(o.cfg.clusters)]


def words(cfg, wl, fp, faults=(), steps=0, drive=None):
    """Flags, QUIET, WAITING and STALLED of every cluster after `steps` steps (or after drive(sim)):
    Words(the words; the clusters with POISON, whose QUIET is not the yardstick's to say; the running
    clusters whose next-step inboxes are all empty, their records being in a later arrival bucket)."""
    o = oracle_lib.OracleSim(cfg, wl, fp, faults)
    if drive:
        drive(o)
    else:
        o.step(steps)
    N = o.N
    st = o.read_state()
    flags = [0] * cfg.clusters
    for c in range(cfg.clusters):
        for r in range(N):
            flags[c] |= st[c * N + r].flags & abi.V_FLAGS
    waiting = [any(w[0] != 0 for w in o.read_client(c)) for c in range(cfg.clusters)]
    inbox_empty = [all(not o.read_inbox(c, r) for r in range(N)) for c in range(cfg.clusters)]
    before = _activity(o, N)
    o.step(cfg.max_delay + 2)
    after = _activity(o, N)
    o.close()
    out, poison, late_only = [], [], []
    for c in range(cfg.clusters):
        w = flags[c]
        quiet = before[c] == after[c]
        if w & abi.F_POISON:
            poison.append(c)
            quiet = False
        if quiet:
            w |= abi.V_QUIET
        elif inbox_empty[c] and not (w & abi.F_POISON):
            late_only.append(c)
        if waiting[c]:
            w |= abi.V_WAITING
        if quiet and waiting[c]:
            w |= abi.V_STALLED
        out.append(w)
    return Words(out, poison, late_only)


LIVE = abi.V_FLAGS | abi.V_QUIET | abi.V_WAITING | abi.V_STALLED   # the bits words() speaks of


def populations(ws):
    """(running, finished, stalled) cluster counts of a words() result."""
    running = sum(1 for w in ws if not w & abi.V_QUIET)
    stalled = sum(1 for w in ws if w & abi.V_STALLED)
    return running, len(ws) - running - stalled, stalled


def agree(cfg, wl, fp, faults=(), steps=0, drive=None):
    """The clusters paxisim_check counts: every cluster stepped as an oracle of its own."""
    bad = []
    for c in range(cfg.clusters):
        one = type(cfg).from_buffer_copy(cfg)
        one.clusters, one.cluster_base = 1, cfg.cluster_base + c
        o = oracle_lib.OracleSim(one, wl, fp, faults)
        if drive:
            drive(o, c)
        else:
            o.step(steps)
        if o.check():
            bad.append(c)
        o.close()
    return bad


def lin(cfg, wl, fp, faults=(), steps=0):
    """ABD: (anomalies per cluster, ops, the oracle's own totals) from history(c) split by key."""
    o = oracle_lib.OracleSim(cfg, wl, fp, faults)
    o.step(steps)
    per, ops = [], 0
    for c in range(cfg.clusters):
        h = o.history(c)
        ops += len(h)
        per.append(sum(oracle_lib.linearizable(p) for p in client_history_ref.partitions(h).values()))
    total = o.linearizable()
    o.close()
    return per, ops, total


_cache = {}


def cached(key, fn):
    """Compute a yardstick once and share it among the tests that need it."""
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]
