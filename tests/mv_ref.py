"""Expected multi-version Database histories, derived from the CPU oracle as it stands.

Paxi's Database appends every written value to history[key] (db.go:123-134), so a replica's
History(k) is its execution log filtered to the writes of key k: for the per-key protocols
(abi.PER_KEY) the writes of exec_log(c, r, key=k), otherwise the writes of exec_log(c, r) whose
command() key is k (a key beyond the key space taken as the last index, as the replicas do).  A
write's value is its command id.

The oracle keeps execution logs only for handles of at most 16 clusters, and its PRNG is keyed by
the global cluster id, so a C-cluster run is derived as ceil(C / 16) oracle handles of 16 clusters
each with cluster_base = 0, 16, 32, ... (the last one partial).  tests/test_multiversion.py checks
that a slice equals the same clusters of one large handle.

Consensus (client.go:279-320) over the histories is sim.consensus_of_histories; `direct` below is an
independent restatement used to check it.
"""
import collections

import oracle_lib
from paxi_amd import abi
from paxi_amd.sim import consensus_of_histories

SLICE = 16


def _copy(struct):
    return type(struct).from_buffer_copy(struct)


class Slices:
    """A C-cluster oracle run as handles of at most 16 clusters; clusters are addressed by their
    index in the whole run, as on the device."""

    def __init__(self, cfg, wl, fp=None, faults=()):
        self.cfg, self.wl, self.N = cfg, wl, abi.n_replicas(cfg)
        self.parts = []
        self._keep = []
        for base in range(0, cfg.clusters, SLICE):
            c = _copy(cfg)
            c.clusters = min(SLICE, cfg.clusters - base)
            c.cluster_base = cfg.cluster_base + base
            self._keep.append(c)
            self.parts.append(oracle_lib.OracleSim(c, wl, fp, faults))
        self._cmd = {}

    def _at(self, cluster):
        return self.parts[cluster // SLICE], cluster % SLICE

    def step(self, n):
        for p in self.parts:
            p.step(n)

    def inject(self, cluster, replica, cid):
        p, c = self._at(cluster)
        p.inject(c, replica, cid)

    def deliver(self, cluster, replica, src, recs):
        p, c = self._at(cluster)
        p.deliver(c, replica, src, recs)

    def command(self, cluster, cid):
        if (cluster, cid) not in self._cmd:
            p, c = self._at(cluster)
            k, w = p.command(c, cid)
            self._cmd[(cluster, cid)] = (min(k, self.cfg.keys - 1), w)
        return self._cmd[(cluster, cid)]

    def read_state(self):
        return [s.as_tuple() for p in self.parts for s in p.read_state()]

    def executed_writes(self):
        return sum(s.executed_writes for p in self.parts for s in p.read_state())

    def read_kv(self, cluster, replica):
        p, c = self._at(cluster)
        return p.read_kv(c, replica, self.cfg.keys)

    def history(self, cluster, replica, key):
        """Database.History(key) of one replica: the values put, in put order."""
        p, c = self._at(cluster)
        if self.cfg.protocol in abi.PER_KEY:
            return [cid for cid in p.exec_log(c, replica, key) if self.command(cluster, cid)[1]]
        return [cid for cid in p.exec_log(c, replica) if self.command(cluster, cid) == (key, True)]

    def histories(self):
        """{(cluster, replica, key): History}"""
        out = {}
        for cl in range(self.cfg.clusters):
            p, c = self._at(cl)
            for r in range(self.N):
                if self.cfg.protocol in abi.PER_KEY:
                    for k in range(self.cfg.keys):
                        out[(cl, r, k)] = [cid for cid in p.exec_log(c, r, k) if self.command(cl, cid)[1]]
                else:
                    rows = [[] for _ in range(self.cfg.keys)]
                    for cid in p.exec_log(c, r):
                        k, w = self.command(cl, cid)
                        if w:
                            rows[k].append(cid)
                    for k in range(self.cfg.keys):
                        out[(cl, r, k)] = rows[k]
        return out

    def close(self):
        for p in self.parts:
            p.close()


def direct(histories):
    """Consensus restated without the reference's loop: every pair of replicas agrees on the common
    prefix of their histories.  (ok, the first index at which some pair differs)."""
    first = None
    for a in range(len(histories)):
        for b in range(a + 1, len(histories)):
            for i, (x, y) in enumerate(zip(histories[a], histories[b])):
                if x != y:
                    first = i if first is None else min(first, i)
                    break
    return first is None, first


Verdict = collections.namedtuple("Verdict", "failed versions dropped masks first longest")


def verdict(hist, clusters, N, keys, cap=None):
    """What the device must report for the histories `hist` with `cap` values kept per row: the
    failing (cluster, key) pairs, the values ever put, the values dropped, the per-cluster masks of
    failing keys, {(cluster, key): first failing index} and the longest history."""
    failed = versions = dropped = longest = 0
    masks, first = [0] * clusters, {}
    for c in range(clusters):
        for k in range(keys):
            rows = [hist[(c, r, k)] for r in range(N)]
            versions += sum(len(h) for h in rows)
            longest = max([longest] + [len(h) for h in rows])
            if cap is not None:
                dropped += sum(max(0, len(h) - cap) for h in rows)
                rows = [h[:cap] for h in rows]
            ok, i = consensus_of_histories(rows)
            if not ok:
                failed += 1
                masks[c] |= 1 << k
                first[(c, k)] = i
    return Verdict(failed, versions, dropped, masks, first, longest)


# ---- the shapes shared by the CPU and GPU suites --------------------------------------------------
def _fp():
    return abi.make_fault_process(drop_ppm=1000, drop_len=10, slow_ppm=2000, slow_len=10, slow_min=1, slow_max=3)


def _shape(npz, clusters, protocol=abi.PAXOS, window=16, keys=8, workers=None, **kw):
    N = sum(npz)
    workers = N if workers is None else workers
    wl_kw = {k: kw.pop(k) for k in ("max_requests",) if k in kw}
    cfg = abi.make_config(npz=npz, protocol=protocol, clusters=clusters, seed=5, kv=1, mbox_cap=32, max_delay=3,
                          keys=keys, window=window, **kw)
    wl = abi.make_workload(outstanding=workers, target=list(range(workers)), write_ppm=600000, **wl_kw)
    return cfg, wl, _fp(), ()


SHAPES = {
    # three tiles and a partial one
    "paxos5": (lambda: _shape((5,), 200), (150, 150)),
    # workers stop after 6 requests each, at different steps: clusters freeze one by one
    "paxos3_freeze": (lambda: _shape((3,), 200, max_requests=6, ephemeral_leader=1, steps_per_launch=8), (100,)),
    # a tile and a partial one
    "epaxos5": (lambda: _shape((5,), 80, protocol=abi.EPAXOS, window=32), (40,)),
    # W = 8: the co-located instance blocks
    "wpaxos9": (lambda: _shape((3, 3, 3), 100, protocol=abi.WPAXOS, window=8), (150,)),
    "kpaxos3": (lambda: _shape((3,), 100, protocol=abi.KPAXOS), (150,)),
}
Ref = collections.namedtuple("Ref", "hist states executed_writes kv")
_refs = {}


def ref(name):
    """The yardstick of a shape after its schedule: histories, replica states, the sum of
    executed_writes and every replica's Database {(cluster, replica): [value per key]}."""
    if name not in _refs:
        make, schedule = SHAPES[name]
        cfg, wl, fp, faults = make()
        s = Slices(cfg, wl, fp, faults)
        for n in schedule:
            s.step(n)
        kv = {(c, r): s.read_kv(c, r) for c in range(cfg.clusters) for r in range(s.N)}
        _refs[name] = Ref(s.histories(), s.read_state(), s.executed_writes(), kv)
        s.close()
    return _refs[name]
