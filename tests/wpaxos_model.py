"""WPaxos, M2Paxos and KPaxos replicas on unbounded maps, for the trace replay of
tests/paxos_model.py.

The CPU oracle and the HIP kernels share one bounded reading of the per-key protocols: a window of W
slots and a ghost table per instance, `exists` bits in place of `map[Key]*kpaxos`, one forwards
table of 32 entries, u16 hit counts visited in index order, the step as the policy clock.  This
model is restated from the Go and shares none of it: `paxi` is a dict that only `init` fills, each
kpaxos is one `paxos_model.Paxos` on an unbounded dict log with a policy object of plain Python
ints and floats, and `forwards`, the Database and the counters are `paxos_model.Replica`'s, one per
replica across all keys.

What is taken from the project and not from Go, each a choice Go leaves to its runtime or a piece
of plumbing: the record encodings of DESIGN.md §3.2 / §3.5b (the key in bits 16-31 of the header,
LeaderChange as {LEADERCHG | key << 16, ballot, to, from}); the step as the clock of `majority`;
the highest index among the ids that qualify in `majority` (Go ranges over a map), counted in
`Majority.ties`; and the key-tagged P2a of a thrifty leader, counted in `WReplica.thrifty_p2as`
(kpaxos wraps Broadcast and Send only, kpaxos.go:51-74, so Go's MulticastQuorum, paxos.go:127,
sends a bare paxos.P2a for which no per-key replica registers a handler, node.go:109-112).
"""
import collections
import math
import struct

import paxos_model as pm
from paxi_amd import abi
from paxos_model import (GHOST, POISON, T_LEADERCHG, T_P1A, T_P1B, T_P2A, T_P2B, T_P3, T_REPLY, T_REQUEST, WOVF,
                         Panic, Paxos, Replica, Request, Chan, CLIENT, i32)


# ---- policy.go -------------------------------------------------------------------------------------
class Null:
    """policy.go:132-136, and NewPolicy's "" / "null" (policy.go:18-23)."""

    def hit(self, r, now):
        return None

    def expect(self):
        return {"policy_last": 0xFF, "policy_hits": 0}


class Consecutive:
    """policy.go:49-69: n consecutive hits of one id return it, and `last` is "" again."""

    def __init__(self, n):
        self.last, self.hits, self.n = None, 0, n

    def hit(self, r, now):
        res = None
        if r == self.last:
            self.hits += 1
        else:
            self.last, self.hits = r, 1
        if self.hits >= self.n:
            res, self.last, self.hits = self.last, None, 0
        return res

    def expect(self):
        return {"policy_last": 0xFF if self.last is None else self.last, "policy_hits": self.hits}


class Majority:
    """policy.go:71-102 with the step as time.Now(): created with its kpaxos (policy.go:30-35), so
    the creation step starts the first interval.  Go ranges over a map and keeps the last id with
    n >= sum / 2; of several such ids the highest index is taken and the case is
    counted in `ties`."""

    def __init__(self, interval, now):
        self.hits, self.interval, self.time, self.sum, self.ties = collections.Counter(), interval, now, 0, 0

    def hit(self, r, now):
        self.hits[r] += 1
        self.sum += 1
        res = None
        if self.sum > 1 and now - self.time >= self.interval:
            ok = [i for i, n in self.hits.items() if n >= self.sum // 2]
            if ok:
                res = max(ok)
                self.ties += len(ok) > 1
            for i in self.hits:
                self.hits[i] = 0
            self.sum, self.time = 0, now
        return res

    def expect(self):
        return {"policy_state": (self.sum, self.time)}     # the per-id hash of word 2 is not documented


def go_round(x):
    """math.Round: half away from zero (x >= 0 here)."""
    f = math.floor(x)
    return f + 1 if x - f >= 0.5 else f


class Ema:
    """policy.go:104-130 on Python floats: every product and the sum are rounded on their own."""

    def __init__(self, alpha, zone_of, first_of):
        self.alpha, self.s, self.epsilon, self.zone, self.zone_of, self.first_of = alpha, 0.0, 0.1, 0, zone_of, first_of

    def hit(self, r, now):
        z = float(self.zone_of(r))
        if self.s == 0:
            self.s = z
            return None
        a = self.alpha * z
        b = (1 - self.alpha) * self.s
        self.s = a + b
        if abs(self.s - go_round(self.s)) > self.epsilon:
            return None
        z = int(go_round(self.s))
        if z != self.zone:
            self.zone = z
            return self.first_of(z)                        # NewID(zone, 1)
        return None

    def expect(self):
        lo, hi = struct.unpack("<II", struct.pack("<d", self.s))
        return {"policy_state": (lo, hi, self.zone)}


class KPaxos(Paxos):
    """wpaxos/kpaxos.go:8-48, m2paxos/kpaxos.go:8-42: a paxos.Paxos whose Broadcast and Send tag
    P1a..P3 with the key (kpaxos.go:51-74; here `tag`), and a Policy.  KPaxos' instances are bare
    paxos.Paxos (kpaxos/replica.go:46-50) tagged with the replica's working key: policy None."""

    def __init__(self, node, key, q1, q2, thrifty, policy):
        super().__init__(node, q1, q2, thrifty, False, key << 16)
        self.key, self.policy = key, policy if policy is not None else Null()


class WReplica(Replica):
    """wpaxos/replica.go, m2paxos/replica.go, kpaxos/replica.go over paxos_model.Replica's node:
    forwards, the Database and the counters are the replica's, shared by all keys."""

    def __init__(self, me, cfg, client, command_of, key_value=None):
        super().__init__(me, cfg, client, command_of)
        self.cfg, self.proto, self.adaptive = cfg, cfg.protocol, bool(cfg.adaptive)
        self.paxi = {}                                     # map[paxi.Key]*kpaxos: only init fills it
        self.key_value = key_value or (lambda k: k)
        self.thrifty_p2as = self.reply_values = 0
        if self.proto == abi.WPAXOS:                       # wpaxos/kpaxos.go:15-27
            self.q = (abi.Q_GRID_ROW, abi.Q_GRID_COLUMN) if cfg.fz == 0 else (abi.Q_FGRID_Q1, abi.Q_FGRID_Q2)
        else:                                              # m2paxos/kpaxos.go:15-21; paxos.go:48-49
            self.q = (abi.Q_MAJORITY, abi.Q_MAJORITY)

    def new_paxos(self, cfg):
        return None

    def instances(self):
        return self.paxi

    def id_of(self, zone, node=1):
        """The replica index of ID "zone.node", or None where the configuration has none."""
        return self.ids.index((zone, node)) if (zone, node) in self.ids else None

    def new_policy(self):
        """NewPolicy (policy.go:15-47); KPaxos has none."""
        cfg = self.cfg
        if self.proto == abi.KPAXOS:
            return None
        if cfg.policy == abi.POLICY_MAJORITY:
            return Majority(cfg.policy_interval, self.client.step)
        if cfg.policy == abi.POLICY_EMA:
            return Ema(cfg.policy_alpha, lambda r: self.ids[r][0], self.id_of)
        return Consecutive(cfg.policy_threshold) if cfg.policy_threshold else Null()

    def init(self, key):
        """replica.go:36-40."""
        if key not in self.paxi:
            self.paxi[key] = KPaxos(self, key, self.q[0], self.q[1], bool(self.cfg.thrifty), self.new_policy())

    def get(self, key, what):
        """r.paxi[m.Key] without init (replica.go:78-82, 90-93, 101-104): a nil *kpaxos."""
        if key not in self.paxi:
            raise Panic(f"replica {self.me}: {what} for key {key}, which it never initialised")
        return self.paxi[key]

    def send(self, dst, *words):
        self.reply_values += words[0] == T_REPLY and words[1] != 0
        super().send(dst, *words)

    def multicast_quorum(self, q, *words):
        self.thrifty_p2as += 1
        super().multicast_quorum(q, *words)

    def kp_index(self, key):
        """index (kpaxos/replica.go:32-44) on the key value: "z.1"."""
        v = self.key_value(key)
        return self.id_of(1 + (v // 200 if v < 800 else 4))

    def handle_request(self, r):
        key = self.command_of(r.cid)[0]
        self.init(key)
        p = self.paxi[key]
        if self.proto == abi.KPAXOS:                       # kpaxos/replica.go:52-62
            leader = self.kp_index(key)
            if leader == self.me:
                p.handle_request(r)
            else:
                self.forward(leader, r)
        elif self.adaptive or self.proto == abi.M2PAXOS:   # wpaxos/replica.go:48-62, m2paxos/replica.go:42-55
            if p.is_leader() or p.ballot == 0:
                p.handle_request(r)
                to = p.policy.hit(r.node_id, self.client.step)
                if to is not None and self.ids[to][0] != self.ids[self.me][0]:
                    self.send(to, T_LEADERCHG | p.tag, p.ballot, to, self.me)
            else:
                self.forward(p.leader(), r)
        else:                                              # wpaxos/replica.go:63-65
            p.handle_request(r)

    def handle_leader_change(self, key, ballot, to):
        """wpaxos/replica.go:101-108, m2paxos/replica.go:86-93."""
        p = self.get(key, "LeaderChange")
        if ballot == p.ballot and to == self.me:
            p.p1a()

    def handle(self, src, words):
        t, key, b, s, cid = words[0] & 0xFF, words[0] >> 16, words[1], i32(words[2]), words[3]
        try:
            if t == T_REQUEST:
                http = src == self.N
                self.handle_request(Request(cid, self.me if http else src, Chan(CLIENT if http else src)))
            elif t == T_REPLY:
                assert cid in self.forwards, f"replica {self.me}: Reply for {cid}, which it never forwarded"
                self.reply(self.forwards[cid], cid, b)
            elif t == T_P1A:                               # handlePrepare
                self.init(key)
                self.paxi[key].handle_p1a(b)
            elif t == T_P1B:                               # handlePromise
                self.get(key, "Promise").handle_p1b(src, b, [(i32(words[4 * k + 2]), words[4 * k + 3], words[4 * k + 1])
                                                             for k in range(1, len(words) // 4)])
            elif t == T_P2A:                               # handleAccept
                self.init(key)
                self.paxi[key].handle_p2a(b, s, cid)
            elif t == T_P2B:                               # handleAccepted
                self.get(key, "Accepted").handle_p2b(src, b, s)
            elif t == T_P3:                                # handleCommit
                self.init(key)
                self.paxi[key].handle_p3(b, s, cid)
            elif t == T_LEADERCHG and self.proto != abi.KPAXOS:
                self.handle_leader_change(key, b, s)
            else:
                raise AssertionError(f"message type {t} is no message of protocol {self.proto}")
        finally:
            out, self.out = self.out, []
        return out


def replay_cluster(sim, sh, c, msgs, injected=(), delivered_in=()):
    """paxos_model.replay_cluster with per-key replicas.  KPaxos reads key values: Bconfig.Min + index."""
    key_min = sh.wl.key_min

    def make(r, cfg, client, command_of):
        return WReplica(r, cfg, client, command_of, lambda k: key_min + k)

    return pm.replay_cluster(sim, sh, c, msgs, injected, delivered_in, make)


# ---- the shapes shared by tests/test_wpaxos_model.py and tests/test_wpaxos_model_gpu.py ------------
SEED, CLUSTERS = pm.SEED, pm.CLUSTERS


def shape(steps, traced, proto=abi.WPAXOS, npz=(3, 3, 3), keys=8, W=16, M=24, D=0, target=None, locality=700_000,
          slow=True, drop_ppm=0, faults=(), key_min=0, max_requests=0, drains=False, seed=SEED, clusters=CLUSTERS,
          base=0, **cfg_kw):
    """Slow faults (20,000 ppm for 10 steps, delays 1..D) where D > 0 and slow is set; Drop faults
    of 10 steps where drop_ppm is set; one worker per replica unless `target` says otherwise."""
    cfg = abi.make_config(protocol=proto, npz=list(npz), keys=keys, clusters=clusters, cluster_base=base, seed=seed,
                          window=W, mbox_cap=M, max_delay=D, **cfg_kw)
    target = list(range(sum(npz))) if target is None else list(target)
    wl = abi.make_workload(outstanding=len(target), target=target, max_requests=max_requests, locality_ppm=locality,
                           write_ppm=600_000, key_min=key_min)
    fp = None
    if drop_ppm or (slow and D):
        fp = abi.make_fault_process(drop_ppm=drop_ppm, drop_len=10 if drop_ppm else 0, slow_ppm=20000 if slow and D else 0,
                                    slow_len=10 if slow and D else 0, slow_min=1 if slow and D else 0,
                                    slow_max=D if slow and D else 0)
    return pm.Shape(cfg, wl, fp, tuple(faults), steps, drains, dict(traced))


def gap_shape(traced):
    """DESIGN.md §3.5c's single cluster (tests/test_oracle_wpaxos.py::test_reference_gap_p1b_omits_committed_slots)."""
    cfg = abi.make_config(protocol=abi.WPAXOS, npz=[3, 3, 3], keys=8, clusters=1, cluster_base=26, seed=7, window=16,
                          mbox_cap=24, max_delay=3)
    wl = abi.make_workload(outstanding=9, target=list(range(9)), locality_ppm=700_000)
    fp = abi.make_fault_process(drop_ppm=2000, drop_len=20, slow_ppm=2000, slow_len=20, slow_min=1, slow_max=3)
    return pm.Shape(cfg, wl, fp, (), 10, False, dict(traced))


CRASH = (abi.make_fault(abi.FAULT_CRASH, 0, step_from=60, step_to=160),
         abi.make_fault(abi.FAULT_FLAKY, 3, dst=abi.ALL_DST, param=200_000, step_from=0, step_to=300),
         abi.make_fault(abi.FAULT_SLOW, 6, dst=7, param=2, step_from=20, step_to=120))
ZONE3_DOWN = tuple(abi.make_fault(abi.FAULT_CRASH, r) for r in (6, 7, 8))
WG, U = WOVF | GHOST, abi.F_UNFAITHFUL
# traced: {cluster: its flag word}: 0, 63, 64 and 69 wherever they are inside the claim, and the first cluster of
# every other flag word inside it; chosen once on the CPU oracle
SHAPES = {
    # two keys at W = 8 (the co-located instance blocks): every traced cluster's busier key passes slot 168 = 21 * W
    "wrap8": lambda: shape(200, {0: 0, 63: 0, 64: 0, 69: 0, 7: GHOST}, keys=2, W=8, D=2, policy_threshold=3),
    "steal": lambda: shape(200, {0: GHOST, 63: GHOST, 64: GHOST, 69: GHOST, 61: 0}, keys=8, W=16, D=2,
                           policy_threshold=2, locality=500_000),
    "fgrid1": lambda: shape(200, {0: WG, 63: WG, 69: WG, 53: GHOST}, fz=1, D=3, drop_ppm=1000),
    "fgrid2": lambda: shape(200, {0: WG, 63: WG, 64: WG, 69: WG, 13: GHOST}, fz=2, D=3, drop_ppm=1000),
    # duelling proposers: the nil-quorum ACK of paxos.go:290 in clusters 1 and 63
    "nonadaptive": lambda: shape(150, {0: GHOST, 1: POISON | GHOST, 63: POISON | GHOST, 69: GHOST}, adaptive=0, D=2),
    "null": lambda: shape(150, {0: 0, 63: 0, 64: 0, 69: 0, 8: GHOST}, policy_threshold=0, D=2, locality=500_000),
    "majority1": lambda: shape(200, {0: GHOST, 63: WG, 64: GHOST, 69: GHOST}, policy=abi.POLICY_MAJORITY,
                               policy_interval=1, W=32, D=2, drop_ppm=2000),
    "majority25": lambda: shape(200, {0: WG, 63: WG, 64: GHOST, 69: GHOST, 8: 0}, policy=abi.POLICY_MAJORITY,
                                policy_interval=25, W=32, D=2, drop_ppm=2000),
    "ema30": lambda: shape(200, {0: GHOST, 63: GHOST, 64: GHOST, 69: GHOST, 44: 0}, policy=abi.POLICY_EMA,
                           policy_alpha=0.3, D=2),
    "ema85": lambda: shape(200, {0: GHOST, 63: GHOST, 64: GHOST, 69: GHOST}, policy=abi.POLICY_EMA, policy_alpha=0.85,
                           D=2),
    "n4k32": lambda: shape(240, {0: GHOST, 63: 0, 64: GHOST, 69: GHOST}, npz=(2, 2), keys=32, W=8, M=8,
                           target=[0, 1, 2, 3] * 2, locality=800_000),
    "onekey": lambda: shape(200, {0: 0, 63: 0, 64: 0, 69: 0, 2: GHOST}, keys=1, thrifty=1, target=[0, 4, 8, 2],
                            locality=0),
    "crash": lambda: shape(250, {0: 0, 63: WG, 64: WG, 69: GHOST, 42: WOVF}, D=2, slow=False,
                           target=[0, 3, 6, 1, 4, 7], faults=CRASH),
    "kv": lambda: shape(200, {0: WG, 63: WG, 64: WOVF, 69: WG, 7: GHOST, 22: 0}, kv=1, D=2, drop_ppm=1000),
    "gap": lambda: gap_shape({0: GHOST}),
    # zone 3 never answers: GridRow could not form a phase-1 quorum, Majority (5 of 9) does
    "m2": lambda: shape(200, {0: 0, 63: WOVF, 64: WOVF, 69: WOVF, 2: GHOST, 16: WG}, proto=abi.M2PAXOS, D=2,
                        drop_ppm=1000, target=[0, 1, 2, 3, 4, 5], faults=ZONE3_DOWN),
    # key values 192..207: 1.1 leads 192..199, 2.1 leads 200..207
    "kp": lambda: shape(200, {0: WOVF, 63: 0, 64: WOVF, 69: WOVF}, proto=abi.KPAXOS, keys=16, key_min=192, D=2,
                        drop_ppm=1000),
    # one zone, key values 185..200: the leader "2.1" of key 200 is not in the configuration
    "kp_missing": lambda: shape(120, {0: 0, 63: 0, 64: 0, 69: 0}, proto=abi.KPAXOS, npz=(3,), keys=16, key_min=185,
                                target=[0, 1, 2] * 3, D=1, locality=0),
}
# the flag words of all 70 clusters of each shape, measured on the oracle (the table of DESIGN.md §3.5g)
FLAG_COUNTS = {
    "wrap8": {0: 59, GHOST: 11},
    "steal": {0: 1, GHOST: 69},
    "fgrid1": {GHOST: 1, WG: 62, WG | U: 7},
    "fgrid2": {GHOST: 6, WG: 61, WG | U: 3},
    "nonadaptive": {GHOST: 52, GHOST | U: 10, POISON | GHOST: 8},
    "null": {0: 68, GHOST: 2},
    "majority1": {GHOST: 43, WG: 20, GHOST | U: 3, WG | U: 4},
    "majority25": {0: 1, GHOST: 35, WG: 29, WG | U: 5},
    "ema30": {0: 1, GHOST: 69},
    "ema85": {GHOST: 70},
    "n4k32": {0: 9, GHOST: 61},
    "onekey": {0: 55, GHOST: 15},
    "crash": {0: 28, WOVF: 2, GHOST: 25, WG: 15},
    "kv": {0: 1, WOVF: 21, GHOST: 1, WG: 37, WOVF | U: 1, WG | U: 9},
    "gap": {GHOST: 1},
    "m2": {0: 26, WOVF: 24, GHOST: 10, WG: 10},
    "kp": {0: 32, WOVF: 38},
    "kp_missing": {0: 70},
}
EXACT = {"gap": 515}                                       # too short for 500 matched messages per shape: pinned
OUT_OF_WINDOW = ("fgrid1", "fgrid2", "crash", "kv")        # traced clusters end with entries on both sides of a window
MAJORITY = ("majority1", "majority25")


def nil_kpaxos_case():
    """3 x 3, 8 keys, one worker at 1.1 with three requests, no delays: commands 1 and 2 are on
    key 4, command 3 (issued at step 8) on key 7.  A transport hands in four LeaderChanges of
    1.1's: at step 4 to 2.3 for key 4 under a ballot 3.1.1 that is not the instance's (ignored,
    replica.go:104); at step 5 to 2.2 for key 4 under 1.1's ballot (2.2 runs P1a under 2.2.2 and steals the
    key while command 2 is in flight); at step 6 to 2.3 the same message, whose `To` is 2.2
    (ignored); at step 7 to 2.3 one for key 7, of which 2.3 holds no instance yet: Go dereferences
    a nil *kpaxos (replica.go:103-104).  Returns the shape and {step: deliver's arguments}."""
    sh = shape(24, {0: POISON}, keys=8, target=[0], max_requests=3, clusters=1, locality=0)
    b = (1 << 4) | 0
    return sh, {4: (0, 5, 0, [(0, T_LEADERCHG | 4 << 16, (3 << 4) | 0, 5, 0)]),
                5: (0, 4, 0, [(0, T_LEADERCHG | 4 << 16, b, 4, 0)]), 6: (0, 5, 0, [(0, T_LEADERCHG | 4 << 16, b, 4, 0)]),
                7: (0, 5, 0, [(0, T_LEADERCHG | 7 << 16, b, 5, 0)])}


def check_shape(name, sh, res):
    """What keeps a shape's replay from being vacuous, asserted by both suites on `res` =
    {traced cluster: (Replay, flag word)}."""
    cfg, W = sh.cfg, sh.cfg.window
    reps = [m for rp, _ in res.values() for m in rp.replicas]
    ps = [p for m in reps for p in m.paxi.values()]
    delivered = collections.Counter()
    for rp, _ in res.values():
        delivered.update(rp.delivered)
    matched = sum(rp.matched for rp, _ in res.values())
    assert matched == EXACT[name] if name in EXACT else matched > 500, f"{matched} messages matched"
    for c, w in sh.traced.items():
        assert bool(res[c][0].panics) == bool(w & POISON), f"cluster {c}: {res[c][0].panics}"
    if name == "wrap8":
        for c, (rp, _) in res.items():
            assert max(p.slot for m in rp.replicas for p in m.paxi.values()) >= 4 * W, f"cluster {c}"
    if name in OUT_OF_WINDOW:
        assert sum(p.below for p in ps) > 0 and sum(p.above for p in ps) > 0
        assert any(s < p.execute for p in ps for s in p.log) and any(s >= p.execute + W for p in ps for s in p.log)
    if name == "steal":                                    # one forwards table across the keys
        assert delivered[T_LEADERCHG] > 0 and delivered[pm.T_P1B_ENTRY] > 0
        assert any(len({m.command_of(cid)[0] for cid in m.forwards}) > 1 for m in reps)
    if name in ("nonadaptive", "null", "kp", "kp_missing"):
        assert delivered[T_LEADERCHG] == 0
    if name == "nonadaptive":                              # only paxos.forward and HandleP2a / P3 send a Request here
        assert delivered[T_REQUEST] > 0
    if name in MAJORITY:
        assert delivered[T_LEADERCHG] > 0 and sum(p.policy.ties for p in ps) > 0
    if name in ("ema30", "ema85"):
        assert delivered[T_LEADERCHG] > 0 and any(p.policy.s != go_round(p.policy.s) for p in ps)
    if name == "n4k32":
        assert len(reps[0].ids) == 4 and max(len(m.paxi) for m in reps) > 16
    if name == "onekey":
        assert sum(m.thrifty_p2as for m in reps) > 0
    if name == "crash":
        assert sum(m.discarded for m in reps) > 0
    if name == "kv":
        assert sum(m.version for m in reps) > 0 and sum(m.reply_values for m in reps) > 0
    if name == "gap":                                      # 3.3 executes 18 where the others executed 8
        orders = [m.paxi[2].order for m in res[0][0].replicas]
        assert orders[:8] == [[8]] * 8 and orders[8] == [18]
    if name == "m2":                                       # a phase-1 quorum without zone 3
        for c, (rp, _) in res.items():
            assert any(p.active and len(p.quorum) >= 5 and max(p.quorum) < 6 for m in rp.replicas
                       for p in m.paxi.values()), f"cluster {c}"
    if name == "kp":                                       # index(): 1.1 below key value 200, 2.1 from there
        led = {(m.me, k < 200 - sh.wl.key_min) for m in reps for k, p in m.paxi.items() if p.active}
        assert led == {(0, True), (3, False)}
    if name == "kp_missing":                               # forwards to "2.1": sends nobody receives
        for c, (rp, _) in res.items():
            assert sum(len(v) for (src, dst), v in rp.unmatched.items() if dst is None) > 0, f"cluster {c}"
            assert any(cur for cur in rp.client.cur), f"cluster {c}: every request was answered"


BASE = (0, 63, 64, 69)                                     # traced wherever they are inside the claim


def check_traced(sh, sim):
    """A finished run's flag words against the shape's pins: a traced cluster carries its pinned
    word and is inside the claim, and a cluster of BASE is left out only where it is outside."""
    st, N = sim.read_state(), sim.N
    words = [0] * (len(st) // N)
    for i, s in enumerate(st):
        words[i // N] |= s.flags
    for c, w in sh.traced.items():
        assert words[c] == w and not w & pm.OUTSIDE, f"cluster {c}: {words[c]:#x}, pinned {w:#x}"
    for c in BASE:
        if c < len(words):
            assert (c in sh.traced) == (not words[c] & pm.OUTSIDE), f"cluster {c}: {words[c]:#x}, traced {c in sh.traced}"


def check_traced_words():
    """Over all shapes the pinned words include none, WOVF, GHOST, WOVF | GHOST and a POISON one,
    and none is outside the claim (check_traced holds each run to its pins)."""
    words = collections.Counter(w for mk in SHAPES.values() for w in mk().traced.values())
    assert not any(w & pm.OUTSIDE for w in words)
    assert all(words[w] for w in (0, WOVF, GHOST, WG)) and any(w & POISON for w in words)


def check_message_types(results):
    """Over all shapes' replays [{cluster: (Replay, word)}]: every socket message type (a Request
    off the socket is a forwarded one), LeaderChange and P1b payload entries are delivered."""
    seen = collections.Counter()
    for res in results:
        for rp, _ in res.values():
            seen.update(rp.delivered)
    for t in pm.SOCKET_TYPES + (T_LEADERCHG, pm.T_P1B_ENTRY):
        assert seen[t] > 0, f"message type {t}"


def check_nil_kpaxos(rp, word):
    """nil_kpaxos_case's replay: the exact counts, the steal, and the panic at 2.3 in step 7."""
    assert word == POISON and rp.panics == [(7, 5)] and rp.last_step == 7
    assert rp.matched == 72 and sum(rp.delivered[t] for t in pm.SOCKET_TYPES + (T_LEADERCHG,)) == rp.matched + 4
    assert rp.delivered[T_LEADERCHG] == 4 and rp.delivered[pm.T_P1B_ENTRY] == 3
    thief = rp.replicas[4].paxi[4]
    assert (thief.ballot, thief.active) == ((2 << 4) | 4, True)
    assert all(set(m.paxi) == {4} for m in rp.replicas)
