"""A plain ABD replica on unbounded maps, and the check of a replayed cluster's end against it
(DESIGN.md §3.5h).

The CPU oracle and the HIP kernels share one bounded reading of abd/replica.go: Go's
`log map[int]*entry`, which is never cleaned, is a ring of abd_ow(outstanding) entries matched by
tag; versions and values live in per-key planes of 32-bit words; the two quorums are 15-bit masks
packed into one word; the history is capped at `history`.  Parity between the two cannot see a flaw
of that reading.  This model shares none of it: `AbdReplica` keeps what abd/replica.go:28-34 keeps -
`cid`, `log = {cid: entry}` from which nothing is ever removed, `version = {key: int}` on unbounded
ints - and the Database of db.go:103-134 as a dict.  Quorums are sets of replica indices under
`Majority()` of quorum.go:60-62.  History.AddOperation's list (history.go:44-52) is kept uncapped,
in completion order.

The replay is tests/paxos_model.py's (`replay`, `Client`, `crash_windows`, the leftover-sends rule):
every message a replica received must be, word for word, one the model's sender emitted earlier on
that link.  `check_end` compares what is left with read_state, read_kv, history and read_client.

The claim: while neither UNFAITHFUL nor an overflow flag (MBOX_OVF, PEND_OVF) is raised, the op ring
equals the log map, the planes equal the version and value maps, and the history is a prefix of
Go's.  HIST_OVF alone only truncates.

One place where the project knowingly differs from Go: a GetReply or SetReply for a CID the replica
never issued makes Go dereference a nil *entry (replica.go:98-99, 139-140) and panic; the backends
return on the tag mismatch and raise nothing.  `AbdReplica` raises `Panic` there; built with
`nil_entry_panics=False` it returns as the project does and counts the message in `nil_entries`.
"""
import collections

import paxos_model as pm
from paxos_model import T_GET, T_GETREPLY, T_REQUEST, T_SET, T_SETREPLY, M32, Panic, mix64
from paxi_amd import abi

GET_PHASE, SET_PHASE, DONE = 0, 1, 2                       # abd/replica.go:11-15


class Entry:
    """abd/replica.go:17-24; `key` and `write` are m.Command's, `start` the step of handleRequest."""

    def __init__(self, cid, key, write, value, version, start):
        self.cid, self.key, self.write, self.value, self.version, self.start = cid, key, write, value, version, start
        self.state, self.get_quorum, self.set_quorum = GET_PHASE, set(), set()
        self.set_at = None                                 # the step of the Get majority (for the tests)


class AbdReplica:
    """abd/replica.go:50-157, with the Database and the sends of node.go / socket.go."""

    def __init__(self, me, cfg, client, command_of, nil_entry_panics=True):
        self.me, self.N, self.client, self.command_of = me, abi.n_replicas(cfg), client, command_of
        self.nil_entry_panics = nil_entry_panics
        self.cid, self.log, self.version, self.data = 0, {}, {}, {}
        self.history = []                                  # (key, is_write, value, start step, end step)
        self.out = []
        self.sent = self.replies = self.discarded = self.client_requests = self.commits = 0
        self.delivered = collections.Counter()
        # what the tests count (no state of the protocol)
        self.late = 0             # replies for an op no longer in its phase: the `e.state != ...` returns
        self.nil_entries = 0      # replies for a CID never issued (nil_entry_panics unset)
        self.raised_in_get = 0    # a handleSet raised a key's version while an own op on it was in GetPhase
        self.lowered = 0          # line 126 set the local version below what a Set had raised it to

    # ---- socket.go
    def send(self, dst, *words):
        self.sent += 1
        self.out.append((dst, tuple(w & M32 for w in words)))

    def broadcast(self, *words):
        for d in range(self.N):                            # every peer in index order
            if d != self.me:
                self.send(d, *words)

    def majority(self, acks):
        return len(acks) > self.N // 2                     # quorum.go:60-62

    # ---- db.go:116-134
    def get(self, key):
        return self.data.get(key, 0)

    def put(self, key, value):
        if value:                                          # Put writes only a non-nil value
            self.data[key] = value

    # ---- abd/replica.go
    def handle_request(self, cid):                         # 50-71
        k, write = self.command_of(cid)
        v, version = self.get(k), self.version.get(k, 0)
        self.cid += 1
        e = self.log[self.cid] = Entry(cid, k, write, v, version, self.client.step)
        e.get_quorum.add(self.me)
        self.broadcast(T_GET | (k << 8), self.cid, 0, 0)

    def handle_get(self, src, key, cid):                   # 73-82
        self.send(src, T_GETREPLY | (key << 8), cid, self.version.get(key, 0), self.get(key))

    def handle_set(self, src, key, cid, version, value):   # 84-95
        if version > self.version.get(key, 0):
            self.put(key, value)
            self.version[key] = version
            if any(e.state == GET_PHASE and e.key == key for e in self.live()):
                self.raised_in_get += 1
        self.send(src, T_SETREPLY | (key << 8), cid, 0, 0)

    def entry(self, cid):
        e = self.log.get(cid)
        if e is None:
            if self.nil_entry_panics:
                raise Panic(f"replica {self.me}: a reply for CID {cid}, a nil *entry (abd/replica.go:98-99, 139-140)")
            self.nil_entries += 1
        return e

    def handle_get_reply(self, src, key, cid, version, value):   # 97-136
        e = self.entry(cid)
        if e is None:
            return
        if e.state != GET_PHASE:
            self.late += 1
            return
        if version > e.version:
            e.value, e.version = value, version
            self.put(key, value)
            self.version[key] = version
        e.get_quorum.add(src)
        if self.majority(e.get_quorum):
            e.state, e.set_at = SET_PHASE, self.client.step
            e.set_quorum.add(self.me)
            if not e.write:
                self.broadcast(T_SET | (key << 8), cid, e.version, e.value)
            else:
                e.value = e.cid                            # line 122: Command.Value, the command id (0 is nil)
                e.version += 1
                self.put(e.key, e.cid)
                if self.version.get(key, 0) > e.version:
                    self.lowered += 1
                self.version[key] = e.version              # line 126, whatever a Set made of it in between
                self.broadcast(T_SET | (e.key << 8), cid, e.version, e.cid)

    def handle_set_reply(self, src, key, cid):             # 138-157
        e = self.entry(cid)
        if e is None:
            return
        if e.state != SET_PHASE:
            self.late += 1
            return
        e.set_quorum.add(src)
        if self.majority(e.set_quorum):
            e.state = DONE
            self.commits += 1
            # the worker's History.AddOperation (benchmark.go:246-275): a write's input, a read's output
            self.history.append((e.key, int(e.write), e.value, e.start, self.client.step))
            if self.client.reply(e.cid, 0 if e.write else e.value):
                self.replies += 1

    def live(self):
        """The entries in GetPhase or SetPhase, oldest first."""
        return [e for e in self.log.values() if e.state != DONE]

    def handle(self, src, words):
        """One message off the socket (src < N) or the HTTP path (src == N): the sends it causes."""
        t, key, cid, version, value = words[0] & 0xFF, words[0] >> 8, words[1], words[2], words[3]
        try:
            if t == T_REQUEST:
                assert src == self.N, f"replica {self.me}: a Request from replica {src}"
                self.handle_request(value)
            elif t == T_GET:
                self.handle_get(src, key, cid)
            elif t == T_GETREPLY:
                self.handle_get_reply(src, key, cid, version, value)
            elif t == T_SET:
                self.handle_set(src, key, cid, version, value)
            elif t == T_SETREPLY:
                self.handle_set_reply(src, key, cid)
            else:
                raise AssertionError(f"message type {t} is no ABD message")
        finally:
            out, self.out = self.out, []
        return out


def lenient(r, cfg, client, command_of):
    """The replica that returns on a reply for a CID it never issued, as the project does."""
    return AbdReplica(r, cfg, client, command_of, nil_entry_panics=False)


OUTSIDE = abi.F_UNFAITHFUL | abi.F_MBOX_OVF | abi.F_PEND_OVF
HIST_OVF = abi.F_HIST_OVF


def kv_digest(m, keys):
    """read_state's digest of an ABD replica (include/paxisim.h): mix64 chained over the keys'
    (version << 32 | value) in key order."""
    d = 0
    for k in range(keys):
        d = mix64(d ^ ((m.version.get(k, 0) << 32) | m.get(k)))
    return d


def check_end(rp, sim, c, cfg, steps, drains):
    """The end of a replayed ABD cluster c against read_state, read_kv, history and read_client of
    `sim`, and the sends nobody received.  Returns the cluster's flag word."""
    states, H = sim.read_state(c, 1), cfg.history
    word = 0
    for st in states:
        word |= st.flags
    assert not word & OUTSIDE, f"cluster {c} is flagged {word:#x}: outside the model's claim"
    assert not word & ~HIST_OVF and not rp.panics, f"cluster {c}: flag word {word:#x}, panics {rp.panics}"
    hist, at = sim.history(c), 0
    for r, m in enumerate(rp.replicas):
        st, where = states[r], f"cluster {c} replica {r}"
        live = m.live()
        got = (st.slot, st.execute, st.npending, st.digest)
        want = (m.cid, min(len(m.history), H), len(live), kv_digest(m, cfg.keys))
        assert got == want, f"{where}: (slot, execute, npending, digest) {got} against the model's {want}"
        got = (st.commits, st.replies, st.client_requests, st.sent, st.discarded)
        want = (m.commits, m.replies, m.client_requests, m.sent, m.discarded)
        assert got == want, f"{where}: (commits, replies, client_requests, sent, discarded) {got} against {want}"
        assert {t: n for t, n in enumerate(st.delivered) if n} == dict(m.delivered), f"{where}: delivered"
        assert sim.read_kv(c, r, cfg.keys) == [m.get(k) for k in range(cfg.keys)], f"{where}: the Database"
        assert all(k < cfg.keys for k in list(m.data) + list(m.version)), f"{where}: a key beyond the key space"
        mine, at = hist[at:at + st.execute], at + st.execute
        if st.flags & HIST_OVF:
            assert len(m.history) > H and mine == m.history[:H], f"{where}: HIST_OVF, and not the model's first {H} ops"
        else:
            assert mine == m.history, f"{where}: the history against the model's {len(m.history)} ops"
    assert at == len(hist), f"cluster {c}: {len(hist)} ops in the history, {at} by the replicas' counts"
    cl = rp.client
    assert sim.read_client(c) == list(zip(cl.cur, cl.issued, cl.reply_value)), f"cluster {c}: the workers' states"
    pm.check_leftovers(rp, states, c, steps, drains, cfg.max_delay)
    return word


def replay_cluster(sim, sh, c, msgs, injected=(), delivered_in=(), make_replica=AbdReplica):
    """paxos_model.replay_cluster with ABD replicas and ABD's check of the end."""
    return pm.replay_cluster(sim, sh, c, msgs, injected, delivered_in, make_replica, check_end)


def partitions(rp):
    """{key: [(is_write, value, start, end)]} of a replayed cluster's model histories in canonical
    order (replica 0's ops first): what History.Linearizable checks one by one."""
    out = collections.defaultdict(list)
    for m in rp.replicas:
        for (k, w, v, s, e) in m.history:
            out[k].append((w, v, s, e))
    return dict(out)


def abd_ow(outstanding):
    """The op ring's size (include/paxisim.h): the power of two >= 2 * outstanding, 4 at least."""
    ow = 4
    while ow < 2 * outstanding:
        ow *= 2
    return ow


# ---- the shapes shared by tests/test_abd_model.py, test_abd_model_gpu.py and test_checker_model.py --
SEED, CLUSTERS = pm.SEED, pm.CLUSTERS
U, PU, MU = abi.F_UNFAITHFUL, abi.F_PEND_OVF | abi.F_UNFAITHFUL, abi.F_MBOX_OVF | abi.F_UNFAITHFUL
LIN_SMAX = 128                                             # partitions above it take lin_big_kernel


def shape(npz, keys, target, steps, traced, M=16, D=2, drop_ppm=0, history=256, faults=(), slow=True):
    """Half the commands are writes; Slow faults (20,000 ppm for 10 steps, delays 1..D) where D > 0
    and `slow` is set; Drop faults of 10 steps where drop_ppm is set."""
    cfg = abi.make_config(protocol=abi.ABD, npz=list(npz), keys=keys, clusters=CLUSTERS, seed=SEED, mbox_cap=M,
                          max_delay=D, history=history)
    wl = abi.make_workload(outstanding=len(target), target=list(target), write_ppm=500_000)
    slow = bool(slow and D)
    fp = None
    if drop_ppm or slow:
        fp = abi.make_fault_process(drop_ppm=drop_ppm, drop_len=10 if drop_ppm else 0, slow_ppm=20000 if slow else 0,
                                    slow_len=10 if slow else 0, slow_min=1 if slow else 0, slow_max=D if slow else 0)
    return pm.Shape(cfg, wl, fp, tuple(faults), steps, False, dict(traced))


def crash(r, a, b):
    return abi.make_fault(abi.FAULT_CRASH, r, step_from=a, step_to=b)


def flaky(r, ppm, a, b):
    return abi.make_fault(abi.FAULT_FLAKY, r, dst=abi.ALL_DST, param=ppm, step_from=a, step_to=b)


NONE4 = {0: 0, 63: 0, 64: 0, 69: 0}
# traced: {cluster: its flag word}: 0, 63, 64 and 69 wherever they are inside the claim, then the first clusters
# inside it up to four; chosen once on the CPU oracle
SHAPES = {
    "n5": lambda: shape((5,), 4, [0, 1, 2], 200, NONE4, drop_ppm=1000),
    # one key: every op of a cluster falls into one partition, of more than 128 ops
    "n3big": lambda: shape((3,), 1, [0, 1, 2], 300, NONE4, D=1, drop_ppm=1000),
    "n2": lambda: shape((2,), 2, [0, 1], 200, NONE4),
    "zones": lambda: shape((2, 2, 3), 8, list(range(7)), 200, NONE4, M=32, D=3, drop_ppm=2000),
    "crash": lambda: shape((5,), 4, [0, 1, 2, 3], 250, NONE4, drop_ppm=1000, faults=[crash(0, 30, 80), crash(4, 60, 120)]),
    "majority_lost": lambda: shape((5,), 4, list(range(5)), 250, NONE4,
                                   faults=[crash(0, 30, 60), crash(1, 40, 70), crash(2, 50, 80)]),
    "evict": lambda: shape((3,), 2, [0, 0, 1, 2], 300, EVICT_TRACED,
                           faults=[flaky(1, 200_000, 10, 200), flaky(2, 200_000, 10, 200)]),
    "evict2": lambda: shape((2,), 4, [0, 0], 200, EVICT2_TRACED, faults=[flaky(1, 50_000, 0, 0xFFFFFFFF)]),
    "hist8": lambda: shape((5,), 4, [0, 1, 2], 200, {c: HIST_OVF for c in NONE4}, history=8),
    "mbox4": lambda: shape((5,), 2, [0, 0, 0, 0], 200, MBOX4_TRACED, M=4),
    "n1": lambda: shape((1,), 4, [0, 0], 50, NONE4, D=0),
    "keys64": lambda: shape((3,), 64, [0, 1, 2, 0, 1, 2], 200, NONE4),
    "ow16": lambda: shape((5,), 4, [0] * 8, 200, NONE4, history=512),
}
# evict: 63 is outside the claim; evict2: 0, 63 and 69 are; mbox4: cluster 19 is the only one inside
EVICT_TRACED = {0: 0, 3: 0, 8: 0, 64: 0, 69: 0}
EVICT2_TRACED = {3: 0, 4: 0, 9: 0, 64: 0}
MBOX4_TRACED = {19: 0}
# the flag words of all 70 clusters of each shape, measured on the oracle (the table of DESIGN.md §3.5h): the
# clusters outside the claim are not replayed, but a raise that went missing would move them
FLAG_COUNTS = {
    "n5": {0: 70}, "n3big": {0: 70}, "n2": {0: 70}, "zones": {0: 70}, "crash": {0: 70}, "majority_lost": {0: 70},
    "evict": {0: 27, PU: 43}, "evict2": {0: 20, PU: 50}, "hist8": {HIST_OVF: 70}, "mbox4": {0: 1, MU: 69},
    "n1": {0: 70}, "keys64": {0: 70}, "ow16": {0: 70},
}
EXACT = {"n1": 0, "evict2": 128}                           # too short for 500 matched messages: pinned
BIG = ("n3big",)                                           # every traced partition exceeds LIN_SMAX; elsewhere none does


def check_shape(name, sh, res):
    """What keeps a shape's replays {cluster: (Replay, word)} from being vacuous, and its own point."""
    reps = [m for rp, _ in res.values() for m in rp.replicas]
    matched = sum(rp.matched for rp, _ in res.values())
    assert matched == EXACT[name] if name in EXACT else matched > 500, f"{matched} matched messages"
    assert all(sum(m.client_requests for m in rp.replicas) >= sh.wl.outstanding for rp, _ in res.values())
    sizes = [len(p) for rp, _ in res.values() for p in partitions(rp).values()]
    if name in BIG:
        assert min(sizes) > LIN_SMAX and all(len(partitions(rp)) == 1 for rp, _ in res.values()), sizes
    else:
        assert max(sizes, default=0) <= LIN_SMAX, sizes
    if name == "n1":
        # a majority is only tested in handleGetReply (abd/replica.go:110): alone, a replica completes nothing
        assert all(not m.history and len(m.live()) == 2 and not m.delivered for m in reps)
        return
    seen = collections.Counter()
    for rp, _ in res.values():
        seen.update(rp.delivered)
    assert all(seen[t] > 0 for t in pm.ABD_TYPES), f"delivered {dict(seen)}"
    if abi.n_replicas(sh.cfg) > 2:                         # N = 2: a phase ends with the one peer's reply, none comes late
        assert sum(m.late for m in reps) > 0
    else:
        assert sum(m.late for m in reps) == 0
    if name == "majority_lost":
        # the ops that lost their majority to the crashes stay in their phase, and their workers wait for ever
        for c, (rp, _) in res.items():
            stuck = [e for m in rp.replicas for e in m.live() if e.start < 80]
            assert stuck, f"cluster {c}: no op lost its majority"
            assert {GET_PHASE, SET_PHASE} >= {e.state for e in stuck}
            for e in stuck:
                w = (e.cid - 1) % sh.wl.outstanding
                assert rp.client.cur[w] == e.cid, f"cluster {c}: worker {w} went on after request {e.cid}"
        assert any(e.state == SET_PHASE for m in reps for e in m.live() if e.start < 80)
        assert any(e.state == GET_PHASE for m in reps for e in m.live() if e.start < 80)
    if name in ("evict", "evict2"):
        ow = abd_ow(sh.wl.outstanding)
        for c, (rp, _) in res.items():
            stuck = [(m, e) for m in rp.replicas for e in m.live() if e.start < sh.steps - 50]
            assert stuck, f"cluster {c}: no stuck op"
            assert all(m.cid - n < ow for m in rp.replicas for n, e in m.log.items() if e.state != DONE), \
                f"cluster {c}: a live op's ring slot was taken again"
    if name == "hist8":
        assert all(len(m.history) > sh.cfg.history for m in reps if m.history)
        assert sum(len(m.history) for m in reps) > 5 * sh.cfg.history * len(res)


def check_out_of_claim(name, sim):
    """evict and evict2: every cluster outside the claim carries PEND_OVF and UNFAITHFUL together."""
    words = pm.flag_counts(sim) if name in ("evict", "evict2") else {}
    assert all(w == PU for w in words if w & OUTSIDE), {hex(w): n for w, n in words.items()}


def check_raised(results):
    """Over all shapes' replays: a handleSet raised a key's version between a coordinator's request
    and its Get majority (the local version that line 126 then overwrites)."""
    assert sum(m.raised_in_get for res in results for rp, _ in res.values() for m in rp.replicas) > 0


# ---- scenarios handed in with paxisim_deliver: one cluster of N = 3, one worker on replica 0, one key, no
# delays, so op j (CID j, command j) is requested at step 5 (j - 1), reaches its Get majority two steps later
# and its Set majority after four; the ring has abd_ow(1) = 4 entries
def scenario_shape(steps=40):
    sh = shape((3,), 1, [0], steps, {0: 0}, D=0)
    return sh._replace(cfg=abi.make_config(protocol=abi.ABD, npz=[3], keys=1, clusters=1, seed=SEED, mbox_cap=16,
                                           max_delay=0, history=64))


def seen_of(deliveries):
    """replay's `delivered_in` of {step: (cluster, dst, src, [record])}."""
    return {(t, src, dst, tuple(recs[0][1:])) for t, (_, dst, src, recs) in deliveries.items()}


def reused_slot_case():
    """CID 1 is Done and CID 5 holds its ring slot: a GetReply for CID 1 while CID 5 is in GetPhase
    (step 21), with a version that would win, and a SetReply for CID 1 while CID 5 is in SetPhase
    (step 23).  Go finds entry 1, Done, and returns; the ring's tag says 5 and the backends return."""
    return scenario_shape(), {21: (0, 0, 1, [(1, T_GETREPLY, 1, 99, 77)]), 23: (0, 0, 2, [(2, T_SETREPLY, 1, 0, 0)])}


def check_reused_slot(rp, word):
    a = rp.replicas[0]
    assert word == 0 and sum(rp.delivered.values()) == rp.matched + 2
    e = a.log[5]
    assert (a.log[1].state, e.start, e.set_at, e.state) == (DONE, 20, 22, DONE) and a.history[4][4] == 24
    assert a.cid == 8 and all(m.nil_entries == 0 for m in rp.replicas) and max(a.version.values()) < 99


def never_issued_case():
    """A GetReply and a SetReply for CID 41, which replica 0 never issued (steps 11 and 13)."""
    return scenario_shape(), {11: (0, 0, 1, [(1, T_GETREPLY, 41, 99, 77)]), 13: (0, 0, 2, [(2, T_SETREPLY, 41, 0, 0)])}


def lowered_case(sim):
    """The first write j >= 2 of the cluster: while it is in GetPhase, replica 1 hands replica 0 a
    Set of version 9 (step 5 (j - 1) + 1).  The local version is 9 when the Get majority comes, and
    line 126 sets it to the write's e.version, which is lower.  Replica 0 answers the Set with a
    SetReply for CID 41, which replica 1 never issued."""
    j = next(j for j in range(2, 8) if sim.commands(0, [j])[0][1])
    return scenario_shape(), {5 * (j - 1) + 1: (0, 0, 1, [(1, T_SET, 41, 9, 77)])}, j


def check_lowered(rp, word, j):
    a = rp.replicas[0]
    assert word == 0 and (a.lowered, a.raised_in_get, rp.replicas[1].nil_entries) == (1, 1, 1)
    assert a.log[j].version < 9 and a.version[0] < 9


def nil_set_case(sim):
    """A Set of version 9 that carries nil, handed to replica 0 one step before the request of its
    first read j that follows a write (step 5 (j - 1) - 1: no op of its own is under way), when its
    Database holds that write's value: Put leaves the value alone (db.go:123-134), the version goes
    to 9, and read j returns the write's value under version 9.  Inside the protocol a version
    above 0 always travels with the value of the write that made it, so only a transport reaches
    Put's nil case."""
    kinds = [w for _, w in sim.commands(0, list(range(1, 8)))]
    j = next(j for j in range(2, 8) if not kinds[j - 1] and any(kinds[:j - 1]))
    return scenario_shape(), {5 * (j - 1) - 1: (0, 0, 1, [(1, T_SET, 41, 9, 0)])}, j


def check_nil_set(rp, word, j):
    a = rp.replicas[0]
    assert word == 0 and rp.replicas[1].nil_entries == 1 and a.raised_in_get == 0
    key, w, value, start, end = a.history[j - 1]
    assert (w, start) == (0, 5 * (j - 1)) and value != 0 and a.log[j].version == 9
    assert a.get(0) != 0 and a.version[0] >= 9
