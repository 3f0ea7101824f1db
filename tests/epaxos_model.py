"""A plain EPaxos replica on unbounded maps, and the replay of a message trace through it
(DESIGN.md §3.5e).

The CPU oracle and the HIP kernel share one design: per-owner log rings of W entries, "slots at or
below executed[o] are COMMITTED for good", and the seq of an instance that left the ring cached in
conflicts[o][key].  Bit-exact parity between the two cannot see a flaw of that design.  This model
shares none of it: `Replica` keeps what epaxos/replica.go keeps - dicts that never forget - and
`attributes` reads log[id][d].seq where the reference reads it.  It restates behaviour (handlers
of replica.go, merge of instance.go, FastQuorum / Majority of quorum.go), and it is the reference
without bounds: a cluster with any flag raised is outside its claim.

`replay` drives one model replica per replica of a traced cluster with exactly the messages the
trace says each one received, in the order the simulator handled them, and checks that every
message a replica received is, word for word, one the model's sender emitted earlier.  `check_end`
compares what is left at the end: per-owner slot / executed / committed, the executed-history
digest, Execute and reply counts, and the sends nobody received.

The order of a step's messages is simulator plumbing, not protocol: the sources of
a replica's inbox are interleaved by a seeded pick over the records left, restated in `handled`.
"""
import collections

from paxi_amd import abi, trace

M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
NONE, PREACCEPTED, ACCEPTED, COMMITTED = 0, 1, 2, 3
T_REQUEST, T_PREACCEPT, T_PREACCEPTREPLY, T_ACCEPT, T_ACCEPTREPLY, T_COMMIT = (
    trace.T_REQUEST, trace.T_PREACCEPT, trace.T_PREACCEPTREPLY, trace.T_ACCEPT, trace.T_ACCEPTREPLY,
    trace.T_COMMIT)


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def fmix32(h):
    h = ((h ^ (h >> 16)) * 0x85EBCA6B) & M32
    h = ((h ^ (h >> 13)) * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def i32(u):
    return u - (1 << 32) if u >= 1 << 31 else u


class Instance:
    """epaxos/instance.go; dep holds the positive entries only, as the Go map does."""

    def __init__(self):
        self.cmd, self.ballot, self.status, self.seq, self.dep = 0, 0, NONE, 0, {}
        self.request, self.acks, self.changed, self.replied = None, set(), False, False


class Replica:
    def __init__(self, me, N, key_of, rwc):
        self.me, self.N, self.key_of, self.rwc = me, N, key_of, rwc
        self.log = [dict() for _ in range(N)]
        self.slot, self.committed, self.executed = [-1] * N, [-1] * N, [-1] * N
        self.conflicts = [dict() for _ in range(N)]
        self.max_seq = {}
        self.out = []                    # (dst, words) of the handler that runs now
        self.digest = self.executions = self.replies = self.retries = 0
        self.order = []                  # commands in Execute order
        self.ran = set()                 # (owner, slot) executed at least once

    # ---- messages out: a header (type, w1, w2, w3) and payload words, two's complement
    def send(self, dst, t, w1, w2, w3, pay=()):
        self.out.append((dst, tuple(w & M32 for w in (t, w1, w2, w3) + tuple(pay))))

    def broadcast(self, *a):
        for d in range(self.N):
            if d != self.me:
                self.send(d, *a)

    def deps(self, i):
        return tuple(i.dep.get(k, 0) for k in range(self.N))

    # ---- replica.go
    def attributes(self, cmd):
        key, seq, dep = self.key_of(cmd), 0, {}
        for o in range(self.N):                            # a max over the owners: order-free
            d = self.conflicts[o].get(key)
            if d is not None and d > dep.get(o, 0):
                dep[o] = d
                seq = max(seq, self.log[o][d].seq + 1)
        if key in self.max_seq:
            seq = max(seq, self.max_seq[key] + 1)
        return seq, dep

    def update(self, cmd, o, slot, seq):
        key = self.key_of(cmd)
        if self.conflicts[o].get(key, -1) < slot:
            self.conflicts[o][key] = slot
        if key not in self.max_seq or self.max_seq[key] < seq:
            self.max_seq[key] = seq

    def reply(self, i):
        """Request.Reply: the first call reaches the client, which counts it; with
        reply_when_commit the second is the one the buffered channel holds back."""
        if not i.replied:
            i.replied = True
            self.replies += 1

    def execute(self):
        for o in range(self.N):                            # owners in index order
            for s in range(self.executed[o] + 1, self.slot[o] + 1):
                i = self.log[o].get(s)
                if i is None:
                    continue                               # a gap: skipped, executed[o] stays
                if i.status != COMMITTED:
                    break
                self.digest = mix64(self.digest ^ ((((o << 24) | s) << 32) | i.cmd))
                self.executions += 1
                self.order.append(i.cmd)
                self.ran.add((o, s))
                if i.request is not None:
                    self.reply(i)
                if s == self.executed[o] + 1:
                    self.executed[o] = s

    def update_commit(self, o):
        while True:
            i = self.log[o].get(self.committed[o] + 1)
            if i is None or i.status != COMMITTED:
                break
            self.committed[o] += 1
        self.execute()

    def on_request(self, cmd):
        me = self.me
        self.slot[me] += 1
        s = self.slot[me]
        i = self.log[me][s] = Instance()
        i.seq, i.dep = self.attributes(cmd)
        i.cmd, i.ballot, i.status, i.request, i.acks = cmd, 1 + me, PREACCEPTED, cmd, {me}
        self.update(cmd, me, s, i.seq)
        self.broadcast(T_PREACCEPT, i.ballot, s, cmd, (i.seq,) + self.deps(i))

    def on_preaccept(self, o, ballot, s, cmd, pay):
        i = self.log[o].setdefault(s, Instance())
        if i.status in (COMMITTED, ACCEPTED):
            if not i.cmd:
                i.cmd = cmd
                self.update(cmd, o, s, i32(pay[0]))
            return
        self.slot[o] = max(self.slot[o], s)
        seq, dep = self.attributes(cmd)
        if ballot >= i.ballot:
            i.ballot, i.cmd, i.status, i.seq, i.dep = ballot, cmd, PREACCEPTED, seq, dep
        self.update(cmd, o, s, seq)
        self.send(o, T_PREACCEPTREPLY, i.ballot, s, seq, self.deps(i) + tuple(self.committed))

    def commit_broadcast(self, i, s):
        self.broadcast(T_COMMIT, i.ballot, s, i.cmd, (i.seq,) + self.deps(i))

    def on_preaccept_reply(self, src, ballot, s, seq, pay):
        N, me = self.N, self.me
        i = self.log[me][s]
        if i.status != PREACCEPTED or ballot > i.ballot:
            return
        i.acks.add(src)
        if i32(seq) > i.seq:                               # merge, instance.go
            i.seq, i.changed = i32(seq), True
        for o in range(N):
            if i32(pay[o]) > i.dep.get(o, 0):
                i.dep[o], i.changed = i32(pay[o]), True
        committed = True
        for o in range(N):
            self.committed[o] = max(self.committed[o], i32(pay[N + o]))
            if 0 <= self.committed[o] < i.dep.get(o, 0):
                committed = False
        if len(i.acks) >= N * 3 // 4:                      # FastQuorum
            if not i.changed and committed:
                i.status = COMMITTED
                self.update_commit(me)
                self.commit_broadcast(i, s)
                if self.rwc:
                    self.reply(i)
            else:
                i.status, i.acks = ACCEPTED, {me}
                self.broadcast(T_ACCEPT, i.ballot, s, i.seq, self.deps(i))

    def on_accept(self, o, ballot, s, seq, pay):
        i = self.log[o].setdefault(s, Instance())
        if i.status == COMMITTED:
            return
        self.slot[o] = max(self.slot[o], s)
        if ballot >= i.ballot:
            i.status, i.ballot, i.seq = ACCEPTED, ballot, i32(seq)
            i.dep = {k: i32(pay[k]) for k in range(self.N) if i32(pay[k]) > 0}
        self.send(o, T_ACCEPTREPLY, i.ballot, s, 0)

    def on_accept_reply(self, src, ballot, s):
        i = self.log[self.me][s]
        if i.status != ACCEPTED:
            return
        if i.ballot < ballot:
            i.ballot = ballot
            return
        i.acks.add(src)
        if 2 * len(i.acks) > self.N:                       # Majority
            i.status = COMMITTED
            self.update_commit(self.me)
            if self.rwc:
                self.reply(i)
            self.commit_broadcast(i, s)

    def on_commit(self, o, ballot, s, cmd, pay):
        self.slot[o] = max(self.slot[o], s)
        i = self.log[o].setdefault(s, Instance())
        if ballot >= i.ballot:
            i.ballot, i.cmd, i.status, i.seq = ballot, cmd, COMMITTED, i32(pay[0])
            i.dep = {k: i32(pay[1 + k]) for k in range(self.N) if i32(pay[1 + k]) > 0}
            self.update(cmd, o, s, i.seq)
        if i.request is not None:
            # r.Retry: only the owner's instances hold a request, only the owner sends their
            # Commit (ballots are 1 + owner for good), and nobody sends to itself - unreachable;
            # counted, not re-queued, and the tests assert 0
            self.retries += 1
            i.request = None
        self.update_commit(o)

    def handle(self, src, words):
        t, w1, w2, w3, pay = words[0] & 0xFF, words[1], words[2], words[3], words[4:]
        if t == T_REQUEST:
            self.on_request(w3)
        elif t == T_PREACCEPT:
            self.on_preaccept(src, w1, i32(w2), w3, pay)
        elif t == T_PREACCEPTREPLY:
            self.on_preaccept_reply(src, w1, i32(w2), w3, pay)
        elif t == T_ACCEPT:
            self.on_accept(src, w1, i32(w2), w3, pay)
        elif t == T_ACCEPTREPLY:
            self.on_accept_reply(src, w1, i32(w2))
        elif t == T_COMMIT:
            self.on_commit(src, w1, i32(w2), w3, pay)
        else:
            raise AssertionError(f"message type {t} is no EPaxos message")
        out, self.out = self.out, []
        return out


def payload_words(t, N):
    return {T_REQUEST: 0, T_PREACCEPT: 1 + N, T_PREACCEPTREPLY: 2 * N, T_ACCEPT: N, T_ACCEPTREPLY: 0,
            T_COMMIT: 1 + N}[t]


def words_of(recs, N):
    """One traced message -> (type, w1, w2, w3, payload...), after checking its framing: the
    record count is 1 + ceil(words / 4) and the payload words past the count are 0."""
    hdr = recs[0][1]
    t = hdr & 0xFF
    nw = payload_words(t, N)
    nrec = (nw + 3) // 4
    assert hdr == t | (nrec << 8) and len(recs) == 1 + nrec, f"framing of {recs}"
    flat = [w for r in recs[1:] for w in r[1:]]
    assert not any(flat[nw:]), f"padding of {recs}"
    return (t,) + tuple(recs[0][2:]) + tuple(flat[:nw])


def handled(step_key, r, by_src, NS):
    """The order in which replica r handles a step's inbox (by_src[src]: its messages, FIFO): the
    next source is picked with a 16-bit draw scaled by the records left, two draws per hash."""
    rem = [sum(len(m) for m in by_src.get(s, ())) for s in range(NS)]
    pos, total, i = [0] * NS, sum(rem), 0
    while total:
        u = fmix32(step_key ^ ((1 << 28) | (r << 20) | (i >> 1)))
        pick = (((u >> 16) if i & 1 else (u & 0xFFFF)) * total) >> 16
        src = 0
        while pick >= rem[src]:
            pick -= rem[src]
            src += 1
        m = by_src[src][pos[src]]
        pos[src] += 1
        rem[src] -= len(m)
        total -= len(m)
        i += 1
        yield src, m


Replay = collections.namedtuple("Replay", "replicas unmatched matched delivered last_step")


def replay(msgs, N, seed, gid, key_of, rwc, max_delay=abi.MAX_DELAY, injected=()):
    """One cluster's trace [(step, src, dst, [records])] through N model replicas.  Returns the
    replicas, the model's sends nobody received ({(src, dst): [(step, words)]}), the number of
    matched messages, the deliveries per type and the last step with a delivery.  `injected`:
    (step, src, dst, words) of messages a transport handed in (paxisim_deliver) - inputs, like
    the client's records."""
    kc = mix64(seed ^ mix64((gid + 0x9E3779B97F4A7C15) & M64)) & M32
    reps = [Replica(r, N, key_of, rwc) for r in range(N)]
    sent = collections.defaultdict(list)          # (src, dst) -> [(step, words)] not yet received
    per = collections.defaultdict(lambda: collections.defaultdict(list))
    for (t, src, dst, recs) in msgs:
        per[(t, dst)][src].append(recs)
    matched, delivered, last = 0, collections.Counter(), -1
    for (t, dst) in sorted(per):
        last = t
        step_key = fmix32(kc ^ ((t * 0x9E3779B1) & M32))
        for src, recs in handled(step_key, dst, per[(t, dst)], N + 1):
            words = words_of(recs, N)
            if src == N:
                assert words[0] == T_REQUEST and words[1:3] == (0, 0), f"client record {recs}"
            elif (t, src, dst, words) in injected:
                delivered[words[0]] += 1
            else:
                link = sent[(src, dst)]
                hit = [k for k, (te, w) in enumerate(link) if w == words and te < t]
                assert hit, f"step {t}: {src}->{dst} delivered {words}, which the model's {src} never sent"
                te = link.pop(hit[0])[0]                   # the oldest: a link's equal messages are one multiset
                assert t - te <= 1 + max_delay, f"step {t}: {src}->{dst} {words} sent at step {te}"
                matched += 1
                delivered[words[0]] += 1
            for to, w in reps[dst].handle(src, words):
                sent[(dst, to)].append((t, w))
    return Replay(reps, {k: v for k, v in sent.items() if v}, matched, delivered, last)


def check_end(rp, states, insts, steps, max_delay, drains):
    """The end of a replayed cluster against read_state / read_instances of that cluster (`states`:
    its N records, `insts`: its N * N), and the sends nobody received."""
    N = len(rp.replicas)
    for r, m in enumerate(rp.replicas):
        st = states[r]
        assert st.flags == 0, f"replica {r} is flagged {st.flags:#x}: outside the model's claim"
        assert m.retries == 0
        for o in range(N):
            q = insts[r * N + o]
            assert (q.slot, q.execute - 1, i32(q.p1_acks) - 1) == (m.slot[o], m.executed[o], m.committed[o]), \
                f"replica {r}, owner {o}"
        assert (st.digest, st.executions, st.replies) == (m.digest, m.executions, m.replies), f"replica {r}"
    left = [(te, k, w) for k, v in rp.unmatched.items() for (te, w) in v]
    if drains:
        assert rp.last_step < steps - 1 - max_delay, "the run has not drained"
        assert len(left) == sum(s.dropped for s in states)
    else:
        assert all(s.dropped == 0 for s in states)
        late = [x for x in left if steps - x[0] > 1 + max_delay]
        assert not late, f"sent and never delivered: {late[:3]}"


def reexecutions(rp):
    """Execute calls beyond one per instance: committed instances behind a gap run again."""
    return sum(m.executions - len(m.ran) for m in rp.replicas)


# ---- the shapes shared by the CPU and GPU suites (tests/test_epaxos_model.py, test_epaxos_edges_gpu.py)
SEED, CLUSTERS, TRACED = 11, 70, (0, 63, 64, 69)
Shape = collections.namedtuple("Shape", "cfg wl fp steps drains")


def shape(npz, keys, W, M, D, steps, drop_ppm=0, max_requests=0, **cfg_kw):
    """One worker per replica; Slow faults on every shape, Drop faults (and a finite run that
    drains) where drop_ppm is set."""
    N = sum(npz)
    cfg = abi.make_config(protocol=abi.EPAXOS, npz=list(npz), clusters=CLUSTERS, seed=SEED, keys=keys, window=W,
                          mbox_cap=M, max_delay=D, **cfg_kw)
    wl = abi.make_workload(outstanding=N, target=list(range(N)), max_requests=max_requests)
    fp = abi.make_fault_process(drop_ppm=drop_ppm, drop_len=10 if drop_ppm else 0, slow_ppm=20000, slow_len=10,
                                slow_min=1, slow_max=D)
    return Shape(cfg, wl, fp, steps, bool(drop_ppm))


SHAPES = {
    "wrap5": lambda: shape((5,), 2, 8, 32, 3, 200),
    "wrap3_1key": lambda: shape((3,), 1, 8, 32, 2, 200),
    "wrap10": lambda: shape((10,), 4, 8, 64, 2, 200),      # 200 steps: every own log passes slot 4 * W
    "n4": lambda: shape((2, 2), 2, 16, 32, 2, 100),
    "n2": lambda: shape((2,), 1, 16, 16, 1, 100),
    "drop7": lambda: shape((7,), 2, 64, 64, 3, 150, drop_ppm=3000, max_requests=8),
    "drop10": lambda: shape((3, 3, 4), 4, 64, 64, 3, 150, drop_ppm=3000, max_requests=6),
    "rwc5": lambda: shape((5,), 1, 64, 32, 3, 200, drop_ppm=5000, max_requests=12, reply_when_commit=1),
    "rwc5_kv": lambda: shape((5,), 1, 64, 32, 3, 200, drop_ppm=5000, max_requests=12, reply_when_commit=1, kv=1),
}


def redelivery_case():
    """N = 3 on one key, a worker at A and, from step 16, one at C; before step 12 a transport
    hands C the Commit of A's slot 1 (command 3) a second time, now with seq 9.  Returns the
    shape, the step, deliver's arguments and the message as `replay` sees it."""
    cfg = abi.make_config(protocol=abi.EPAXOS, npz=[3], clusters=1, seed=1, keys=1, window=16, mbox_cap=16,
                          max_delay=0)
    wl = abi.make_workload(outstanding=2, target=[0, 2], start_step=[0, 16], max_requests=3)
    again = [(0, T_COMMIT | (1 << 8), 1, 1, 3), (0, 9, 0, 0, 0)]      # {ballot 1, slot 1, cmd 3} + (seq 9, no deps)
    return Shape(cfg, wl, None, 40, True), 12, (0, 2, 0, again), (12, 0, 2, (T_COMMIT, 1, 1, 3, 9, 0, 0, 0))


def replay_cluster(sim, sh, c, msgs, injected=()):
    """Replay traced cluster c of a finished run of shape `sh` on `sim` (the oracle or the device)
    and check its end.  Returns the Replay."""
    cfg, N = sh.cfg, abi.n_replicas(sh.cfg)
    cids = sorted({m[3][0][4] for m in msgs if (m[3][0][1] & 0xFF) in (T_REQUEST, T_PREACCEPT, T_COMMIT)})
    keys = {cid: min(k, cfg.keys - 1) for cid, (k, _) in zip(cids, sim.commands(c, cids))}
    rp = replay(msgs, N, cfg.seed, cfg.cluster_base + c, keys.__getitem__, bool(cfg.reply_when_commit),
                cfg.max_delay, injected)
    check_end(rp, sim.read_state(c, 1), sim.read_instances(c, 1), sh.steps, cfg.max_delay, sh.drains)
    return rp
