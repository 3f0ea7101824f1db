"""A plain Multi-Paxos replica on unbounded maps, and the replay of a message trace through it
(DESIGN.md §3.5f).

The CPU oracle and the HIP kernels share one bounded design: a window of W slots
over [execute, execute + W), a table of eight ghosts that live 2 + 2 * max_delay steps, a forwards
table of 32 entries that retires an entry when its Reply is routed, the `quorum != nil` bit, POISON
for the two Go panics.  Bit-exact parity between the two cannot see a flaw of that design, and
neither can the same code at W = 16 against W = 64.  This model shares none of it: `Paxos` keeps
what paxos/paxos.go keeps - a dict slot -> entry from which only exec deletes and in which nothing
expires, entries re-created below `execute` included - and `Replica` keeps node.go's `forwards`,
which is never cleaned.  Quorums are sets of (zone, node) ids under the predicates of quorum.go.
The two panics (a nil quorum's ACK, paxos.go:290; a nil request's Reply under ReplyWhenCommit,
paxos.go:300-304) raise `Panic`.

`replay` drives one model replica per replica of a traced cluster with exactly the messages the
trace says each one received, in the order the simulator handled them, and checks that every socket
message a replica received is, word for word, one the model's sender emitted earlier on that link.
Crash windows, injected requests and delivered messages are inputs; the client's records are
inputs too, but their timing is checked against the replies the model handed the client.
`check_end` compares what is left: every field of read_state, the window entry by entry against
read_log, the model's entries outside the window against WOVF / GHOST, the panics against POISON,
and the sends nobody received.

The claim: while neither UNFAITHFUL nor an overflow flag (MBOX_OVF, PEND_OVF, BALLOT_OVF) is
raised, the window, the ghost table and the forwards table equal the maps; WOVF and GHOST alone
change nothing; POISON appears exactly where Go panics.

`replay`, `words_of` and `check_end` also serve the per-key protocols (tests/wpaxos_model.py,
DESIGN.md §3.5g): `replay` takes a replica factory, `words_of` accepts the key tag of P1a..P3 and
LeaderChange there, and `check_end` then compares every (replica, key) instance of read_instances
and its window, and read_state's aggregates over them.  ABD (tests/abd_model.py)
uses `replay`, `Client`, `crash_windows` and the leftover-sends rule (`check_leftovers`) with a
check of the end of its own; `words_of` holds its records to ABD's framing.

Simulator plumbing, not protocol, and shared with tests/epaxos_model.py: mix64 / fmix32 and the
merge order of a step's inbox (`handled`).  Record encodings are those of DESIGN.md §3.1-3.2; the
executed-history digest is the chain of include/paxisim.h ("hash chain of executed (slot,
command)"): digest' = mix64(digest ^ (slot << 32 | command)).
"""
import collections

from epaxos_model import M32, M64, fmix32, handled, i32, mix64
from paxi_amd import abi, trace

T_REQUEST, T_REPLY, T_P1A, T_P1B, T_P1B_ENTRY, T_P2A, T_P2B, T_P3 = (
    trace.T_REQUEST, trace.T_REPLY, trace.T_P1A, trace.T_P1B, trace.T_P1B_ENTRY, trace.T_P2A, trace.T_P2B,
    trace.T_P3)
T_LEADERCHG = trace.T_LEADERCHG
SOCKET_TYPES = (T_REQUEST, T_REPLY, T_P1A, T_P1B, T_P2A, T_P2B, T_P3)
# the per-key protocols (tests/wpaxos_model.py): kpaxos.Broadcast / Send tag P1a..P3 with the key
# (hdr bits 16-31); Requests and Replies stay untagged; WPaxos and M2Paxos add LeaderChange
KEYED_TYPES = (T_P1A, T_P1B, T_P2A, T_P2B, T_P3, T_LEADERCHG)
# ABD (tests/abd_model.py): hdr = type | key << 8, one record per message; a Request comes from the client only
T_GET, T_GETREPLY, T_SET, T_SETREPLY = trace.T_GET, trace.T_GETREPLY, trace.T_SET, trace.T_SETREPLY
ABD_TYPES = (T_GET, T_GETREPLY, T_SET, T_SETREPLY)
CLIENT = abi.CLIENT_SRC


class Panic(Exception):
    """A Go panic: the process of this replica dies."""


class Blocked(AssertionError):
    """A third Reply into a request's channel of capacity 1: Go's goroutine would block for good."""


# ---- ids, ballots, quorums (id.go, ballot.go, quorum.go) ------------------------------------------
def ids_of(npz):
    """Replica index -> (zone, node), both 1-based, in IDs.Less order."""
    return [(z + 1, k + 1) for z, n in enumerate(npz) for k in range(n)]


def ballot_id(b):
    """Ballot.ID() of the compressed ballot (n << 4) | r; the zero ballot names nobody ("0.0")."""
    return b & 15 if b else None


def ballot_next(b, r):
    """Ballot.Next(id): n + 1 under id."""
    return (((b >> 4) + 1) << 4) | r


class Quorums:
    """The predicates of quorum.go over a set of acknowledged (zone, node) ids."""

    def __init__(self, npz, fz):
        self.npz, self.fz, self.n, self.z = {z + 1: n for z, n in enumerate(npz)}, fz, sum(npz), len(npz)

    def zones(self, acks):
        return collections.Counter(z for (z, _) in acks)

    def majorities(self, acks):
        return sum(1 for z, n in self.zones(acks).items() if n > self.npz[z] // 2)

    def ok(self, kind, acks):
        if kind == abi.Q_MAJORITY:
            return len(acks) > self.n // 2
        if kind == abi.Q_ALL:
            return len(acks) == self.n
        if kind == abi.Q_FAST:
            return len(acks) >= self.n * 3 // 4
        if kind == abi.Q_GRID_ROW:                         # AllZones
            return len(self.zones(acks)) == self.z
        if kind == abi.Q_ZONE_MAJORITY:
            return self.majorities(acks) > 0
        if kind == abi.Q_GRID_COLUMN:
            return any(n == self.npz[z] for z, n in self.zones(acks).items())
        if kind == abi.Q_FGRID_Q1:
            return self.majorities(acks) >= self.z - self.fz
        if kind == abi.Q_FGRID_Q2:
            return self.majorities(acks) >= self.fz + 1
        raise AssertionError(f"quorum kind {kind}")


# ---- paxi.Request and the log entry ----------------------------------------------------------------
class Chan:
    """A request's reply channel, capacity 1 (http.go:97, node.go:84), and who reads it, once: the
    HTTP handler for the client (http.go:97-104), or the goroutine that sends the Reply back to the
    replica the request came from (node.go:85-87)."""

    def __init__(self, reader):
        self.reader, self.n = reader, 0


class Request:
    """paxi.Request: the command, NodeID (the receiving replica for a client's request, http.go:96;
    the forwarder for a forwarded one, node.go:167) and the reply channel, which the copy made by
    Forward shares (node.go:165-172)."""

    def __init__(self, cid, node_id, chan):
        self.cid, self.node_id, self.chan = cid, node_id, chan

    def word(self):
        """As read_log reports it: cid | origin << 27."""
        return self.cid | self.chan.reader << 27


class Entry:
    """paxos.go:11-18; quorum is a set of replica indices, or None for Go's nil."""

    def __init__(self, ballot=0, command=0, commit=False, request=None, quorum=None):
        self.ballot, self.command, self.commit, self.request, self.quorum = ballot, command, commit, request, quorum


class Paxos:
    """paxos/paxos.go:86-376 over a node that sends, forwards, executes and replies.  It knows
    nothing of the replica-level request path, so a per-key wrapper can hold one per key."""

    def __init__(self, node, q1, q2, thrifty=False, reply_when_commit=False, tag=0):
        self.node, self.q1, self.q2, self.thrifty, self.rwc, self.tag = node, q1, q2, thrifty, reply_when_commit, tag
        self.log, self.slot, self.execute, self.active, self.ballot = {}, -1, 0, False, 0
        self.quorum, self.requests = set(), []
        self.digest = self.commits = 0
        self.order = []                                    # commands in exec order
        self.below = self.above = 0                        # entries ever created below execute / at or above execute + W

    def is_leader(self):
        return self.active or ballot_id(self.ballot) == self.node.me

    def leader(self):
        return ballot_id(self.ballot)

    def put(self, s, e):
        self.log[s] = e
        self.node.created(self, s)

    def handle_request(self, r):
        if not self.active:
            self.requests.append(r)
            if ballot_id(self.ballot) != self.node.me:
                self.p1a()
        else:
            self.p2a(r)

    def p1a(self):
        if self.active:
            return
        self.ballot = ballot_next(self.ballot, self.node.me)
        self.quorum = {self.node.me}
        self.node.broadcast(T_P1A | self.tag, self.ballot, 0, 0)

    def p2a(self, r):
        self.slot += 1
        self.put(self.slot, Entry(self.ballot, r.cid, False, r, {self.node.me}))
        if self.thrifty:
            self.node.multicast_quorum(self.node.N // 2 + 1, T_P2A | self.tag, self.ballot, self.slot, r.cid)
        else:
            self.node.broadcast(T_P2A | self.tag, self.ballot, self.slot, r.cid)

    def forward(self):
        for r in self.requests:
            self.node.forward(ballot_id(self.ballot), r)
        self.requests = []

    def handle_p1a(self, ballot):
        if ballot > self.ballot:
            self.ballot, self.active = ballot, False
            self.forward()
        log = []
        for s in range(self.execute, self.slot + 1):
            e = self.log.get(s)
            if e is not None and not e.commit:
                log.append((s, e.command, e.ballot))
        self.node.send_p1b(ballot_id(ballot), self.tag, self.ballot, log)

    def update(self, log):
        for (s, command, ballot) in log:
            self.slot = max(self.slot, s)
            e = self.log.get(s)
            if e is not None:
                if not e.commit and ballot > e.ballot:
                    e.ballot, e.command = ballot, command
            else:
                self.put(s, Entry(ballot, command))

    def handle_p1b(self, src, ballot, log):
        if ballot < self.ballot or self.active:
            return
        self.update(log)
        if ballot > self.ballot:
            self.ballot, self.active = ballot, False
            self.forward()
        if ballot_id(ballot) == self.node.me and ballot == self.ballot:
            self.quorum.add(src)
            if self.node.quorum_ok(self.q1, self.quorum):
                self.active = True
                for s in range(self.execute, self.slot + 1):
                    e = self.log.get(s)
                    if e is None or e.commit:
                        continue
                    e.ballot, e.quorum = self.ballot, {self.node.me}
                    self.node.broadcast(T_P2A | self.tag, self.ballot, s, e.command)
                for r in self.requests:
                    self.p2a(r)
                self.requests = []

    def handle_p2a(self, ballot, s, command):
        if ballot >= self.ballot:
            self.ballot, self.active = ballot, False
            self.slot = max(self.slot, s)
            e = self.log.get(s)
            if e is not None:
                if not e.commit and ballot > e.ballot:
                    if e.command != command and e.request is not None:
                        self.node.forward(ballot_id(ballot), e.request)
                        e.request = None
                    e.command, e.ballot = command, ballot
            else:
                self.put(s, Entry(ballot, command))
        self.node.send(ballot_id(ballot), T_P2B | self.tag, self.ballot, s, 0)

    def handle_p2b(self, src, ballot, s):
        e = self.log.get(s)
        if e is None or ballot < e.ballot or e.commit:
            return
        if ballot > self.ballot:
            self.ballot, self.active = ballot, False
        if ballot_id(ballot) == self.node.me and ballot == e.ballot:
            if e.quorum is None:
                raise Panic(f"slot {s}: ACK on a nil quorum (paxos.go:290)")
            e.quorum.add(src)
            if self.node.quorum_ok(self.q2, e.quorum):
                e.commit = True
                self.commits += 1
                self.node.broadcast(T_P3 | self.tag, ballot, s, e.command)
                if self.rwc:
                    if e.request is None:
                        raise Panic(f"slot {s}: Reply on a nil request (paxos.go:300-304)")
                    self.node.reply(e.request, e.request.cid, 0)
                else:
                    self.exec()

    def handle_p3(self, ballot, s, command):
        self.slot = max(self.slot, s)
        e = self.log.get(s)
        if e is not None:
            if e.command != command and e.request is not None:
                self.node.forward(ballot_id(ballot), e.request)
                e.request = None
        else:
            e = Entry()
            self.put(s, e)
        e.command, e.commit = command, True
        if self.rwc:
            if e.request is not None:
                self.node.reply(e.request, e.request.cid, 0)
        else:
            self.exec()

    def exec(self):
        while True:
            e = self.log.get(self.execute)
            if e is None or not e.commit:
                break
            value = self.node.execute(e.command)
            self.digest = mix64(self.digest ^ ((self.execute << 32) | e.command))
            self.order.append(e.command)
            if e.request is not None:
                self.node.reply(e.request, e.command, value)
                e.request = None
            del self.log[self.execute]
            self.execute += 1


class Replica:
    """paxos/replica.go and what it uses of node.go and socket.go: the request path, Forward and
    the Reply's way back along `forwards`, the Database (db.go:103-134) and the sends."""

    def __init__(self, me, cfg, client, command_of):
        npz = [cfg.npz[z] for z in range(cfg.n_zones)]
        self.me, self.N, self.ids, self.quorums = me, sum(npz), ids_of(npz), Quorums(npz, cfg.fz)
        self.W, self.kv, self.ephemeral = cfg.window, bool(cfg.kv), bool(cfg.ephemeral_leader)
        self.client, self.command_of = client, command_of
        self.paxos = self.new_paxos(cfg)
        self.forwards = {}                                 # never cleaned (node.go:83-97, 165-172)
        self.data, self.version = {}, 0
        self.out = []
        self.sent = self.replies = self.discarded = self.client_requests = 0
        self.delivered = collections.Counter()

    def new_paxos(self, cfg):
        """The replica's single paxos.Paxos (paxos/replica.go:26); a per-key replica has none."""
        return Paxos(self, cfg.q1, cfg.q2, bool(cfg.thrifty), bool(cfg.reply_when_commit))

    def instances(self):
        """{key: Paxos} of the instances this replica holds."""
        return {0: self.paxos}

    # ---- socket.go
    def send(self, dst, *words):
        self.sent += 1
        self.out.append((dst, tuple(w & M32 for w in words)))

    def broadcast(self, *words):
        for d in range(self.N):                            # every peer in index order
            if d != self.me:
                self.send(d, *words)

    def multicast_quorum(self, q, *words):
        for i in range(1, min(q, self.N - 1) + 1):         # the q peers after self in ring order
            self.send((self.me + i) % self.N, *words)

    def send_p1b(self, dst, tag, ballot, log):
        pay = [w for (s, command, b) in log for w in (T_P1B_ENTRY, b, s, command)]
        self.send(dst, T_P1B | (len(log) << 8) | tag, ballot, 0, 0, *pay)

    def quorum_ok(self, kind, acks):
        return self.quorums.ok(kind, {self.ids[r] for r in acks})

    def created(self, p, s):
        if s < p.execute:
            p.below += 1
        elif s >= p.execute + self.W:
            p.above += 1

    # ---- node.go
    def forward(self, to, r):
        m = Request(r.cid, self.me, r.chan)
        self.forwards[m.cid] = m
        self.send(to, T_REQUEST, 0, 0, m.cid)

    def reply(self, r, command, value):
        """Request.Reply(Reply{Command, Value}) (message.go:32-34)."""
        r.chan.n += 1
        if r.chan.n > 2:
            raise Blocked(f"replica {self.me}: a third Reply to request {r.cid}")
        if r.chan.n == 2:                                  # stays in the buffer: nobody reads twice
            return
        if r.chan.reader == CLIENT:
            if self.client.reply(r.cid, value):
                self.replies += 1
        else:
            self.send(r.chan.reader, T_REPLY, value, 0, command)

    def execute(self, command):
        """database.Execute: the key's previous value; a write puts its own (its command id)."""
        if not self.kv:
            return 0
        key, write = self.command_of(command)
        v = self.data.get(key, 0)
        if write:
            self.data[key] = command
            self.version += 1
        return v

    # ---- paxos/replica.go:42-66, with -read unset
    def handle_request(self, r):
        p = self.paxos
        if self.ephemeral or p.is_leader() or p.ballot == 0:
            p.handle_request(r)
        else:
            self.forward(p.leader(), r)

    def handle(self, src, words):
        """One message off the socket (src < N) or the HTTP path (src == N): the sends it causes."""
        t, b, s, cid = words[0] & 0xFF, words[1], i32(words[2]), words[3]
        p = self.paxos
        try:
            if t == T_REQUEST:
                http = src == self.N
                self.handle_request(Request(cid, self.me if http else src, Chan(CLIENT if http else src)))
            elif t == T_REPLY:
                assert cid in self.forwards, f"replica {self.me}: Reply for {cid}, which it never forwarded"
                self.reply(self.forwards[cid], cid, b)
            elif t == T_P1A:
                p.handle_p1a(b)
            elif t == T_P1B:
                p.handle_p1b(src, b, [(i32(words[4 * k + 2]), words[4 * k + 3], words[4 * k + 1])
                                      for k in range(1, len(words) // 4)])
            elif t == T_P2A:
                p.handle_p2a(b, s, cid)
            elif t == T_P2B:
                p.handle_p2b(src, b, s)
            elif t == T_P3:
                p.handle_p3(b, s, cid)
            else:
                raise AssertionError(f"message type {t} is no Multi-Paxos message")
        finally:
            out, self.out = self.out, []
        return out


class Client:
    """The closed-loop workers of one cluster: worker w's first request 1 + w
    waits at its target at start_step[w]; a reply to its current request at step t puts the next,
    1 + w + outstanding * j, into its target's inbox of step t + 1.  Other replies are ignored."""

    def __init__(self, wl):
        self.wl, self.WK = wl, wl.outstanding
        self.cur = [1 + w for w in range(self.WK)]
        self.issued = [1] * self.WK
        self.due = {(wl.start_step[w], wl.target[w], 1 + w) for w in range(self.WK)}
        self.reply_value = [0] * self.WK                   # Reply.Value of the worker's last answered request
        self.step = 0

    def reply(self, cid, value):
        w = (cid - 1) % self.WK
        if self.cur[w] != cid:
            return False
        self.reply_value[w] = value
        if self.wl.max_requests == 0 or self.issued[w] < self.wl.max_requests:
            self.cur[w] = 1 + w + self.WK * self.issued[w]
            self.issued[w] += 1
            self.due.add((self.step + 1, self.wl.target[w], self.cur[w]))
        else:
            self.cur[w] = 0
        return True

    def arrives(self, t, dst, cid):
        """A client record of the trace: the model's client must have sent exactly it for step t."""
        assert (t, dst, cid) in self.due, \
            f"step {t}: request {cid} at replica {dst}; the model's client has {sorted(self.due)}"
        self.due.remove((t, dst, cid))


def words_of(recs, keys=0, abd=False):
    """One traced message -> its words, after checking its framing: only a P1b carries payload
    records, as many as its header says, each a P1B_ENTRY.  Multi-Paxos (keys = 0) has no key tag
    and no LeaderChange; of a per-key protocol's messages P1a..P3 and LeaderChange carry a key
    below `keys`, Requests and Replies none.  ABD: hdr = type | key << 8 with the key below `keys`,
    one record per message, no payload; its only other record is the client's Request."""
    hdr = recs[0][1]
    if abd:
        assert hdr == T_REQUEST or (hdr & 0xFF in ABD_TYPES and hdr >> 8 < keys), f"header of {recs}"
        assert len(recs) == 1, f"framing of {recs}"
        return tuple(recs[0][1:])
    t, n = hdr & 0xFF, (hdr >> 8) & 0xFF
    if keys and t in KEYED_TYPES:
        assert hdr >> 16 < keys, f"key tag of {recs}"
    else:
        assert hdr >> 16 == 0 and t in SOCKET_TYPES, f"header of {recs}"
    assert (n == 0 or t == T_P1B) and len(recs) == 1 + n, f"framing of {recs}"
    assert all(r[1] == T_P1B_ENTRY for r in recs[1:]), f"payload of {recs}"
    return tuple(w for r in recs for w in r[1:])


def crash_windows(faults, gid):
    """[(replica, from, to)] of the scripted Crash faults that cover cluster gid."""
    return [(f.src, f.step_from, f.step_to) for f in faults
            if f.kind == abi.FAULT_CRASH and f.cluster_lo <= gid < f.cluster_hi]


Replay = collections.namedtuple("Replay", "replicas unmatched matched delivered last_step panics client")


def replay(msgs, cfg, wl, gid, command_of, crashes=(), injected=(), delivered_in=(), make_replica=Replica):
    """One cluster's trace [(step, src, dst, [records])] through its model replicas.  Returns the
    replicas, the model's sends nobody received ({(src, dst): [(step, words)]}), the number of
    matched messages, the deliveries per type (P1B_ENTRY: payload entries), the last step with a
    record, the panics [(step, replica)] and the client.
    Inputs besides the trace: `crashes` [(replica, from, to)]; `injected` {(step, dst, cid)} of
    paxisim_inject; `delivered_in` {(step, src, dst, words)} of paxisim_deliver.  `make_replica`
    (index, cfg, client, command_of) builds one model replica: `Replica`, or a per-key one."""
    N, D = abi.n_replicas(cfg), cfg.max_delay
    abd = cfg.protocol == abi.ABD
    keys = cfg.keys if abd or cfg.protocol in abi.PER_KEY else 0
    kc = mix64(cfg.seed ^ mix64((gid + 0x9E3779B97F4A7C15) & M64)) & M32
    client = Client(wl)
    reps = [make_replica(r, cfg, client, command_of) for r in range(N)]
    sent = collections.defaultdict(list)          # (src, dst) -> [(step, words)] not yet received
    per = collections.defaultdict(lambda: collections.defaultdict(list))
    for (t, src, dst, recs) in msgs:
        per[(t, dst)][src].append(recs)
    matched, delivered, last, panics = 0, collections.Counter(), -1, []

    def match(t, src, dst, words):
        if (t, src, dst, words) in delivered_in:
            return 0
        link = sent[(src, dst)]
        hit = [k for k, (te, w) in enumerate(link) if w == words and te < t]
        assert hit, f"step {t}: {src}->{dst} delivered {words}, which the model's {src} never sent"
        # a link's equal messages are one multiset: the oldest that can still be on its way.  An older
        # equal one (a LeaderChange repeats under an unchanged ballot) was lost and stays a leftover,
        # which check_end holds against `dropped`.
        young = [k for k in hit if t - link[k][0] <= 1 + D]
        assert young, f"step {t}: {src}->{dst} {words} sent at step {link[hit[-1]][0]}"
        link.pop(young[0])
        return 1

    for (t, dst) in sorted(per):
        assert not panics or t == panics[0][0], f"step {t}: the trace goes on after the panic {panics[0]}"
        last, client.step = t, t
        by_src, me = per[(t, dst)], reps[dst]
        if any(r == dst and a <= t < b for (r, a, b) in crashes):        # socket.Recv discards (socket.go:111-118)
            for src in [s for s in by_src if s < N]:
                for recs in by_src.pop(src):
                    matched += match(t, src, dst, words_of(recs, keys, abd))
                    me.discarded += 1
        step_key = fmix32(kc ^ ((t * 0x9E3779B1) & M32))
        dead = False
        for src, recs in handled(step_key, dst, by_src, N + 1):
            words = words_of(recs, keys, abd)
            if src == N:
                assert words[0] == T_REQUEST and words[1:3] == (0, 0), f"client record {recs}"
                if (t, dst, words[3]) not in injected:
                    client.arrives(t, dst, words[3])
            else:
                matched += match(t, src, dst, words)
            if dead:                                       # the process died earlier in this step
                continue
            if src == N:
                me.client_requests += 1
            else:
                me.delivered[words[0] & 0xFF] += 1
                delivered[words[0] & 0xFF] += 1
                delivered[T_P1B_ENTRY] += len(words) // 4 - 1
            try:
                for to, w in me.handle(src, words):
                    sent[(dst, to)].append((t, w))
            except Panic:
                panics.append((t, dst))
                dead = True
    return Replay(reps, {k: v for k, v in sent.items() if v}, matched, delivered, last, panics, client)


def ballot64(ids, b):
    """The compressed ballot as read_state reports it: n << 32 | zone << 16 | node (ballot.go:15-17)."""
    if b == 0:
        return 0
    z, n = ids[b & 15]
    return ((b >> 4) << 32) | (z << 16) | n


OUTSIDE = abi.F_UNFAITHFUL | abi.F_MBOX_OVF | abi.F_PEND_OVF | abi.F_BALLOT_OVF


def check_instance(sim, c, r, m, p, st, W, key=0):
    """One paxos.Paxos `p` of model replica `m` against an instance record or a Multi-Paxos
    replica state `st`, and its window against read_log."""
    where = f"cluster {c} replica {r} key {key}"
    got = (st.ballot, st.slot, st.execute, st.active, st.npending, bin(st.p1_acks).count("1"), st.digest)
    want = (ballot64(m.ids, p.ballot), p.slot, p.execute, int(p.active), len(p.requests), len(p.quorum), p.digest)
    assert got == want, f"{where}: (ballot, slot, execute, active, npending, |p1 quorum|, digest) {got} against {want}"
    assert {k for k in range(m.N) if st.p1_acks >> k & 1} == p.quorum, f"{where}: phase-1 quorum"
    for le in sim.read_log(c, r, p.execute, W, key=key):
        e = p.log.get(le.slot)
        assert le.flags & abi.LOG_HELD
        if e is None:
            assert not le.flags & abi.LOG_EXISTS, f"{where} slot {le.slot}: the model holds no entry"
            continue
        bits = abi.LOG_HELD | abi.LOG_EXISTS | (abi.LOG_COMMIT if e.commit else 0) | \
            (abi.LOG_QUORUM if e.quorum is not None else 0) | (abi.LOG_REQUEST if e.request is not None else 0)
        want = (ballot64(m.ids, e.ballot), e.command, bits, sum(1 << k for k in e.quorum or ()),
                e.request.word() if e.request is not None else 0)
        assert (le.ballot, le.cmd, le.flags, le.acks, le.request) == want, f"{where} slot {le.slot}"


def check_keyed(sim, c, r, m, st, ins, cfg):
    """A per-key replica: every (replica, key) record of read_instances against the instance map
    and the policies, then read_state's aggregates over the instances as include/paxisim.h defines
    them (ballot: the highest; slot: keys led, Replica.keys; execute, active, npending: sums;
    p1_acks: the mask of existing instances; digest: mix64 chained over the key digests in key
    order, 0 for a key without instance)."""
    paxi, digest = m.instances(), 0
    for k in range(cfg.keys):
        i, p = ins[k], paxi.get(k)
        assert i.exists == (p is not None), f"cluster {c} replica {r} key {k}: exists = {i.exists}"
        if p is None:                                      # never initialised: nothing but the empty record
            got = (i.ballot, i.slot, i.execute, i.active, i.p1_acks, i.npending, i.digest, tuple(i.policy_state))
            assert got == (0, -1, 0, 0, 0, 0, 0, (0, 0, 0, 0)), f"cluster {c} replica {r} key {k}: {got}"
            digest = mix64(digest)
            continue
        check_instance(sim, c, r, m, p, i, cfg.window, k)
        for name, want in p.policy.expect().items():
            got = getattr(i, name)
            got = tuple(got[:len(want)]) if name == "policy_state" else got
            assert got == want, f"cluster {c} replica {r} key {k}: {name} {got} against the model's {want}"
        digest = mix64(digest ^ p.digest)
    ps = list(paxi.values())
    got = (st.ballot, st.slot, st.execute, st.active, st.p1_acks, st.npending, st.digest)
    want = (ballot64(m.ids, max((p.ballot for p in ps), default=0)), sum(1 for p in ps if p.is_leader()),
            sum(p.execute for p in ps), sum(p.active for p in ps), sum(1 << k for k in paxi),
            sum(len(p.requests) for p in ps), digest)
    assert got == want, f"cluster {c} replica {r}: (highest ballot, keys led, executed, active, exists mask, " \
                        f"pending, digest chain) {got} against the model's {want}"


def check_leftovers(rp, states, c, steps, drains, D):
    """The sends nobody received against `dropped`, and the client's requests against the trace."""
    left = [(te, k, w) for k, v in rp.unmatched.items() for (te, w) in v]
    if rp.panics:
        # the cluster is frozen after the panic's step: the leftovers are held against `dropped` as
        # those of a run of that many steps that does not drain
        assert rp.last_step <= rp.panics[0][0]
        steps, drains = rp.panics[0][0] + 1, False
    else:
        due = [d for d in rp.client.due if d[0] < steps]
        assert not due, f"cluster {c}: requests the model's client sent and the trace lacks: {sorted(due)[:3]}"
    dropped = sum(s.dropped for s in states)
    if drains:
        assert rp.last_step < steps - 1 - D, "the run has not drained"
        assert len(left) == dropped, f"cluster {c}: {len(left)} sends nobody received, {dropped} dropped"
    else:
        # a leftover is a dropped send or still on its way: none dropped, none old; and never more
        # old ones than were dropped, nor more dropped than are left
        late = [x for x in left if steps - x[0] > 1 + D]
        assert len(late) <= dropped <= len(left), f"cluster {c}: {dropped} dropped, never delivered: {late[:3]}"


def check_end(rp, sim, c, cfg, steps, drains):
    """The end of a replayed cluster c against read_state / read_log (a per-key protocol: and
    read_instances) of `sim`, and the sends nobody received.  Returns the cluster's flag word."""
    N, W, D = len(rp.replicas), cfg.window, cfg.max_delay
    keyed = cfg.protocol in abi.PER_KEY
    states = sim.read_state(c, 1)
    ins = sim.read_instances(c, 1) if keyed else None
    word = 0
    for st in states:
        word |= st.flags
    assert not word & OUTSIDE, f"cluster {c} is flagged {word:#x}: outside the model's claim"
    dead = {r for (_, r) in rp.panics}
    for r, m in enumerate(rp.replicas):
        st, ps = states[r], list(m.instances().values())
        assert bool(st.flags & abi.F_POISON) == (r in dead), f"cluster {c} replica {r}: POISON against {rp.panics}"
        if keyed:
            check_keyed(sim, c, r, m, st, ins[r * cfg.keys:(r + 1) * cfg.keys], cfg)
        else:
            check_instance(sim, c, r, m, m.paxos, st, W)
        got = (st.commits, st.replies, st.executions, st.executed_writes, st.client_requests, st.sent, st.discarded)
        want = (sum(p.commits for p in ps), m.replies, sum(p.execute for p in ps), m.version, m.client_requests, m.sent,
                m.discarded)
        assert got == want, f"cluster {c} replica {r}: (commits, replies, executions, executed_writes, " \
                            f"client_requests, sent, discarded) {got} against the model's {want}"
        assert {t: n for t, n in enumerate(st.delivered) if n} == dict(m.delivered), f"cluster {c} replica {r}: delivered"
        if any(s >= p.execute + W for p in ps for s in p.log):
            assert st.flags & abi.F_WOVF, f"cluster {c} replica {r}: an entry beyond the window, and no WOVF"
        if any(s < p.execute for p in ps for s in p.log):
            assert st.flags & abi.F_GHOST, f"cluster {c} replica {r}: an entry below execute, and no GHOST"
    check_leftovers(rp, states, c, steps, drains, D)
    return word


def replay_cluster(sim, sh, c, msgs, injected=(), delivered_in=(), make_replica=Replica, check=None):
    """Replay traced cluster c of a finished run of shape `sh` on `sim` (the oracle or the device)
    and check its end (`check`: check_end, or a protocol's own with its arguments).  Returns the
    Replay and the cluster's flag word."""
    cfg = sh.cfg
    memo = {}

    def command_of(cid):
        if cid not in memo:
            key, write = sim.commands(c, [cid])[0]
            memo[cid] = (min(key, cfg.keys - 1), write)
        return memo[cid]

    rp = replay(msgs, cfg, sh.wl, cfg.cluster_base + c, command_of, crash_windows(sh.faults, cfg.cluster_base + c),
                injected, delivered_in, make_replica)
    return rp, (check or check_end)(rp, sim, c, cfg, sh.steps, sh.drains)


# ---- the shapes shared by the CPU and GPU suites (tests/test_paxos_model.py, test_paxos_model_gpu.py)
SEED, CLUSTERS = 11, 70
WOVF, GHOST, POISON = abi.F_WOVF, abi.F_GHOST, abi.F_POISON
# traced: {cluster: the flag word expected of it}, chosen once on the CPU oracle
Shape = collections.namedtuple("Shape", "cfg wl fp faults steps drains traced")


def shape(npz, W, M, D, target, steps, traced, drop_ppm=0, drains=False, max_requests=0, start_step=0, faults=(),
          slow=True, **cfg_kw):
    """Slow faults on every shape (slow = False: none), Drop faults where drop_ppm is set."""
    cfg = abi.make_config(npz=list(npz), clusters=CLUSTERS, seed=SEED, window=W, mbox_cap=M, max_delay=D, **cfg_kw)
    wl = abi.make_workload(outstanding=len(target), target=list(target), max_requests=max_requests,
                           start_step=start_step, write_ppm=600_000, keys=8)
    fp = abi.make_fault_process(drop_ppm=drop_ppm, drop_len=10 if drop_ppm else 0, slow_ppm=20000, slow_len=10,
                                slow_min=1, slow_max=D) if slow and D else None
    return Shape(cfg, wl, fp, tuple(faults), steps, drains, dict(traced))


def crash_shape(traced):
    """The crash-and-return shape of tests/trace_ref.py (replica 0 crashed over [30, 80), a late
    worker, the Database on) at 200 steps."""
    import trace_ref
    cfg, wl, fp, faults = trace_ref.crash_case(CLUSTERS)
    return Shape(cfg, wl, fp, tuple(faults), 200, False, dict(traced))


def failover_shape(traced):
    """test_parity_gpu.py::test_late_workers_crash_failover's 3 x 3 at seed 11, with Drop faults:
    the clients turn from the crashed 1.1 to 2.1 at step 90."""
    sh = shape((3, 3, 3), 16, 24, 0, [0, 0, 0, 0, 3, 3, 3, 3], 240, traced, start_step=[0, 0, 0, 0, 90, 90, 90, 90],
               ephemeral_leader=1, faults=[abi.make_fault(abi.FAULT_CRASH, 0, step_from=90)], **FGRID)
    return sh._replace(fp=abi.make_fault_process(drop_ppm=1000, drop_len=10))


FGRID = dict(q1=abi.Q_FGRID_Q1, q2=abi.Q_FGRID_Q2, fz=1)
FLAKY = (abi.make_fault(abi.FAULT_FLAKY, 1, dst=abi.ALL_DST, param=100000, step_from=10, step_to=200),
         abi.make_fault(abi.FAULT_SLOW, 2, dst=abi.ALL_DST, param=3, step_from=0, step_to=300))
SHAPES = {
    # three workers at W = 8: the pipeline stays shorter than the window, the leader passes slot 34 * W
    "wrap": lambda: shape((5,), 8, 32, 3, [0, 0, 0], 300,
                          {0: GHOST, 7: WOVF, 30: WOVF | GHOST, 63: WOVF | GHOST, 64: WOVF | GHOST, 69: GHOST},
                          drop_ppm=1000),
    "wrap9": lambda: shape((3, 3, 3), 8, 32, 2, [0, 0, 4], 300, {0: WOVF, 1: 0, 63: WOVF, 64: WOVF, 69: WOVF},
                           drop_ppm=1000, **FGRID),
    "forwarding": lambda: shape((5,), 16, 32, 3, [0, 1, 2, 3, 4, 2], 200,
                                {0: WOVF | GHOST, 3: GHOST, 13: 0, 63: WOVF | GHOST, 64: WOVF | GHOST, 69: WOVF},
                                drop_ppm=3000),
    "thrifty": lambda: shape((5,), 16, 32, 3, [0] * 5, 200, {0: GHOST, 63: GHOST, 64: 0, 69: GHOST}, thrifty=1),
    "n3": lambda: shape((3,), 8, 32, 1, [0] * 3, 200, {0: 0, 63: WOVF, 64: 0, 69: 0}, drop_ppm=1000),
    "n2": lambda: shape((2,), 16, 32, 2, [0, 1], 200, {0: 0, 63: 0, 64: 0, 69: 0}),
    "ephemeral": lambda: shape((5,), 16, 32, 3, [0, 1, 2, 3, 4], 250,
                               {0: GHOST, 34: POISON | GHOST, 47: POISON | GHOST, 63: GHOST, 64: GHOST},
                               drop_ppm=3000, drains=True, max_requests=6, ephemeral_leader=1),
    "flaky": lambda: shape((5,), 16, 24, 3, [0, 1, 2], 200,
                           {2: POISON | GHOST, 5: POISON | GHOST, 6: POISON | GHOST, 33: GHOST, 64: WOVF | GHOST},
                           slow=False, ephemeral_leader=1, faults=FLAKY),
    "crash": lambda: crash_shape({0: WOVF | GHOST, 11: GHOST, 64: WOVF | GHOST, 69: WOVF | GHOST}),
    "failover": lambda: failover_shape({0: 0, 45: WOVF | GHOST, 63: WOVF, 64: 0}),
    # reply_when_commit never calls exec, execute stays 0: 12 requests in all, within W
    "rwc": lambda: shape((5,), 16, 32, 3, [0] * 4, 150, {0: 0, 63: 0, 64: 0, 69: 0}, max_requests=3, reply_when_commit=1),
    "rwc_forwarded": lambda: shape((5,), 16, 32, 3, [0, 1, 2, 3], 150, {0: 0, 63: 0, 64: 0, 69: 0}, max_requests=3,
                                   reply_when_commit=1),
    "rwc_ephemeral": lambda: shape((5,), 16, 32, 3, [0, 1, 2, 3, 4], 150,
                                   {0: POISON, 63: POISON, 64: POISON, 69: POISON}, max_requests=3,
                                   reply_when_commit=1, ephemeral_leader=1),
}
U = abi.F_UNFAITHFUL
# the flag words of all 70 clusters of each shape, measured on the oracle (the table of DESIGN.md §3.5f): the
# clusters outside the claim are not replayed, but a raise of UNFAITHFUL that went missing would move them
FLAG_COUNTS = {
    "wrap": {WOVF: 5, GHOST: 25, WOVF | GHOST: 40},
    "wrap9": {0: 7, WOVF: 63},
    "forwarding": {0: 3, WOVF: 19, GHOST: 7, WOVF | GHOST: 41},
    "thrifty": {0: 29, GHOST: 41},
    "n3": {0: 51, WOVF: 19},
    "n2": {0: 70},
    "ephemeral": {GHOST: 51, POISON | GHOST: 2, GHOST | U: 8, WOVF | GHOST | U: 8, POISON | GHOST | U: 1},
    "flaky": {GHOST: 3, WOVF | GHOST: 7, POISON | GHOST: 13, GHOST | U: 3, WOVF | GHOST | U: 35, POISON | GHOST | U: 6,
              POISON | WOVF | GHOST | U: 3},
    "crash": {GHOST: 8, WOVF | GHOST: 52, WOVF | GHOST | U: 10},
    "failover": {0: 16, WOVF: 20, WOVF | GHOST: 1, WOVF | U: 21, WOVF | GHOST | U: 12},
    "rwc": {0: 70},
    "rwc_forwarded": {0: 70},
    "rwc_ephemeral": {POISON: 70},
}


def flag_counts(sim):
    """{flag word: clusters} over every cluster of a finished run."""
    st, N = sim.read_state(), sim.N
    words = [0] * (len(st) // N)
    for i, s in enumerate(st):
        words[i // N] |= s.flags
    return dict(collections.Counter(words))


WRAPS = ("wrap", "wrap9")                                  # slot >= 4 * W
OUT_OF_WINDOW = ("wrap", "crash")                          # model entries below execute and beyond the window


def committed_ghost_case():
    """N = 3, one worker at A, no delays: A leads under ballot 1.A and has executed slot 0 by step
    5.  A transport then hands A, from B, the P3 of slot 0 once more (step 8: Go re-creates the
    entry below execute, committed) and a P2b for slot 0 under the higher ballot 2.B (step 9: the
    entry is committed, so HandleP2b returns before it looks at the ballot, paxos.go:273).  A must
    stay the active leader under 1.A.  Returns the shape and {step: deliver's arguments}."""
    sh = shape((3,), 16, 16, 0, [0], 20, {0: GHOST}, max_requests=3, slow=False)
    sh = sh._replace(cfg=abi.make_config(npz=[3], clusters=1, seed=SEED, window=16, mbox_cap=16, max_delay=0))
    return sh, {8: (0, 0, 1, [(1, T_P3, (1 << 4) | 0, 0, 1)]), 9: (0, 0, 1, [(1, T_P2B, (2 << 4) | 1, 0, 0)])}


def inject_case():
    """test_parity_gpu.py::test_inject_and_read_log's run on the traced clusters: every 9 steps a
    client request goes to a replica that need not be the leader.  Under its heavy Drop faults
    most clusters raise UNFAITHFUL; the traced four do not.  Returns the shape and
    [(step, cluster, replica, cid)]."""
    sh = shape((5,), 16, 16, 3, [0, 0], 108, {12: GHOST, 21: GHOST, 45: GHOST, 57: GHOST}, max_requests=40,
               ephemeral_leader=1)
    sh = sh._replace(cfg=abi.make_config(npz=[5], clusters=CLUSTERS, seed=13, window=16, mbox_cap=16, max_delay=3,
                                         ephemeral_leader=1),
                     fp=abi.make_fault_process(drop_ppm=20000, drop_len=5, slow_ppm=20000, slow_len=5, slow_min=1,
                                               slow_max=3))
    inj, cid = [], 1 << 20
    for k in range(12):
        for c in range(0, CLUSTERS, 3):
            inj.append((9 * k, c, (c + k) % 5, cid))
            cid += 1
    return sh, inj
