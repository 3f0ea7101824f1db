"""ctypes mirror of include/paxisim.h (the C-ABI boundary).

Only type and constant definitions live here; no library is loaded.  The HIP
product binding (paxi_amd.sim) and the test-side oracle loader both use these
structs, so the two speak exactly the same ABI.
"""
import ctypes as C

ABI_VERSION = 14
MAX_N = 16
MAX_ZONES = 16
MAX_WORKERS = 32
MAX_KEYS = 64
MAX_FAULTS = 64
MAX_WINDOW = 64
MAX_MBOX = 64
MAX_DELAY = 14
CLIENT_SRC = 31
ALL_DST = 0xFF
LAT_MAX_BINS = 4096          # paxisim_latency_enable: bins is a power of two in [16, LAT_MAX_BINS]
ALL_WORKERS = 0xFFFFFFFF     # paxisim_latency_get: every worker summed
MV_MAX = 1 << 16             # paxisim_multiversion_enable: versions_per_key is in [1, MV_MAX]
TRACE_MAX_CLUSTERS = 1 << 16 # paxisim_trace_enable: n_clusters is in [1, TRACE_MAX_CLUSTERS]
TRACE_MAX_RECORDS = 1 << 20  # and records_per_replica in [1, TRACE_MAX_RECORDS]

# error codes
OK, EINVAL, ENOMEM, EDEVICE, EUNSUPP, ERANGE = 0, -1, -2, -3, -4, -5

# protocols (server/server.go:38-84)
PAXOS, ABD, WPAXOS, M2PAXOS, KPAXOS, EPAXOS = 0, 1, 2, 3, 4, 5
PER_KEY = (WPAXOS, M2PAXOS, KPAXOS)   # protocols with one Paxos instance per key

# quorum predicates (quorum.go)
Q_MAJORITY, Q_ALL, Q_FAST, Q_GRID_ROW, Q_ZONE_MAJORITY, Q_GRID_COLUMN, Q_FGRID_Q1, Q_FGRID_Q2 = range(8)

# message types
(MSG_NONE, MSG_REQUEST, MSG_REPLY, MSG_P1A, MSG_P1B, MSG_P1B_ENTRY, MSG_P2A, MSG_P2B,
 MSG_P3, MSG_GET, MSG_GETREPLY, MSG_SET, MSG_SETREPLY, MSG_LEADERCHG, MSG_PREACCEPT, MSG_PREACCEPTREPLY,
 MSG_ACCEPT, MSG_ACCEPTREPLY, MSG_COMMIT) = range(19)
NMSG = 20
MSG_NAMES = {MSG_REQUEST: "Request", MSG_REPLY: "Reply", MSG_P1A: "P1a", MSG_P1B: "P1b",
             MSG_P2A: "P2a", MSG_P2B: "P2b", MSG_P3: "P3", MSG_GET: "Get",
             MSG_GETREPLY: "GetReply", MSG_SET: "Set", MSG_SETREPLY: "SetReply",
             MSG_LEADERCHG: "LeaderChange", MSG_PREACCEPT: "PreAccept", MSG_PREACCEPTREPLY: "PreAcceptReply",
             MSG_ACCEPT: "Accept", MSG_ACCEPTREPLY: "AcceptReply", MSG_COMMIT: "Commit"}

# flags
F_WOVF, F_GHOST, F_MBOX_OVF, F_PEND_OVF, F_UNFAITHFUL, F_POISON, F_BALLOT_OVF, F_HIST_OVF = (
    0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80)

# WPaxos leader-migration policies (policy.go)
POLICY_CONSECUTIVE, POLICY_MAJORITY, POLICY_EMA = 0, 1, 2

# workload key distributions (benchmark.go:202-233)
DIST_UNIFORM, DIST_ORDER, DIST_CONFLICT, DIST_TABLE = 0, 1, 2, 3

# scripted faults (socket.go:163-199)
FAULT_DROP, FAULT_SLOW, FAULT_FLAKY, FAULT_CRASH = 0, 1, 2, 3


class Config(C.Structure):
    _fields_ = [
        ("protocol", C.c_uint32),
        ("n_zones", C.c_uint32),
        ("npz", C.c_uint32 * MAX_ZONES),
        ("q1", C.c_uint32), ("q2", C.c_uint32),
        ("fz", C.c_uint32),
        ("thrifty", C.c_uint32),
        ("ephemeral_leader", C.c_uint32),
        ("reply_when_commit", C.c_uint32),
        ("adaptive", C.c_uint32),
        ("policy_threshold", C.c_uint32),
        ("window", C.c_uint32),
        ("mbox_cap", C.c_uint32),
        ("max_delay", C.c_uint32),
        ("keys", C.c_uint32),
        ("steps_per_launch", C.c_uint32),
        ("history", C.c_uint32),
        ("device", C.c_int32),
        ("clusters", C.c_uint64),
        ("cluster_base", C.c_uint64),
        ("seed", C.c_uint64),
        ("policy", C.c_uint32),
        ("policy_interval", C.c_uint32),
        ("policy_alpha", C.c_double),
        ("agree_ring", C.c_uint32), ("kv", C.c_uint32),
    ]


class Workload(C.Structure):
    _fields_ = [
        ("outstanding", C.c_uint32),
        ("max_requests", C.c_uint32),
        ("write_ppm", C.c_uint32),
        ("locality_ppm", C.c_uint32),
        ("target", C.c_uint32 * MAX_WORKERS),
        ("distribution", C.c_uint32),
        ("conflicts", C.c_uint32),
        ("key_cdf", C.c_uint32 * MAX_KEYS),
        ("start_step", C.c_uint32 * MAX_WORKERS),
        ("key_min", C.c_uint32),
        ("key_space", C.c_uint32),
        ("key_tail", C.c_uint32),
        ("move_every", C.c_uint32),
        ("move_tables", C.c_uint32),
        ("move_loop", C.c_uint32),
        ("move_cdf", C.POINTER(C.c_uint32)),
    ]


class FaultProcess(C.Structure):
    _fields_ = [
        ("drop_ppm", C.c_uint32), ("drop_len", C.c_uint32),
        ("slow_ppm", C.c_uint32), ("slow_len", C.c_uint32),
        ("slow_min", C.c_uint32), ("slow_max", C.c_uint32),
    ]


class Fault(C.Structure):
    _fields_ = [
        ("kind", C.c_uint32), ("src", C.c_uint32), ("dst", C.c_uint32), ("param", C.c_uint32),
        ("cluster_lo", C.c_uint64), ("cluster_hi", C.c_uint64),
        ("step_from", C.c_uint32), ("step_to", C.c_uint32),
    ]


class ReplicaState(C.Structure):
    _fields_ = [
        ("ballot", C.c_uint64),
        ("slot", C.c_int32), ("execute", C.c_int32),
        ("active", C.c_uint32), ("flags", C.c_uint32),
        ("digest", C.c_uint64),
        ("p1_acks", C.c_uint32), ("npending", C.c_uint32),
        ("delivered", C.c_uint32 * NMSG),
        ("client_requests", C.c_uint32), ("sent", C.c_uint32),
        ("dropped", C.c_uint32), ("discarded", C.c_uint32),
        ("commits", C.c_uint32), ("replies", C.c_uint32),
        ("executed_writes", C.c_uint32), ("executions", C.c_uint32),
    ]

    def as_tuple(self):
        return (self.ballot, self.slot, self.execute, self.active, self.flags, self.digest,
                self.p1_acks, self.npending, tuple(self.delivered), self.client_requests,
                self.sent, self.dropped, self.discarded, self.commits, self.replies,
                self.executed_writes, self.executions)


class InstanceState(C.Structure):
    """One Paxos instance: a Multi-Paxos replica's paxos.Paxos, or a WPaxos kpaxos per key."""
    _fields_ = [
        ("ballot", C.c_uint64),
        ("slot", C.c_int32), ("execute", C.c_int32),
        ("active", C.c_uint32), ("exists", C.c_uint32),
        ("p1_acks", C.c_uint32), ("npending", C.c_uint32),
        ("digest", C.c_uint64),
        ("policy_last", C.c_uint32), ("policy_hits", C.c_uint32),
        ("policy_state", C.c_uint32 * 4),
    ]

    def as_tuple(self):
        return (self.ballot, self.slot, self.execute, self.active, self.exists, self.p1_acks,
                self.npending, self.digest, self.policy_last, self.policy_hits, tuple(self.policy_state))


LOG_EXISTS, LOG_COMMIT, LOG_QUORUM, LOG_REQUEST, LOG_HELD = 0x1, 0x2, 0x4, 0x8, 0x10


class LogEntry(C.Structure):
    """One paxos/paxos.go:11-18 entry of a replica's window (read_log)."""
    _fields_ = [
        ("ballot", C.c_uint64), ("slot", C.c_int32), ("cmd", C.c_uint32), ("flags", C.c_uint32),
        ("acks", C.c_uint32), ("request", C.c_uint32), ("pad", C.c_uint32),
    ]

    def as_tuple(self):
        return (self.ballot, self.slot, self.cmd, self.flags, self.acks, self.request)


class InboxRecord(C.Structure):
    """One record of a replica's next-step inbox (paxisim_read_inbox / paxisim_deliver)."""
    _fields_ = [("src", C.c_uint32), ("hdr", C.c_uint32), ("ballot", C.c_uint32), ("slot", C.c_uint32),
                ("cid", C.c_uint32)]

    def as_tuple(self):
        return (self.src, self.hdr, self.ballot, self.slot, self.cid)


class TraceRecord(C.Structure):
    """paxisim_trace_record: one record a traced replica received (paxisim_trace_read)."""
    _fields_ = [("step", C.c_uint32), ("src", C.c_uint32), ("hdr", C.c_uint32), ("ballot", C.c_uint32),
                ("slot", C.c_uint32), ("cid", C.c_uint32)]

    def as_tuple(self):
        return (self.step, self.src, self.hdr, self.ballot, self.slot, self.cid)


class WorkerState(C.Structure):
    """paxisim_worker_state: a closed-loop worker (benchmark.go:246-275) and its last Reply.Value."""
    _fields_ = [("cid", C.c_uint32), ("issued", C.c_uint32), ("reply_value", C.c_uint32), ("pad", C.c_uint32)]

    def as_tuple(self):
        return (self.cid, self.issued, self.reply_value)


class Latency(C.Structure):
    """paxisim_latency: the samples of one worker, or of all workers summed (latencies in steps)."""
    _fields_ = [("count", C.c_uint64), ("sum", C.c_uint64), ("overflow", C.c_uint64),
                ("min", C.c_uint32), ("max", C.c_uint32), ("bins", C.c_uint32), ("pad", C.c_uint32)]


class LatencyStat(C.Structure):
    """paxisim_latency_stat: Stat of stat.go:12-22, in ms = steps * step_ms."""
    _fields_ = [("size", C.c_uint64), ("mean", C.c_double), ("min", C.c_double), ("max", C.c_double),
                ("median", C.c_double), ("p95", C.c_double), ("p99", C.c_double), ("p999", C.c_double),
                ("exact", C.c_uint32), ("pad", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k in ("size", "mean", "min", "max", "median", "p95", "p99", "p999", "exact")}


class Stats(C.Structure):
    _fields_ = [
        ("steps", C.c_uint64), ("clusters", C.c_uint64),
        ("delivered", C.c_uint64 * NMSG),
        ("delivered_total", C.c_uint64),
        ("client_requests", C.c_uint64),
        ("sent", C.c_uint64), ("dropped", C.c_uint64), ("discarded", C.c_uint64),
        ("commits", C.c_uint64), ("replies", C.c_uint64),
        ("flagged", C.c_uint64 * 8),
        ("agree_compared", C.c_uint64), ("agree_missed", C.c_uint64), ("agree_mismatch", C.c_uint64),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k in ("steps", "clusters", "delivered_total", "client_requests",
                                            "sent", "dropped", "discarded", "commits", "replies",
                                            "agree_compared", "agree_missed", "agree_mismatch")}
        d["delivered"] = {MSG_NAMES.get(i, str(i)): self.delivered[i] for i in range(NMSG) if self.delivered[i]}
        d["flagged"] = list(self.flagged)
        return d


# Snapshot, restore and fork (include/paxisim_snapshot.h)
SNAPSHOT_SECTIONS = ("plan", "faults", "pools", "arena", "mailbox", "lat", "chist", "mv", "trace")
SNAPSHOT_HEADER = 256
SNAP_HAS_LAT, SNAP_HAS_CHIST, SNAP_HAS_MV, SNAP_HAS_TRACE = 1, 2, 4, 8


class SnapshotInfo(C.Structure):
    """struct paxisim_snapshot_info: what a snapshot's header says (paxisim_snapshot_info)."""
    _fields_ = [("version", C.c_uint32), ("protocol", C.c_uint32), ("n_replicas", C.c_uint32), ("step", C.c_uint32),
                ("clusters", C.c_uint64), ("cluster_base", C.c_uint64), ("mailbox_records", C.c_uint64),
                ("total_bytes", C.c_uint64), ("plan_hash", C.c_uint64), ("recorders", C.c_uint32),
                ("n_faults", C.c_uint32), ("section_bytes", C.c_uint64 * len(SNAPSHOT_SECTIONS)),
                ("build_id", C.c_char * 32)]


# Per-cluster verdict words and the search over them (include/paxisim_verdict.h).
# Bits 0..7 of a word are the F_* flags above.
V_FLAGS = 0xFF
V_AGREE, V_CONSENSUS, V_LIN, V_CLIENT_LIN, V_LIN_SKIPPED, V_TRUNCATED = (1 << b for b in range(8, 14))
V_QUIET, V_WAITING, V_STALLED = (1 << b for b in range(16, 19))
V_SCANS = V_CONSENSUS | V_LIN | V_CLIENT_LIN
V_ALL = 0x00073FFF
# bit number -> name, for Simulation.verdict_counts
V_NAMES = {0: "WOVF", 1: "GHOST", 2: "MBOX_OVF", 3: "PEND_OVF", 4: "UNFAITHFUL", 5: "POISON", 6: "BALLOT_OVF",
           7: "HIST_OVF", 8: "AGREE", 9: "CONSENSUS", 10: "LIN", 11: "CLIENT_LIN", 12: "LIN_SKIPPED",
           13: "TRUNCATED", 16: "QUIET", 17: "WAITING", 18: "STALLED"}


# enum paxisim_unit (include/paxisim_shape.h): what Simulation.step_unit returns
UNIT_GENERIC, UNIT_FIXED_PAXOS5 = 0, 1


class PaxisimError(RuntimeError):
    pass


# The C prototypes, name -> (restype, argtypes): the binding's single source, in the headers' own
# types (tests/test_abi.py compares every entry with include/*.h and oracle/oracle.h).  A handle
# (paxisim*, paxisim_dist*, oracle_sim*) and void* are c_void_p.
_P, _h, _int, _u32, _u64, _dbl = C.POINTER, C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_double
_pu32, _pu64 = _P(_u32), _P(_u64)

# calls the product library ("paxisim_") and the tests' CPU oracle ("oracle_") both have
_SHARED = {
    "create": (_int, [_P(Config), _P(Workload), _P(FaultProcess), _P(_h)]),
    "destroy": (_int, [_h]),
    "fault_add": (_int, [_h, _P(Fault)]),
    "stats_get": (_int, [_h, _P(Stats)]),
    "read_state": (_int, [_h, _u64, _u64, _P(ReplicaState)]),
    "read_instances": (_int, [_h, _u64, _u64, _P(InstanceState)]),
    "check": (_int, [_h, _pu64]),
    "inject": (_int, [_h, _u64, _u32, _u32]),
    "read_inbox": (_int, [_h, _u64, _u32, _P(InboxRecord), _u32, _pu32]),
    "deliver": (_int, [_h, _u64, _u32, _u32, _P(InboxRecord), _u32]),
    "read_log": (_int, [_h, _u64, _u32, _u32, C.c_int32, _u32, _P(LogEntry)]),
    "read_client": (_int, [_h, _u64, _P(WorkerState), _u32, _pu32]),
    "history": (_int, [_h, _u64, _pu32, _u32, _pu32]),
    "history_load": (_int, [_h, _u64, _u32, _pu32, _u32]),
    "read_kv": (_int, [_h, _u64, _u32, _pu32, _u32]),
    "last_error": (C.c_char_p, []),
}
PROTOTYPES = {f"{prefix}_{name}": proto for prefix in ("paxisim", "oracle") for name, proto in _SHARED.items()}
PROTOTYPES.update({
    "paxisim_abi_version": (_int, []),
    "paxisim_build_id": (C.c_char_p, []),
    "paxisim_step": (_int, [_h, _u32]),
    "paxisim_sync": (_int, [_h]),
    "paxisim_commands": (_int, [_h, _u64, _pu32, _u32, _pu32, _pu32]),
    "paxisim_kernel_time": (_int, [_h, _P(_dbl), _pu64, _int]),
    "paxisim_linearizable": (_int, [_h, _pu64, _pu64, _pu64]),
    "paxisim_occupancy": (_int, [_h, _P(_int), _pu32, _pu32]),
    "paxisim_active_clusters": (_int, [_h, _pu64]),
    "paxisim_read_activity": (_int, [_h, _u64, _u64, _pu32]),
    "paxisim_quorum": (_int, [_P(Config), _u32, _u32, _P(_int)]),
    "paxisim_device_bytes": (_int, [_h, _pu64]),
    # client request latency
    "paxisim_latency_enable": (_int, [_h, _u32]),
    "paxisim_latency_reset": (_int, [_h]),
    "paxisim_latency_get": (_int, [_h, _u32, _P(Latency), _pu64]),
    "paxisim_latency_stat_of": (_int, [_P(Latency), _pu64, _dbl, _P(LatencyStat)]),
    # the client-side op history of every protocol (§3.13)
    "paxisim_client_history_enable": (_int, [_h, _u32]),
    "paxisim_client_history": (_int, [_h, _u64, _pu32, _u32, _pu32, _pu32]),
    "paxisim_client_history_load": (_int, [_h, _u64, _u32, _pu32, _u32]),
    "paxisim_client_linearizable": (_int, [_h, _pu64, _pu64, _pu64]),
    # the multi-version Database and Consensus (§3.14)
    "paxisim_multiversion_enable": (_int, [_h, _u32]),
    "paxisim_kv_history": (_int, [_h, _u64, _u32, _u32, _pu32, _u32, _pu32, _pu32]),
    "paxisim_consensus": (_int, [_h, _pu64, _pu64, _pu64]),
    "paxisim_consensus_failed": (_int, [_h, _u64, _u64, _pu64]),
    # the device message trace (§3.15)
    "paxisim_trace_enable": (_int, [_h, _pu64, _u32, _u32, _u32, _u32]),
    "paxisim_trace_read": (_int, [_h, _u64, _u32, _P(TraceRecord), _u32, _pu32, _pu32]),
    "paxisim_trace_totals": (_int, [_h, _pu64, _pu64]),
    # RCCL reduction of statistics over handles
    "paxisim_dist_init": (_int, [_P(_h), _int, _P(_h)]),
    "paxisim_dist_unique_id": (_int, [C.c_char_p]),
    "paxisim_dist_init_rank": (_int, [_h, C.c_char_p, _int, _int, _P(_h)]),
    "paxisim_dist_allreduce": (_int, [_h, _pu64, _u32, _P(_dbl), _u32, _pu64, _P(_dbl)]),
    "paxisim_dist_stats": (_int, [_h, _P(Stats), _P(_dbl)]),
    "paxisim_dist_destroy": (_int, [_h]),
    # snapshot, restore and fork (include/paxisim_snapshot.h, §3.16)
    "paxisim_snapshot_size": (_int, [_h, _pu64]),
    "paxisim_snapshot": (_int, [_h, _h, _u64, _pu64]),
    "paxisim_restore": (_int, [_h, _h, _u64]),
    "paxisim_fork": (_int, [_h, _P(_h)]),
    "paxisim_snapshot_info": (_int, [_h, _u64, _P(SnapshotInfo)]),
    # per-cluster verdict words and the search over them (include/paxisim_verdict.h, §3.17)
    "paxisim_verdict_available": (_int, [_h, _pu32]),
    "paxisim_verdicts": (_int, [_h, _u32, _u64, _u64, _pu32]),
    "paxisim_find": (_int, [_h, _u32, _u32, _u32, _pu64, _u64, _pu64]),
    "paxisim_verdict_counts": (_int, [_h, _u32, _pu64]),
    "paxisim_select_words": (_int, [_int, _pu32, _u64, _u32, _u32, _pu64, _u64, _pu64]),
    # which step-kernel unit a handle runs (include/paxisim_shape.h, §5.20)
    "paxisim_step_unit": (_int, [_h, _pu32]),
    # the oracle's own
    "oracle_step": (_int, [_h, _u32, _int]),
    "oracle_set_replica_order": (_int, [_h, _u32]),
    "oracle_exec_log": (_int, [_h, _u64, _u32, _pu32, _u32, _pu32]),
    "oracle_lin_check": (_int, [_h, _pu64, _pu64]),
    "oracle_command": (_int, [_h, _u64, _u32, _pu32, _pu32]),
    "oracle_new_ballot": (_u64, [_u32, _u32, _u32]),
    "oracle_ballot_next": (_u64, [_u64, _u32, _u32]),
    "oracle_quorum": (_int, [_u32, _u32, _u32, _pu32, _u32]),
    "oracle_linearizable": (_int, [_P(C.c_int64), _int]),
})
# the two calls only an instrumented build has (paxisim.hip, in no header): tools/ bind them too
DEBUG_PROTOTYPES = {
    "paxisim_dbg_enable": (_int, [_h]),
    "paxisim_dbg_read": (_int, [_h, _P(C.c_ulonglong)]),
}


class Bound:
    """A loaded library's calls of one prefix, each under its table prototype, as attributes by
    full name and by the name without the prefix (`L.paxisim_check` is `L.check`).  A library built
    from older sources (the miscompile guard's pinned reproducers) lacks the newer calls: they are
    listed in `missing`, and looking one up raises PaxisimError.  That holds for hasattr(L, name)
    and getattr(L, name, None) too, which only catch AttributeError: ask `name in L.missing`."""

    def __init__(self, lib, prefix, table):
        self.lib, self.prefix, self.missing = lib, prefix, []
        for name, (res, args) in table.items():
            if not name.startswith(prefix + "_"):
                continue
            try:
                fn = getattr(lib, name)
            except AttributeError:
                self.missing.append(name)
                continue
            fn.restype, fn.argtypes = res, args
            self.__dict__[name] = self.__dict__[name[len(prefix) + 1:]] = fn

    def __getattr__(self, name):  # only reached for a name that __init__ did not bind
        d = self.__dict__                # empty before __init__ ran (copy, pickle): no lookups on self
        full = name if name.startswith(d.get("prefix", "") + "_") else f"{d.get('prefix')}_{name}"
        if full in d.get("missing", ()):
            raise PaxisimError(f"{d['lib']._name} was built without {full}")
        raise AttributeError(name)


def bind(lib, prefix, table=PROTOTYPES):
    """Give every `prefix`_ call of `table` that the ctypes library `lib` exports its prototype."""
    return Bound(lib, prefix, table)


def declare(lib, prefix):
    """bind() for a loader that keeps the ctypes library itself and returns it: the prototypes sit on
    lib's own function objects.  A call lib lacks is then ctypes' AttributeError, not PaxisimError."""
    return bind(lib, prefix).lib


def make_config(npz=(5,), protocol=PAXOS, q1=Q_MAJORITY, q2=Q_MAJORITY, fz=0, thrifty=0,
                ephemeral_leader=0, reply_when_commit=0, adaptive=1, policy_threshold=3,
                window=16, mbox_cap=16, max_delay=4, keys=16, steps_per_launch=0, device=0,
                clusters=1, cluster_base=0, seed=1, history=0, policy=POLICY_CONSECUTIVE, policy_interval=1,
                policy_alpha=0.5, agree_ring=0, kv=0):
    c = Config()
    c.protocol = protocol
    c.n_zones = len(npz)
    for i, v in enumerate(npz):
        c.npz[i] = v
    c.q1, c.q2, c.fz = q1, q2, fz
    c.thrifty, c.ephemeral_leader, c.reply_when_commit = thrifty, ephemeral_leader, reply_when_commit
    c.adaptive, c.policy_threshold = adaptive, policy_threshold
    c.window, c.mbox_cap, c.max_delay, c.keys = window, mbox_cap, max_delay, keys
    c.steps_per_launch, c.device, c.history = steps_per_launch, device, history
    c.clusters, c.cluster_base, c.seed = clusters, cluster_base, seed
    c.policy, c.policy_interval, c.policy_alpha = policy, policy_interval, policy_alpha
    c.agree_ring = agree_ring
    c.kv = kv
    return c


def make_workload(outstanding=1, max_requests=0, write_ppm=1_000_000, locality_ppm=0, target=0,
                  distribution="uniform", keys=None, start_step=0, key_min=0, **dist_params):
    """Closed-loop workload.  `distribution` is a Bconfig.Distribution name
    (benchmark.go:202-233, see paxi_amd.workload); the table distributions
    ("normal", "zipfan", "exponential") need the cluster's `keys`.  Other
    options: key_space (Bconfig.K of order/uniform/conflict), move_every
    (Bconfig.Move for normal), and the distribution's parameters."""
    from . import workload as _wl
    w = Workload()
    w.outstanding, w.max_requests, w.write_ppm, w.locality_ppm = outstanding, max_requests, write_ppm, locality_ppm
    w.key_min = key_min
    for i in range(MAX_WORKERS):
        w.target[i] = target[i % len(target)] if isinstance(target, (list, tuple)) else target
        w.start_step[i] = start_step[i % len(start_step)] if isinstance(start_step, (list, tuple)) else start_step
    _wl.set_distribution(w, distribution, keys, **dist_params)
    return w


def make_fault_process(drop_ppm=0, drop_len=0, slow_ppm=0, slow_len=0, slow_min=0, slow_max=0):
    f = FaultProcess()
    f.drop_ppm, f.drop_len, f.slow_ppm, f.slow_len, f.slow_min, f.slow_max = (
        drop_ppm, drop_len, slow_ppm, slow_len, slow_min, slow_max)
    return f


def make_fault(kind, src, dst=ALL_DST, param=0, cluster_lo=0, cluster_hi=2**63, step_from=0,
               step_to=0xFFFFFFFF):
    f = Fault()
    f.kind, f.src, f.dst, f.param = kind, src, dst, param
    f.cluster_lo, f.cluster_hi, f.step_from, f.step_to = cluster_lo, cluster_hi, step_from, step_to
    return f


def n_replicas(cfg):
    return sum(cfg.npz[i] for i in range(cfg.n_zones))


def n_instances(cfg):
    """read_instances records per replica: one kpaxos per key (WPaxos, M2Paxos,
    KPaxos), one per owner log (EPaxos), else one."""
    if cfg.protocol == EPAXOS:
        return n_replicas(cfg)
    return cfg.keys if cfg.protocol in PER_KEY else 1
