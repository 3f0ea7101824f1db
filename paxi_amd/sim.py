"""Host-side mirror of the reference's simulation entry point over the HIP C-ABI.

`Simulation` plays the role of `server -sim` (server/server.go:87-101) for a
whole batch of clusters: it takes a paxi.Config-like description (zones and
nodes per zone, quorum options, config.go:14-35), a benchmark workload
(benchmark.go:21-48) and fault injection (socket.go:163-199), and advances all
clusters on one GPU through libpaxisim.so.  There is no CPU fallback: if the
HIP library or the device is missing, construction raises.
"""
import ctypes as C
import os

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# PAXISIM_LIB selects another build of the same HIP library (tuning variants)
LIB_PATH = os.environ.get("PAXISIM_LIB") or os.path.join(_HERE, "libpaxisim.so")
_lib = None
_PU32, _PU64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)   # what the numpy-buffer wrappers hand over
PaxisimError = abi.PaxisimError
# every call include/*.h declares: the product's names of the one prototype table
EXPORTED = [name for name in abi.PROTOTYPES if name.startswith("paxisim_")]


def quorum(cfg, kind, ack_mask):
    """paxisim_quorum: the kernels' quorum predicate (quorum.go:55-119) for cfg's zones; host only."""
    ok = C.c_int()
    _check(load_library().paxisim_quorum(C.byref(cfg), kind, ack_mask, C.byref(ok)))
    return bool(ok.value)


def load_library():
    """Load the in-tree HIP library, bound by abi.PROTOTYPES; raise if it is absent (no fallback).
    A call the library lacks raises PaxisimError where it is looked up (abi.Bound)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PaxisimError(f"HIP library not built: {LIB_PATH} (run `python -c 'import __graft_entry__ as g; g.build()'`)")
    L = abi.bind(C.CDLL(LIB_PATH), "paxisim")
    if L.paxisim_abi_version() != abi.ABI_VERSION:
        raise PaxisimError("ABI version mismatch between paxi_amd/abi.py and libpaxisim.so")
    _lib = L
    return L


def build_id():
    """The source fingerprint compiled into the loaded library (paxisim_build_id)."""
    return load_library().paxisim_build_id().decode()


def consensus_of_histories(histories):
    """HTTPClient.Consensus (client.go:302-319) over the replicas' History(k) lists: at every index
    the values present form a set of at most one.  (True, None), or (False, the first index that fails)."""
    n = max((len(h) for h in histories), default=0)
    for i in range(n):
        present = set()
        for h in histories:
            if len(h) > i:
                present.add(h[i])
        if len(present) > 1:
            return False, i
    return True, None


def _select(fn, n, cap):
    """Run a select call `fn(ids pointer or None, cap, total pointer)` so that it returns the first
    `cap` matches, or every match when cap is None: (ids as a numpy uint64 array, total).  With cap
    None the first call offers room for 65,536 ids, and only a larger total costs a second call."""
    import numpy as np
    tot = C.c_uint64()
    room = min(n, 1 << 16) if cap is None else min(int(cap), n)
    ids = np.empty(room, dtype=np.uint64)
    fn(ids.ctypes.data_as(_PU64) if room else None, room, C.byref(tot))
    if cap is None and tot.value > room:
        room = tot.value
        ids = np.empty(room, dtype=np.uint64)
        fn(ids.ctypes.data_as(_PU64), room, C.byref(tot))
    return ids[:min(room, tot.value)], tot.value


def select_words(words, any, none=0, cap=None, device=0):
    """paxisim_select_words: the indices i of `words` (uint32) with (any == 0 or words[i] & any) and
    not words[i] & none, ascending, found on the device: (the first `cap` of them - all when cap is
    None - as a numpy uint64 array, the exact number of matches)."""
    import numpy as np
    fn = load_library().paxisim_select_words
    w = np.ascontiguousarray(words, dtype=np.uint32)
    ptr = w.ctypes.data_as(_PU32) if w.size else None
    return _select(lambda ids, k, tot: _check(fn(device, ptr, w.size, any, none, ids, k, tot)), w.size, cap)


def _check(rc):
    if rc != 0:
        raise PaxisimError(f"paxisim error {rc}: {load_library().paxisim_last_error().decode()}")


# The two readers below take the call and the error check as arguments: a handle class written
# outside Handle (a loader of its own around abi.declare) imports them from here.
def _read_inbox(fn, h, cluster, replica, check):
    n = C.c_uint32()
    cap = 256
    while True:
        arr = (abi.InboxRecord * cap)()
        check(fn(h, cluster, replica, arr, cap, C.byref(n)))
        if n.value <= cap:
            return [arr[i].as_tuple() for i in range(n.value)]
        cap = n.value


def _read_client(fn, h, cluster, n, check):
    arr = (abi.WorkerState * max(1, n))()
    got = C.c_uint32()
    check(fn(h, cluster, arr, n, C.byref(got)))
    return [arr[i].as_tuple() for i in range(min(n, got.value))]


class Handle:
    """What a Simulation and the tests' CPU oracle share: a batch of clusters behind one handle of
    a bound library (abi.Bound, which knows the prefix), with that library's error check.  A
    subclass sets `_library`, the function that returns its bound library, and `_raise_on`, which
    raises on a non-zero return code."""
    _library = staticmethod(load_library)
    _raise_on = staticmethod(_check)

    def __init__(self, cfg, wl, fp=None, faults=()):
        self.cfg, self.wl, self.fp = cfg, wl, fp
        self.N = abi.n_replicas(cfg)
        self.h = C.c_void_p()
        self._raise_on(self._library().create(C.byref(cfg), C.byref(wl), C.byref(fp) if fp else None,
                                              C.byref(self.h)))
        for f in faults:
            self.fault(f)

    # socket.go Drop/Slow/Flaky/Crash, scripted
    def fault(self, f):
        self._raise_on(self._library().fault_add(self.h, C.byref(f)))

    def stats(self):
        s = abi.Stats()
        self._raise_on(self._library().stats_get(self.h, C.byref(s)))
        return s

    def read_state(self, lo=0, n=None):
        n = self.cfg.clusters - lo if n is None else n
        arr = (abi.ReplicaState * (n * self.N))()
        self._raise_on(self._library().read_state(self.h, lo, n, arr))
        return arr

    def read_instances(self, lo=0, n=None):
        """Per (cluster, replica, key) Paxos instance state (paxisim_read_instances)."""
        n = self.cfg.clusters - lo if n is None else n
        arr = (abi.InstanceState * (n * self.N * abi.n_instances(self.cfg)))()
        self._raise_on(self._library().read_instances(self.h, lo, n, arr))
        return arr

    def check(self):
        v = C.c_uint64()
        self._raise_on(self._library().check(self.h, C.byref(v)))
        return v.value

    def inject(self, cluster, replica, cid):
        """A client request for command `cid` at `replica` in the next step (http.go:99)."""
        self._raise_on(self._library().inject(self.h, cluster, replica, cid))

    def read_inbox(self, cluster, replica):
        """Records replica `replica` receives at the next step, by source (paxisim_read_inbox)."""
        return _read_inbox(self._library().read_inbox, self.h, cluster, replica, self._raise_on)

    def deliver(self, cluster, replica, src, recs):
        """Append records (src, hdr, ballot, slot, cid) to the replica's next-step
        inbox from source `src` (paxisim_deliver; a record's own src is ignored)."""
        arr = (abi.InboxRecord * max(1, len(recs)))(*[abi.InboxRecord(src, *r[-4:]) for r in recs])
        self._raise_on(self._library().deliver(self.h, cluster, replica, src, arr, len(recs)))

    def read_log(self, cluster, replica, slot_lo, n, key=0):
        """paxos.go entries of slots [slot_lo, slot_lo+n) of one instance (paxisim_read_log)."""
        arr = (abi.LogEntry * max(1, n))()
        self._raise_on(self._library().read_log(self.h, cluster, replica, key, slot_lo, n, arr))
        return list(arr[:n])

    def history(self, cluster):
        fn = self._library().history
        n = C.c_uint32()
        self._raise_on(fn(self.h, cluster, None, 0, C.byref(n)))
        buf = (C.c_uint32 * max(1, 5 * n.value))()
        self._raise_on(fn(self.h, cluster, buf, n.value, C.byref(n)))
        return [tuple(buf[5 * i: 5 * i + 5]) for i in range(n.value)]

    def read_client(self, cluster):
        """[(cid, issued, reply_value)] of the cluster's closed-loop workers (paxisim_read_client)."""
        return _read_client(self._library().read_client, self.h, cluster, self.wl.outstanding, self._raise_on)

    def read_kv(self, cluster, replica, n):
        """Database.Get (db.go:116-121) of keys [0, n) of one replica (paxisim_read_kv)."""
        buf = (C.c_uint32 * max(1, n))()
        self._raise_on(self._library().read_kv(self.h, cluster, replica, buf, n))
        return list(buf[:n])

    def history_load(self, cluster, replica, ops):
        """History.ReadFile into the device (paxisim_history_load): ops are
        (key, is_write, value, start, end) tuples."""
        flat = [int(v) for o in ops for v in o]
        buf = (C.c_uint32 * max(1, len(flat)))(*flat)
        self._raise_on(self._library().history_load(self.h, cluster, replica, buf, len(ops)))

    def close(self):
        if self.h:
            self._library().destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Simulation(Handle):
    """A batch of independent N-replica clusters on one GPU (one handle)."""

    def step(self, n):
        _check(load_library().paxisim_step(self.h, n))

    def step_unit(self):
        """paxisim_step_unit: the step-kernel unit the next launch runs - abi.UNIT_GENERIC, or
        abi.UNIT_FIXED_PAXOS5 for a handle of the headline's fixed shape (include/paxisim_shape.h)."""
        u = C.c_uint32()
        _check(load_library().paxisim_step_unit(self.h, C.byref(u)))
        return u.value

    def sync(self):
        _check(load_library().paxisim_sync(self.h))

    def commands(self, cluster, cids):
        """[(key index, is_write)] of command ids of a cluster (paxisim_commands)."""
        n = len(cids)
        a = (C.c_uint32 * max(1, n))(*cids)
        k, w = (C.c_uint32 * max(1, n))(), (C.c_uint32 * max(1, n))()
        _check(load_library().paxisim_commands(self.h, cluster, a, n, k, w))
        return [(k[i], bool(w[i])) for i in range(n)]

    def linearizable(self):
        """History.Linearizable (history.go:55-71): (anomalies, ops checked, partitions skipped)."""
        a, n, sk = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(load_library().paxisim_linearizable(self.h, C.byref(a), C.byref(n), C.byref(sk)))
        return a.value, n.value, sk.value

    def kernel_time(self, reset=False):
        ms, n = C.c_double(), C.c_uint64()
        _check(load_library().paxisim_kernel_time(self.h, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    def occupancy(self):
        """(workgroups resident per CU, dynamic LDS bytes per workgroup, messages staged per replica-step)"""
        b, lds, j = C.c_int(), C.c_uint32(), C.c_uint32()
        _check(load_library().paxisim_occupancy(self.h, C.byref(b), C.byref(lds), C.byref(j)))
        return b.value, lds.value, j.value

    def active_clusters(self):
        """Clusters the step kernels still visit (the rest are frozen at a fixed point)."""
        b = C.c_uint64()
        _check(load_library().paxisim_active_clusters(self.h, C.byref(b)))
        return b.value

    def activity(self, lo=0, n=None):
        """Per cluster: None while the step kernels visit it, else the step at
        which it froze at its fixed point (paxisim_read_activity)."""
        n = self.cfg.clusters - lo if n is None else n
        buf = (C.c_uint32 * max(1, n))()
        _check(load_library().paxisim_read_activity(self.h, lo, n, buf))
        return [None if buf[i] == 0xFFFFFFFF else buf[i] for i in range(n)]

    def device_bytes(self):
        b = C.c_uint64()
        _check(load_library().paxisim_device_bytes(self.h, C.byref(b)))
        return b.value

    # client request latency (stat.go, benchmark.go:186)
    def latency_enable(self, bins=256):
        """Record every worker's request latency from now on, in `bins` one-step
        bins (a power of two in [16, abi.LAT_MAX_BINS]); before the first step only."""
        _check(load_library().paxisim_latency_enable(self.h, bins))

    def latency_reset(self):
        """Forget the samples so far (a warm-up); requests in flight keep their issue step."""
        _check(load_library().paxisim_latency_reset(self.h))

    def latency(self, worker=None):
        """The latency.Histogram of one worker, or of all workers (worker=None)."""
        from .latency import Histogram
        lat = abi.Latency()
        fn = load_library().paxisim_latency_get
        w = abi.ALL_WORKERS if worker is None else worker
        hist = (C.c_uint64 * abi.LAT_MAX_BINS)()
        _check(fn(self.h, w, C.byref(lat), hist))
        return Histogram(hist[:lat.bins], lat.count, lat.sum, lat.overflow, lat.min, lat.max)

    # client-side op history of every protocol (benchmark.go:246-275, history.go)
    def client_history_enable(self, ops_per_worker):
        """Record every worker's completed ops, `ops_per_worker` per worker and cluster (later ones
        are counted as dropped); once, before the first step and after latency_enable."""
        _check(load_library().paxisim_client_history_enable(self.h, ops_per_worker))

    def client_history(self, cluster):
        """([(key, is_write, value, start, end)] in canonical order - worker 0's ops in completion
        order, then worker 1's, ... -, ops dropped past ops_per_worker) of one cluster."""
        fn = load_library().paxisim_client_history
        n, d = C.c_uint32(), C.c_uint32()
        _check(fn(self.h, cluster, None, 0, C.byref(n), C.byref(d)))
        buf = (C.c_uint32 * max(1, 5 * n.value))()
        _check(fn(self.h, cluster, buf, n.value, C.byref(n), C.byref(d)))
        return [tuple(buf[5 * i: 5 * i + 5]) for i in range(n.value)], d.value

    def client_history_load(self, cluster, worker, ops):
        """History.ReadFile into the device (paxisim_client_history_load): replace one worker's
        ops with (key, is_write, value, start, end) tuples."""
        flat = [int(v) for o in ops for v in o]
        buf = (C.c_uint32 * max(1, len(flat)))(*flat)
        _check(load_library().paxisim_client_history_load(self.h, cluster, worker, buf, len(ops)))

    def client_linearizable(self):
        """History.Linearizable over the client histories: (anomalies, ops checked, partitions skipped)."""
        a, n, sk = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(load_library().paxisim_client_linearizable(self.h, C.byref(a), C.byref(n), C.byref(sk)))
        return a.value, n.value, sk.value

    # multi-version Database and Consensus (db.go:123-155, client.go:279-320)
    def multiversion_enable(self, versions_per_key):
        """Keep every replica's History(key): the first `versions_per_key` values put per key (later
        ones are counted as dropped); once, before the first step and after latency_enable."""
        _check(load_library().paxisim_multiversion_enable(self.h, versions_per_key))
        self._mv_cap = versions_per_key

    def kv_history(self, cluster, replica, key):
        """Database.History(key) of one replica: (the values kept, in put order; values dropped)."""
        fn = load_library().paxisim_kv_history
        cap = getattr(self, "_mv_cap", 0)
        buf = (C.c_uint32 * max(1, cap))()
        n, d = C.c_uint32(), C.c_uint32()
        _check(fn(self.h, cluster, replica, key, buf, cap, C.byref(n), C.byref(d)))
        return list(buf[:n.value]), d.value

    def consensus(self):
        """Consensus over every (cluster, key): (pairs that fail over the kept prefixes, values ever
        put, values dropped)."""
        f, v, d = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(load_library().paxisim_consensus(self.h, C.byref(f), C.byref(v), C.byref(d)))
        return f.value, v.value, d.value

    def consensus_failed(self, lo=0, n=None):
        """Per cluster of [lo, lo + n): the bit mask of the keys whose Consensus fails."""
        n = self.cfg.clusters - lo if n is None else n
        buf = (C.c_uint64 * max(1, n))()
        _check(load_library().paxisim_consensus_failed(self.h, lo, n, buf))
        return list(buf[:n])

    def consensus_of(self, cluster, key):
        """HTTPClient.Consensus(key) of one cluster from the replicas' readouts: (True, None), or
        (False, the first index at which two replicas hold different values)."""
        return consensus_of_histories([self.kv_history(cluster, r, key)[0] for r in range(self.N)])

    # message traces of chosen clusters, recorded on the device
    def trace_enable(self, clusters, records_per_replica, step_from=0, step_to=2**32 - 1):
        """Record what every replica of the local clusters `clusters` receives at steps [step_from,
        step_to): the first `records_per_replica` records per (cluster, replica), later ones counted
        as dropped; once, before the first step and after latency_enable."""
        clusters = list(clusters)
        arr = (C.c_uint64 * max(1, len(clusters)))(*clusters)
        _check(load_library().paxisim_trace_enable(self.h, arr, len(clusters), records_per_replica, step_from,
                                                   step_to))

    def trace_read(self, cluster, replica):
        """([(step, src, hdr, ballot, slot, cid)] one replica of a traced cluster received, by step,
        then source, then FIFO; records dropped past records_per_replica)."""
        fn = load_library().paxisim_trace_read
        n, d = C.c_uint32(), C.c_uint32()
        _check(fn(self.h, cluster, replica, None, 0, C.byref(n), C.byref(d)))
        arr = (abi.TraceRecord * max(1, n.value))()
        _check(fn(self.h, cluster, replica, arr, n.value, C.byref(n), C.byref(d)))
        return [arr[i].as_tuple() for i in range(n.value)], d.value

    def trace_totals(self):
        """(records kept, records dropped) over every traced (cluster, replica)."""
        k, d = C.c_uint64(), C.c_uint64()
        _check(load_library().paxisim_trace_totals(self.h, C.byref(k), C.byref(d)))
        return k.value, d.value

    # snapshot, restore and fork
    def snapshot_size(self):
        """The exact size in bytes of a snapshot taken now."""
        n = C.c_uint64()
        _check(load_library().paxisim_snapshot_size(self.h, C.byref(n)))
        return n.value

    def snapshot(self):
        """The handle's whole simulation state at this step, as a numpy uint8 array (the blob of
        include/paxisim_snapshot.h; of the mailboxes only the live records)."""
        import numpy as np
        blob = np.empty(self.snapshot_size(), dtype=np.uint8)
        n = C.c_uint64()
        _check(load_library().paxisim_snapshot(self.h, blob.ctypes.data_as(C.c_void_p), blob.nbytes, C.byref(n)))
        assert n.value == blob.nbytes
        return blob

    def restore(self, blob):
        """Overwrite the handle's state with a snapshot's: of the same build, plan and recorders
        (else PaxisimError, and the handle is unchanged).  Restoring a handle's own snapshot rewinds it."""
        import numpy as np
        blob = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob)
        _check(load_library().paxisim_restore(self.h, blob.ctypes.data_as(C.c_void_p), blob.nbytes))

    def fork(self):
        """A second, independent Simulation on the same device at the same state (device to device)."""
        h = C.c_void_p()
        _check(load_library().paxisim_fork(self.h, C.byref(h)))
        f = object.__new__(Simulation)
        f.cfg, f.wl, f.fp, f.N, f.h = self.cfg, self.wl, self.fp, self.N, h
        if hasattr(self, "_mv_cap"):
            f._mv_cap = self._mv_cap
        return f

    # per-cluster verdict words and the search over them
    def verdict_available(self):
        """The abi.V_* / abi.F_* bits this handle can produce."""
        b = C.c_uint32()
        _check(load_library().paxisim_verdict_available(self.h, C.byref(b)))
        return b.value

    def verdicts(self, scans=0, lo=0, n=None):
        """The verdict words of local clusters [lo, lo + n) as a numpy uint32 array, evaluated now;
        `scans`: which of abi.V_CONSENSUS | V_LIN | V_CLIENT_LIN to run (their bits are 0 otherwise)."""
        import numpy as np
        n = self.cfg.clusters - lo if n is None else n
        w = np.empty(max(0, n), dtype=np.uint32)
        _check(load_library().paxisim_verdicts(self.h, scans, lo, n, w.ctypes.data_as(_PU32) if w.size else None))
        return w

    def find(self, any, none=0, scans=None, cap=None, global_ids=False):
        """The clusters whose verdict word has a bit of `any` (any == 0: every cluster) and none of
        `none`, found on the device: (ids ascending as a numpy uint64 array - the first `cap`, all when
        cap is None -, the exact number of matches).  `scans` defaults to the scan bits in any | none;
        ids are local, or with global_ids have cfg.cluster_base added."""
        scans = (any | none) & abi.V_SCANS if scans is None else scans
        fn = load_library().paxisim_find
        ids, total = _select(lambda p, k, tot: _check(fn(self.h, scans, any, none, p, k, tot)), self.cfg.clusters, cap)
        if global_ids:
            ids = ids + ids.dtype.type(self.cfg.cluster_base)
        return ids, total

    def verdict_counts(self, scans=0):
        """{bit name: clusters whose verdict word has the bit} (names: abi.V_NAMES)."""
        c = (C.c_uint64 * 32)()
        _check(load_library().paxisim_verdict_counts(self.h, scans, c))
        return {name: c[b] for b, name in abi.V_NAMES.items()}


class Dist:
    """RCCL reduction of statistics over handles (paxisim_dist_*): either one
    process driving several handles (`Dist(sims)`) or one handle per process
    (`Dist.join(sim, uid, nranks, rank)` with `uid` from `Dist.unique_id()` on
    one rank, shipped by the caller's launcher)."""

    def __init__(self, sims=None, _h=None, _members=1):
        L = load_library()
        self.h = C.c_void_p()
        if _h is not None:
            self.h, self.members = _h, _members
            return
        arr = (C.c_void_p * len(sims))(*[s.h.value for s in sims])
        _check(L.paxisim_dist_init(arr, len(sims), C.byref(self.h)))
        self.members = len(sims)

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        _check(load_library().paxisim_dist_unique_id(buf))
        return buf.raw

    @classmethod
    def join(cls, sim, uid, nranks, rank):
        h = C.c_void_p()
        _check(load_library().paxisim_dist_init_rank(sim.h, uid, nranks, rank, C.byref(h)))
        return cls(_h=h, _members=1)

    def allreduce(self, sums, maxes):
        """Sum `sums` (per member: a list of ints) and max `maxes` (per member: floats)."""
        n, m = len(sums[0]) if sums else 0, len(maxes[0]) if maxes else 0
        si = (C.c_uint64 * max(1, n * self.members))(*[int(v) for row in sums for v in row])
        mi = (C.c_double * max(1, m * self.members))(*[float(v) for row in maxes for v in row])
        so, mo = (C.c_uint64 * max(1, n))(), (C.c_double * max(1, m))()
        _check(load_library().paxisim_dist_allreduce(self.h, si, n, mi, m, so, mo))
        return list(so[:n]), list(mo[:m])

    def stats(self):
        """(paxisim_stats summed over the job, max step-kernel ms of any handle)"""
        s, ms = abi.Stats(), C.c_double()
        _check(load_library().paxisim_dist_stats(self.h, C.byref(s), C.byref(ms)))
        return s, ms.value

    def close(self):
        if self.h:
            load_library().paxisim_dist_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
