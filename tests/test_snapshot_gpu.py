"""Snapshot, restore and fork of a handle on the device.

The core property, for every protocol and kernel form: run A steps T1 then T2; run B steps T1, takes
a snapshot and is destroyed, a fresh handle restores the blob and steps T2; A and B are equal in
every readout the handle type has - read_inbox of every (cluster, replica) right after the restore
and at the end included - and A equals the oracle.  T1 = 37 is no multiple of a launch chunk, of D
or of 16.  The snapshot carries only live mailbox records: the blob's mailbox section is exactly
16 * mailbox_records bytes, and at max_delay 0 mailbox_records is the total length of read_inbox."""
import functools

import numpy as np
import pytest

from paxi_amd import abi, snapshot
import oracle_lib as ol
import trace_ref

pytestmark = pytest.mark.gpu
T1, T2 = 37, 63


def _sim():
    from paxi_amd.sim import Simulation
    return Simulation


def _err():
    from paxi_amd.sim import PaxisimError
    return PaxisimError


# ---- the shapes: (cfg, wl, fp, faults, recorders) -----------------------------------------------
def paxos5(clusters=130, **kw):
    """Shape 1: Multi-Paxos N = 5, the last block partial, the random fault process on, and a scripted
    Slow window of delay 3 on link 0 -> 1 over [T1 - 10, T1 + 10): what replica 0 sent to 1 before T1
    sits in buckets beyond the next one at T1."""
    cfg = abi.make_config(npz=[5], clusters=clusters, seed=11, window=16, mbox_cap=32, max_delay=4, kv=1, **kw)
    wl = abi.make_workload(outstanding=8, target=0, write_ppm=600_000, keys=8)
    fp = abi.make_fault_process(drop_ppm=3000, drop_len=20, slow_ppm=3000, slow_len=20, slow_min=1, slow_max=4)
    faults = (abi.make_fault(abi.FAULT_SLOW, 0, dst=1, param=3, step_from=T1 - 10, step_to=T1 + 10),)
    return cfg, wl, fp, faults, dict(lat=64, chist=16, mv=16)


def paxos9():
    """Shape 2: Multi-Paxos N = 9, FGrid 3x3: the idle-skip unit."""
    cfg = abi.make_config(npz=[3, 3, 3], clusters=130, seed=42, q1=abi.Q_FGRID_Q1, q2=abi.Q_FGRID_Q2, fz=1,
                          ephemeral_leader=1, window=16, mbox_cap=32, max_delay=0, steps_per_launch=20)
    wl = abi.make_workload(outstanding=8, target=[0, 0, 0, 0, 3, 3, 3, 3], start_step=[0, 0, 0, 0, 30, 30, 30, 30])
    return cfg, wl, None, (abi.make_fault(abi.FAULT_CRASH, 0, step_from=30),), {}


def wpaxos(window=8, **kw):
    """Shape 3: WPaxos 3x3; W = 8 uses the co-located blocks, the ema policy at W = 16 adds wpx."""
    cfg = abi.make_config(protocol=abi.WPAXOS, npz=[3, 3, 3], keys=6, fz=0, adaptive=1, policy_threshold=2,
                          clusters=70, seed=5, window=window, mbox_cap=24, max_delay=0, **kw)
    wl = abi.make_workload(outstanding=9, target=list(range(9)), locality_ppm=700_000, write_ppm=500_000)
    return cfg, wl, None, (), {}


def kpaxos():
    cfg = abi.make_config(protocol=abi.KPAXOS, npz=[3, 3, 3], keys=6, clusters=70, seed=7, window=8, mbox_cap=24,
                          max_delay=1)
    wl = abi.make_workload(outstanding=6, target=[0, 1, 3, 4, 6, 7], write_ppm=500_000)
    return cfg, wl, None, (), {}


def abd():
    cfg = abi.make_config(protocol=abi.ABD, npz=[5], clusters=70, seed=3, keys=4, mbox_cap=16, max_delay=2, history=64)
    wl = abi.make_workload(outstanding=3, target=[0, 1, 2], write_ppm=500_000)
    return cfg, wl, None, (), dict(lat=64, chist=16)


def epaxos():
    cfg = abi.make_config(protocol=abi.EPAXOS, npz=[5], clusters=70, seed=11, keys=4, window=32, mbox_cap=32,
                          max_delay=2, kv=1)
    wl = abi.make_workload(outstanding=5, target=list(range(5)), write_ppm=700_000)
    fp = abi.make_fault_process(drop_ppm=3000, drop_len=10, slow_ppm=3000, slow_len=20, slow_min=1, slow_max=2)
    return cfg, wl, fp, (), dict(lat=64, mv=16)


def overflow():
    """Shape 6: M = 8 against 8 workers and Slow windows: buckets fill and overflow."""
    cfg = abi.make_config(npz=[5], clusters=130, seed=77, window=8, mbox_cap=8, max_delay=6)
    wl = abi.make_workload(outstanding=8, target=0)
    fp = abi.make_fault_process(drop_ppm=5000, drop_len=40, slow_ppm=8000, slow_len=30, slow_min=2, slow_max=6)
    return cfg, wl, fp, (), {}


def dying(clusters=200):
    """Shape 5: every worker stops after 8 requests.  On the oracle 167 of the 200 clusters stop changing
    by step 30, the second compaction (every 15 steps), and the other 33 within five more steps: that
    compaction freezes most clusters and packs the live ones to the front."""
    cfg = abi.make_config(npz=[5], clusters=clusters, seed=13, window=16, mbox_cap=16, max_delay=3,
                          steps_per_launch=5)
    wl = abi.make_workload(outstanding=2, target=0, max_requests=8)
    fp = abi.make_fault_process(slow_ppm=30000, slow_len=6, slow_min=1, slow_max=3)
    return cfg, wl, fp, (), {}


def delay0():
    cfg = abi.make_config(npz=[5], clusters=130, seed=21, window=16, mbox_cap=16, max_delay=0)
    return cfg, abi.make_workload(outstanding=6, target=[0, 1, 2, 0, 0, 0]), None, (), {}


SHAPES = {"paxos5": paxos5, "paxos5_581": lambda: paxos5(581, steps_per_launch=20), "paxos9": paxos9,
          "wpaxos_w8": wpaxos, "wpaxos_ema_w16": lambda: wpaxos(16, policy=abi.POLICY_EMA, policy_alpha=0.3),
          "kpaxos": kpaxos, "abd": abd, "epaxos": epaxos, "overflow": overflow, "dying": dying, "delay0": delay0}


def make(name, env=None, monkeypatch=None, recorders=None, cls=None, faults=None):
    cfg, wl, fp, fl, rec = SHAPES[name]()
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    s = (cls or _sim())(cfg, wl, fp, fl if faults is None else faults)
    if cls is None:
        rec = rec if recorders is None else recorders
        if rec.get("lat"):
            s.latency_enable(rec["lat"])
        if rec.get("chist"):
            s.client_history_enable(rec["chist"])
        if rec.get("mv"):
            s.multiversion_enable(rec["mv"])
        s._rec = rec
    return s


def inboxes(s):
    return [s.read_inbox(c, r) for c in range(s.cfg.clusters) for r in range(s.N)]


def core(s):
    """The readouts an oracle handle has too."""
    n = s.cfg.clusters
    d = {"state": [x.as_tuple() for x in s.read_state()], "inst": [x.as_tuple() for x in s.read_instances()],
         "stats": s.stats().as_dict(), "check": s.check(), "client": [s.read_client(c) for c in range(n)],
         "inbox": inboxes(s)}
    if s.cfg.protocol == abi.ABD or s.cfg.kv:
        d["kv"] = [s.read_kv(c, r, s.cfg.keys) for c in range(n) for r in range(s.N)]
    if s.cfg.protocol == abi.ABD and s.cfg.history:
        d["history"] = [s.history(c) for c in range(n)]
    return d


def readout(s):
    """Every readout the handle type has."""
    n = s.cfg.clusters
    d = core(s)
    d["active"] = s.active_clusters()
    d["activity"] = s.activity()
    rec = getattr(s, "_rec", {})
    if s.cfg.protocol == abi.ABD and s.cfg.history:
        d["lin"] = s.linearizable()
    if rec.get("lat"):
        h = s.latency()
        d["lat"] = (h.counts.tolist(), h.count, h.sum, h.overflow, h.min, h.max)
        d["lat_w0"] = s.latency(0).counts.tolist()
    if rec.get("chist"):
        d["chist"] = [s.client_history(c) for c in range(n)]
        d["clin"] = s.client_linearizable()
    if rec.get("mv"):
        d["kvh"] = [s.kv_history(c, r, k) for c in range(0, n, 7) for r in range(s.N) for k in range(s.cfg.keys)]
        d["consensus"] = s.consensus()
        d["consensus_failed"] = s.consensus_failed()
    return d


def same(a, b, ctx):
    assert a.keys() == b.keys(), (ctx, sorted(a), sorted(b))
    for k in a:
        assert a[k] == b[k], f"{ctx}: {k} differ"


@functools.lru_cache(maxsize=None)
def oracle(name, steps=T1 + T2):
    o = make(name, cls=ol.OracleSim)
    o.step(steps)
    d = core(o)
    o.close()
    return d


def run_a(name, **kw):
    """Run A: T1 then T2 -> (readout at T1, readout at the end); a readout holds every inbox."""
    a = make(name, **kw)
    a.step(T1)
    mid = readout(a)
    a.step(T2)
    end = readout(a)
    a.close()
    return mid, end


def run_b(name, **kw):
    """Run B: T1, snapshot, destroy; a fresh handle restores and steps T2."""
    b = make(name, **kw)
    b.step(T1)
    size = b.snapshot_size()
    blob = b.snapshot()
    b.close()
    assert len(blob) == size
    f = make(name, **kw)
    f.restore(blob)
    mid = readout(f)
    f.step(T2)
    end = readout(f)
    f.close()
    return blob, mid, end


def check_blob(blob, name):
    i = snapshot.info(blob)
    cfg = SHAPES[name]()[0]
    assert i["step"] == T1 and i["clusters"] == cfg.clusters and i["N"] == abi.n_replicas(cfg)
    assert i["protocol"] == cfg.protocol and i["total_bytes"] == len(blob)
    assert i["sections"]["mailbox"] == 16 * i["mailbox_records"]      # the format's size claim
    assert sum(i["sections"].values()) + abi.SNAPSHOT_HEADER == len(blob)
    return i


def core_property(name, against_oracle=True, **kw):
    a_mid, a_end = run_a(name, **kw)
    blob, b_mid, b_end = run_b(name, **kw)
    check_blob(blob, name)
    same(a_mid, b_mid, f"{name} right after the restore")
    same(a_end, b_end, f"{name} at T1 + T2")
    if against_oracle:
        o = dict(oracle(name))
        if SHAPES[name]()[0].protocol == abi.ABD:
            del o["inst"]     # ABD has no Paxos instances: the two sides fill read_instances differently
        same({k: a_end[k] for k in o}, o, f"{name}: run A against the oracle")
    return blob, a_mid, a_end


# ---- shape 1 in every kernel form ----------------------------------------------------------------
def test_slow_window_puts_records_beyond_the_next_bucket():
    """On the oracle: replica 0 leads and sends to replica 1 inside the Slow window before T1, so at T1
    records for replica 1 are in flight in buckets the next step does not read."""
    o = make("paxos5", cls=ol.OracleSim)
    o.step(T1 - 10)
    st = o.read_state()
    assert sum(st[c * 5].active == 1 for c in range(130)) > 100, "replica 0 leads"
    sent0 = [st[c * 5].sent for c in range(130)]
    o.step(10)
    st = o.read_state()
    assert sum(st[c * 5].sent > sent0[c] for c in range(130)) > 100, "replica 0 sends inside the window"
    o.close()


@pytest.mark.parametrize("form", ["serial_pipelined", "barrier", "serial_unpipelined"])
def test_paxos5_forms(monkeypatch, form):
    env = {"barrier": {"PAXISIM_SERIAL": "0"}, "serial_unpipelined": {"PAXISIM_PIPE": "1"}, "serial_pipelined": {}}[form]
    core_property("paxos5", env=env, monkeypatch=monkeypatch)


def test_paxos5_two_pools(monkeypatch):
    env = {"PAXISIM_POOLS": "2", "PAXISIM_PHASE_SORT": "1"}
    core_property("paxos5_581", env=env, monkeypatch=monkeypatch)
    g = make("paxos5_581", env=env, monkeypatch=monkeypatch)
    g1 = make("paxos5_581", env={"PAXISIM_POOLS": "1"}, monkeypatch=monkeypatch)
    g.step(T1)
    blob = g.snapshot()
    with pytest.raises(_err(), match=r"snapshot plan differs: plan\.npools"):
        g1.restore(blob)
    g.close()
    g1.close()


@pytest.mark.parametrize("name", ["paxos9", "wpaxos_w8", "wpaxos_ema_w16", "kpaxos", "abd", "epaxos"])
def test_protocols(name):
    core_property(name)


# ---- shape 5: compaction -------------------------------------------------------------------------
def test_compaction_maps_travel_and_inject_wakes():
    name = "dying"
    cid = 1 << 20

    def run(restored):
        g = make(name)
        g.step(T1)
        if restored:
            blob = g.snapshot()
            g.close()
            g = make(name)
            g.restore(blob)
        n = g.cfg.clusters
        assert g.active_clusters() < n
        frozen = [c for c, f in enumerate(g.activity()) if f is not None]
        mid = readout(g)
        g.inject(frozen[0], 2, cid)
        g.inject(frozen[-1], 0, cid + 1)
        g.step(T2)
        end = readout(g)
        g.close()
        return mid, end, frozen

    a_mid, a_end, frozen = run(False)
    b_mid, b_end, _ = run(True)
    same(a_mid, b_mid, "dying right after the restore")
    same(a_end, b_end, "dying after the inject")
    # the maps are exercised: activity reports a cluster frozen only when its slot is at or past the
    # bound (= active_clusters, one pool), so a frozen cluster whose id is below the bound has left
    # its original slot
    assert any(c < a_mid["active"] for c in frozen), "some frozen cluster was swapped out of its slot"
    o = make(name, cls=ol.OracleSim)
    o.step(T1)
    o.inject(frozen[0], 2, cid)
    o.inject(frozen[-1], 0, cid + 1)
    o.step(T2)
    oc = core(o)
    same({k: a_end[k] for k in oc}, oc, "dying against the oracle")


# ---- shape 6: a full bucket ----------------------------------------------------------------------
def test_full_bucket_and_overflow():
    o = make("overflow", cls=ol.OracleSim)
    o.step(T1)
    st = o.read_state()
    assert any(s.flags & abi.F_MBOX_OVF for s in st), "some cluster overflowed a bucket before T1"
    M = o.cfg.mbox_cap
    full = 0
    for c in range(o.cfg.clusters):
        for r in range(o.N):
            by_src = {}
            for rec in o.read_inbox(c, r):
                by_src[rec[0]] = by_src.get(rec[0], 0) + 1
            full += sum(1 for v in by_src.values() if v == M)
    assert full > 0, "a box holds exactly M records at T1"
    o.close()
    core_property("overflow")


# ---- shape 7: pending inject and deliver -----------------------------------------------------------
def test_pending_inject_and_deliver():
    name = "paxos5"
    p1b = [(1, 2 | (1 << 8), (2 << 4) | 1, 0, 0), (1, 0, (1 << 4) | 0, 5, 77)]   # a P1b header and one log record

    def put(s):
        s.deliver(3, 0, 1, p1b)
        s.inject(64, 2, 1 << 21)

    a = make(name)
    a.step(T1)
    put(a)
    a_in = inboxes(a)
    a.step(T2)
    a_end = readout(a)
    a.close()
    b = make(name)
    b.step(T1)
    put(b)
    blob = b.snapshot()
    b.close()
    f = make(name)
    f.restore(blob)
    b_in = inboxes(f)
    assert b_in == a_in
    assert any(r[0] == 1 and r[4] == 77 for r in b_in[3 * 5 + 0]) and any(r[4] == 1 << 21 for r in b_in[64 * 5 + 2])
    f.step(T2)
    same(a_end, readout(f), "pending inject and deliver")
    f.close()


# ---- shape 8: stale records and rewind ------------------------------------------------------------
def test_rewind_over_stale_records():
    name = "paxos5"
    _, a_end = run_a(name)
    c = make(name)
    c.step(T1)
    blob = c.snapshot()
    c.step(T2 + 13)                 # dead rec slots now hold later records
    c.restore(blob)
    c.step(T2)
    same(a_end, readout(c), "rewound handle")
    c.close()


# ---- the exact count -------------------------------------------------------------------------------
def test_exact_live_record_count():
    g = make("delay0")
    g.step(T1)
    total = sum(len(x) for x in inboxes(g))
    size = g.snapshot_size()
    blob = g.snapshot()
    i = snapshot.info(blob)
    assert total > 0 and i["mailbox_records"] == total
    assert len(blob) == size
    assert i["sections"]["mailbox"] == 16 * total
    g.close()


# ---- fork --------------------------------------------------------------------------------------------
def test_fork():
    name = "paxos5"
    _, a_end = run_a(name)
    p = make(name)
    p.step(T1)
    f = p.fork()
    f._rec = p._rec
    assert f.kernel_time() == (0.0, 0)
    p.step(T2)
    f.step(T2)
    same(a_end, readout(p), "parent")
    same(a_end, readout(f), "fork")
    p.close()
    f.close()
    # a what-if on the fork only; the parent goes first
    crash = abi.make_fault(abi.FAULT_CRASH, 2, step_from=T1 + 5)
    p = make(name)
    p.step(T1)
    f = p.fork()
    f._rec = p._rec
    f.fault(crash)
    p.step(T2)
    same(a_end, readout(p), "parent beside a forked what-if")
    p.close()
    f.step(T2)
    got = core(f)
    f.close()
    o = make(name, cls=ol.OracleSim, faults=SHAPES[name]()[3] + (crash,))
    o.step(T1 + T2)
    same(got, core(o), "fork with a crash against the oracle")
    o.close()


# ---- every recorder at once --------------------------------------------------------------------------
def test_all_four_recorders_through_restore_and_fork():
    """Latency, client history, multiversion and trace on one handle: the one list of recorder buffers
    (snapshot_plan.h) carries all eight through snapshot -> restore and through fork.  48 steps, then
    48 more; the restored and the forked handle equal the one stepped straight through in every
    readout, the traced rows and the device bytes included."""
    traced, steps = (3, 64), 48

    def new():
        s = make("paxos5", recorders=dict(lat=16, chist=8, mv=4))
        s.trace_enable(traced, 32)
        return s

    def out(s):
        d = readout(s)
        d["trace"] = [s.trace_read(c, r) for c in traced for r in range(s.N)]
        d["trace_totals"] = s.trace_totals()
        d["device_bytes"] = s.device_bytes()
        return d

    a = new()
    a.step(2 * steps)
    want = out(a)
    a.close()
    # every recorder has recorded something
    assert want["trace_totals"][0] > 0 and want["lat"][1] > 0 and want["consensus"][1] > 0
    assert any(ops for ops, _ in want["chist"])

    b = new()
    b.step(steps)
    blob = b.snapshot()
    f = b.fork()
    f._rec = b._rec
    b.close()
    assert snapshot.info(blob)["recorders"] == {"latency": True, "client_history": True, "multiversion": True, "trace": True}
    r = new()
    r.restore(blob)
    for s, ctx in ((r, "restored"), (f, "forked")):
        s.step(steps)
        same(want, out(s), f"all four recorders, {ctx}")
        s.close()


# ---- rewind and trace --------------------------------------------------------------------------------
def test_rewind_and_trace():
    cfg, wl, fp, faults = trace_ref.paxos_case()
    traced = trace_ref.TILE_EDGE
    S = _sim()
    src = S(cfg, wl, fp, faults)
    src.latency_enable(64)
    src.step(T1)
    blob = src.snapshot()
    src.close()
    full = S(cfg, wl, fp, faults)
    full.latency_enable(64)
    full.trace_enable(traced, 4096)
    full.step(T1 + T2)
    g = S(cfg, wl, fp, faults)
    g.latency_enable(64)
    g.trace_enable(traced, 4096)
    g.restore(blob)
    g.step(T2)
    o = ol.OracleSim(cfg, wl, fp, faults)
    o.step(T1)
    ref = trace_ref.capture_many(o, traced, [T2], clients=False)
    for c in traced:
        want = trace_ref.rows_of(ref.msgs[c], 5)
        for r in range(5):
            rows, dropped = g.trace_read(c, r)
            whole, _ = full.trace_read(c, r)
            assert dropped == 0 and rows == [x for x in whole if x[0] >= T1], (c, r)
            assert rows == want[r], (c, r)
    # a blob with a trace does not go into a handle without one, nor into one with other clusters
    tb = g.snapshot()
    assert snapshot.info(tb)["recorders"]["trace"]
    plain = S(cfg, wl, fp, faults)
    plain.latency_enable(64)
    with pytest.raises(_err(), match="the snapshot carries a trace, the handle has none"):
        plain.restore(tb)
    other = S(cfg, wl, fp, faults)
    other.latency_enable(64)
    other.trace_enable((1, 2, 3, 4, 5, 6), 4096)
    with pytest.raises(_err(), match="the traced clusters"):
        other.restore(tb)
    full.restore(tb)                      # alike on both sides: the rows are carried
    assert full.trace_read(64, 0) == g.trace_read(64, 0)
    for s in (g, full, plain, other):
        s.close()


# ---- refusals ----------------------------------------------------------------------------------------
def test_refusals():
    import ctypes as C
    from paxi_amd.sim import load_library
    name = "paxos5"
    g = make(name)
    g.step(T1)
    blob = g.snapshot()
    L = load_library()
    n = C.c_uint64()
    small = np.full(len(blob), 0xAB, dtype=np.uint8)
    assert L.paxisim_snapshot(g.h, small.ctypes.data_as(C.c_void_p), len(blob) - 1, C.byref(n)) == -5   # PAXISIM_ERANGE
    assert (small == 0xAB).all(), "nothing is written when cap is too small"
    assert L.paxisim_snapshot(g.h, None, 0, None) == -1 and L.paxisim_restore(g.h, None, 0) == -1
    assert L.paxisim_restore(None, blob.ctypes.data_as(C.c_void_p), len(blob)) == -1
    assert L.paxisim_fork(g.h, None) == -1 and L.paxisim_snapshot_size(None, C.byref(n)) == -1
    g.close()

    cfg, wl, fp, faults, rec = SHAPES[name]()

    def target(recorders=rec, **cfg_kw):
        c = abi.make_config(**{**dict(npz=[5], clusters=130, seed=11, window=16, mbox_cap=32, max_delay=4, kv=1), **cfg_kw})
        s = _sim()(c, wl, fp, faults)
        if recorders.get("lat"):
            s.latency_enable(recorders["lat"])
        if recorders.get("chist"):
            s.client_history_enable(recorders["chist"])
        if recorders.get("mv"):
            s.multiversion_enable(recorders["mv"])
        return s

    cases = [(target({}), "snapshot recorders differ: latency bins"),
             (target(dict(lat=128, chist=16, mv=16)), r"latency bins \(snapshot 64, handle 128\)"),
             (target(dict(lat=64, chist=8, mv=16)), "client history ops_per_worker"),
             (target(seed=12), r"snapshot plan differs: config\.seed \(snapshot 11, handle 12\)"),
             (target(clusters=131), r"snapshot plan differs: config\.clusters"),
             (target(window=32), r"snapshot plan differs: config\.window"),
             (target(), "snapshot truncated")]
    for s, msg in cases:
        s.step(5)
        before = [x.as_tuple() for x in s.read_state()]
        with pytest.raises(_err(), match=msg):
            s.restore(blob[:-16] if msg == "snapshot truncated" else blob)
        if msg == "snapshot truncated":
            with pytest.raises(_err(), match=msg):
                s.restore(blob[:0])                         # an empty buffer
        assert [x.as_tuple() for x in s.read_state()] == before and s.stats().steps == 5, msg
        s.close()
    bad = blob.copy()
    bad[0] ^= 1
    s = target()
    with pytest.raises(_err(), match="bad magic"):
        s.restore(bad)
    s.close()
