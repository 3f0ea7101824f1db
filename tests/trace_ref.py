"""Expected device message traces, derived from the CPU oracle as it stands.

The device trace of replica dst of a traced cluster is what its inbox holds when its step t begins.
`capture_many` therefore steps an oracle handle one step at a time and, before each step, reads
read_inbox of every (traced cluster, replica), exactly as paxi_amd.trace.capture does for one
cluster - the same grouping by source, the same synthesized request of a worker that starts at this
step (it enters the inbox during the step, behind what is queued), the same split into messages.  A
cluster's trace ends with the step at which any of its replicas first shows PAXISIM_F_POISON: the
cluster is frozen from the next step on.

The same loop watches read_client of every cluster, as latency_ref and client_history_ref do, so a
shape's yardstick also holds the latency samples and the client histories of the run.

The shapes are module-level builders shared by the CPU and GPU suites (the parameters of
tests/test_trace.py's cases); seeds, steps and the late worker's start step were chosen on the CPU
so that the self-checks of tests/test_trace_device.py hold.
"""
import collections

import oracle_lib
from paxi_amd import abi, trace

# msgs: {cluster: [(step, src, dst, [records])]} in capture's order; samples: {worker: [(reply step,
# latency)]} over every cluster; hist: {cluster: [worker] -> ops}; poisoned: {cluster: step}
Ref = collections.namedtuple("Ref", "msgs states stats samples hist poisoned steps")


def capture_many(osim, clusters, steps_list, before=None, clients=True):
    """Step `osim` sum(steps_list) steps, one at a time, tracing `clusters`.  before: {step: fn(osim)}
    called before the inboxes of that step are read (an inject or a deliver between two step()
    calls of the run under test)."""
    N, wl, cfg = osim.N, osim.wl, osim.cfg
    before = before or {}
    t0 = osim.stats().steps
    msgs = {c: [] for c in clusters}
    poisoned = {}
    workers = range(wl.outstanding)
    watch = range(cfg.clusters) if clients else ()
    prev = {c: [s[:2] for s in osim.read_client(c)] for c in watch}
    issued_at = {c: [wl.start_step[w] for w in workers] for c in watch}
    samples = {w: [] for w in workers}
    hist = {c: [[] for _ in workers] for c in watch}
    for k in range(sum(steps_list)):
        t = t0 + k
        if t in before:
            before[t](osim)
        for c in clusters:
            if c in poisoned:
                continue
            for dst in range(N):
                by_src = {}
                for r in osim.read_inbox(c, dst):
                    by_src.setdefault(r[0], []).append(r)
                for w in workers:
                    if t > 0 and wl.start_step[w] == t and wl.target[w] == dst:
                        by_src.setdefault(N, []).append((N, trace.T_REQUEST, 0, 0, 1 + w))
                for src in sorted(by_src):
                    for m in trace._split(by_src[src]):
                        msgs[c].append((t, src, dst, m))
        osim.step(1)
        for c in clusters:
            if c not in poisoned and any(s.flags & abi.F_POISON for s in osim.read_state(c, 1)):
                poisoned[c] = t
        for c in watch:
            full = osim.read_client(c)
            now = [s[:2] for s in full]
            for w in workers:
                if now[w] != prev[c][w]:
                    cid = prev[c][w][0]
                    if cid != 0:
                        samples[w].append((t, t - issued_at[c][w]))
                        key, is_write = osim.command(c, cid)
                        key = min(key, cfg.keys - 1)
                        hist[c][w].append((key, int(is_write), cid if is_write else full[w][2], issued_at[c][w], t))
                    issued_at[c][w] = t
            prev[c] = now
    states = [s.as_tuple() for s in osim.read_state()]
    return Ref(msgs, states, osim.stats().as_dict(), samples, hist, poisoned, sum(steps_list))


def rows_of(msgs, N):
    """The recorder's rows of one cluster's yardstick: per replica dst, [(step, src, hdr, ballot,
    slot, cid)] in step, source and FIFO order."""
    rows = [[] for _ in range(N)]
    for (t, src, dst, recs) in msgs:
        for r in recs:
            rows[dst].append((t,) + tuple(r))
    return rows


# ---- the shapes --------------------------------------------------------------------------------
CHUNKS = (1, 17, 64, 38)            # 120 steps in four step() calls
TILE_EDGE = (0, 63, 64, 65, 128, 129)


def paxos_case(clusters=130, base=0, fp=True, **cfg_kw):
    """Multi-Paxos N=5, random Drop/Slow; workers on replicas 0, 0, 1, 2: replicas 1 and 2 forward."""
    cfg = abi.make_config(npz=[5], clusters=clusters, cluster_base=base, seed=11, window=16, mbox_cap=16,
                          max_delay=3, kv=1, **cfg_kw)
    wl = abi.make_workload(outstanding=4, target=[0, 0, 1, 2], write_ppm=600_000, keys=8)
    f = abi.make_fault_process(drop_ppm=8000, drop_len=10, slow_ppm=8000, slow_len=10, slow_min=1,
                               slow_max=3) if fp else None
    return cfg, wl, f, ()


def paxos_pools_case():
    """The smallest shape with which tests/test_pools_gpu.py gets two pools: 512 + 64 + 5 clusters."""
    return paxos_case(clusters=512 + 64 + 5, steps_per_launch=20)


POOLS_TRACED = TILE_EDGE + (511, 512, 575, 576, 580)

# Replica 0 - the first leader - is crashed over [CRASH_FROM, CRASH_TO): it discards what it
# receives.  Worker 1 sits on replica 1, which under ephemeral_leader runs phase 1 itself and
# collects P1bs with the followers' uncommitted entries; worker 2 starts late on replica 1, at a
# step at which worker 1's next request is already queued there (chosen on the CPU, asserted in
# tests/test_trace_device.py).
CRASH_FROM, CRASH_TO, LATE_AT = 30, 80, 47


def crash_case(clusters=70, base=0, late_at=LATE_AT):
    cfg = abi.make_config(npz=[5], clusters=clusters, cluster_base=base, seed=11, window=16, mbox_cap=16,
                          max_delay=3, kv=1, ephemeral_leader=1)
    wl = abi.make_workload(outstanding=3, target=[0, 1, 1], start_step=[0, 0, late_at], write_ppm=600_000, keys=8)
    fp = abi.make_fault_process(drop_ppm=4000, drop_len=10, slow_ppm=8000, slow_len=10, slow_min=1, slow_max=3)
    return cfg, wl, fp, (abi.make_fault(abi.FAULT_CRASH, 0, step_from=CRASH_FROM, step_to=CRASH_TO),)


CRASH_TRACED = (62, 63, 64, 65)


def wpaxos_case(clusters=70, base=0):
    """WPaxos 3x3 at W = 8: the co-located instance blocks, the 9-replica unit."""
    cfg = abi.make_config(protocol=abi.WPAXOS, npz=[3, 3, 3], keys=6, fz=0, adaptive=1, policy_threshold=2,
                          clusters=clusters, cluster_base=base, seed=5, window=8, mbox_cap=24, max_delay=0)
    wl = abi.make_workload(outstanding=9, target=list(range(9)), locality_ppm=700_000, write_ppm=500_000,
                           key_min=1000)
    return cfg, wl, None, ()


def abd_case(clusters=70, base=0):
    cfg = abi.make_config(protocol=abi.ABD, npz=[5], clusters=clusters, cluster_base=base, seed=3, keys=4,
                          mbox_cap=16, max_delay=2, history=64)
    wl = abi.make_workload(outstanding=3, target=[0, 1, 2], write_ppm=500_000)
    return cfg, wl, None, ()


def perkey_case(proto):
    def mk(clusters=70, base=0):
        cfg = abi.make_config(protocol=proto, npz=[3, 3, 3], keys=16, clusters=clusters, cluster_base=base,
                              seed=9, window=16, mbox_cap=24, max_delay=0)
        wl = abi.make_workload(outstanding=9, target=list(range(9)), locality_ppm=700_000, key_min=192,
                               write_ppm=500_000)
        return cfg, wl, None, ()
    return mk


def epaxos_case(clusters=70, base=0):
    cfg = abi.make_config(protocol=abi.EPAXOS, npz=[2, 2, 1], clusters=clusters, cluster_base=base, seed=11, keys=4,
                          window=32, mbox_cap=32, max_delay=2, kv=1)
    wl = abi.make_workload(outstanding=5, target=list(range(5)), write_ppm=700_000)
    fp = abi.make_fault_process(drop_ppm=1500, drop_len=10, slow_ppm=3000, slow_len=20, slow_min=1, slow_max=2)
    return cfg, wl, fp, ()


CASES = {"paxos": paxos_case, "wpaxos": wpaxos_case, "abd": abd_case, "m2paxos": perkey_case(abi.M2PAXOS),
         "kpaxos": perkey_case(abi.KPAXOS), "epaxos": epaxos_case, "crash": crash_case, "pools": paxos_pools_case}
PROTO_TRACED = (62, 63, 64, 65)
PROTO_STEPS = (100,)

_refs = {}


def ref(name, traced, chunks):
    """The yardstick of a shape traced at `traced` over the step() calls `chunks`: once per process."""
    key = (name, tuple(traced), tuple(chunks))
    if key not in _refs:
        cfg, wl, fp, faults = CASES[name]()
        o = oracle_lib.OracleSim(cfg, wl, fp, faults)
        _refs[key] = capture_many(o, list(traced), list(chunks))
        o.close()
    return _refs[key]
