"""The exists bits and the "has request state" bit of a packed Multi-Paxos
window: a follower's HandleP2a on a fresh slot and HandleP3
at a replica that never held a request or a quorum object decide from bits
kept in registers, without loading the 16-B entry.

Nothing a caller can see changes, so every case runs against the CPU oracle:
replica states and totals (assert_same) and the held window of every replica
of the first 64 clusters (read_log), with the helpers of
test_packed_window_gpu.  Each case first checks on the oracle alone that its
inputs reach the path it is there for."""
import pytest

from paxi_amd import abi
import oracle_lib as ol
from test_parity_gpu import assert_same
from test_packed_window_gpu import (_assert_windows, _case1, _oracle1, _run, _windows, WOVF, UNFAITHFUL)

pytestmark = pytest.mark.gpu

CASE1_FAULTS = dict(drop_ppm=5000, drop_len=20, slow_ppm=5000, slow_len=20, slow_min=1, slow_max=4)


def _early_commits(o, cfg):
    """Follower entries that exist, are committed and have ballot 0: a P3 that
    arrived before its P2a created them (&entry{}, G6)."""
    N = abi.n_replicas(cfg)
    states = o.read_state()
    n = 0
    for c in range(cfg.clusters):
        for r in range(1, N):
            for e in o.read_log(c, r, states[c * N + r].execute, cfg.window):
                n += (e.flags & abi.LOG_EXISTS) and (e.flags & abi.LOG_COMMIT) and e.ballot == 0
    return n


# ---------------------------------------------------------------------------
# 1: the config-2 shape; 9: the same on the plane kernel, which shares the rows
# ---------------------------------------------------------------------------
def test_config2_shape():
    cfg, wl, fp = _case1()
    o = ol.OracleSim(cfg, wl, fp)
    found, at = 0, 0
    for t in (30, 60, 190):                 # P3 before P2a: the blind P3 creates an entry, a later P2a finds it
        o.step(t - at)
        at = t
        found += _early_commits(o, cfg)
    assert found > 0, "no follower entry committed before its P2a at steps 30, 60, 190"
    _run(cfg, wl, fp, (), (200, 200), _oracle1(), "config-2 shape")


def test_plane_kernel_shares_the_rows(monkeypatch):
    monkeypatch.setenv("PAXISIM_SERIAL", "0")
    cfg, wl, fp = _case1()
    _run(cfg, wl, fp, (), (200, 200), _oracle1(), "PAXISIM_SERIAL=0")


# ---------------------------------------------------------------------------
# 2: W = 8 - both halves of the mask wrap with the ring
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("npz", [[3], [5]])
def test_ring_wrap(npz):
    cfg = abi.make_config(npz=npz, clusters=192, seed=32, window=8, mbox_cap=8, max_delay=6, kv=1)
    wl = abi.make_workload(outstanding=8, target=0)
    fp = abi.make_fault_process(drop_ppm=5000, drop_len=40, slow_ppm=8000, slow_len=30, slow_min=2, slow_max=6)
    o = ol.OracleSim(cfg, wl, fp)
    o.step(400)
    st = o.stats().as_dict()
    assert st["flagged"][WOVF] > 0 and st["flagged"][UNFAITHFUL] > 0, st
    _run(cfg, wl, fp, (), (400,), o, f"ring wrap npz={npz}")


# ---------------------------------------------------------------------------
# 3: forwarded requests - non-leaders hold request state from the start;
# 8: the forwards count shares its row with the exists bits, so every reader masks it
# ---------------------------------------------------------------------------
def test_request_state_from_the_start():
    cfg = abi.make_config(npz=[5], clusters=128, seed=21, window=16, kv=1)
    wl = abi.make_workload(outstanding=5, target=[0, 1, 2, 3, 4])
    fp = abi.make_fault_process(drop_ppm=2000, drop_len=15, slow_ppm=2000, slow_len=15, slow_min=1, slow_max=4)
    o = ol.OracleSim(cfg, wl, fp)
    o.step(300)
    st = o.stats().as_dict()
    assert st["delivered"]["Request"] > 0 and st["delivered"]["Reply"] > 0, st
    g, _ = _run(cfg, wl, fp, (), (150, 150), o, "forwarded requests")
    # every read_state field, once more by name: a reader that took the raw row would differ here
    assert [s.as_tuple() for s in g.read_state()] == [s.as_tuple() for s in o.read_state()]
    assert [s.as_tuple() for s in g.read_instances(0, 64)] == [s.as_tuple() for s in o.read_instances(0, 64)]


# ---------------------------------------------------------------------------
# 4: a follower starts to lead mid-run: its request-state bit turns on at step 60
# ---------------------------------------------------------------------------
def test_request_state_mid_run():
    cfg = abi.make_config(npz=[5], clusters=128, seed=5, ephemeral_leader=1, window=16, mbox_cap=24, kv=1)
    wl = abi.make_workload(outstanding=8, target=[0, 0, 0, 0, 3, 3, 3, 3], start_step=[0, 0, 0, 0, 60, 60, 60, 60])
    faults = [abi.make_fault(abi.FAULT_CRASH, 0, step_from=60)]
    o = ol.OracleSim(cfg, wl, None, faults)
    o.step(60)
    before = o.stats().as_dict()["commits"]
    o.step(240)
    st = o.stats().as_dict()
    assert st["discarded"] > 0 and st["commits"] > before > 0, st
    _run(cfg, wl, None, faults, (40, 40, 220), o, "leader change at step 60")


# ---------------------------------------------------------------------------
# 5: the any-N unit; 6: W > 16 reads the entry as before
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("npz,window", [([7], 16), ([5], 64)])
def test_other_units_and_fallback(npz, window):
    cfg = abi.make_config(npz=npz, clusters=128, seed=31, window=window, mbox_cap=32, max_delay=4, kv=1)
    wl = abi.make_workload(outstanding=8, target=0)
    fp = abi.make_fault_process(**CASE1_FAULTS)
    o = ol.OracleSim(cfg, wl, fp)
    o.step(300)
    st = o.stats().as_dict()
    assert st["commits"] > 0 and st["dropped"] > 0 and st["delivered"]["P3"] > 0, st
    _run(cfg, wl, fp, (), (150, 150), o, f"npz={npz} W={window}")


# ---------------------------------------------------------------------------
# 7: the bits travel with the cluster through compaction and the wake path
# ---------------------------------------------------------------------------
def test_bits_travel_with_the_cluster(monkeypatch):
    cfg, wl, fp = _case1()
    chunks = (60, 60, 60, 60, 60, 100)
    g1, _ = _run(cfg, wl, fp, (), chunks, _oracle1(), "compaction on")
    assert g1.active_clusters() < cfg.clusters      # clusters were frozen: slots have been swapped
    monkeypatch.setenv("PAXISIM_COMPACT", "0")
    g0, _ = _run(cfg, wl, fp, (), chunks, _oracle1(), "compaction off")
    monkeypatch.delenv("PAXISIM_COMPACT")
    assert [s.as_tuple() for s in g1.read_state()] == [s.as_tuple() for s in g0.read_state()]
    assert _windows(g1, cfg) == _windows(g0, cfg)
    # one request into a frozen cluster: its rows and window come back as they were frozen
    frozen = [c for c, t in enumerate(g1.activity()) if t is not None]
    assert frozen, "no frozen cluster to wake"
    o = ol.OracleSim(cfg, wl, fp)                   # (the shared oracle stays as it is)
    o.step(sum(chunks))
    g1.inject(frozen[0], 0, 1 << 22)
    o.inject(frozen[0], 0, 1 << 22)
    g1.step(60)
    o.step(60)
    assert_same(g1, o, "woken")
    _assert_windows(g1, o, cfg, "woken")
