"""Client request latency recorded on the device (lat_kernel.h)
against the oracle-derived samples of latency_ref: per worker and for all
workers the histogram, count, sum, min, max and overflow are equal bin by bin,
the count is the growth of stats().replies, and the replica states still equal
the oracle's with recording on - in every kernel form and for every protocol."""
import pytest

import latency_ref
from paxi_amd import abi
from paxi_amd.sim import PaxisimError, Simulation

pytestmark = pytest.mark.gpu


def _sim(name, bins):
    cfg, wl, fp, faults = latency_ref.SHAPES[name]()
    g = Simulation(cfg, wl, fp, faults)
    if bins:
        g.latency_enable(bins)
    return g


def _assert_latency(g, r, bins, since=0):
    for w in [None] + list(range(g.wl.outstanding)):
        got, want = g.latency(w), latency_ref.expected(r, bins, w, since)
        print("worker", w, got, "expected", want)
        assert got == want, f"worker {w}: {got} != {want}\n{got.counts}\n{want.counts}"


def _assert_states(g, r):
    assert [s.as_tuple() for s in g.read_state()] == r.states, "replica states differ from the oracle"


def _check(name, bins, schedule=(150, 150)):
    r = latency_ref.ref(name, sum(schedule))
    with _sim(name, bins) as g:
        before = g.stats().replies
        for n in schedule:
            g.step(n)
        _assert_latency(g, r, bins)
        assert g.latency().count == g.stats().replies - before == r.replies
        _assert_states(g, r)
        return g.latency()


@pytest.mark.parametrize("env", [{}, {"PAXISIM_SERIAL": "0"}, {"PAXISIM_PIPE": "1"}],
                         ids=["default", "serial0", "pipe1"])
def test_paxos5_partial_tile_every_kernel_form(monkeypatch, env):
    """130 clusters: two full tiles and a two-lane one, so the wave fold runs with inactive lanes."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h = _check("paxos5", 32)
    assert (h.min, h.max, h.overflow) == (3, 7, 0)


def test_faulted_paxos5_many_keys_per_wave():
    h = _check("paxos5_faulted", 32)
    assert h.max == 29 and h.overflow == 0
    s = h.stat()
    assert (s.exact, s.p95, s.p99) == (1, 12.0, 17.0)


def test_faulted_paxos5_overflow_bin():
    r = latency_ref.ref("paxos5_faulted")
    h = _check("paxos5_faulted", 16)
    whole = latency_ref.expected(r, 32)
    assert h.overflow > 0 and (h.min, h.max, h.sum, h.count) == (whole.min, whole.max, whole.sum, whole.count)
    s = h.stat()
    assert s.exact == 0 and s.p99 == s.max == 29.0 and s.mean == whole.stat().mean


def test_paxos9_idle_skip_with_late_workers():
    _check("paxos9_late", 32)


def test_max_requests_keeps_the_last_sample_and_reset_clears():
    name, bins = "paxos3_max_requests", 32
    r = latency_ref.ref(name)
    cfg, wl, _, _ = latency_ref.SHAPES[name]()
    with _sim(name, bins) as g:
        g.step(150)
        g.step(150)
        _assert_latency(g, r, bins)
        assert g.latency().count == 10 * wl.outstanding * cfg.clusters == g.stats().replies
        _assert_states(g, r)
        g.latency_reset()
        g.step(20)
        empty = g.latency()
        assert (empty.count, empty.sum, empty.overflow, empty.min, empty.max) == (0, 0, 0, 0xFFFFFFFF, 0)
        assert not empty.counts.any()


def test_reset_mid_run_keeps_full_latencies():
    """Samples answered from step 100 on, each with its whole latency (its issue may precede the reset)."""
    r = latency_ref.ref("paxos5")
    with _sim("paxos5", 32) as g:
        g.step(100)
        before = g.stats().replies
        g.latency_reset()
        g.step(200)
        _assert_latency(g, r, 32, since=100)
        assert g.latency().count == g.stats().replies - before
        _assert_states(g, r)
    straddling = [t - lat for w in r.samples for t, lat in r.samples[w] if t >= 100 and t - lat < 100]
    assert straddling, "no request was in flight across the reset"


def test_compaction_moves_the_stamps_with_the_cluster():
    name, bins, schedule = "paxos5_compaction", 32, (75, 75, 75, 75)
    r = latency_ref.ref(name)
    with _sim(name, bins) as g:
        for n in schedule[:3]:
            g.step(n)
        active, replies = g.active_clusters(), g.stats().replies
        assert active < 192, "no cluster was frozen: the row move is not exercised"
        g.step(schedule[3])
        assert g.stats().replies > replies, "no reply after the compaction"
        _assert_latency(g, r, bins)
        assert g.latency().count == g.stats().replies == r.replies
        _assert_states(g, r)


@pytest.mark.parametrize("name", ["abd5", "wpaxos9", "epaxos5"])
def test_other_protocols(name):
    _check(name, 32)


def test_off_path_identity_and_errors():
    r = latency_ref.ref("paxos5")
    with _sim("paxos5", 0) as g:
        with pytest.raises(PaxisimError):
            g.latency()
        with pytest.raises(PaxisimError):
            g.latency_reset()
        for bad in (0, 8, 48, 2 * abi.LAT_MAX_BINS):
            with pytest.raises(PaxisimError):
                g.latency_enable(bad)
        g.step(150)
        g.step(150)
        _assert_states(g, r)
        assert g.stats().replies == r.replies
        with pytest.raises(PaxisimError):
            g.latency_enable(32)                       # only before the first step
        with pytest.raises(PaxisimError):
            g.latency()
    with _sim("paxos5", 32) as g:
        with pytest.raises(PaxisimError):
            g.latency_enable(32)                       # only once
        with pytest.raises(PaxisimError):
            g.latency(3)                               # workers 0..2
        assert g.latency(2).count == 0
