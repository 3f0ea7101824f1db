"""The ABD kernels against the map-based model of tests/abd_model.py: the
recording build's own trace of the pinned clusters of a shape, replayed through replicas that keep
abd/replica.go's maps, and the end of the run - read_state, read_kv, history, read_client, the flags -
checked against them.  The shapes, their pinned flag words and the coverage assertions are those of
tests/test_abd_model.py."""
import pytest

import abd_model as am
import paxos_model as pm
import wpaxos_model as wm
from paxi_amd import snapshot, trace
from paxi_amd.sim import PaxisimError, Simulation

pytestmark = pytest.mark.gpu
CAP = 1 << 13                       # records per traced replica; the longest row seen on the oracle is 2816
_runs = {}                          # {shape: its replays} of the default kernel form, once per process


def plan_of(sh):
    """What the ABI shows of a handle's plan: the LDS bytes per tile, the staged picks, the device
    bytes, and the plan hash in a snapshot's header, which covers the launch schedule."""
    with Simulation(sh.cfg, sh.wl, sh.fp, sh.faults) as g:
        return g.occupancy()[1:], g.device_bytes(), snapshot.info(g.snapshot())["plan_hash"]


def device_against_model(name, chunks=None):
    sh = am.SHAPES[name]()
    with Simulation(sh.cfg, sh.wl, sh.fp, sh.faults) as g:
        g.latency_enable(64)
        g.trace_enable(list(sh.traced), CAP)
        for n in chunks or (sh.steps,):
            g.step(n)
        assert g.stats().steps == sh.steps
        assert g.trace_totals()[1] == 0
        assert pm.flag_counts(g) == am.FLAG_COUNTS[name]
        wm.check_traced(sh, g)
        am.check_out_of_claim(name, g)
        res = {c: am.replay_cluster(g, sh, c, trace.from_device(g, c)["msgs"]) for c in sh.traced}
    assert {c: word for c, (_, word) in res.items()} == sh.traced
    am.check_shape(name, sh, res)
    return res


@pytest.mark.parametrize("name", list(am.SHAPES))
def test_device_trace_against_model(name):
    _runs[name] = device_against_model(name)


def test_a_set_raises_the_version_under_a_coordinator():
    """Over all shapes, from the device's own traces (a shape that has not run in this process runs now)."""
    am.check_raised([_runs[name] if name in _runs else device_against_model(name) for name in am.SHAPES])


# the replica-per-wave kernel keeps a cluster's whole mailbox image in LDS: zones (N = 7, M = 32, D = 3) needs
# 222,464 B of the 163,840 B, and paxisim_create refuses it; n2 is the generic unit's shape on that kernel
REFUSED = {("zones", "PAXISIM_SERIAL"): "exceeds LDS"}


@pytest.mark.parametrize("env", [{"PAXISIM_SERIAL": "0"}, {"PAXISIM_PIPE": "1"}], ids=["serial0", "pipe1"])
@pytest.mark.parametrize("name", ["n5", "zones", "n2"])
def test_kernel_forms_against_model(monkeypatch, name, env):
    """The replica-per-wave kernel and the unpipelined serial one, on the <5> unit and on the
    generic one.  The knob must change what the ABI shows of the plan, or the run would be the
    default form once more."""
    for k in ("PAXISIM_SERIAL", "PAXISIM_PIPE"):
        monkeypatch.delenv(k, raising=False)
    default = plan_of(am.SHAPES[name]())
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    why = REFUSED.get((name, next(iter(env))))
    if why:
        with pytest.raises(PaxisimError, match=why):
            plan_of(am.SHAPES[name]())
        return
    assert plan_of(am.SHAPES[name]()) != default, f"{env} left the plan as it was: {default}"
    device_against_model(name)


@pytest.mark.parametrize("name", ["n5", "zones"])
def test_two_unequal_chunks_against_model(name):
    device_against_model(name, chunks=(37, 163))


def delivered_run(sh, deliveries, make_replica=am.lenient):
    with Simulation(sh.cfg, sh.wl) as g:
        g.latency_enable(64)
        g.trace_enable([0], 256)
        at = 0
        for t, args in sorted(deliveries.items()):
            g.step(t - at)
            g.deliver(*args)
            at = t
        g.step(sh.steps - at)
        assert g.trace_totals()[1] == 0
        return am.replay_cluster(g, sh, 0, trace.from_device(g, 0)["msgs"], delivered_in=am.seen_of(deliveries),
                                 make_replica=make_replica)


def test_replies_for_a_done_op_whose_ring_slot_was_reused():
    sh, deliveries = am.reused_slot_case()
    am.check_reused_slot(*delivered_run(sh, deliveries, am.AbdReplica))


def test_a_reply_for_a_cid_never_issued():
    """Go panics on the nil *entry; the kernels return on the tag mismatch and raise nothing (the
    known difference of DESIGN.md §3.5h; tests/test_abd_model.py shows the model's Panic)."""
    sh, deliveries = am.never_issued_case()
    rp, word = delivered_run(sh, deliveries)
    assert word == 0 and rp.replicas[0].nil_entries == 2 and rp.replicas[0].cid == 8
    assert sum(rp.delivered.values()) == rp.matched + 2


def test_line_126_lowers_a_version_a_set_had_raised():
    with Simulation(*am.scenario_shape()[:2]) as g:
        sh, deliveries, j = am.lowered_case(g)
    am.check_lowered(*delivered_run(sh, deliveries), j)


def test_put_ignores_a_nil_value():
    with Simulation(*am.scenario_shape()[:2]) as g:
        sh, deliveries, j = am.nil_set_case(g)
    am.check_nil_set(*delivered_run(sh, deliveries), j)
