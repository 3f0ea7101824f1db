"""The WPaxos, M2Paxos and KPaxos kernels against the map-based model of tests/wpaxos_model.py
(DESIGN.md §3.5g): the recording build's own trace of the pinned clusters of a shape, replayed
through replicas that keep `map[Key]*kpaxos` as a dict and policy.go on plain Python state, and the
end of the run - read_instances, read_state, every window by read_log, the flags - checked against
them.  The shapes, their pinned flag words and the coverage assertions are those of
tests/test_wpaxos_model.py."""
import pytest

import paxos_model as pm
import wpaxos_model as wm
from paxi_amd import trace
from paxi_amd.sim import Simulation

pytestmark = pytest.mark.gpu
CAP = 1 << 12                       # records per traced replica; the longest row seen on the oracle is 2075
_runs = {}                          # {shape: its replays} of the default kernel form, once per process


def plan_of(sh):
    """What the ABI shows of a handle's plan (tests/test_create_plan_gpu.py): the LDS bytes per tile,
    the staged picks and the device bytes."""
    with Simulation(sh.cfg, sh.wl, sh.fp, sh.faults) as g:
        return g.occupancy()[1:], g.device_bytes()


def device_against_model(name, chunks=None):
    sh = wm.SHAPES[name]()
    with Simulation(sh.cfg, sh.wl, sh.fp, sh.faults) as g:
        g.latency_enable(64)
        g.trace_enable(list(sh.traced), CAP)
        for n in chunks or (sh.steps,):
            g.step(n)
        assert g.stats().steps == sh.steps
        assert g.trace_totals()[1] == 0
        assert pm.flag_counts(g) == wm.FLAG_COUNTS[name]
        wm.check_traced(sh, g)
        res = {c: wm.replay_cluster(g, sh, c, trace.from_device(g, c)["msgs"]) for c in sh.traced}
    assert {c: word for c, (_, word) in res.items()} == sh.traced
    wm.check_shape(name, sh, res)
    return res


@pytest.mark.parametrize("name", list(wm.SHAPES))
def test_device_trace_against_model(name):
    _runs[name] = device_against_model(name)


def test_every_message_type_is_delivered():
    """Over all shapes, from the device's own traces (a shape that has not run in this process runs now)."""
    wm.check_message_types([_runs[name] if name in _runs else device_against_model(name) for name in wm.SHAPES])


def test_every_flag_class_is_traced():
    wm.check_traced_words()


@pytest.mark.parametrize("name,env", [("wrap8", {"PAXISIM_WCOLOC": "0"}), ("wrap8", {"PAXISIM_WLDS": "1"}),
                                      ("wrap8", {"PAXISIM_SERIAL": "0"}), ("steal", {"PAXISIM_WCOLOC": "1"})],
                         ids=["wrap8-packed", "wrap8-lds", "wrap8-serial0", "steal-coloc"])
def test_kernel_forms_against_model(monkeypatch, name, env):
    """The three homes of the instance scalars and the replica-per-wave kernel: wrap8 (W = 8, the
    co-located block by default) on the packed table, in the tile image's word planes and unserialised; steal (W = 16, the
    packed table by default) on the co-located block.  The knob must change what the ABI shows of
    the plan, or the run would be the default form once more."""
    for k in ("PAXISIM_WCOLOC", "PAXISIM_WLDS", "PAXISIM_SERIAL"):
        monkeypatch.delenv(k, raising=False)
    default = plan_of(wm.SHAPES[name]())
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert plan_of(wm.SHAPES[name]()) != default, f"{env} left the plan as it was: {default}"
    device_against_model(name)


def test_two_unequal_chunks_against_model():
    """steal stepped as 37 + 163: the entry cache is primed at bind time of each launch."""
    device_against_model("steal", chunks=(37, 163))


def test_the_nil_kpaxos_panic():
    """A LeaderChange for a key of which the receiver holds no instance, handed in by a transport
    (tests/test_wpaxos_model.py has the scenario): the device against the model, from its own trace."""
    sh, deliveries = wm.nil_kpaxos_case()
    with Simulation(sh.cfg, sh.wl) as g:
        assert [k for k, _ in g.commands(0, [1, 2, 3])] == [4, 4, 7]
        g.latency_enable(64)
        g.trace_enable([0], 256)
        at = 0
        for t, args in sorted(deliveries.items()):
            g.step(t - at)
            g.deliver(*args)
            at = t
        g.step(sh.steps - at)
        assert g.trace_totals()[1] == 0
        seen = {(t, src, dst, tuple(recs[0][1:])) for t, (_, dst, src, recs) in deliveries.items()}
        rp, word = wm.replay_cluster(g, sh, 0, trace.from_device(g, 0)["msgs"], delivered_in=seen)
    wm.check_nil_kpaxos(rp, word)
