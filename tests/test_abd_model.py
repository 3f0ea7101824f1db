"""The ABD oracle against the map-based model of tests/abd_model.py: traces of the
oracle replayed through replicas that keep abd/replica.go's maps, at shapes where the op ring wraps
and evicts, where majorities are lost for good, where the history overflows, where one partition
outgrows the register checker, and at N = 1, 2 and 7.  Every traced cluster carries exactly its
pinned flag word; none is skipped."""
import pytest

import abd_model as am
import oracle_lib as ol
import paxos_model as pm
import trace_ref
import wpaxos_model as wm

_runs = {}


def run(name):
    """The oracle's run of a shape, traced at its pinned clusters and replayed: once per process."""
    if name not in _runs:
        sh = am.SHAPES[name]()
        o = ol.OracleSim(sh.cfg, sh.wl, sh.fp, sh.faults)
        ref = trace_ref.capture_many(o, list(sh.traced), [sh.steps], clients=False)
        assert pm.flag_counts(o) == am.FLAG_COUNTS[name]
        wm.check_traced(sh, o)
        am.check_out_of_claim(name, o)
        _runs[name] = (sh, {c: am.replay_cluster(o, sh, c, ref.msgs[c]) for c in sh.traced})
        o.close()
    return _runs[name]


@pytest.mark.parametrize("name", list(am.SHAPES))
def test_oracle_against_model(name):
    sh, res = run(name)
    assert {c: word for c, (_, word) in res.items()} == sh.traced
    am.check_shape(name, sh, res)


def test_every_shape_is_pinned():
    assert set(am.FLAG_COUNTS) == set(am.SHAPES)
    for name, mk in am.SHAPES.items():
        sh = mk()
        assert sh.traced and not any(w & am.OUTSIDE for w in sh.traced.values()), name
        assert sum(n for w, n in am.FLAG_COUNTS[name].items() if not w & am.OUTSIDE) >= len(sh.traced), name
        assert len(sh.traced) >= min(4, sum(n for w, n in am.FLAG_COUNTS[name].items() if not w & am.OUTSIDE)), name


def test_a_set_raises_the_version_under_a_coordinator():
    am.check_raised([run(name)[1] for name in am.SHAPES])


def delivered_run(sh, deliveries, make_replica=am.lenient):
    o = ol.OracleSim(sh.cfg, sh.wl)
    before = {t: (lambda s, a=a: s.deliver(*a)) for t, a in deliveries.items()}
    ref = trace_ref.capture_many(o, [0], [sh.steps], before=before, clients=False)
    try:
        return am.replay_cluster(o, sh, 0, ref.msgs[0], delivered_in=am.seen_of(deliveries), make_replica=make_replica)
    finally:
        o.close()


def test_replies_for_a_done_op_whose_ring_slot_was_reused():
    """No seeded shape reaches it: it needs a delay longer than the ring's worth of ops."""
    sh, deliveries = am.reused_slot_case()
    am.check_reused_slot(*delivered_run(sh, deliveries, am.AbdReplica))


def test_a_reply_for_a_cid_never_issued():
    """Go dereferences a nil *entry and panics (abd/replica.go:98-99, 139-140); the oracle returns on
    the tag mismatch and raises nothing: a known difference."""
    sh, deliveries = am.never_issued_case()
    m = am.AbdReplica(0, sh.cfg, pm.Client(sh.wl), None)
    with pytest.raises(pm.Panic):
        m.handle(1, deliveries[11][3][0][1:])
    with pytest.raises(pm.Panic):
        m.handle(2, deliveries[13][3][0][1:])
    with pytest.raises(AssertionError, match="goes on after the panic"):      # the model's process died at step 11
        delivered_run(sh, deliveries, am.AbdReplica)
    rp, word = delivered_run(sh, deliveries)
    assert word == 0 and rp.replicas[0].nil_entries == 2 and rp.replicas[0].cid == 8
    assert sum(rp.delivered.values()) == rp.matched + 2


def test_line_126_lowers_a_version_a_set_had_raised():
    """r.version[m.Key] = e.version (abd/replica.go:126) is no maximum: no seeded shape has a Set
    run two versions ahead of a coordinator's Get majority, a transport that hands one in does."""
    o = ol.OracleSim(*am.scenario_shape()[:2])
    sh, deliveries, j = am.lowered_case(o)
    o.close()
    am.check_lowered(*delivered_run(sh, deliveries), j)


def test_put_ignores_a_nil_value():
    o = ol.OracleSim(*am.scenario_shape()[:2])
    sh, deliveries, j = am.nil_set_case(o)
    o.close()
    am.check_nil_set(*delivered_run(sh, deliveries), j)
