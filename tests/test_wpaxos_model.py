"""The WPaxos, M2Paxos and KPaxos oracle against the map-based model of tests/wpaxos_model.py
(DESIGN.md §3.5g): traces of the oracle replayed through replicas that keep `map[Key]*kpaxos` as a
dict, unbounded logs, one never-cleaned `forwards` per replica and policy.go on plain Python state.
Every traced cluster carries exactly its pinned flag word; none is skipped."""
import pytest

import oracle_lib as ol
import paxos_model as pm
import trace_ref
import wpaxos_model as wm
from paxi_amd import abi

_runs = {}


def run(name):
    """The oracle's run of a shape, traced at its pinned clusters and replayed: once per process."""
    if name not in _runs:
        sh = wm.SHAPES[name]()
        o = ol.OracleSim(sh.cfg, sh.wl, sh.fp, sh.faults)
        ref = trace_ref.capture_many(o, list(sh.traced), [sh.steps], clients=False)
        assert pm.flag_counts(o) == wm.FLAG_COUNTS[name]
        wm.check_traced(sh, o)
        _runs[name] = (sh, ref, {c: wm.replay_cluster(o, sh, c, ref.msgs[c]) for c in sh.traced})
        o.close()
    return _runs[name]


@pytest.mark.parametrize("name", list(wm.SHAPES))
def test_oracle_against_model(name):
    sh, ref, res = run(name)
    assert {c: word for c, (_, word) in res.items()} == sh.traced
    wm.check_shape(name, sh, res)
    assert {c: rp.panics[0][0] for c, (rp, _) in res.items() if rp.panics} == ref.poisoned


def test_shapes_and_traced_clusters():
    """70 clusters at seed 11 (the last wave is partial; gap is its single cluster), and every flag
    class among the pinned words.  That clusters 0, 63, 64 and 69 are traced wherever they are
    inside the claim is held against each run's own flag words (wm.check_traced)."""
    for name, mk in wm.SHAPES.items():
        sh = mk()
        assert name == "gap" or (sh.cfg.clusters, sh.cfg.seed) == (70, 11)
    wm.check_traced_words()


def test_every_message_type_is_delivered():
    wm.check_message_types([run(name)[2] for name in wm.SHAPES])


def test_the_nil_kpaxos_panic():
    """A LeaderChange for a key of which the receiver holds no instance (replica.go:101-104).  No
    seeded shape reaches it (the POISON clusters of nonadaptive are paxos.go:290's), so a transport
    hands it in, after one LeaderChange under a ballot that is not the instance's, one that steals
    a key and one that is not for its receiver."""
    sh, deliveries = wm.nil_kpaxos_case()
    o = ol.OracleSim(sh.cfg, sh.wl)
    assert [k for k, _ in o.commands(0, [1, 2, 3])] == [4, 4, 7]
    before = {t: (lambda s, a=a: s.deliver(*a)) for t, a in deliveries.items()}
    ref = trace_ref.capture_many(o, [0], [sh.steps], before=before, clients=False)
    seen = {(t, src, dst, tuple(recs[0][1:])) for t, (_, dst, src, recs) in deliveries.items()}
    rp, word = wm.replay_cluster(o, sh, 0, ref.msgs[0], delivered_in=seen)
    assert ref.poisoned == {0: 7}
    wm.check_nil_kpaxos(rp, word)
    o.close()
