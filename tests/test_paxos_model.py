"""The Multi-Paxos oracle against the map-based model of tests/paxos_model.py:
traces of the oracle replayed through replicas that keep unbounded maps, at shapes where the window
of W slots wraps and overflows, where ghosts are re-created below `execute`, where requests are
forwarded and replies routed back, where leaders change and P1bs carry payload, and where Go
panics.  Every traced cluster carries exactly its pinned flag word; none is skipped."""
import collections

import pytest

import gtrace_lib
import oracle_lib as ol
import paxos_model as pm
import trace_ref

_runs = {}


def run(name):
    """The oracle's run of a shape, traced at its pinned clusters and replayed: once per process."""
    if name not in _runs:
        sh = pm.SHAPES[name]()
        o = ol.OracleSim(sh.cfg, sh.wl, sh.fp, sh.faults)
        ref = trace_ref.capture_many(o, list(sh.traced), [sh.steps], clients=False)
        assert pm.flag_counts(o) == pm.FLAG_COUNTS[name]
        _runs[name] = (sh, ref, {c: pm.replay_cluster(o, sh, c, ref.msgs[c]) for c in sh.traced})
        o.close()
    return _runs[name]


@pytest.mark.parametrize("name", list(pm.SHAPES))
def test_oracle_against_model(name):
    sh, ref, res = run(name)
    assert {c: word for c, (_, word) in res.items()} == sh.traced
    assert sum(rp.matched for rp, _ in res.values()) > 500
    assert {c: rp.panics[0][0] for c, (rp, _) in res.items() if rp.panics} == ref.poisoned


def test_every_flag_class_is_traced():
    words = collections.Counter(w for mk in pm.SHAPES.values() for w in mk().traced.values())
    assert not any(w & pm.OUTSIDE for w in words)
    assert all(words[w] for w in (0, pm.WOVF, pm.GHOST, pm.WOVF | pm.GHOST)) and any(w & pm.POISON for w in words)


def test_every_message_type_is_delivered():
    seen = collections.Counter()
    for name in pm.SHAPES:
        for rp, _ in run(name)[2].values():
            seen.update(rp.delivered)
    for t in pm.SOCKET_TYPES + (pm.T_P1B_ENTRY,):          # T_REQUEST: forwarded ones, off the socket
        assert seen[t] > 0, f"message type {t}"


@pytest.mark.parametrize("name", pm.WRAPS)
def test_the_window_wraps(name):
    sh, _, res = run(name)
    for c, (rp, _) in res.items():
        assert max(m.paxos.slot for m in rp.replicas) >= 4 * sh.cfg.window, f"cluster {c}"
    if name == "wrap":
        assert max(m.paxos.slot for rp, _ in res.values() for m in rp.replicas) >= 34 * sh.cfg.window
        assert any(m.paxos.execute == 0 for rp, _ in res.values() for m in rp.replicas)


@pytest.mark.parametrize("name", pm.OUT_OF_WINDOW)
def test_entries_outside_the_window(name):
    """The model creates entries below execute and at or above execute + W, and keeps some to the
    end: the one-directional WOVF / GHOST checks of check_end are not vacuous."""
    _, _, res = run(name)
    reps = [m.paxos for rp, _ in res.values() for m in rp.replicas]
    assert sum(p.below for p in reps) > 0 and sum(p.above for p in reps) > 0
    assert any(s < p.execute for p in reps for s in p.log)


@pytest.mark.parametrize("name", ["ephemeral", "flaky", "rwc_ephemeral"])
def test_both_panics(name):
    """The nil-quorum ACK (ephemeral, flaky) and the nil request under ReplyWhenCommit."""
    sh, ref, res = run(name)
    assert sum(1 for rp, _ in res.values() if rp.panics) >= 2
    for c, (rp, _) in res.items():
        assert len(rp.panics) <= 1 or len({t for t, _ in rp.panics}) == 1, f"cluster {c}"


def test_injected_requests():
    """Client requests handed to non-leaders mid-run (paxisim_inject) are inputs of the replay."""
    sh, inj = pm.inject_case()
    o = ol.OracleSim(sh.cfg, sh.wl, sh.fp)
    before = {t: (lambda s, t=t: [s.inject(c, r, cid) for (t2, c, r, cid) in inj if t2 == t])
              for t in {i[0] for i in inj}}
    ref = trace_ref.capture_many(o, list(sh.traced), [sh.steps], before=before, clients=False)
    got = {}
    for c in sh.traced:
        rp, got[c] = pm.replay_cluster(o, sh, c, ref.msgs[c], {(t, r, cid) for (t, c2, r, cid) in inj if c2 == c})
        assert sum(m.client_requests for m in rp.replicas) > 12
        assert sum(len(m.forwards) for m in rp.replicas) > 0
    assert got == sh.traced


def test_a_p2b_for_a_committed_ghost_is_ignored():
    """The commit bit of a ghost.  No seeded run of the shapes reaches it: a P2b
    for an executed slot whose entry a P3 re-created.  A transport that hands both in does."""
    sh, deliveries = pm.committed_ghost_case()
    o = ol.OracleSim(sh.cfg, sh.wl)
    before = {t: (lambda s, a=a: s.deliver(*a)) for t, a in deliveries.items()}
    ref = trace_ref.capture_many(o, [0], [sh.steps], before=before, clients=False)
    seen = {(t, src, dst, tuple(recs[0][1:])) for t, (_, dst, src, recs) in deliveries.items()}
    rp, word = pm.replay_cluster(o, sh, 0, ref.msgs[0], delivered_in=seen)
    a = rp.replicas[0].paxos
    assert word == sh.traced[0] and sum(rp.delivered.values()) == rp.matched + 2
    assert a.log[0].commit and a.log[0].ballot == 0 and a.execute == 3
    assert (a.ballot, a.active) == ((1 << 4) | 0, True)


GTRACES = {tr["name"]: tr for tr in gtrace_lib.GTRACES if not tr.get("seed_dependent")}


@pytest.mark.parametrize("seed", [1, 42])
@pytest.mark.parametrize("name", list(GTRACES))
def test_hand_derived_traces(name, seed):
    """G1-G14, the scripted one-cluster scenarios whose answers were derived by hand from the Go
    source: the model executes what they say each replica executes."""
    tr = GTRACES[name]
    cfg, wl, faults = gtrace_lib.build(tr, seed)
    o = ol.OracleSim(cfg, wl, None, faults)
    before = {t: (lambda s, t=t: [s.inject(0, r, cid) for (t2, r, cid) in tr["inject"] if t2 == t])
              for t in {i[0] for i in tr["inject"]}}
    ref = trace_ref.capture_many(o, [0], [tr["steps"]], before=before, clients=False)
    sh = pm.Shape(cfg, wl, None, tuple(faults), tr["steps"], False, {})
    rp, _ = pm.replay_cluster(o, sh, 0, ref.msgs[0], {(t, r, cid) for (t, r, cid) in tr["inject"]})
    assert [m.paxos.order for m in rp.replicas] == [e["executed"] for e in tr["expect"]]
