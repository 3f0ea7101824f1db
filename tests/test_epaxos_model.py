"""The EPaxos oracle against the map-based model of tests/epaxos_model.py: traces
of the oracle replayed through replicas that keep unbounded maps, at shapes where the ring of W
entries wraps, where the quorum rules have their edges (N = 2, 4), where the payloads fill every
record (N = 10) and where Drop faults leave gaps that execute() runs over again."""
import pytest

import epaxos_model as em
import oracle_lib as ol
import trace_ref
from paxi_amd import abi
from test_epaxos import ep_cfg

_runs = {}


def run(name):
    """The oracle's run of a shape, traced at em.TRACED and replayed: once per process."""
    if name not in _runs:
        sh = em.SHAPES[name]()
        o = ol.OracleSim(sh.cfg, sh.wl, sh.fp)
        ref = trace_ref.capture_many(o, list(em.TRACED), [sh.steps], clients=False)
        _runs[name] = (sh, o, {c: em.replay_cluster(o, sh, c, ref.msgs[c]) for c in em.TRACED})
    return _runs[name]


@pytest.mark.parametrize("name", list(em.SHAPES))
def test_oracle_against_model(name):
    sh, o, rps = run(name)
    assert sum(rp.matched for rp in rps.values()) > 500
    for c, rp in rps.items():
        assert rp.delivered[em.T_COMMIT] > 0
        assert all(m.replies > 0 for m in rp.replicas), f"cluster {c}"


@pytest.mark.parametrize("name", ["wrap5", "wrap3_1key", "wrap10"])
def test_the_ring_wraps(name):
    sh, o, rps = run(name)
    for c, rp in rps.items():
        for r, m in enumerate(rp.replicas):
            assert m.slot[r] >= 4 * sh.cfg.window, f"cluster {c} replica {r}"


def test_both_paths_at_n10():
    rps = run("wrap10")[2]
    assert sum(rp.delivered[em.T_ACCEPT] for rp in rps.values()) > 0
    assert sum(rp.delivered[em.T_PREACCEPTREPLY] for rp in rps.values()) > 0


@pytest.mark.parametrize("name", ["drop7", "drop10", "rwc5", "rwc5_kv"])
def test_gaps_are_executed_again(name):
    sh, o, rps = run(name)
    assert sum(em.reexecutions(rp) for rp in rps.values()) > 0
    assert sum(len(v) for rp in rps.values() for v in rp.unmatched.values()) > 0
    for c, rp in rps.items():                                  # at most one counted reply per request
        for r, m in enumerate(rp.replicas):
            assert 0 < m.replies <= min(m.slot[r] + 1, sh.wl.max_requests), f"cluster {c} replica {r}"


def test_reply_when_commit_is_the_database_off_run():
    """kv = 1 adds the Database and changes nothing the model sees."""
    a, b = run("rwc5")[2], run("rwc5_kv")[2]
    for c in em.TRACED:
        assert [m.digest for m in a[c].replicas] == [m.digest for m in b[c].replicas]


def test_a_redelivered_commit_recommits_in_place():
    """A Commit for a slot at or below executed[o] (the re-commit branch of ep_handle_commit).  No
    run reaches it: a non-owner holds a COMMITTED instance only through the owner's one Commit,
    links do not duplicate, and nobody sends to itself.  A transport that hands a Commit in twice
    does (deliver): C gets A's Commit of slot 1 again with seq 9 once it has executed that slot.
    In the maps that rewrites log[A][1].seq and raises maxSeqPerKey, and the next command C
    leads takes seq 10; the ring, where slot 1 is gone, has to end up the same."""
    sh, at, args, seen = em.redelivery_case()
    o = ol.OracleSim(sh.cfg, sh.wl)
    ref = trace_ref.capture_many(o, [0], [sh.steps], before={at: lambda s: s.deliver(*args)}, clients=False)
    inst = o.read_instances()
    rp = em.replay_cluster(o, sh, 0, ref.msgs[0], {seen})
    c = rp.replicas[2]
    assert c.log[0][1].seq == 9 and c.max_seq[0] >= 9
    assert c.log[2][0].seq == 10 and c.executed[0] >= 1
    assert sum(rp.delivered.values()) == rp.matched + 1
    assert [i.slot for i in inst[6:9]] == c.slot == [2, -1, 2]


KATS = [
    (dict(npz=(5,), keys=4), dict(outstanding=1, max_requests=1, target=[0]), [], 10, [[1]] * 5),
    (dict(), dict(outstanding=2, target=[0, 1], max_requests=1),
     [(abi.FAULT_SLOW, 1, 2, 1, {}), (abi.FAULT_SLOW, 2, 0, 1, {})], 10, [[1, 2], [2, 1], [1, 2]]),
    (dict(), dict(outstanding=2, target=[0, 0], max_requests=2, start_step=[0, 1]),
     [(abi.FAULT_DROP, 0, 2, 0, dict(step_from=0, step_to=1)), (abi.FAULT_DROP, 0, 2, 0, dict(step_from=2, step_to=3))],
     20, [[1, 2, 3, 4], [1, 2, 3, 4], [2, 2, 3, 2, 3, 4]]),
]


@pytest.mark.parametrize("k", range(3), ids=["fast_path", "conflict_slow_path", "nil_gap"])
@pytest.mark.parametrize("seed", [1, 5])
def test_hand_derived_scenarios(k, seed):
    """The three scenarios of tests/test_epaxos.py: the model's execution orders are the ones
    derived by hand in their docstrings, and the oracle's."""
    ckw, wkw, faults, steps, want = KATS[k]
    cfg, wl = ep_cfg(seed=seed, **ckw), abi.make_workload(**wkw)
    o = ol.OracleSim(cfg, wl, faults=[abi.make_fault(kind, s, d, p, **kw) for (kind, s, d, p, kw) in faults])
    ref = trace_ref.capture_many(o, [0], [steps], clients=False)
    sh = em.Shape(cfg, wl, None, steps, True)
    rp = em.replay_cluster(o, sh, 0, ref.msgs[0])
    assert [m.order for m in rp.replicas] == want
    assert [o.exec_log(0, r) for r in range(o.N)] == want
