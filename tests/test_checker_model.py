"""The linearizability scan against the map-based checker of tests/checker_model.py (DESIGN.md
§3.7): `oracle_linearizable` on the reference's ten checker_test.go histories, the two tie-order
KATs and 3,000 seeded random histories; and, for every ABD shape of tests/abd_model.py, the oracle's
and the device's History.Linearizable on the model's own histories of the traced clusters (the
register checker where every partition has at most 128 ops, lin_big_kernel for n3big).  Every
comparison is exact."""
import random

import pytest

import abd_model as am
import checker_model as cm
import oracle_lib as ol
from paxi_amd import abi
from test_abd_model import run
from test_lin_gpu import gen_future_reads, gen_partition
from test_oracle_kats import KATS


@pytest.mark.parametrize("case", KATS["checker"], ids=[c["name"] for c in KATS["checker"]])
def test_reference_histories(case):
    ops = [tuple(o) for o in case["ops"]]
    a, e = cm.anomalies(ops), case["expect"]
    assert a == ol.linearizable(ops)
    assert a == 0 if e == "zero" else (a > 0 if e == "nonzero" else a == e)


@pytest.mark.parametrize("order", ["a", "b"])
def test_tie_order(order):
    k = KATS["lin_tie_order"]
    ops = [tuple(o) for o in k[order]]
    assert cm.anomalies(ops) == ol.linearizable(ops) == k["expect_" + order]


def sizes():
    """3,000 sizes from 1 to 200: nine in ten below 81, every size reached."""
    return [81 + (7 * (i // 10)) % 120 if i % 10 == 0 else 1 + (7 * (i - i // 10)) % 80 for i in range(3000)]


def test_random_histories():
    rng, total, ns = random.Random(1), 0, sizes()
    assert set(ns) == set(range(1, 201))
    for i, n in enumerate(ns):
        ops = cm.as_ops((gen_future_reads if i % 2 else gen_partition)(rng, n))
        a = cm.anomalies(ops)
        assert a == ol.linearizable(ops), f"history {i} of {n} ops: {ops}"
        total += a
    assert total > 3000


def loaded(name, make):
    """A handle of `make` that holds only the model's histories of the shape's traced clusters, the
    model's count of their anomalies and of their ops."""
    sh, res = run(name)
    reps = [rp.replicas for rp, _ in res.values()]
    cfg = abi.make_config(protocol=abi.ABD, npz=[sh.cfg.npz[z] for z in range(sh.cfg.n_zones)], clusters=len(reps),
                          keys=sh.cfg.keys, history=max([1] + [len(m.history) for ms in reps for m in ms]))
    sim = make(cfg, abi.make_workload(outstanding=1, max_requests=1, target=[0]))
    for c, ms in enumerate(reps):
        for r, m in enumerate(ms):
            sim.history_load(c, r, m.history)
    want = sum(cm.linearizable(am.partitions(rp)) for rp, _ in res.values())
    return sim, want, sum(len(m.history) for ms in reps for m in ms)


@pytest.mark.parametrize("name", list(am.SHAPES))
def test_oracle_on_the_models_histories(name):
    o, want, n = loaded(name, ol.OracleSim)
    assert o.linearizable() == (want, n)
    o.close()


def test_the_shapes_have_anomalies():
    """Not vacuous: most shapes' traced clusters hold anomalous reads, n3big's big partitions hundreds."""
    got = {name: loaded(name, ol.OracleSim)[1] for name in am.SHAPES}
    assert got["n3big"] > 100 and sum(1 for a in got.values() if a) >= 6, got


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(am.SHAPES))
def test_device_on_the_models_histories(name):
    from paxi_amd.sim import Simulation
    g, want, n = loaded(name, Simulation)
    assert g.linearizable() == (want, n, 0)
    g.close()
