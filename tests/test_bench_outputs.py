"""bench.py --dump-outputs and --full.

dump_outputs writes what a caller of the timed path holds after the last timed
step: the statistics and a fixed sample of paxisim_read_state records, as
float64 arrays in which every uint32 word of a record is exact.  The CPU tests
drive it with the oracle (the same surface as Simulation); the GPU test runs
the command line once, as a plain run: the dumped records are the library's,
--steps sets the number of timed steps, and the legs behind --full stay out."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from paxi_amd import abi  # noqa: E402
import oracle_lib as ol  # noqa: E402

CLUSTERS = 600          # three blocks of 256, the last one short
STEPS = 120
WORDS = ctypes.sizeof(abi.ReplicaState) // 4


def oracle(clusters=CLUSTERS, steps=STEPS):
    a = argparse.Namespace(window=16, mbox=32, kv=1, history=512, clusters=clusters, sim_steps=400,
                           warmup=5, steps=20, crash_step=None, fz=1)
    cfg, wl, fp, faults, _ = bench.workload(2, clusters, 0, 0, a)
    o = ol.OracleSim(cfg, wl, fp, faults)
    o.step(steps)
    return o


def load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in ("stats", "clusters", "replica_state")}


def test_dump_holds_every_cluster_when_they_fit(tmp_path):
    o = oracle()
    bench.dump_outputs(o, str(tmp_path))
    got = load(tmp_path)
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["clusters"].tolist() == list(range(CLUSTERS))
    want = np.frombuffer(bytes(o.read_state()), dtype="<u4").reshape(CLUSTERS, o.N, WORDS)
    assert got["replica_state"].shape == want.shape and (got["replica_state"] == want).all()
    assert got["stats"].tolist() == np.frombuffer(bytes(o.stats()), dtype="<u8").tolist()
    assert o.stats().delivered_total > 0 and got["replica_state"].any()
    o.close()


def test_dump_sample_is_fixed_and_repeats(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BLOCKS", 2)
    runs = []
    for name in ("a", "b"):
        o = oracle()
        bench.dump_outputs(o, str(tmp_path / name))
        runs.append(load(tmp_path / name))
        ids = runs[-1]["clusters"].astype(int)
        want = np.frombuffer(bytes(o.read_state()), dtype="<u4").reshape(CLUSTERS, o.N, WORDS)[ids]
        assert (runs[-1]["replica_state"] == want).all()
        o.close()
    a, b = runs
    ids = a["clusters"].astype(int)
    assert 0 < len(ids) < CLUSTERS and (np.diff(ids) > 0).all() and ids.max() < CLUSTERS
    assert all((a[k] == b[k]).all() and a[k].shape == b[k].shape for k in a)


def test_dump_stays_within_its_size_limit():
    """The default sample of the largest records (9 replicas) and of the 1M-cluster headline."""
    for n in (5, 9):
        per_block = bench.DUMP_BLOCK * n * WORDS * 8
        keep = min(bench.DUMP_BLOCKS, (bench.DUMP_MAX_BYTES - (1 << 20)) // per_block)
        assert keep >= 1 and keep * per_block + (1 << 20) <= bench.DUMP_MAX_BYTES == 64 << 20


@pytest.mark.gpu
def test_plain_run_dumps_the_librarys_state_and_skips_the_full_legs(tmp_path):
    from paxi_amd.sim import Simulation
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--clusters", str(CLUSTERS), "--sim-steps", "40", "--dump-outputs", str(tmp_path)],
                         cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["unit"] == "messages/s"
    assert line["config"]["timed_sim_steps"] == [40, 160]
    assert not {"cpu_baseline", "parity_sampled", "shard_digests"} & set(line)
    got = load(tmp_path)
    a = argparse.Namespace(window=16, mbox=32, kv=1, history=512, clusters=CLUSTERS, sim_steps=40,
                           warmup=1, steps=3, crash_step=None, fz=1)
    cfg, wl, fp, faults, _ = bench.workload(2, CLUSTERS, 0, 0, a)
    with Simulation(cfg, wl, fp, faults) as g:
        for _ in range(4):
            g.step(40)
        want = np.frombuffer(bytes(g.read_state()), dtype="<u4").reshape(CLUSTERS, g.N, WORDS)
        stats = np.frombuffer(bytes(g.stats()), dtype="<u8")
    assert got["clusters"].tolist() == list(range(CLUSTERS))
    assert (got["replica_state"] == want).all() and got["stats"].tolist() == stats.tolist()
    assert stats.any() and want.any()
