"""Client request latency, host side (no GPU): Paxi's percentile rule in
paxisim_latency_stat_of against an independent numpy computation, Histogram's
merge / samples / write_file, the gloo reduction over two ranks, the ABI structs
and exports, and the oracle-derived reference the GPU tests compare with."""
import ctypes
import os
import re
import socket
import subprocess

import numpy as np
import pytest

import latency_ref
from paxi_amd import abi, sim
from paxi_amd import dist as pdist
from paxi_amd.latency import Histogram, go_float

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS = {"median": 0.5, "p95": 0.95, "p99": 0.99, "p999": 0.999}


def _numpy_stat(x, step_ms):
    """Statistic() of stat.go:44-66 on the raw samples."""
    ms = np.sort(np.asarray(x, dtype=np.float64) * step_ms)
    d = {k: ms[int(p * len(ms))] for k, p in PS.items()}
    d.update(size=len(ms), mean=float(np.asarray(x, dtype=np.int64).sum()) * step_ms / len(ms), min=ms[0], max=ms[-1])
    return d


def _cases():
    rng = np.random.default_rng(5)
    for n in (1, 2, 19, 20, 999, 1000, 1001):        # int(0.95 n) and int(0.999 n) change at these
        yield f"n{n}", rng.integers(0, 64, size=n)
        yield f"ramp{n}", np.arange(n) % 64
    yield "constant", np.full(500, 7)
    yield "two_spikes", np.array([3] * 990 + [60] * 10)
    yield "spike_at_p999", np.array([3] * 999 + [60])


@pytest.mark.parametrize("name,x", list(_cases()), ids=[c[0] for c in _cases()])
@pytest.mark.parametrize("step_ms", [1.0, 0.25])
def test_stat_of_matches_numpy(name, x, step_ms):
    h = Histogram.from_samples(x, 64)
    assert h.overflow == 0 and h.count == len(x)
    got, want = h.stat(step_ms).as_dict(), _numpy_stat(x, step_ms)
    assert got.pop("exact") == 1
    assert got == want


def test_stat_of_overflow_is_flagged_and_summaries_stay_exact():
    x = np.array([3] * 90 + [20, 40, 70, 70, 70, 100, 100, 100, 100, 1000])    # 16 bins: the last ten overflow
    h = Histogram.from_samples(x, 16)
    assert (h.overflow, h.count, h.min, h.max, h.sum) == (10, 100, 3, 1000, int(x.sum()))
    s, want = h.stat(0.5), _numpy_stat(x, 0.5)
    assert s.exact == 0
    assert (s.size, s.mean, s.min, s.max, s.median) == (100, want["mean"], 1.5, 500.0, 1.5)
    assert s.p95 == s.p99 == s.p999 == s.max               # inside the overflow bin: its upper bound
    with pytest.raises(ValueError):
        h.samples()
    # the same samples with enough bins are exact again
    assert Histogram.from_samples(x, 1024).stat(0.5).as_dict() == dict(want, exact=1)


def test_stat_of_rejects_empty_and_oversized():
    with pytest.raises(sim.PaxisimError):
        Histogram.from_samples([], 16).stat()
    h = Histogram.from_samples([1, 2], 2 * abi.LAT_MAX_BINS)
    with pytest.raises(sim.PaxisimError):
        h.stat()


def test_merge_of_halves_is_the_whole():
    x = np.random.default_rng(11).integers(2, 200, size=4001)
    for bins in (64, 256):
        whole = Histogram.from_samples(x, bins)
        halves = Histogram.from_samples(x[:1777], bins).merge(Histogram.from_samples(x[1777:], bins))
        assert halves == whole
        assert whole.merge(Histogram.from_samples([], bins)) == whole
    with pytest.raises(ValueError):
        Histogram.from_samples(x, 64).merge(Histogram.from_samples(x, 128))
    assert np.array_equal(Histogram.from_samples(x, 256).samples(), np.sort(x))


def test_write_file_prints_floats_like_go(tmp_path):
    h = Histogram.from_samples([5, 3, 5, 12], 16)
    for step_ms, lines in ((1, ["3", "5", "5", "12"]), (0.5, ["1.5", "2.5", "2.5", "6"]),
                           (0.25, ["0.75", "1.25", "1.25", "3"])):
        p = tmp_path / f"latency_{step_ms}"
        h.write_file(str(p), step_ms)
        got = p.read_text().split("\n")
        assert got[-1] == "" and got[:-1] == lines
        assert [float(v) for v in got[:-1]] == [s * step_ms for s in h.samples()]     # round trip
    assert [go_float(v) for v in (5.0, 2.5, 0.75, 0.0, 1e20, 1e21, 0.0001, 0.00001, 0.1 + 0.2)] == [
        "5", "2.5", "0.75", "0", "100000000000000000000", "1e+21", "0.0001", "1e-05", "0.30000000000000004"]


def test_struct_sizes_match_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "paxisim.h"
int main(void){
 printf("%zu %zu %zu %zu %zu %zu %u %u\n", sizeof(paxisim_latency), sizeof(paxisim_latency_stat),
   offsetof(paxisim_latency, min), offsetof(paxisim_latency, bins), offsetof(paxisim_latency_stat, p999),
   offsetof(paxisim_latency_stat, exact), (unsigned)PAXISIM_LAT_MAX_BINS, (unsigned)PAXISIM_ALL_WORKERS);
 return 0;}
'''
    (tmp_path / "p.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "p"), str(tmp_path / "p.c")],
                   check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "p")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(abi.Latency), ctypes.sizeof(abi.LatencyStat), abi.Latency.min.offset,
                   abi.Latency.bins.offset, abi.LatencyStat.p999.offset, abi.LatencyStat.exact.offset,
                   abi.LAT_MAX_BINS, abi.ALL_WORKERS]
    assert abi.ABI_VERSION == 14


def test_new_symbols_are_declared_and_exported():
    names = ["paxisim_latency_enable", "paxisim_latency_reset", "paxisim_latency_get", "paxisim_latency_stat_of"]
    hdr = open(os.path.join(ROOT, "include", "paxisim.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "paxi_amd", "libpaxisim.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (paxisim_\w+)", out))
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in exported and n in sim.EXPORTED
    assert all(hasattr(sim.Simulation, m) for m in ("latency_enable", "latency_reset", "latency"))


def test_reference_counts_every_reply():
    """The yardstick of the GPU tests: every oracle reply is one sample (derive asserts it),
    a finished worker keeps its last sample and a late worker's start is none."""
    r = latency_ref.ref("paxos3_max_requests")
    assert {w: len(v) for w, v in r.samples.items()} == {0: 660, 1: 660} and r.replies == 1320
    assert min(t for t, _ in r.samples[1]) > 40
    e = latency_ref.expected(r, 32)
    assert e.count == 1320 and e == latency_ref.expected(r, 32, 0).merge(latency_ref.expected(r, 32, 1))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_hist(rank):
    x = np.random.default_rng(100 + rank).integers(2 + rank, 90, size=300 + 50 * rank)
    return Histogram.from_samples(x, 64), x


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    h = pdist.reduce_latency(_rank_hist(rank)[0])
    q.put((rank, h.counts.tolist(), h.count, h.sum, h.overflow, h.min, h.max))
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_reduce_latency_two_rank_gloo():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in procs])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    whole = Histogram.from_samples(np.concatenate([_rank_hist(r)[1] for r in range(2)]), 64)
    assert whole.overflow > 0
    for _, counts, count, total, overflow, lo, hi in res:
        assert Histogram(counts, count, total, overflow, lo, hi) == whole
    # without a process group: the rank's own histogram
    assert pdist.reduce_latency(_rank_hist(0)[0]) == _rank_hist(0)[0]
