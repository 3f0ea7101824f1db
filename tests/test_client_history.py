"""Client-side op history, host side (no GPU): the C ABI's new symbols and the pinned
header, the oracle-derived yardstick the GPU tests compare with (client_history_ref),
and History.from_client through Paxi's history files."""
import os
import re
import subprocess

import client_history_ref as chr_
import oracle_lib
from paxi_amd import abi, sim
from paxi_amd.history import History

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["paxisim_client_history_enable", "paxisim_client_history", "paxisim_client_history_load",
         "paxisim_client_linearizable"]


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "paxisim.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "paxi_amd", "libpaxisim.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (paxisim_\w+)", out))
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr), n + " is not declared"
        assert n in exported, n + " is not exported"
        assert n in sim.EXPORTED, n + " is not listed"
    for m in ("client_history_enable", "client_history", "client_history_load", "client_linearizable"):
        assert callable(getattr(sim.Simulation, m, None)), m
    assert hasattr(History, "from_client")


def test_pinned_header_is_the_trees_and_the_abi_version_stays():
    tree = open(os.path.join(ROOT, "include", "paxisim.h"), "rb").read()
    pinned = open(os.path.join(ROOT, "paxi_amd", "guard", "pinned", "242a73e", "include", "paxisim.h"), "rb").read()
    assert tree == pinned
    assert abi.ABI_VERSION == 14
    assert re.search(rb"#define\s+PAXISIM_ABI_VERSION\s+14\b", tree)


def _anomalies(name):
    return chr_.check([chr_.canonical(h) for h in chr_.ref(name).hist])


def test_yardstick_multipaxos_is_linearizable():
    anomalies, ops, _ = _anomalies("paxos5")
    assert anomalies == 0 and ops == chr_.ref("paxos5").replies > 0
    reads = [op for h in chr_.ref("paxos5").hist for op in chr_.canonical(h) if not op[1]]
    assert any(op[2] for op in reads), "no read returned a value: the check would be vacuous"


def test_yardstick_reports_epaxos_and_abd_anomalies():
    """The reference's own behaviour (conflicting EPaxos commands execute in different orders at
    different replicas): reported, not fixed.  The shapes keep the GPU tests from
    being vacuous."""
    for name in ("epaxos5_keys1", "abd5"):
        anomalies, ops, _ = _anomalies(name)
        print(name, anomalies, ops)
        assert anomalies > 0 and ops == chr_.ref(name).replies


def test_hand_written_stale_read_is_one_anomaly():
    assert chr_.check([chr_.STALE_READ]) == (1, 3, 3)
    fresh = chr_.STALE_READ[:2] + [(0, 0, 2, 4, 5)]
    assert chr_.check([fresh]) == (0, 3, 3)
    # the partitions are per key: the same read on another key matches no write
    assert chr_.check([chr_.STALE_READ[:2] + [(1, 0, 1, 4, 5)]]) == (0, 3, 2)
    assert oracle_lib.linearizable([(1, None, 0, 1), (2, None, 2, 3), (None, 1, 4, 5)]) == 1


def test_yardstick_counts_every_reply_of_late_and_finished_workers():
    """derive asserts ops == replies; a late worker's start is no op, a finished worker keeps its last."""
    r = chr_.ref("paxos3_max_requests")
    assert r.replies == 1320
    assert all([len(ops) for ops in cl] == [10, 10] for cl in r.hist)
    assert all(cl[1][0][3] == 40 for cl in r.hist), "worker 1's first op starts at its start_step"
    r = chr_.ref("paxos9_late")
    assert sum(len(ops) for cl in r.hist for ops in cl) == r.replies
    assert all(cl[2][0][3] == 40 and cl[3][0][3] == 41 for cl in r.hist)


class _Stub:
    """What History.from_client reads of a Simulation."""

    class cfg:
        clusters = 2

    hist = {0: [(0, 1, 1, 0, 3), (1, 1, 2, 0, 4), (0, 0, 1, 4, 7), (1, 0, 0, 5, 9)],
            1: [(3, 0, 0, 0, 2)]}

    def client_history(self, cluster):
        return list(self.hist[cluster]), 0


def test_from_client_round_trips_through_the_history_files(tmp_path):
    hs = History.from_client(_Stub(), step_ns=1000)
    assert [len(h.operations) for h in hs] == [4, 1]
    h = hs[0]
    assert sorted(h.shard) == [0, 1]
    assert (h.shard[0][0].input, h.shard[0][0].output) == (1, None)        # a write has an input
    assert (h.shard[0][1].input, h.shard[0][1].output) == (None, 1)        # a read an output
    assert (h.shard[1][1].output, h.shard[1][1].start, h.shard[1][1].end) == (0, 5000, 9000)   # a read of nil: 0
    assert History.from_client(_Stub(), clusters=[1])[0].shard[3][0].output == 0
    path = str(tmp_path / "history")
    h.write_log(path)
    back = History.read_file(path)
    assert sorted(back.shard) == [0, 1]
    for key in h.shard:
        got = [(o.input, o.output, o.start, o.end) for o in back.shard[key]]
        want = [(None if o.input is None else str(o.input), None if o.output is None else str(o.output), o.start, o.end)
                for o in h.shard[key]]
        assert got == want
    h.write_file(path)
    lines = open(path + ".csv").read().splitlines()
    assert lines[0] == "1,<nil>,0.000000,0.000003" and len([x for x in lines if not x.startswith("PerSecond")]) == 4
