"""Per-cluster verdict words and the device-side search over them, on the GPU
against tests/verdict_ref.py.  tests/test_verdict.py asserts the yardstick's populations."""
import json
import os
import re

import numpy as np
import pytest

from paxi_amd import abi, sim, trace
from paxi_amd.sim import Simulation, PaxisimError, select_words
import client_history_ref
import mv_ref
import oracle_lib
import trace_ref
import verdict_ref as vr
from test_agreement import same_step_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPP, ERANGE = r"error -1:", r"error -4:", r"error -5:"
V = abi


def _kernel_const(name):
    text = open(os.path.join(ROOT, "paxi_amd", "csrc", "verdict_kernel.h")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1))


SEL_WG, SEL_SCAN = _kernel_const("SEL_WG"), _kernel_const("SEL_SCAN")


def _ids(a):
    return [int(x) for x in a]


# ---- 1. The select at its edges ----------------------------------------------------------------
SIZES = sorted({0, 1, 63, 64, 65, SEL_WG - 1, SEL_WG, SEL_WG + 1, SEL_WG * SEL_SCAN - 1, SEL_WG * SEL_SCAN,
                SEL_WG * SEL_SCAN + 1, SEL_WG * (SEL_SCAN + 1), SEL_WG * (SEL_SCAN + 1) + 1, 300001})
BIT, OTHER = 0x100, 0x10


def _patterns(n):
    rng = np.random.default_rng(n)
    pats = {"none": np.zeros(n, np.uint32), "all": np.full(n, BIT, np.uint32)}
    for name, idx in (("last", [n - 1]), ("first", [0])):
        w = np.zeros(n, np.uint32)
        if n:
            w[idx] = BIT
        pats[name] = w
    w = np.zeros(n, np.uint32)
    w[::64] = BIT
    pats["every64"] = w
    pats["random"] = (rng.integers(0, 4, n).astype(np.uint32) == 0) * np.uint32(BIT) | \
        (rng.integers(0, 3, n).astype(np.uint32) == 0) * np.uint32(OTHER)
    return pats


@pytest.mark.parametrize("n", SIZES)
def test_select_words_against_nonzero(n):
    for name, w in _patterns(n).items():
        want = np.nonzero(w & BIT)[0]
        ids, total = select_words(w, BIT)
        assert total == len(want) and np.array_equal(ids, want), (n, name)
        ids, total = select_words(w, BIT, cap=0)                            # NULL ids
        assert total == len(want) and len(ids) == 0, (n, name)
        for cap in {max(0, len(want) - 1), len(want), len(want) + 1, len(want) // 2}:
            ids, total = select_words(w, BIT, cap=cap)
            assert total == len(want) and np.array_equal(ids, want[:cap]), (n, name, cap)
    w = _patterns(n)["random"]
    want = np.nonzero((w & BIT != 0) & (w & OTHER == 0))[0]                  # any and none
    ids, total = select_words(w, BIT, none=OTHER)
    assert total == len(want) and np.array_equal(ids, want), n
    want = np.nonzero(w & OTHER == 0)[0]                                     # any = 0: none alone
    ids, total = select_words(w, 0, none=OTHER)
    assert total == len(want) and np.array_equal(ids, want), n
    ids, total = select_words(w, 0)                                          # every word
    assert total == n and np.array_equal(ids, np.arange(n)), n
    ids, total = select_words(w[:0], BIT)                                    # no words: NULL words and ids
    assert total == 0 and len(ids) == 0 and ids.dtype == np.uint64


# ---- 2. Stall triage ---------------------------------------------------------------------------
def _plain(shape, chunks):
    """Replica states and stats of a run that never calls a verdict function."""
    with Simulation(*shape) as g:
        for n in chunks:
            g.step(n)
        return [s.as_tuple() for s in g.read_state()], g.stats().as_dict()


def _triage(shape, chunks, ref, frozen=False):
    """frozen: the form compacts, so by the end some clusters must sit frozen in permuted slots."""
    cfg = shape[0]
    with Simulation(*shape) as g:
        for n in chunks[:-1]:
            g.step(n)
        g.verdicts()                                        # a verdict call between two steps changes nothing
        g.step(chunks[-1])
        got = g.verdicts()
        assert got.dtype == np.uint32 and len(got) == cfg.clusters
        want = np.array(ref.words, dtype=np.uint32)
        keep = np.ones(cfg.clusters, bool)
        keep[ref.poison] = False
        bad = np.nonzero(((got ^ want) & vr.LIVE != 0) & keep)[0]
        assert len(bad) == 0, f"clusters {bad[:8]}: got {got[bad[:8]]}, want {want[bad[:8]]}"
        assert not np.any(got[ref.poison] & (V.V_QUIET | V.V_STALLED))
        assert np.array_equal(got & V.V_FLAGS, want & V.V_FLAGS)
        assert np.array_equal(g.verdicts(lo=60, n=10), got[60:70])
        if not ref.poison:
            ids, total = g.find(V.V_STALLED)
            stalled = [c for c, w in enumerate(ref.words) if w & V.V_STALLED]
            assert _ids(ids) == stalled and total == len(stalled)
            ids, total = g.find(V.V_STALLED, cap=3)
            assert _ids(ids) == stalled[:3] and total == len(stalled)
            ids, total = g.find(V.V_STALLED, cap=0)             # NULL ids: the count alone
            assert len(ids) == 0 and total == len(stalled)
            ids, _ = g.find(V.V_STALLED, global_ids=True)
            assert _ids(ids) == [c + cfg.cluster_base for c in stalled]
        counts = g.verdict_counts()
        flagged = list(g.stats().flagged)
        assert [counts[V.V_NAMES[b]] for b in range(8)] == flagged
        for b, name in V.V_NAMES.items():
            assert counts[name] == int(np.count_nonzero(got & (1 << b))), name
        if frozen:
            assert g.active_clusters() < cfg.clusters
        seen = [s.as_tuple() for s in g.read_state()], g.stats().as_dict()
    return seen


FORMS = {"default": {}, "serial0": {"PAXISIM_SERIAL": "0"}, "pipe1": {"PAXISIM_PIPE": "1"},
         "compact16": {"PAXISIM_COMPACT_EVERY": "16"}}
PAXOS3_CHUNKS = (1, 15, 16, 1)     # 33 steps, uneven


@pytest.mark.parametrize("form", list(FORMS))
def test_stall_triage_paxos3(monkeypatch, form):
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    kw = {"steps_per_launch": 8} if form == "compact16" else {}
    ref = vr.cached("paxos3", lambda: vr.words(*vr.paxos3(), steps=vr.PAXOS3_STEP))
    assert sum(PAXOS3_CHUNKS) == vr.PAXOS3_STEP
    seen = _triage(vr.paxos3(**kw), PAXOS3_CHUNKS, ref, frozen=form == "compact16")
    assert seen == _plain(vr.paxos3(**kw), PAXOS3_CHUNKS)


def test_stall_triage_two_pools(monkeypatch):
    """512 + 64 + 5 clusters, the smallest shape that gets two pools (tests/test_pools_gpu.py)."""
    monkeypatch.setenv("PAXISIM_POOLS", "2")
    monkeypatch.setenv("PAXISIM_PHASE_SORT", "1")
    monkeypatch.setenv("PAXISIM_COMPACT_EVERY", "16")
    n = 512 + 64 + 5
    ref = vr.cached("paxos3_pools", lambda: vr.words(*vr.paxos3(n), steps=vr.PAXOS3_STEP))
    running, finished, stalled = vr.populations(ref.words)
    assert min(running, finished, stalled) >= 8
    seen = _triage(vr.paxos3(n, steps_per_launch=8), PAXOS3_CHUNKS, ref, frozen=True)
    assert seen == _plain(vr.paxos3(n, steps_per_launch=8), PAXOS3_CHUNKS)


def test_stall_triage_wpaxos9():
    ref = vr.cached("wpaxos9", lambda: vr.words(*vr.wpaxos9(130), steps=vr.WPAXOS9_STEP))
    chunks = (3, 30, 1)
    assert _triage(vr.wpaxos9(130), chunks, ref) == _plain(vr.wpaxos9(130), chunks)


def test_stall_triage_abd3():
    ref = vr.cached("abd3", lambda: vr.words(*vr.abd3(), steps=vr.ABD3_STEP))
    chunks = (7, 100, 43)
    assert _triage(vr.abd3(), chunks, ref) == _plain(vr.abd3(), chunks)


# ---- 3. Agreement --------------------------------------------------------------------------------
def test_agreement_names_the_wpaxos_cluster():
    with Simulation(*vr.wpaxos9(200)) as g:
        g.step(vr.WPAXOS9_AGREE_STEP)
        ids, total = g.find(V.V_AGREE)
        assert (_ids(ids), total) == (vr.WPAXOS9_AGREE_SET, 1)
        assert g.verdict_counts()["AGREE"] == g.check() == 1
        assert g.verdicts(lo=181, n=1)[0] & V.V_FLAGS == V.F_GHOST


FORGED = (0, 63, 64, 129)


def _forge(s, clusters=FORGED):
    """tests/test_agreement.py's forged P3s (replicas 1..4 commit slots 0..15 with commands A, B, B, C)."""
    base = {1: 100, 2: 200, 3: 200, 4: 300}
    for c in clusters:
        for r, b in base.items():
            s.deliver(c, r, 0, [(0, abi.MSG_P3, 0, sl, b + sl) for sl in range(16)])
    s.step(1)


def test_agreement_names_the_forged_clusters():
    cfg, wl, faults = same_step_case(130)
    o = oracle_lib.OracleSim(cfg, wl, faults=faults)
    _forge(o)
    assert o.check() == len(FORGED)
    o.close()
    bad = vr.agree(cfg, wl, None, faults, drive=lambda o1, c: _forge(o1, [0] if c in FORGED else []))
    assert bad == list(FORGED)
    with Simulation(cfg, wl, faults=faults) as g:
        _forge(g)
        ids, total = g.find(V.V_AGREE)
        assert (_ids(ids), total) == (list(FORGED), len(FORGED))
        assert g.verdict_counts()["AGREE"] == g.check() == len(FORGED)
        assert not np.any(g.verdicts() & V.V_QUIET)         # the workers never start: nothing is quiet


def test_epaxos_has_no_agree_bit():
    make, schedule = mv_ref.SHAPES["epaxos5"]
    with Simulation(*make()) as g:
        g.step(schedule[0])
        assert not g.verdict_available() & V.V_AGREE
        assert g.find(V.V_AGREE)[1] == 0 and g.check() == 0


# ---- 4. Linearizability --------------------------------------------------------------------------
def test_lin_bit_matches_the_oracle_per_cluster():
    per, ops, total = vr.cached("abd3_lin", lambda: vr.lin(*vr.abd3(), steps=vr.ABD3_STEP))
    with Simulation(*vr.abd3()) as g:
        g.step(vr.ABD3_STEP)
        before = g.linearizable()
        assert before == (total[0], total[1], 0)
        got = g.verdicts(scans=V.V_LIN)
        assert [bool(w & V.V_LIN) for w in got] == [p > 0 for p in per]
        assert not np.any(got & (V.V_LIN_SKIPPED | V.V_CLIENT_LIN | V.V_CONSENSUS | V.V_TRUNCATED))
        assert not np.any(g.verdicts() & V.V_LIN)           # not requested: 0
        ids, n = g.find(V.V_LIN)                            # scans default to the bits asked about
        assert _ids(ids) == [c for c, p in enumerate(per) if p] and n == len(ids)
        assert g.verdict_counts(scans=V.V_LIN)["LIN"] == n
        assert g.linearizable() == before


KAT = next(k for k in json.load(open(os.path.join(ROOT, "tests", "golden", "kats.json")))["checker"]
           if k["name"] == "read_misses_write")
KAT_OPS = [(0, 1, i, s, e) if i is not None else (0, 0, o, s, e) for (i, o, s, e) in KAT["ops"]]
MARKED = (3, 64, 199)


def _long_history(stale):
    """200 ops of one key, more than a register partition holds: writes 1..199 one after the other,
    then a read of the last value (clean) or of the first (stale: an anomaly)."""
    ops = [(0, 1, v, 2 * v, 2 * v + 1) for v in range(1, 200)]
    return ops + [(0, 0, 1 if stale else 199, 500, 501)]


def test_lin_bit_lands_on_the_loaded_clusters():
    assert oracle_lib.linearizable([tuple(o) for o in KAT["ops"]]) > 0
    cfg = abi.make_config(protocol=abi.ABD, npz=[3], clusters=200, keys=2, history=16)
    wl = abi.make_workload(outstanding=1, max_requests=1, target=[0])
    with Simulation(cfg, wl) as g:
        for c in MARKED:
            g.history_load(c, 1, KAT_OPS)
        got = g.verdicts(scans=V.V_LIN)
        assert _ids(np.nonzero(got & V.V_LIN)[0]) == list(MARKED)
        assert g.linearizable()[0] == 3 * oracle_lib.linearizable([tuple(o) for o in KAT["ops"]])


def test_lin_bit_of_a_partition_beyond_the_register_path():
    to_op = lambda ops: [(v if w else None, None if w else v, s, e) for (_, w, v, s, e) in ops]
    assert oracle_lib.linearizable(to_op(_long_history(True))) > 0
    assert oracle_lib.linearizable(to_op(_long_history(False))) == 0
    cfg = abi.make_config(protocol=abi.ABD, npz=[3], clusters=200, keys=2, history=128)
    wl = abi.make_workload(outstanding=1, max_requests=1, target=[0])
    with Simulation(cfg, wl) as g:
        for c in range(0, 200, 7):                          # clean long partitions around the marked ones
            ops = _long_history(c in MARKED)
            for r in range(3):
                g.history_load(c, r, ops[r * 67:(r + 1) * 67])
        for c in MARKED:
            ops = _long_history(True)
            for r in range(3):
                g.history_load(c, r, ops[r * 67:(r + 1) * 67])
        got = g.verdicts(scans=V.V_LIN)
        assert _ids(np.nonzero(got & V.V_LIN)[0]) == list(MARKED)
        a, n, sk = g.linearizable()
        assert sk == 0 and n == 200 * len(set(range(0, 200, 7)) | set(MARKED)) and a > 0


def _recording(shape, chist=None, mv=None):
    g = Simulation(*shape)
    g.latency_enable(64)
    if chist:
        g.client_history_enable(chist)
    if mv:
        g.multiversion_enable(mv)
    return g


def test_client_lin_bit():
    with _recording(vr.paxos3(), chist=16) as g:
        for c in MARKED:
            g.client_history_load(c, 0, client_history_ref.STALE_READ)
        got = g.verdicts(scans=V.V_CLIENT_LIN)
        assert _ids(np.nonzero(got & V.V_CLIENT_LIN)[0]) == list(MARKED)
        assert not np.any(got & V.V_TRUNCATED)
    with _recording(vr.paxos3(), chist=16) as g:            # a natural Multi-Paxos run: linearizable
        g.step(vr.PAXOS3_STEP)
        assert g.client_linearizable()[0] == 0
        assert not np.any(g.verdicts(scans=V.V_CLIENT_LIN) & (V.V_CLIENT_LIN | V.V_TRUNCATED | V.V_LIN_SKIPPED))


# ---- 5. CONSENSUS and TRUNCATED ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["epaxos5", "paxos3_freeze"])
def test_consensus_bit(name):
    make, schedule = mv_ref.SHAPES[name]
    cfg = make()[0]
    r = mv_ref.ref(name)
    N = abi.n_replicas(cfg)
    lens = sorted(len(h) for h in r.hist.values())
    cap = max(1, lens[len(lens) * 3 // 4])                  # overflows some rows and not others
    want = mv_ref.verdict(r.hist, cfg.clusters, N, cfg.keys, cap=cap)
    with _recording(make(), mv=cap) as g:
        for n in schedule:
            g.step(n)
        got = g.verdicts(scans=V.V_CONSENSUS)
        assert [bool(w & V.V_CONSENSUS) for w in got] == [m != 0 for m in want.masks]
        assert [bool(w & V.V_CONSENSUS) for w in got] == [m != 0 for m in g.consensus_failed()]
        cut = [any(g.kv_history(c, rr, k)[1] for rr in range(N) for k in range(cfg.keys)) for c in range(cfg.clusters)]
        assert [bool(w & V.V_TRUNCATED) for w in got] == cut
        assert 0 < sum(cut) < cfg.clusters
        assert not np.any(g.verdicts() & (V.V_CONSENSUS | V.V_TRUNCATED))
    if name == "epaxos5":
        assert 0 < sum(1 for m in want.masks if m) < cfg.clusters


def test_truncated_client_history():
    with _recording(vr.paxos3(), chist=vr.CHIST_CAP) as g:
        g.step(vr.CHIST_STEP)
        got = g.verdicts(scans=V.V_CLIENT_LIN)
        cut = [g.client_history(c)[1] > 0 for c in range(g.cfg.clusters)]
        assert [bool(w & V.V_TRUNCATED) for w in got] == cut
        assert 0 < sum(cut) < g.cfg.clusters


# ---- 6. The none mask ------------------------------------------------------------------------------
def test_none_mask_filters_the_flagged():
    """WPaxos 3x3 at W = 8 raises flags in some clusters and not in others: every predicate below
    against the same filter on the host."""
    with Simulation(*vr.wpaxos9(200)) as g:
        g.step(vr.WPAXOS9_AGREE_STEP)
        w = g.verdicts()
        for any_, none in ((V.V_AGREE, V.F_UNFAITHFUL | V.F_POISON), (V.V_STALLED, V.F_GHOST),
                           (V.V_AGREE | V.V_STALLED, V.V_FLAGS), (0, V.V_FLAGS), (V.V_QUIET | V.F_GHOST, V.V_WAITING)):
            want = [c for c, x in enumerate(w) if (any_ == 0 or x & any_) and not x & none]
            ids, total = g.find(any_, none=none)
            assert _ids(ids) == want and total == len(want), (any_, none)
        assert 0 < len(g.find(V.V_FLAGS)[0]) < 200 and 0 < g.find(0, none=V.V_FLAGS)[1] < 200


# ---- 7. Errors and state ---------------------------------------------------------------------------
def test_errors():
    with Simulation(*vr.paxos3(70)) as g:
        assert g.verdict_available() == V.V_FLAGS | V.V_AGREE | V.V_QUIET | V.V_WAITING | V.V_STALLED
        for scan in (V.V_LIN, V.V_CLIENT_LIN, V.V_CONSENSUS):
            for call in (lambda: g.verdicts(scans=scan), lambda: g.find(scan), lambda: g.verdict_counts(scans=scan)):
                with pytest.raises(PaxisimError, match=EUNSUPP):
                    call()
        with pytest.raises(PaxisimError, match=EINVAL):
            g.verdicts(scans=V.V_AGREE)                     # not a scan
        for any_, none in ((1 << 14, 0), (0, 1 << 19), (1 << 31, 0)):
            with pytest.raises(PaxisimError, match=EINVAL):
                g.find(any_, none=none, scans=0)
        for lo, n in ((0, 71), (70, 1), (71, 0), (1, 70)):
            with pytest.raises(PaxisimError, match=ERANGE):
                g.verdicts(lo=lo, n=n)
        assert len(g.verdicts(lo=70, n=0)) == 0
    with Simulation(*vr.abd3(70)) as g:
        assert g.verdict_available() & V.V_SCANS == V.V_LIN
        with pytest.raises(PaxisimError, match=EUNSUPP):
            g.verdicts(scans=V.V_LIN | V.V_CONSENSUS)
    with _recording(vr.paxos3(70), chist=8, mv=8) as g:
        assert g.verdict_available() == V.V_ALL & ~V.V_LIN


def test_verdicts_survive_snapshot_restore_and_fork():
    with Simulation(*vr.paxos3()) as g:
        g.step(20)
        blob = g.snapshot()
        g.step(13)
        want = g.verdicts()
        with Simulation(*vr.paxos3()) as f:
            f.restore(blob)
            f.step(13)
            assert np.array_equal(f.verdicts(), want)
        k = g.fork()
        assert np.array_equal(k.verdicts(), want)
        assert _ids(k.find(V.V_STALLED)[0]) == _ids(g.find(V.V_STALLED)[0])
        k.close()
        s1 = g.snapshot()
        g.verdicts()
        g.find(V.V_STALLED)
        g.verdict_counts()
        assert np.array_equal(g.snapshot(), s1)             # the verdict calls leave the state as it was


# ---- 8. End to end ---------------------------------------------------------------------------------
def test_found_clusters_are_traced_on_a_small_handle():
    cfg, wl, faults = same_step_case(130)
    with Simulation(cfg, wl, faults=faults) as g:           # pass 1: which clusters disagree
        _forge(g)
        found = _ids(g.find(V.V_AGREE, none=V.F_UNFAITHFUL)[0])
    assert found == list(FORGED)
    o = oracle_lib.OracleSim(cfg, wl, faults=faults)
    for c in FORGED:
        for r, b in {1: 100, 2: 200, 3: 200, 4: 300}.items():
            o.deliver(c, r, 0, [(0, abi.MSG_P3, 0, sl, b + sl) for sl in range(16)])
    ref = trace_ref.capture_many(o, found, [1], clients=False)
    o.close()
    with Simulation(cfg, wl, faults=faults) as g:           # pass 2: the recorder on, for the found ids only
        g.latency_enable(64)
        g.trace_enable(found, 256)
        _forge(g)
        for c in found:
            got = trace.from_device(g, c)["msgs"]
            assert got == ref.msgs[c] and sum(len(m[3]) for m in got) == 4 * 16, c
        assert g.trace_totals() == (4 * 16 * len(found), 0)


# ---- 9. The tool -----------------------------------------------------------------------------------
def test_triage_tool_from_a_config_to_gob_files(tmp_path):
    """tools/triage.py on bench config 2 at 128 clusters: the stalled clusters are the yardstick's, and
    each found cluster, re-run alone under its global id, shows the same word and leaves its streams."""
    import argparse
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench
    import triage
    d = bench.DEFAULTS[2]
    ns = argparse.Namespace(window=d["window"], mbox=d["mbox"], history=512, kv=1, crash_step=100)
    cfg, wl, fp, faults, _ = bench.workload(2, 128, 0, 0, ns)
    ref = vr.words(cfg, wl, fp, faults, steps=120)
    stalled = [c for c, w in enumerate(ref.words) if w & V.V_STALLED]
    assert 0 < len(stalled) < 128
    args = argparse.Namespace(config=2, clusters=128, steps=120, crash_step=100, find="stalled", any="0", none="0",
                              max_ids=None, max_traces=2, records=0, out=str(tmp_path))
    lines = []
    r = triage.triage(args, out=lines.append)
    assert r["ids"] == stalled and r["total"] == len(stalled) and r["counts"]["STALLED"] == len(stalled)
    assert [t["cluster"] for t in r["traced"]] == stalled[:2]
    for t in r["traced"]:
        assert t["word"] & vr.LIVE == ref.words[t["cluster"]] & vr.LIVE
        files = os.listdir(t["dir"])
        assert "schedule.json" in files and any(f.endswith(".gob") for f in files) and t["messages"] > 0
    assert os.path.exists(os.path.join(str(tmp_path), "triage.json")) and len(lines) == 3 + 2
