"""Per-cluster verdict words: the interface as it is declared and exported, and the
yardstick's populations on the oracle alone - so that the GPU tests of tests/test_verdict_gpu.py,
which compare against this yardstick, cannot pass vacuously."""
import os
import re
import subprocess

from paxi_amd import abi, sim
import oracle_lib
import verdict_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["paxisim_verdict_available", "paxisim_verdicts", "paxisim_find", "paxisim_verdict_counts",
           "paxisim_select_words"]


def test_header_declares_the_symbols_and_the_bits():
    text = open(os.path.join(ROOT, "include", "paxisim_verdict.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\bint %s\(" % s, text), s
    for name in ("AGREE", "CONSENSUS", "LIN", "CLIENT_LIN", "LIN_SKIPPED", "TRUNCATED", "QUIET", "WAITING", "STALLED",
                 "ALL", "FLAGS"):
        m = re.search(r"#define PAXISIM_V_%s\s+(0x[0-9A-Fa-f]+)u" % name, text)
        assert m and int(m.group(1), 16) == getattr(abi, "V_" + name), name
    assert abi.V_ALL == abi.V_FLAGS | sum(1 << b for b in abi.V_NAMES)
    assert abi.V_STALLED == 1 << 18 and abi.V_AGREE == 1 << 8
    assert {n for n in abi.PROTOTYPES if re.search(r"\b%s\(" % n, text)} == set(SYMBOLS)


def test_symbols_are_exported_and_listed():
    out = subprocess.run(["nm", "-D", "--defined-only", sim.LIB_PATH], check=True, capture_output=True, text=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in SYMBOLS:
        assert s in defined and s in sim.EXPORTED, s


def test_abi_version_stays_14():
    assert abi.ABI_VERSION == 14
    text = open(os.path.join(ROOT, "include", "paxisim.h")).read()
    assert re.search(r"#define PAXISIM_ABI_VERSION\s+14\b", text)


def test_select_constants_are_where_the_gpu_suite_reads_them():
    text = open(os.path.join(ROOT, "paxi_amd", "csrc", "verdict_kernel.h")).read()
    assert re.search(r"constexpr uint32_t SEL_WG = (\d+);", text)
    assert re.search(r"constexpr uint32_t SEL_SCAN = (\d+);", text)


# ---- the yardstick's populations -----------------------------------------------------------------
def test_paxos3_has_running_finished_and_stalled_clusters():
    w = vr.cached("paxos3", lambda: vr.words(*vr.paxos3(), steps=vr.PAXOS3_STEP))
    running, finished, stalled = vr.populations(w.words)
    print("paxos3 step 33: running/finished/stalled", running, finished, stalled, "late-bucket only", len(w.late_only))
    assert min(running, finished, stalled) >= 8            # measured 46 / 132 / 22
    assert len(w.late_only) >= 1                           # records only in a later arrival bucket; measured 1
    assert not w.poison


def test_wpaxos9_has_running_finished_and_stalled_clusters():
    w = vr.cached("wpaxos9", lambda: vr.words(*vr.wpaxos9(130), steps=vr.WPAXOS9_STEP))
    running, finished, stalled = vr.populations(w.words)
    print("wpaxos9 step 34: running/finished/stalled", running, finished, stalled)
    assert min(running, finished, stalled) >= 8            # measured 36 / 44 / 50


def test_wpaxos9_agreement_set():
    cfg, wl, fp, faults = vr.wpaxos9(200)
    bad = vr.cached("wpaxos9_agree", lambda: vr.agree(cfg, wl, fp, faults, steps=vr.WPAXOS9_AGREE_STEP))
    assert bad == vr.WPAXOS9_AGREE_SET
    o = oracle_lib.OracleSim(cfg, wl, fp, faults)
    o.step(vr.WPAXOS9_AGREE_STEP)
    assert o.check() == 1                                  # the total names no cluster
    flags = 0
    for s in o.read_state(181, 1):
        flags |= s.flags
    assert flags == abi.F_GHOST
    o.close()


def test_abd3_has_anomalous_and_clean_clusters():
    per, ops, total = vr.cached("abd3_lin", lambda: vr.lin(*vr.abd3(), steps=vr.ABD3_STEP))
    anomalous = sum(1 for p in per if p)
    print("abd3 step 150: anomalous/clean", anomalous, len(per) - anomalous, "anomalies", sum(per), "ops", ops)
    assert anomalous >= 8 and len(per) - anomalous >= 8    # measured 126 / 74
    assert (sum(per), ops) == total                        # the per-cluster counts sum to the oracle's total


def test_client_history_overflows_in_some_clusters_only():
    import client_history_ref
    cfg, wl, fp, faults = vr.paxos3()
    r = client_history_ref.derive(cfg, wl, fp, faults, steps=vr.CHIST_STEP)
    cut = sum(1 for c in range(cfg.clusters) if any(len(ops) > vr.CHIST_CAP for ops in r.hist[c]))
    print("paxos3 step 20, rows of 5 ops: clusters with a dropped op", cut, "of", cfg.clusters)
    assert 0 < cut < cfg.clusters                          # measured 198 of 200


def test_no_step_unit_includes_the_changed_headers():
    """The verdict kernels and the per-cluster marks of the linearizability scan live in headers that
    only host_check.hip includes, so no step kernel is compiled from different text."""
    import __graft_entry__ as ge
    for src in ge.HIP_SOURCES:
        if src.startswith("k_"):
            inc = {os.path.basename(p) for p in ge._includes(os.path.join(ge.CSRC, src))}
            assert not inc & {"verdict_kernel.h", "lin_kernel.h", "paxisim_verdict.h"}, src
    assert "verdict_kernel.h" in ge.HIP_HEADERS
