"""Times of the verdict calls at bench scale against the routes there were before them.

    python tools/verdict_bench.py [c2|c3|rec|all] [OUT.json]

c2: bench config 2 (Multi-Paxos N=5, 2^20 clusters) after one bench step of 400 virtual steps: find(STALLED),
verdict_counts and verdicts against read_state of the whole handle plus a host reduction.  c3: bench config 3
(ABD, 2^20 clusters, 80 steps): the LIN-bearing calls against paxisim_linearizable.  rec: config 2 at 2^18
clusters with the client history and the multi-version Database on: the CLIENT_LIN- and CONSENSUS-bearing
calls against their total-only scans.  Wall times of the calls through the Python binding, syncs included.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import bench
from paxi_amd import abi, sim
from paxi_amd.sim import Simulation

out = {"build_id": sim.build_id()}
def timed(fn, reps=5):
    ts, r = [], None
    for _ in range(reps):
        t = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t)
    return {"median_ms": round(1e3 * statistics.median(ts), 3), "min_ms": round(1e3 * min(ts), 3), "reps": reps}, r
def shape(cfg_id, clusters):
    d = bench.DEFAULTS[cfg_id]
    ns = argparse.Namespace(window=d["window"], mbox=d["mbox"], history=512, kv=1, crash_step=100)
    return bench.workload(cfg_id, clusters, 0, 0, ns)[:4], d
def dump():
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out), flush=True)

which = sys.argv[1] if len(sys.argv) > 1 else "all"
if which in ("all", "c2"):
    (cfg, wl, fp, faults), d = shape(2, 1 << 20)
    with Simulation(cfg, wl, fp, faults) as g:
        g.step(d["sim_steps"])
        g.sync()
        r = {"clusters": cfg.clusters, "steps": d["sim_steps"]}
        r["find_stalled"], (ids, total) = timed(lambda: g.find(abi.V_STALLED))
        r["stalled"] = total
        r["find_quiet_cap0"], _ = timed(lambda: g.find(abi.V_QUIET, cap=0))
        r["verdict_counts"], counts = timed(lambda: g.verdict_counts())
        r["counts"] = {k: v for k, v in counts.items() if v}
        r["verdicts_all"], _ = timed(lambda: g.verdicts())
        r["check"], _ = timed(lambda: g.check())
        r["stats"], _ = timed(lambda: g.stats())
        # the only route before the verdict calls to per-cluster flags: read_state of the whole handle and a host reduction
        N = g.N
        def old():
            st = g.read_state()
            a = np.frombuffer(st, dtype=np.uint8).reshape(cfg.clusters, N, C.sizeof(abi.ReplicaState))
            off = abi.ReplicaState.flags.offset
            fl = a[:, :, off:off + 4].copy().view(np.uint32).reshape(cfg.clusters, N)
            return np.nonzero(np.bitwise_or.reduce(fl, axis=1))[0]
        r["read_state_route"], flagged = timed(old, reps=2)
        r["read_state_bytes"] = cfg.clusters * N * C.sizeof(abi.ReplicaState)
        r["flagged_agree"] = bool(np.array_equal(flagged, g.find(abi.V_FLAGS)[0]))
    out["config2"] = r
    dump()
if which in ("all", "c3"):
    (cfg, wl, fp, faults), d = shape(3, 1 << 20)
    with Simulation(cfg, wl, fp, faults) as g:
        g.step(d["sim_steps"])
        g.sync()
        r = {"clusters": cfg.clusters, "steps": d["sim_steps"]}
        r["linearizable"], tot = timed(lambda: g.linearizable(), reps=3)
        r["totals"] = tot
        r["verdict_counts_lin"], counts = timed(lambda: g.verdict_counts(scans=abi.V_LIN), reps=3)
        r["lin_clusters"] = counts["LIN"]
        r["find_lin"], (ids, total) = timed(lambda: g.find(abi.V_LIN), reps=3)
        r["linearizable_after"] = g.linearizable()
    out["config3"] = r
    dump()
if which in ("all", "rec"):
    (cfg, wl, fp, faults), d = shape(2, 1 << 18)
    with Simulation(cfg, wl, fp, faults) as g:
        g.latency_enable(64)
        g.client_history_enable(64)
        g.multiversion_enable(64)
        g.step(200)
        g.sync()
        r = {"clusters": cfg.clusters, "steps": 200}
        r["client_linearizable"], r["client_totals"] = timed(lambda: g.client_linearizable(), reps=3)
        r["verdict_counts_client_lin"], c1 = timed(lambda: g.verdict_counts(scans=abi.V_CLIENT_LIN), reps=3)
        r["consensus"], r["consensus_totals"] = timed(lambda: g.consensus(), reps=3)
        r["consensus_failed_all"], _ = timed(lambda: g.consensus_failed(), reps=3)
        r["verdict_counts_consensus"], c2 = timed(lambda: g.verdict_counts(scans=abi.V_CONSENSUS), reps=3)
        r["counts"] = {"CLIENT_LIN": c1["CLIENT_LIN"], "TRUNCATED_client": c1["TRUNCATED"], "CONSENSUS": c2["CONSENSUS"],
                       "TRUNCATED_mv": c2["TRUNCATED"]}
    out["recorders"] = r
    dump()
