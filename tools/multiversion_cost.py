"""What keeping the multi-version Database costs the recording step kernels.

Runs BASELINE config 2's shape (bench.py workload(2): Multi-Paxos 5 replicas, Drop/Slow faults, 1M
clusters) with kv = 1 and latency recording on, without and with multiversion (--versions values
kept per key, replica and cluster) in mirrored order (without, with, with, without), each a fresh
handle, and times the step launches with paxisim_kernel_time (HIP events on the launch stream).
The "with" runs then time paxisim_consensus over the handle (host wall clock around the call, the
second of two calls) and report the bytes it reads - the counts plus the kept values, 4 bytes each -
and the rate.  Prints one JSON line.
usage: python tools/multiversion_cost.py [--clusters N] [--steps K] [--warmup W] [--bins B] [--versions H]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from paxi_amd import abi, sim  # noqa: E402


def run(args, on):
    cfg, wl, fp, faults, _ = bench.workload(2, args.clusters, 0, 0, args)
    with sim.Simulation(cfg, wl, fp, faults) as g:
        g.latency_enable(args.bins)
        if on:
            g.multiversion_enable(args.versions)
        for _ in range(args.warmup):
            g.step(args.sim_steps)
        g.sync()
        g.kernel_time(reset=True)
        before = g.stats()
        for _ in range(args.steps):
            g.step(args.sim_steps)
        g.sync()
        ms, launches = g.kernel_time()
        after = g.stats()
        out = {"multiversion": bool(on), "kernel_ms_per_step": ms / args.steps, "launches": launches,
               "msgs_per_s": (after.delivered_total - before.delivered_total) / (ms / 1e3)}
        if on:
            g.consensus()
            t0 = time.perf_counter()
            failed, versions, dropped = g.consensus()
            out["scan_s"] = time.perf_counter() - t0
            rows = cfg.keys * abi.n_replicas(cfg) * cfg.clusters
            out["scan"] = {"failed": failed, "versions": versions, "dropped": dropped}
            out["scan_bytes"] = 4 * (rows + versions - dropped)
            out["scan_gb_per_s"] = out["scan_bytes"] / out["scan_s"] / 1e9
            out["device_bytes"] = g.device_bytes()
        return out


def main():
    ap = argparse.ArgumentParser()
    d = bench.DEFAULTS[2]
    ap.add_argument("--clusters", type=int, default=d["clusters"])
    ap.add_argument("--sim-steps", type=int, default=d["sim_steps"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--versions", type=int, default=64, help="values kept per (key, replica, cluster)")
    args = ap.parse_args()
    args.window, args.mbox, args.kv = d["window"], d["mbox"], 1
    runs = [run(args, on) for on in (False, True, True, False)]
    off = [r["kernel_ms_per_step"] for r in runs if not r["multiversion"]]
    on = [r["kernel_ms_per_step"] for r in runs if r["multiversion"]]
    print(json.dumps({"build_id": sim.build_id(), "clusters": args.clusters, "sim_steps": args.sim_steps,
                      "steps": args.steps, "warmup": args.warmup, "bins": args.bins, "versions": args.versions,
                      "runs": runs, "off_ms": off, "on_ms": on,
                      "on_cost_percent": 100.0 * (sum(on) / sum(off) - 1.0)}))


if __name__ == "__main__":
    main()
