"""What recording client request latency costs the step kernels.

Runs BASELINE config 2's shape (bench.py workload(2): Multi-Paxos 5 replicas,
Drop/Slow faults, 1M clusters) with latency off and on in mirrored order (off,
on, on, off), each a fresh handle, and times the step launches with
paxisim_kernel_time (HIP events on the launch stream).  Prints one JSON line:
ms per bench step of each run, the on-cost, the histogram's Stat and the
library's build id.  With --history N the "on" runs also record the client-side
op history, N ops per worker, and report the time of
paxisim_client_linearizable over the handle (host wall clock around the call).
usage: python tools/latency_cost.py [--clusters N] [--steps K] [--warmup W] [--bins B] [--history N]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from paxi_amd import sim  # noqa: E402


def run(args, on):
    cfg, wl, fp, faults, _ = bench.workload(2, args.clusters, 0, 0, args)
    with sim.Simulation(cfg, wl, fp, faults) as g:
        if on:
            g.latency_enable(args.bins)
            if args.history:
                g.client_history_enable(args.history)
        for _ in range(args.warmup):
            g.step(args.sim_steps)
        g.sync()
        g.kernel_time(reset=True)
        before = g.stats()
        if on:
            g.latency_reset()
        for _ in range(args.steps):
            g.step(args.sim_steps)
        g.sync()
        ms, launches = g.kernel_time()
        after = g.stats()
        out = {"latency": bool(on), "kernel_ms_per_step": ms / args.steps, "launches": launches,
               "msgs_per_s": (after.delivered_total - before.delivered_total) / (ms / 1e3)}
        if on:
            h = g.latency()
            assert h.count == after.replies - before.replies, (h.count, after.replies - before.replies)
            out["stat_steps"] = h.stat(1.0).as_dict()
            out["overflow"] = h.overflow
        if on and args.history:
            t0 = time.perf_counter()
            anomalies, ops, skipped = g.client_linearizable()
            out["scan_s"] = time.perf_counter() - t0
            out["scan"] = {"anomalies": anomalies, "ops": ops, "skipped": skipped}
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
    ap.add_argument("--history", type=int, default=0, help="also record the client op history, N ops per worker")
    args = ap.parse_args()
    args.window, args.mbox, args.kv = d["window"], d["mbox"], 1
    runs = [run(args, on) for on in (False, True, True, False)]
    off = [r["kernel_ms_per_step"] for r in runs if not r["latency"]]
    on = [r["kernel_ms_per_step"] for r in runs if r["latency"]]
    print(json.dumps({"build_id": sim.build_id(), "clusters": args.clusters, "sim_steps": args.sim_steps,
                      "steps": args.steps, "warmup": args.warmup, "bins": args.bins, "history": args.history, "runs": runs,
                      "off_ms": off, "on_ms": on,
                      "on_cost_percent": 100.0 * (sum(on) / sum(off) - 1.0)}))


if __name__ == "__main__":
    main()
