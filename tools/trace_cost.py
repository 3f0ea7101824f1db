"""What the device message trace costs the recording step kernels.

Runs BASELINE config 2's shape (bench.py workload(2): Multi-Paxos 5 replicas, Drop/Slow faults, 1M
clusters) with kv = 1 and latency recording on in four states, each a fresh handle, in mirrored
order (lat, one, trace, closed, closed, trace, one, lat):
  lat     latency only
  one     one cluster traced: every replica-step looks its cluster up in the table, the hook itself
          runs in one lane of one tile
  trace   --traced clusters of the handle traced (spread evenly over it), every step recorded
  closed  the same clusters traced, the step window closed before the timed steps
and times the step launches with paxisim_kernel_time.  Prints one JSON line: ms per bench step of
each run, the costs against latency only, the records kept and dropped, and the library's build id.
usage: python tools/trace_cost.py [--clusters N] [--steps K] [--warmup W] [--bins B] [--traced T] [--records R]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from paxi_amd import sim  # noqa: E402


def run(args, state):
    cfg, wl, fp, faults, _ = bench.workload(2, args.clusters, 0, 0, args)
    with sim.Simulation(cfg, wl, fp, faults) as g:
        g.latency_enable(args.bins)
        if state != "lat":
            stride = max(1, cfg.clusters // args.traced)
            ids = [cfg.clusters // 2] if state == "one" else list(range(0, cfg.clusters, stride))[:args.traced]
            g.trace_enable(ids, args.records, 0, 1 if state == "closed" else 2**32 - 1)
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
        out = {"state": state, "kernel_ms_per_step": ms / args.steps, "launches": launches,
               "msgs_per_s": (after.delivered_total - before.delivered_total) / (ms / 1e3)}
        if state != "lat":
            out["records"], out["dropped"] = g.trace_totals()
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
    ap.add_argument("--traced", type=int, default=1024, help="clusters traced")
    ap.add_argument("--records", type=int, default=4096, help="records kept per (traced cluster, replica)")
    args = ap.parse_args()
    args.window, args.mbox, args.kv = d["window"], d["mbox"], 1
    order = ("lat", "one", "trace", "closed", "closed", "trace", "one", "lat")
    runs = [run(args, s) for s in order]
    ms = {s: [r["kernel_ms_per_step"] for r in runs if r["state"] == s] for s in ("lat", "one", "trace", "closed")}
    cost = {s: 100.0 * (sum(ms[s]) / sum(ms["lat"]) - 1.0) for s in ("one", "trace", "closed")}
    print(json.dumps({"build_id": sim.build_id(), "clusters": args.clusters, "sim_steps": args.sim_steps,
                      "steps": args.steps, "warmup": args.warmup, "bins": args.bins, "traced": args.traced,
                      "records": args.records, "runs": runs, "ms": ms, "cost_percent": cost}))


if __name__ == "__main__":
    main()
