"""From "how many clusters" to the failing clusters' message traces, in one command.

    python tools/triage.py --config 2 --clusters 65536 --steps 300 --find stalled [--max-traces 4] --out DIR

Pass 1 runs a BASELINE config (bench.py's workloads), prints verdict_counts and finds on the device
the clusters that match a named predicate:

    stalled     a worker waits for a reply and no message is in flight anywhere
    agree       replicas disagree, in a cluster the bounded model still speaks for (not UNFAITHFUL or POISON)
    flagged     any PAXISIM_F_* flag
    poison      the Go reference would panic
    lin         (ABD, config 3) the replica-side history has an anomaly

or --any / --none masks given in hex.  Pass 2 re-runs each found cluster (at most --max-traces of
them) as a one-cluster handle with the same global id - the PRNG is keyed by it, so the run is the
same - with the device recorder on, and writes DIR/cluster_<id>/<src>-<dst>.gob and schedule.json
through paxi_amd.trace.export, the files tools/trace_cli.py replay reads.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from paxi_amd import abi, trace  # noqa: E402

PREDICATES = {
    "stalled": (abi.V_STALLED, 0),
    "agree": (abi.V_AGREE, abi.F_UNFAITHFUL | abi.F_POISON),
    "flagged": (abi.V_FLAGS, 0),
    "poison": (abi.F_POISON, 0),
    "lin": (abi.V_LIN, 0),
}


def triage(args, out=print):
    import bench
    from paxi_amd.sim import Simulation
    d = bench.DEFAULTS[args.config]
    ns = argparse.Namespace(window=d["window"], mbox=d["mbox"], history=512, kv=1, crash_step=args.crash_step)
    cfg, wl, fp, faults, desc = bench.workload(args.config, args.clusters, 0, 0, ns)
    any_, none = PREDICATES[args.find] if args.find else (int(args.any, 16), int(args.none, 16))
    scans = (any_ | none) & abi.V_SCANS
    with Simulation(cfg, wl, fp, faults) as g:                 # pass 1: which clusters
        g.step(args.steps)
        counts = g.verdict_counts(scans=scans)
        ids, total = g.find(any_, none=none, scans=scans, cap=args.max_ids)
    out(f"{desc['workload']}: {cfg.clusters} clusters after {args.steps} steps")
    out("  " + "  ".join(f"{k} {v}" for k, v in counts.items() if v))
    out(f"  {total} clusters match any 0x{any_:x} none 0x{none:x}; first ids: {[int(c) for c in ids[:16]]}")
    result = {"counts": counts, "total": total, "ids": [int(c) for c in ids], "traced": []}
    for c in result["ids"][:args.max_traces]:                  # pass 2: one small handle per found cluster
        cfg.clusters, cfg.cluster_base = 1, int(c)
        with Simulation(cfg, wl, fp, faults) as g:
            g.latency_enable(16)                               # the recording step kernels
            g.trace_enable([0], args.records or 64 * args.steps)
            g.step(args.steps)
            word = int(g.verdicts(scans=scans)[0])
            tr = trace.from_device(g, 0, 0, args.steps)
            outdir = os.path.join(args.out, f"cluster_{c}")
            os.makedirs(outdir, exist_ok=True)
            streams, _ = trace.export(g, 0, tr, outdir=outdir)
        out(f"  cluster {c}: word 0x{word:x}, {len(tr['msgs'])} messages on {len(streams)} links -> {outdir}")
        result["traced"].append({"cluster": int(c), "word": word, "messages": len(tr["msgs"]), "dir": outdir})
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "triage.json"), "w") as f:
            json.dump(result, f)
    return result


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", type=int, default=2, choices=[2, 3, 4, 5])
    ap.add_argument("--clusters", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--crash-step", type=int, default=100)
    ap.add_argument("--find", choices=sorted(PREDICATES))
    ap.add_argument("--any", default="0", help="hex mask, when --find is not given")
    ap.add_argument("--none", default="0", help="hex mask, when --find is not given")
    ap.add_argument("--max-ids", type=int, default=None, help="ids to read back (default: all)")
    ap.add_argument("--max-traces", type=int, default=4)
    ap.add_argument("--records", type=int, default=0, help="records kept per replica (default 64 per step)")
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    triage(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
