"""Sizes and wall times of snapshot, restore and fork at a bench shape.

  python tools/snapshot_bench.py --config 2 [--clusters N] [--warmup 5] [--skip-fork]

Builds bench.py's config (its workload, window, mailbox and launch steps), steps it to where the
bench starts timing (warmup * sim_steps), then prints one JSON line per measurement: the handle's
device bytes and the arithmetic size of the mailbox region, the snapshot's size by section, and the
wall times of snapshot_size, snapshot, restore (a rewind onto the same handle) and fork.  Each
step reports its own failure (a fork that does not fit beside its parent says so with the sizes)
and the run goes on.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(what, fn):
    t = time.perf_counter()
    try:
        out = fn()
    except Exception as e:          # reported, not fatal: the other measurements still run
        emit(what=what, error=str(e), seconds=round(time.perf_counter() - t, 3))
        return None
    emit(what=what, seconds=round(time.perf_counter() - t, 3))
    return out


def main():
    import bench
    from paxi_amd import abi, sim, snapshot
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2, choices=[2, 3, 4, 5])
    ap.add_argument("--clusters", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-fork", action="store_true")
    a = ap.parse_args()
    d = bench.DEFAULTS[a.config]
    args = argparse.Namespace(window=d["window"], mbox=d["mbox"], kv=1, history=512, fz=1,
                              crash_step=a.warmup * d["sim_steps"])
    clusters = a.clusters or d["clusters"]
    cfg, wl, fp, faults, _ = bench.workload(a.config, clusters, 0, 0, args)
    g = sim.Simulation(cfg, wl, fp, faults)
    steps = a.warmup * d["sim_steps"]
    N = abi.n_replicas(cfg)
    D, M = cfg.max_delay + 2, cfg.mbox_cap
    rec_per_cluster = D * N * (N + 1) * M * 16
    timed(f"step {steps}", lambda: (g.step(steps), g.sync()))
    emit(what="handle", config=a.config, clusters=clusters, step=steps, build=sim.build_id(),
         device_bytes=g.device_bytes(), rec_bytes_per_cluster=rec_per_cluster,
         rec_bytes_arithmetic=rec_per_cluster * ((clusters + 63) // 64 * 64), active_clusters=g.active_clusters())
    size = timed("snapshot_size", g.snapshot_size)
    avail = None
    try:
        avail = next(int(ln.split()[1]) * 1024 for ln in open("/proc/meminfo") if ln.startswith("MemAvailable"))
    except (OSError, StopIteration):
        pass
    blob = None
    if size is not None and avail is not None and 2 * size > avail:
        emit(what="snapshot", error="skipped: the blob does not fit twice into the host's available memory",
             snapshot_bytes=size, host_available=avail)
    else:
        blob = timed("snapshot", g.snapshot)
    if blob is not None:
        i = snapshot.info(blob)
        emit(what="blob", total_bytes=i["total_bytes"], mailbox_records=i["mailbox_records"], sections=i["sections"],
             live_share_of_rec=round(i["sections"]["mailbox"] / (rec_per_cluster * clusters), 6))
        before = g.stats().as_dict()
        g.step(d["sim_steps"])
        if timed("restore", lambda: (g.restore(blob), g.sync())) is not None:
            assert g.stats().as_dict() == before, "the rewound handle's stats differ"
        del blob
    if not a.skip_fork:
        f = timed("fork", lambda: (lambda h: (h.sync(), h)[1])(g.fork()))
        if f is not None:
            assert f.stats().as_dict() == g.stats().as_dict(), "the fork's stats differ"
            emit(what="fork", device_bytes=f.device_bytes())
            f.close()
    g.close()


if __name__ == "__main__":
    main()
