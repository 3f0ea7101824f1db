"""Where the step kernels and the compaction kernels of bench.py's timed window ran, from a
rocprofv3 kernel trace: per stream the step launches' start and end, the share
of the window in which at least one step kernel ran, the share in which two did, and how much of
the compaction kernels' time (cmp_*, ph_*, pipe_verify) ran beside a step kernel of another stream.
usage: python tools/pool_trace.py <kernel_trace.csv> <timed step launches> [launches listed per stream]"""
import csv
import json
import sys


def union(iv):
    iv = sorted(iv)
    out = []
    for a, b in iv:
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out


def length(iv):
    return sum(b - a for a, b in iv)


def inter(x, y):
    """Length of the intersection of two sorted disjoint interval lists."""
    i = j = 0
    s = 0
    while i < len(x) and j < len(y):
        a, b = max(x[i][0], y[j][0]), min(x[i][1], y[j][1])
        if b > a:
            s += b - a
        if x[i][1] < y[j][1]:
            i += 1
        else:
            j += 1
    return s


rows = list(csv.DictReader(open(sys.argv[1])))
timed = int(sys.argv[2])
show = int(sys.argv[3]) if len(sys.argv) > 3 else 10
key = "Stream_Id" if rows and "Stream_Id" in rows[0] else "Queue_Id"
for r in rows:
    r["a"], r["b"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
step = sorted((r for r in rows if "sim_serial" in r["Kernel_Name"] or "sim_steps" in r["Kernel_Name"]), key=lambda r: r["a"])
step = step[-timed:]
lo, hi = step[0]["a"], max(r["b"] for r in step)
win = hi - lo
streams = sorted({r[key] for r in step})
per = {s: union([(r["a"], r["b"]) for r in step if r[key] == s]) for s in streams}
busy = union([(r["a"], r["b"]) for r in step])
both = sum(inter(per[s], per[t]) for i, s in enumerate(streams) for t in streams[i + 1:])
small = [r for r in rows if r["a"] >= lo and r["b"] <= hi and "sim_s" not in r["Kernel_Name"] and
         any(k in r["Kernel_Name"] for k in ("cmp_", "ph_", "pipe_verify"))]
beside = 0
for r in small:
    others = union([iv for s in streams if s != r[key] for iv in per[s]])
    beside += inter([[r["a"], r["b"]]], others)
out = {
    "stream_key": key, "streams": streams, "timed_step_launches": len(step), "window_ms": win / 1e6,
    "step_kernel_busy_share": length(busy) / win, "no_step_kernel_share": 1 - length(busy) / win,
    "two_step_kernels_share": both / win,
    "step_launch_ms_mean": sum(r["b"] - r["a"] for r in step) / len(step) / 1e6,
    "compaction_kernels": len(small), "compaction_kernels_ms": sum(r["b"] - r["a"] for r in small) / 1e6,
    "compaction_share_of_window": sum(r["b"] - r["a"] for r in small) / win,
    "compaction_ms_beside_another_streams_step_kernel": beside / 1e6,
    "launches_ms_from_window_start": {
        s: [[round((r["a"] - lo) / 1e6, 3), round((r["b"] - lo) / 1e6, 3)] for r in step if r[key] == s][:show] for s in streams},
}
print(json.dumps(out, indent=1))
