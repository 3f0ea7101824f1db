"""Client request latency as Paxi reports it (stat.go, benchmark.go:186).

`Simulation.latency()` returns a `Histogram`: the exact per-step counts the
device keeps for one worker or for all workers (include/paxisim.h
paxisim_latency).  A latency is a whole number of virtual
steps; `step_ms` scales it to Paxi's milliseconds.  The percentile rule of
`Statistic()` lives in the C library alone (paxisim_latency_stat_of); `stat`
calls it.
"""
import ctypes as C
from decimal import Decimal

import numpy as np

from . import abi


def go_float(v):
    """A float64 as Go's fmt.Println prints it ('%v'): the shortest digits that
    round-trip, no trailing '.0', exponent form below 1e-4 and from 1e21."""
    d = Decimal(repr(float(v))).normalize()      # repr: the shortest round-trip digits
    if d == 0:
        return "0"
    x = d.adjusted()
    if -4 <= x < 21:
        return format(d, "f")
    digits = "".join(str(k) for k in d.as_tuple().digits)
    m = digits[0] + ("." + digits[1:] if len(digits) > 1 else "")
    return "%s%se%s%02d" % ("-" if d < 0 else "", m, "-" if x < 0 else "+", abs(x))


class Histogram:
    """Latency samples in steps: counts[b] samples of b steps for b < bins,
    `overflow` samples of at least `bins` steps, and the exact count, sum, min
    and max of all of them (min = 2^32-1, max = 0 while empty)."""

    def __init__(self, counts, count=None, total=None, overflow=0, lo=None, hi=None):
        self.counts = np.ascontiguousarray(counts, dtype=np.uint64)
        self.overflow = int(overflow)
        self.count = int(self.counts.sum()) + self.overflow if count is None else int(count)
        nz = np.nonzero(self.counts)[0]
        if total is None or lo is None or hi is None:
            if self.overflow:
                raise ValueError("sum, min and max of overflowed samples must be given")
            total = int((self.counts * np.arange(len(self.counts), dtype=np.uint64)).sum())
            lo = int(nz[0]) if len(nz) else 0xFFFFFFFF
            hi = int(nz[-1]) if len(nz) else 0
        self.sum, self.min, self.max = int(total), int(lo), int(hi)

    @classmethod
    def from_samples(cls, samples, bins):
        """The histogram of a list of latencies in steps."""
        x = np.asarray(samples, dtype=np.int64)
        inside = x[x < bins]
        counts = np.bincount(inside, minlength=bins).astype(np.uint64)
        return cls(counts, len(x), int(x.sum()), int((x >= bins).sum()),
                   int(x.min()) if len(x) else 0xFFFFFFFF, int(x.max()) if len(x) else 0)

    @property
    def bins(self):
        return len(self.counts)

    def _c(self):
        lat = abi.Latency(self.count, self.sum, self.overflow, self.min, self.max, self.bins, 0)
        return lat, self.counts.ctypes.data_as(C.POINTER(C.c_uint64))

    def stat(self, step_ms=1.0):
        """Stat of stat.go:44-66 (paxisim_latency_stat_of), in ms = steps * step_ms."""
        from . import sim
        lat, hist = self._c()
        out = abi.LatencyStat()
        sim._check(sim.load_library().paxisim_latency_stat_of(C.byref(lat), hist, float(step_ms), C.byref(out)))
        return out

    def merge(self, other):
        """Both sets of samples in one histogram."""
        if other.bins != self.bins:
            raise ValueError(f"histograms of {self.bins} and {other.bins} bins")
        return Histogram(self.counts + other.counts, self.count + other.count, self.sum + other.sum,
                         self.overflow + other.overflow, min(self.min, other.min), max(self.max, other.max))

    def samples(self):
        """The sorted samples in steps; only when none overflowed the bins."""
        if self.overflow:
            raise ValueError(f"{self.overflow} samples lie beyond the {self.bins} bins")
        return np.repeat(np.arange(self.bins, dtype=np.int64), self.counts.astype(np.int64))

    def write_file(self, path, step_ms=1.0):
        """Stat.WriteFile (stat.go:25-37): one sorted value in ms per line, as Go's Println prints a float64."""
        if self.overflow:
            raise ValueError(f"{self.overflow} samples lie beyond the {self.bins} bins")
        with open(path, "w") as fh:
            for b in np.nonzero(self.counts)[0]:
                fh.write((go_float(int(b) * float(step_ms)) + "\n") * int(self.counts[b]))

    def __eq__(self, other):
        return (isinstance(other, Histogram) and np.array_equal(self.counts, other.counts) and
                (self.count, self.sum, self.overflow, self.min, self.max) ==
                (other.count, other.sum, other.overflow, other.min, other.max))

    def __repr__(self):
        return (f"Histogram(bins={self.bins}, count={self.count}, sum={self.sum}, overflow={self.overflow}, "
                f"min={self.min}, max={self.max})")
