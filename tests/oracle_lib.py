"""Test-side loader for the CPU oracle (oracle/liboracle_paxisim.so).

The oracle is test infrastructure: only tests/, __graft_entry__.smoke() and
bench.py's cpu_baseline leg load it, and only as the checker.
"""
import ctypes as C
import os

from paxi_amd import abi
from paxi_amd.sim import Handle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SO = os.path.join(ROOT, "oracle", "liboracle_paxisim.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(ORACLE_SO):
            raise RuntimeError(f"oracle not built: run `make -C oracle` ({ORACLE_SO})")
        _lib = abi.bind(C.CDLL(ORACLE_SO), "oracle")
    return _lib


def _check(rc):
    if rc != 0:
        raise RuntimeError(f"oracle error {rc}: {lib().oracle_last_error().decode()}")


class OracleSim(Handle):
    """Same surface as paxi_amd.sim.Simulation, backed by the CPU restatement."""
    _library = staticmethod(lib)
    _raise_on = staticmethod(_check)

    def step(self, n, threads=1):
        _check(lib().oracle_step(self.h, n, threads))

    def set_replica_order(self, mode):
        """Test hook: 0 = index order, 1 = reversed, 2 = shuffled per (cluster, step)."""
        _check(lib().oracle_set_replica_order(self.h, mode))

    def commands(self, cluster, cids):
        return [self.command(cluster, c) for c in cids]

    def command(self, cluster, cid):
        """(key, is_write) of command `cid` of a cluster, as the workers draw it."""
        k, w = C.c_uint32(), C.c_uint32()
        _check(lib().oracle_command(self.h, cluster, cid, C.byref(k), C.byref(w)))
        return k.value, bool(w.value)

    def exec_log(self, cluster, replica, key=0):
        rk = replica | (key << 16)
        n = C.c_uint32()
        _check(lib().oracle_exec_log(self.h, cluster, rk, None, 0, C.byref(n)))
        buf = (C.c_uint32 * max(1, n.value))()
        _check(lib().oracle_exec_log(self.h, cluster, rk, buf, n.value, C.byref(n)))
        return list(buf[: n.value])

    def linearizable(self):
        a, n = C.c_uint64(), C.c_uint64()
        _check(lib().oracle_lin_check(self.h, C.byref(a), C.byref(n)))
        return a.value, n.value


def new_ballot(n, zone, node):
    return lib().oracle_new_ballot(n, zone, node)


def ballot_next(b, zone, node):
    return lib().oracle_ballot_next(b, zone, node)


def quorum(kind, npz, mask, fz=0):
    arr = (C.c_uint32 * len(npz))(*npz)
    return bool(lib().oracle_quorum(kind, fz, len(npz), arr, mask))


def linearizable(ops):
    """ops: list of (input, output, start, end) with None for nil (operation.go)."""
    flat = []
    for i, o, s, e in ops:
        flat += [0 if i is None else 1, 0 if i is None else i, 0 if o is None else 1, 0 if o is None else o, s, e]
    arr = (C.c_int64 * len(flat))(*flat)
    n = lib().oracle_linearizable(arr, len(ops))
    if n < 0:
        raise RuntimeError("linearizable failed")
    return n
