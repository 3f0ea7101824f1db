"""Snapshots of a Simulation as files and what their headers say.

A snapshot is the blob `Simulation.snapshot()` returns: a numpy uint8 array in the format of
include/paxisim_snapshot.h.  `info` parses its header on the host - no GPU needed -, `save` and
`load` move the raw blob, and nothing else, to and from a file.
"""
import ctypes as C

import numpy as np

from . import abi
from .sim import _check, load_library


def _blob(blob):
    if isinstance(blob, np.ndarray):
        return np.ascontiguousarray(blob.view(np.uint8).reshape(-1))
    return np.frombuffer(bytes(blob), dtype=np.uint8)


def info(blob):
    """What the blob's header says (paxisim_snapshot_info): protocol, N, clusters, cluster_base,
    step, build id, the recorders present, each section's byte size and mailbox_records."""
    b = _blob(blob)
    out = abi.SnapshotInfo()
    _check(load_library().paxisim_snapshot_info(b.ctypes.data_as(C.c_void_p), b.nbytes, C.byref(out)))
    return {
        "version": out.version, "protocol": out.protocol, "N": out.n_replicas, "clusters": out.clusters,
        "cluster_base": out.cluster_base, "step": out.step, "build_id": out.build_id.decode(),
        "plan_hash": out.plan_hash, "total_bytes": out.total_bytes, "mailbox_records": out.mailbox_records,
        "faults": out.n_faults,
        "recorders": {"latency": bool(out.recorders & abi.SNAP_HAS_LAT),
                      "client_history": bool(out.recorders & abi.SNAP_HAS_CHIST),
                      "multiversion": bool(out.recorders & abi.SNAP_HAS_MV),
                      "trace": bool(out.recorders & abi.SNAP_HAS_TRACE)},
        "sections": {name: out.section_bytes[i] for i, name in enumerate(abi.SNAPSHOT_SECTIONS)},
    }


def save(path, blob):
    """Write the raw blob to `path`."""
    _blob(blob).tofile(path)


def load(path):
    """The raw blob of `path` as a numpy uint8 array."""
    return np.fromfile(path, dtype=np.uint8)
