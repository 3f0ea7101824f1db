"""The multi-version Database's yardstick (tests/mv_ref.py) and host-side pieces, on the CPU: the
oracle-derived histories are self-consistent on every shape the GPU suite uses, a 16-cluster slice
equals the same clusters of one large oracle handle, the Consensus loop agrees with a direct
restatement, and include/paxisim.h and paxi_amd/abi.py agree on the new prototypes."""
import ctypes as C
import os
import re

import pytest

import mv_ref
import oracle_lib as ol
from paxi_amd import abi
from paxi_amd.sim import consensus_of_histories

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(mv_ref.SHAPES))
def test_yardstick_is_self_consistent(name):
    """The last value of History(r, k) is what the replica's Database holds at k (nil when it never
    put one), and the lengths add up to the replicas' executed_writes."""
    cfg = mv_ref.SHAPES[name][0]()[0]
    r = mv_ref.ref(name)
    N = abi.n_replicas(cfg)
    assert len(r.hist) == cfg.clusters * N * cfg.keys
    for (c, rep), db in r.kv.items():
        assert db == [(r.hist[(c, rep, k)] or [0])[-1] for k in range(cfg.keys)], (c, rep)
    assert sum(len(h) for h in r.hist.values()) == r.executed_writes > 0


def test_slice_equals_the_clusters_of_a_large_handle():
    """Clusters [56, 72) of a 200-cluster oracle equal a 16-cluster oracle at cluster_base 56 (a
    cluster's PRNG is keyed by its global id), state for state and Database for Database."""
    cfg, wl, fp, faults = mv_ref.SHAPES["paxos5"][0]()
    big = ol.OracleSim(cfg, wl, fp, faults)
    big.step(300)
    r = mv_ref.ref("paxos5")
    N = 5
    assert [s.as_tuple() for s in big.read_state(56, 16)] == r.states[56 * N: 72 * N]
    assert [s.as_tuple() for s in big.read_state()] == r.states
    for c in range(56, 72):
        for rep in range(N):
            assert big.read_kv(c, rep, cfg.keys) == r.kv[(c, rep)]
    big.close()


@pytest.mark.parametrize("rows,want", [
    ([[1, 2, 3], [1, 2, 3, 4, 5], [1, 2]], (True, None)),          # prefixes of one another
    ([[1, 2, 3, 4], [1, 2, 9, 4], [1, 2, 3]], (False, 2)),         # two lists differ at index 2
    ([[1, 2, 3, 4], [], [1, 2, 3]], (True, None)),                 # an empty list constrains nothing
    ([[], [], []], (True, None)),
    ([[7], [8]], (False, 0)),
    ([[1, 5, 3], [1, 2], [1, 2, 4]], (False, 1)),                  # the lowest failing index, not the first pair's
    ([[1, 2, 3], [1, 2], [1, 2, 4]], (False, 2)),                  # fails only beyond the shortest list
])
def test_consensus_loop_agrees_with_a_direct_restatement(rows, want):
    assert consensus_of_histories(rows) == want
    assert mv_ref.direct(rows) == want


def test_verdict_over_prefixes():
    hist = {(0, 0, 0): [1, 2, 3], (0, 1, 0): [1, 2, 4], (0, 0, 1): [5], (0, 1, 1): []}
    v = mv_ref.verdict(hist, 1, 2, 2)
    assert (v.failed, v.versions, v.dropped, v.masks, v.first, v.longest) == (1, 7, 0, [1], {(0, 0): 2}, 3)
    v = mv_ref.verdict(hist, 1, 2, 2, cap=2)
    assert (v.failed, v.versions, v.dropped, v.masks, v.first) == (0, 7, 2, [0], {})


MV_CALLS = ("paxisim_multiversion_enable", "paxisim_kv_history", "paxisim_consensus", "paxisim_consensus_failed")
_CTYPES = {"paxisim*": C.c_void_p, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
           "uint32_t*": C.POINTER(C.c_uint32), "uint64_t*": C.POINTER(C.c_uint64)}


def test_header_and_abi_agree_on_the_new_prototypes():
    hdr = open(os.path.join(ROOT, "include", "paxisim.h")).read()
    assert int(re.search(r"#define PAXISIM_MV_MAX \(1u << (\d+)\)", hdr).group(1)) == abi.MV_MAX.bit_length() - 1
    assert f"#define PAXISIM_ABI_VERSION {abi.ABI_VERSION}" in re.sub(r"[ \t]+", " ", hdr)
    for name in MV_CALLS:
        res, args = abi.PROTOTYPES[name]
        assert res is C.c_int
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared"
        types = []
        for param in m.group(1).split(","):
            words = param.replace("*", " * ").split()
            words = [w for w in words[:-1] if w != "const"]      # drop the parameter's name
            types.append("".join(words))
        assert [_CTYPES[t] for t in types] == args, name
    pinned = open(os.path.join(ROOT, "paxi_amd", "guard", "pinned", "242a73e", "include", "paxisim.h")).read()
    assert pinned == hdr


def test_library_exports_the_new_calls():
    from paxi_amd import sim
    L = sim.load_library()
    for name in MV_CALLS:
        assert name in sim.EXPORTED
        assert getattr(L, name).argtypes == abi.PROTOTYPES[name][1]
