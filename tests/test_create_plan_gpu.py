"""tests/golden/create_plan.txt against the live library: every case of the fixture is created (no
stepping) with the case's knobs, and what the ABI shows of the plan - occupancy()'s LDS bytes and
staged picks, device_bytes() - equals the record; a refusal raises the recorded code and message.
The fixture carries the kernels' register counts of the build it was recorded on, so a kernel change
that moves them enough to reshape a launch shows up here as a stale fixture (re-record it by the
recipe in its first lines), not as a silent change of G, J or the LDS budget."""
import ctypes as C
import os

import pytest

from paxi_amd import abi
from paxi_amd.sim import Simulation, PaxisimError

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "create_plan.txt")
KNOBS = ["PAXISIM_SERIAL", "PAXISIM_WLDS", "PAXISIM_WCOLOC", "PAXISIM_GROUPS", "PAXISIM_STAGE", "PAXISIM_COMPACT",
         "PAXISIM_PHASE_SORT", "PAXISIM_PHASE_PERIOD", "PAXISIM_PIPE", "PAXISIM_PIPE_SPIN", "PAXISIM_PIPE_SLOTS",
         "PAXISIM_COMPACT_EVERY", "PAXISIM_POOLS", "PAXISIM_ARENA_PAD_MB", "PAXISIM_ARENA_CONTIG"]


def load_cases(path=FIXTURE):
    """{case name: {key: value}} in the fixture's order."""
    cases, cur = {}, None
    with open(path) as fh:
        for line in fh:
            line = line.rstrip("\n")
            if line.startswith("["):
                cur = cases.setdefault(line[1:-1], {})
            elif line and not line.startswith("#") and cur is not None:
                k, _, v = line.partition("=")
                cur[k] = v
    return cases


def _fill(struct, case, prefix):
    for name, ctype in struct._fields_:
        v = case.get(prefix + name)
        if v is None or name == "move_cdf":
            continue
        if hasattr(ctype, "_length_"):
            arr = getattr(struct, name)
            for i, x in enumerate(v.split(",")):
                arr[i] = int(x)
        else:
            setattr(struct, name, float(v) if ctype is C.c_double else int(v))
    return struct


def inputs_of(case):
    """(Config, Workload, FaultProcess) of a case's recorded inputs."""
    cfg = _fill(abi.Config(), case, "in.cfg.")
    wl = _fill(abi.Workload(), case, "in.wl.")
    if "in.wl.move_cdf" in case:
        vals = [int(x) for x in case["in.wl.move_cdf"].split(",")]
        wl._move_buf = (C.c_uint32 * len(vals))(*vals)   # keeps the tables alive while wl is
        wl.move_cdf = C.cast(wl._move_buf, C.POINTER(C.c_uint32))
    return cfg, wl, _fill(abi.FaultProcess(), case, "in.fp.")


CASES = load_cases()


def test_fixture_is_whole():
    assert len(CASES) >= 50 and sum("err.code" in c for c in CASES.values()) >= 6


@pytest.mark.parametrize("name", list(CASES))
def test_create_matches_fixture(name, monkeypatch):
    case = CASES[name]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.items():
        if k.startswith("knob."):
            monkeypatch.setenv(k[len("knob."):], v)
    cfg, wl, fp = inputs_of(case)
    if "err.code" in case:
        with pytest.raises(PaxisimError) as e:
            Simulation(cfg, wl, fp)
        assert str(e.value) == f"paxisim error {case['err.code']}: {case['err.msg']}"
        return
    with Simulation(cfg, wl, fp) as g:
        _, lds_bytes, staged = g.occupancy()
        assert (lds_bytes, staged) == (int(case["out.P.lds_bytes"]), int(case["out.P.J"]))
        assert g.device_bytes() == int(case["out.total"])
