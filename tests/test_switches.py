"""The compile-time switches of the step kernels and their one list.

Every PXS_* name that a preprocessor conditional of paxi_amd/csrc tests, or that a -D flag of
__graft_entry__ sets, has a row in DESIGN.md's table of remaining switches; and no switch of the
retired list below that table occurs anywhere under paxi_amd/csrc, so a retired experiment cannot
come back without its row.  Reads sources only: no build, no GPU."""
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

NAME = re.compile(r"PXS_[A-Z0-9_]+")
CSRC = sorted(glob.glob(os.path.join(ROOT, ge.CSRC, "*.h")) + glob.glob(os.path.join(ROOT, ge.CSRC, "*.hip")))


def design_lists():
    """(names in the first column of the table, names that head an entry of the retired list)."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 5.21 Compile-time switches"):]
    sec = sec[:sec.index("\n## ")]
    table, retired = sec.split("**Retired.**")
    kept = set()
    for line in table.splitlines():
        if line.startswith("| `PXS_"):
            kept.update(NAME.findall(line.split("|")[1]))
    gone = set()
    for line in retired.splitlines():
        if line.startswith("- `PXS_"):
            gone.update(NAME.findall(line.split("(")[0]))
    return kept, gone


def conditional_names():
    """PXS_* names in #if / #ifdef / #ifndef / #elif lines of the product sources."""
    names = {}
    for path in CSRC:
        text = open(path).read().replace("\\\n", " ")
        for line in text.splitlines():
            if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                for n in NAME.findall(line):
                    names.setdefault(n, os.path.basename(path))
    return names


def flag_names():
    """PXS_* names in the -D flags __graft_entry__ compiles anything with."""
    flags = list(ge.HIP_FLAGS) + list(ge.LAT_FLAGS)
    for extra in list(ge.TU_FLAGS.values()) + list(ge.GUARDS.values()):
        flags += extra
    return {n for f in flags if f.startswith("-D") for n in NAME.findall(f)}


def test_lists_are_read():
    kept, gone = design_lists()
    assert "PXS_ABSORB_MAX" in kept and "PXS_LAT" in kept and len(kept) >= 20, sorted(kept)
    assert "PXS_FLUSH_LATE" in gone and "PXS_LANE_ASYNC" in gone and len(gone) >= 30, sorted(gone)
    assert conditional_names() and flag_names() >= {"PXS_LAT", "PXS_SHAPE", "PXS_PIPE_PERSIST"}


def test_every_switch_in_use_has_a_row_in_the_design_table():
    kept, _ = design_lists()
    missing = {n: where for n, where in conditional_names().items() if n not in kept}
    missing.update({n: "__graft_entry__" for n in flag_names() if n not in kept})
    assert not missing, f"PXS_* switches without a row in DESIGN.md §5.21: {missing}"


def test_no_retired_switch_under_csrc():
    _, gone = design_lists()
    found = {}
    for path in CSRC:
        for n in set(NAME.findall(open(path).read())) & gone:
            found.setdefault(n, []).append(os.path.basename(path))
    assert not found, f"retired switches (DESIGN.md §5.21) named under {ge.CSRC}: {found}"
