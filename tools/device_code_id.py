#!/usr/bin/env python3
"""Fingerprint the device code of every translation unit of a source tree.

    python tools/device_code_id.py [ROOT] > listing.txt

For each entry of ROOT's __graft_entry__.product_units() (the default and the PXS_LAT build of
each unit, with its per-unit flags) and for the absorb_oneexit guard unit, compile the unit to
device assembly (--offload-device-only -S) from ROOT with the source as a relative path, drop
the lines that name __hip_cuid_ (a per-compile hash), and print

    unit sha256 instruction-line-count

Two trees whose listings are equal compile to the same device code, unit by unit: a refactor
that only deletes dead source is checked by comparing its listing with its parent's
(profiles/switches).  A host-side build tool: it runs no GPU code and reads nothing but
compiler output.  ROOT defaults to the tree this script is in; the assembly is left under
ROOT/build/device_code_id.
"""
import hashlib
import importlib.util
import os
import sys

OUT_DIR = "build/device_code_id"


def load_entry(root):
    """ROOT's own __graft_entry__, so that the flags and the unit list are that tree's."""
    spec = importlib.util.spec_from_file_location("_graft_entry_of_root", os.path.join(root, "__graft_entry__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def units(ge):
    """(name, compile command) of every unit; the source goes last, as _parallel's weights expect."""
    out = []
    for src, obj, flags in ge.product_units():
        name = os.path.basename(obj)[:-2]
        out.append((name, flags, os.path.join(ge.CSRC, src)))
    pinned = ge._pinned_sources()
    if pinned is not None:
        root = os.path.relpath(ge._send_patched(pinned), ge.ROOT)
        out.append(("guard_absorb_oneexit", ge.HIP_FLAGS + ge.GUARDS["absorb_oneexit"],
                    os.path.join(root, "paxi_amd", "csrc", ge.GUARD_UNIT)))
    return [(name, [ge.HIPCC] + flags + ["--offload-device-only", "-S", "-o", os.path.join(OUT_DIR, name + ".s"), path])
            for name, flags, path in out]


def fingerprint(path):
    """sha256 of the assembly without its __hip_cuid_ lines, and the number of instruction lines."""
    h, n = hashlib.sha256(), 0
    with open(path) as fh:
        for line in fh:
            if "__hip_cuid_" in line:
                continue
            h.update(line.encode())
            s = line.strip()
            if s and s[0] not in ".;" and not s.split(";")[0].rstrip().endswith(":"):
                n += 1
    return h.hexdigest(), n


def main(argv):
    root = os.path.abspath(argv[1]) if len(argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ge = load_entry(root)
    os.makedirs(os.path.join(root, OUT_DIR), exist_ok=True)
    os.makedirs(os.path.join(root, ge.GUARD_OBJ), exist_ok=True)
    todo = units(ge)
    out, sys.stdout = sys.stdout, sys.stderr      # the compile commands' echo goes to stderr
    try:
        ge._parallel([cmd for _, cmd in todo])
    finally:
        sys.stdout = out
    for name, cmd in sorted(todo):
        print(name, *fingerprint(os.path.join(root, cmd[cmd.index("-o") + 1])))


if __name__ == "__main__":
    main(sys.argv)
