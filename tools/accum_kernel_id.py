#!/usr/bin/env python3
"""Compares the render kernels of two builds: every instantiation of render_kernel (every mode x six shapes), by the sha256 of its
position-independent machine code in the gfx950 code object of the library and of its body in the ISA listing (both from
tools/kernel_id.py, whose own output stays with the production MODE 0 kernels: bench.py reads it).

Usage: python tools/accum_kernel_id.py [--against OTHER_LIB OTHER_LISTING]
  prints the hashes of the in-tree build; with --against, also whether each kernel that the other build (e.g. the parent commit's)
  holds too is unchanged (exit status 1 if one differs or is missing here)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_id as K  # noqa: E402


def name(key):
    mode, narrow, cached, paired = key
    return "render_kernel<%d,%d,%d%s>" % (mode, narrow, cached, ",paired" if paired else "")


def main(argv):
    here = (K.render_code_hashes(K.LIB, K.RENDER_ALL), K.render_listing_hashes(K.ISA, K.RENDER_ALL))
    other = None
    if len(argv) == 3 and argv[0] == "--against":
        other = (K.render_code_hashes(argv[1], K.RENDER_ALL), K.render_listing_hashes(argv[2], K.RENDER_ALL))
    differ = 0
    for kind, k in (("code", 0), ("listing", 1)):
        for key in sorted(here[k]):
            line = "%-7s %-28s %s" % (kind, name(key), here[k][key])
            if other is not None and key in other[k]:
                same = other[k][key] == here[k][key]
                differ += 0 if same else 1
                line += "  %s" % ("same as the other build" if same else "DIFFERS from the other build (%s)" % other[k][key])
            print(line)
    if other is not None:
        for k in (0, 1):
            missing = sorted(set(other[k]) - set(here[k]))
            differ += len(missing)
            for key in missing:
                print("missing %s" % name(key))
        modes = sorted(set(key[0] for k in (0, 1) for key in other[k] if key in here[k]))
        print("MODE %s kernels (%d instantiations): %s" % (", ".join(str(m) for m in modes), len(set(other[0]) & set(here[0])),
                                                         "unchanged" if differ == 0 else "%d hashes differ" % differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
