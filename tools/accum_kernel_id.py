#!/usr/bin/env python3
"""Identity of the accumulating (MODE 3), adaptive (MODE 4) and spectral (MODE 5) render kernels, the way tools/kernel_id.py identifies the production
(MODE 0) ones: sha256 of each kernel's position-independent machine code in the gfx950 code object of a library, and sha256 of its
body in an ISA listing (comments and file / ident / loc directives removed).  kernel_id.py's own output is left to the production
kernels (bench.py reads it).

Usage: python tools/accum_kernel_id.py [--against OTHER_LIB OTHER_LISTING]
  prints the hashes of MODE 0, 3, 4 and 5 of the in-tree build; with --against, also those of another build (e.g. the parent commit's)
  and whether the MODE 0, 3 and 4 kernels are unchanged (exit status 1 if one differs; a build without MODE 4 compares 0 and 3 only)."""
import hashlib
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_id as K  # noqa: E402

SYM = re.compile(r"^_ZN3srt13render_kernelILi([0345])ELb([01])ELb([01])ELb([01])EEEvNS_12RenderParamsE$")
LABEL = re.compile(r"^_ZN3srt13render_kernelILi([0345])ELb([01])ELb([01])ELb([01])EEEvNS_12RenderParamsE:")


def code_hashes(lib):
    """{(mode, narrow, all_cached, paired): sha256 of the position-independent machine code}"""
    out = {}
    data = open(lib, "rb").read()
    pos = data.find(K.BUNDLE_MAGIC)
    while pos >= 0:
        n, = K.struct.unpack_from("<Q", data, pos + len(K.BUNDLE_MAGIC))
        o = pos + len(K.BUNDLE_MAGIC) + 8
        for _ in range(min(n, 16)):
            off, size, tlen = K.struct.unpack_from("<QQQ", data, o)
            triple = data[o + 24:o + 24 + tlen]
            o += 24 + tlen
            if b"gfx950" in triple and size:
                for name, code in K._elf_function_bytes(data[pos + off:pos + off + size]).items():
                    m = SYM.match(name)
                    if m:
                        out[tuple(int(g) for g in m.groups())] = hashlib.sha256(K.position_independent(code)).hexdigest()
        pos = data.find(K.BUNDLE_MAGIC, pos + 1)
    return out


def listing_hashes(path):
    """{(mode, narrow, all_cached, paired): sha256 of the kernel's body in the ISA listing}"""
    out, h, key = {}, None, None
    if not os.path.exists(path):
        return out
    for line in open(path, errors="replace"):
        if h is None:
            m = LABEL.match(line)
            if not m:
                continue
            h, key = hashlib.sha256(), tuple(int(g) for g in m.groups())
        body = re.sub(r";.*$", "", line).rstrip()
        if body and not re.match(r"\s*\.(file|ident|loc)\b", body):
            h.update(body.encode() + b"\n")
        if re.match(r"\s*s_endpgm", body):
            out[key] = h.hexdigest()
            h = None
    return out


def name(key):
    mode, narrow, cached, paired = key
    return "render_kernel<%d,%d,%d%s>" % (mode, narrow, cached, ",paired" if paired else "")


def main(argv):
    here = (code_hashes(K.LIB), listing_hashes(K.ISA))
    other = None
    if len(argv) == 3 and argv[0] == "--against":
        other = (code_hashes(argv[1]), listing_hashes(argv[2]))
    differ = 0
    checked = (0, 3, 4) if other is not None and any(x[0] == 4 for x in other[0]) else (0, 3)
    for kind, k in (("code", 0), ("listing", 1)):
        for key in sorted(here[k]):
            line = "%-7s %-28s %s" % (kind, name(key), here[k][key])
            if other is not None and key[0] in checked:
                same = other[k].get(key) == here[k][key]
                differ += 0 if same else 1
                line += "  %s" % ("same as the other build" if same else "DIFFERS from the other build (%s)" % other[k].get(key))
            print(line)
    if other is not None:
        for k in (0, 1):
            missing = sorted(set(x for x in other[k] if x[0] in checked) - set(here[k]))
            differ += len(missing)
            for key in missing:
                print("missing %s" % name(key))
        print("MODE %s kernels: %s" % (", ".join(str(m) for m in checked), "unchanged" if differ == 0 else "%d hashes differ" % differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
