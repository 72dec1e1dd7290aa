"""Regenerates the stored outputs of the reference's own compiled functions that tests/test_ref_host.py and tests/test_ref_tables.py
compare the product with: ref_host_vectors.json and ref_arrays.npz (host code: rotation matrix, argument parser, run log, BMP
writer, constant tables) and, with --sellmeier, ref_sellmeier.npz (the reference's sellmeier_index run on the GPU).

It loads the oracle/_ref libraries (oracle/Makefile target `ref`, built from the reference sources by __graft_entry__.build() where
those are present) and calls them on exactly the inputs the tests generate (the tests' own case functions).  Regenerate only when a
test's inputs change on purpose:

    python tests/golden/make_ref_vectors.py [--out DIR]               # host vectors (no GPU)
    python tests/golden/make_ref_vectors.py --sellmeier [--out DIR]   # Sellmeier vectors (needs a GPU)
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.path.join(ROOT, "oracle", "_ref")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_ref_host as H      # noqa: E402
import test_ref_tables as T    # noqa: E402


def _lib(name):
    path = os.path.join(REF, name)
    if not os.path.exists(path):
        raise SystemExit("%s not built (oracle/Makefile target `ref`)" % path)
    return C.CDLL(path)


def host_vectors(out):
    R, I, Tb = _lib("libref_host.so"), _lib("libref_image.so"), _lib("libref_tables.so")
    fp = C.POINTER(C.c_float)
    arrays = {}
    # constant tables
    for name, n in [(k, T.N) for k in T.TABLES] + [("d65_XYZ_to_sRGB", 9)]:
        arrays["table_" + name] = np.ctypeslib.as_array((C.c_float * n).in_dll(Tb, name)).copy().view(np.uint32)
    # rotation matrices
    cases = H.rotation_cases()
    mats = []
    for axis, th, start in cases:
        a = start.copy()
        assert R.ref_rot_matrix(C.c_float(float(th)), axis, a.ctypes.data_as(fp)) == 0
        mats.append(a.view(np.uint32))
    arrays["rot_matrix_bits"] = np.stack(mats)
    arrays["rot_inputs_sha256"] = np.array(H.rotation_inputs_digest(cases))
    np.savez_compressed(os.path.join(out, "ref_arrays.npz"), **arrays)

    doc = {"_source": "outputs of the reference's own functions compiled unmodified (oracle/_ref, oracle/Makefile target `ref`) on the "
                      "inputs of tests/test_ref_host.py; written by tests/golden/make_ref_vectors.py",
           "parse_args": {}, "run_log": {}, "bmp": []}
    R.ref_parse_args.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(H.Params)]
    for argv in H.ARGV_TABLE:
        full = [b"prog"] + [a.encode() for a in argv]
        p = H.Params()
        assert R.ref_parse_args(len(full), (C.c_char_p * len(full))(*full), C.byref(p)) == 0
        doc["parse_args"][H.argv_key(argv)] = {"argv": argv, "params": H.params_to_json(p.as_dict())}
    with tempfile.TemporaryDirectory() as tmp:
        for k, (title, subdir) in enumerate(H.LOG_CASES):
            d = Path(tmp) / ("log%d" % k)
            d.mkdir()
            doc["run_log"]["%s|%s" % (title, subdir)] = list(H.run_log(R.ref_log_to_file, d, title, subdir, H.LOG_ENTRIES))
        for k, (w, h, planes) in enumerate(H.bmp_cases()):
            d = Path(tmp) / ("bmp%d" % k)
            d.mkdir()
            data = H.save_image(I.ref_save_image, d, planes, w, h, "img %d.bmp" % k)
            doc["bmp"].append({"width": w, "height": h, "planes_sha256": H.inputs_digest(*planes), "length": len(data),
                               "sha256": hashlib.sha256(data).hexdigest(), "header": data[:54].hex()})
    with open(os.path.join(out, "ref_host_vectors.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def sellmeier_vectors(out):
    fp = C.POINTER(C.c_float)
    L, Lc = _lib("libref_sellmeier.so"), _lib("libref_sellmeier_contract.so")
    for lib in (L, Lc):
        lib.ref_sellmeier_run.argtypes = [fp, fp, fp, C.c_uint, fp]
    cases = T.sellmeier_cases()
    ref, ref_c = [], []
    for b, c, lam in cases:
        for lib, dst in ((L, ref), (Lc, ref_c)):
            o = np.zeros(lam.size, np.float32)
            assert lib.ref_sellmeier_run(b.ctypes.data_as(fp), c.ctypes.data_as(fp), lam.ctypes.data_as(fp), lam.size, o.ctypes.data_as(fp)) == 0
            dst.append(o.view(np.uint32))
    ref, ref_c = np.stack(ref), np.stack(ref_c)
    # the contracted build differs from the other in a few per cent of the values: stored as the XOR of the two, it compresses to little
    np.savez_compressed(os.path.join(out, "ref_sellmeier.npz"), ref_bits=ref, ref_contract_xor=ref ^ ref_c,
                        inputs_sha256=np.array(T.sellmeier_inputs_digest(cases)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--sellmeier", action="store_true", help="the Sellmeier vectors (runs the reference's device function: needs a GPU)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    (sellmeier_vectors if a.sellmeier else host_vectors)(a.out)


if __name__ == "__main__":
    main()
