#!/usr/bin/env python3
"""Generates tests/golden/ref_vectors_bgv_decrypt.npz by RUNNING THE REFERENCE ITSELF: a small generator of our own
(tests/golden/gen_bgv_decrypt.cpp, linked against oracle/_ref's stock libraries) records BGV ciphertexts, their secret keys and the NativePoly
that PKEBGVRNS::Decrypt (bgvrns-pke.cpp:44-99) returns before decoding, at ring dimension 64 and t = 65537: under FIXEDMANUAL a fresh
ciphertext, a three-element EvalMultNoRelin product and a ciphertext after ModReduce, under the default FLEXIBLEAUTOEXT a fresh ciphertext.
Arrays and meta: see the head of the generator, which fails unless every case has at least two limbs and decodes to the encoded values.
Data only.
Run from the repo root:  python tests/golden/make_golden_bgv_decrypt.py   (needs ./build.sh ref and the reference's sources)
"""
import os
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CASES = ("fm_fresh", "fm_prod", "fm_reduced", "fx_fresh")


def run_generator(ref_src="/root/reference"):
    """compile and run gen_bgv_decrypt.cpp; returns {name: flat uint64 array}"""
    stub = os.path.join(ROOT, "third_party_stubs")
    lib = os.path.join(ROOT, "oracle", "_ref")
    incs = [f"-I{stub}/stub", f"-I{stub}/gen"] + [f"-I{ref_src}/src/{m}/{d}" for m in ("core", "binfhe", "pke") for d in ("include", "lib")]
    flags = "-std=c++17 -O2 -DNDEBUG -fopenmp -fPIC -DPARALLEL -DMATHBACKEND=4 -DOPENFHE_VERSION=1.5.1 -w".split()
    with tempfile.TemporaryDirectory() as tmp:
        exe, dump = os.path.join(tmp, "gen_bgv_decrypt"), os.path.join(tmp, "dump.bin")
        subprocess.check_call(["g++"] + flags + incs + [os.path.join(ROOT, "tests", "golden", "gen_bgv_decrypt.cpp"), "-o", exe, f"-L{lib}",
                                                        "-lOPENFHEpke", "-lOPENFHEbinfhe", "-lOPENFHEcore", f"-Wl,-rpath,{lib}"])
        subprocess.check_call([exe, dump])
        raw = open(dump, "rb").read()
    out, off = {}, 0
    while off < len(raw):
        (n,) = struct.unpack_from("<I", raw, off)
        name = raw[off + 4:off + 4 + n].decode()
        _, count = struct.unpack_from("<IQ", raw, off + 4 + n)
        off += 4 + n + 12
        out[name] = np.frombuffer(raw, dtype=np.uint64, count=count, offset=off).copy()
        off += 8 * count
    return out


def shaped(out):
    ring = int(out["meta"][0])
    for p in ("fm_", "fx_"):
        out[p + "s"] = out[p + "s"].reshape(len(out[p + "q"]), ring)
    for c in CASES:
        n_elem, size_ql = (int(v) for v in out[c + "_meta"])
        out[c + "_c"] = out[c + "_c"].reshape(n_elem, size_ql, ring)
    return out


if __name__ == "__main__":
    out = shaped(run_generator())
    path = os.path.join(ROOT, "tests", "golden", "ref_vectors_bgv_decrypt.npz")
    np.savez_compressed(path, **out)
    print("wrote tests/golden/ref_vectors_bgv_decrypt.npz with", len(out), "arrays,", os.path.getsize(path), "bytes")
