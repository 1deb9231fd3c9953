#!/usr/bin/env python3
"""Generates tests/golden/ref_vectors_bgv.npz by RUNNING THE REFERENCE ITSELF: a small generator of our own
(tests/golden/gen_bgv_hybrid.cpp, linked against oracle/_ref's stock libraries) records BGV on HYBRID keys through the reference's scheme
layer (KeySwitchHYBRID with ApproxModDown's t > 0, keyswitch-hybrid.cpp:308-400; LeveledSHEBase::EvalMult / EvalAutomorphism /
EvalFastRotation, base-leveledshe.cpp; LeveledSHEBGVRNS::ModReduceInternalInPlace, bgvrns-leveledshe.cpp:44-75) at ring dimension 64,
t = 65537, depth 3, FIXEDMANUAL, 2 digits.  Arrays and meta: see the head of the generator.  The generator fails unless the product sits
at the full level and ModReduce drops exactly one limb.  Data only.
Run from the repo root:  python tests/golden/make_golden_bgv.py   (needs ./build.sh ref and the reference's sources)
"""
import os
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
META = ("ring", "t", "numQ", "numP", "dnum", "k", "sizeQlMul", "sizeQlReduced")


def run_generator(ref_src="/root/reference"):
    """compile and run gen_bgv_hybrid.cpp; returns {name: flat uint64 array}"""
    stub = os.path.join(ROOT, "third_party_stubs")
    lib = os.path.join(ROOT, "oracle", "_ref")
    incs = [f"-I{stub}/stub", f"-I{stub}/gen"] + [f"-I{ref_src}/src/{m}/{d}" for m in ("core", "binfhe", "pke") for d in ("include", "lib")]
    flags = "-std=c++17 -O2 -DNDEBUG -fopenmp -fPIC -DPARALLEL -DMATHBACKEND=4 -DOPENFHE_VERSION=1.5.1 -w".split()
    with tempfile.TemporaryDirectory() as tmp:
        exe, dump = os.path.join(tmp, "gen_bgv_hybrid"), os.path.join(tmp, "dump.bin")
        subprocess.check_call(["g++"] + flags + incs + [os.path.join(ROOT, "tests", "golden", "gen_bgv_hybrid.cpp"), "-o", exe, f"-L{lib}",
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
    g = dict(zip(META, (int(v) for v in out["meta"])))
    ring, numQ, numP, dnum = g["ring"], g["numQ"], g["numP"], g["dnum"]
    for k in ("mulB", "mulA", "rotB", "rotA"):
        out[k] = out[k].reshape(dnum, numQ + numP, ring)
    for k, limbs in (("a", numQ), ("b", numQ), ("m", g["sizeQlMul"]), ("r", g["sizeQlReduced"]), ("rot", numQ), ("rotL", g["sizeQlReduced"]),
                     ("mL", g["sizeQlReduced"])):
        out[k] = out[k].reshape(2, limbs, ring)
    return out


if __name__ == "__main__":
    out = shaped(run_generator())
    path = os.path.join(ROOT, "tests", "golden", "ref_vectors_bgv.npz")
    np.savez_compressed(path, **out)
    print("wrote tests/golden/ref_vectors_bgv.npz with", len(out), "arrays,", os.path.getsize(path), "bytes")
