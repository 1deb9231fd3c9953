#!/usr/bin/env python3
"""Generates tests/golden/ref_vectors_bfv_hybrid.npz by RUNNING THE REFERENCE ITSELF: a small generator of our own
(tests/golden/gen_bfv_hybrid.cpp, linked against oracle/_ref's stock libraries) records rotations and leveled relinearisation of BFV
ciphertexts on HYBRID keys (LeveledSHEBFVRNS::EvalAutomorphism, EvalFastRotationPrecompute, EvalFastRotation, RelinearizeCore, EvalMult,
src/pke/lib/scheme/bfvrns/bfvrns-leveledshe.cpp, with KeySwitchHYBRID) at ring dimension 64, t = 65537, HPSPOVERQLEVELED + HYBRID,
numLargeDigits 2 and 3.  Arrays and meta: see the head of the generator.  The generator fails unless the dropped-level cases drop a level.
Data only.
Run from the repo root:  python tests/golden/make_golden_bfv_hybrid.py   (needs ./build.sh ref and the reference's sources)
"""
import os
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
META = ("ring", "t", "numQ", "sizeP", "dnum", "k0", "k1", "sizeQlRot", "degRotL", "sizeQlRotL", "degMul", "sizeQlMul", "sizeQlRelin")
CASES = ("bfvh2_", "bfvh3_")


def run_generator(ref_src="/root/reference"):
    """compile and run gen_bfv_hybrid.cpp; returns {name: flat uint64 array}"""
    stub = os.path.join(ROOT, "third_party_stubs")
    lib = os.path.join(ROOT, "oracle", "_ref")
    incs = [f"-I{stub}/stub", f"-I{stub}/gen"] + [f"-I{ref_src}/src/{m}/{d}" for m in ("core", "binfhe", "pke") for d in ("include", "lib")]
    flags = "-std=c++17 -O2 -DNDEBUG -fopenmp -fPIC -DPARALLEL -DMATHBACKEND=4 -DOPENFHE_VERSION=1.5.1 -w".split()
    with tempfile.TemporaryDirectory() as tmp:
        exe, dump = os.path.join(tmp, "gen_bfv_hybrid"), os.path.join(tmp, "dump.bin")
        subprocess.check_call(["g++"] + flags + incs + [os.path.join(ROOT, "tests", "golden", "gen_bfv_hybrid.cpp"), "-o", exe, f"-L{lib}",
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
    for pre in CASES:
        g = dict(zip(META, (int(v) for v in out[pre + "meta"])))
        ring, numQ, sizeP, dnum = g["ring"], g["numQ"], g["sizeP"], g["dnum"]
        for k in ("rotB0", "rotA0", "rotB1", "rotA1", "mulB", "mulA"):
            out[pre + k] = out[pre + k].reshape(dnum, numQ + sizeP, ring)
        for k, elems in (("a", 2), ("b", 2), ("rot0", 2), ("rot1", 2), ("rotL0", 2), ("rotL1", 2), ("d", 3), ("m", 2)):
            out[pre + k] = out[pre + k].reshape(elems, numQ, ring)
        for k, sizeQl in (("dig", g["sizeQlRot"]), ("digL", g["sizeQlRotL"])):
            out[pre + k] = out[pre + k].reshape(-1, sizeQl + sizeP, ring)
    return out


if __name__ == "__main__":
    out = shaped(run_generator())
    path = os.path.join(ROOT, "tests", "golden", "ref_vectors_bfv_hybrid.npz")
    np.savez_compressed(path, **out)
    print("wrote tests/golden/ref_vectors_bfv_hybrid.npz with", len(out), "arrays,", os.path.getsize(path), "bytes")
