#!/usr/bin/env python3
"""Generates tests/golden/ref_vectors_keygen_bv.npz by RUNNING THE REFERENCE ITSELF: a small generator of our own
(tests/golden/gen_keygen_bv.cpp, linked against oracle/_ref's stock libraries) records the keys of the reference's KeyGen, EvalMultKeyGen,
EvalRotateKeyGen (KeySwitchBV::KeySwitchGenInternal, keyswitch-bv.cpp:49-103, through LeveledSHEBase::EvalAutomorphismKeyGen,
base-leveledshe.cpp:336-379) and ReKeyGen (keyswitch-bv.cpp:162-225 through PREBase::ReKeyGen, base-pre.cpp:42-45) at ring dimension 64
for three parameter sets: BFV with t = 65537 and three 60-bit limbs at digit sizes 0 and 10, and CKKS FIXEDMANUAL with limbs of 60 / 50 /
51 bits at digit size 10.  Arrays and meta: see the head of the generator, which fails unless the shapes are what its meta block says.
Data only.
Run from the repo root:  python tests/golden/make_golden_keygen_bv.py   (needs ./build.sh ref and the reference's sources)
"""
import os
import struct
import subprocess
import tempfile

import numpy as np

from make_golden_bgv import ROOT

META = ("ring", "ns", "numQ", "r", "D0", "kPlus", "kMinus", "sigma100", "t")
SETS = ("bfv0_", "bfv10_", "ckks10_")


def run_generator(ref_src="/root/reference"):
    """compile and run gen_keygen_bv.cpp; returns {name: flat uint64 array}"""
    stub = os.path.join(ROOT, "third_party_stubs")
    lib = os.path.join(ROOT, "oracle", "_ref")
    incs = [f"-I{stub}/stub", f"-I{stub}/gen"] + [f"-I{ref_src}/src/{m}/{d}" for m in ("core", "binfhe", "pke") for d in ("include", "lib")]
    flags = "-std=c++17 -O2 -DNDEBUG -fopenmp -fPIC -DPARALLEL -DMATHBACKEND=4 -DOPENFHE_VERSION=1.5.1 -w".split()
    with tempfile.TemporaryDirectory() as tmp:
        exe, dump = os.path.join(tmp, "gen_keygen_bv"), os.path.join(tmp, "dump.bin")
        subprocess.check_call(["g++"] + flags + incs + [os.path.join(ROOT, "tests", "golden", "gen_keygen_bv.cpp"), "-o", exe, f"-L{lib}",
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
    for pre in SETS:
        g = dict(zip(META, (int(v) for v in out[pre + "meta"])))
        ring, numQ, D0 = g["ring"], g["numQ"], g["D0"]
        for k in ("s", "pkB", "pkA", "s2", "pk2B", "pk2A"):
            out[pre + k] = out[pre + k].reshape(numQ, ring)
        for k in ("mulB", "mulA", "rotPB", "rotPA", "rotMB", "rotMA", "reB", "reA"):
            out[pre + k] = out[pre + k].reshape(D0, numQ, ring)
        if g["t"]:
            out[pre + "ct"] = out[pre + "ct"].reshape(2, numQ, ring)
    return out


if __name__ == "__main__":
    out = shaped(run_generator())
    path = os.path.join(ROOT, "tests", "golden", "ref_vectors_keygen_bv.npz")
    np.savez_compressed(path, **out)
    print("wrote tests/golden/ref_vectors_keygen_bv.npz with", len(out), "arrays,", os.path.getsize(path), "bytes")
