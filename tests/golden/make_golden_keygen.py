#!/usr/bin/env python3
"""Generates tests/golden/ref_vectors_keygen.npz by RUNNING THE REFERENCE ITSELF: a small generator of our own
(tests/golden/gen_keygen_hybrid.cpp, linked against oracle/_ref's stock libraries) records the keys of the reference's KeyGen
(PKEBase::KeyGenInternal, base-pke.cpp:47-98), EvalMultKeyGen and EvalRotateKeyGen (KeySwitchHYBRID::KeySwitchGenInternal,
keyswitch-hybrid.cpp:51-130, through LeveledSHEBase::EvalAutomorphismKeyGen, base-leveledshe.cpp:336-379) at ring dimension 64 for two
parameter sets: CKKS on HYBRID keys with 2 digits and a short last digit, and BGV FIXEDMANUAL with t = 65537 on HYBRID keys.  Arrays and
meta: see the head of the generator, which fails unless the shapes are what its meta block says.  Data only.
Run from the repo root:  python tests/golden/make_golden_keygen.py   (needs ./build.sh ref and the reference's sources)
"""
import os
import subprocess
import tempfile

import numpy as np

from make_golden_bgv import ROOT

META = ("ring", "ns", "numQ", "numP", "dnum", "alpha", "kPlus", "kMinus", "sigma100")
SETS = ("ckks_", "bgv_")


def run_generator(ref_src="/root/reference"):
    """compile and run gen_keygen_hybrid.cpp; returns {name: flat uint64 array}"""
    import struct
    stub = os.path.join(ROOT, "third_party_stubs")
    lib = os.path.join(ROOT, "oracle", "_ref")
    incs = [f"-I{stub}/stub", f"-I{stub}/gen"] + [f"-I{ref_src}/src/{m}/{d}" for m in ("core", "binfhe", "pke") for d in ("include", "lib")]
    flags = "-std=c++17 -O2 -DNDEBUG -fopenmp -fPIC -DPARALLEL -DMATHBACKEND=4 -DOPENFHE_VERSION=1.5.1 -w".split()
    with tempfile.TemporaryDirectory() as tmp:
        exe, dump = os.path.join(tmp, "gen_keygen_hybrid"), os.path.join(tmp, "dump.bin")
        subprocess.check_call(["g++"] + flags + incs + [os.path.join(ROOT, "tests", "golden", "gen_keygen_hybrid.cpp"), "-o", exe, f"-L{lib}",
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
        ring, numQ, numP, dnum = g["ring"], g["numQ"], g["numP"], g["dnum"]
        for k in ("s", "pkB", "pkA"):
            out[pre + k] = out[pre + k].reshape(numQ, ring)
        for k in ("mulB", "mulA", "rotPB", "rotPA", "rotMB", "rotMA"):
            out[pre + k] = out[pre + k].reshape(dnum, numQ + numP, ring)
    return out


if __name__ == "__main__":
    out = shaped(run_generator())
    path = os.path.join(ROOT, "tests", "golden", "ref_vectors_keygen.npz")
    np.savez_compressed(path, **out)
    print("wrote tests/golden/ref_vectors_keygen.npz with", len(out), "arrays,", os.path.getsize(path), "bytes")
