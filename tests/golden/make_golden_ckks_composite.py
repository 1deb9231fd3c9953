#!/usr/bin/env python3
"""Generates tests/golden/ref_vectors_ckks_composite.npz by RUNNING THE REFERENCE ITSELF: a small generator of our own
(tests/golden/gen_ckks_composite.cpp, linked against oracle/_ref's stock libraries) records the rescale of a CKKS product under
COMPOSITESCALINGMANUAL (LeveledSHECKKSRNS::ModReduceInternalInPlace(ct, compositeDegree), ckksrns-leveledshe.cpp:172-191) at ring dimension
64 for composite degree 2 and 3.  Arrays and meta: see the head of the generator.  The generator fails unless the call dropped exactly
compositeDegree limbs.  Data only.
Run from the repo root:  python tests/golden/make_golden_ckks_composite.py   (needs ./build.sh ref and the reference's sources)
"""
import os
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
META = ("ring", "degree", "sizeQ", "sizeQl", "sizeQlAfter")
DEGREES = (2, 3)


def run_generator(ref_src="/root/reference"):
    """compile and run gen_ckks_composite.cpp; returns {name: flat uint64 array}"""
    stub = os.path.join(ROOT, "third_party_stubs")
    lib = os.path.join(ROOT, "oracle", "_ref")
    incs = [f"-I{stub}/stub", f"-I{stub}/gen"] + [f"-I{ref_src}/src/{m}/{d}" for m in ("core", "binfhe", "pke") for d in ("include", "lib")]
    flags = "-std=c++17 -O2 -DNDEBUG -fopenmp -fPIC -DPARALLEL -DMATHBACKEND=4 -DOPENFHE_VERSION=1.5.1 -w".split()
    with tempfile.TemporaryDirectory() as tmp:
        exe, dump = os.path.join(tmp, "gen_ckks_composite"), os.path.join(tmp, "dump.bin")
        subprocess.check_call(["g++"] + flags + incs + [os.path.join(ROOT, "tests", "golden", "gen_ckks_composite.cpp"), "-o", exe, f"-L{lib}",
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
    for d in DEGREES:
        g = dict(zip(META, (int(v) for v in out[f"meta_d{d}"])))
        assert g["degree"] == d and g["sizeQlAfter"] == g["sizeQl"] - d
        out[f"x_d{d}"] = out[f"x_d{d}"].reshape(2, g["sizeQl"], g["ring"])
        out[f"y_d{d}"] = out[f"y_d{d}"].reshape(2, g["sizeQlAfter"], g["ring"])
    return out


if __name__ == "__main__":
    out = shaped(run_generator())
    path = os.path.join(ROOT, "tests", "golden", "ref_vectors_ckks_composite.npz")
    np.savez_compressed(path, **out)
    print("wrote tests/golden/ref_vectors_ckks_composite.npz with", len(out), "arrays,", os.path.getsize(path), "bytes")
