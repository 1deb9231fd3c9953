#!/usr/bin/env python3
"""Generates tests/golden/ref_vectors_bgv_auto.npz by RUNNING THE REFERENCE ITSELF: a small generator of our own
(tests/golden/gen_bgv_auto.cpp, linked against oracle/_ref's stock libraries) records, for BGV on HYBRID keys at ring dimension 64 and
t = 65537 under FLEXIBLEAUTO and under FLEXIBLEAUTOEXT, ciphertext pairs before and after LeveledSHEBGVRNS::AdjustLevelsAndDepthInPlace and
AdjustLevelsAndDepthToOneInPlace (bgvrns-leveledshe.cpp:83-233) on every branch of the case table, with their levels, noise degrees,
scaling-factor integers and the parameter tables the plan helper reads, and cc->EvalAdd / cc->EvalMult of operands at different levels.
Arrays and meta: see the head of the generator, which fails unless every branch was reached.  Data only.
Run from the repo root:  python tests/golden/make_golden_bgv_auto.py   (needs ./build.sh ref and the reference's sources)
"""
import os
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PREFIXES = ("fa_", "fx_")


def run_generator(ref_src="/root/reference"):
    """compile and run gen_bgv_auto.cpp; returns {name: flat uint64 array}"""
    stub = os.path.join(ROOT, "third_party_stubs")
    lib = os.path.join(ROOT, "oracle", "_ref")
    incs = [f"-I{stub}/stub", f"-I{stub}/gen"] + [f"-I{ref_src}/src/{m}/{d}" for m in ("core", "binfhe", "pke") for d in ("include", "lib")]
    flags = "-std=c++17 -O2 -DNDEBUG -fopenmp -fPIC -DPARALLEL -DMATHBACKEND=4 -DOPENFHE_VERSION=1.5.1 -w".split()
    with tempfile.TemporaryDirectory() as tmp:
        exe, dump = os.path.join(tmp, "gen_bgv_auto"), os.path.join(tmp, "dump.bin")
        subprocess.check_call(["g++"] + flags + incs + [os.path.join(ROOT, "tests", "golden", "gen_bgv_auto.cpp"), "-o", exe, f"-L{lib}",
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
    ring, dnum = int(out["meta"][0]), int(out["meta"][2])
    for p in PREFIXES:
        tot = len(out[p + "q"]) + len(out[p + "p"])
        out[p + "mulB"] = out[p + "mulB"].reshape(dnum, tot, ring)
        out[p + "mulA"] = out[p + "mulA"].reshape(dnum, tot, ring)
        out[p + "cases"] = out[p + "cases"].reshape(-1, 3)
    for name in list(out):
        if name.endswith("_meta") or name.split("_")[-1] in ("q", "psiQ", "p", "psiP", "mulB", "mulA", "mrf", "big", "cases") or name == "meta":
            continue
        out[name] = out[name].reshape(2, -1, ring)  # a ciphertext: its two elements
    return out


if __name__ == "__main__":
    out = shaped(run_generator())
    path = os.path.join(ROOT, "tests", "golden", "ref_vectors_bgv_auto.npz")
    np.savez_compressed(path, **out)
    print("wrote tests/golden/ref_vectors_bgv_auto.npz with", len(out), "arrays,", os.path.getsize(path), "bytes")
