#!/usr/bin/env python3
"""Generates tests/golden/ref_vectors_bv.npz by RUNNING THE REFERENCE ITSELF: a small generator of our own
(tests/golden/gen_bv_keyswitch.cpp, linked against oracle/_ref's stock libraries) records BV key switching (KeySwitchBV,
src/pke/lib/keyswitch/keyswitch-bv.cpp) through the reference's scheme layer at ring dimension 64 for the digit sizes 0 and 10:
  bfv<r>_*   BFV depth 4 (3 limbs of 60 bits), HPSPOVERQLEVELED + BV — the reference's default BFV configuration: moduli and roots of Q
             and R, both operands, the key's b and a vectors, cc->EvalMultNoRelin, KeySwitchCore of its third element, cc->EvalMult
  ckks<r>_*  CKKS depth 2, FIXEDMANUAL (limbs of 60, 50, 51 bits): the key, the third element of an EvalMultNoRelin at 2 of 3 limbs and
             its KeySwitchCore
meta = (ring, t, sizeQ, sizeQl, digit size, D_0).  Data only.
Run from the repo root:  python tests/golden/make_golden_bv.py   (needs ./build.sh ref and the reference's sources)
"""
import os
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run_generator(ref_src="/root/reference"):
    """compile and run gen_bv_keyswitch.cpp; returns {name: flat uint64 array}"""
    stub = os.path.join(ROOT, "third_party_stubs")
    lib = os.path.join(ROOT, "oracle", "_ref")
    incs = [f"-I{stub}/stub", f"-I{stub}/gen"] + [f"-I{ref_src}/src/{m}/{d}" for m in ("core", "binfhe", "pke") for d in ("include", "lib")]
    flags = "-std=c++17 -O2 -DNDEBUG -fopenmp -fPIC -DPARALLEL -DMATHBACKEND=4 -DOPENFHE_VERSION=1.5.1 -w".split()
    with tempfile.TemporaryDirectory() as tmp:
        exe, dump = os.path.join(tmp, "gen_bv_keyswitch"), os.path.join(tmp, "dump.bin")
        subprocess.check_call(["g++"] + flags + incs + [os.path.join(ROOT, "tests", "golden", "gen_bv_keyswitch.cpp"), "-o", exe, f"-L{lib}",
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
    for pre in ("bfv0_", "bfv10_", "ckks0_", "ckks10_"):
        ring, _, sizeQ, sizeQl, _, D0 = (int(v) for v in out[pre + "meta"])
        out[pre + "keyB"] = out[pre + "keyB"].reshape(D0, sizeQ, ring)
        out[pre + "keyA"] = out[pre + "keyA"].reshape(D0, sizeQ, ring)
        if pre.startswith("bfv"):
            for k, elems in (("a", 2), ("b", 2), ("d", 3), ("ks", 2), ("m", 2)):
                out[pre + k] = out[pre + k].reshape(elems, sizeQ, ring)
        else:
            out[pre + "c"] = out[pre + "c"].reshape(sizeQl, ring)
            out[pre + "ks"] = out[pre + "ks"].reshape(2, sizeQl, ring)
    return out


if __name__ == "__main__":
    out = shaped(run_generator())
    path = os.path.join(ROOT, "tests", "golden", "ref_vectors_bv.npz")
    np.savez_compressed(path, **out)
    print("wrote tests/golden/ref_vectors_bv.npz with", len(out), "arrays,", os.path.getsize(path), "bytes")
