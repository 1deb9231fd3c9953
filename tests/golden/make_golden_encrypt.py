#!/usr/bin/env python3
"""Generates tests/golden/ref_vectors_encrypt.npz by RUNNING THE REFERENCE ITSELF: a small generator of our own
(tests/golden/gen_encrypt.cpp, linked against oracle/_ref's stock libraries) records fresh ciphertexts of the reference's Encrypt under
the secret key and under the public key (PKERNS::Encrypt / EncryptZeroCore, rns-pke.cpp:40-70, 111-197; PKEBFVRNS::Encrypt,
bfvrns-pke.cpp:99-213) at ring dimension 64 for four parameter sets: CKKS with 3 limbs (one plaintext at full level, one encoded one level
down), CKKS with a Gaussian secret, BGV FIXEDMANUAL with t = 65537, BFV HPS with STANDARD encryption.  Arrays and meta: see the head of
the generator, which fails unless the shapes are what its meta block says.  Data only.
Run from the repo root:  python tests/golden/make_golden_encrypt.py   (needs ./build.sh ref and the reference's sources)
"""
import os
import subprocess
import tempfile

import numpy as np

from make_golden_bgv import ROOT

META = ("ring", "ns", "numQ", "t", "sigma100", "gaussian", "downLimbs")
SETS = ("ckks_", "ckksg_", "bgv_", "bfv_")
LIMIT = 1 << 20  # bytes: the largest file the repository takes


def run_generator(ref_src="/root/reference"):
    """compile and run gen_encrypt.cpp; returns {name: flat uint64 array}"""
    import struct
    stub = os.path.join(ROOT, "third_party_stubs")
    lib = os.path.join(ROOT, "oracle", "_ref")
    incs = [f"-I{stub}/stub", f"-I{stub}/gen"] + [f"-I{ref_src}/src/{m}/{d}" for m in ("core", "binfhe", "pke") for d in ("include", "lib")]
    flags = "-std=c++17 -O2 -DNDEBUG -fopenmp -fPIC -DPARALLEL -DMATHBACKEND=4 -DOPENFHE_VERSION=1.5.1 -w".split()
    with tempfile.TemporaryDirectory() as tmp:
        exe, dump = os.path.join(tmp, "gen_encrypt"), os.path.join(tmp, "dump.bin")
        subprocess.check_call(["g++"] + flags + incs + [os.path.join(ROOT, "tests", "golden", "gen_encrypt.cpp"), "-o", exe, f"-L{lib}",
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
        ring, numQ, down = g["ring"], g["numQ"], g["downLimbs"]
        assert len(out[pre + "q"]) == numQ == len(out[pre + "psi"])
        for k in ("s", "pkB", "pkA", "pt", "sk0", "sk1", "pk0", "pk1"):
            out[pre + k] = out[pre + k].reshape(numQ, ring)
        if down:
            for k in ("ptd", "skd0", "skd1", "pkd0", "pkd1"):
                out[pre + k] = out[pre + k].reshape(down, ring)
    return out


if __name__ == "__main__":
    out = shaped(run_generator())
    path = os.path.join(ROOT, "tests", "golden", "ref_vectors_encrypt.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < LIMIT, f"{size} bytes: too large to commit"
    print("wrote tests/golden/ref_vectors_encrypt.npz with", len(out), "arrays,", size, "bytes")
