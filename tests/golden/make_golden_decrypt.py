#!/usr/bin/env python3
"""Generates tests/golden/ref_vectors_decrypt.npz by RUNNING THE REFERENCE ITSELF: a small generator of our own
(tests/golden/gen_decrypt.cpp, linked against oracle/_ref's stock libraries) records, at ring dimension 64, ciphertexts, secret keys and what
the reference's scheme layer decrypts them to before decoding: for BFV (HPSPOVERQLEVELED on 60-bit moduli, HPS on 45-bit moduli, BEHZ;
t = 65537) the NativePoly of PKEBFVRNS::Decrypt (bfvrns-pke.cpp:215-245) and the decryption tables of CryptoParametersBFVRNS; for CKKS
(FIXEDMANUAL, 3 limbs) the Poly of PKECKKSRNS::Decrypt (ckksrns-pke.cpp:44-96) reduced modulo every limb; for two-party threshold BFV and
CKKS the joint ciphertext, both secret shares, the partial decryptions of MultipartyDecryptLead / Main (rns-multiparty.cpp:46-171) and
the result of MultipartyDecryptFusion.  Arrays and meta: see the head of the generator, which fails unless every shape is what its meta
block says and every case decodes to the encoded values.  Data only.
Run from the repo root:  python tests/golden/make_golden_decrypt.py   (needs ./build.sh ref and the reference's sources)
"""
import os
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
META = ("ring", "numQ", "t", "technique", "ns")
BFV_SETS = ("hps_", "hpsu_", "behz_")
BFV_CASES = ("hps_fresh", "hps_prod", "hpsu_fresh", "hpsu_prod", "behz_fresh")
CKKS_CASES = ("ckks_fresh", "ckks_rescaled", "ckks_prod", "ckks_one")
THRESHOLD_SETS = ("tbfv_", "tckks_")
LIMIT = 1 << 20  # bytes: the largest file the repository takes


def run_generator(ref_src="/root/reference"):
    """compile and run gen_decrypt.cpp; returns {name: flat uint64 array}"""
    stub = os.path.join(ROOT, "third_party_stubs")
    lib = os.path.join(ROOT, "oracle", "_ref")
    incs = [f"-I{stub}/stub", f"-I{stub}/gen"] + [f"-I{ref_src}/src/{m}/{d}" for m in ("core", "binfhe", "pke") for d in ("include", "lib")]
    flags = "-std=c++17 -O2 -DNDEBUG -fopenmp -fPIC -DPARALLEL -DMATHBACKEND=4 -DOPENFHE_VERSION=1.5.1 -w".split()
    with tempfile.TemporaryDirectory() as tmp:
        exe, dump = os.path.join(tmp, "gen_decrypt"), os.path.join(tmp, "dump.bin")
        subprocess.check_call(["g++"] + flags + incs + [os.path.join(ROOT, "tests", "golden", "gen_decrypt.cpp"), "-o", exe, f"-L{lib}",
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
    def meta(pre):
        g = dict(zip(META, (int(v) for v in out[pre + "meta"])))
        assert len(out[pre + "q"]) == g["numQ"] == len(out[pre + "psi"]), pre
        return g["ring"], g["numQ"]

    for pre in BFV_SETS + ("ckks_",):
        ring, numQ = meta(pre)
        out[pre + "s"] = out[pre + "s"].reshape(numQ, ring)
    for c in BFV_CASES + CKKS_CASES:
        n_elem, size_ql, _ = (int(v) for v in out[c + "_meta"])
        out[c + "_c"] = out[c + "_c"].reshape(n_elem, size_ql, ring)
        if c in CKKS_CASES:
            out[c + "_b"] = out[c + "_b"].reshape(size_ql, ring)
        else:
            assert out[c + "_m"].shape == (ring,), c
    for pre in THRESHOLD_SETS:
        ring, numQ = meta(pre)
        for k in ("s1", "s2", "lead", "main"):
            out[pre + k] = out[pre + k].reshape(numQ, ring)
        out[pre + "c"] = out[pre + "c"].reshape(2, numQ, ring)
    out["tckks_fusion"] = out["tckks_fusion"].reshape(-1, ring)
    assert out["tbfv_fusion"].shape == (ring,)
    return out


if __name__ == "__main__":
    out = shaped(run_generator())
    path = os.path.join(ROOT, "tests", "golden", "ref_vectors_decrypt.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < LIMIT, f"{size} bytes: too large to commit"
    print("wrote tests/golden/ref_vectors_decrypt.npz with", len(out), "arrays,", size, "bytes")
