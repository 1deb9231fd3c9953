#!/usr/bin/env python3
"""Generates tests/golden/ref_vectors_hps.npz by RUNNING THE REFERENCE ITSELF (oracle/_ref/libref_shim.so): for the
multiplication techniques HPS (1), HPSPOVERQ (2) and HPSPOVERQLEVELED (3), two fresh BFV ciphertexts and their
LeveledSHEBFVRNS::EvalMult product through the reference's scheme layer (cc->EvalMultNoRelin,
src/pke/lib/scheme/bfvrns/bfvrns-leveledshe.cpp:198-439) at small ring dimensions, with the moduli of Q and of the auxiliary
basis R (bfvrns-cryptoparameters.cpp:75, 126-139) from the reference's own prime search.  A non-BEHZ context has no BEHZ parameter
set, so the Q chain is rebuilt from the ciphertext's limb count (q_0 = LastPrime(scalingModSize, 2N), q_i = PreviousPrime).
A second part comes from a small generator of our own (tests/golden/gen_hps_leveled.cpp, linked against oracle/_ref's stock
libraries): an HPSPOVERQLEVELED product for which the reference DROPS a level (a 30-bit chain at N = 1024, operands of noiseScaleDeg 3),
with the reference's own tables of every level (keys hpslev_*).
Run from the repo root:  python tests/golden/make_golden_hps.py   (needs ./build.sh ref and the reference's sources)
"""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import libs  # noqa: E402

CASES = ((64, 65537, 2, 60), (1024, 786433, 3, 55))


def session(r, tech, ring, t, depth, sms):
    h = r.ref_bfv_create(ring, t, depth, sms, tech)
    r.ref_bfv_keygen(h)
    a, b = r.ref_bfv_encrypt(h, 1), r.ref_bfv_encrypt(h, 2)
    c = r.ref_bfv_eval_mult_no_relin(h, a, b)

    def export(ct):
        ci = np.zeros(3, np.uint32)
        r.ref_bfv_ct_info(h, ct, ci)
        out = np.zeros((int(ci[0]), int(ci[1]), ring), np.uint64)
        for e in range(int(ci[0])):
            r.ref_bfv_ct_export(h, ct, e, out[e])
        return out, int(ci[2])

    (A, fa), (B, fb), (D, fd) = export(a), export(b), export(c)
    assert (fa, fb, fd) == (0, 0, 1) and D.shape[0] == 3  # inputs EVALUATION, product COEFFICIENT with 3 elements
    numQ, M = A.shape[1], 2 * ring
    q = [r.ref_last_prime(sms, M)]
    while len(q) < numQ:
        q.append(r.ref_previous_prime(q[-1], M))
    rr = [r.ref_previous_prime(q[-1], M)]
    while len(rr) < (numQ + 1 if tech == 1 else numQ):
        rr.append(r.ref_previous_prime(rr[-1], M))
    roots = lambda v: np.array([r.ref_root_of_unity(M, int(m)) for m in v], np.uint64)
    r.ref_bfv_destroy(h)
    return dict(t=np.array([t], np.uint64), q=np.array(q, np.uint64), psiQ=roots(q), r=np.array(rr, np.uint64), psiR=roots(rr),
                a=A, b=B, d=D)


def leveled_session(ref_src="/root/reference"):
    """compile and run gen_hps_leveled.cpp; returns {name: array}"""
    stub = os.path.join(ROOT, "third_party_stubs")
    lib = os.path.join(ROOT, "oracle", "_ref")
    incs = [f"-I{stub}/stub", f"-I{stub}/gen"] + [f"-I{ref_src}/src/{m}/{d}" for m in ("core", "binfhe", "pke") for d in ("include", "lib")]
    flags = "-std=c++17 -O2 -DNDEBUG -fopenmp -fPIC -DPARALLEL -DMATHBACKEND=4 -DOPENFHE_VERSION=1.5.1 -w".split()
    with tempfile.TemporaryDirectory() as tmp:
        exe, dump = os.path.join(tmp, "gen_hps_leveled"), os.path.join(tmp, "dump.bin")
        subprocess.check_call(["g++"] + flags + incs + [os.path.join(ROOT, "tests", "golden", "gen_hps_leveled.cpp"), "-o", exe, f"-L{lib}",
                                                        "-lOPENFHEpke", "-lOPENFHEbinfhe", "-lOPENFHEcore", f"-Wl,-rpath,{lib}"])
        subprocess.check_call([exe, dump])
        raw = open(dump, "rb").read()
    out, off = {}, 0
    while off < len(raw):
        (n,) = struct.unpack_from("<I", raw, off)
        name = raw[off + 4:off + 4 + n].decode()
        typ, count = struct.unpack_from("<IQ", raw, off + 4 + n)
        off += 4 + n + 12
        out[name] = np.frombuffer(raw, dtype=np.float64 if typ else np.uint64, count=count, offset=off).copy()
        off += 8 * count
    ring, t, numQ, sizeQl = (int(v) for v in out["meta"][:4])
    assert sizeQl < numQ, "the generator must observe a dropped level"
    for k, elems in (("a", 2), ("b", 2), ("d", 3)):
        out[k] = out[k].reshape(elems, numQ, ring)
    assert not out["d"][:, sizeQl:].any()  # ExpandCRTBasisQlHat: zero rows above Q_l
    return out


if __name__ == "__main__":
    r = libs.load_ref()
    out = {}
    for tech in (1, 2, 3):
        for ring, t, depth, sms in CASES:
            for k, v in session(r, tech, ring, t, depth, sms).items():
                out[f"hps{tech}_{ring}_{k}"] = v
    for k, v in leveled_session().items():
        out["hpslev_" + k] = v
    path = os.path.join(ROOT, "tests", "golden", "ref_vectors_hps.npz")
    np.savez_compressed(path, **out)
    print("wrote tests/golden/ref_vectors_hps.npz with", len(out), "arrays,", os.path.getsize(path), "bytes")
