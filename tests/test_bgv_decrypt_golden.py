"""BGV decryption against words recorded from the reference itself (tests/golden/ref_vectors_bgv_decrypt.npz, written by
tests/golden/make_golden_bgv_decrypt.py): ring 64, t = 65537, depth 3.  Under FIXEDMANUAL a fresh ciphertext, the three-element product of
EvalMultNoRelin and a ciphertext after cc->ModReduce; under the default FLEXIBLEAUTOEXT a fresh ciphertext.  For each the generator kept the
secret key, the elements and the NativePoly that PKEBGVRNS::Decrypt (bgvrns-pke.cpp:44-99) returns before decoding; the elements go through
fhe_bgv_decrypt here and every word is compared.  Ring 64 pins the composition (DecryptCore, the format switch, the chain, the residues modulo
t), the oracle tests of test_parity_bgv_decrypt.py pin the kernel's shapes.  `backend` = the lane emulator on the CPU, the product library
with -m gpu."""
import os

import numpy as np
import pytest

from openfhe_amd import fhe_hip as fh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_vectors_bgv_decrypt.npz")
CASES = (("fm_fresh", 2), ("fm_prod", 3), ("fm_reduced", 2), ("fx_fresh", 2))


def record():
    z = np.load(GOLDEN)  # (a missing fixture is an error, not a skip)
    return {k: z[k] for k in z.files}


def test_the_record_is_what_the_generator_checked():
    g = record()
    ring, t = (int(v) for v in g["meta"])
    assert (ring, t) == (64, 65537) and os.path.getsize(GOLDEN) < 100 * 1024
    for name, n_elem in CASES:
        c, m, p = g[name + "_c"], g[name + "_m"], name[:3]
        assert c.shape[0] == n_elem == int(g[name + "_meta"][0]) and c.shape[1] == int(g[name + "_meta"][1]) >= 2 and c.shape[2] == ring
        assert c.shape[1] <= len(g[p + "q"]) and g[p + "s"].shape == (len(g[p + "q"]), ring)
        assert m.shape == (ring,) and int(m.max()) < t
    assert g["fm_reduced_c"].shape[1] == g["fm_fresh_c"].shape[1] - 1


@pytest.mark.parametrize("name,n_elem", CASES)
def test_bgv_decrypt_matches_the_reference(backend, name, n_elem):
    g = record()
    ring, t = (int(v) for v in g["meta"])
    p = name[:3]
    ctx = fh.Context(backend, ring.bit_length() - 1, g[p + "q"], g[p + "psi"])
    c = g[name + "_c"]
    size_ql = c.shape[1]
    elems = [ctx.tower(c[e][None]) for e in range(n_elem)]
    s = ctx.tower(g[p + "s"][:size_ql][None])
    got = fh.bgv_decrypt(ctx, elems, s, t)
    assert got.shape == (1, ring) and np.array_equal(got[0], g[name + "_m"]), name
    # the same from its parts: DecryptCore with the tower operations, the format switch, fhe_mod_reduce_to_t
    b = elems[0].Plus(elems[1].Times(s))
    if n_elem == 3:
        b = b.Plus(elems[2].Times(s.Times(s)))
    b.SetFormat(fh.COEFFICIENT)
    assert np.array_equal(fh.mod_reduce_to_t(ctx, b, t)[0], g[name + "_m"]), name + " (from its parts)"
    # ... and one ciphertext among three of a batch
    batch = [ctx.tower(np.stack([c[e], np.zeros_like(c[e]), c[e]])) for e in range(n_elem)]
    got3 = fh.bgv_decrypt(ctx, batch, s, t)
    assert np.array_equal(got3[0], g[name + "_m"]) and np.array_equal(got3[2], g[name + "_m"]) and not got3[1].any()
    ctx.close()
