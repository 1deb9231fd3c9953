"""Encryption against fresh ciphertexts recorded from the reference itself (tests/golden/ref_vectors_encrypt.npz, written by
tests/golden/make_golden_encrypt.py): Encrypt(secretKey) and Encrypt(publicKey) of one plaintext at ring 64 for CKKS with 3 limbs (plus a
plaintext encoded one level down), CKKS with a Gaussian secret, BGV FIXEDMANUAL with t = 65537 and BFV HPS with STANDARD encryption.

What is pinned on the reference, and what on the composition only:

(a) The secret-key form is pinned on the reference completely.  The reference exposes neither a nor e, but c1 = -a gives a, and
        e = (c0 - m - a * s) * ns^-1  mod q_i
    must then come out as ONE polynomial of small signed integers: the centred inverse transforms of all limbs agree and no coefficient
    exceeds the length B of the Gaussian sampler's inversion table, ceil(12.006 sigma) = 39 (no larger integer can be drawn; the bound
    the key-generation record uses).  With a wrong sign, a wrong message scaling or the wrong key rows the recovered words are uniform
    residues.  Fed with that a and e, fhe_encrypt_sk_combine must reproduce the recorded c0 and c1 word for word.  BFV's message is
    fhe_times_q_over_t of the COEFFICIENT plaintext, joined to e before the forward transform as the seeded calls do.
(b) The public-key form cannot be pinned word for word: v, e0 and e1 are three unknowns in two equations.  Its pin is the decryption
    residue: c0 + c1 * s - m, centred over Q_l, is ns * r with r = e_pk * v + e0 + e1 * s, so |r| <= N * B + B + N * B = 2 N B + B for
    ternary v and s (|e_pk|, |e0|, |e1| <= B), and 2 N B^2 + B when v and s are Gaussian (|v|, |s| <= B).  The bound is derived, not
    measured.  The recorded ciphertexts satisfy it (in BGV every coefficient of the residue is a multiple of t); ciphertexts that
    fhe_encrypt_pk_blake2 makes from the RECORDED public key satisfy the same bound and decrypt to the recorded message (BGV:
    fhe_bgv_decrypt; BFV: round(t / Q * (c0 + c1 * s)) mod t with python integers; CKKS: the bound alone).  The plaintext encoded one
    level down pins the use of the key's first rows.  The randomness of the seeded form is ours (blake2 in counter mode), not the
    reference's sequential stream: its words are pinned on its composition (tests/test_parity_encrypt.py), not on the record.

`backend` = the lane emulator on the CPU, the product library with -m gpu."""
import ctypes as C
import os

import numpy as np
import pytest

from openfhe_amd import fhe_hip as fh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_vectors_encrypt.npz")
META = ("ring", "ns", "numQ", "t", "sigma100", "gaussian", "downLimbs")
SETS = ("ckks_", "ckksg_", "bgv_", "bfv_")
CASES = [("ckks_", ""), ("ckks_", "d"), ("ckksg_", ""), ("bgv_", ""), ("bfv_", "")]
KEY = bytes(range(50, 114))
_rec = {}


def obj(a):
    return np.asarray(a).astype(object)


class Rec:
    """one recorded parameter set with everything the checks share, computed once on the CPU"""

    def __init__(self, o, pre):
        z = np.load(GOLDEN)  # (a missing fixture is an error, not a skip)
        self.o, self.pre = o, pre
        self.g = g = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
        g.update(zip(META, (int(v) for v in g["meta"])))
        self.N, self.numQ, self.ns, self.t, self.sigma = g["ring"], g["numQ"], g["ns"], g["t"], g["sigma100"] / 100.0
        self.qs, self.psi, self.s = g["q"], g["psi"], g["s"]
        self.bfv = pre == "bfv_"
        self.octx = o.orc_ctx_create(self.N, self.numQ, self.qs, self.psi)
        vals, a = (C.c_double * 4096)(), C.c_double()
        self.B = o.orc_dgg_table(self.sigma, vals, 4096, C.byref(a))  # the table's length: the largest |integer| drawn
        self.bound = 2 * self.N * self.B * (self.B if g["gaussian"] else 1) + self.B

    def ntt_row(self, row, limb, inverse):
        x = np.ascontiguousarray(row, dtype=np.uint64).reshape(1, 1, self.N).copy()
        f = self.o.orc_ntt_inv_tower if inverse else self.o.orc_ntt_fwd_tower
        f(self.octx, x, np.array([limb], np.uint32).ctypes.data_as(C.c_void_p), 1, 1, 0)
        return x[0, 0]

    def centred_row(self, row, limb):
        q = int(self.qs[limb])
        return [int(v) - q if int(v) > q // 2 else int(v) for v in self.ntt_row(row, limb, True)]

    def scaled(self, pt):
        """DCRTPoly::TimesQovert of the COEFFICIENT plaintext with python integers (dcrtpoly-impl.h:868-885)"""
        neg, tinv = int(self.g["negQModt"][0]), self.g["tInvModq"]
        return np.stack([((obj(pt[i]) * neg % self.t) * int(tinv[i]) % int(self.qs[i])).astype(np.uint64) for i in range(len(pt))])

    def message(self, tag):
        """the EVALUATION tower Encrypt adds to c0: the plaintext itself, or BFV's scaled plaintext transformed"""
        pt = self.g["pt" + tag]
        if not self.bfv:
            return pt
        return np.stack([self.ntt_row(row, i, False) for i, row in enumerate(self.scaled(pt))])

    def integers(self, rows):
        """EVALUATION rows [L][N] -> the N integers they hold, centred over Q_L (CRT with python integers)"""
        L = len(rows)
        coef = [self.ntt_row(rows[i], i, True) for i in range(L)]
        Q = 1
        for q in self.qs[:L]:
            Q *= int(q)
        out = []
        for n in range(self.N):
            x = 0
            for i in range(L):
                q = int(self.qs[i])
                x += int(coef[i][n]) * (Q // q) * pow(Q // q, -1, q)
            x %= Q
            out.append(x - Q if x > Q // 2 else x)
        return out, Q

    def phase(self, c0, c1, m=None):
        """c0 + c1 * s (- m) per limb, EVALUATION"""
        rows = []
        for i in range(len(c0)):
            q = int(self.qs[i])
            v = obj(c0[i]) + obj(c1[i]) * obj(self.s[i])
            rows.append(((v - obj(m[i]) if m is not None else v) % q).astype(np.uint64))
        return np.stack(rows)

    def check_residue(self, c0, c1, tag, what):
        """the decryption residue is ns * r with |r| within the derived bound, and not zero"""
        res, _ = self.integers(self.phase(c0, c1, self.message(tag)))
        assert all(v % self.ns == 0 for v in res), f"{what}: the residue is not a multiple of the noise scale"
        top = max(abs(v) // self.ns for v in res)
        assert 0 < top <= self.bound, (what, top, self.bound)

    def plain_mod_t(self, tag):
        """the recorded message: the plaintext's integer coefficients modulo t"""
        pt, q = self.g["pt" + tag], int(self.qs[0])
        vals = [int(v) - q if int(v) > q // 2 else int(v) for v in pt[0]] if self.bfv else self.centred_row(pt[0], 0)  # (BFV's is COEFFICIENT)
        return np.array([v % self.t for v in vals], np.uint64)

    def bfv_decrypt(self, c0, c1):
        """round(t / Q * (c0 + c1 * s)) mod t with python integers"""
        y, Q = self.integers(self.phase(c0, c1))
        return np.array([((2 * self.t * v + Q) // (2 * Q)) % self.t for v in y], np.uint64)


def rec(o, pre):
    if pre not in _rec:
        _rec[pre] = Rec(o, pre)
    return _rec[pre]


def test_the_record_is_what_the_generator_checked():
    z = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 1 << 20 and all(z[k].dtype == np.uint64 for k in z.files), "data only, small enough to commit"
    for pre, ns, numQ, t, gaussian, down in (("ckks_", 1, 3, 0, 0, 2), ("ckksg_", 1, 3, 0, 1, 0), ("bgv_", 65537, 3, 65537, 0, 0),
                                              ("bfv_", 1, 2, 65537, 0, 0)):
        g = dict(zip(META, (int(v) for v in z[pre + "meta"])))
        assert g == dict(ring=64, ns=ns, numQ=numQ, t=t, sigma100=319, gaussian=gaussian, downLimbs=down), pre
        for k in ("s", "pkB", "pkA", "pt", "sk0", "sk1", "pk0", "pk1"):
            assert z[pre + k].shape == (numQ, 64), (pre, k)
        if down:
            for k in ("ptd", "skd0", "skd1", "pkd0", "pkd1"):
                assert z[pre + k].shape == (down, 64), (pre, k)
    assert all(int(q) % 65537 == 1 for q in z["bgv_q"]), "BGV's moduli are 1 modulo t: ModReduce leaves the message unscaled"
    assert z["bfv_tInvModq"].shape == (2,) and z["bfv_negQModt"].shape == (1,)


def recovered(r, tag):
    """(a, e) of the recorded secret-key ciphertext, EVALUATION towers [L][N]"""
    c0, c1, m = r.g["sk" + tag + "0"], r.g["sk" + tag + "1"], r.message(tag)
    a, e = np.empty_like(c1), np.empty_like(c0)
    for i in range(len(c0)):
        q = int(r.qs[i])
        a[i] = ((q - obj(c1[i])) % q).astype(np.uint64)
        e[i] = ((obj(c0[i]) - obj(m[i]) - obj(a[i]) * obj(r.s[i])) * pow(r.ns, -1, q) % q).astype(np.uint64)
    return a, e


@pytest.mark.parametrize("pre,tag", CASES)
def test_secret_key_form_the_recovered_error_is_one_small_polynomial(oracle, pre, tag):
    r = rec(oracle, pre)
    assert r.B == 39  # ceil(12.00610553538285 * 3.19)
    a, e = recovered(r, tag)
    rows = [r.centred_row(e[i], i) for i in range(len(e))]
    assert all(row == rows[0] for row in rows), f"{pre}{tag}: the limbs do not hold one integer polynomial"
    assert 0 < max(abs(v) for v in rows[0]) <= r.B, (pre, tag, max(abs(v) for v in rows[0]))
    sec = r.centred_row(r.s[0], 0)
    assert (max(abs(v) for v in sec) <= r.B and max(abs(v) for v in sec) > 1) if r.g["gaussian"] else set(sec) <= {-1, 0, 1}
    if tag == "":  # the check can fail: with the sign of a wrong, the recovered words are uniform residues
        q = int(r.qs[0])
        wrong = ((obj(r.g["sk0"][0]) - obj(r.message("")[0]) + obj(a[0]) * obj(r.s[0])) * pow(r.ns, -1, q) % q).astype(np.uint64)
        assert max(abs(v) for v in r.centred_row(wrong, 0)) > 1 << 40


@pytest.mark.parametrize("pre,tag", CASES)
def test_secret_key_form_reproduces_the_record_word_for_word(backend, oracle, pre, tag):
    r = rec(oracle, pre)
    a, e = recovered(r, tag)
    L = len(a)
    ctx = fh.Context(backend, r.N.bit_length() - 1, r.qs, r.psi)
    try:
        s = ctx.tower(r.s)  # all numQ rows: a plaintext one level down meets the first of them
        if r.bfv:
            pt = ctx.tower(r.g["pt"], fmt=fh.COEFFICIENT)
            m = fh._bfv_scaled(ctx, pt, r.t, int(r.g["negQModt"][0]), r.g["tInvModq"], None)
            assert np.array_equal(m.to_host()[0], r.scaled(r.g["pt"]))
            joined = ctx.tower(e).SwitchFormat().Plus(m).SwitchFormat()  # e and the scaled message meet in COEFFICIENT format
            c0, c1 = fh.encrypt_sk_combine(ctx, s, ctx.tower(a), joined, None, r.ns)
        else:
            c0, c1 = fh.encrypt_sk_combine(ctx, s, ctx.tower(a), ctx.tower(e), ctx.tower(r.g["pt" + tag]), r.ns)
        assert c0.n_limbs == L
        assert np.array_equal(c1.to_host()[0], r.g["sk" + tag + "1"]) and np.array_equal(c0.to_host()[0], r.g["sk" + tag + "0"])
    finally:
        ctx.close()


@pytest.mark.parametrize("pre,tag", CASES)
def test_public_key_form_the_recorded_residue_is_within_the_derived_bound(oracle, pre, tag):
    r = rec(oracle, pre)
    assert r.bound == (2 * 64 * 39 * 39 + 39 if pre == "ckksg_" else 2 * 64 * 39 + 39)
    r.check_residue(r.g["pk" + tag + "0"], r.g["pk" + tag + "1"], tag, f"{pre}{tag} recorded")
    r.check_residue(r.g["sk" + tag + "0"], r.g["sk" + tag + "1"], tag, f"{pre}{tag} recorded, secret key")
    if r.bfv:  # the CPU decryption used below recovers the recorded message from the recorded ciphertext
        assert np.array_equal(r.bfv_decrypt(r.g["pk0"], r.g["pk1"]), r.plain_mod_t(""))
    if pre == "ckks_" and tag == "":  # the check can fail: without the message taken off, the residue is as large as the scaled message
        res, _ = r.integers(r.phase(r.g["pk0"], r.g["pk1"]))
        assert max(abs(v) for v in res) > 1 << 40


@pytest.mark.parametrize("pre,tag", CASES)
def test_public_key_form_device_ciphertexts_meet_the_bound_and_decrypt(backend, oracle, pre, tag):
    """ciphertexts fhe_encrypt_pk_blake2 makes from the RECORDED public key, v from the sampler the reference uses for the set (Gaussian
    under SecretKeyDist == GAUSSIAN, ternary otherwise), with the workspace behind the ciphertexts and apart from them"""
    r = rec(oracle, pre)
    v_dist = fh.GAUSSIAN if r.g["gaussian"] else fh.TERNARY
    L = len(r.g["pt" + tag])
    ctx = fh.Context(backend, r.N.bit_length() - 1, r.qs, r.psi)
    try:
        pk_b, pk_a = ctx.tower(r.g["pkB"]), ctx.tower(r.g["pkA"])
        nv, ne = fh.encrypt_counters(ctx, L, 1)
        for contiguous in (True, False):
            if r.bfv:
                pt = ctx.tower(r.g["pt"], fmt=fh.COEFFICIENT)
                c0, c1 = fh.bfv_encrypt_pk_blake2(ctx, pk_b, pk_a, pt, r.t, int(r.g["negQModt"][0]), r.g["tInvModq"], KEY, 3, 3 + nv,
                                                  sigma=r.sigma, v_dist=v_dist, contiguous=contiguous)
            else:
                c0, c1 = fh.encrypt_pk_blake2(ctx, pk_b, pk_a, 1, KEY, 3, 3 + nv, n_limbs=L, msg=ctx.tower(r.g["pt" + tag]), ns=r.ns,
                                              sigma=r.sigma, v_dist=v_dist, contiguous=contiguous)
            h0, h1 = c0.to_host()[0], c1.to_host()[0]
            assert h0.shape == (L, r.N)
            r.check_residue(h0, h1, tag, f"{pre}{tag} device")
            if pre == "bgv_":
                assert np.array_equal(fh.bgv_decrypt(ctx, [c0, c1], ctx.tower(r.s), r.t)[0], r.plain_mod_t(tag))
            if r.bfv:
                assert np.array_equal(r.bfv_decrypt(h0, h1), r.plain_mod_t(tag))
        if r.bfv:  # and the secret-key helper
            c0, c1 = fh.bfv_encrypt_sk_blake2(ctx, ctx.tower(r.s), pt, r.t, int(r.g["negQModt"][0]), r.g["tInvModq"], KEY, 100, 200, sigma=r.sigma)
            h0, h1 = c0.to_host()[0], c1.to_host()[0]
            r.check_residue(h0, h1, tag, "bfv_ device, secret key")
            assert np.array_equal(r.bfv_decrypt(h0, h1), r.plain_mod_t(tag))
    finally:
        ctx.close()
