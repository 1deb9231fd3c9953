"""BV key generation against keys recorded from the reference itself (tests/golden/ref_vectors_keygen_bv.npz, written by
tests/golden/make_golden_keygen_bv.py): the secret key, the EvalMultKeyGen key, the EvalRotateKeyGen keys of +1 and -1, a second key pair
and ReKeyGen(sk, pk') at ring 64, for BFV with t = 65537 and three 60-bit limbs at digit sizes 0 and 10 and for CKKS FIXEDMANUAL with limbs
of 60 / 50 / 51 bits at digit size 10 (6 + 5 + 6 towers).

The reference never exposes the error of a key.  It is recovered on the CPU,
    secret-key form   e[d][i] = (b[d][i] + a[d][i] * sigma_kNew(s)[i] - f[d][i] * sOld[i]) * ns^-1  mod q_i,
and must come out as ONE polynomial of small signed integers per tower: the centred inverse transforms of all limbs agree and no
coefficient exceeds B, the length of the Gaussian sampler's inversion table (ceil(12.006 sigma): no larger integer can be drawn).  With a
wrong digit order, window power or factor limb the recovered words are uniform residues instead.  Feeding the recovered e and the recorded
a to the device must then give the recorded b word for word.
    public-key form   (b[d][i] + a[d][i] * s'[i] - f[d][i] * s[i]) * ns^-1 = e_pk' * u + e0 + e1 * s'
is one integer polynomial per tower as well, bounded by B * (2 N + 1) for ternary u and s' (e_pk' = pk'_0 + pk'_1 * s' is the error of the
second public key).  The recorded key is held against that bound first, then a key the device makes with fhe_bv_keygen_pk_blake2.
End to end on the device, BFV sets: the recorded ciphertext re-encrypted with the device-made key (and with the recorded one) decrypts
under s' to the recorded NativePoly; squared with a seeded EvalMult key through fhe_bfv_eval_mult_relin_hps_bv it decrypts to the
plaintext's square modulo t.  `backend` = the lane emulator on the CPU, the product library with -m gpu."""
import ctypes as C
import os

import numpy as np
import pytest

from openfhe_amd import fhe_hip as fh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_vectors_keygen_bv.npz")
META = ("ring", "ns", "numQ", "r", "D0", "kPlus", "kMinus", "sigma100", "t")
SETS = ("bfv0_", "bfv10_", "ckks10_")
BFV = ("bfv0_", "bfv10_")
KEY = bytes(range(60, 124))
_rec = {}


def mulmod(a, b, q):
    """object arrays of python integers (exact)"""
    return (np.asarray(a).astype(object) * np.asarray(b).astype(object)) % int(q)


class Rec:
    """one recorded parameter set with everything the checks share, computed once on the CPU; read-only"""

    def __init__(self, o, pre):
        z = np.load(GOLDEN)  # (a missing fixture is an error, not a skip)
        self.o, self.pre = o, pre
        self.g = g = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
        g.update(zip(META, (int(v) for v in g["meta"])))
        self.N, self.numQ, self.r, self.D0, self.ns, self.t = g["ring"], g["numQ"], g["r"], g["D0"], g["ns"], g["t"]
        self.qs, self.psi, self.s, self.s2 = g["q"], g["psiQ"], g["s"], g["s2"]
        self.octx = o.orc_ctx_create(self.N, self.numQ, self.qs, self.psi)
        self.f = np.array(fh.bv_keygen_factors(self.qs, self.r), np.uint64)
        self.ss = np.stack([mulmod(self.s[i], self.s[i], q) for i, q in enumerate(self.qs)]).astype(np.uint64)
        inv = lambda k: pow(k, -1, 2 * self.N)
        # name -> (b, a, kNew, sOld): EvalMultKeyGen switches s^2 to s; EvalAutomorphismKeyGen(k) switches s to sigma_{k^-1}(s)
        self.keys = {"mul": (g["mulB"], g["mulA"], 1, self.ss), "rotP": (g["rotPB"], g["rotPA"], inv(g["kPlus"]), self.s),
                     "rotM": (g["rotMB"], g["rotMA"], inv(g["kMinus"]), self.s)}
        vals, a = (C.c_double * 4096)(), C.c_double()
        self.bound = o.orc_dgg_table(g["sigma100"] / 100.0, vals, 4096, C.byref(a))  # the table's length: the largest |integer| drawn
        self.e = {name: self.recover_e(*k) for name, k in self.keys.items()}

    def ntt_row(self, row, limb, inverse):
        x = np.ascontiguousarray(row, dtype=np.uint64).reshape(1, 1, self.N).copy()
        f = self.o.orc_ntt_inv_tower if inverse else self.o.orc_ntt_fwd_tower
        f(self.octx, x, np.array([limb], np.uint32).ctypes.data_as(C.c_void_p), 1, 1, 0)
        return x[0, 0]

    def perm(self, row, k):
        if k == 1:
            return row
        out = np.empty(self.N, np.uint64)
        self.o.orc_automorph_eval_k(out, np.ascontiguousarray(row), self.N, k)
        return out

    def recover_e(self, b, a, k_new, s_old, factor=None, s_new=None):
        """(b + a * sigma_kNew(sNew) - f * sOld) * ns^-1, [D0][numQ][N]"""
        f = self.f if factor is None else factor
        s_new = self.s if s_new is None else s_new
        e = np.empty_like(b)
        for d in range(self.D0):
            for i, q in enumerate(int(v) for v in self.qs):
                v = b[d, i].astype(object) + mulmod(a[d, i], self.perm(s_new[i], k_new), q)
                if f[d, i]:
                    v = v - mulmod(s_old[i], np.array([f[d, i]], np.uint64), q)
                e[d, i] = ((v % q) * pow(self.ns, -1, q) % q).astype(np.uint64)
        return e

    def centred(self, row, limb):
        q = int(self.qs[limb])
        return [int(v) - q if int(v) > q // 2 else int(v) for v in self.ntt_row(row, limb, True)]

    def one_polynomial(self, e, what):
        """max |coefficient| over all towers, after asserting that every tower is the same integer polynomial in every limb"""
        worst = 0
        for d in range(self.D0):
            rows = [self.centred(e[d, i], i) for i in range(self.numQ)]
            assert all(row == rows[0] for row in rows), f"{self.pre}{what} tower {d}: the limbs do not hold one integer polynomial"
            assert any(rows[0]), f"{self.pre}{what} tower {d}: no noise at all"
            worst = max(worst, max(abs(v) for v in rows[0]))
        return worst


def rec(o, pre):
    if pre not in _rec:
        _rec[pre] = Rec(o, pre)
    return _rec[pre]


def test_the_record_is_what_the_generator_checked():
    z = np.load(GOLDEN)
    for pre, r, D0, t, bits in (("bfv0_", 0, 3, 65537, (60, 60, 60)), ("bfv10_", 10, 18, 65537, (60, 60, 60)), ("ckks10_", 10, 17, 0, (60, 50, 51))):
        g = dict(zip(META, (int(v) for v in z[pre + "meta"])))
        assert (g["ring"], g["ns"], g["numQ"], g["r"], g["D0"], g["t"], g["sigma100"]) == (64, 1, 3, r, D0, t, 319)
        assert tuple(int(v) for v in z[pre + "meta"][len(META):]) == bits == tuple(int(q).bit_length() for q in z[pre + "q"])
        assert (g["kPlus"] * g["kMinus"]) % 128 == 1 and g["kPlus"] != g["kMinus"]
        for k in ("s", "pkB", "pkA", "s2", "pk2B", "pk2A"):
            assert z[pre + k].shape == (3, 64)
        for k in ("mulB", "mulA", "rotPB", "rotPA", "rotMB", "rotMA", "reB", "reA"):
            assert z[pre + k].shape == (D0, 3, 64)
        if t:
            assert z[pre + "ct"].shape == (2, 3, 64) and z[pre + "m"].shape == (64,) and np.array_equal(z[pre + "m"], z[pre + "reM"])
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("pre", SETS)
def test_recovered_errors_are_one_small_polynomial_per_tower(oracle, pre):
    r = rec(oracle, pre)
    assert r.bound == 39  # ceil(12.00610553538285 * 3.19)
    for name, e in r.e.items():
        assert r.one_polynomial(e, name) <= r.bound, (pre, name)
    assert set(r.centred(r.s[0], 0)) <= {-1, 0, 1} and set(r.centred(r.s2[0], 0)) <= {-1, 0, 1}
    # the check can fail: a wrong automorphism index leaves uniform residues; with digits (r > 0) so do the towers in another order, the
    # factor at another limb and a window's power off by one digit (at r = 0 every factor is 1 and sOld itself is small)
    b, a, k_new, s_old = r.keys["rotP"]

    def passes(e):
        for d in range(r.D0):
            rows = [r.centred(e[d, i], i) for i in range(r.numQ)]
            if any(row != rows[0] for row in rows) or max(abs(v) for v in rows[0]) > r.bound:
                return False
        return True

    assert passes(r.e["rotP"]) and not passes(r.recover_e(b, a, r.g["kPlus"], s_old))
    if r.r:
        assert not passes(r.recover_e(b, a, k_new, s_old, factor=r.f[::-1]))
        assert not passes(r.recover_e(b, a, k_new, s_old, factor=np.roll(r.f, 1, axis=1)))
        off = r.f.copy()  # window k at 2^((r + 1) k) instead of 2^(r k)
        for d, i in zip(*np.nonzero(off)):
            k = int(off[d, i]).bit_length() - 1 if int(off[d, i]) < (1 << 59) else None  # (a power below q_i is not reduced: its exponent)
            if k:
                off[d, i] = pow(2, k // r.r * (r.r + 1), int(r.qs[i]))
        assert not np.array_equal(off, r.f) and not passes(r.recover_e(b, a, k_new, s_old, factor=off))


class Setup:
    def __init__(self, backend, r):
        logN = r.N.bit_length() - 1
        self.hps = None
        if r.t:
            rq, psiR = backend.hps_r(logN, r.qs, fh.HPSPOVERQLEVELED)
            assert np.array_equal(rq, r.g["r_q"]) and np.array_equal(psiR, r.g["r_psiQ"])
            self.ctx = fh.Context(backend, logN, np.concatenate([r.qs, rq]), np.concatenate([r.psi, psiR]))
            self.hps = fh.Hps(self.ctx, np.arange(r.numQ), np.arange(r.numQ, 2 * r.numQ), r.t, fh.HPSPOVERQLEVELED)
            self.dec = fh.BfvDecrypt(self.ctx, r.t, fh.BfvDecrypt.HPSPOVERQLEVELED, size_q=r.numQ)
        else:
            self.ctx = fh.Context(backend, logN, r.qs, r.psi)
        self.s, self.s2, self.ss = self.ctx.tower(r.s), self.ctx.tower(r.s2), self.ctx.tower(r.ss)

    def close(self):
        if self.hps:
            self.hps.close()
            self.dec.close()
        self.ctx.close()


@pytest.mark.parametrize("pre", SETS)
def test_device_reproduces_the_recorded_keys(backend, oracle, pre):
    r = rec(oracle, pre)
    d = Setup(backend, r)
    try:
        b, a, _, _ = r.keys["mul"]
        got, _, keys = fh.BvKey.keygen(d.ctx, r.r, d.s, d.ss, d.ctx.tower(a), d.ctx.tower(r.e["mul"]), ns=r.ns)
        assert np.array_equal(got.to_host(), b), "EvalMultKeyGen"
        keys[0].close()
        # both rotation keys in one call, from the rotation indices
        a2 = np.concatenate([r.keys["rotP"][1], r.keys["rotM"][1]])
        e2 = np.concatenate([r.e["rotP"], r.e["rotM"]])
        got, _, keys = fh.BvKey.keygen(d.ctx, r.r, d.s, d.s, d.ctx.tower(a2), d.ctx.tower(e2), 2, ns=r.ns, rotations=[1, -1])
        assert np.array_equal(got.to_host(), np.concatenate([r.keys["rotP"][0], r.keys["rotM"][0]])), "EvalRotateKeyGen({1, -1})"
        assert sorted(keys) == [-1, 1]
        for k in keys.values():
            k.close()
    finally:
        d.close()


def device_rekey(d, r):
    nu, ne = fh.bv_keygen_counters(d.ctx, r.numQ, r.r, 1, fh.PUBLIC_KEY_FORM)
    return fh.BvKey.keygen_pk_blake2(d.ctx, r.r, d.ctx.tower(r.g["pk2B"]), d.ctx.tower(r.g["pk2A"]), d.s, 1, KEY, 3, 3 + nu, ns=r.ns,
                                     sigma=r.g["sigma100"] / 100.0)


@pytest.mark.parametrize("pre", SETS)
def test_public_key_form_residue_is_one_bounded_polynomial(backend, oracle, pre):
    r = rec(oracle, pre)
    limit = r.bound * (2 * r.N + 1)
    # the reference alone must pass ...
    ref = r.one_polynomial(r.recover_e(r.g["reB"], r.g["reA"], 1, r.s, s_new=r.s2), "ReKeyGen")
    assert ref <= limit, (pre, ref)
    # ... (and can fail: the residue taken under the wrong secret is uniform) ...
    wrong = r.recover_e(r.g["reB"], r.g["reA"], 1, r.s, s_new=r.s)
    assert max(abs(v) for v in r.centred(wrong[0, 0], 0)) > 1 << 40
    # ... then the key the device makes
    d = Setup(backend, r)
    try:
        b, a, keys = device_rekey(d, r)
        dev = r.one_polynomial(r.recover_e(b.to_host(), a.to_host(), 1, r.s, s_new=r.s2), "fhe_bv_keygen_pk_blake2")
        print(f"{pre}: max |residue| recorded {ref}, device {dev}, bound {limit}")
        assert dev <= limit, (pre, dev)
        keys[0].close()
    finally:
        d.close()


@pytest.mark.parametrize("pre", BFV)
def test_pre_end_to_end(backend, oracle, pre):
    """ReEncrypt = the second element switched, the first added (base-pre.cpp); decrypted under the delegatee's secret"""
    r = rec(oracle, pre)
    d = Setup(backend, r)
    try:
        c0, c1 = d.ctx.tower(r.g["ct"][0]), d.ctx.tower(r.g["ct"][1])
        assert np.array_equal(d.dec.Decrypt([c0, c1], d.s), r.g["m"][None]), "the recorded ciphertext under its own secret"
        b, a, keys = device_rekey(d, r)
        recorded = fh.BvKey(d.ctx, r.numQ, r.r, r.g["reB"], r.g["reA"])
        for name, key in (("device-made", keys[0]), ("recorded", recorded)):
            o0, o1 = key.KeySwitchCore(c1)
            assert np.array_equal(d.dec.Decrypt([c0.Plus(o0), o1], d.s2), r.g["m"][None]), f"{name} re-encryption key"
            assert not np.array_equal(d.dec.Decrypt([c0.Plus(o0), o1], d.s), r.g["m"][None]), "the old secret no longer decrypts"
        keys[0].close()
        recorded.close()
    finally:
        d.close()


@pytest.mark.parametrize("pre", BFV)
def test_relinearisation_end_to_end(backend, oracle, pre):
    r = rec(oracle, pre)
    d = Setup(backend, r)
    try:
        na, ne = fh.bv_keygen_counters(d.ctx, r.numQ, r.r, 1)
        _, _, keys = fh.BvKey.keygen_blake2(d.ctx, r.r, d.s, d.ss, 1, KEY, 40, 40 + na, ns=r.ns, sigma=r.g["sigma100"] / 100.0)
        li = np.arange(r.numQ)
        c0, c1 = d.ctx.tower(r.g["ct"][0][None], limb_idx=li), d.ctx.tower(r.g["ct"][1][None], limb_idx=li)
        p0, p1 = d.hps.EvalMult(keys[0], c0, c1, c0, c1)
        m = [int(v) for v in r.g["m"]]
        want = [0] * r.N
        for i in range(r.N):  # the square modulo (X^N + 1, t)
            for j in range(r.N):
                k, sign = (i + j) % r.N, -1 if i + j >= r.N else 1
                want[k] = (want[k] + sign * m[i] * m[j]) % r.t
        assert np.array_equal(d.dec.Decrypt([p0, p1], d.s)[0], np.array(want, np.uint64))
        keys[0].close()
    finally:
        d.close()
