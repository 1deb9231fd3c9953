"""Key generation against keys recorded from the reference itself (tests/golden/ref_vectors_keygen.npz, written by
tests/golden/make_golden_keygen.py): the secret key, the public key, the EvalMultKeyGen key and the EvalRotateKeyGen keys of +1 and -1 at
ring 64, for CKKS on HYBRID keys with 2 digits of 2 and 1 limbs, and for BGV FIXEDMANUAL with t = 65537 on HYBRID keys.

The reference never exposes the error e of a key.  It is recovered on the CPU,
    e[j][i] = (b[j][i] + a[j][i] * sNewExt[i] - f[j][i] * sOld[i]) * ns^-1  mod q_i,
and must come out as ONE polynomial of small signed integers per digit: the centred inverse transforms of all limbs agree, and no
coefficient exceeds the length of the Gaussian sampler's inversion table, ceil(12.006 sigma) (discretegaussiangenerator-impl.h:75-89: no
larger integer can be drawn).  With a wrong sign, factor table, digit partition, secret extension or automorphism index the recovered
words are uniform residues instead: that check is what pins the formula on the reference.  Feeding the recovered e and the recorded a to
the device must then give the recorded b word for word.

The seeded form has no recording (its randomness is ours): a key it makes must switch keys with the noise the reference's recorded key
gives, and in BGV the noise must be divisible by t.  `backend` = the lane emulator on the CPU, the product library with -m gpu."""
import ctypes as C
import os

import numpy as np
import pytest

from openfhe_amd import fhe_hip as fh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_vectors_keygen.npz")
META = ("ring", "ns", "numQ", "numP", "dnum", "alpha", "kPlus", "kMinus", "sigma100")
SETS = ("ckks_", "bgv_")
KEY = bytes(range(100, 164))
_rec = {}


def mulmod(a, b, q):
    """object arrays of python integers (exact)"""
    return (np.asarray(a).astype(object) * np.asarray(b).astype(object)) % int(q)


class Rec:
    """one recorded parameter set with everything the checks share, computed once on the CPU"""

    def __init__(self, o, pre):
        z = np.load(GOLDEN)  # (a missing fixture is an error, not a skip)
        self.o, self.pre = o, pre
        self.g = g = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
        g.update(zip(META, (int(v) for v in g["meta"])))
        self.N, self.numQ, self.numP, self.dnum, self.ns = g["ring"], g["numQ"], g["numP"], g["dnum"], g["ns"]
        N, numQ, numP = self.N, self.numQ, self.numP
        self.qs, self.psi = np.concatenate([g["q"], g["p"]]), np.concatenate([g["psiQ"], g["psiP"]])
        self.octx = o.orc_ctx_create(N, numQ + numP, self.qs, self.psi)
        self.s = g["s"]
        # sNewExt (keyswitch-hybrid.cpp:59-83) on the CPU: limb 0 in COEFFICIENT format, centre-switched to p_j, transformed
        coef0 = self.intt(self.s[0], 0)
        self.s_ext = np.concatenate([self.s, np.stack([self.ntt(self.switch(coef0, 0, numQ + j), numQ + j) for j in range(numP)])])
        P = 1
        for v in g["p"]:
            P *= int(v)
        self.f = np.zeros((self.dnum, numQ + numP), np.uint64)
        for j in range(self.dnum):
            for i in range(g["alpha"] * j, min(g["alpha"] * (j + 1), numQ)):
                self.f[j, i] = P % int(self.qs[i])
        s2 = np.stack([mulmod(self.s[i], self.s[i], self.qs[i]) for i in range(numQ)]).astype(np.uint64)
        inv = lambda k: pow(k, -1, 2 * N)
        # name -> (b, a, kNew, sOld): EvalMultKeyGen switches s^2 to s; EvalAutomorphismKeyGen(k) switches s to sigma_{k^-1}(s)
        self.keys = {"mul": (g["mulB"], g["mulA"], 1, s2), "rotP": (g["rotPB"], g["rotPA"], inv(g["kPlus"]), self.s),
                     "rotM": (g["rotMB"], g["rotMA"], inv(g["kMinus"]), self.s)}
        vals, a = (C.c_double * 4096)(), C.c_double()
        self.bound = o.orc_dgg_table(g["sigma100"] / 100.0, vals, 4096, C.byref(a))  # the table's length: the largest |integer| drawn
        self.e = {name: self.recover_e(*k) for name, k in self.keys.items()}
        self.e_pk = np.stack([mulmod((self.g["pkB"][i].astype(object) + mulmod(g["pkA"][i], self.s[i], q)) % int(q),
                                     np.array([pow(self.ns, -1, int(q))], object), q) for i, q in enumerate(self.qs[:numQ])]).astype(np.uint64)

    def ntt_row(self, row, limb, inverse):
        x = np.ascontiguousarray(row, dtype=np.uint64).reshape(1, 1, self.N).copy()
        f = self.o.orc_ntt_inv_tower if inverse else self.o.orc_ntt_fwd_tower
        f(self.octx, x, np.array([limb], np.uint32).ctypes.data_as(C.c_void_p), 1, 1, 0)
        return x[0, 0]

    def intt(self, row, limb):
        return self.ntt_row(row, limb, True)

    def ntt(self, row, limb):
        return self.ntt_row(row, limb, False)

    def switch(self, row, src, dst):
        v = row.copy()
        self.o.orc_switch_modulus(v, self.N, int(self.qs[src]), int(self.qs[dst]))
        return v

    def perm(self, row, k):
        if k == 1:
            return row
        out = np.empty(self.N, np.uint64)
        self.o.orc_automorph_eval_k(out, np.ascontiguousarray(row), self.N, k)
        return out

    def recover_e(self, b, a, k_new, s_old):
        e = np.empty_like(b)
        for j in range(self.dnum):
            for i, q in enumerate(int(v) for v in self.qs):
                v = b[j, i].astype(object) + mulmod(a[j, i], self.perm(self.s_ext[i], k_new), q)
                if self.f[j, i]:
                    v = v - mulmod(s_old[i], np.array([self.f[j, i]], np.uint64), q)
                e[j, i] = ((v % q) * pow(self.ns, -1, q) % q).astype(np.uint64)
        return e

    def centred(self, row, limb):
        q = int(self.qs[limb])
        return [int(v) - q if int(v) > q // 2 else int(v) for v in self.intt(row, limb)]


def rec(o, pre):
    if pre not in _rec:
        _rec[pre] = Rec(o, pre)
    return _rec[pre]


def test_the_record_is_what_the_generator_checked():
    z = np.load(GOLDEN)
    for pre, ns, numQ in (("ckks_", 1, 3), ("bgv_", 65537, 4)):
        g = dict(zip(META, (int(v) for v in z[pre + "meta"])))
        assert g["ring"] == 64 and g["ns"] == ns and g["dnum"] == 2 and g["numQ"] == numQ and g["sigma100"] == 319
        assert (g["kPlus"] * g["kMinus"]) % 128 == 1 and g["kPlus"] != g["kMinus"]
        assert z[pre + "s"].shape == z[pre + "pkB"].shape == z[pre + "pkA"].shape == (numQ, 64)
        for k in ("mulB", "mulA", "rotPB", "rotPA", "rotMB", "rotMA"):
            assert z[pre + k].shape == (2, numQ + g["numP"], 64)
    g = dict(zip(META, (int(v) for v in z["ckks_meta"])))
    assert g["alpha"] * g["dnum"] > g["numQ"], "the CKKS set's last digit is shorter than the others"


@pytest.mark.parametrize("pre", SETS)
def test_recovered_errors_are_one_small_polynomial_per_digit(oracle, pre):
    r = rec(oracle, pre)
    assert r.bound == 39  # ceil(12.00610553538285 * 3.19)
    for name, e in r.e.items():
        for j in range(r.dnum):
            rows = [r.centred(e[j, i], i) for i in range(r.numQ + r.numP)]
            assert all(row == rows[0] for row in rows), f"{pre}{name} digit {j}: the limbs do not hold one integer polynomial"
            assert 0 < max(abs(v) for v in rows[0]) <= r.bound, (pre, name, j, max(abs(v) for v in rows[0]))
    rows = [r.centred(r.e_pk[i], i) for i in range(r.numQ)]
    assert all(row == rows[0] for row in rows) and 0 < max(abs(v) for v in rows[0]) <= r.bound, f"{pre}public key"
    # the secret itself is ternary, and a wrong automorphism index does NOT give a small error (the check can fail)
    assert set(r.centred(r.s[0], 0)) <= {-1, 0, 1}
    b, a, k_new, s_old = r.keys["rotP"]
    wrong = r.recover_e(b, a, r.g["kPlus"], s_old)
    assert max(abs(v) for v in r.centred(wrong[0, 0], 0)) > 1 << 40


class Setup:
    def __init__(self, backend, r):
        self.ctx = fh.Context(backend, r.N.bit_length() - 1, r.qs, r.psi)
        self.plan = fh.KeySwitchPlan(self.ctx, r.numQ, r.numP, r.dnum)
        self.s = self.ctx.tower(r.s)
        self.s_ext = self.plan.extend_secret(self.s)

    def close(self):
        self.plan.close()
        self.ctx.close()


@pytest.mark.parametrize("pre", SETS)
def test_device_reproduces_the_recorded_keys(backend, oracle, pre):
    r = rec(oracle, pre)
    d = Setup(backend, r)
    try:
        assert np.array_equal(d.s_ext.to_host()[0], r.s_ext), "fhe_ks_secret_extend"
        b, a, k_new, s2 = r.keys["mul"]
        got, _, keys = d.plan.keygen(d.s_ext, d.ctx.tower(s2), d.ctx.tower(a), d.ctx.tower(r.e["mul"]), ns=r.ns)
        assert np.array_equal(got.to_host(), b), "EvalMultKeyGen"
        d.plan.destroy_keys(keys)
        # both rotation keys in one call, from the rotation indices
        a2 = np.concatenate([r.keys["rotP"][1], r.keys["rotM"][1]])
        e2 = np.concatenate([r.e["rotP"], r.e["rotM"]])
        got, _, keys = d.plan.keygen(d.s_ext, d.s, d.ctx.tower(a2), d.ctx.tower(e2), ns=r.ns, rotations=[1, -1])
        assert np.array_equal(got.to_host(), np.concatenate([r.keys["rotP"][0], r.keys["rotM"][0]])), "EvalRotateKeyGen({1, -1})"
        assert sorted(keys) == [-1, 1]
        d.plan.destroy_keys(keys)
        pk = fh.public_key(d.ctx, d.s, d.ctx.tower(r.g["pkA"]), d.ctx.tower(r.e_pk), r.ns)
        assert np.array_equal(pk.to_host()[0], r.g["pkB"]), "KeyGen's public key"
    finally:
        d.close()


def crt_centred(rows, qs):
    """the integer polynomial of smallest absolute value with the residues rows[i] modulo qs[i]"""
    Q = 1
    for q in qs:
        Q *= int(q)
    out = []
    for n in range(len(rows[0])):
        x = sum(int(rows[i][n]) * (Q // int(q)) * pow(Q // int(q), -1, int(q)) for i, q in enumerate(qs)) % Q
        out.append(x - Q if x > Q // 2 else x)
    return out


def switching_noise(r, o0, o1, c, k_new):
    """d = o0 + o1 * sNew - c * sOld over Q as a centred integer polynomial (sOld = s, sNew = sigma_kNew(s))"""
    rows = []
    for i in range(r.numQ):
        q = int(r.qs[i])
        v = (o0[i].astype(object) + mulmod(o1[i], r.perm(r.s[i], k_new), q) - mulmod(c[i], r.s[i], q)) % q
        rows.append(r.intt(v.astype(np.uint64), i))
    return crt_centred(rows, r.qs[:r.numQ])


@pytest.mark.parametrize("pre", SETS)
def test_seeded_keys_switch_with_the_noise_of_the_recorded_keys(backend, oracle, pre):
    o = oracle
    r = rec(o, pre)
    d = Setup(backend, r)
    rng = np.random.default_rng(len(pre))
    try:
        na, ne = d.plan.keygen_counters(2)
        b, a, keys = d.plan.keygen_blake2(d.s_ext, d.s, 2, KEY, 0, na, ns=r.ns, sigma=r.g["sigma100"] / 100.0, rotations=[1, -1])
        hy = o.orc_hybrid_create(r.N, r.numQ, r.g["q"], r.g["psiQ"], r.numP, r.g["p"], r.g["psiP"], r.dnum)
        for rot, name in ((1, "rotP"), (-1, "rotM")):
            c = np.stack([rng.integers(0, int(q), size=r.N, dtype=np.uint64) for q in r.qs[:r.numQ]])
            rb, ra, k_new, _ = r.keys[name]
            w0, w1 = np.empty_like(c), np.empty_like(c)
            o.orc_hybrid_key_switch(hy, c, r.numQ, np.ascontiguousarray(rb), np.ascontiguousarray(ra), w0, w1)
            ref = max(abs(v) for v in switching_noise(r, w0, w1, c, k_new))
            d.plan.key = keys[rot]
            o0, o1 = d.plan.KeySwitchCore(d.ctx.tower(c))
            dev = max(abs(v) for v in switching_noise(r, o0.to_host()[0], o1.to_host()[0], c, k_new))
            print(f"{pre}{name}: max|d| with the seeded key {dev} (2^{dev.bit_length()}), with the recorded key {ref} (2^{ref.bit_length()})")
            # the two keys carry errors of one distribution: a factor of 8 covers the draw-to-draw spread of a maximum over a few hundred
            # Gaussian sums; a wrong sign, factor or partition leaves d at the size of Q, dozens of bits above
            assert ref < int(r.qs[1]) >> 16, "the recorded key itself must switch with small noise"
            assert ref <= 8 * dev and dev <= 8 * ref, (pre, name, dev, ref)
            if r.ns != 1:  # BGV: the exact property
                o0, o1 = d.plan.KeySwitchCore(d.ctx.tower(c), t=r.ns)
                noise = switching_noise(r, o0.to_host()[0], o1.to_host()[0], c, k_new)
                assert all(v % r.ns == 0 for v in noise) and any(noise), "BGV: the switching noise is a multiple of t"
        d.plan.key = None
        d.plan.destroy_keys(keys)
        o.orc_hybrid_destroy(hy)
    finally:
        d.close()
