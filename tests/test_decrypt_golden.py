"""Decryption against what the reference itself decrypts to (tests/golden/ref_vectors_decrypt.npz, written by
tests/golden/make_golden_decrypt.py), at ring 64: BFV under HPSPOVERQLEVELED on 60-bit moduli (the split branch of the decryption
ScaleAndRound), HPS on 45-bit moduli (the unsplit branch) and BEHZ, fresh ciphertexts and three-element products with the NativePoly of
PKEBFVRNS::Decrypt; CKKS FIXEDMANUAL with 3 limbs, fresh, rescaled to 2 limbs, a three-element product and a ciphertext at one limb with the
Poly of PKECKKSRNS::Decrypt reduced modulo every limb; two-party threshold BFV and CKKS with the partial decryptions of
MultipartyDecryptLead / Main and the result of MultipartyDecryptFusion.

  * the plan's derived tables are the recorded tables of CryptoParametersBFVRNS bit for bit, the doubles included;
  * fhe_bfv_decrypt returns the recorded NativePoly word for word, fhe_decrypt_core (COEFFICIENT) the recorded residues;
  * the reference exposes no flooding term, but (lead - c0 - s1 * c1) * ns^-1 (Main: s2 * c1 alone) must come out as ONE polynomial of
    centred integers, the same in every limb, with |e| <= 2^26: 64 standard deviations of MP_SD = 2^20 (rns-multiparty.cpp:99-101,
    160-162), a condition, not a measurement.  With a wrong sign or the wrong share the recovered words are uniform residues.  Fed with
    that term, fhe_decrypt_core reproduces the recorded partials word for word; their sum (fhe_add) through fhe_bfv_decrypt_b, or through
    fhe_ntt_inv for CKKS, is the recorded fusion result.

`backend` = the lane emulator on the CPU, the product library with -m gpu."""
import os

import numpy as np
import pytest

from openfhe_amd import fhe_hip as fh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_vectors_decrypt.npz")
META = ("ring", "numQ", "t", "technique", "ns")
BFV_CASES = [("hps_", "fresh"), ("hps_", "prod"), ("hpsu_", "fresh"), ("hpsu_", "prod"), ("behz_", "fresh")]
CKKS_CASES = ["fresh", "rescaled", "prod", "one"]
FLOOD_BOUND = 1 << 26  # 64 * MP_SD
_z = {}


def golden():
    if not _z:
        z = np.load(GOLDEN)  # (a missing fixture is an error, not a skip)
        _z.update({k: z[k] for k in z.files})
    return _z


def rec(pre):
    z = golden()
    g = {k[len(pre):]: v for k, v in z.items() if k.startswith(pre)}
    g.update(zip(META, (int(v) for v in g["meta"])))
    assert g["ring"] == 64 and g["ns"] == 1 and len(g["q"]) == g["numQ"]
    return g


def context(backend, g):
    return fh.Context(backend, g["ring"].bit_length() - 1, g["q"], g["psi"])


def obj(a):
    return np.asarray(a).astype(object)


def elements(ctx, g, case):
    """the recorded elements as EVALUATION Towers (COEFFICIENT ones transformed, as PKERNS::DecryptCore does to its copies)"""
    n_elem, size_ql, fmt = (int(v) for v in g[case + "_meta"])
    assert g[case + "_c"].shape == (n_elem, size_ql, g["ring"])
    out = [ctx.tower(e, fmt=fmt) for e in g[case + "_c"]]
    return [e.SwitchFormat() if fmt == fh.COEFFICIENT else e for e in out]


@pytest.mark.parametrize("pre", ["hps_", "hpsu_", "behz_", "tbfv_"])
def test_derived_tables_are_the_recorded_ones(backend, pre):
    g = rec(pre)
    ctx = context(backend, g)
    plan = fh.BfvDecrypt(ctx, g["t"], g["technique"])
    try:
        if pre == "tbfv_":  # (tables not recorded: the plan is used below)
            assert plan.table("tQHatInvModqDivqModt") is not None
            return
        names = ("tgamma", "tgammaQHatInvModq", "negInvqModtgamma") if pre == "behz_" else (
            "tQHatInvModqDivqModt", "tQHatInvModqBDivqModt", "tQHatInvModqDivqFrac", "tQHatInvModqBDivqFrac")
        held = 0
        for name in fh.BfvDecrypt.TABLES:
            got = plan.table(name)
            if name in names and name in g:
                held += 1
                assert got is not None and np.array_equal(got, g[name]), f"{pre}{name}"  # (doubles: their 64 bits)
            else:
                assert got is None, f"{pre}{name}: the reference holds no such table for this set"
        assert held == {"hps_": 4, "hpsu_": 2, "behz_": 3}[pre]
    finally:
        plan.close()
        ctx.close()


@pytest.mark.parametrize("pre,case", BFV_CASES)
def test_bfv_decrypt_returns_the_recorded_native_poly(backend, pre, case):
    g = rec(pre)
    ctx = context(backend, g)
    plan = fh.BfvDecrypt(ctx, g["t"], g["technique"])
    try:
        te, s = elements(ctx, g, case), ctx.tower(g["s"])
        assert len(te) == (3 if case == "prod" else 2)
        want = g[case + "_m"][None]
        assert np.array_equal(plan.Decrypt(te, s), want)
        # a batch of three: the recorded ciphertext between two that differ from it
        other = [ctx.tower(np.stack([np.roll(h, 1, axis=-1), h, np.roll(h, 5, axis=-1)])) for h in (e.to_host()[0] for e in te)]
        assert np.array_equal(plan.Decrypt(other, s)[1], want[0])
        # the tail alone on the device's b
        assert np.array_equal(plan.DecryptB(fh.decrypt_core(ctx, te, s)), want)
    finally:
        plan.close()
        ctx.close()


@pytest.mark.parametrize("case", CKKS_CASES)
def test_ckks_decrypt_core_returns_the_recorded_residues(backend, case):
    g = rec("ckks_")
    ctx = context(backend, g)
    try:
        te, s = elements(ctx, g, case), ctx.tower(g["s"])  # the full-level key: a lower level reads its first rows
        size_ql = te[0].n_limbs
        assert size_ql == {"fresh": 3, "rescaled": 2, "prod": 3, "one": 1}[case] and s.n_limbs == 3
        assert np.array_equal(fh.ckks_decrypt(ctx, te, s), g[case + "_b"][None])
    finally:
        ctx.close()


class Threshold:
    """one recorded two-party set with the recovered flooding terms, computed once on the CPU with python integers and the oracle"""

    def __init__(self, o, pre):
        self.g = g = rec(pre)
        self.N, self.qs = g["ring"], [int(q) for q in g["q"]]
        self.octx = o.orc_ctx_create(self.N, len(self.qs), g["q"], g["psi"])
        self.o = o
        c0, c1 = g["c"]
        # ns = 1: (lead - c0 - s1 * c1), (main - s2 * c1)
        self.e_lead = self.rows(lambda i, q: (obj(g["lead"][i]) - obj(c0[i]) - obj(g["s1"][i]) * obj(c1[i])) % q)
        self.e_main = self.rows(lambda i, q: (obj(g["main"][i]) - obj(g["s2"][i]) * obj(c1[i])) % q)

    def rows(self, f):
        return np.stack([f(i, q).astype(np.uint64) for i, q in enumerate(self.qs)])

    def centred(self, rows):
        x = np.ascontiguousarray(rows[None]).copy()
        self.o.orc_ntt_inv_tower(self.octx, x, None, len(self.qs), 1, 0)
        return [[int(v) - q if int(v) > q // 2 else int(v) for v in x[0, i]] for i, q in enumerate(self.qs)]


_thr = {}


def threshold(o, pre):
    if pre not in _thr:
        _thr[pre] = Threshold(o, pre)
    return _thr[pre]


@pytest.mark.parametrize("pre", ["tbfv_", "tckks_"])
@pytest.mark.parametrize("which", ["lead", "main"])
def test_recovered_flooding_term_is_one_bounded_polynomial(oracle, pre, which):
    th = threshold(oracle, pre)
    limbs = th.centred(th.e_lead if which == "lead" else th.e_main)
    assert all(row == limbs[0] for row in limbs[1:]), "the recovered term differs between the limbs: not one integer polynomial"
    assert max(abs(v) for v in limbs[0]) <= FLOOD_BOUND
    assert any(abs(v) > 1 << 10 for v in limbs[0]), "a flooding term of sigma = 2^20 is not this small"


@pytest.mark.parametrize("pre", ["tbfv_", "tckks_"])
def test_threshold_partials_and_fusion(backend, oracle, pre):
    th = threshold(oracle, pre)
    g = th.g
    ctx = context(backend, g)
    plan = fh.BfvDecrypt(ctx, g["t"], g["technique"]) if pre == "tbfv_" else None
    try:
        c0, c1 = (ctx.tower(e) for e in g["c"])
        lead = fh.decrypt_core(ctx, [c0, c1], ctx.tower(g["s1"]), noise=ctx.tower(th.e_lead), ns=g["ns"])
        main = fh.decrypt_core(ctx, [None, c1], ctx.tower(g["s2"]), noise=ctx.tower(th.e_main), ns=g["ns"], with_c0=False)
        assert np.array_equal(lead.to_host()[0], g["lead"]) and np.array_equal(main.to_host()[0], g["main"])
        b = lead.Plus(main)  # MultipartyDecryptFusion's sum (fhe_add)
        if plan:
            assert np.array_equal(plan.DecryptB(b)[0], g["fusion"])
        else:
            assert np.array_equal(b.SwitchFormat().to_host()[0], g["fusion"])
            # the joint secret decrypts the joint ciphertext to the same integers but for the two flooding terms
            joint = np.stack([((obj(g["s1"][i]) + obj(g["s2"][i])) % q).astype(np.uint64) for i, q in enumerate(th.qs)])
            flood = ctx.tower(th.e_lead).Plus(ctx.tower(th.e_main))
            assert np.array_equal(fh.ckks_decrypt(ctx, [c0, c1], ctx.tower(joint), noise=flood), g["fusion"][None])
    finally:
        if plan:
            plan.close()
        ctx.close()
