"""BGV on HYBRID keys against words recorded from the reference itself (tests/golden/ref_vectors_bgv.npz, written by
tests/golden/make_golden_bgv.py): ring 64, t = 65537, depth 3, FIXEDMANUAL, HYBRID with 2 digits.  cc->EvalMult, cc->ModReduce,
cc->EvalRotate and EvalFastRotationPrecompute / EvalFastRotation of fresh ciphertexts, and the rotation and the product one level down,
each replayed through the new entry points word for word.  Ring 64 pins the composition and the use of t, not the fused kernels (the
oracle tests of test_parity_bgv.py pin those).  `backend` = the lane emulator on the CPU, the product library with -m gpu."""
import os

import numpy as np
import pytest

from openfhe_amd import fhe_hip as fh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_vectors_bgv.npz")
META = ("ring", "t", "numQ", "numP", "dnum", "k", "sizeQlMul", "sizeQlReduced")


class Setup:
    def __init__(self, backend):
        z = np.load(GOLDEN)  # (a missing fixture is an error, not a skip)
        self.g = g = {k: z[k] for k in z.files}
        g.update(zip(META, (int(v) for v in g["meta"])))
        logN = g["ring"].bit_length() - 1
        self.ctx = fh.Context(backend, logN, np.concatenate([g["q"], g["p"]]), np.concatenate([g["psiQ"], g["psiP"]]))
        self.plan = fh.KeySwitchPlan(self.ctx, g["numQ"], g["numP"], g["dnum"])
        self.plan.upload_key(g["mulB"], g["mulA"])
        self.rot = self.plan.make_key(g["rotB"], g["rotA"])

    def pair(self, name):
        return self.ctx.tower(self.g[name][0][None]), self.ctx.tower(self.g[name][1][None])

    def tables(self, sizeQl):
        """negtInvModq and qlInvModq of the level (bgvrns-cryptoparameters.cpp: -t^-1 mod q_l, q_l^-1 mod q_i)"""
        q, t = [int(v) for v in self.g["q"][:sizeQl]], self.g["t"]
        return (-pow(t, -1, q[-1])) % q[-1], [pow(q[-1], -1, qi) for qi in q[:-1]]

    def close(self):
        self.plan.close()
        self.ctx.close()


def same(pair, want):
    return np.array_equal(pair[0].to_host()[0], want[0]) and np.array_equal(pair[1].to_host()[0], want[1])


def test_the_record_is_what_the_generator_checked():
    z = np.load(GOLDEN)
    g = dict(zip(META, (int(v) for v in z["meta"])))
    assert g["ring"] == 64 and g["t"] == 65537 and g["dnum"] == 2 and g["sizeQlMul"] == g["numQ"] and g["sizeQlReduced"] == g["numQ"] - 1
    assert z["m"].shape == (2, g["numQ"], 64) and z["r"].shape == (2, g["numQ"] - 1, 64)
    assert z["mulB"].shape == (2, g["numQ"] + g["numP"], 64)


def test_eval_mult_matches_the_reference(backend):
    s = Setup(backend)
    g, t = s.g, s.g["t"]
    a0, a1 = s.pair("a")
    b0, b1 = s.pair("b")
    assert same(s.plan.EvalMult(a0, a1, b0, b1, t=t), g["m"]), "cc->EvalMult"
    assert not same(s.plan.EvalMult(a0, a1, b0, b1), g["m"]), "the CKKS form (t = 0) cannot give the BGV words"
    # the same from its parts: tensor, then the accumulating key switch of the third element
    qs = [int(v) for v in g["q"]]
    h = [x.to_host()[0].astype(object) for x in (a0, a1, b0, b1)]
    mod = np.array(qs, dtype=object)[:, None]
    d0, d1, d2 = (h[0] * h[2]) % mod, (h[0] * h[3] + h[1] * h[2]) % mod, (h[1] * h[3]) % mod
    acc0, acc1 = s.ctx.tower(d0.astype(np.uint64)[None]), s.ctx.tower(d1.astype(np.uint64)[None])
    s.plan.KeySwitchCoreAcc(s.ctx.tower(d2.astype(np.uint64)[None]), acc0, acc1, t=t)
    assert same((acc0, acc1), g["m"]), "tensor + KeySwitchCore + add"
    k0, k1 = s.plan.KeySwitchCore(s.ctx.tower(d2.astype(np.uint64)[None]), t=t)
    for got, d, want in ((k0, d0, g["m"][0]), (k1, d1, g["m"][1])):
        assert np.array_equal((got.to_host()[0].astype(object) + d) % mod, want.astype(object)), "KeySwitchCore"
    s.close()


def test_mod_reduce_matches_the_reference(backend):
    s = Setup(backend)
    g, t = s.g, s.g["t"]
    m0, m1 = s.pair("m")
    negt_inv, ql_inv = s.tables(g["numQ"])
    assert same(fh.mod_reduce_pair(s.ctx, m0, m1, t, negt_inv, ql_inv), g["r"]), "cc->ModReduce (both elements in one call)"
    for j, m in enumerate((m0, m1)):
        assert np.array_equal(fh.mod_reduce_limbs(s.ctx, m, t, negt_inv, ql_inv).to_host()[0], g["r"][j]), f"ModReduce, element {j}"
        assert np.array_equal(fh.mod_reduce(s.ctx, m, t).to_host()[0], g["r"][j]), f"fhe_mod_reduce, element {j}"
    s.close()


@pytest.mark.parametrize("level", ["fresh", "reduced"])
def test_rotations_match_the_reference(backend, level):
    s = Setup(backend)
    g, t, k = s.g, s.g["t"], s.g["k"]
    c0, c1 = s.pair("a" if level == "fresh" else "r")
    want = g["rot" if level == "fresh" else "rotL"]
    assert c0.n_limbs == (g["numQ"] if level == "fresh" else g["sizeQlReduced"])
    assert same(s.plan.EvalAutomorphism(s.rot, c0, c1, k, t=t), want), "cc->EvalRotate"
    s.plan.EvalFastRotationPrecompute(c1)
    assert same(s.plan.EvalFastRotation(s.rot, c0, c1, k, t=t), want), "EvalFastRotationPrecompute + EvalFastRotation"
    assert not same(s.plan.EvalFastRotation(s.rot, c0, c1, k), want), "the CKKS form on the same digits gives other words"
    s.close()


def test_eval_mult_one_level_down_matches_the_reference(backend):
    s = Setup(backend)
    g, t = s.g, s.g["t"]
    r0, r1 = s.pair("r")
    assert same(s.plan.EvalMult(r0, r1, r0, r1, t=t), g["mL"]), "cc->EvalMult at sizeQl = numQ - 1"
    s.close()
