"""Rotations and leveled relinearisation of BFV ciphertexts on BV keys against words recorded from the reference itself
(tests/golden/ref_vectors_bv_rot.npz, written by tests/golden/make_golden_bv_rot.py): ring 64, t = 65537, depth 4 (3 limbs of 60 bits),
HPSPOVERQLEVELED + BV — the reference's default BFV configuration — digit sizes 0 and 20.  cc->EvalRotate and EvalFastRotationPrecompute /
EvalFastRotation of a fresh ciphertext (nothing dropped: the sizeQl == numQ case) and of one whose noiseScaleDeg makes the reference drop a
level for the key switch, and cc->EvalMult of operands whose degrees make both the product and its relinearisation drop a level.  The levels
are the ones the generator saw FindLevelsToDrop answer (meta).  `backend` = the lane emulator on the CPU, the product library with -m gpu."""
import os

import numpy as np
import pytest

from openfhe_amd import fhe_hip as fh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_vectors_bv_rot.npz")
CASES = ("bfv0", "bfv20")
META = ("ring", "t", "numQ", "r", "D0", "k0", "k1", "sizeQlRot", "degRotL", "sizeQlRotL", "degMul", "sizeQlMul", "sizeQlRelin")


def load(case):
    z = np.load(GOLDEN)  # (a missing fixture is an error, not a skip)
    g = {k[len(case) + 1:]: z[k] for k in z.files if k.startswith(case + "_")}
    g.update(zip(META, (int(v) for v in g["meta"])))
    return g


class Setup:
    def __init__(self, backend, case):
        self.g = g = load(case)
        numQ = g["numQ"]
        logN = g["ring"].bit_length() - 1
        r, psiR = backend.hps_r(logN, g["q"], fh.HPSPOVERQLEVELED)
        assert np.array_equal(r, g["r_q"]) and np.array_equal(psiR, g["r_psiQ"]), "the recorded auxiliary basis is the one fhe_param_hps_r picks"
        self.ctx = fh.Context(backend, logN, np.concatenate([g["q"], r]), np.concatenate([g["psiQ"], psiR]))
        self.plan = fh.Hps(self.ctx, np.arange(numQ), np.arange(numQ, 2 * numQ), g["t"], fh.HPSPOVERQLEVELED)
        self.keys = {}

    def key(self, name, j=""):
        """the recorded key <name>B<j> / <name>A<j>"""
        g = self.g
        if (name, j) not in self.keys:
            kb, ka = g[f"{name}B{j}"], g[f"{name}A{j}"]
            assert kb.shape[0] == g["D0"]
            self.keys[name, j] = fh.BvKey(self.ctx, g["numQ"], g["r"], kb, ka)
        return self.keys[name, j]

    def tower(self, x, fmt=fh.EVALUATION):
        return self.ctx.tower(x[None], limb_idx=np.arange(self.g["numQ"]), fmt=fmt)

    def close(self):
        for k in self.keys.values():
            k.close()
        self.plan.close()
        self.ctx.close()


def same(pair, want):
    return np.array_equal(pair[0].to_host()[0], want[0]) and np.array_equal(pair[1].to_host()[0], want[1])


@pytest.mark.parametrize("level", ["fresh", "dropped"])
@pytest.mark.parametrize("case", CASES)
def test_rotations_match_the_reference(backend, case, level):
    """fresh: sizeQl == numQ, where the composites skip ScaleAndRound and ExpandCRTBasisQlHat — the reference's words say they are the
    identity there; dropped: the key switch one level down"""
    s = Setup(backend, case)
    g = s.g
    tag, size_ql = ("", g["sizeQlRot"]) if level == "fresh" else ("L", g["sizeQlRotL"])
    assert (size_ql == g["numQ"]) == (level == "fresh")
    c0, c1 = s.tower(g["a"][0]), s.tower(g["a"][1])
    ws, _ = s.plan.FastRotationPrecompute(c1, g["r"], size_ql=size_ql)
    dig = g["dig" + tag]
    assert np.array_equal(s.ctx.download(ws, (dig.shape[0], 1, size_ql, g["ring"]))[:, 0], dig), "EvalFastRotationPrecompute's digits"
    for j in range(2):
        key, k, want = s.key("rot", j), g[f"k{j}"], g[f"rot{tag}{j}"]
        assert same(s.plan.FastRotation(key, c0, k, size_ql=size_ql), want), f"EvalFastRotation, automorphism index {k}"
        assert same(s.plan.Automorphism(key, c0, c1, k, size_ql=size_ql), want), f"EvalRotate, automorphism index {k}"
    if level == "dropped":  # the record tests a drop: the top level gives other words
        assert not same(s.plan.Automorphism(s.key("rot", 0), c0, c1, g["k0"]), g["rotL0"])
    s.close()


@pytest.mark.parametrize("case", CASES)
def test_eval_mult_at_dropped_levels_matches_the_reference(backend, case):
    s = Setup(backend, case)
    g = s.g
    numQ = g["numQ"]
    assert g["sizeQlMul"] < numQ and g["sizeQlRelin"] < numQ, "the record drops a level for the product and for its relinearisation"
    key = s.key("mul")
    T = [s.tower(x) for x in (g["a"][0], g["a"][1], g["b"][0], g["b"][1])]
    d = s.plan.EvalMultNoRelin(*T, size_ql=g["sizeQlMul"])
    for k in range(3):
        assert np.array_equal(d[k].to_host()[0], g["d"][k]), f"EvalMultNoRelin element {k}"
    assert same(s.plan.Relinearize(key, *d, size_ql=g["sizeQlRelin"]), g["m"]), "RelinearizeCore from the COEFFICIENT elements"
    e = [t.SwitchFormat() for t in d]
    assert same(s.plan.Relinearize(key, *e, size_ql=g["sizeQlRelin"]), g["m"]), "RelinearizeCore from EVALUATION elements"
    assert same(s.plan.EvalMult(key, *T, size_ql=g["sizeQlMul"], size_ql_relin=g["sizeQlRelin"]), g["m"]), "cc->EvalMult"
    # the composite that relinearises at numQ limbs cannot produce these words; if it ever does, the record is not testing a drop
    assert not same(s.plan.EvalMult(key, *T, size_ql=g["sizeQlMul"]), g["m"])
    s.close()
