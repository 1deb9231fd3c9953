"""BGV level alignment of the automatic scaling modes against words recorded from the reference itself
(tests/golden/ref_vectors_bgv_auto.npz, written by tests/golden/make_golden_bgv_auto.py): ring 64, t = 65537, depth 4, HYBRID with 2 digits,
once under FLEXIBLEAUTO ("fa_") and once under FLEXIBLEAUTOEXT ("fx_").  Ciphertext pairs on every branch of
LeveledSHEBGVRNS::AdjustLevelsAndDepthInPlace / AdjustLevelsAndDepthToOneInPlace (bgvrns-leveledshe.cpp:83-233): the plan helper
reproduces every level, noise degree and scaling-factor integer, the executor every tower, word for word; the executor followed by
fhe_add / fhe_bgv_eval_mult reproduces cc->EvalAdd and cc->EvalMult of operands at different levels.  Ring 64 takes the step-by-step
path: this file pins the case table and the bookkeeping on the reference, test_parity_mod_reduce_multi.py pins the fused pass on the
oracle's loop.  `backend` = the lane emulator on the CPU, the product library with -m gpu."""
import os

import numpy as np
import pytest

from openfhe_amd import fhe_hip as fh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_vectors_bgv_auto.npz")
ALL_BRANCHES = {0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 12, 13, 14, 15, 16, 17, 20, 21, 22}


class Setup:
    def __init__(self, backend, prefix):
        z = np.load(GOLDEN)  # (a missing fixture is an error, not a skip)
        self.p = prefix
        self.g = g = {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}
        self.ring, self.t, self.dnum = (int(v) for v in z["meta"])
        self.ctx = fh.Context(backend, self.ring.bit_length() - 1, np.concatenate([g["q"], g["p"]]), np.concatenate([g["psiQ"], g["psiP"]]))
        self.mrf, self.big = [int(v) for v in g["mrf"]], [int(v) for v in g["big"]]

    def meta(self, j):
        return tuple(int(v) for v in self.g[f"pool{j}_meta"])

    def pair(self, j):
        w = self.g[f"pool{j}"]
        return self.ctx.tower(w[0][None]), self.ctx.tower(w[1][None])

    def plan(self, a, b, to_one):
        return fh.bgv_adjust_plan(self.meta(a), self.meta(b), self.t, self.mrf, self.big, to_one)

    def close(self):
        self.ctx.close()


def same(pair, want):
    return pair[0].n_limbs == want.shape[1] and np.array_equal(pair[0].to_host()[0], want[0]) and np.array_equal(pair[1].to_host()[0], want[1])


def meta_of(op):
    return (op.level, op.noise_scale_deg, op.n_out, op.scaling_factor_int)


@pytest.mark.parametrize("prefix", ["fa_", "fx_"])
def test_the_record_covers_the_case_table(prefix):
    z = np.load(GOLDEN)
    ring, t, dnum = (int(v) for v in z["meta"])
    assert (ring, t, dnum) == (64, 65537, 2)
    cases = z[prefix + "cases"]
    assert {int(c[2]) for c in cases} == ALL_BRANCHES
    seen = set()
    for a, b, _ in cases:
        (l1, d1, _, _), (l2, d2, _, _) = z[f"{prefix}pool{a}_meta"], z[f"{prefix}pool{b}_meta"]
        if l1 != l2:
            seen.add((int(d1 if l1 < l2 else d2), int(d2 if l1 < l2 else d1), abs(int(l1) - int(l2))))
    assert seen == {(dl, dh, gap) for dl in (1, 2) for dh in (1, 2) for gap in (1, 2, 3)}
    assert os.path.getsize(GOLDEN) < 512 * 1024


@pytest.mark.parametrize("prefix", ["fa_", "fx_"])
def test_plan_and_executor_reproduce_every_case(backend, prefix):
    s = Setup(backend, prefix)
    for n, row in enumerate(s.g["cases"]):
        a, b, branch = (int(v) for v in row)
        for which, to_one in (("adj", False), ("one", True)):
            p1, p2 = s.plan(a, b, to_one)
            want = tuple(int(v) for v in s.g[f"c{n}_{which}_meta"])
            assert meta_of(p1) + meta_of(p2) == want, f"{prefix}c{n} ({which}, branch {branch}): level, degree, sizeQl, scaling factor"
            for o, (src, plan) in enumerate(((a, p1), (b, p2)), 1):
                rec = s.g.get(f"c{n}_{which}{o}")
                c0, c1 = s.pair(src)
                r0, r1 = fh.bgv_adjust(s.ctx, c0, c1, plan, s.t)
                if rec is None:  # the reference left this operand's words alone
                    assert plan.drop_rows == [] and plan.n_out == c0.n_limbs and (r0 is c0 or same((r0, r1), s.g[f"pool{src}"]))
                else:
                    assert same((r0, r1), rec), f"{prefix}c{n} ({which}, branch {branch}): operand {o}"
    s.close()


@pytest.mark.parametrize("prefix", ["fa_", "fx_"])
def test_the_branches_pick_the_expected_plans(backend, prefix):
    """the shape of the plan on each branch: which operand moves, whether a scalar, how many ModReduce steps and whether rows are discarded
    between or behind them"""
    s = Setup(backend, prefix)
    for a, b, branch in (tuple(int(v) for v in row) for row in s.g["cases"]):
        p1, p2 = s.plan(a, b, False)
        side, kind = divmod(branch, 10)
        if side == 2:
            assert [p1.scalar != 1, p2.scalar != 1] == [kind == 1, kind == 2] and not p1.drop_rows and not p2.drop_rows
            continue
        lo, hi = (p1, p2) if side == 0 else (p2, p1)
        assert hi.untouched() and lo.n_out == hi.size_ql
        top = lo.size_ql - 1
        steps, scalar, gap_between, gap_behind = {
            0: (1, True, False, False), 1: (1, True, False, True), 2: (1, False, False, False), 3: (2, True, False, False),
            4: (2, True, True, False), 5: (0, True, False, True), 6: (1, True, False, False), 7: (1, True, False, False)}[kind]
        assert len(lo.drop_rows) == steps and (lo.scalar != 1) == scalar, (branch, lo.drop_rows, lo.scalar)
        if kind == 7:
            assert lo.drop_rows[0] < top  # rows discarded in front of the only ModReduce
        elif steps:
            assert lo.drop_rows[0] == top
        if steps == 2:
            assert (lo.drop_rows[1] < lo.drop_rows[0] - 1) == gap_between
        if steps and kind != 7:
            assert (lo.n_out < lo.drop_rows[-1]) == gap_behind
    s.close()


@pytest.mark.parametrize("prefix", ["fa_", "fx_"])
def test_eval_add_and_eval_mult_of_operands_at_different_levels(backend, prefix):
    s = Setup(backend, prefix)
    g, t = s.g, s.t
    # cc->EvalAdd: AdjustLevelsAndDepthInPlace, then the sum
    a, b, *meta = (int(v) for v in g["add_meta"])
    p1, p2 = s.plan(a, b, False)
    assert meta_of(p1) == tuple(meta)
    x = fh.bgv_adjust(s.ctx, *s.pair(a), p1, t)
    y = fh.bgv_adjust(s.ctx, *s.pair(b), p2, t)
    assert same((x[0].Plus(y[0]), x[1].Plus(y[1])), g["add"]), "cc->EvalAdd"
    # cc->EvalMult: AdjustLevelsAndDepthToOneInPlace, the tensor product and the relinearisation
    a, b, level, degree, size_ql, scf = (int(v) for v in g["mul_meta"])
    p1, p2 = s.plan(a, b, True)
    assert (p1.level, p1.noise_scale_deg + p2.noise_scale_deg, p1.n_out, p1.scaling_factor_int * p2.scaling_factor_int % t) == \
        (level, degree, size_ql, scf)
    x = fh.bgv_adjust(s.ctx, *s.pair(a), p1, t)
    y = fh.bgv_adjust(s.ctx, *s.pair(b), p2, t)
    ks = fh.KeySwitchPlan(s.ctx, len(g["q"]), len(g["p"]), s.dnum)
    ks.upload_key(g["mulB"], g["mulA"])
    assert same(ks.EvalMult(x[0], x[1], y[0], y[1], t=t), g["mul"]), "cc->EvalMult"
    ks.close()
    s.close()
