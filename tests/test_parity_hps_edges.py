"""The fused HPS kernels (p_over_q_expand_kernel, scale_round_switch_kernel<true> and <false>) at rounding edges and small moduli.

Each of the three kernels chains two conversions with the middle basis in registers and takes integers from two double-precision
sums (`nu` of the ScaleAndRound and `nu` of the exact basis switch) that must round as the reference's do.  They are reached through
fhe_bfv_eval_mult_hps only, whose first step on every path but HPS's is an inverse NTT: the operands here are chosen as COEFFICIENT
polynomials of Python integers and transformed with the oracle, which fixes what each fused kernel reads:
  (a) p_over_q_expand_kernel            : b = floor(Q/2) + d; the value in R_l after the integer conversion is R_l/2 + small
  (b) scale_round_switch_kernel<true>   : a = floor(I/2) + d + I (floor(Q_l/2) + d'), I = Q/Q_l: both sums on their edge in one coefficient
  (c) scale_round_switch_kernel<false>  : a = (1, 0), b = round((2k+1) Q / (2t)) + d: the tail's ScaleAndRound sits on k + 1/2
  (d) the same kernel's exact switch    : t above 3 r_j, a = (floor(Q/3), 0), b = round((2k+1) Q R / (2 t a)) + d: round(t a b / Q) = R/2 + small
  (e), (f) the ScaleAndRound of (c) and of (b) on residues below 2^52 of 60-bit moduli: the sum then ends where a double's last place
      is 1 or 2, the only place where it matters WHEN the 0.5 is added (below 2^52 adding it first or last gives the same double but
      for a partial sum within 0.5 of a power of two, and above 2^54 it is lost either way)
(a)-(d) at 30-, 36-, 45- and 60-bit moduli and a chain that puts Q (36 bits) and R (35 bits) on either side of the reduction switch, with few
limbs, at the register bound of the fused kernels and just past it.  Expected words: hps_ref.Composer; every comparison is exact.
That the inputs sit on the edge is shown, not assumed: `share` = the part of the crafted coefficients on which the oracle's member
differs from exact rounding (Python integers), printed (-s) and asserted positive (the figures, and which cases notice which change
of the two sums, are recorded in profiles/r11_hps_edge_parity.md).  The member calls the Composer makes on these
towers are pinned against the reference build at the end (CPU only)."""
import functools

import numpy as np
import pytest

import hps_ref
import libs
from openfhe_amd import fhe_hip as fh
from test_parity_edges import centred, crt_lift, half_modulus_residues, native_inputs, note_share, product, roots
from test_parity_hps import NAMES, device_plan, to_eval

LOGN = 9  # (at N = 32 the crafted operands rarely exposed a changed order of the additions; the NTT is covered elsewhere)
N, BATCH = 1 << LOGN, 2
T34 = (1 << 34) - 41
MIXED = "36/35"  # Q = the smallest primes above 2^35, descending: the auxiliary basis drops to 35 bits
FUSED = ("p_over_q_expand_kernel", "scale_round_switch_kernel")
PINNED = ("orc_fast_expand_crt_basis_p_over_q", "orc_expand_crt_basis_ql_hat")


# ---- moduli ------------------------------------------------------------------------------------------------------------------------
def moduli(o, bits, numQ, tech):
    """(q, psiQ, r, psiR): the reference's chain of `bits`-bit primes (or the MIXED chain) and the auxiliary basis that follows it"""
    M = 2 << LOGN
    if bits == MIXED:
        q = [o.orc_first_prime(35, M)]
        while len(q) < numQ:
            q.append(o.orc_next_prime(q[-1], M))
        q = np.array(q[::-1], np.uint64)
        size_q, size_r = 36, 35
    else:
        q, _ = hps_ref.chain(o, LOGN, bits, numQ)
        size_q = size_r = bits
    r, cur = [], int(q[-1])
    for _ in range(numQ + 1 if tech == fh.HPS else numQ):
        cur = o.orc_previous_prime(cur, M)
        r.append(cur)
    r = np.array(r, np.uint64)
    assert all(int(v).bit_length() == size_q and int(v) % M == 1 and o.orc_is_prime(int(v)) for v in q), (bits, q)
    assert all(int(v).bit_length() == size_r and int(v) % M == 1 and o.orc_is_prime(int(v)) for v in r), (bits, r)
    assert len(set(int(v) for v in np.concatenate([q, r]))) == len(q) + len(r)
    return q, roots(o, LOGN, q), r, roots(o, LOGN, r)


# ---- the composition with every member call kept -----------------------------------------------------------------------------------
class _Tap:
    """the oracle with the calls of PINNED kept as (name, arguments); the last argument is the result"""

    def __init__(self, o, calls):
        self._o, self._calls = o, calls

    def __getattr__(self, name):
        f = getattr(self._o, name)
        if name not in PINNED:
            return f

        def call(*args):
            f(*args)
            self._calls.append((name,) + tuple(np.array(a) if isinstance(a, np.ndarray) else a for a in args))
        return call


class Tracer(hps_ref.Composer):
    """hps_ref.Composer that keeps the operands and the result of every conversion it calls, in call order"""

    def __init__(self, o, *args):
        self.calls = []
        super().__init__(_Tap(o, self.calls), *args)

    def switch_exact(self, x, S, D):
        out = super().switch_exact(x, S, D)
        self.calls.append(("switch", np.array(x), np.array(S), np.array(D), out.copy()))
        return out

    def scale_round(self, x, I, O, t, output_first):
        out = super().scale_round(x, I, O, t, output_first)
        self.calls.append(("scale", np.array(x), np.array(I), np.array(O), int(t), bool(output_first), out.copy()))
        return out

    def of(self, name):
        return [c for c in self.calls if c[0] == name]


def off_switch(call):
    """[N] bool: where the oracle's SwitchCRTBasis differs from the centred lift"""
    _, x, S, D, out = call
    return (out != centred(crt_lift(x, S), product(S), D)).any(axis=0)


def off_scale(call):
    """[N] bool: where the oracle's ScaleAndRound differs from round(t X / I)"""
    _, x, I, O, t, first, out = call
    X, Ip = crt_lift(x, np.concatenate([O, I] if first else [I, O])), product(I)
    exact = np.stack([(((2 * t * X + Ip) // (2 * Ip)) % int(oj)).astype(np.uint64) for oj in O])
    return (out != exact).any(axis=0)


def off_half(call):
    """[N] bool: where the ScaleAndRound sum taken with the 0.5 first (the reference's order) and with the 0.5 last floor differently;
    numpy's float64 products and sums round once each, as the reference's do"""
    _, x, I, O, t, first, _ = call
    frac = hps_ref.sr_tables(I, O, t)[1]
    a, b = np.full(x.shape[1], 0.5), np.zeros(x.shape[1])
    for f, xi in zip(frac, x[len(O):] if first else x[:len(I)]):
        a, b = a + f * xi.astype(np.float64), b + f * xi.astype(np.float64)
    return np.floor(a) != np.floor(b + 0.5)


def off_expand(call):
    """[N] bool: where the second (exact) conversion of FastExpandCRTBasisPloverQ differs from the centred lift of what the first gave"""
    Rl, Ql, out = call[9], call[16], call[-1]
    L = len(Ql)
    return (out[:L] != centred(crt_lift(out[L:], Rl), product(Rl), Ql)).any(axis=0)


# ---- crafted operands --------------------------------------------------------------------------------------------------------------
def residues(X, mods):
    """[B][N] Python integers -> [B][len(mods)][N] residues"""
    return np.stack([np.stack([(Xb % int(m)).astype(np.uint64) for m in mods]) for Xb in X])


def head_operand(rng, q, L):
    """(b): X = floor(I/2) + d + I (floor(Q_l/2) + d'), |d|, |d'| <= 3"""
    I, Ql = product(q[L:]), product(q[:L])
    X = np.empty((BATCH, N), dtype=object)
    for b in range(BATCH):
        X[b] = [I // 2 + int(d) + I * (Ql // 2 + int(e)) for d, e in zip(rng.integers(-3, 4, size=N), rng.integers(-3, 4, size=N))]
    assert all(0 <= v < I * Ql for v in X.ravel())
    return residues(X, q)


def tail_operand(rng, q, r, t):
    """(d): B = round((2k+1) Q R / (2 t A)) + d for A = floor(Q/3), k in {0, 1}; d as in half_modulus_residues"""
    Q, R = product(q), product(r)
    A = Q // 3
    X = np.empty((BATCH, N), dtype=object)
    for b in range(BATCH):
        d = rng.permutation(np.concatenate([rng.integers(-3, 4, size=N // 2), rng.integers(-(1 << 20) + 1, 1 << 20, size=N - N // 2)]))
        X[b] = [((2 * int(k) + 1) * Q * R + t * A) // (2 * t * A) + int(v) for k, v in zip(rng.integers(0, 2, size=N), d)]
    # (the products stay inside (-QR/2, QR/2) and the operand inside (0, Q/2): nothing wraps before the tail)
    assert all(0 < v < Q // 2 and 2 * A * v < Q * R for v in X.ravel())
    return residues(X, q)


def small_residues(rng, q, lo, hi):
    """(e), (f): residues below 2^52 in the limbs lo .. hi - 1 (the ScaleAndRound's input basis), uniform in the others"""
    x = libs.rand_tower(rng, q, N, BATCH)
    x[:, lo:hi] = rng.integers(0, 1 << 52, size=(BATCH, hi - lo, N), dtype=np.uint64)
    assert all(int(v) > 1 << 52 for v in q[lo:hi])
    return x


def constant(q, value):
    """the EVALUATION form of the constant polynomial `value`: its residue in every slot"""
    return np.stack([np.stack([np.full(N, value % int(m), np.uint64) for m in q])] * BATCH)


@functools.lru_cache(maxsize=None)
def crafted(kind, tech, bits, numQ, L, t, keep_calls=False):
    """operands (EVALUATION), expected product and edge shares of one case, computed once (shared by backends and outEval variants)"""
    o = libs.load_oracle()
    q, psiQ, r, psiR = moduli(o, bits, numQ, tech)
    rng = np.random.default_rng([ord(kind), tech, numQ, L, t % 1000003, 0 if bits == MIXED else bits])
    comp = Tracer(o, N, q, psiQ, r, psiR, t, tech)
    qidx = np.arange(numQ, dtype=np.uint32)
    ev = lambda x: np.stack([comp.ntt(xb, qidx, False) for xb in x])
    uniform = lambda: libs.rand_tower(rng, q, N, BATCH)
    if kind == "a":
        ops = [uniform(), uniform(), ev(half_modulus_residues(rng, q, N, BATCH)[0]), ev(half_modulus_residues(rng, q, N, BATCH)[0])]
    elif kind == "b":
        ops = [ev(head_operand(rng, q, L)), ev(head_operand(rng, q, L)), uniform(), uniform()]
    elif kind == "c":
        ops = [constant(q, 1), constant(q, 0), ev(native_inputs(rng, q, t, N, BATCH)[0]), ev(native_inputs(rng, q, t, N, BATCH)[0])]
    elif kind == "e":
        ops = [constant(q, 1), constant(q, 0), ev(small_residues(rng, q, 0, numQ)), ev(small_residues(rng, q, 0, numQ))]
    elif kind == "f":
        ops = [ev(small_residues(rng, q, L, numQ)), ev(small_residues(rng, q, L, numQ)), uniform(), uniform()]
    else:
        ops = [constant(q, product(q) // 3), constant(q, 0), ev(tail_operand(rng, q, r, t)), ev(tail_operand(rng, q, r, t))]
    D, off, calls = [], {}, []
    for b in range(BATCH):
        comp.calls.clear()
        D.append(comp.eval_mult(np.stack([ops[0][b], ops[1][b]]), np.stack([ops[2][b], ops[3][b]]), L))
        # the calls that read crafted coefficients, by their place in Composer.eval_mult
        if kind == "a":
            picked = {"exact switch R_l -> Q_l": [off_expand(c) for c in comp.of(PINNED[0])]}
        elif kind == "b":
            picked = {"ScaleAndRound Q -> Q_l": [off_scale(c) for c in comp.of("scale")[:2]],
                      "exact switch Q_l -> R_l": [off_switch(c) for c in comp.of("switch")[:2]]}
        elif kind == "c":  # (the third product is a1 b1 = 0)
            picked = {"ScaleAndRound QR -> R": [off_scale(c) for c in comp.of("scale")[:2]]}
        elif kind in ("e", "f"):
            picked = {"place of the 0.5 in the ScaleAndRound sum": [off_half(c) for c in comp.of("scale")[:2]]}
        else:  # (four expansions come first)
            picked = {"exact switch R -> Q": [off_switch(c) for c in comp.of("switch")[4:6]]}
        for k, v in picked.items():
            assert len(v) == 2
            off.setdefault(k, []).extend(v)
        if keep_calls:
            calls += comp.calls
    comp.close()
    D = np.stack(D)
    for a in ops + [D, q, psiQ, r, psiR]:
        a.setflags(write=False)
    shares = {k: float(np.mean(np.concatenate(v))) for k, v in off.items()}
    return q, psiQ, r, psiR, ops, D, shares, calls


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
P, LV, H = fh.HPSPOVERQ, fh.HPSPOVERQLEVELED, fh.HPS
# (kind, technique, bits, numQ, sizeQl, t); per kind and size of the moduli: few limbs, the register bound, just past it.
CASES = [
    # (a) p_over_q_expand_kernel: fused while numQ <= 16; at 17 limbs the two separate conversions.  (Below the top level the value in
    # R_l is always above R_l/2, and whether the reference's sum lands on k + 1 or an ulp under it depends on the basis: the levels
    # taken here are ones where, with the oracle alone, it lands under it on a clear share of the coefficients.)
    ("a", P, 30, 3, 3, 2), ("a", LV, 36, 4, 4, 65537), ("a", LV, 45, 6, 3, 786433), ("a", P, 60, 6, 6, 1 << 20),
    ("a", LV, 30, 16, 16, 65537), ("a", P, 36, 16, 16, T34), ("a", P, 45, 16, 16, 2), ("a", LV, 60, 16, 8, 786433),
    ("a", P, 30, 17, 17, 1 << 20), ("a", LV, 36, 17, 17, 2), ("a", LV, 45, 17, 16, 65537), ("a", P, 60, 17, 17, T34),
    ("a", LV, MIXED, 4, 4, 65537), ("a", LV, MIXED, 5, 3, 786433),
    # (b) scale_round_switch_kernel<true>: L = numQ / 2 with few limbs, 8 at and past the bound (numQ = 17 still fuses the head: it holds
    # Q_l and Q / Q_l, 8 and 9 limbs, while the expansion of b goes to the separate launches); 19 -> 17 limbs: every stage separate
    ("b", LV, 30, 4, 2, 65537), ("b", LV, 36, 6, 3, 2), ("b", LV, 45, 5, 2, 1 << 20), ("b", LV, 60, 5, 2, 786433),
    ("b", LV, 30, 16, 8, 786433), ("b", LV, 36, 16, 8, 65537), ("b", LV, 45, 16, 8, T34), ("b", LV, 60, 16, 8, 2),
    ("b", LV, 30, 17, 8, 2), ("b", LV, 36, 17, 8, 1 << 20), ("b", LV, 45, 17, 8, 65537), ("b", LV, 60, 17, 8, 786433),
    ("b", LV, 45, 19, 17, 65537), ("b", LV, MIXED, 4, 2, 65537),
    # (c) scale_round_switch_kernel<false>, its ScaleAndRound: R has numQ + 1 limbs, fused up to numQ = 15
    ("c", H, 30, 3, 3, 65537), ("c", H, 36, 4, 4, 786433), ("c", H, 45, 5, 5, 2), ("c", H, 60, 6, 6, T34),
    ("c", H, 30, 15, 15, 1 << 20), ("c", H, 36, 15, 15, 2), ("c", H, 45, 15, 15, 65537), ("c", H, 60, 15, 15, 786433),
    ("c", H, 30, 16, 16, 786433), ("c", H, 36, 16, 16, 65537), ("c", H, 45, 16, 16, 1 << 20), ("c", H, 60, 16, 16, 2),
    ("c", H, MIXED, 4, 4, 65537),
    # (d) the same kernel's exact switch: reachable when t > 3 r_j
    ("d", H, 30, 3, 3, T34), ("d", H, 30, 15, 15, T34), ("d", H, 30, 16, 16, T34),
    # (e), (f) small residues of 60-bit moduli through the tail and through the head
    ("e", H, 60, 4, 4, 65537), ("e", H, 60, 15, 15, 2), ("e", H, 60, 16, 16, 786433),
    ("f", LV, 60, 5, 2, 65537), ("f", LV, 60, 16, 8, T34), ("f", LV, 60, 19, 17, 2),
]
# one (bits, numQ, L, t) per fused chain at 30, 45 and 60 bits, the mixed chain and (d), for the pinning against the reference build
PIN_CASES = [c for c in CASES if c[3] <= 6 and c[2] in (30, 45, 60, MIXED)] + [("b", LV, 60, 16, 8, 2), ("d", H, 30, 15, 15, T34)]


def case_id(c):
    kind, tech, bits, numQ, L, t = c
    return f"{kind}-{NAMES[tech]}-{str(bits).replace('/', '_')}bit-Q{numQ}-l{L}-t{t}"


def device_cases():
    out = []
    for c in CASES:
        for out_eval in ((False, True) if c[3] <= 6 else (False,)):  # (both output formats with few limbs only)
            out.append(pytest.param(c, out_eval, id=case_id(c) + ("-eval" if out_eval else "")))
    return out


def fused_launches(tech, numQ, L):
    """launches of FUSED that one composite call makes (the bookkeeping of test_parity_hps.test_composition)"""
    Lr = numQ + 1 if tech == fh.HPS else L
    regs = L <= 16 and Lr <= 16
    if tech == fh.HPS:
        return [0, 3 if regs else 0]
    return [2 if (regs and numQ <= 16) else 0, 2 if (L < numQ and regs and numQ - L <= 16) else 0]


def test_the_cases_reach_every_fused_kernel_on_both_sides_of_the_bound():
    for kind, slot in (("a", 0), ("b", 1), ("c", 1), ("d", 1), ("e", 1), ("f", 1)):
        for bits in {"d": (30,), "e": (60,), "f": (60,)}.get(kind, (30, 36, 45, 60)):
            mine = [fused_launches(tech, numQ, L) for k, tech, b, numQ, L, t in CASES if k == kind and b == bits]
            assert any(u[slot] > 0 for u in mine), (kind, bits)
            assert any(u[slot] == 0 or (kind == "b" and u[0] == 0) for u in mine), (kind, bits)
    assert {c[5] for c in CASES} == {2, 65537, 786433, 1 << 20, T34}
    # (b) with 17 limbs keeps its head fused; the case with 19 -> 17 limbs is the one without
    assert fused_launches(LV, 17, 8) == [0, 2] and fused_launches(LV, 19, 17) == [0, 0]


@pytest.mark.parametrize("case,out_eval", device_cases())
def test_crafted_operands(backend, oracle, case, out_eval):
    """fhe_bfv_eval_mult_hps on the crafted towers of one case against the Composer's words; the crafted coefficients sit on the
    edge (share > 0), the auxiliary basis is the library's own choice, and the fused kernels ran exactly where the case says"""
    kind, tech, bits, numQ, L, t = case
    q, psiQ, r, psiR, ops, D, shares, _ = crafted(*case)
    for stage, share in shares.items():
        note_share(f"{case_id(case)} {stage}", share)
        assert share > 0, f"{stage}: the crafted coefficients do not sit on the rounding edge"
    rr, pp = backend.hps_r(LOGN, q, tech)
    assert np.array_equal(rr, r) and np.array_equal(pp, psiR), "the auxiliary basis is the one fhe_param_hps_r picks"
    ctx, plan = device_plan(backend, LOGN, q, psiQ, r, psiR, t, tech)
    before = [backend.launch_count(k) for k in FUSED]
    T = [ctx.tower(x, limb_idx=np.arange(numQ)) for x in ops]
    got = plan.EvalMultNoRelin(*T, size_ql=L, out_eval=out_eval)
    used = [backend.launch_count(k) - b for k, b in zip(FUSED, before)]
    assert used == fused_launches(tech, numQ, L), "which of the fused kernels ran"
    want = to_eval(oracle, N, q, psiQ, D) if out_eval else D
    for k in range(3):
        g = got[k].to_host()
        bad = np.count_nonzero((g != want[:, k]).any(axis=1))
        assert bad == 0, f"product element {k}: {bad} of {BATCH * N} coefficients differ"
    if kind in ("c", "d", "e"):
        assert not D[:, 2].any() and D[:, 0].any() and D[:, 1].any()
    plan.close()
    ctx.close()


# ---- the members the Composer calls on these towers, against the reference build (CPU) ---------------------------------------------
@pytest.mark.parametrize("case", PIN_CASES, ids=case_id)
def test_members_on_crafted_towers_against_live_reference(oracle, ref, case):
    """ScaleAndRound, SwitchCRTBasis, FastExpandCRTBasisPloverQ and ExpandCRTBasisQlHat of the reference on every operand the
    composition hands to the oracle's member of the same name, crafted coefficients included"""
    o, r = oracle, ref
    calls = crafted(*case, keep_calls=True)[-1]
    seen = set()
    for c in calls:
        seen.add(c[0])
        out = c[-1]
        want = np.zeros_like(out)
        if c[0] == "switch":
            _, x, S, D, _ = c
            hatInv, _, hatMod, alpha, inv, _ = libs.crt_tables(S, D)
            r.ref_switch_crt_basis(N, len(S), S, roots(o, LOGN, S), x, hatInv, np.ascontiguousarray(hatMod.T), alpha, len(D), D,
                                   roots(o, LOGN, D), inv, want)
        elif c[0] == "scale":
            _, x, I, O, t, first, _ = c
            tab, frac = hps_ref.sr_tables(I, O, t)
            mods = np.concatenate([O, I] if first else [I, O])
            r.ref_scale_and_round(N, len(I), len(O), 1 if first else 0, mods, roots(o, LOGN, mods), x, tab, frac, want)
        elif c[0] == PINNED[0]:
            _, x, nQ, _, q, m, _, qinvp, nR, Rl, _, hatInv2, _, hm2, alpha2, L, Ql, _, rInv, _ = c
            r.ref_fast_expand_crt_basis_p_over_q(N, nQ, q, roots(o, LOGN, q), x, m, qinvp, nR, Rl, roots(o, LOGN, Rl), hatInv2, hm2, alpha2,
                                                 L, Ql, roots(o, LOGN, Ql), rInv, want)
        else:
            _, y, L, _, q, hat, nQ, _ = c
            r.ref_expand_crt_basis_ql_hat(N, nQ, q, roots(o, LOGN, q), y, L, 0, hat, want)
        assert np.array_equal(out, want), f"{c[0]} (call {len(seen)})"
    kind, tech, _, numQ, L, _ = case
    assert {"scale"} <= seen and (tech != fh.HPS or "switch" in seen) and (tech == fh.HPS or PINNED[0] in seen)
    assert (PINNED[1] in seen) == (L < numQ)
