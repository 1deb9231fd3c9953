"""Parity at boundary moduli, worst-case operands and rounding edges.

The other parity files draw uniformly random residues of 45..60-bit moduli.  This file drives the same kernels with
  * moduli on both sides of the 36-bit switch between the quotient-estimate reduction and the ladder of conditional subtractions
    (fhe_ctx_create), down to the smallest prime the ring admits, alone and mixed with 60-bit limbs in one launch,
  * operands at the top of the lazy ranges: all q-1, all 0, alternating, a single q-1, "mix" (a quarter q-1, a quarter 0, the rest
    uniform), and for the transforms the inputs whose OUTPUT is all q-1,
  * the double-precision roundings (modulus switch, exact basis switch, ScaleAndRound) on inputs whose exact value sits within
    an ulp of k + 1/2, where the order of the floating-point operations decides the integer.
Every comparison is word for word against the oracle (which restates the reference's operation order) on the emulator and, with
-m gpu, on the device; the oracle itself is pinned on the same inputs against the reference build (the *_against_live_reference
tests at the end, CPU only)."""
import ctypes as C
import os
from fractions import Fraction

import numpy as np
import pytest

import libs
from openfhe_amd import fhe_hip as fh
from test_parity import conv_tables, is_emu

vp = C.c_void_p
u64p = C.POINTER(C.c_uint64)

# ---- moduli ------------------------------------------------------------------------------------------------------------------------
# "min" = the smallest prime = 1 mod 2N; 36 and 59 = the FIRST prime of that size, the others the LAST one
SIZES = ("min", 20, 31, 32, 33, 35, 36, 37, 59, 60)
# (logN, size) pairs for which no prime = 1 mod 2N of that size exists: none for logN 4..17 (at logN 16 and 17 the only 20-bit prime,
# 786433, is also the smallest prime of the ring: the set then has 9 distinct limbs)
LEFT_OUT_SIZES = []
# (first, scale, aux) bit sizes of the CKKS-shaped chains
CHAINS = [(36, 35, 36), (35, 30, 35), (37, 36, 37), (60, 59, 60), (30, 20, 30)]
# (logN, sizeQ, chain) left out: logN 14 has 2 primes of 20 bits = 1 mod 2N and the rescale shape needs sizeQ - 1 = 4 scale limbs
# (fhe_ctx_create rejects a chain that wrapped into repeats); every other ring used here has enough (8 at logN 12, 5 at logN 13)
LEFT_OUT_CHAINS = [(14, 5, (30, 20, 30))]


def prime(o, logN, size):
    """one prime = 1 mod 2N of the size asked for; its bit length is asserted (a search that wrapped must fail, not test another size)"""
    M = 2 << logN
    if size == "min":
        q = M + 1
        while not o.orc_is_prime(q):
            q += M
        return q
    if size in (36, 59):
        q = o.orc_first_prime(size - 1, M)  # the first prime above 2^(size-1)
    else:
        q = o.orc_last_prime(size, M)
    assert int(q).bit_length() == size and q % M == 1 and o.orc_is_prime(q), (logN, size, q)
    return q


def primes_of(o, logN, size, n, avoid=()):
    """n distinct primes of `size` bits = 1 mod 2N, descending from the last one (orc_previous_prime), each checked"""
    M = 2 << logN
    out, cur = [], o.orc_last_prime(size, M)
    while len(out) < n:
        assert int(cur).bit_length() == size and cur % M == 1 and o.orc_is_prime(cur), (logN, size, n, cur)
        if cur not in avoid:
            out.append(cur)
        cur = o.orc_previous_prime(cur, M)
    return out


def size_set(o, logN):
    """the ring's moduli of every size in SIZES, 60 bits first (duplicates dropped: `min` may be the 20-bit prime)"""
    qs = []
    for s in reversed(SIZES):
        if (logN, s) in LEFT_OUT_SIZES:
            continue
        v = prime(o, logN, s)
        if v not in qs:
            qs.append(v)
    return np.array(qs, np.uint64)


def roots(o, logN, qs):
    return np.array([o.orc_root_of_unity(2 << logN, int(v)) for v in qs], np.uint64)


def chain(o, logN, sizeQ, dnum, bits):
    """CKKS-shaped tower (first modulus, sizeQ - 1 scale moduli, the auxiliary basis PrecomputeCRTTables would pick) with every
    prime's size asserted"""
    first, scale, aux = bits
    assert (logN, sizeQ, bits) not in LEFT_OUT_CHAINS
    M = 2 << logN
    q = [o.orc_last_prime(first, M)] + primes_of(o, logN, scale, sizeQ - 1)
    assert int(q[0]).bit_length() == first and len(set(q)) == sizeQ
    q = np.array(q, np.uint64)
    psiQ = roots(o, logN, q)
    if dnum == 0:
        return q, psiQ, None, None
    p, psiP = np.zeros(64, np.uint64), np.zeros(64, np.uint64)
    sizeP = o.orc_hybrid_select_p(1 << logN, sizeQ, q, dnum, aux, p, psiP)
    p, psiP = p[:sizeP].copy(), psiP[:sizeP].copy()
    assert sizeP > 0 and all(int(v).bit_length() == aux and int(v) % M == 1 for v in p), (logN, bits, p)
    assert len(set(int(v) for v in np.concatenate([q, p]))) == sizeQ + sizeP
    return q, psiQ, p, psiP


# ---- operand patterns --------------------------------------------------------------------------------------------------------------
PATTERNS = ("max", "zero", "alt", "first", "last", "mix", "uniform")


def pattern(rng, name, qs, N):
    """one tower [len(qs)][N] of the named pattern"""
    out = np.zeros((len(qs), N), np.uint64)
    for i, q in enumerate(qs):
        top = np.uint64(int(q) - 1)
        if name == "max":
            out[i] = top
        elif name == "alt":
            out[i, 0::2] = top
        elif name == "first":
            out[i, 0] = top
        elif name == "last":
            out[i, N - 1] = top
        elif name in ("mix", "uniform"):
            out[i] = rng.integers(0, int(q), size=N, dtype=np.uint64)
            if name == "mix":
                sel = rng.permutation(N)
                out[i, sel[:N // 4]] = top
                out[i, sel[N // 4:N // 2]] = 0
        else:
            assert name == "zero"
    return out


def patterns(rng, names, qs, N):
    return np.stack([pattern(rng, n, qs, N) for n in names])


def limit_pair(rng, qs, N):
    """the two-tower batch of the composite tests: tower 0 all q-1, tower 1 `mix`"""
    return patterns(rng, ("max", "mix"), qs, N)


def below36(qs):
    return any(int(v).bit_length() < 36 for v in qs)


def counts(lib, names):
    return {n: lib.launch_count(n) for n in names}


def big_emu():
    return bool(os.environ.get("FHE_TEST_BIG_EMU"))


# ---- 1. NTT ------------------------------------------------------------------------------------------------------------------------
def ntt_rings(lib):
    """(logN, sizes or None = the whole set, patterns or None = all): the emulator takes rings of every kernel family and one limb each of
    2^16 and 2^17 (as test_parity.ntt_sizes does), the GPU every ring 2^4..2^17 with the whole set"""
    if is_emu(lib):
        return [(4, None, None), (7, None, None), (10, None, None), (11, None, None), (12, None, None), (13, None, None),
                (16, (35,), ("max",)), (17, (20,), ("mix",))]
    return [(n, None, None) for n in range(4, 18)]


def test_ntt_boundary_moduli_and_patterns(backend, oracle):
    """fhe_ntt_fwd / fhe_ntt_inv: one launch per ring over the limbs of every size (60 .. 20 bits and the ring's smallest prime) and a
    batch with one tower per pattern, plus the tower whose transform is all q-1; fhe_ntt_fwd_oop / fhe_ntt_inv_oop on the `top` and
    `mix` towers; a scattered limbIdx; ntt_pass_kernel, ntt_static_kernel and ntt_row8_kernel each run with limbs below 36 bits"""
    o = oracle
    rng = np.random.default_rng(801)
    ran = {"ntt_pass_kernel": 0, "ntt_static_kernel": 0, "ntt_row8_kernel": 0}
    for logN, sizes, names in ntt_rings(backend):
        N = 1 << logN
        whole = sizes is None
        q = size_set(o, logN) if whole else np.array([prime(o, logN, s) for s in sizes], np.uint64)
        names = PATTERNS if names is None else names
        L = len(q)
        assert below36(q)
        psi = roots(o, logN, q)
        ctx = fh.Context(backend, logN, q, psi)
        octx = o.orc_ctx_create(N, L, q, psi)
        top = pattern(rng, "max", q, N)[None]
        before = counts(backend, ran)
        for inverse in (False, True):
            orc, orc_back = (o.orc_ntt_inv_tower, o.orc_ntt_fwd_tower) if inverse else (o.orc_ntt_fwd_tower, o.orc_ntt_inv_tower)
            x = patterns(rng, names, q, N)
            if whole:  # the input whose transform is all q-1: the last stage ends at the top of its range
                pre = top.copy()
                orc_back(octx, pre, None, L, 1, 0)
                x = np.concatenate([x, pre])
            B = len(x)
            want = x.copy()
            orc(octx, want, None, L, B, 0)
            assert not whole or np.array_equal(want[-1], top[0]), "the oracle's transforms are inverse to each other"
            t = ctx.tower(x, fmt=fh.EVALUATION if inverse else fh.COEFFICIENT)
            t.SwitchFormat()
            got = t.to_host()
            for b in range(B):
                for l in range(L):
                    assert np.array_equal(got[b, l], want[b, l]), \
                        f"{'inverse' if inverse else 'forward'} logN={logN} q={q[l]} pattern={(names + ('top',))[b]}"
            if whole:  # out of place, and the way back, on the towers `top`, `uniform` and `mix`
                # (the emulator's two-pass ring takes the `top` tower only: the ring's time is what the CPU suite pays most for)
                pick = [-1] if is_emu(backend) and logN > 12 else [-1, -2, names.index("mix")]
                sub = np.ascontiguousarray(x[pick])
                tin, out = ctx.tower(sub, fmt=t.fmt), ctx.empty(len(pick), L)
                f = backend.L.fhe_ntt_inv_oop if inverse else backend.L.fhe_ntt_fwd_oop
                backend.check(f(ctx.h, tin.ptr, out.ptr, None, L, len(pick), None))
                assert np.array_equal(out.to_host(), want[pick]), f"out of place logN={logN} inverse={inverse}"
                assert np.array_equal(tin.to_host(), sub), "out-of-place transform must not touch its input"
                out.fmt = fh.COEFFICIENT if inverse else fh.EVALUATION
                out.SwitchFormat()
                assert np.array_equal(out.to_host(), sub), f"round trip logN={logN} inverse={inverse}"
        if whole:  # a tower over scattered limbs of the context, sizes mixed (60, 20, 36, 32 and 35 bits)
            sel = np.array([0, L - 2, 3, 6, 4], np.uint32)
            x = patterns(rng, ("max", "mix"), q[sel], N)
            for inverse in (False, True):
                want = x.copy()
                (o.orc_ntt_inv_tower if inverse else o.orc_ntt_fwd_tower)(octx, want, sel.ctypes.data, len(sel), 2, 0)
                t = ctx.tower(x, limb_idx=sel, fmt=fh.EVALUATION if inverse else fh.COEFFICIENT)
                t.SwitchFormat()
                assert np.array_equal(t.to_host(), want), f"scattered limbs logN={logN} inverse={inverse}"
        after = counts(backend, ran)
        for k in ran:
            ran[k] += after[k] - before[k]
        o.orc_ctx_destroy(octx)
        ctx.close()
    assert all(v > 0 for v in ran.values()), ran


# ---- 2. polynomial product ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logN", [12, 13, 16])
def test_poly_mul_boundary_moduli(backend, oracle, logN):
    """fhe_poly_mul over the limbs of every size in one launch, operands all q-1 (tower 0) and `mix` (tower 1); the fused row kernels
    of the two-pass rings run with limbs below 36 bits"""
    o = oracle
    if is_emu(backend) and logN > 13 and not big_emu():
        pytest.skip("emulator: 2^16 runs on the GPU (FHE_TEST_BIG_EMU=1 runs it here too)")
    rng = np.random.default_rng(802)
    N = 1 << logN
    q = size_set(o, logN)
    L, B = len(q), 2
    psi = roots(o, logN, q)
    ctx = fh.Context(backend, logN, q, psi)
    octx = o.orc_ctx_create(N, L, q, psi)
    a, b = limit_pair(rng, q, N), limit_pair(rng, q, N)
    wa, wb = a.copy(), b.copy()
    o.orc_ntt_fwd_tower(octx, wa, None, L, B, 0)
    o.orc_ntt_fwd_tower(octx, wb, None, L, B, 0)
    want = np.empty_like(a)
    for bb in range(B):
        for l in range(L):
            o.orc_vec_mul(want[bb, l], wa[bb, l], wb[bb, l], N, q[l])
    o.orc_ntt_inv_tower(octx, want, None, L, B, 0)
    # (x^N = -1: the square of the all-(q-1) polynomial is known in closed form, c_k = (2k + 2 - N) mod q)
    for l in range(L):
        closed = (2 * np.arange(N, dtype=object) + 2 - N) % int(q[l])
        assert np.array_equal(want[0, l].astype(object), closed), "oracle against the closed form"
    names = ("poly_mul_row_a_kernel", "poly_mul_row_b_kernel")
    before = counts(backend, names)
    ta, tb = ctx.tower(a, fmt=fh.COEFFICIENT), ctx.tower(b, fmt=fh.COEFFICIENT)
    got = ta.PolyMul(tb).to_host()
    for l in range(L):
        assert np.array_equal(got[:, l], want[:, l]), f"polynomial product logN={logN} q={q[l]}"
    assert np.array_equal(ta.to_host(), a) and np.array_equal(tb.to_host(), b), "operands must not change"
    if logN > 12:
        after = counts(backend, names)
        assert all(after[k] > before[k] for k in names), (before, after)
    o.orc_ctx_destroy(octx)
    ctx.close()


# ---- 3. HYBRID key switching -------------------------------------------------------------------------------------------------------
# (logN, sizeQ, dnum, sizeQl): the two small shapes of test_hybrid_keyswitch_and_eval_mult, one with more than 8 digits (the chunked
# ks_inner_product_kernel) and one with dnum = 1 on more than 32 limbs (chunked conversions); batch 2 = {all q-1, mix} everywhere
KS_SHAPES = [(10, 4, 2, 4), (12, 5, 3, 4), (8, 10, 10, 10), (7, 34, 1, 34)]


def chain_id(bits):
    return "chain" + "_".join(map(str, bits))


def ks_cases():
    return [pytest.param(*shape, bits, id="-".join(map(str, shape)) + "-" + chain_id(bits))
            for bits in CHAINS for shape in KS_SHAPES if (shape[0], shape[1], bits) not in LEFT_OUT_CHAINS]


def ks_setup(backend, o, logN, sizeQ, dnum, bits):
    N = 1 << logN
    q, psiQ, p, psiP = chain(o, logN, sizeQ, dnum, bits)
    hy = o.orc_hybrid_create(N, sizeQ, q, psiQ, len(p), p, psiP, dnum)
    allq = np.concatenate([q, p])
    ctx = fh.Context(backend, logN, allq, np.concatenate([psiQ, psiP]))
    plan = fh.KeySwitchPlan(ctx, sizeQ, len(p), dnum)
    return N, q, p, allq, hy, ctx, plan


@pytest.mark.parametrize("logN,sizeQ,dnum,sizeQl,bits", ks_cases())
def test_hybrid_keyswitch_boundary_chains(backend, oracle, logN, sizeQ, dnum, sizeQl, bits):
    """KeySwitchCore, its accumulating form, EvalMult, ApproxModDown (t = 0, 65537, 2) and fhe_ks_precompute + fhe_ks_fast_keyswitch on
    chains around the 36-bit switch; key half b all q-1, key half a `mix`; ciphertext towers all q-1 and `mix`"""
    o = oracle
    rng = np.random.default_rng(803)
    N, q, p, allq, hy, ctx, plan = ks_setup(backend, o, logN, sizeQ, dnum, bits)
    B = 2
    keyB = np.stack([pattern(rng, "max", allq, N) for _ in range(dnum)])
    keyA = np.stack([pattern(rng, "mix", allq, N) for _ in range(dnum)])
    plan.upload_key(keyB, keyA)
    ql = q[:sizeQl]
    a0, a1, b0, b1 = (limit_pair(rng, ql, N) for _ in range(4))
    names = ("ks_inner_product_kernel", "ks_inner_multi_kernel", "switch_basis_kernel")
    before = counts(backend, names)
    w0, w1 = np.empty_like(a0), np.empty_like(a0)
    for bb in range(B):
        o.orc_hybrid_key_switch(hy, a0[bb], sizeQl, keyB, keyA, w0[bb], w1[bb])
    g0, g1 = plan.KeySwitchCore(ctx.tower(a0))
    assert np.array_equal(g0.to_host(), w0) and np.array_equal(g1.to_host(), w1), "KeySwitchCore"
    after = counts(backend, names)
    assert after["switch_basis_kernel"] > before["switch_basis_kernel"]
    inner = "ks_inner_product_kernel" if dnum > 8 else "ks_inner_multi_kernel"
    assert after[inner] > before[inner] and below36(allq) == (bits[1] < 36)
    # hoisted form: the digits once, then the inner product + ApproxModDown
    ta0 = ctx.tower(a0)
    plan.EvalFastRotationPrecompute(ta0)
    ws, wsb = plan.workspace(sizeQl, B)
    h0, h1 = ta0.like(), ta0.like()
    backend.check(backend.L.fhe_ks_fast_keyswitch(plan.h, plan.key, ta0.ptr, sizeQl, B, h0.ptr, h1.ptr, ws, wsb, None))
    assert np.array_equal(h0.to_host(), w0) and np.array_equal(h1.to_host(), w1), "fhe_ks_precompute + fhe_ks_fast_keyswitch"
    acc0, acc1 = ctx.tower(a1), ctx.tower(b0)
    plan.KeySwitchCoreAcc(ctx.tower(a0), acc0, acc1)
    wa0, wa1 = np.empty_like(a0), np.empty_like(a0)
    for bb in range(B):
        for l in range(sizeQl):
            o.orc_vec_add(wa0[bb, l], a1[bb, l], w0[bb, l], N, ql[l])
            o.orc_vec_add(wa1[bb, l], b0[bb, l], w1[bb, l], N, ql[l])
    assert np.array_equal(acc0.to_host(), wa0) and np.array_equal(acc1.to_host(), wa1), "KeySwitchCore (accumulating)"
    c0, c1 = np.empty_like(a0), np.empty_like(a0)
    for bb in range(B):
        o.orc_ckks_eval_mult_relin(hy, a0[bb], a1[bb], b0[bb], b1[bb], sizeQl, keyB, keyA, c0[bb], c1[bb])
    r0, r1 = plan.EvalMult(ctx.tower(a0), ctx.tower(a1), ctx.tower(b0), ctx.tower(b1))
    assert np.array_equal(r0.to_host(), c0) and np.array_equal(r1.to_host(), c1), "EvalMult"
    x = limit_pair(rng, np.concatenate([ql, p]), N)
    wd = np.empty((B, sizeQl, N), np.uint64)
    for bb in range(B):
        o.orc_hybrid_approx_mod_down(hy, x[bb], sizeQl, wd[bb])
    assert np.array_equal(plan.ApproxModDown(ctx.tower(x), sizeQl).to_host(), wd), "ApproxModDown"
    for t in (65537, 2):
        for bb in range(B):
            o.orc_hybrid_approx_mod_down_t(hy, x[bb], sizeQl, t, wd[bb])
        assert np.array_equal(plan.ApproxModDown(ctx.tower(x), sizeQl, t=t).to_host(), wd), f"ApproxModDown (BGV, t={t})"
    plan.close()
    ctx.close()
    o.orc_hybrid_destroy(hy)


@pytest.mark.parametrize("logN,sizeQ,dnum,sizeQl,bits", [pytest.param(10, 4, 2, 3, b, id=chain_id(b)) for b in CHAINS])
def test_hoisted_rotations_boundary_chains(backend, oracle, logN, sizeQ, dnum, sizeQl, bits):
    """fhe_eval_fast_rotation, fhe_eval_fast_rotation_ext and fhe_ks_down (the several-key inner product) on the same chains"""
    o = oracle
    rng = np.random.default_rng(804)
    N, q, p, allq, hy, ctx, plan = ks_setup(backend, o, logN, sizeQ, dnum, bits)
    B, sizeP = 2, len(p)
    ql = q[:sizeQl]
    c0, c1 = limit_pair(rng, ql, N), limit_pair(rng, ql, N)
    t0, t1 = ctx.tower(c0), ctx.tower(c1)
    ks = [o.orc_find_automorphism_index_2n_complex(1, 2 * N), 2 * N - 1]
    keys = [(np.stack([pattern(rng, nb, allq, N) for _ in range(dnum)]), np.stack([pattern(rng, na, allq, N) for _ in range(dnum)]))
            for nb, na in (("max", "mix"), ("mix", "max"))]
    handles = [plan.make_key(kb, ka) for kb, ka in keys]
    before = backend.launch_count("ks_inner_multi_kernel")
    plan.EvalFastRotationPrecompute(t1)
    wacc0 = np.zeros((B, sizeQl + sizeP, N), np.uint64)
    wacc1 = np.zeros_like(wacc0)
    extq = np.concatenate([ql, p])
    acc = None
    for j, (k, hnd, (kb, ka)) in enumerate(zip(ks, handles, keys)):
        w0, w1 = np.empty_like(c0), np.empty_like(c0)
        for b in range(B):
            o.orc_eval_automorphism(hy, c0[b], c1[b], sizeQl, k, kb, ka, w0[b], w1[b])
        g0, g1 = plan.EvalFastRotation(hnd, t0, t1, k)
        assert np.array_equal(g0.to_host(), w0) and np.array_equal(g1.to_host(), w1), f"EvalFastRotation k={k}"
        e0, e1 = plan.EvalFastRotationExt(hnd, t0, t1, k, j == 0)
        x0, x1 = np.empty_like(wacc0), np.empty_like(wacc0)
        for b in range(B):
            o.orc_eval_fast_rotation_ext(hy, c0[b], c1[b], sizeQl, k, 1 if j == 0 else 0, kb, ka, x0[b], x1[b])
        assert np.array_equal(e0.to_host(), x0) and np.array_equal(e1.to_host(), x1), f"EvalFastRotationExt k={k}"
        for i, m in enumerate(extq):
            wacc0[:, i] = (wacc0[:, i] + x0[:, i]) % m
            wacc1[:, i] = (wacc1[:, i] + x1[:, i]) % m
        if acc is None:
            acc = (e0, e1)
        else:
            idx = plan.ext_limbs(sizeQl)
            for a, e in zip(acc, (e0, e1)):
                backend.check(backend.L.fhe_add(ctx.h, a.ptr, a.ptr, e.ptr, idx.ctypes.data_as(fh.u32p), len(idx), B, None))
    assert backend.launch_count("ks_inner_multi_kernel") > before
    d0, d1 = plan.KeySwitchDown(acc[0], acc[1], sizeQl)
    wd0, wd1 = np.empty((B, sizeQl, N), np.uint64), np.empty((B, sizeQl, N), np.uint64)
    for b in range(B):
        o.orc_hybrid_approx_mod_down(hy, wacc0[b], sizeQl, wd0[b])
        o.orc_hybrid_approx_mod_down(hy, wacc1[b], sizeQl, wd1[b])
    assert np.array_equal(d0.to_host(), wd0) and np.array_equal(d1.to_host(), wd1), "KeySwitchDown"
    for hnd in handles:
        backend.L.fhe_ks_key_destroy(hnd)
    plan.close()
    ctx.close()
    o.orc_hybrid_destroy(hy)


@pytest.mark.parametrize("bits", [(35, 30, 35), (36, 35, 36)], ids=chain_id)
def test_bsgs_transform_boundary_chains(backend, oracle, bits):
    """one small fhe_ckks_bsgs_transform (3 inner rotations, 2 outer steps, one diagonal absent) with keys, diagonals and ciphertexts
    all q-1 or `mix`"""
    from test_parity_lt import run_oracle
    o = oracle
    rng = np.random.default_rng(805)
    logN, sizeQ, dnum, sizeQl, B = 8, 4, 2, 3, 2
    N, q, p, allq, hy, ctx, plan = ks_setup(backend, o, logN, sizeQ, dnum, bits)
    extq = np.concatenate([q[:sizeQl], p])
    c0, c1 = limit_pair(rng, q[:sizeQl], N), limit_pair(rng, q[:sizeQl], N)
    handles = []

    def rot(index, nb, na):
        if index == 0:
            return None, None
        k = o.orc_find_automorphism_index_2n_complex(index, 2 * N)
        kb = np.stack([pattern(rng, nb, allq, N) for _ in range(dnum)])
        ka = np.stack([pattern(rng, na, allq, N) for _ in range(dnum)])
        handles.append(plan.make_key(kb, ka))
        return (k, kb, ka), (k, handles[-1])
    ins = [rot(0, "", ""), rot(1, "max", "mix"), rot(2, "mix", "max")]
    outs = [rot(0, "", ""), rot(3, "max", "max")]
    diag = [[None if (i, j) == (1, 2) else pattern(rng, "max" if (i + j) % 2 == 0 else "mix", extq, N) for j in range(3)] for i in range(2)]
    want = run_oracle(o, hy, c0, c1, sizeQl, [r[0] for r in ins], [r[0] for r in outs], diag)
    ddev = [[None if d is None else ctx.upload(d) for d in row] for row in diag]
    g0, g1 = plan.BsgsTransform(ctx.tower(c0), ctx.tower(c1), [r[1] for r in ins], [r[1] for r in outs], ddev)
    assert np.array_equal(g0.to_host(), want[0]) and np.array_equal(g1.to_host(), want[1])
    for hnd in handles:
        backend.L.fhe_ks_key_destroy(hnd)
    plan.close()
    ctx.close()
    o.orc_hybrid_destroy(hy)


# ---- 4. rescale and modulus reduction ----------------------------------------------------------------------------------------------
def rescale_cases():
    return [pytest.param(logN, bits, id=f"{logN}-{chain_id(bits)}") for logN in (8, 12, 13, 14) for bits in CHAINS
            if (logN, 5, bits) not in LEFT_OUT_CHAINS]


@pytest.mark.parametrize("logN,bits", rescale_cases())
def test_rescale_and_mod_reduce_boundary_chains(backend, oracle, logN, bits):
    """fhe_rescale, fhe_rescale_limbs (scattered limbs), fhe_rescale_limbs_pair and fhe_mod_reduce in both formats; towers all q-1
    and `mix`; 2^12 and 2^13 take the fused forms"""
    o = oracle
    if is_emu(backend) and logN > 13 and not big_emu():
        pytest.skip("emulator: 2^14 runs on the GPU (FHE_TEST_BIG_EMU=1 runs it here too)")
    rng = np.random.default_rng(806)
    N, sizeQ, B = 1 << logN, 5, 2
    q, psi, _, _ = chain(o, logN, sizeQ, 0, bits)
    ctx = fh.Context(backend, logN, q, psi)
    octx = o.orc_ctx_create(N, sizeQ, q, psi)
    for sizeQl in (sizeQ, 2):
        x = limit_pair(rng, q[:sizeQl], N)
        want = np.empty((B, sizeQl - 1, N), np.uint64)
        for bb in range(B):
            o.orc_drop_last_element_and_scale(octx, x[bb], sizeQl, want[bb])
        assert np.array_equal(fh.rescale(ctx, ctx.tower(x)).to_host(), want), f"fhe_rescale sizeQl={sizeQl}"
        for t, ev in ((65537, 1), (65537, 0), (2, 1)):
            for bb in range(B):
                o.orc_mod_reduce(octx, x[bb], sizeQl, t, ev, want[bb])
            got = fh.mod_reduce(ctx, ctx.tower(x, fmt=fh.EVALUATION if ev else fh.COEFFICIENT), t)
            assert np.array_equal(got.to_host(), want), f"fhe_mod_reduce sizeQl={sizeQl} t={t} ev={ev}"
    # a tower over scattered limbs with the caller's tables: the dropped limb is a scale limb, the first modulus sits in the middle
    limbs = [3, 0, 4, 2]
    qs = [int(q[i]) for i in limbs]
    sub = o.orc_ctx_create(N, len(limbs), np.array(qs, np.uint64), np.array([int(psi[i]) for i in limbs], np.uint64))
    x = limit_pair(rng, np.array(qs, np.uint64), N)
    want = np.empty((B, len(limbs) - 1, N), np.uint64)
    for bb in range(B):
        o.orc_drop_last_element_and_scale(sub, x[bb], len(limbs), want[bb])
    inv = [pow(qs[-1] % qi, -1, qi) for qi in qs[:-1]]
    neg = [(qi - v) % qi for v, qi in zip(inv, qs[:-1])]
    assert np.array_equal(fh.rescale_limbs(ctx, ctx.tower(x, limbs), neg, inv).to_host(), want), "fhe_rescale_limbs"
    x1, x0 = ctx.tower(x[1:2], limbs), ctx.tower(x[0:1], limbs)
    r0, r1 = fh.rescale_limbs_pair(ctx, x0, x1, neg, inv)
    assert np.array_equal(r0.to_host()[0], want[0]) and np.array_equal(r1.to_host()[0], want[1]), "fhe_rescale_limbs_pair"
    o.orc_ctx_destroy(sub)
    o.orc_ctx_destroy(octx)
    ctx.close()


# ---- 5. conversions ----------------------------------------------------------------------------------------------------------------
def basis(o, logN, sizes):
    """distinct primes of the listed sizes (repeats of a size descend from its last prime)"""
    out = []
    for s in sizes:
        out.append(primes_of(o, logN, s, 1, avoid=out)[0])
    return out


# (logN, source sizes, target sizes)
CONV_CASES = [
    (12, (30, 30, 30, 30), (60, 60, 60)),                       # small -> large
    (12, (60, 60, 60), (35, 33, 31, 20)),                       # large -> small
    (13, (60, 36, 35, 30), (59, 37, 32, 20, 60)),               # mixed, both sides of the 36-bit switch on either side
    (6, (35,) * 34, (60, 30)),                                  # more than 32 source limbs: chunked plan
    (5, (20, 20, 20), (36, 35)),
]


@pytest.mark.parametrize("logN,ssz,dsz", CONV_CASES, ids=lambda v: "-".join(map(str, v[:4])) if isinstance(v, tuple) else str(v))
def test_conversions_boundary_moduli(backend, oracle, logN, ssz, dsz):
    """fhe_approx_switch_basis, fhe_switch_basis_exact, fhe_mod_up (both formats), fhe_expand_crt_basis (both orders) and
    fhe_fast_expand_crt_basis_p_over_q between bases of small, large and mixed moduli; towers all q-1 and `mix`"""
    o = oracle
    rng = np.random.default_rng(807)
    N, B = 1 << logN, 2
    allq = np.array(basis(o, logN, ssz + dsz), np.uint64)
    nS, nD = len(ssz), len(dsz)
    src, dst = allq[:nS], allq[nS:]
    allpsi = roots(o, logN, allq)
    ctx = fh.Context(backend, logN, allq, allpsi)
    octx = o.orc_ctx_create(N, nS + nD, allq, allpsi)
    src_idx, dst_idx = np.arange(nS, dtype=np.uint32), np.arange(nS, nS + nD, dtype=np.uint32)
    hatInv, hatPre, hatMod, alpha, qInv, mu = libs.crt_tables(src, dst)
    hi2, hp2, hm2, mu2 = conv_tables(o, src, dst)  # (the oracle-side derivation gives the same tables)
    assert np.array_equal(hatInv, hi2) and np.array_equal(hatMod, hm2) and np.array_equal(mu, mu2)
    hm_pq = np.ascontiguousarray(hatMod.T)
    x = limit_pair(rng, src, N)
    conv = fh.Conv(ctx, src_idx, dst_idx)
    before = backend.launch_count("switch_basis_kernel")
    tin = ctx.tower(x, limb_idx=src_idx, fmt=fh.COEFFICIENT)
    want = np.empty((B, nD, N), np.uint64)
    for bb in range(B):
        o.orc_approx_switch_crt_basis(x[bb], nS, N, src, hatInv, hatPre, hatMod, nD, dst, mu, want[bb])
    assert np.array_equal(conv.run(tin).to_host(), want), "ApproxSwitchCRTBasis"
    for bb in range(B):
        o.orc_switch_crt_basis(x[bb], nS, N, src, hatInv, hatPre, hm_pq, alpha, nD, dst, mu, qInv, want[bb])
    assert np.array_equal(conv.run(tin, exact=True).to_host(), want), "SwitchCRTBasis"
    assert backend.launch_count("switch_basis_kernel") > before and below36(allq)
    wantu = np.empty((B, nS + nD, N), np.uint64)
    for fmt, inEval in ((fh.EVALUATION, 1), (fh.COEFFICIENT, 0)):
        for bb in range(B):
            o.orc_approx_mod_up(octx, nS, nD, x[bb], inEval, hatInv, hatPre, hatMod, mu, wantu[bb])
        got = conv.ApproxModUp(ctx.tower(x, limb_idx=src_idx, fmt=fmt))
        assert np.array_equal(got.to_host(), wantu), f"ApproxModUp inEval={inEval}"
    for inEval, resEval, rev in ((1, 1, 0), (0, 0, 1), (0, 1, 0)):
        for bb in range(B):
            o.orc_expand_crt_basis(octx, nS, nD, x[bb], inEval, hatInv, hatPre, hm_pq, alpha, mu, qInv, resEval, rev, wantu[bb])
        t = ctx.tower(x, limb_idx=src_idx, fmt=fh.EVALUATION if inEval else fh.COEFFICIENT)
        got = conv.ExpandCRTBasis(t, fh.EVALUATION if resEval else fh.COEFFICIENT, reverse=bool(rev))
        assert np.array_equal(got.to_host(), wantu), f"ExpandCRTBasis inEval={inEval} resEval={resEval} rev={rev}"
    conv.close()
    want_pq = fast_expand_want(o, x, src, dst, N)
    to_pl, to_ql = fast_expand_plans(ctx, src, dst)
    got = to_pl.FastExpandCRTBasisPloverQ(to_ql, tin)
    assert np.array_equal(got.to_host(), want_pq), "FastExpandCRTBasisPloverQ"
    to_pl.close(), to_ql.close()
    o.orc_ctx_destroy(octx)
    ctx.close()


def fast_expand_want(o, x, q, pl, N):
    nQ, nP = len(q), len(pl)
    m, mpre, qinvp = libs.p_over_q_tables(q, pl)
    hatInv2, hatPre2, hatMod2, alpha2, pInv, muQ = libs.crt_tables(pl, q)
    muP = libs.crt_tables(q, pl)[5]
    hm2_qp = np.ascontiguousarray(hatMod2.T)
    want = np.zeros((x.shape[0], nQ + nP, N), np.uint64)
    for b in range(x.shape[0]):
        o.orc_fast_expand_crt_basis_p_over_q(x[b], nQ, N, q, m, mpre, qinvp, nP, pl, muP, hatInv2, hatPre2, hm2_qp, alpha2, nQ, q,
                                             muQ, pInv, want[b])
    return want


def fast_expand_plans(ctx, q, pl):
    nQ, nP = len(q), len(pl)
    m, _, qinvp = libs.p_over_q_tables(q, pl)
    return (fh.Conv(ctx, np.arange(nQ), np.arange(nQ, nQ + nP), hat_inv=m, hat_mod=qinvp), fh.Conv(ctx, np.arange(nQ, nQ + nP), np.arange(nQ)))


@pytest.mark.parametrize("logN", [4, 12, 13])
def test_switch_modulus_boundary_moduli(backend, oracle, logN):
    """fhe_switch_modulus between the limbs of every size: from the 60-bit limb down to every other (20 bits and the ring's smallest
    prime included), from the 20-bit limb and from the smallest prime up, with the values around q/2, 0 and q-1 planted and the
    patterns in the batch"""
    o = oracle
    rng = np.random.default_rng(808)
    N = 1 << logN
    q = size_set(o, logN)
    L = len(q)
    names = ("max", "mix", "alt")
    ctx = fh.Context(backend, logN, q, roots(o, logN, q))
    pos20 = [int(v).bit_length() for v in q].index(20)
    for srcPos in (0, pos20, L - 1, 5):
        x = patterns(rng, names, q, N)
        qs = int(q[srcPos])
        edge = [qs // 2 - 1, qs // 2, qs // 2 + 1, 0, qs - 1]
        x[1, srcPos, :5] = edge
        x[1, srcPos, N - 5:] = edge
        tx, out = ctx.tower(x), ctx.empty(len(names), L)
        backend.check(backend.L.fhe_switch_modulus(ctx.h, out.ptr, None, L, tx.ptr, L, srcPos, srcPos, len(names), None))
        want = np.empty_like(x)
        for bb in range(len(names)):
            for l in range(L):
                want[bb, l] = x[bb, srcPos]
                o.orc_switch_modulus(want[bb, l], N, q[srcPos], q[l])
        got = out.to_host()
        for l in range(L):
            assert np.array_equal(got[:, l], want[:, l]), f"SwitchModulus logN={logN} {q[srcPos]} -> {q[l]}"
        # (python integers on the planted values: centred lift, dcrtpoly's SwitchModulus)
        for l in range(L):
            ql = int(q[l])
            lift = [(v if v <= qs // 2 else v - qs) % ql for v in edge]
            assert [int(v) for v in want[1, l, :5]] == lift, (qs, ql)
    ctx.close()


# ---- 6. element-wise at the arithmetic limit ---------------------------------------------------------------------------------------
def limit_moduli(o, logN):
    """the largest 60-bit prime, the smallest 36-bit prime, the largest 35-bit prime and the smallest prime of the ring"""
    return np.array([prime(o, logN, s) for s in (60, 36, 35, "min")], np.uint64)


def obj(a):
    return a.astype(object)


@pytest.mark.parametrize("logN", [5, 12, 13])
def test_elementwise_at_the_arithmetic_limit(backend, oracle, logN):
    """fhe_mul, fhe_mul_add, fhe_tensor, fhe_tensor_square, fhe_mul_const, fhe_mult_acc, fhe_add_const, fhe_sub_const with every operand
    q-1 (tower 0) or `mix` (tower 1), constants q-1 and constants >= q (reduced by the entry point), against python integers"""
    o = oracle
    rng = np.random.default_rng(809)
    N, B = 1 << logN, 2
    q = limit_moduli(o, logN)
    L = len(q)
    qo = np.array([int(v) for v in q], dtype=object)[None, :, None]
    ctx = fh.Context(backend, logN, q, roots(o, logN, q))
    a0, a1, b0, b1, acc = (limit_pair(rng, q, N) for _ in range(5))
    T = lambda h: ctx.tower(h)
    # (the oracle's product on the all-(q-1) rows: (q-1)^2 = 1 mod q)
    probe = np.empty(N, np.uint64)
    for l in range(L):
        o.orc_vec_mul(probe, a0[0, l], b0[0, l], N, q[l])
        assert (probe == 1).all()
    ta0, ta1, tb0, tb1 = T(a0), T(a1), T(b0), T(b1)
    assert np.array_equal(obj(ta0.Times(tb0).to_host()), obj(a0) * obj(b0) % qo), "fhe_mul"
    tacc = T(acc)
    backend.check(backend.L.fhe_mul_add(ctx.h, tacc.ptr, ta0.ptr, tb0.ptr, None, L, B, None))
    assert np.array_equal(obj(tacc.to_host()), (obj(acc) + obj(a0) * obj(b0)) % qo), "fhe_mul_add"
    d = [ctx.empty(B, L) for _ in range(3)]
    backend.check(backend.L.fhe_tensor(ctx.h, ta0.ptr, ta1.ptr, tb0.ptr, tb1.ptr, d[0].ptr, d[1].ptr, d[2].ptr, None, L, B, None))
    w = [obj(a0) * obj(b0) % qo, (obj(a0) * obj(b1) + obj(a1) * obj(b0)) % qo, obj(a1) * obj(b1) % qo]
    for e in range(3):
        assert np.array_equal(obj(d[e].to_host()), w[e]), f"fhe_tensor element {e}"
    assert (d[1].to_host()[0] == 2).all()
    backend.check(backend.L.fhe_tensor_square(ctx.h, ta0.ptr, ta1.ptr, d[0].ptr, d[1].ptr, d[2].ptr, None, L, B, None))
    w = [obj(a0) * obj(a0) % qo, 2 * obj(a0) * obj(a1) % qo, obj(a1) * obj(a1) % qo]
    for e in range(3):
        assert np.array_equal(obj(d[e].to_host()), w[e]), f"fhe_tensor_square element {e}"
    big = (1 << 64) - 1
    for consts in ([int(v) - 1 for v in q], [int(v) for v in q], [2 * int(v) - 1 if 2 * int(v) - 1 <= big else int(v) + 1 for v in q],
                   [big - i for i in range(L)]):
        k = np.array(consts, np.uint64)
        ko = np.array([c % int(v) for c, v in zip(consts, q)], dtype=object)[None, :, None]
        assert np.array_equal(obj(ta0.Times(k).to_host()), obj(a0) * ko % qo), f"fhe_mul_const {consts}"
        tacc = T(acc)
        tacc.MultAccEqNoCheck(ta1, k)
        assert np.array_equal(obj(tacc.to_host()), (obj(acc) + obj(a1) * ko) % qo), f"fhe_mult_acc {consts}"
        out = ta0.like()
        cp = k.ctypes.data_as(u64p)
        backend.check(backend.L.fhe_add_const(ctx.h, out.ptr, ta0.ptr, cp, None, L, B, 0, None))
        assert np.array_equal(obj(out.to_host()), (obj(a0) + ko) % qo), f"fhe_add_const {consts}"
        backend.check(backend.L.fhe_sub_const(ctx.h, out.ptr, ta0.ptr, cp, None, L, B, None))
        assert np.array_equal(obj(out.to_host()), (obj(a0) - ko) % qo), f"fhe_sub_const {consts}"
    ctx.close()


@pytest.mark.parametrize("logN,terms", [(5, 16), (12, 16), (12, 37), (6, 37)])
def test_lincomb_at_the_arithmetic_limit(backend, oracle, logN, terms):
    """fhe_lincomb with 16 and 37 terms, every operand and every constant q-1 (each term is (q-1)^2 = 1: the sum is `terms` mod q),
    then the same with a `mix` tower per term; also accumulating onto an all-(q-1) tower"""
    o = oracle
    rng = np.random.default_rng(810)
    N, B = 1 << logN, 2
    q = limit_moduli(o, logN)
    qs = [int(v) for v in q]
    qo = np.array(qs, dtype=object)[None, :, None]
    ctx = fh.Context(backend, logN, q, roots(o, logN, q))
    xs = [limit_pair(rng, q, N) for _ in range(terms)]
    ks = [[qi - 1 for qi in qs] for _ in range(terms)]
    tw = [ctx.tower(x) for x in xs]
    want = sum(obj(x) * np.array(k, dtype=object)[None, :, None] for x, k in zip(xs, ks)) % qo
    got = fh.lincomb(ctx, tw, ks).to_host()
    assert np.array_equal(obj(got), want)
    for l, qi in enumerate(qs):
        assert (got[0, l] == terms % qi).all()
    acc_h = limit_pair(rng, q, N)
    acc = fh.lincomb(ctx, tw, ks, accumulate_into=ctx.tower(acc_h))
    assert np.array_equal(obj(acc.to_host()), (want + obj(acc_h)) % qo)
    ctx.close()


@pytest.mark.parametrize("logN", [5, 12])
def test_inner_product_at_the_arithmetic_limit(backend, oracle, logN):
    """fhe_inner_product with 8 terms, digits and key rows all q-1 (tower 0: eight products (q-1)^2 in the 64-bit column sums) and
    `mix` (tower 1), against the oracle and python integers"""
    o = oracle
    rng = np.random.default_rng(811)
    N, B, nTerms = 1 << logN, 2, 8
    q = limit_moduli(o, logN)
    L = len(q)
    ctx = fh.Context(backend, logN, q, roots(o, logN, q))
    xs = [limit_pair(rng, q, N) for _ in range(nTerms)]
    k0 = [pattern(rng, "max", q, N) for _ in range(nTerms)]
    k1 = [pattern(rng, "mix", q, N) for _ in range(nTerms)]
    want0, want1 = np.empty((B, L, N), np.uint64), np.empty((B, L, N), np.uint64)
    for bb in range(B):
        for i in range(L):
            for keys, want in ((k0, want0), (k1, want1)):
                xp = (vp * nTerms)(*[x[bb, i].ctypes.data for x in xs])
                kp = (vp * nTerms)(*[k[i].ctypes.data for k in keys])
                o.orc_vec_inner_product(want[bb, i], xp, kp, nTerms, N, q[i])
    for i in range(L):
        assert (want0[0, i] == 8 % int(q[i])).all()
    tx = [ctx.tower(x) for x in xs]
    tk0, tk1 = [ctx.tower(k[None]) for k in k0], [ctx.tower(k[None]) for k in k1]
    out0, out1 = tx[0].like(), tx[0].like()
    px, p0, p1 = ((vp * nTerms)(*[t.ptr for t in ts]) for ts in (tx, tk0, tk1))
    backend.check(backend.L.fhe_inner_product(ctx.h, nTerms, px, p0, p1, None, None, L, B, out0.ptr, out1.ptr, None))
    assert np.array_equal(out0.to_host(), want0) and np.array_equal(out1.to_host(), want1)
    ctx.close()


# ---- rounding edges ----------------------------------------------------------------------------------------------------------------
# The oracle restates the reference's order of floating-point operations; the exact rational result only shows that the inputs sit on
# the edge: `share` = the part of the coefficients on which the oracle's integer differs from exact rounding (printed: run with -s;
# the figures measured on the CPU are recorded in profiles/r08_edge_parity.md).
def note_share(case, share):
    print(f"order-sensitivity share {case}: {share:.4f}")


def product(mods):
    out = 1
    for v in mods:
        out *= int(v)
    return out


def mod_switch_pairs(o):
    M = 1 << 13
    p = lambda bits: int(o.orc_last_prime(bits, M))
    pairs = [(p(60), p(30)), (p(60), p(59)), (p(59), p(60)), (p(54), 1 << 13), (p(27), 1 << 11), (1 << 59, 1 << 11), (1 << 32, p(30))]
    for (a, b), (ba, bb) in zip(pairs, ((60, 30), (60, 59), (59, 60), (54, 14), (27, 12), (60, 12), (33, 30))):
        assert a.bit_length() == ba and b.bit_length() == bb
    # two more with a ratio that is not 1/2 or 1 up to a few ulps (the last primes of neighbouring sizes give such ratios, and then
    # x * ratio + 0.5 rounds the same way fused or not): 2^59.5 against the last 60-bit prime, both directions
    g = int(o.orc_next_prime((int(2 ** 59.5) // M) * M + 1, M))
    assert g.bit_length() == 60 and g % M == 1 and o.orc_is_prime(g)
    return pairs + [(p(60), g), (g, p(60))]


def mod_switch_inputs(rng, qFrom, qTo, n=2048):
    """x = floor((2k + 1) qFrom / (2 qTo)) and x + 1 for random k: x qTo / qFrom straddles k + 1/2; (2^32, odd qTo): x = 2^31 * odd are exact
    ties.  x - 1 is taken too: where qTo divides qFrom the floor is itself an exact tie, and only the word below it sits under the edge
    (there the uint64 -> double conversion of a 59-bit x decides)"""
    ks = [int(v) for v in rng.integers(0, qTo, size=n // 2, dtype=np.uint64)]
    xs = []
    for k in ks:
        x = (2 * k + 1) * qFrom // (2 * qTo)
        xs += [max(x - 1, 0), min(x, qFrom - 1), min(x + 1, qFrom - 1)]
    if qFrom == 1 << 32:
        xs[:64] = [(1 << 31) * (2 * i + 1) for i in range(64)]
    x = np.array(xs, np.uint64)
    exact = np.array([((2 * v * qTo + qFrom) // (2 * qFrom)) % qTo for v in xs], np.uint64)
    return x, exact


def test_mod_switch_round_on_the_rounding_edge(backend, oracle):
    """fhe_mod_switch_round where x qTo / qFrom is within an ulp of k + 1/2"""
    o = oracle
    rng = np.random.default_rng(812)
    ctx = fh.Context(backend, 4, [97], [19])
    for qFrom, qTo in mod_switch_pairs(o):
        x, exact = mod_switch_inputs(rng, qFrom, qTo)
        n = len(x)
        want = np.zeros(n, np.uint64)
        o.orc_set_values_mod_switch(x, n, qFrom, qTo, want)
        share = float(np.mean(want != exact))
        note_share(f"mod_switch_round {qFrom.bit_length()}-bit {qFrom} -> {qTo}", share)
        if qFrom.bit_length() >= 54:
            assert share > 0, "the inputs do not sit on the rounding edge"
        dx, dout = ctx.upload(x), ctx.malloc(n * 8)
        backend.check(backend.L.fhe_mod_switch_round(ctx.h, dx, qFrom, qTo, dout, n, None))
        got = ctx.download(dout, (n,))
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{qFrom} -> {qTo}: {bad.size} words differ, first x={x[bad[0]]} got={got[bad[0]]} want={want[bad[0]]}"
    ctx.close()


# (logN, source limbs, size): the target basis has one limb more, of the same size (the shape of the BFV HPS extensions)
KNIFE_BASES = [(12, 3, 60), (10, 7, 60), (8, 12, 60), (12, 4, 36), (12, 3, 30)]


def knife_basis(o, logN, nS, size):
    allq = np.array(primes_of(o, logN, size, 2 * nS + 1), np.uint64)
    return allq, allq[:nS], allq[nS:]


def half_modulus_residues(rng, src, N, B):
    """the residues of X = floor(Q / 2) + d, d in [-3, 3] on half of the coefficients and |d| < 2^20 on the rest; returns (x, X)"""
    Q = product(src)
    X = np.empty((B, N), dtype=object)
    for b in range(B):
        d = np.concatenate([rng.integers(-3, 4, size=N // 2), rng.integers(-(1 << 20) + 1, 1 << 20, size=N - N // 2)])
        X[b] = [Q // 2 + int(v) for v in rng.permutation(d)]
    x = np.stack([np.stack([(X[b] % int(s)).astype(np.uint64) for s in src]) for b in range(B)])
    return x, X


def centred(X, Q, mods):
    """[len(mods)][...]: the residues of X lifted to (-Q/2, Q/2)"""
    Xc = np.where(2 * X < Q, X, X - Q)
    return np.stack([(Xc % int(m)).astype(np.uint64) for m in mods])


def crt_lift(res, mods):
    """object array of the integers in [0, prod mods) with residues res[j] modulo mods[j]"""
    P = product(mods)
    out = 0
    for r, m in zip(res, mods):
        h = P // int(m)
        out = out + obj(r) * (h * pow(h % int(m), -1, int(m)))
    return out % P


@pytest.mark.parametrize("logN,nS,size", KNIFE_BASES)
def test_exact_basis_switch_on_the_rounding_edge(backend, oracle, logN, nS, size):
    """fhe_switch_basis_exact, fhe_expand_crt_basis and fhe_fast_expand_crt_basis_p_over_q on the residues of X = floor(Q/2) + d: the
    double sum that counts the multiples of Q to take off is k + 1/2 + d/Q, its rounding is decided by the order of the additions"""
    o = oracle
    rng = np.random.default_rng(813)
    N, B = 1 << logN, 2
    allq, src, dst = knife_basis(o, logN, nS, size)
    nD = len(dst)
    allpsi = roots(o, logN, allq)
    ctx = fh.Context(backend, logN, allq, allpsi)
    octx = o.orc_ctx_create(N, nS + nD, allq, allpsi)
    x, X = half_modulus_residues(rng, src, N, B)
    hatInv, hatPre, hatMod, alpha, qInv, mu = libs.crt_tables(src, dst)
    hm_pq = np.ascontiguousarray(hatMod.T)
    want = np.empty((B, nD, N), np.uint64)
    for bb in range(B):
        o.orc_switch_crt_basis(x[bb], nS, N, src, hatInv, hatPre, hm_pq, alpha, nD, dst, mu, qInv, want[bb])
    exact = np.stack([centred(X[bb], product(src), dst) for bb in range(B)])
    share = float(np.mean((want != exact).any(axis=1)))
    note_share(f"switch_basis_exact {nS} x {size}-bit", share)
    if size >= 54:
        assert share > 0, "the inputs do not sit on the rounding edge"
    src_idx, dst_idx = np.arange(nS, dtype=np.uint32), np.arange(nS, nS + nD, dtype=np.uint32)
    conv = fh.Conv(ctx, src_idx, dst_idx)
    tin = ctx.tower(x, limb_idx=src_idx, fmt=fh.COEFFICIENT)
    got = conv.run(tin, exact=True).to_host()
    assert np.array_equal(got, want), f"SwitchCRTBasis: {np.count_nonzero((got != want).any(axis=1))} coefficients differ"
    wantu = np.empty((B, nS + nD, N), np.uint64)
    for resEval, rev in ((0, 0), (1, 1)):
        for bb in range(B):
            o.orc_expand_crt_basis(octx, nS, nD, x[bb], 0, hatInv, hatPre, hm_pq, alpha, mu, qInv, resEval, rev, wantu[bb])
        got = conv.ExpandCRTBasis(tin, fh.EVALUATION if resEval else fh.COEFFICIENT, reverse=bool(rev))
        assert np.array_equal(got.to_host(), wantu), f"ExpandCRTBasis resEval={resEval} rev={rev}"
    conv.close()
    # FastExpandCRTBasisPloverQ: the value in the basis P after the first (integer) conversion is P X / Q + (0 .. nS), i.e. P/2 + small:
    # its exact switch back to Q is on the same edge
    want_pq = fast_expand_want(o, x, src, dst, N)
    P = product(dst)
    exact = np.stack([centred(crt_lift(want_pq[bb, nS:], dst), P, src) for bb in range(B)])
    share = float(np.mean((want_pq[:, :nS] != exact).any(axis=1)))
    note_share(f"fast_expand_crt_basis_p_over_q {nS} x {size}-bit", share)
    if size >= 54:
        assert share > 0, "the inputs do not sit on the rounding edge"
    to_pl, to_ql = fast_expand_plans(ctx, src, dst)
    got = to_pl.FastExpandCRTBasisPloverQ(to_ql, tin)
    assert np.array_equal(got.to_host(), want_pq), "FastExpandCRTBasisPloverQ"
    to_pl.close(), to_ql.close()
    o.orc_ctx_destroy(octx)
    ctx.close()


def scale_and_round_tables(inp, outp, t):
    """the tables of DCRTPoly::ScaleAndRound for round(t X / I) in the basis `outp`, X given over inp u outp (I = prod inp, O = prod outp,
    S = I O): tab[j][i] = floor(t O [(S/q_i)^-1]_{q_i} / q_i) mod o_j, frac[i] the fractional part of the same quotient, and
    tab[j][sizeI] = t [(S/o_j)^-1]_{o_j} (O / o_j) mod o_j"""
    S, O = product(inp) * product(outp), product(outp)
    v = [t * O * pow((S // int(s)) % int(s), -1, int(s)) for s in inp]
    tab = np.array([[(vi // int(s)) % int(oj) for vi, s in zip(v, inp)] +
                    [t * pow((S // int(oj)) % int(oj), -1, int(oj)) * (O // int(oj)) % int(oj)] for oj in outp], np.uint64)
    frac = np.array([float(Fraction(vi % int(s), int(s))) for vi, s in zip(v, inp)], np.float64)
    return tab, frac


def scale_and_round_inputs(rng, inp, outp, t, N, edge=True):
    """X = round((k + 1/2) I / t) + d + I r (k < t, |d| <= 3, r < O) over the limbs inp u outp; edge = False: uniform X"""
    I, O = product(inp), product(outp)
    X = np.empty(N, dtype=object)
    for n in range(N):
        r = int(rng.integers(0, 1 << 62)) * int(rng.integers(0, 1 << 62)) ** (len(outp)) % O
        if edge:
            k, d = int(rng.integers(0, t)), int(rng.integers(-3, 4))
            X[n] = ((2 * k + 1) * I + t) // (2 * t) + d + I * r
        else:
            X[n] = (int(rng.integers(0, 1 << 62)) ** (len(inp) + 1) % I) + I * r
    exact = np.stack([(((2 * t * X + I) // (2 * I)) % int(oj)).astype(np.uint64) for oj in outp])
    return X, exact


@pytest.mark.parametrize("logN,sizeI,sizeO,outputFirst,bits", [(6, 3, 2, 1, 60), (10, 4, 3, 0, 60), (12, 7, 8, 0, 60), (6, 2, 2, 0, 30)])
def test_scale_and_round_on_the_rounding_edge(backend, oracle, logN, sizeI, sizeO, outputFirst, bits):
    """fhe_scale_and_round (exact form) with the tables of round(t X / I) on X = round((k + 1/2) I / t) + d; the 30-bit case also
    checks the tables and the exact formula: there the double sum is exact enough for uniform X, where the oracle must agree with
    exact rounding everywhere"""
    from test_parity_bfv import mu128
    o = oracle
    rng = np.random.default_rng(814)
    N, L, B, t = 1 << logN, sizeI + sizeO, 2, 65537
    q = np.array(primes_of(o, logN, bits, L), np.uint64)
    ctx = fh.Context(backend, logN, q, roots(o, logN, q))
    off = 0 if outputFirst else sizeI
    out_idx = np.arange(off, off + sizeO, dtype=np.uint32)
    om = q[off:off + sizeO].copy()
    im = np.concatenate([q[:off], q[off + sizeO:]])
    tab, frac = scale_and_round_tables(im, om, t)
    for edge in ((True, False) if bits == 30 else (True,)):
        x, exact = np.empty((B, L, N), np.uint64), np.empty((B, sizeO, N), np.uint64)
        for b in range(B):
            X, exact[b] = scale_and_round_inputs(rng, im, om, t, N, edge)
            x[b] = np.stack([(X % int(m)).astype(np.uint64) for m in q])
        want = np.zeros((B, sizeO, N), np.uint64)
        for b in range(B):
            o.orc_scale_and_round(x[b], sizeI, sizeO, N, outputFirst, tab, frac, om, mu128(o, om), want[b])
        share = float(np.mean((want != exact).any(axis=1)))
        note_share(f"scale_and_round {sizeI} x {bits}-bit -> {sizeO}{'' if edge else ' (uniform X)'}", share)
        if not edge:
            assert share == 0, "tables / exact formula"
        elif bits >= 54:
            assert share > 0, "the inputs do not sit on the rounding edge"
        plan = fh.ScaleAndRoundPlan(ctx, sizeI, out_idx, tab, frac)
        got = plan.run(ctx.tower(x, fmt=fh.COEFFICIENT), outputFirst).to_host()
        assert np.array_equal(got, want), f"{np.count_nonzero((got != want).any(axis=1))} coefficients differ"
        plan.close()
    ctx.close()


# (the parameters of test_parity_bfv.test_scale_and_round_native: the unsplit and the split branch, t a power of two or not)
NATIVE_CASES = [(4, 2, 28, 65537, 2), (10, 3, 45, 1 << 20, 2), (12, 3, 60, 65537, 1), (12, 4, 60, 1 << 30, 1), (10, 2, 50, 786433, 2),
                (12, 3, 59, (1 << 34) - 41, 1), (4, 2, 30, (1 << 34) - 41, 2)]


def native_inputs(rng, q, t, N, B):
    Q = product(q)
    x, exact = np.empty((B, len(q), N), np.uint64), np.empty((B, N), np.uint64)
    for b in range(B):
        X = np.empty(N, dtype=object)
        for n in range(N):
            k, d = int(rng.integers(0, t)), int(rng.integers(-3, 4))
            X[n] = min(max(((2 * k + 1) * Q + t) // (2 * t) + d, 0), Q - 1)
        x[b] = np.stack([(X % int(m)).astype(np.uint64) for m in q])
        exact[b] = (((2 * t * X + Q) // (2 * Q)) % t).astype(np.uint64)
    return x, exact


@pytest.mark.parametrize("logN,sizeQ,bits,t,B", NATIVE_CASES)
def test_scale_and_round_native_on_the_rounding_edge(backend, oracle, logN, sizeQ, bits, t, B):
    """fhe_scale_and_round_native on X = round((k + 1/2) Q / t) + d"""
    from test_parity import params
    o = oracle
    rng = np.random.default_rng(815)
    N = 1 << logN
    q, psi = params(o, logN, sizeQ, bits)
    assert all(int(v).bit_length() == bits for v in q)
    a, b, fr, bf = libs.decrypt_tables(q, t)
    x, exact = native_inputs(rng, q, t, N, B)
    want = np.zeros((B, N), np.uint64)
    for bb in range(B):
        o.orc_scale_and_round_native(x[bb], sizeQ, N, q, t, a, b, fr, bf, want[bb])
    share = float(np.mean(want != exact))
    note_share(f"scale_and_round_native {sizeQ} x {bits}-bit t={t}", share)
    if bits >= 54:
        assert share > 0, "the inputs do not sit on the rounding edge"
    ctx = fh.Context(backend, logN, q, psi)
    got = fh.scale_and_round_native(ctx, ctx.tower(x, fmt=fh.COEFFICIENT), t, a, fr, b, bf)
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} coefficients differ"
    ctx.close()


# ---- the oracle against the reference build on the same inputs (CPU; skipped where oracle/_ref is absent) --------------------------
@pytest.mark.parametrize("logN", [4, 10, 12, 13])
def test_oracle_ntt_against_live_reference(oracle, ref, logN):
    """ChineseRemainderTransformFTT of the reference on every size of the set and every pattern, both directions"""
    o, r = oracle, ref
    rng = np.random.default_rng(821)
    N = 1 << logN
    q = size_set(o, logN)
    L = len(q)
    psi = roots(o, logN, q)
    octx = o.orc_ctx_create(N, L, q, psi)
    top = pattern(rng, "max", q, N)[None]
    pre_f, pre_i = top.copy(), top.copy()
    o.orc_ntt_inv_tower(octx, pre_f, None, L, 1, 0)
    o.orc_ntt_fwd_tower(octx, pre_i, None, L, 1, 0)
    for inverse, extra in ((0, pre_f), (1, pre_i)):
        x = np.concatenate([patterns(rng, PATTERNS, q, N), extra])
        got = x.copy()
        (o.orc_ntt_inv_tower if inverse else o.orc_ntt_fwd_tower)(octx, got, None, L, len(x), 0)
        for b in range(len(x)):
            for l in range(L):
                w = x[b, l].copy()
                r.ref_ntt(int(q[l]), int(psi[l]), N, w, inverse)
                assert np.array_equal(got[b, l], w), f"logN={logN} q={q[l]} inverse={inverse} tower {b}"
    o.orc_ctx_destroy(octx)


def test_oracle_switch_modulus_against_live_reference(oracle, ref):
    o, r = oracle, ref
    rng = np.random.default_rng(822)
    q = [int(v) for v in size_set(o, 12)]
    for oldq in q:
        for newq in q:
            v = np.concatenate([patterns(rng, ("max", "mix", "alt"), [oldq], 64).reshape(-1),
                                np.array([oldq // 2 - 1, oldq // 2, oldq // 2 + 1, 0, oldq - 1], np.uint64)])
            a, b = v.copy(), v.copy()
            o.orc_switch_modulus(a, len(a), oldq, newq)
            r.ref_switch_modulus(b, len(b), oldq, newq)
            assert np.array_equal(a, b), (oldq, newq)


def _pin_basis_switches(o, r, logN, allq, nS, x):
    N = 1 << logN
    src, dst = allq[:nS], allq[nS:]
    nD = len(dst)
    psi = roots(o, logN, allq)
    hatInv, hatPre, hatMod, alpha, qInv, mu = libs.crt_tables(src, dst)
    hm_pq = np.ascontiguousarray(hatMod.T)
    want, got = np.zeros((nD, N), np.uint64), np.zeros((nD, N), np.uint64)
    for xb in x:
        r.ref_approx_switch_crt_basis(N, nS, src, psi[:nS].copy(), xb, hatInv, hatMod, nD, dst, psi[nS:].copy(), want)
        o.orc_approx_switch_crt_basis(xb, nS, N, src, hatInv, hatPre, hatMod, nD, dst, mu, got)
        assert np.array_equal(got, want), "ApproxSwitchCRTBasis"
        r.ref_switch_crt_basis(N, nS, src, psi[:nS].copy(), xb, hatInv, hm_pq, alpha, nD, dst, psi[nS:].copy(), qInv, want)
        o.orc_switch_crt_basis(xb, nS, N, src, hatInv, hatPre, hm_pq, alpha, nD, dst, mu, qInv, got)
        assert np.array_equal(got, want), "SwitchCRTBasis"


@pytest.mark.parametrize("logN,ssz,dsz", CONV_CASES, ids=lambda v: "-".join(map(str, v[:4])) if isinstance(v, tuple) else str(v))
def test_oracle_basis_switches_against_live_reference(oracle, ref, logN, ssz, dsz):
    """ApproxSwitchCRTBasis and SwitchCRTBasis of the reference on the boundary bases, towers all q-1 and `mix`"""
    rng = np.random.default_rng(823)
    logN = min(logN, 8)  # (element-wise in the coefficient index: a small ring of the same sizes)
    allq = np.array(basis(oracle, logN, ssz + dsz), np.uint64)
    _pin_basis_switches(oracle, ref, logN, allq, len(ssz), limit_pair(rng, allq[:len(ssz)], 1 << logN))


@pytest.mark.parametrize("logN,nS,size", KNIFE_BASES)
def test_oracle_exact_basis_switch_on_the_rounding_edge_against_live_reference(oracle, ref, logN, nS, size):
    rng = np.random.default_rng(813)
    logN = min(logN, 8)
    allq, src, dst = knife_basis(oracle, logN, nS, size)
    x, _ = half_modulus_residues(rng, src, 1 << logN, 2)
    _pin_basis_switches(oracle, ref, logN, allq, nS, x)


def test_oracle_mod_switch_round_against_live_reference(oracle, ref):
    """SetValuesModSwitch of the reference on the rounding-edge words (the ring plays no part: the moduli need not be NTT primes)"""
    o, r = oracle, ref
    rng = np.random.default_rng(812)
    for qFrom, qTo in mod_switch_pairs(o):
        x, _ = mod_switch_inputs(rng, qFrom, qTo)
        x = x[x < qFrom].copy()  # (the 2^31 * odd words above 2^32 are not values of a polynomial modulo qFrom)
        n = 1 << (len(x).bit_length() - 1)
        x = x[:n].copy()
        want, got = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        r.ref_set_values_mod_switch(n, qFrom, 1, x, qTo, 1, want)
        o.orc_set_values_mod_switch(x, n, qFrom, qTo, got)
        assert np.array_equal(got, want), (qFrom, qTo)


@pytest.mark.parametrize("logN,sizeI,sizeO,outputFirst,bits", [(6, 3, 2, 1, 60), (6, 4, 3, 0, 60), (6, 7, 8, 0, 60), (6, 2, 2, 0, 30)])
def test_oracle_scale_and_round_on_the_rounding_edge_against_live_reference(oracle, ref, logN, sizeI, sizeO, outputFirst, bits):
    from test_parity_bfv import mu128
    o, r = oracle, ref
    rng = np.random.default_rng(814)
    N, L, t = 1 << logN, sizeI + sizeO, 65537
    q = np.array(primes_of(o, logN, bits, L), np.uint64)
    psi = roots(o, logN, q)
    off = 0 if outputFirst else sizeI
    om = q[off:off + sizeO].copy()
    im = np.concatenate([q[:off], q[off + sizeO:]])
    tab, frac = scale_and_round_tables(im, om, t)
    X, _ = scale_and_round_inputs(rng, im, om, t, N)
    x = np.stack([(X % int(m)).astype(np.uint64) for m in q])
    want, got = np.zeros((sizeO, N), np.uint64), np.zeros((sizeO, N), np.uint64)
    r.ref_scale_and_round(N, sizeI, sizeO, outputFirst, q, psi, x, tab, frac, want)
    o.orc_scale_and_round(x, sizeI, sizeO, N, outputFirst, tab, frac, om, mu128(o, om), got)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("logN,sizeQ,bits,t,B", NATIVE_CASES)
def test_oracle_scale_and_round_native_on_the_rounding_edge_against_live_reference(oracle, ref, logN, sizeQ, bits, t, B):
    from test_parity import params
    o, r = oracle, ref
    rng = np.random.default_rng(815)
    logN = min(logN, 8)
    N = 1 << logN
    q, psi = params(o, logN, sizeQ, bits)
    a, b, fr, bf = libs.decrypt_tables(q, t)
    x, _ = native_inputs(rng, q, t, N, 1)
    want, got = np.zeros(N, np.uint64), np.zeros(N, np.uint64)
    r.ref_scale_and_round_native(N, sizeQ, q, psi, x[0], t, a, b, fr, bf, want)
    o.orc_scale_and_round_native(x[0], sizeQ, N, q, t, a, b, fr, bf, got)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("bits", CHAINS, ids=chain_id)
def test_oracle_rescale_and_mod_down_against_live_reference(oracle, ref, bits):
    """DropLastElementAndScale and ApproxModDown (t = 0, 65537, 2) of the reference on the boundary chains, towers all q-1 and `mix`"""
    o, r = oracle, ref
    rng = np.random.default_rng(824)
    logN, sizeQ, dnum = 8, 5, 2
    N = 1 << logN
    q, psiQ, p, psiP = chain(o, logN, sizeQ, dnum, bits)
    octx = o.orc_ctx_create(N, sizeQ, q, psiQ)
    qs = [int(v) for v in q]
    inv = np.array([pow(qs[-1] % qi, -1, qi) for qi in qs[:-1]], np.uint64)
    neg = np.array([(qi - int(v)) % qi for v, qi in zip(inv, qs[:-1])], np.uint64)
    want, got = np.zeros((sizeQ - 1, N), np.uint64), np.zeros((sizeQ - 1, N), np.uint64)
    for xb in limit_pair(rng, q, N):
        r.ref_drop_last_element_and_scale(N, sizeQ, q, psiQ, xb, neg, inv, want)
        o.orc_drop_last_element_and_scale(octx, xb, sizeQ, got)
        assert np.array_equal(got, want), "DropLastElementAndScale"
    o.orc_ctx_destroy(octx)
    hy = o.orc_hybrid_create(N, sizeQ, q, psiQ, len(p), p, psiP, dnum)
    sizeQl = sizeQ - 1
    ql, psiQl = q[:sizeQl].copy(), psiQ[:sizeQl].copy()
    hatInv, _, hatMod, _, _, _ = libs.crt_tables(p, ql)
    P = product(p)
    pinv = np.array([pow(P % int(v), -1, int(v)) for v in ql], np.uint64)
    want, got = np.zeros((sizeQl, N), np.uint64), np.zeros((sizeQl, N), np.uint64)
    for xb in limit_pair(rng, np.concatenate([ql, p]), N):
        for t in (0, 65537, 2):
            r.ref_approx_mod_down(N, sizeQl, ql, psiQl, len(p), p, psiP, xb, pinv, hatInv, hatMod, t, want)
            if t:
                o.orc_hybrid_approx_mod_down_t(hy, xb, sizeQl, t, got)
            else:
                o.orc_hybrid_approx_mod_down(hy, xb, sizeQl, got)
            assert np.array_equal(got, want), f"ApproxModDown t={t}"
    o.orc_hybrid_destroy(hy)
