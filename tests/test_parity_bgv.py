"""BGV on the device: the fused ModReduce and the HYBRID composites with the plaintext modulus t.

  * fhe_mod_reduce / fhe_mod_reduce_limbs / fhe_mod_reduce_limbs_pair against the oracle's restatement of DCRTPolyImpl::ModReduce
    (dcrtpoly-impl.h:736-755), on every path of the dispatch: the small kernels, the single pass of N = 4096, the two-pass rings with
    both swizzle branches of the column pass, the 5-stage column pass, both formats, t below and above the limbs, and operands chosen so
    that delta = INTT(x_l) * (-t^-1 mod q_l) takes 0, 1, floor(q_l/2), floor(q_l/2) + 1 and q_l - 1 (the points where SwitchModulus and its
    negation change branch);
  * the launches of one fused call (no stand-alone modulus switch, at most one element-wise launch);
  * fhe_bgv_keyswitch_hybrid[_acc], fhe_bgv_eval_mult, fhe_bgv_ks_fast_keyswitch, fhe_bgv_eval_fast_rotation, fhe_bgv_eval_automorphism
    against orc_hybrid_precompute_digits -> orc_hybrid_inner_product -> orc_hybrid_approx_mod_down_t (-> orc_automorph_eval_k).
Every comparison is word for word."""
import ctypes as C
import os

import numpy as np
import pytest

import libs
from openfhe_amd import fhe_hip as fh
from test_parity import ckks_like_params, is_emu, params
from test_parity_edges import pattern, primes_of, roots

u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)

T_SMALL = (2, 65537, 786433)
T_BIG = (1 << 40) + 15  # larger than the 25-bit limb of the mixed chain


def big_emu():
    return bool(os.environ.get("FHE_TEST_BIG_EMU"))


# ---- ModReduce ---------------------------------------------------------------------------------------------------------------------
def delta_targets(ql):
    h = ql // 2
    return [0, 1, h, h + 1, ql - 1]


def edge_tower(o, rng, octx, qs, N, t, names, ev):
    """towers [len(names)][len(qs)][N] in the format `ev`: the kept limbs follow the named patterns, the dropped limb is built from a
    COEFFICIENT row for which delta = row * (-t^-1 mod q_l) is 0, 1, floor(q_l/2), floor(q_l/2) + 1, q_l - 1 at coefficients 0..4 and, in
    reverse order, at N-5..N-1 (checked here with python integers)"""
    l, ql = len(qs) - 1, int(qs[-1])
    negt_inv = (-pow(t % ql, -1, ql)) % ql
    tg = delta_targets(ql)
    x = np.stack([pattern(rng, n, qs, N) for n in names])
    for b in range(len(names)):
        row = rng.integers(0, ql, size=N, dtype=np.uint64)
        for j, d in enumerate(tg):
            row[j] = (d * (-t)) % ql  # delta = row * negtInv = d
            row[N - 1 - j] = row[j]
        delta = [(int(v) * negt_inv) % ql for v in list(row[:5]) + list(row[N - 5:])]
        assert delta == tg + tg[::-1], (delta, tg)
        if ev:
            row = row.reshape(1, N).copy()
            o.orc_ntt_fwd_tower(octx, row, np.array([l], np.uint32).ctypes.data_as(C.c_void_p), 1, 1, 0)
            row = row[0]
        x[b, l] = row
    return x


def tower_names(logN, B):
    return ("max", "mix", "uniform")[:B] if B > 1 else (("max",) if logN % 2 else ("mix",))


def mixed_chain(o, logN):
    """a 60-bit, a 25-bit and a 50-bit prime, in that order: dropping the 50-bit limb switches it up into the first and down into the second"""
    q = np.array([primes_of(o, logN, b, 1)[0] for b in (60, 25, 50)], np.uint64)
    return q, roots(o, logN, q)


def mod_reduce_case(backend, o, logN, q, psi, B, ts, formats, seed):
    N, sizeQl = 1 << logN, len(q)
    rng = np.random.default_rng(seed)
    ctx = fh.Context(backend, logN, q, psi)
    octx = o.orc_ctx_create(N, sizeQl, q, psi)
    try:
        for t in ts:
            for ev in formats:
                x = edge_tower(o, rng, octx, q, N, t, tower_names(logN, B), ev)
                want = np.zeros((B, sizeQl - 1, N), np.uint64)
                for b in range(B):
                    o.orc_mod_reduce(octx, x[b], sizeQl, t, ev, want[b])
                got = fh.mod_reduce(ctx, ctx.tower(x, fmt=fh.EVALUATION if ev else fh.COEFFICIENT), t).to_host()
                assert np.array_equal(got, want), f"ModReduce logN={logN} sizeQl={sizeQl} t={t} ev={ev}"
    finally:
        o.orc_ctx_destroy(octx)
        ctx.close()


# (logN, sizeQl, batch, GPU only).  At 2^13 a row has two tiles: 3 kept limbs give 6 (limb, tile) groups, not a multiple of 8, 4 give 8:
# both orders of the column pass; 2^16 and 2^17 are the 12-stage row passes (17: the 5-stage column pass)
MR_SHAPES = [(4, 3, 2, False), (12, 3, 2, False), (13, 4, 1, False), (13, 5, 3, False), (14, 3, 2, False), (16, 3, 1, True), (17, 2, 1, True)]


@pytest.mark.parametrize("logN,sizeQl,B,gpu_only", MR_SHAPES)
def test_mod_reduce_edges(backend, oracle, logN, sizeQl, B, gpu_only):
    if gpu_only and is_emu(backend) and not big_emu():
        pytest.skip("emulator: the 12-stage row passes run on the GPU (FHE_TEST_BIG_EMU=1 runs them here too)")
    q, psi = params(oracle, logN, sizeQl)
    mod_reduce_case(backend, oracle, logN, q, psi, B, T_SMALL, (1, 0) if logN in (12, 13) else (1,), 100 + logN)


@pytest.mark.parametrize("logN,B,gpu_only", [(4, 2, False), (12, 2, False), (14, 2, False), (16, 1, True)])
def test_mod_reduce_t_above_a_limb_and_both_switch_directions(backend, oracle, logN, B, gpu_only):
    if gpu_only and is_emu(backend) and not big_emu():
        pytest.skip("emulator: the 12-stage row passes run on the GPU (FHE_TEST_BIG_EMU=1 runs them here too)")
    q, psi = mixed_chain(oracle, logN)
    assert T_BIG > int(q[1]) and [int(v).bit_length() for v in q] == [60, 25, 50]
    mod_reduce_case(backend, oracle, logN, q, psi, B, (T_BIG, 65537), (1, 0) if logN == 12 else (1,), 200 + logN)


FUSED_KERNELS = ("switch_modulus_kernel", "elemwise_kernel", "elemwise_cv_kernel", "ntt_static_kernel<PRO2>", "ntt_static_kernel<EPI>")


def launches(lib):
    return np.array([lib.launch_count(k) for k in FUSED_KERNELS], np.int64)


@pytest.mark.parametrize("logN", [13, 14])
def test_fused_mod_reduce_launches(backend, oracle, logN):
    """an EVALUATION fhe_mod_reduce on a ring of two static passes: no stand-alone modulus switch, no element-wise kernel besides the
    one-row product, and the prologue and epilogue instances of the forward transform both run"""
    o = oracle
    N, sizeQl, t = 1 << logN, 3, 65537
    q, psi = params(o, logN, sizeQl)
    ctx = fh.Context(backend, logN, q, psi)
    x = ctx.tower(libs.rand_tower(np.random.default_rng(5), q, N, 2))
    before = launches(backend)
    fh.mod_reduce(ctx, x, t)
    sw, el, elcv, pro, epi = launches(backend) - before
    ctx.close()
    assert sw == 0, "a stand-alone modulus-switch kernel ran"
    assert el + elcv <= 1, "element-wise kernels besides the one-row product ran"
    assert pro >= 1 and epi >= 1, (pro, epi)


def ref_tables(qs, t):
    ql = int(qs[-1])
    return (-pow(t % ql, -1, ql)) % ql, [pow(ql % int(qi), -1, int(qi)) for qi in qs[:-1]]


def member_formula(o, sub, qs, N, x, t, negt_inv, ql_inv, ev):
    """DCRTPolyImpl::ModReduce (dcrtpoly-impl.h:736-755) with the given tables, step by step on the host: x [sizeQl][N] -> [sizeQl-1][N]"""
    l, ql = len(qs) - 1, int(qs[-1])
    li = lambda i: np.array([i], np.uint32).ctypes.data_as(C.c_void_p)
    delta = x[l].reshape(1, N).copy()
    if ev:
        o.orc_ntt_inv_tower(sub, delta, li(l), 1, 1, 0)
    delta = np.array([(int(v) * negt_inv) % ql for v in delta[0]], np.uint64)
    out = np.empty((l, N), np.uint64)
    for i in range(l):
        qi = int(qs[i])
        s = delta.copy()
        o.orc_switch_modulus(s, N, ql, qi)
        s = s.reshape(1, N)
        if ev:
            o.orc_ntt_fwd_tower(sub, s, li(i), 1, 1, 0)
        out[i] = ((x[i].astype(object) + t * s[0].astype(object)) * ql_inv[i]) % qi
    return out


@pytest.mark.parametrize("logN,ev", [(8, 1), (12, 1), (12, 0), (13, 1), (13, 0)])
def test_mod_reduce_limbs_with_the_callers_tables(backend, oracle, logN, ev):
    """a tower over scattered limbs of the context: with the reference's tables (fused on the rings of static passes), then with one
    table entry altered (the member's formula with the caller's values, launch by launch)"""
    o = oracle
    rng = np.random.default_rng(61)
    N, t = 1 << logN, 65537
    q, psiQ, _, _ = ckks_like_params(o, logN, 7, 2)
    ctx = fh.Context(backend, logN, q, psiQ)
    limbs = [5, 0, 3, 6, 2]
    sizeQl, B = len(limbs), 2
    qs = np.array([int(q[i]) for i in limbs], np.uint64)
    sub = o.orc_ctx_create(N, sizeQl, qs, np.array([int(psiQ[i]) for i in limbs], np.uint64))
    x = edge_tower(o, rng, sub, qs, N, t, ("max", "mix"), ev)
    want = np.empty((B, sizeQl - 1, N), np.uint64)
    for b in range(B):
        o.orc_mod_reduce(sub, x[b], sizeQl, t, ev, want[b])
    negt_inv, ql_inv = ref_tables(qs, t)
    xt = ctx.tower(x, limbs, fmt=fh.EVALUATION if ev else fh.COEFFICIENT)
    before = launches(backend)
    assert np.array_equal(fh.mod_reduce_limbs(ctx, xt, t, negt_inv, ql_inv).to_host(), want)
    pro = (launches(backend) - before)[3]
    assert (pro >= 1) == (ev == 1 and logN >= 13), "the reference's tables take the fused form exactly on EVALUATION towers of two-pass rings"
    for what in ("qlInvModq", "negtInvModq"):
        n2, i2 = negt_inv, list(ql_inv)
        if what == "qlInvModq":
            i2[1] = (3 * i2[1] + 1) % int(qs[1])
        else:
            n2 = (n2 + 1) % int(qs[-1])
        before = launches(backend)
        got = fh.mod_reduce_limbs(ctx, xt, t, n2, i2).to_host()
        used = launches(backend) - before
        assert used[3] == 0 and used[4] == 0, f"altered {what}: the fused kernels ran"
        for b in range(B):
            assert np.array_equal(got[b], member_formula(o, sub, qs, N, x[b], t, n2, i2, ev)), f"altered {what}, tower {b}"
    o.orc_ctx_destroy(sub)
    ctx.close()


@pytest.mark.parametrize("logN,ev", [(8, 1), (12, 1), (12, 0), (13, 1), (17, 1)])
def test_mod_reduce_pair_equals_two_single_calls(backend, oracle, logN, ev):
    """fhe_mod_reduce_limbs_pair on the two elements of a ciphertext, each a buffer of its own (in either address order)"""
    if logN == 17 and is_emu(backend) and not big_emu():
        pytest.skip("emulator: the 5-stage column pass with separately allocated towers runs on the GPU; N = 2^13 covers the emulator")
    o = oracle
    rng = np.random.default_rng(67)
    N, L, t = 1 << logN, 4, 786433
    q, psi = params(o, logN, L)
    ctx = fh.Context(backend, logN, q, psi)
    octx = o.orc_ctx_create(N, L, q, psi)
    fmt = fh.EVALUATION if ev else fh.COEFFICIENT
    h0 = edge_tower(o, rng, octx, q, N, t, ("max",), ev)
    h1 = edge_tower(o, rng, octx, q, N, t, ("mix",), ev)
    negt_inv, ql_inv = ref_tables(q, t)
    for order in (0, 1):
        if order:
            a1, a0 = ctx.tower(h1, fmt=fmt), ctx.tower(h0, fmt=fmt)
        else:
            a0, a1 = ctx.tower(h0, fmt=fmt), ctx.tower(h1, fmt=fmt)
        r0, r1 = fh.mod_reduce_pair(ctx, a0, a1, t, negt_inv, ql_inv)
        assert np.array_equal(r0.to_host(), fh.mod_reduce_limbs(ctx, a0, t, negt_inv, ql_inv).to_host())
        assert np.array_equal(r1.to_host(), fh.mod_reduce_limbs(ctx, a1, t, negt_inv, ql_inv).to_host())
    want = np.empty((L - 1, N), np.uint64)
    o.orc_mod_reduce(octx, h1[0], L, t, ev, want)
    assert np.array_equal(r1.to_host()[0], want)
    o.orc_ctx_destroy(octx)
    ctx.close()


def test_mod_reduce_argument_errors(backend, oracle):
    o = oracle
    logN, L, t = 6, 3, 65537
    N = 1 << logN
    q, psi = params(o, logN, L)
    ctx = fh.Context(backend, logN, q, psi)
    x0, x1 = ctx.tower(np.zeros((1, L, N), np.uint64)), ctx.tower(np.zeros((1, L, N), np.uint64))
    o0, o1 = ctx.empty(1, L - 1), ctx.empty(1, L - 1)
    negt_inv, ql_inv = ref_tables(q, t)
    inv = np.array(ql_inv, np.uint64)
    ip = inv.ctypes.data_as(u64p)
    wsb = backend.L.fhe_rescale_workspace_bytes(ctx.h, L, 2)
    ws = ctx.malloc(wsb)
    f, g = backend.L.fhe_mod_reduce_limbs, backend.L.fhe_mod_reduce_limbs_pair
    ql = int(q[-1])

    def bad(status, text):
        assert status != 0 and text in backend.L.fhe_last_error().decode(), (status, backend.L.fhe_last_error())

    bad(f(ctx.h, None, None, L, t, negt_inv, ip, 1, 1, o0.ptr, ws, wsb, None), "null argument")
    bad(f(ctx.h, x0.ptr, None, L, t, negt_inv, None, 1, 1, o0.ptr, ws, wsb, None), "null argument")
    bad(f(ctx.h, x0.ptr, None, 1, t, negt_inv, ip, 1, 1, o0.ptr, ws, wsb, None), "Removing last element")
    bad(f(ctx.h, x0.ptr, None, L, t, negt_inv, ip, 1, 1, o0.ptr, ws, 8, None), "workspace too small")
    bad(f(ctx.h, x0.ptr, None, L, t, negt_inv, ip, 1, 0, o0.ptr, ws, wsb, None), "workspace too small")  # (batch 0)
    far = np.array([0, 1, L], np.uint32)
    bad(f(ctx.h, x0.ptr, far.ctypes.data_as(u32p), L, t, negt_inv, ip, 1, 1, o0.ptr, ws, wsb, None), "limb index exceeds context size")
    bad(f(ctx.h, x0.ptr, None, L, 1, negt_inv, ip, 1, 1, o0.ptr, ws, wsb, None), "invertible modulo the dropped limb")
    bad(f(ctx.h, x0.ptr, None, L, 3 * ql, negt_inv, ip, 1, 1, o0.ptr, ws, wsb, None), "invertible modulo the dropped limb")
    bad(f(ctx.h, x0.ptr, None, L, t, ql, ip, 1, 1, o0.ptr, ws, wsb, None), "negtInvModq is not reduced")
    big = inv.copy()
    big[0] = q[0]
    bad(f(ctx.h, x0.ptr, None, L, t, negt_inv, big.ctypes.data_as(u64p), 1, 1, o0.ptr, ws, wsb, None), "qlInvModq is not reduced")
    bad(g(ctx.h, x0.ptr, x0.ptr, None, L, t, negt_inv, ip, 1, o0.ptr, o1.ptr, ws, wsb, None), "two distinct towers")
    bad(g(ctx.h, x0.ptr, x1.ptr, None, L, t, negt_inv, ip, 1, o0.ptr, o0.ptr, ws, wsb, None), "two distinct towers")
    bad(g(ctx.h, x0.ptr, None, None, L, t, negt_inv, ip, 1, o0.ptr, o1.ptr, ws, wsb, None), "two distinct towers")
    bad(g(ctx.h, x0.ptr, x1.ptr, None, L, t, negt_inv, ip, 1, o0.ptr, o1.ptr, ws, wsb // 2, None), "workspace too small")
    bad(backend.L.fhe_mod_reduce(ctx.h, x0.ptr, L, 2 * ql, 1, 1, o0.ptr, ws, wsb, None), "invertible modulo the dropped limb")
    assert f(ctx.h, x0.ptr, None, L, t, negt_inv, ip, 1, 1, o0.ptr, ws, wsb, None) == 0
    ctx.sync()
    ctx.close()


# ---- HYBRID composites -------------------------------------------------------------------------------------------------------------
class Hybrid:
    """a CKKS-shaped chain with its HYBRID plan on the device and in the oracle, and one evaluation key"""

    def __init__(self, backend, o, logN, sizeQ, dnum, seed):
        self.o, self.logN, self.N, self.sizeQ, self.dnum = o, logN, 1 << logN, sizeQ, dnum
        self.rng = np.random.default_rng(seed)
        self.q, psiQ, self.p, psiP = ckks_like_params(o, logN, sizeQ, dnum)
        self.sizeP = len(self.p)
        self.hy = o.orc_hybrid_create(self.N, sizeQ, self.q, psiQ, self.sizeP, self.p, psiP, dnum)
        self.allq = np.concatenate([self.q, self.p])
        self.ctx = fh.Context(backend, logN, self.allq, np.concatenate([psiQ, psiP]))
        self.plan = fh.KeySwitchPlan(self.ctx, sizeQ, self.sizeP, dnum)

    def key(self):
        return libs.rand_tower(self.rng, self.allq, self.N, self.dnum), libs.rand_tower(self.rng, self.allq, self.N, self.dnum)

    def extended(self, c, sizeQl, keyB, keyA):
        """EvalKeySwitchPrecomputeCore + EvalFastKeySwitchCoreExt of one tower c [sizeQl][N]: the two accumulators over Q_l u P"""
        o = self.o
        digits = np.zeros((self.dnum, sizeQl + self.sizeP, self.N), np.uint64)
        parts = o.orc_hybrid_precompute_digits(self.hy, c, sizeQl, digits)
        e0 = np.empty((sizeQl + self.sizeP, self.N), np.uint64)
        e1 = np.empty_like(e0)
        o.orc_hybrid_inner_product(self.hy, digits, parts, sizeQl, keyB, keyA, e0, e1)
        return e0, e1

    def down(self, e, sizeQl, t):
        out = np.empty((sizeQl, self.N), np.uint64)
        self.o.orc_hybrid_approx_mod_down_t(self.hy, e, sizeQl, t, out)
        return out

    def add(self, a, b, sizeQl):
        out = np.empty_like(a)
        for i in range(sizeQl):
            self.o.orc_vec_add(out[i], a[i], b[i], self.N, self.q[i])
        return out

    def mul(self, a, b, sizeQl):
        out = np.empty_like(a)
        for i in range(sizeQl):
            self.o.orc_vec_mul(out[i], a[i], b[i], self.N, self.q[i])
        return out

    def auto(self, a, k):
        out = np.empty_like(a)
        for i in range(a.shape[0]):
            self.o.orc_automorph_eval_k(out[i], a[i], self.N, k)
        return out

    def close(self):
        self.plan.close()
        self.ctx.close()
        self.o.orc_hybrid_destroy(self.hy)


@pytest.mark.parametrize("logN,sizeQ,dnum,sizeQl,B", [(8, 5, 2, 3, 2), (12, 6, 3, 6, 2), (13, 4, 2, 4, 4), (14, 5, 3, 4, 2), (16, 2, 2, 2, 1)])
def test_bgv_hybrid_keyswitch_and_eval_mult(backend, oracle, logN, sizeQ, dnum, sizeQl, B):
    if is_emu(backend) and logN > 13 and not big_emu():
        pytest.skip("emulator: keep the CPU suite short (FHE_TEST_BIG_EMU=1 runs these too)")
    H = Hybrid(backend, oracle, logN, sizeQ, dnum, 71)
    ctx, plan, N = H.ctx, H.plan, H.N
    keyB, keyA = H.key()
    plan.upload_key(keyB, keyA)
    ql = H.q[:sizeQl]
    a0, a1, b0, b1 = (libs.rand_tower(H.rng, ql, N, B) for _ in range(4))
    # the CKKS call first: the t = 0 path, and the plan's caches before any BGV conversion exists
    ck0, ck1 = (v.to_host() for v in plan.KeySwitchCore(ctx.tower(a0)))
    ext = [H.extended(a0[bb], sizeQl, keyB, keyA) for bb in range(B)]
    d0 = np.stack([H.mul(a0[bb], b0[bb], sizeQl) for bb in range(B)])
    d1 = np.stack([H.add(H.mul(a0[bb], b1[bb], sizeQl), H.mul(a1[bb], b0[bb], sizeQl), sizeQl) for bb in range(B)])
    d2 = np.stack([H.mul(a1[bb], b1[bb], sizeQl) for bb in range(B)])
    ext2 = [H.extended(d2[bb], sizeQl, keyB, keyA) for bb in range(B)]
    for t in (2, 65537):
        w0 = np.stack([H.down(ext[bb][0], sizeQl, t) for bb in range(B)])
        w1 = np.stack([H.down(ext[bb][1], sizeQl, t) for bb in range(B)])
        g0, g1 = plan.KeySwitchCore(ctx.tower(a0), t=t)
        assert np.array_equal(g0.to_host(), w0) and np.array_equal(g1.to_host(), w1), f"KeySwitchCore t={t}"
        acc0, acc1 = ctx.tower(a1), ctx.tower(b0)
        plan.KeySwitchCoreAcc(ctx.tower(a0), acc0, acc1, t=t)
        wa0 = np.stack([H.add(a1[bb], w0[bb], sizeQl) for bb in range(B)])
        wa1 = np.stack([H.add(b0[bb], w1[bb], sizeQl) for bb in range(B)])
        assert np.array_equal(acc0.to_host(), wa0) and np.array_equal(acc1.to_host(), wa1), f"KeySwitchCore (accumulating) t={t}"
        c0 = np.stack([H.add(d0[bb], H.down(ext2[bb][0], sizeQl, t), sizeQl) for bb in range(B)])
        c1 = np.stack([H.add(d1[bb], H.down(ext2[bb][1], sizeQl, t), sizeQl) for bb in range(B)])
        r0, r1 = plan.EvalMult(ctx.tower(a0), ctx.tower(a1), ctx.tower(b0), ctx.tower(b1), t=t)
        assert np.array_equal(r0.to_host(), c0) and np.array_equal(r1.to_host(), c1), f"EvalMult t={t}"
        if t == 2:
            assert not np.array_equal(w0, ck0), "the BGV result must differ from the CKKS one"
    # ... and the CKKS call again: same words as before the BGV calls
    k0, k1 = (v.to_host() for v in plan.KeySwitchCore(ctx.tower(a0)))
    assert np.array_equal(k0, ck0) and np.array_equal(k1, ck1)
    want0 = np.empty_like(a0)
    want1 = np.empty_like(a0)
    for bb in range(B):
        oracle.orc_hybrid_key_switch(H.hy, a0[bb], sizeQl, keyB, keyA, want0[bb], want1[bb])
    assert np.array_equal(k0, want0) and np.array_equal(k1, want1), "KeySwitchCore (t = 0) after the BGV calls"
    H.close()


@pytest.mark.parametrize("logN,sizeQ,dnum,sizeQl,B", [(10, 4, 2, 3, 2), (12, 6, 3, 6, 1), (13, 4, 2, 4, 1)])
def test_bgv_rotations(backend, oracle, logN, sizeQ, dnum, sizeQl, B):
    """fhe_bgv_eval_automorphism against digits -> inner product -> ApproxModDown(t) -> automorphism; hoisting: one fhe_ks_precompute, then
    fhe_bgv_eval_fast_rotation and fhe_bgv_ks_fast_keyswitch with two keys (and a CKKS rotation on the same digits)"""
    H = Hybrid(backend, oracle, logN, sizeQ, dnum, 73)
    ctx, plan, N = H.ctx, H.plan, H.N
    ql = H.q[:sizeQl]
    c0, c1 = libs.rand_tower(H.rng, ql, N, B), libs.rand_tower(H.rng, ql, N, B)
    t0, t1 = ctx.tower(c0), ctx.tower(c1)
    ks = [5, 25, 2 * N - 1]
    keys = [H.key() for _ in ks]
    handles = [plan.make_key(kb, ka) for kb, ka in keys]
    ext = [[H.extended(c1[bb], sizeQl, kb, ka) for bb in range(B)] for kb, ka in keys]

    def want(i, t, rotate=True):
        w0 = np.stack([H.down(ext[i][bb][0], sizeQl, t) for bb in range(B)])
        w1 = np.stack([H.down(ext[i][bb][1], sizeQl, t) for bb in range(B)])
        if not rotate:
            return w0, w1
        return (np.stack([H.auto(H.add(c0[bb], w0[bb], sizeQl), ks[i]) for bb in range(B)]),
                np.stack([H.auto(w1[bb], ks[i]) for bb in range(B)]))

    for i, k in enumerate(ks):
        for t in ((65537, 2) if i == 0 else (65537,)):
            g0, g1 = plan.EvalAutomorphism(handles[i], t0, t1, k, t=t)
            w0, w1 = want(i, t)
            assert np.array_equal(g0.to_host(), w0) and np.array_equal(g1.to_host(), w1), f"EvalAutomorphism k={k} t={t}"
    # hoisting: the digits of ONE precompute serve two keys, a plain fast key switch and a CKKS rotation
    plan.EvalFastRotationPrecompute(t1)
    for i in (1, 2):
        g0, g1 = plan.EvalFastRotation(handles[i], t0, t1, ks[i], t=65537)
        w0, w1 = want(i, 65537)
        assert np.array_equal(g0.to_host(), w0) and np.array_equal(g1.to_host(), w1), f"EvalFastRotation k={ks[i]}"
    g0, g1 = plan.FastKeySwitch(handles[0], t1, t=2)
    w0, w1 = want(0, 2, rotate=False)
    assert np.array_equal(g0.to_host(), w0) and np.array_equal(g1.to_host(), w1), "FastKeySwitch"
    e0, e1 = plan.EvalFastRotation(handles[1], t0, t1, ks[1])  # (t = 0 on the same digits)
    a0, a1 = plan.EvalAutomorphism(handles[1], t0, t1, ks[1])
    assert np.array_equal(e0.to_host(), a0.to_host()) and np.array_equal(e1.to_host(), a1.to_host())
    H.close()


def test_bgv_composite_argument_errors(backend, oracle):
    """the twins' checks plus t >= 2 and t invertible modulo every p_j, each before any launch"""
    H = Hybrid(backend, oracle, 6, 3, 2, 79)
    other = fh.KeySwitchPlan(H.ctx, H.sizeQ, H.sizeP, H.dnum)
    ctx, plan, L = H.ctx, H.plan, backend.L
    keyB, keyA = H.key()
    plan.upload_key(keyB, keyA)
    other.upload_key(keyB, keyA)
    sizeQl, t = 3, 65537
    x = [ctx.empty(1, sizeQl) for _ in range(6)]
    ws, wsb = plan.workspace(sizeQl, 1)
    p0 = int(H.p[0])

    def bad(status, text):
        assert status != 0 and text in L.fhe_last_error().decode(), (status, L.fhe_last_error())

    calls = {
        "fhe_bgv_keyswitch_hybrid": lambda key, lvl, tt, b, w: L.fhe_bgv_keyswitch_hybrid(plan.h, key, x[0].ptr, lvl, tt, b, x[1].ptr, x[2].ptr, ws, w, None),
        "fhe_bgv_keyswitch_hybrid_acc": lambda key, lvl, tt, b, w: L.fhe_bgv_keyswitch_hybrid_acc(plan.h, key, x[0].ptr, lvl, tt, b, x[1].ptr, x[2].ptr, ws, w, None),
        "fhe_bgv_eval_mult": lambda key, lvl, tt, b, w: L.fhe_bgv_eval_mult(plan.h, key, x[0].ptr, x[1].ptr, x[2].ptr, x[3].ptr, lvl, tt, b, x[4].ptr, x[5].ptr, ws, w, None),
        "fhe_bgv_ks_fast_keyswitch": lambda key, lvl, tt, b, w: L.fhe_bgv_ks_fast_keyswitch(plan.h, key, x[0].ptr, lvl, tt, b, x[1].ptr, x[2].ptr, ws, w, None),
        "fhe_bgv_eval_fast_rotation": lambda key, lvl, tt, b, w: L.fhe_bgv_eval_fast_rotation(plan.h, key, x[0].ptr, x[1].ptr, 5, lvl, tt, b, x[2].ptr, x[3].ptr, ws, w, None),
        "fhe_bgv_eval_automorphism": lambda key, lvl, tt, b, w: L.fhe_bgv_eval_automorphism(plan.h, key, x[0].ptr, x[1].ptr, 5, lvl, tt, b, x[2].ptr, x[3].ptr, ws, w, None),
    }
    for name, f in calls.items():
        bad(f(plan.key, sizeQl, 0, 1, wsb), name + ": t must be at least 2")
        bad(f(plan.key, sizeQl, 1, 1, wsb), name + ": t must be at least 2")
        bad(f(plan.key, sizeQl, p0, 1, wsb), name + ": t must be invertible modulo every p_j")
        bad(f(plan.key, sizeQl, 3 * p0, 1, wsb), name + ": t must be invertible modulo every p_j")
        bad(f(plan.key, 0, t, 1, wsb), name + ": bad level or batch")
        bad(f(plan.key, H.sizeQ + 1, t, 1, wsb), name + ": bad level or batch")
        bad(f(plan.key, sizeQl, t, 0, wsb), name + ": bad level or batch")
        bad(f(plan.key, sizeQl, t, 1, 8), name + ": workspace too small")
        bad(f(other.key, sizeQl, t, 1, wsb), name + ": bad key or null argument")
        bad(f(None, sizeQl, t, 1, wsb), name + ": bad key or null argument")
    bad(L.fhe_bgv_eval_fast_rotation(plan.h, plan.key, x[0].ptr, x[1].ptr, 4, sizeQl, t, 1, x[2].ptr, x[3].ptr, ws, wsb, None), "Automorphism index not odd")
    bad(L.fhe_bgv_eval_automorphism(plan.h, plan.key, x[0].ptr, x[1].ptr, 4, sizeQl, t, 1, x[2].ptr, x[3].ptr, ws, wsb, None), "Automorphism index not odd")
    bad(L.fhe_bgv_keyswitch_hybrid(plan.h, plan.key, None, sizeQl, t, 1, x[1].ptr, x[2].ptr, ws, wsb, None), "bad key or null argument")
    bad(L.fhe_approx_mod_down_bgv(plan.h, x[0].ptr, sizeQl, p0, 1, x[1].ptr, ws, wsb, None), "fhe_approx_mod_down_bgv: t must be invertible modulo every p_j")
    other.close()
    H.close()
