"""CKKS rescale by several limbs in one fused pass (fhe_rescale_multi, fhe_rescale_multi_limbs, fhe_rescale_multi_limbs_pair).

The expected words are the reference's loop, LeveledSHECKKSRNS::ModReduceInternalInPlace(ct, levels) (ckksrns-leveledshe.cpp:172-191):
the oracle's restatement of DropLastElementAndScale applied `levels` times, after the scalar's residues were multiplied in with Python
integers, of which the first nOut limbs are kept.  Every comparison is word for word, on every path of the dispatch: the small kernels and
the single pass (step by step), the two-pass rings with both swizzle branches of the column pass, a single kept limb, chunks of at most four
limbs, the 12-stage row passes and the 5-stage column pass."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import libs
from openfhe_amd import fhe_hip as fh
from test_parity import ckks_like_params, is_emu, params
from test_parity_edges import pattern, primes_of, roots

u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)


def big_emu():
    return bool(os.environ.get("FHE_TEST_BIG_EMU"))


def sm(v, qs, qn):
    """centred SwitchModulus of one residue (mubintvecnat.cpp:109-122) over Python integers"""
    v = int(v)
    return (v - qs if v > qs // 2 else v) % qn


def tower_names(B):
    return ("max", "mix", "uniform")[:B] if B > 1 else ("mix",)


def random_scale(rng, qs):
    return np.array([int(rng.integers(1, int(q))) for q in qs], np.uint64)


def loop_of_the_reference(o, octx, x, levels, n_out=None, scale=None, qs=None):
    """x [B][sizeQl][N] over the leading limbs of octx -> [B][n_out][N]: orc_drop_last_element_and_scale `levels` times"""
    B, sizeQl, N = x.shape
    n_out = sizeQl - levels if n_out is None else n_out
    out = np.empty((B, n_out, N), np.uint64)
    for b in range(B):
        cur = np.ascontiguousarray(x[b])
        if scale is not None:
            cur = np.stack([((cur[i].astype(object) * int(scale[i])) % int(qs[i])).astype(np.uint64) for i in range(sizeQl)])
        for k in range(levels):
            nxt = np.empty((sizeQl - 1 - k, N), np.uint64)
            o.orc_drop_last_element_and_scale(octx, np.ascontiguousarray(cur), sizeQl - k, nxt)
            cur = nxt
        out[b] = cur[:n_out]
    return out


def ref_tables(qs, levels):
    """step k's QlQlInvModqlDivqlModq / qlInvModq (ckksrns-cryptoparameters.cpp:60-81), one after the other"""
    a, b = [], []
    for k in range(levels):
        ql = int(qs[len(qs) - 1 - k])
        for i in range(len(qs) - 1 - k):
            qi = int(qs[i])
            inv = pow(ql % qi, -1, qi)
            b.append(inv)
            a.append((qi - inv) % qi)
    return np.array(a, np.uint64), np.array(b, np.uint64)


def run_case(backend, o, logN, q, psi, B, levels, n_outs=(None,), scaled=False, seed=0, x=None):
    N, sizeQl = 1 << logN, len(q)
    rng = np.random.default_rng(seed)
    ctx = fh.Context(backend, logN, q, psi)
    octx = o.orc_ctx_create(N, sizeQl, q, psi)
    try:
        if x is None:
            x = np.stack([pattern(rng, n, q, N) for n in tower_names(B)])
        scale = random_scale(rng, q) if scaled else None
        xt = ctx.tower(x)
        before = backend.launch_count("ntt_static_kernel<PRO3>")
        for n_out in n_outs:
            want = loop_of_the_reference(o, octx, x, levels, n_out, scale, q)
            got = fh.rescale_multi(ctx, xt, levels, n_out, scale).to_host()
            assert got.shape == want.shape and np.array_equal(got, want), f"logN={logN} sizeQl={sizeQl} levels={levels} nOut={n_out}"
        if os.environ.get("FHE_RESCALE_UNFUSED", "0") != "0":
            assert backend.launch_count("ntt_static_kernel<PRO3>") == before, "FHE_RESCALE_UNFUSED=1: the fused kernels ran"
    finally:
        o.orc_ctx_destroy(octx)
        ctx.close()


# (logN, sizeQl, levels, batch, nOuts, with scale, GPU only)
SHAPES = [
    (4, 4, 2, 2, (None,), False, False),    # the small kernels: step by step
    (12, 4, 2, 2, (None,), False, False),   # the single pass: step by step
    (13, 5, 2, 1, (None,), False, False),   # 3 kept limbs: 6 (limb, tile) groups, not a multiple of 8
    (13, 6, 2, 3, (None,), False, False),   # 4 kept limbs: 8 groups, the other order of the column pass
    (13, 5, 4, 1, (None,), False, False),   # a single kept limb
    (14, 8, 5, 2, (None,), False, False),   # chunks of 4 + 1
    (14, 6, 3, 2, (None,), True, False),    # the scalar
    (14, 6, 3, 2, (1, 2), False, False),    # the level drop behind
    (16, 4, 2, 1, (None,), False, True),    # the 12-stage row passes
    (17, 4, 3, 1, (None,), False, True),    # the 5-stage column pass
]


@pytest.mark.parametrize("logN,sizeQl,levels,B,n_outs,scaled,gpu_only", SHAPES)
def test_rescale_multi_shapes(backend, oracle, logN, sizeQl, levels, B, n_outs, scaled, gpu_only):
    if gpu_only and is_emu(backend) and not big_emu():
        pytest.skip("emulator: the 12-stage row passes run on the GPU (FHE_TEST_BIG_EMU=1 runs them here too)")
    q, psi = params(oracle, logN, sizeQl)
    run_case(backend, oracle, logN, q, psi, B, levels, n_outs, scaled, 300 + logN + levels)


@pytest.mark.parametrize("logN", [4, 13])
def test_scale_and_level_drop_together(backend, oracle, logN):
    q, psi = params(oracle, logN, 6)
    run_case(backend, oracle, logN, q, psi, 2, 3, (1, 3), True, 330 + logN)


@pytest.mark.parametrize("logN", [4, 13])
def test_zero_scale_residue_takes_the_loop(backend, oracle, logN):
    """a scalar that is a multiple of one limb: that limb's words are all zero, by the member's own steps"""
    o = oracle
    N, sizeQl, levels = 1 << logN, 5, 2
    q, psi = params(o, logN, sizeQl)
    rng = np.random.default_rng(7)
    ctx = fh.Context(backend, logN, q, psi)
    octx = o.orc_ctx_create(N, sizeQl, q, psi)
    x = np.stack([pattern(rng, "uniform", q, N)])
    scale = random_scale(rng, q)
    scale[1] = 0
    want = loop_of_the_reference(o, octx, x, levels, None, scale, q)
    before = backend.launch_count("ntt_static_kernel<PRO3>")
    got = fh.rescale_multi(ctx, ctx.tower(x), levels, None, scale).to_host()
    assert backend.launch_count("ntt_static_kernel<PRO3>") == before
    assert np.array_equal(got, want)
    o.orc_ctx_destroy(octx)
    ctx.close()


def mixed_chain4(o, logN):
    """60, 25, 50 and 60 bits: dropping the last two limbs switches rows up and down, in the chain kernel and in the column pass's load"""
    big = primes_of(o, logN, 60, 2)
    q = np.array([big[0], primes_of(o, logN, 25, 1)[0], primes_of(o, logN, 50, 1)[0], big[1]], np.uint64)
    return q, roots(o, logN, q)


@pytest.mark.parametrize("logN", [4, 12, 13])
def test_mixed_chain_switches_up_and_down(backend, oracle, logN):
    q, psi = mixed_chain4(oracle, logN)
    assert [int(v).bit_length() for v in q] == [60, 25, 50, 60] and len(set(int(v) for v in q)) == 4
    run_case(backend, oracle, logN, q, psi, 2, 2, (None, 1), False, 400 + logN)
    run_case(backend, oracle, logN, q, psi, 2, 2, (None,), True, 410 + logN)


def targets(q):
    h = q // 2
    return [0, 1, h, h + 1, q - 1]


def edge_tower(o, rng, octx, qs, N, names):
    """towers [len(names)][len(qs)][N], EVALUATION, levels = 2: the kept limbs follow the named patterns; the two dropped limbs are built from
    COEFFICIENT rows for which r_0 AND r_1 of the chain take 0, 1, floor(q/2), floor(q/2) + 1, q - 1 at coefficients 0..4 and, in reverse
    order, at N-5..N-1 (r_1's targets run the other way round, so that the pairs differ); checked here with Python integers"""
    L = len(qs)
    m0, m1 = L - 1, L - 2
    q0, q1 = int(qs[m0]), int(qs[m1])
    t0, t1 = targets(q0), targets(q1)[::-1]
    li = lambda i: np.array([i], np.uint32).ctypes.data_as(C.c_void_p)
    x = np.stack([pattern(rng, n, qs, N) for n in names])
    for b in range(len(names)):
        e0 = rng.integers(0, q0, size=N, dtype=np.uint64)
        e1 = rng.integers(0, q1, size=N, dtype=np.uint64)
        for j in range(5):
            for pos, tj in ((j, j), (N - 1 - j, j)):
                e0[pos] = t0[tj]
                e1[pos] = (t1[tj] * q0 + sm(t0[tj], q0, q1)) % q1
        inv = pow(q0 % q1, -1, q1)
        pos = list(range(5)) + list(range(N - 5, N))
        r0 = [int(e0[p]) for p in pos]
        r1 = [((int(e1[p]) - sm(e0[p], q0, q1)) * inv) % q1 for p in pos]
        assert r0 == t0 + t0[::-1] and r1 == t1 + t1[::-1], (r0, r1)
        for m, e in ((m0, e0), (m1, e1)):
            row = e.reshape(1, N).copy()
            o.orc_ntt_fwd_tower(octx, row, li(m), 1, 1, 0)
            x[b, m] = row[0]
    return x


@pytest.mark.parametrize("logN,sizeQl,mixed", [(4, 4, False), (12, 4, False), (13, 5, False), (13, 4, True), (14, 6, False)])
def test_rounding_edges_and_operand_patterns(backend, oracle, logN, sizeQl, mixed):
    o = oracle
    q, psi = mixed_chain4(o, logN) if mixed else params(o, logN, sizeQl)
    N = 1 << logN
    octx = o.orc_ctx_create(N, len(q), q, psi)
    x = edge_tower(o, np.random.default_rng(500 + logN), octx, q, N, ("max", "mix", "uniform"))
    o.orc_ctx_destroy(octx)
    run_case(backend, o, logN, q, psi, 3, 2, (None,), False, 0, x)


@pytest.mark.parametrize("logN", [4, 12, 13])
def test_one_level_equals_fhe_rescale(backend, oracle, logN):
    o = oracle
    N, sizeQl = 1 << logN, 4
    q, psi = params(o, logN, sizeQl)
    ctx = fh.Context(backend, logN, q, psi)
    x = ctx.tower(libs.rand_tower(np.random.default_rng(21), q, N, 2))
    one = fh.rescale(ctx, x).to_host()
    assert np.array_equal(fh.rescale_multi(ctx, x, 1).to_host(), one)
    assert np.array_equal(fh.rescale_multi(ctx, x, 1, 2).to_host(), one[:, :2])  # (the fused form of one level on the two-pass ring)
    ctx.close()


@pytest.mark.parametrize("logN,levels,gpu_only", [(8, 2, False), (13, 2, False), (13, 5, False), (17, 2, True)])
def test_pair_equals_two_single_calls(backend, oracle, logN, levels, gpu_only):
    """fhe_rescale_multi_limbs_pair on the two elements of a ciphertext, each a buffer of its own (in either address order), over scattered
    limbs of the context"""
    if gpu_only and is_emu(backend) and not big_emu():
        pytest.skip("emulator: the 5-stage column pass with separately allocated towers runs on the GPU; N = 2^13 covers the emulator")
    o = oracle
    rng = np.random.default_rng(67)
    N = 1 << logN
    q, psiQ, _, _ = ckks_like_params(o, logN, 9, 2)
    ctx = fh.Context(backend, logN, q, psiQ)
    limbs = [5, 0, 3, 6, 2, 8, 1][:levels + 2]
    qs = np.array([int(q[i]) for i in limbs], np.uint64)
    sub = o.orc_ctx_create(N, len(limbs), qs, np.array([int(psiQ[i]) for i in limbs], np.uint64))
    h0, h1 = np.stack([pattern(rng, "max", qs, N)]), np.stack([pattern(rng, "mix", qs, N)])
    ta, tb = ref_tables(qs, levels)
    scale = random_scale(rng, qs)
    for order in (0, 1):
        if order:
            a1, a0 = ctx.tower(h1, limbs), ctx.tower(h0, limbs)
        else:
            a0, a1 = ctx.tower(h0, limbs), ctx.tower(h1, limbs)
        r0, r1 = fh.rescale_multi_pair(ctx, a0, a1, levels, ta, tb, None, scale)
        assert np.array_equal(r0.to_host(), fh.rescale_multi_limbs(ctx, a0, levels, ta, tb, None, scale).to_host())
        assert np.array_equal(r1.to_host(), fh.rescale_multi_limbs(ctx, a1, levels, ta, tb, None, scale).to_host())
    assert np.array_equal(r1.to_host(), loop_of_the_reference(o, sub, h1, levels, None, scale, qs))
    o.orc_ctx_destroy(sub)
    ctx.close()


def member_formula(o, sub, qs, N, x, ta, tb):
    """DropLastElementAndScale (dcrtpoly-impl.h:693-712) with the given tables on the host: x [n][N] -> [n-1][N]"""
    n = len(x)
    l, ql = n - 1, int(qs[n - 1])
    li = lambda i: np.array([i], np.uint32).ctypes.data_as(C.c_void_p)
    last = x[l].reshape(1, N).copy()
    o.orc_ntt_inv_tower(sub, last, li(l), 1, 1, 0)
    out = np.empty((l, N), np.uint64)
    for i in range(l):
        qi = int(qs[i])
        s = last[0].copy()
        o.orc_switch_modulus(s, N, ql, qi)
        s = ((s.astype(object) * int(ta[i])) % qi).astype(np.uint64).reshape(1, N)
        o.orc_ntt_fwd_tower(sub, s, li(i), 1, 1, 0)
        out[i] = (x[i].astype(object) * int(tb[i]) + s[0].astype(object)) % qi
    return out


@pytest.mark.parametrize("logN", [4, 13])
def test_foreign_tables_run_the_members_formula(backend, oracle, logN):
    """caller tables that are reduced but not the negated pair of inverses: the member's formula with the caller's values, step by step
    (the expected words at logN 4 are that formula over Python integers; at 2^13 the check is that no fused kernel runs)"""
    o = oracle
    rng = np.random.default_rng(71)
    N, levels = 1 << logN, 2
    q, psiQ, _, _ = ckks_like_params(o, logN, 7, 2)
    ctx = fh.Context(backend, logN, q, psiQ)
    limbs = [5, 0, 3, 6, 2]
    qs = np.array([int(q[i]) for i in limbs], np.uint64)
    sub = o.orc_ctx_create(N, len(limbs), qs, np.array([int(psiQ[i]) for i in limbs], np.uint64))
    x = np.stack([pattern(rng, n, qs, N) for n in ("mix", "uniform")])
    xt = ctx.tower(x, limbs)
    ta, tb = ref_tables(qs, levels)
    assert np.array_equal(fh.rescale_multi_limbs(ctx, xt, levels, ta, tb).to_host(), loop_of_the_reference(o, sub, x, levels))
    for which, at in (("a", 1), ("b", len(limbs) - 1 + 2)):  # an entry of step 0's first table, one of step 1's second
        a2, b2 = ta.copy(), tb.copy()
        t = a2 if which == "a" else b2
        qi = int(qs[at if at < len(limbs) - 1 else at - (len(limbs) - 1)])
        t[at] = (3 * int(t[at]) + 1) % qi
        before = backend.launch_count("ntt_static_kernel<PRO3>")
        got = fh.rescale_multi_limbs(ctx, xt, levels, a2, b2).to_host()
        assert backend.launch_count("ntt_static_kernel<PRO3>") == before, "foreign tables took the fused form"
        if logN == 4:
            for b in range(len(x)):
                step0 = member_formula(o, sub, qs, N, x[b], a2[:4], b2[:4])
                assert np.array_equal(got[b], member_formula(o, sub, qs, N, step0, a2[4:], b2[4:]))
    o.orc_ctx_destroy(sub)
    ctx.close()


COUNTED = ("ntt_static_kernel<PRO3>", "ntt_static_kernel<EPI>", "rescale_chain_kernel", "switch_modulus_kernel", "elemwise_kernel",
           "elemwise_cv_kernel")


def launches(lib):
    total = C.c_uint64(0)
    lib.L.fhe_launch_stats(None, 0, C.byref(total))
    return np.array([total.value] + [lib.launch_count(k) for k in COUNTED], np.int64)


@pytest.mark.parametrize("levels", [2, 4])
def test_fused_call_is_five_launches(backend, oracle, levels):
    o = oracle
    logN, sizeQl = 13, 6
    N = 1 << logN
    q, psi = params(o, logN, sizeQl)
    ctx = fh.Context(backend, logN, q, psi)
    x = ctx.tower(libs.rand_tower(np.random.default_rng(5), q, N, 1))
    scale = random_scale(np.random.default_rng(6), q)
    for sc in (None, scale):
        before = launches(backend)
        fh.rescale_multi(ctx, x, levels, None, sc)
        total, pro, epi, chain, sw, el, elcv = launches(backend) - before
        assert (total, pro, epi, chain) == (5, 1, 1, 1), (total, pro, epi, chain)
        assert sw == 0 and el + elcv == 0, "a stand-alone modulus switch or an element-wise kernel ran"
    ctx.close()


def test_argument_errors(backend, oracle):
    o = oracle
    logN, L, levels = 6, 5, 2
    N = 1 << logN
    q, psi = params(o, logN, L)
    ctx = fh.Context(backend, logN, q, psi)
    x0, x1 = ctx.tower(np.zeros((1, L, N), np.uint64)), ctx.tower(np.zeros((1, L, N), np.uint64))
    o0, o1 = ctx.empty(1, L - levels), ctx.empty(1, L - levels)
    ta, tb = ref_tables(q, levels)
    ap, bp = ta.ctypes.data_as(u64p), tb.ctypes.data_as(u64p)
    Lb = backend.L
    wsb = Lb.fhe_rescale_multi_workspace_bytes(ctx.h, L, levels, 2)
    assert wsb > 0 and Lb.fhe_rescale_multi_workspace_bytes(ctx.h, L, 0, 2) == 0 and Lb.fhe_rescale_multi_workspace_bytes(ctx.h, L, L, 2) == 0
    ws = ctx.malloc(wsb)
    f, g, h = Lb.fhe_rescale_multi, Lb.fhe_rescale_multi_limbs, Lb.fhe_rescale_multi_limbs_pair
    total = C.c_uint64(0)
    Lb.fhe_launch_stats(None, 0, C.byref(total))
    before = total.value

    def bad(status, text):
        assert status != 0 and text in Lb.fhe_last_error().decode(), (status, Lb.fhe_last_error())

    n = L - levels
    bad(f(ctx.h, None, L, levels, n, None, 1, o0.ptr, ws, wsb, None), "null argument")
    bad(f(ctx.h, x0.ptr, L, levels, n, None, 1, None, ws, wsb, None), "null argument")
    bad(f(ctx.h, x0.ptr, L, levels, n, None, 1, o0.ptr, None, wsb, None), "null argument")
    bad(g(ctx.h, x0.ptr, None, L, levels, n, None, None, bp, 1, o0.ptr, ws, wsb, None), "null argument")
    bad(g(ctx.h, x0.ptr, None, L, levels, n, None, ap, None, 1, o0.ptr, ws, wsb, None), "null argument")
    bad(h(ctx.h, x0.ptr, None, None, L, levels, n, None, ap, bp, o0.ptr, o1.ptr, ws, wsb, None), "null argument")
    bad(h(ctx.h, x0.ptr, x1.ptr, None, L, levels, n, None, ap, bp, o0.ptr, None, ws, wsb, None), "null argument")
    bad(h(ctx.h, x0.ptr, x0.ptr, None, L, levels, n, None, ap, bp, o0.ptr, o1.ptr, ws, wsb, None), "two distinct towers")
    bad(f(ctx.h, x0.ptr, L, 0, n, None, 1, o0.ptr, ws, wsb, None), "levels must be in [1, sizeQl)")
    bad(f(ctx.h, x0.ptr, L, L, 1, None, 1, o0.ptr, ws, wsb, None), "levels must be in [1, sizeQl)")
    bad(f(ctx.h, x0.ptr, 1, 1, 1, None, 1, o0.ptr, ws, wsb, None), "Removing last element")
    bad(f(ctx.h, x0.ptr, L, levels, 0, None, 1, o0.ptr, ws, wsb, None), "nOut must be in [1, sizeQl - levels]")
    bad(f(ctx.h, x0.ptr, L, levels, n + 1, None, 1, o0.ptr, ws, wsb, None), "nOut must be in [1, sizeQl - levels]")
    far = np.array([0, 1, 2, 3, L], np.uint32)
    bad(g(ctx.h, x0.ptr, far.ctypes.data_as(u32p), L, levels, n, None, ap, bp, 1, o0.ptr, ws, wsb, None), "limb index exceeds context size")
    bad(f(ctx.h, x0.ptr, L + 1, levels, n, None, 1, o0.ptr, ws, wsb, None), "Removing last element")
    for tab in (0, 1):
        a2, b2 = ta.copy(), tb.copy()
        (a2, b2)[tab][L - 1 + 1] = q[1]  # an entry of step 1
        bad(g(ctx.h, x0.ptr, None, L, levels, n, None, a2.ctypes.data_as(u64p), b2.ctypes.data_as(u64p), 1, o0.ptr, ws, wsb, None),
            "table entry is not reduced modulo its limb")
    sc = np.array([1, 1, int(q[2]), 1, 1], np.uint64)
    bad(f(ctx.h, x0.ptr, L, levels, n, sc.ctypes.data_as(u64p), 1, o0.ptr, ws, wsb, None), "scale is not reduced modulo its limb")
    bad(f(ctx.h, x0.ptr, L, levels, n, None, 1, o0.ptr, ws, 8, None), "workspace too small")
    bad(f(ctx.h, x0.ptr, L, levels, n, None, 0, o0.ptr, ws, wsb, None), "workspace too small")  # (batch 0)
    bad(f(ctx.h, x0.ptr, L, levels, n, None, 1, x0.ptr, ws, wsb, None), "out must not alias x")
    bad(h(ctx.h, x0.ptr, x1.ptr, None, L, levels, n, None, ap, bp, o0.ptr, x0.ptr, ws, wsb, None), "out must not alias x")
    Lb.fhe_launch_stats(None, 0, C.byref(total))
    assert total.value == before, "an erroneous call launched a kernel"
    assert f(ctx.h, x0.ptr, L, levels, n, None, 1, o0.ptr, ws, wsb, None) == 0
    ctx.sync(None)
    ctx.free(ws)
    ctx.close()


def test_unfused_knob_gives_the_same_words(backend):
    """FHE_RESCALE_UNFUSED is read once per process: two-pass shapes again in a child process, where every call runs the member step by
    step (run_case checks there that the fused kernels stay idle; the expected words are the same oracle loop)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FHE_RESCALE_UNFUSED="1")
    emu = is_emu(backend)
    sel = "test_rescale_multi_shapes and (13-5-2 or 14-6-3)"
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-m",
                          "not gpu" if emu else "gpu", "-k", sel if emu else f"hip and {sel}"],
                         env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert out.returncode == 0 and " passed" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_host_tables_against_python_integers(backend):
    """the triangle B, the load's weights W, the store's constants C and their Shoup companions (host_math.h rescale_multi_tables) against
    exact integers (host code only: nothing is launched)"""
    rng = np.random.default_rng(3)

    def is_prime(n):  # Miller-Rabin with the bases that decide every n < 2^64
        d, r = n - 1, 0
        while d % 2 == 0:
            d, r = d // 2, r + 1
        for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
            if a % n == 0:
                continue
            y = pow(a, d, n)
            if y in (1, n - 1):
                continue
            for _ in range(r - 1):
                y = y * y % n
                if y == n - 1:
                    break
            else:
                return False
        return True

    def prime_below(n):
        n -= 1
        while not is_prime(n):
            n -= 1
        return n

    qd = [prime_below(1 << 60), prime_below(1 << 50), prime_below(1 << 25), prime_below(1 << 59)]
    qk = [prime_below(1 << 61), prime_below(1 << 40), 65537]
    for d in (1, 2, 3, 4):
        for scaled in (False, True):
            drop, keep = qd[:d], qk
            sd = [int(rng.integers(1, v)) for v in drop] if scaled else None
            sk = [int(rng.integers(1, v)) for v in keep] if scaled else None
            arr = lambda v: np.array(v, np.uint64)
            B, W = np.zeros((d, d, 2), np.uint64), np.zeros((d, len(keep), 2), np.uint64)
            Cc, S = np.zeros((len(keep), 2), np.uint64), np.zeros((d, 2), np.uint64)
            p = lambda a: a.ctypes.data_as(u64p)
            a_d, a_k = arr(drop), arr(keep)
            a_sd, a_sk = (arr(sd), arr(sk)) if scaled else (None, None)
            assert backend.L.fhe_rescale_multi_host_tables(p(a_d), d, p(a_k), len(keep), p(a_sd) if scaled else None,
                                                           p(a_sk) if scaled else None, p(B), p(W), p(Cc), p(S)) == 0
            shoup = lambda v, m: (v << 64) // m
            for k in range(d):
                assert (int(S[k, 0]), int(S[k, 1])) == ((sd[k] if scaled else 1), shoup(sd[k] if scaled else 1, drop[k]))
                for j in range(d):
                    v = pow(drop[k], -1, drop[j]) if k < j else 0
                    assert (int(B[k, j, 0]), int(B[k, j, 1])) == (v, shoup(v, drop[j]) if k < j else 0)
            for i, m in enumerate(keep):
                s = sk[i] if scaled else 1
                prod = 1
                for k in range(d):
                    w = pow(s, -1, m) * prod % m
                    assert (int(W[k, i, 0]), int(W[k, i, 1])) == (w, shoup(w, m)), (d, k, i)
                    prod = prod * drop[k] % m
                c = s * pow(prod, -1, m) % m
                assert (int(Cc[i, 0]), int(Cc[i, 1])) == (c, shoup(c, m))
                # the identity of DESIGN 4.2 on the constants: W[k][i] * C[i] = prod_{j >= k} q_j^-1
                for k in range(d):
                    tail = 1
                    for j in range(k, d):
                        tail = tail * pow(drop[j], -1, m) % m
                    assert int(W[k, i, 0]) * c % m == tail
