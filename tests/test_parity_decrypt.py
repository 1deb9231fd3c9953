"""Decryption on the device: decrypt_combine_kernel and the entry points on it, word for word against expectations built from the
oracle's element-wise members (orc_vec_mul / _add / _mul_const) applied in the reference's loop order (PKERNS::DecryptCore,
rns-pke.cpp:199-225: `b = cv[0]`, then `b += sPower * cv[i]; sPower *= s` from sPower = s), orc_ntt_inv_tower, and
orc_scale_and_round_native / orc_scale_and_round_behz_decrypt for the BFV tail.

  b = [c0] + s * c1 + s^2 * c2 + s^3 * c3 [+ ns * e]     mod q_i, every ciphertext, every tower row

The shapes are the smallest at which the kernel can go wrong: N = 2^4 and 2^5 (less than one workgroup of coefficients, most lanes idle),
N = 2^10 (half a tile), N = 2^12 (two tiles per row), N = 2^13 (a two-pass ring); 2, 3 and 4 elements; 1 and 3 limbs; batches of 1, 3 and 9
and the smallest batches whose last chunk of ciphertexts is short at chunk 2 and chunk 8 (the chunk is the library's choice:
fhe_decrypt_chunk); two rows of a three-row key; a limb subset of the 60/25/50/59-bit chain with a noise scale above its 25-bit limb;
every operand at q - 1 and at 0; with and without noise; without c0; in place on c[0] and on the noise tower; both output formats; the
launches of every call; every error with the outputs untouched; a BFV round trip with secret, ciphertexts and decryption on the device."""
import ctypes as C

import numpy as np
import pytest

import libs
from openfhe_amd import fhe_hip as fh
from test_parity_encrypt import add, chain, mul, mul_const
from test_parity_keygen import KEY, T_BIG, mixed_context, towers
from test_parity_edges import primes_of, roots

u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
T = 65537


def expect_core(o, qs, s, elems, noise=None, ns=1, with_c0=True):
    """s [>= L][N]; elems: list of [B][L][N] (elems[0] may be None without c0); noise [B][L][N] or None.  The reference's loop order."""
    B, L, N = elems[1].shape
    b = np.empty_like(elems[1])
    flat = lambda x, i: np.ascontiguousarray(x[:, i]).reshape(-1)
    for i, q in enumerate(int(v) for v in qs):
        srow = np.tile(s[i], B)
        acc = mul(o, srow, flat(elems[1], i), q)
        if with_c0:
            acc = add(o, flat(elems[0], i), acc, q)
        power = srow
        for e in elems[2:]:
            power = mul(o, power, srow, q)
            acc = add(o, acc, mul(o, power, flat(e, i), q), q)
        if noise is not None:
            acc = add(o, acc, mul_const(o, flat(noise, i), ns, q), q)
        b[:, i] = acc.reshape(B, N)
    return b


def to_coefficient(o, qs, psi, b):
    octx = o.orc_ctx_create(b.shape[2], len(qs), np.ascontiguousarray(qs, dtype=np.uint64), np.ascontiguousarray(psi, dtype=np.uint64))
    out = np.ascontiguousarray(b.copy())
    o.orc_ntt_inv_tower(octx, out, None, len(qs), b.shape[0], 0)
    o.orc_ctx_destroy(octx)
    return out


def operands(rng, qs, N, batch, n_elem, kind, key_rows=None):
    """(s [1][rows][N], elements, noise) uniform, at q - 1 or at 0"""
    kq = qs if key_rows is None else key_rows
    if kind == "zero":
        return np.zeros((1, len(kq), N), np.uint64), [np.zeros((batch, len(qs), N), np.uint64) for _ in range(n_elem)], np.zeros(
            (batch, len(qs), N), np.uint64)
    top = kind == "top"
    return towers(rng, kq, N, 1, top), [towers(rng, qs, N, batch, top) for _ in range(n_elem)], towers(rng, qs, N, batch, top)


def check_core(o, ctx, qs, psi, rng, batch, n_elem, kind="uniform", ns=1, idx=None, key_rows=None, what=""):
    """every form of one shape: without and with noise, without c0 (two elements), COEFFICIENT output, in place on c[0] and on the noise;
    the inputs of an out-of-place call are left as they were"""
    N = ctx.N
    s, elems, noise = operands(rng, qs, N, batch, n_elem, kind, key_rows)
    ts, te, tn = ctx.tower(s, idx), [ctx.tower(e, idx) for e in elems], ctx.tower(noise, idx)
    want = expect_core(o, qs, s[0], elems)
    want_n = expect_core(o, qs, s[0], elems, noise, ns)
    got = fh.decrypt_core(ctx, te, ts)
    assert got.fmt == fh.EVALUATION and np.array_equal(got.to_host(), want), f"{what}: no noise"
    assert np.array_equal(fh.decrypt_core(ctx, te, ts, noise=tn, ns=ns).to_host(), want_n), f"{what}: noise ns={ns}"
    assert all(np.array_equal(t.to_host(), h) for t, h in zip(te + [tn, ts], elems + [noise, s])), f"{what}: operands modified"
    got = fh.decrypt_core(ctx, te, ts, noise=tn, ns=ns, out_format=fh.COEFFICIENT)
    assert got.fmt == fh.COEFFICIENT and np.array_equal(got.to_host(), to_coefficient(o, qs, psi, want_n)), f"{what}: COEFFICIENT"
    if n_elem == 2:
        main = expect_core(o, qs, s[0], elems, noise, ns, with_c0=False)
        assert np.array_equal(fh.decrypt_core(ctx, [None, te[1]], ts, noise=tn, ns=ns, with_c0=False).to_host(), main), f"{what}: Main"
        assert np.array_equal(fh.decrypt_core(ctx, te, ts, with_c0=False).to_host(), expect_core(o, qs, s[0], elems, with_c0=False)), what
    out = fh.decrypt_core(ctx, te, ts, noise=tn, ns=ns, out=tn)
    assert out is tn and np.array_equal(tn.to_host(), want_n), f"{what}: in place on the noise"
    out = fh.decrypt_core(ctx, te, ts, out=te[0])
    assert out is te[0] and np.array_equal(te[0].to_host(), want), f"{what}: in place on c[0]"


@pytest.mark.parametrize("n_limbs", [1, 3])
@pytest.mark.parametrize("logN", [4, 5, 10, 12, 13])
def test_combine_matches_the_reference_loop(backend, oracle, logN, n_limbs):
    qs, psi = chain(oracle, logN, n_limbs)
    ctx = fh.Context(backend, logN, qs, psi)
    rng = np.random.default_rng(100 * logN + n_limbs)
    try:
        # (batch, nElem, operands, ns)
        cases = [(1, 2, "uniform", 1), (3, 3, "uniform", T), (9, 4, "uniform", T_BIG), (3, 2, "top", T), (1, 4, "top", 1), (3, 3, "zero", 2)]
        for batch, n_elem, kind, ns in cases if logN < 12 else cases[1:4]:
            check_core(oracle, ctx, qs, psi, rng, batch, n_elem, kind, ns, what=f"batch={batch} nElem={n_elem} {kind} ns={ns}")
    finally:
        ctx.close()


def short_last_chunk(ctx, n_limbs, chunk):
    """the smallest batch that the library walks in chunks of `chunk` ciphertexts with a short last chunk"""
    for batch in range(2, 1 << 14):
        if fh.decrypt_chunk(ctx, n_limbs, batch) == chunk and batch % chunk:
            return batch
    raise AssertionError(f"no batch below 2^14 is walked in chunks of {chunk}")


@pytest.mark.parametrize("logN,n_limbs,chunk,n_elem", [(4, 1, 2, 3), (4, 1, 8, 2), (10, 3, 2, 4)])
def test_batch_with_a_short_last_chunk(backend, oracle, logN, n_limbs, chunk, n_elem):
    """a batch that is no multiple of the chunk the host chose: the last workgroup of every (row, tile) walks fewer ciphertexts.  The host
    takes chunks above 1 only when they still fill the part, so these batches are the smallest that reach them (batch 9 above runs in
    chunks of 1 on a device with many compute units)"""
    qs, psi = chain(oracle, logN, n_limbs)
    ctx = fh.Context(backend, logN, qs, psi)
    try:
        assert fh.decrypt_chunk(ctx, n_limbs, 9) == backend.L.fhe_encrypt_chunk(ctx.h, n_limbs, 9)
        batch = short_last_chunk(ctx, n_limbs, chunk)
        check_core(oracle, ctx, qs, psi, np.random.default_rng(logN), batch, n_elem, ns=T, what=f"batch={batch} chunk={chunk}")
    finally:
        ctx.close()


@pytest.mark.parametrize("logN", [4, 10])
def test_lower_level_uses_the_first_rows_of_the_key(backend, oracle, logN):
    """two tower rows against a three-row key: rows 0 and 1 of the key (DropLastElements on the copy), row 2 is never read"""
    qs, psi = chain(oracle, logN, 3)
    ctx = fh.Context(backend, logN, qs, psi)
    try:
        for n_elem, ns in ((2, 1), (3, T)):
            check_core(oracle, ctx, qs[:2], psi[:2], np.random.default_rng(logN), 3, n_elem, ns=ns, key_rows=qs, what="lower level")
    finally:
        ctx.close()


@pytest.mark.parametrize("logN", [4, 10])
def test_limb_subset_on_the_mixed_chain(backend, oracle, logN):
    """context limbs (2, 0, 1) of the 60/25/50/59-bit chain, a noise scale above the 25-bit limb, operands at q - 1, uniform and 0"""
    q, ctx = mixed_context(backend, oracle, logN)
    idx = np.array([2, 0, 1], np.uint32)
    psi = roots(oracle, logN, q)
    rng = np.random.default_rng(60 + logN)
    try:
        for n_elem, ns, kind in ((2, T_BIG, "top"), (3, T_BIG, "uniform"), (4, 1, "top"), (2, T, "zero")):
            check_core(oracle, ctx, q[idx], psi[idx], rng, 3, n_elem, kind, ns, idx=idx, what=f"subset nElem={n_elem} ns={ns} {kind}")
        # a noise scale that is 1 modulo every limb in use but not 1: the product is skipped, the words are the same
        check_core(oracle, ctx, q[:1], psi[:1], rng, 1, 2, ns=int(q[0]) + 1, what="ns = q + 1")
    finally:
        ctx.close()


def launches(lib):
    total = C.c_uint64()
    lib.L.fhe_launch_stats(None, 0, C.byref(total))
    return total.value, lib.launch_count("decrypt_combine_kernel")


def spent(backend, ctx, call):
    ctx.sync()
    t0, k0 = launches(backend)
    call()
    ctx.sync()
    t1, k1 = launches(backend)
    return t1 - t0, k1 - k0


def bfv_moduli(o, logN, bits, n):
    q = np.array(primes_of(o, logN, bits, n), np.uint64)
    return q, roots(o, logN, q)


@pytest.mark.parametrize("logN", [10, 13])
def test_launches(backend, oracle, logN):
    """EVALUATION: ONE launch, the combine; COEFFICIENT: plus those of fhe_ntt_inv on the same shape; fhe_bfv_decrypt: 1 + those + 1, four
    on a two-pass ring; the same for batch 1 and 3 and for every number of elements"""
    qs, psi = bfv_moduli(oracle, logN, 50, 3)
    ctx = fh.Context(backend, logN, qs, psi)
    rng = np.random.default_rng(logN)
    plan = fh.BfvDecrypt(ctx, T, fh.BfvDecrypt.HPS)
    try:
        s = ctx.tower(towers(rng, qs, ctx.N, 1))
        seen = set()
        for batch in (1, 3):
            for n_elem in (2, 3, 4):
                te = [ctx.tower(towers(rng, qs, ctx.N, batch)) for _ in range(n_elem)]
                tn = ctx.tower(towers(rng, qs, ctx.N, batch))
                x = ctx.tower(towers(rng, qs, ctx.N, batch))
                ntt = spent(backend, ctx, lambda: ctx.lib.check(backend.L.fhe_ntt_inv(ctx.h, x.ptr, None, 3, batch, None)))[0]
                assert ntt == (2 if logN == 13 else 1)
                assert spent(backend, ctx, lambda: fh.decrypt_core(ctx, te, s)) == (1, 1)
                assert spent(backend, ctx, lambda: fh.decrypt_core(ctx, te, s, noise=tn, ns=T)) == (1, 1)
                assert spent(backend, ctx, lambda: fh.decrypt_core(ctx, te, s, out_format=fh.COEFFICIENT)) == (1 + ntt, 1)
                ws, d = ctx.malloc(plan.workspace_bytes(batch)), ctx.malloc(batch * ctx.N * 8)
                run = lambda: ctx.lib.check(backend.L.fhe_bfv_decrypt(plan.h, fh._elem_ptrs(te), n_elem, s.ptr, batch, d, ws,
                                                                      plan.workspace_bytes(batch), None))
                assert spent(backend, ctx, run) == (2 + ntt, 1)
                tail = lambda fmt: ctx.lib.check(backend.L.fhe_bfv_decrypt_b(plan.h, x.ptr, fmt, batch, d, ws, plan.workspace_bytes(batch), None))
                assert spent(backend, ctx, lambda: tail(1)) == (1 + ntt, 0) and spent(backend, ctx, lambda: tail(0)) == (1, 0)
                seen.add(2 + ntt)
        assert seen == {4 if logN == 13 else 3}
    finally:
        plan.close()
        ctx.close()


def bfv_want(o, qs, t, b_coef, technique):
    """the reference's ScaleAndRound of COEFFICIENT towers b [B][sizeQ][N] with tables from python integers"""
    B, sizeQ, N = b_coef.shape
    out = np.empty((B, N), np.uint64)
    qa = np.ascontiguousarray(qs, dtype=np.uint64)
    for k in range(B):
        if technique == fh.BfvDecrypt.BEHZ:
            tg, ta, tb = libs.behz_decrypt_tables(qs, t)
            o.orc_scale_and_round_behz_decrypt(np.ascontiguousarray(b_coef[k]), sizeQ, N, qa, tg, ta, tb, out[k])
        else:
            ta, tb, fr, bf = libs.decrypt_tables(qs, t)
            o.orc_scale_and_round_native(np.ascontiguousarray(b_coef[k]), sizeQ, N, qa, t, ta, tb, fr, bf, out[k])
    return out


# (logN, bits, sizeQ, t, technique): 60-bit moduli take the reference's split ("B") branch, 45-bit ones the unsplit branch
# (qMSB + sizeQMSB < 52); t a power of two and t = 65537 take different roundings; BEHZ has tables of its own
BFV_CASES = [(4, 60, 2, T, 1), (4, 60, 3, 1 << 16, 3), (10, 45, 3, T, 2), (5, 45, 1, 1 << 20, 1), (12, 60, 2, T, 1), (13, 45, 2, 2, 1),
             (4, 60, 2, T, 0), (10, 50, 3, 1 << 16, 0), (13, 60, 2, T, 0)]


@pytest.mark.parametrize("logN,bits,sizeQ,t,technique", BFV_CASES)
def test_bfv_decrypt_matches_the_scale_and_round_of_the_oracle(backend, oracle, logN, bits, sizeQ, t, technique):
    o = oracle
    qs, psi = bfv_moduli(o, logN, bits, sizeQ)
    split = int(max(qs)).bit_length() + sizeQ.bit_length() >= 52
    assert split == (bits == 60) or technique == 0
    ctx = fh.Context(backend, logN, qs, psi)
    rng = np.random.default_rng(logN + bits + sizeQ)
    plan = fh.BfvDecrypt(ctx, t, technique)
    try:
        if technique:
            assert (plan.table("tQHatInvModqBDivqModt") is not None) == split and plan.table("tgamma") is None
            ta, tb, fr, bf = libs.decrypt_tables(qs, t)
            assert np.array_equal(plan.table("tQHatInvModqDivqModt"), ta)
            assert not split or np.array_equal(plan.table("tQHatInvModqBDivqModt"), tb)
            # (python's correctly rounded quotient and the reference's double / double differ by an ulp at most)
            assert np.allclose(plan.table("tQHatInvModqDivqFrac").view(np.float64), fr, rtol=2 ** -51, atol=0)
        else:
            tg, ta, tb = libs.behz_decrypt_tables(qs, t)
            assert int(plan.table("tgamma")[0]) == tg and plan.table("tQHatInvModqDivqModt") is None
            assert np.array_equal(plan.table("tgammaQHatInvModq"), ta) and np.array_equal(plan.table("negInvqModtgamma"), tb)
        for batch, n_elem, kind in ((1, 2, "uniform"), (3, 3, "uniform"), (2, 4, "top")):
            s, elems, _ = operands(rng, qs, ctx.N, batch, n_elem, kind)
            b = to_coefficient(o, qs, psi, expect_core(o, qs, s[0], elems))
            want = bfv_want(o, qs, t, b, technique)
            ts, te = ctx.tower(s), [ctx.tower(e) for e in elems]
            assert np.array_equal(plan.Decrypt(te, ts), want), f"batch={batch} nElem={n_elem} {kind}"
            assert all(np.array_equal(x.to_host(), h) for x, h in zip(te + [ts], elems + [s])), "operands modified"
            # the tail alone, from either format; b is only read
            be = fh.decrypt_core(ctx, te, ts)
            assert np.array_equal(plan.DecryptB(be), want) and be.fmt == fh.EVALUATION
            assert np.array_equal(be.to_host(), expect_core(o, qs, s[0], elems)), "fhe_bfv_decrypt_b wrote to b"
            assert np.array_equal(plan.DecryptB(ctx.tower(b, fmt=fh.COEFFICIENT)), want)
    finally:
        plan.close()
        ctx.close()


@pytest.mark.parametrize("technique", [0, 1])
def test_bfv_round_trip_on_the_device(backend, oracle, technique):
    """N = 2^10, two 60-bit limbs, t = 65537: the secret from fhe_sample_ternary_blake2, ciphertexts from bfv_encrypt_sk_blake2, their
    product of three elements by hand (no relinearisation), fhe_bfv_decrypt: the residues modulo t are the message.  (Noise of a fresh
    ciphertext: |e| < 39 and the rounding of Q/t, far below Q / 2t = 2^103.)"""
    o, logN, batch = oracle, 10, 3
    qs, psi = bfv_moduli(o, logN, 60, 2)
    ctx = fh.Context(backend, logN, qs, psi)
    rng = np.random.default_rng(2027)
    N = ctx.N
    Q = int(qs[0]) * int(qs[1])
    plan = fh.BfvDecrypt(ctx, T, technique)
    try:
        s = ctx.sample("ternary", 1, 2, generator="blake2", key=KEY, counter0=0).SwitchFormat()
        msg = rng.integers(0, T, size=(batch, N), dtype=np.uint64)
        ptxt = ctx.tower(np.repeat(msg[:, None, :], 2, axis=1), fmt=fh.COEFFICIENT)
        t_inv = np.array([pow(T, -1, int(q)) for q in qs], np.uint64)
        c0, c1 = fh.bfv_encrypt_sk_blake2(ctx, s, ptxt, T, (-Q) % T, t_inv, KEY, 100, 200)
        assert np.array_equal(plan.Decrypt([c0, c1], s), msg)
        # one more element that is zero, and s^2 * c2 with c2 = 0: the same message through the three-element instance
        zero = ctx.tower(np.zeros((batch, 2, N), np.uint64))
        assert np.array_equal(plan.Decrypt([c0, c1, zero], s), msg)
        # the COEFFICIENT tower of CKKS's decryption is the same b
        b = fh.ckks_decrypt(ctx, [c0, c1], s)
        assert np.array_equal(plan.DecryptB(ctx.tower(b, fmt=fh.COEFFICIENT)), msg)
    finally:
        plan.close()
        ctx.close()


def test_errors_leave_the_outputs_untouched(backend, oracle):
    logN, n_limbs, batch = 5, 3, 2
    qs, psi = chain(oracle, logN, n_limbs)
    ctx = fh.Context(backend, logN, np.concatenate([qs, qs[:1]]), np.concatenate([psi, psi[:1]]))  # limb 3 repeats limb 0
    L, N = backend.L, ctx.N
    rng = np.random.default_rng(5)
    words = batch * n_limbs * N
    plan = fh.BfvDecrypt(ctx, T, 1, size_q=n_limbs)
    behz = fh.BfvDecrypt(ctx, T, 0, size_q=n_limbs)
    try:
        # c0 | c1 | c2 | c3 | noise | out | ws | res | spare, contiguous; s apart
        buf = ctx.upload(rng.integers(0, 1 << 20, size=9 * words, dtype=np.uint64))
        before = ctx.download(buf, (9 * words,))
        at = lambda w: C.c_void_p(buf.value + 8 * w)
        c = [at(e * words) for e in range(4)]
        noise, out, ws, res = at(4 * words), at(5 * words), at(6 * words), at(7 * words)
        s = ctx.upload(rng.integers(0, 1 << 20, size=n_limbs * N, dtype=np.uint64))
        bad_limb = np.array([0, 1, 4], np.uint32).ctypes.data_as(u32p)
        twice = np.array([0, 1, 3], np.uint32).ctypes.data_as(u32p)
        arr = lambda ps: (C.c_void_p * 4)(*[p.value if p is not None else None for p in ps])

        def core(c=c, ne=2, s=s, li=None, nl=n_limbs, b=batch, noise=noise, ns=1, c0=1, fmt=0, out=out):
            return L.fhe_decrypt_core(ctx.h, None if c is None else arr(c), ne, s, li, nl, b, noise, ns, c0, fmt, out, None)

        def bfv(p=plan, c=c, ne=2, s=s, b=batch, out=res, ws=ws, wsb=8 * words):
            return L.fhe_bfv_decrypt(p.h if p else None, None if c is None else arr(c), ne, s, b, out, ws, wsb, None)

        def tail(p=plan, x=c[0], fmt=1, b=batch, out=res, ws=ws, wsb=8 * words):
            return L.fhe_bfv_decrypt_b(p.h if p else None, x, fmt, b, out, ws, wsb, None)

        def create(li=None, n=n_limbs, t=T, tech=1):
            h = C.c_void_p()
            st = L.fhe_bfv_decrypt_create(ctx.h, li, n, t, tech, C.byref(h))
            assert st != 0 and not h.value
            return st

        cases = {
            "core: null c": (lambda: core(c=None), "null", 1),
            "core: null c[1]": (lambda: core(c=[c[0], None, c[2], c[3]]), "null", 1),
            "core: null c[0] with c0": (lambda: core(c=[None, c[1], c[2], c[3]]), "null", 1),
            "core: null c[2] of three": (lambda: core(c=[c[0], c[1], None, c[3]], ne=3), "null", 1),
            "core: null s": (lambda: core(s=None), "null", 1),
            "core: null out": (lambda: core(out=None), "null", 1),
            "core: nElem 1": (lambda: core(ne=1), "2 to 4 elements", 1),
            "core: nElem 5": (lambda: core(ne=5), "2 to 4 elements", 1),
            "core: three elements without c0": (lambda: core(ne=3, c0=0), "without c0", 1),
            "core: batch == 0": (lambda: core(b=0), "batch", 1),
            "core: nLimbs == 0": (lambda: core(nl=0), "nLimbs", 1),
            "core: limb outside the context": (lambda: core(li=bad_limb), "limb index", 1),
            "core: ns == 0 with noise": (lambda: core(ns=0), "noise scale", 1),
            "core: outFormat 2": (lambda: core(fmt=2), "outFormat", 1),
            "core: outFormat -1": (lambda: core(fmt=-1), "outFormat", 1),
            "core: out is c[1]": (lambda: core(out=c[1]), "overlap", 1),
            "core: out half over c[0]": (lambda: core(out=at(N)), "overlap", 1),
            "core: out is c[2] of three": (lambda: core(ne=3, out=c[2]), "overlap", 1),
            "core: out half over the noise": (lambda: core(out=at(4 * words + N)), "overlap", 1),
            "core: out over s": (lambda: core(s=at(5 * words + N)), "overlap", 1),
            "bfv: null plan": (lambda: bfv(p=None), "null", 1),
            "bfv: null c": (lambda: bfv(c=None), "null", 1),
            "bfv: null s": (lambda: bfv(s=None), "null", 1),
            "bfv: null out": (lambda: bfv(out=None), "null", 1),
            "bfv: null ws": (lambda: bfv(ws=None), "null", 1),
            "bfv: nElem 5": (lambda: bfv(ne=5), "2 to 4 elements", 1),
            "bfv: batch == 0": (lambda: bfv(b=0), "batch", 1),
            "bfv: short workspace": (lambda: bfv(wsb=8 * words - 8), "workspace", 1),
            "bfv: ws is c[0]": (lambda: bfv(ws=c[0]), "overlap", 1),
            "bfv: ws over c[1]": (lambda: bfv(ws=at(words + N)), "overlap", 1),
            "bfv: out in ws": (lambda: bfv(out=at(6 * words + N)), "overlap", 1),
            "bfv: out in c[1]": (lambda: bfv(out=at(words)), "overlap", 1),
            "tail: null plan": (lambda: tail(p=None), "null", 1),
            "tail: null b": (lambda: tail(x=None), "null", 1),
            "tail: null out": (lambda: tail(out=None), "null", 1),
            "tail: null ws with an EVALUATION b": (lambda: tail(ws=None), "null", 1),
            "tail: batch == 0": (lambda: tail(b=0), "batch", 1),
            "tail: short workspace": (lambda: tail(wsb=8), "workspace", 1),
            "tail: ws over b": (lambda: tail(ws=at(N)), "overlap", 1),
            "tail: out in b": (lambda: tail(out=at(N)), "overlap", 1),
            "tail: out in ws": (lambda: tail(out=at(6 * words)), "overlap", 1),
            "create: limb outside the context": (lambda: create(li=bad_limb), "limb index", 1),
            "create: equal moduli": (lambda: create(li=twice), "distinct", 1),
            "create: t == 1": (lambda: create(t=1), "plaintext modulus", 1),
            "create: technique 4": (lambda: create(tech=4), "technique", 1),
            "create: technique -1": (lambda: create(tech=-1), "technique", 1),
            "create: sizeQ == 0": (lambda: create(n=0), "sizeQ", 1),
            "create: BEHZ with t = 2^32": (lambda: create(t=1 << 32, tech=0), "BEHZ", 4),
        }
        for name, (call, text, status) in cases.items():
            assert call() == status, f"{name}: status {status} expected"
            assert text in L.fhe_last_error().decode(), (name, L.fhe_last_error().decode())
            ctx.sync()
            assert np.array_equal(ctx.download(buf, (9 * words,)), before), f"{name}: device memory changed"
        assert L.fhe_decrypt_chunk(None, 1, 1) == 0 and L.fhe_decrypt_chunk(ctx.h, 0, 1) == 0 and L.fhe_decrypt_chunk(ctx.h, 1, 0) == 0
        # ... and the same arguments without the fault run
        assert core() == 0 and core(ne=4, fmt=1) == 0 and core(c=[None, c[1], None, None], c0=0) == 0 and core(noise=None, ns=0) == 0
        assert core(out=c[0]) == 0 and core(out=noise) == 0
        assert bfv() == 0 and bfv(ne=4) == 0 and bfv(p=behz) == 0 and tail() == 0 and tail(fmt=0, ws=None, wsb=0) == 0
        ctx.sync()
    finally:
        plan.close()
        behz.close()
        ctx.close()
