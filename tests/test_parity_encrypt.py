"""Encryption on the device: encrypt_combine_kernel and the entry points on it, word for word against expectations built from the
oracle's element-wise members (orc_vec_mul / _mul_const / _add / _neg) and orc_ntt_fwd_tower.

  public key:  c0 = pkB * v + ns * e0 (+ m),  c1 = pkA * v + ns * e1
  secret key:  c0 = a * s + ns * e (+ m),     c1 = -a                       mod q_i, every ciphertext, every tower row

The shapes are the smallest at which the kernel can go wrong: N = 2^4 and 2^5 (a workgroup holds less than one 16-byte pair per lane,
most lanes idle), N = 2^10 (two pairs per lane), N = 2^12 (two tiles per row); 1 and 3 limbs; batches of 1, 3 and the smallest batch
whose last chunk of ciphertexts is short (the chunk is the library's choice: fhe_encrypt_chunk); two rows of a three-row key; a limb
subset; the 60/25/50-bit chain with a noise scale above its 25-bit limb; operands at q - 1; in place and out of place; with and without a
message; both forms; every error with the outputs untouched; the seeded forms against their composition, with the launch counts; an end
to end BGV round trip with keys and ciphertexts made on the device."""
import ctypes as C

import numpy as np
import pytest

from openfhe_amd import fhe_hip as fh
from test_parity_keygen import KEY, T_BIG, mixed_context, towers
from test_parity_edges import primes_of, roots

u32p = C.POINTER(C.c_uint32)
T = 65537


def mul(o, x, y, q):
    out = np.empty_like(x)
    o.orc_vec_mul(out, np.ascontiguousarray(x), np.ascontiguousarray(y), len(x), q)
    return out


def mul_const(o, x, c, q):
    out = np.empty_like(x)
    o.orc_vec_mul_const(out, np.ascontiguousarray(x), c % q, len(x), q)
    return out


def add(o, x, y, q):
    out = np.empty_like(x)
    o.orc_vec_add(out, np.ascontiguousarray(x), np.ascontiguousarray(y), len(x), q)
    return out


def neg(o, x, q):
    out = np.empty_like(x)
    o.orc_vec_neg(out, np.ascontiguousarray(x), len(x), q)
    return out


def expect_pk(o, qs, pkb, pka, v, e0, e1, m, ns):
    """pkb, pka [>= L][N]; v, e0, e1, m [B][L][N] (m may be None)"""
    c0, c1 = np.empty_like(v), np.empty_like(v)
    for b in range(v.shape[0]):
        for i, q in enumerate(int(x) for x in qs):
            r = add(o, mul(o, pkb[i], v[b, i], q), mul_const(o, e0[b, i], ns, q), q)
            c0[b, i] = r if m is None else add(o, r, m[b, i], q)
            c1[b, i] = add(o, mul(o, pka[i], v[b, i], q), mul_const(o, e1[b, i], ns, q), q)
    return c0, c1


def expect_sk(o, qs, s, a, e, m, ns):
    c0, c1 = np.empty_like(a), np.empty_like(a)
    for b in range(a.shape[0]):
        for i, q in enumerate(int(x) for x in qs):
            r = add(o, mul(o, a[b, i], s[i], q), mul_const(o, e[b, i], ns, q), q)
            c0[b, i] = r if m is None else add(o, r, m[b, i], q)
            c1[b, i] = neg(o, a[b, i], q)
    return c0, c1


def chain(o, logN, n_limbs):
    q = np.array([o.orc_last_prime(60, 2 << logN)] + primes_of(o, logN, 50, n_limbs - 1), np.uint64)
    return q, roots(o, logN, q)


def short_last_chunk(ctx, n_limbs, chunk):
    """the smallest batch that the library walks in chunks of `chunk` ciphertexts with a short last chunk (k * chunk + 1)"""
    for batch in range(2, 1 << 14):
        if ctx.lib.L.fhe_encrypt_chunk(ctx.h, n_limbs, batch) == chunk and batch % chunk:
            return batch
    raise AssertionError(f"no batch below 2^14 is walked in chunks of {chunk}")


def check_both_forms(o, ctx, qs, rng, batch, ns, top, with_msg, idx=None, key_rows=None, what=""):
    """one explicit public-key and one explicit secret-key call out of place, then in place, against the oracle"""
    N = ctx.N
    kq = qs if key_rows is None else key_rows  # the moduli of the key's rows (a prefix of them meets the towers)
    pkb, pka, s = (towers(rng, kq, N, 1, top)[0] for _ in range(3))
    v, e0, e1 = (towers(rng, qs, N, batch, top) for _ in range(3))
    m = towers(rng, qs, N, batch, top) if with_msg else None
    tb, ta, ts = ctx.tower(pkb, idx), ctx.tower(pka, idx), ctx.tower(s, idx)
    tv, t0, t1 = ctx.tower(v, idx), ctx.tower(e0, idx), ctx.tower(e1, idx)
    tm = None if m is None else ctx.tower(m, idx)
    w0, w1 = expect_pk(o, qs, pkb, pka, v, e0, e1, m, ns)
    c0, c1 = fh.encrypt_pk_combine(ctx, tb, ta, tv, t0, t1, tm, ns)
    assert np.array_equal(c0.to_host(), w0) and np.array_equal(c1.to_host(), w1), f"pk {what}"
    assert all(np.array_equal(t.to_host(), h) for t, h in ((tv, v), (t0, e0), (t1, e1), (tb, pkb[None]), (ta, pka[None]))), "operands modified"
    x0, x1 = expect_sk(o, qs, s, v, e0, m, ns)
    c0, c1 = fh.encrypt_sk_combine(ctx, ts, tv, t0, tm, ns)
    assert np.array_equal(c0.to_host(), x0) and np.array_equal(c1.to_host(), x1), f"sk {what}"
    assert np.array_equal(tv.to_host(), v) and np.array_equal(t0.to_host(), e0), "operands modified"
    c0, c1 = fh.encrypt_pk_combine(ctx, tb, ta, tv, t0, t1, tm, ns, in_place=True)
    assert c0 is t0 and c1 is t1 and np.array_equal(t0.to_host(), w0) and np.array_equal(t1.to_host(), w1), f"pk in place {what}"
    t0 = ctx.tower(e0, idx)
    c0, c1 = fh.encrypt_sk_combine(ctx, ts, tv, t0, tm, ns, in_place=True)
    assert c0 is t0 and c1 is tv and np.array_equal(t0.to_host(), x0) and np.array_equal(tv.to_host(), x1), f"sk in place {what}"


@pytest.mark.parametrize("n_limbs", [1, 3])
@pytest.mark.parametrize("logN", [4, 5, 10, 12])
def test_combine_matches_the_formula(backend, oracle, logN, n_limbs):
    qs, psi = chain(oracle, logN, n_limbs)
    ctx = fh.Context(backend, logN, qs, psi)
    rng = np.random.default_rng(100 * logN + n_limbs)
    try:
        cases = [(1, 1, False, True), (3, T, False, True), (3, 2, True, False), (1, T_BIG, True, True), (3, 1, False, False)]
        for batch, ns, top, with_msg in cases if logN < 12 else cases[1:3]:
            check_both_forms(oracle, ctx, qs, rng, batch, ns, top, with_msg, what=f"batch={batch} ns={ns} top={top} msg={with_msg}")
    finally:
        ctx.close()


@pytest.mark.parametrize("logN,n_limbs,chunk", [(4, 1, 2), (4, 1, 8), (10, 3, 2)])
def test_batch_with_a_short_last_chunk(backend, oracle, logN, n_limbs, chunk):
    """a batch that is no multiple of the chunk the host chose: the last workgroup of every (row, tile) walks fewer ciphertexts.  The
    host takes chunks above 1 only when they still fill the part, so these batches are the smallest that reach them: on 256 compute units
    2047 and 8185 rows of 16 words, and 683 towers of 3 x 1024."""
    qs, psi = chain(oracle, logN, n_limbs)
    ctx = fh.Context(backend, logN, qs, psi)
    try:
        batch = short_last_chunk(ctx, n_limbs, chunk)
        check_both_forms(oracle, ctx, qs, np.random.default_rng(logN), batch, T, False, True, what=f"batch={batch} chunk={chunk}")
    finally:
        ctx.close()


@pytest.mark.parametrize("logN", [4, 10])
def test_prefix_level_uses_the_first_rows_of_the_key(backend, oracle, logN):
    """two tower rows against a three-row key: rows 0 and 1 of the key (DropLastElements on the clones), row 2 is never read"""
    qs, psi = chain(oracle, logN, 3)
    ctx = fh.Context(backend, logN, qs, psi)
    try:
        for ns, with_msg in ((1, True), (T, False)):
            check_both_forms(oracle, ctx, qs[:2], np.random.default_rng(logN), 3, ns, False, with_msg, key_rows=qs, what="prefix level")
    finally:
        ctx.close()


@pytest.mark.parametrize("logN", [4, 10])
def test_limb_subset_on_the_mixed_chain(backend, oracle, logN):
    """context limbs (2, 0, 1) of the 60/25/50/59-bit chain, a noise scale above the 25-bit limb, operands at q - 1 and uniform"""
    q, ctx = mixed_context(backend, oracle, logN)
    idx = np.array([2, 0, 1], np.uint32)
    rng = np.random.default_rng(60 + logN)
    try:
        for ns, top, with_msg in ((T_BIG, True, True), (T_BIG, False, False), (1, True, False), (T, False, True)):
            check_both_forms(oracle, ctx, q[idx], rng, 3, ns, top, with_msg, idx=idx, what=f"subset ns={ns} top={top}")
        # a noise scale that is 1 modulo every limb in use but not 1: the product is skipped, the words are the same
        check_both_forms(oracle, ctx, q[:1], rng, 1, int(q[0]) + 1, False, True, what="ns = q + 1")
    finally:
        ctx.close()


def launches(lib):
    total = C.c_uint64()
    lib.L.fhe_launch_stats(None, 0, C.byref(total))
    return total.value, lib.launch_count("encrypt_combine_kernel")


def composition_pk(o, ctx, qs, tb, ta, batch, n_limbs, v_dist, ns, sigma, cv, ce, m, idx=None):
    """the public-key ciphertexts from the separate sampler, fhe_ntt_fwd and explicit-combine calls; a COEFFICIENT message joins e0"""
    v = ctx.sample("ternary" if v_dist == fh.TERNARY else "gaussian", batch, n_limbs, limb_idx=idx, sigma=sigma, generator="blake2", key=KEY,
                   counter0=cv).SwitchFormat()
    e = ctx.sample("gaussian", 2 * batch, n_limbs, limb_idx=idx, sigma=sigma, generator="blake2", key=KEY, counter0=ce)
    e0, e1 = fh._window(e, 0, batch), fh._window(e, batch, batch)
    if m is not None and m.fmt == fh.COEFFICIENT:
        ctx.lib.check(ctx.lib.L.fhe_add(ctx.h, e0.ptr, e0.ptr, m.ptr, e0._li(), n_limbs, batch, None))
    e.SwitchFormat()
    e0.fmt = e1.fmt = fh.EVALUATION
    c0, c1 = fh.encrypt_pk_combine(ctx, tb, ta, v, e0, e1, m if m is not None and m.fmt == fh.EVALUATION else None, ns)
    return c0.to_host(), c1.to_host()


@pytest.mark.parametrize("logN,n_limbs,ns,v_dist", [(10, 3, T, fh.TERNARY), (5, 1, 1, fh.GAUSSIAN), (13, 2, 1, fh.TERNARY)])
def test_seeded_public_key_form_is_its_composition(backend, oracle, logN, n_limbs, ns, v_dist):
    """fhe_encrypt_pk_blake2 == the sampler calls + fhe_ntt_fwd + fhe_encrypt_pk_combine with the same key and counters, word for word;
    exactly one combine launch; the same number of launches for batch 1 and batch 3; at N = 2^13 (a two-pass ring) five launches with
    the contiguous workspace; a COEFFICIENT message costs one launch more"""
    o = oracle
    qs, psi = chain(o, logN, n_limbs)
    ctx = fh.Context(backend, logN, qs, psi)
    rng = np.random.default_rng(90 + logN)
    N, sigma = ctx.N, 3.19
    try:
        tb, ta = ctx.tower(towers(rng, qs, N, 1)), ctx.tower(towers(rng, qs, N, 1))
        spent = {}
        for batch in (1, 3, 2):
            nv, ne = fh.encrypt_counters(ctx, n_limbs, batch)
            assert nv == -(-batch * N // 512) and ne == -(-2 * batch * N // 512)
            cv, ce = 7, 7 + nv  # disjoint counter ranges, laid out with the counts
            m = ctx.tower(towers(rng, qs, N, batch))
            want = composition_pk(o, ctx, qs, tb, ta, batch, n_limbs, v_dist, ns, sigma, cv, ce, m)
            for contiguous in (True, False):
                ctx.sync()
                t0, k0 = launches(backend)
                c0, c1 = fh.encrypt_pk_blake2(ctx, tb, ta, batch, KEY, cv, ce, msg=m, ns=ns, sigma=sigma, v_dist=v_dist, contiguous=contiguous)
                t1, k1 = launches(backend)
                assert k1 - k0 == 1, "exactly one combine launch"
                spent[batch, contiguous] = t1 - t0
                assert np.array_equal(c0.to_host(), want[0]) and np.array_equal(c1.to_host(), want[1]), f"batch={batch} contiguous={contiguous}"
            if ns == 1:  # the BFV path: the message in COEFFICIENT format
                mc = ctx.tower(towers(rng, qs, N, batch), fmt=fh.COEFFICIENT)
                want = composition_pk(o, ctx, qs, tb, ta, batch, n_limbs, v_dist, ns, sigma, cv, ce, mc)
                t0, _ = launches(backend)
                c0, c1 = fh.encrypt_pk_blake2(ctx, tb, ta, batch, KEY, cv, ce, msg=mc, ns=ns, sigma=sigma, v_dist=v_dist)
                t1, _ = launches(backend)
                assert t1 - t0 == spent[batch, True] + 1, "a COEFFICIENT message is one launch more"
                assert np.array_equal(c0.to_host(), want[0]) and np.array_equal(c1.to_host(), want[1]), f"COEFFICIENT batch={batch}"
        assert spent[1, True] == spent[3, True] and spent[1, False] == spent[3, False], spent
        if logN == 13:
            # sampler v, sampler e0 ‖ e1, two passes of ONE transform, the combine; apart: the passes of two transforms
            assert spent[2, True] == 5 and spent[2, False] == 7, spent
        # apart from ct, the call costs what the composition costs (counted, not assumed)
        t0, _ = launches(backend)
        composition_pk(o, ctx, qs, tb, ta, 2, n_limbs, v_dist, ns, sigma, 7, 99, None)
        t1, _ = launches(backend)
        assert spent[2, False] == t1 - t0, "apart from ct, the workspace costs the composition's launches"
    finally:
        ctx.close()


@pytest.mark.parametrize("logN,n_limbs,ns", [(10, 3, T), (5, 1, 1), (13, 2, 1)])
def test_seeded_secret_key_form_is_its_composition(backend, oracle, logN, n_limbs, ns):
    qs, psi = chain(oracle, logN, n_limbs)
    ctx = fh.Context(backend, logN, qs, psi)
    rng = np.random.default_rng(70 + logN)
    N, sigma = ctx.N, 3.19
    try:
        ts = ctx.tower(towers(rng, qs, N, 1))
        spent = {}
        for batch in (1, 3):
            na, ne = fh.encrypt_counters(ctx, n_limbs, batch, fh.SECRET_KEY)
            assert na == -(-2 * batch * n_limbs * N // 512) and ne == -(-batch * N // 512)
            ca, ce = 11, 11 + na
            m = ctx.tower(towers(rng, qs, N, batch))
            a = ctx.sample("uniform", batch, n_limbs, generator="blake2", key=KEY, counter0=ca)
            a.fmt = fh.EVALUATION  # used as drawn
            e = ctx.sample("gaussian", batch, n_limbs, sigma=sigma, generator="blake2", key=KEY, counter0=ce).SwitchFormat()
            w0, w1 = fh.encrypt_sk_combine(ctx, ts, a, e, m, ns)
            ctx.sync()
            t0, k0 = launches(backend)
            c0, c1 = fh.encrypt_sk_blake2(ctx, ts, batch, KEY, ca, ce, msg=m, ns=ns, sigma=sigma)
            ctx.sync()
            t1, k1 = launches(backend)
            spent[batch] = t1 - t0
            assert k1 - k0 == 1, "exactly one combine launch"
            assert np.array_equal(c1.to_host(), w1.to_host()), "the c1 half is not minus the uniform sampler's words"
            assert np.array_equal(c0.to_host(), w0.to_host()), f"batch={batch}"
            if ns == 1:
                mc = ctx.tower(towers(rng, qs, N, batch), fmt=fh.COEFFICIENT)
                e = ctx.sample("gaussian", batch, n_limbs, sigma=sigma, generator="blake2", key=KEY, counter0=ce)
                w0, w1 = fh.encrypt_sk_combine(ctx, ts, a, e.Plus(mc).SwitchFormat(), None, ns)
                t0, _ = launches(backend)
                c0, c1 = fh.encrypt_sk_blake2(ctx, ts, batch, KEY, ca, ce, msg=mc, ns=ns, sigma=sigma)
                ctx.sync()
                t1, _ = launches(backend)
                assert t1 - t0 == spent[batch] + 1
                assert np.array_equal(c0.to_host(), w0.to_host()) and np.array_equal(c1.to_host(), w1.to_host()), "COEFFICIENT message"
        assert spent[1] == spent[3], spent
        if logN == 13:
            assert spent[1] == 5, spent  # two samplers, two passes of one transform, the combine
    finally:
        ctx.close()


def test_the_samplers_consume_the_counted_ranges(backend, oracle):
    """fhe_encrypt_counters == the blocks the samplers consume (512 words of 64 bits per 4 KiB block: one word per ternary / Gaussian
    coefficient, two per uniform residue), and the ranges are used as documented: with pkB = 1 and pkA = 0 the ciphertext is
    (v + e0, e1), v the ternary sampler's towers from counter_v and e0 ‖ e1 ONE Gaussian call over 2 * batch towers from counter_e"""
    logN, n_limbs, batch = 10, 2, 3
    qs, psi = chain(oracle, logN, n_limbs)
    ctx = fh.Context(backend, logN, qs, psi)
    N = ctx.N
    try:
        nv, ne = fh.encrypt_counters(ctx, n_limbs, batch)
        na, ne_sk = fh.encrypt_counters(ctx, n_limbs, batch, fh.SECRET_KEY)
        # words per 4 KiB block: 512; one word per ternary / Gaussian coefficient, two per uniform residue
        assert (nv, ne, na, ne_sk) == (batch * N // 512, 2 * batch * N // 512, 2 * batch * n_limbs * N // 512, batch * N // 512)
        n0, n1 = C.c_uint64(), C.c_uint64()
        assert backend.L.fhe_encrypt_counters(ctx.h, n_limbs, batch, 2, C.byref(n0), C.byref(n1)) == 1  # unknown form
        assert backend.L.fhe_encrypt_counters(ctx.h, n_limbs, 0, 0, C.byref(n0), C.byref(n1)) == 1
        assert fh.encrypt_counters(ctx, 1, 1) == (2, 4) and fh.encrypt_counters(ctx, 3, 1, fh.SECRET_KEY) == (12, 2)
        one, zero = ctx.tower(np.ones((1, n_limbs, N), np.uint64)), ctx.tower(np.zeros((1, n_limbs, N), np.uint64))
        c0, c1 = fh.encrypt_pk_blake2(ctx, one, zero, batch, KEY, 5, 5 + nv)
        v = ctx.sample("ternary", batch, n_limbs, generator="blake2", key=KEY, counter0=5).SwitchFormat()
        e = ctx.sample("gaussian", 2 * batch, n_limbs, generator="blake2", key=KEY, counter0=5 + nv)
        want = e.to_host()  # ... transformed by the oracle
        octx = oracle.orc_ctx_create(N, n_limbs, qs, psi)
        oracle.orc_ntt_fwd_tower(octx, want, None, n_limbs, 2 * batch, 0)
        oracle.orc_ctx_destroy(octx)
        assert np.array_equal(c1.to_host(), want[batch:])
        assert np.array_equal(c0.to_host(), v.Plus(ctx.tower(want[:batch])).to_host())
    finally:
        ctx.close()


def test_errors_leave_the_outputs_untouched(backend, oracle):
    logN, n_limbs, batch = 5, 3, 2
    qs, psi = chain(oracle, logN, n_limbs)
    ctx = fh.Context(backend, logN, qs, psi)
    L, N = backend.L, ctx.N
    rng = np.random.default_rng(5)
    words = batch * n_limbs * N
    try:
        # v | e0 | e1 | ct (2 slabs) | ws | msg | spare, contiguous
        buf = ctx.upload(rng.integers(0, 1 << 20, size=8 * words, dtype=np.uint64))
        before = ctx.download(buf, (8 * words,))
        at = lambda w: C.c_void_p(buf.value + 8 * w)
        v, e0, e1, ct, ws, msg = at(0), at(words), at(2 * words), at(3 * words), at(5 * words), at(6 * words)
        c0, c1 = ct, at(4 * words)
        keys = ctx.upload(rng.integers(0, 1 << 20, size=3 * n_limbs * N, dtype=np.uint64))  # pkB | pkA | s
        pkb, pka, s = keys, C.c_void_p(keys.value + 8 * n_limbs * N), C.c_void_p(keys.value + 16 * n_limbs * N)
        key = np.frombuffer(KEY, dtype="<u4").astype(np.uint32).ctypes.data_as(u32p)
        bad_limb = np.array([0, 1, 3], np.uint32).ctypes.data_as(u32p)

        def pk(li=None, nl=n_limbs, b=batch, pkb=pkb, pka=pka, v=v, e0=e0, e1=e1, msg=msg, ns=1, c0=c0, c1=c1):
            return L.fhe_encrypt_pk_combine(ctx.h, li, nl, b, pkb, pka, v, e0, e1, msg, ns, c0, c1, None)

        def sk(nl=n_limbs, b=batch, s=s, a=v, e=e0, msg=msg, ns=1, c0=c0, c1=c1):
            return L.fhe_encrypt_sk_combine(ctx.h, None, nl, b, s, a, e, msg, ns, c0, c1, None)

        def spk(nl=n_limbs, b=batch, pkb=pkb, pka=pka, vd=0, ns=1, sigma=3.19, key=key, msg=msg, fmt=0, ct=ct, ws=ws, wsb=8 * words):
            return L.fhe_encrypt_pk_blake2(ctx.h, None, nl, b, pkb, pka, vd, ns, sigma, key, 0, 1 << 20, msg, fmt, ct, ws, wsb, None)

        def ssk(nl=n_limbs, b=batch, s=s, ns=1, sigma=3.19, key=key, msg=msg, fmt=0, ct=ct):
            return L.fhe_encrypt_sk_blake2(ctx.h, None, nl, b, s, ns, sigma, key, 0, 1 << 20, msg, fmt, ct, None)

        cases = {
            "pk: batch == 0": (lambda: pk(b=0), "batch"),
            "pk: nLimbs == 0": (lambda: pk(nl=0), "nLimbs"),
            "pk: limb outside the context": (lambda: pk(li=bad_limb), "limb index"),
            "pk: ns == 0": (lambda: pk(ns=0), "noise scale"),
            "pk: null pkB": (lambda: pk(pkb=None), "null"),
            "pk: null pkA": (lambda: pk(pka=None), "null"),
            "pk: null v": (lambda: pk(v=None), "null"),
            "pk: null e0": (lambda: pk(e0=None), "null"),
            "pk: null e1": (lambda: pk(e1=None), "null"),
            "pk: null c0": (lambda: pk(c0=None), "null"),
            "pk: null c1": (lambda: pk(c1=None), "null"),
            "pk: c0 half over e0": (lambda: pk(c0=at(words + N), c1=at(7 * words)), "overlap"),
            "pk: c0 is e1": (lambda: pk(c0=e1), "overlap"),
            "pk: c1 is e0": (lambda: pk(c1=e0), "overlap"),
            "pk: c1 is c0": (lambda: pk(c1=c0), "overlap"),
            "pk: c0 is v": (lambda: pk(c0=v), "overlap"),
            "pk: v is e0": (lambda: pk(v=e0), "overlap"),
            "pk: v over e1": (lambda: pk(v=at(2 * words - N)), "overlap"),
            "pk: c0 over msg": (lambda: pk(c0=at(6 * words - N), c1=at(7 * words)), "overlap"),
            "pk: c1 over pkB": (lambda: pk(pkb=at(4 * words + N)), "overlap"),
            "pk: c0 over pkA": (lambda: pk(pka=at(3 * words)), "overlap"),
            "sk: batch == 0": (lambda: sk(b=0), "batch"),
            "sk: nLimbs == 0": (lambda: sk(nl=0), "nLimbs"),
            "sk: ns == 0": (lambda: sk(ns=0), "noise scale"),
            "sk: null s": (lambda: sk(s=None), "null"),
            "sk: null a": (lambda: sk(a=None), "null"),
            "sk: null e": (lambda: sk(e=None), "null"),
            "sk: null c1": (lambda: sk(c1=None), "null"),
            "sk: c0 is a": (lambda: sk(c0=v), "overlap"),
            "sk: c1 is e": (lambda: sk(c1=e0), "overlap"),
            "sk: c1 half over a": (lambda: sk(c1=at(N)), "overlap"),
            "sk: c0 over s": (lambda: sk(s=at(3 * words + N)), "overlap"),
            "sk: c1 over msg": (lambda: sk(msg=at(4 * words)), "overlap"),
            "seeded pk: batch == 0": (lambda: spk(b=0), "batch"),
            "seeded pk: nLimbs == 0": (lambda: spk(nl=0), "nLimbs"),
            "seeded pk: ns == 0": (lambda: spk(ns=0), "noise scale"),
            "seeded pk: sigma 0.5": (lambda: spk(sigma=0.5), "sigma"),
            "seeded pk: sigma 300": (lambda: spk(sigma=300.0), "sigma"),
            "seeded pk: vDist 2": (lambda: spk(vd=2), "vDist"),
            "seeded pk: msgFormat 2": (lambda: spk(fmt=2), "msgFormat"),
            "seeded pk: COEFFICIENT message with ns = t": (lambda: spk(ns=T, fmt=1), "COEFFICIENT"),
            "seeded pk: null key": (lambda: spk(key=None), "null"),
            "seeded pk: null pkA": (lambda: spk(pka=None), "null"),
            "seeded pk: null ct": (lambda: spk(ct=None), "null"),
            "seeded pk: null ws": (lambda: spk(ws=None), "null"),
            "seeded pk: short workspace": (lambda: spk(wsb=8 * words - 8), "workspace"),
            "seeded pk: ws inside ct": (lambda: spk(ws=at(4 * words + N)), "overlap"),
            "seeded pk: ws over msg": (lambda: spk(ws=at(6 * words - N)), "overlap"),
            "seeded pk: ws over the key": (lambda: spk(pkb=at(5 * words)), "overlap"),
            "seeded pk: ct over msg": (lambda: spk(msg=at(4 * words), ws=at(7 * words)), "overlap"),
            "seeded pk: ct over pkB": (lambda: spk(pkb=at(3 * words + N)), "overlap"),
            "seeded sk: batch == 0": (lambda: ssk(b=0), "batch"),
            "seeded sk: ns == 0": (lambda: ssk(ns=0), "noise scale"),
            "seeded sk: sigma 1": (lambda: ssk(sigma=1.0), "sigma"),
            "seeded sk: msgFormat -1": (lambda: ssk(fmt=-1), "msgFormat"),
            "seeded sk: COEFFICIENT message with ns = 2": (lambda: ssk(ns=2, fmt=1), "COEFFICIENT"),
            "seeded sk: null key": (lambda: ssk(key=None), "null"),
            "seeded sk: null s": (lambda: ssk(s=None), "null"),
            "seeded sk: null ct": (lambda: ssk(ct=None), "null"),
            "seeded sk: ct over s": (lambda: ssk(s=at(4 * words)), "overlap"),
            "seeded sk: ct over msg": (lambda: ssk(msg=at(3 * words + N)), "overlap"),
        }
        for name, (call, text) in cases.items():
            assert call() == 1, f"{name}: FHE_ERR_ARG expected"
            assert text in L.fhe_last_error().decode(), (name, L.fhe_last_error().decode())
            ctx.sync()
            assert np.array_equal(ctx.download(buf, (8 * words,)), before), f"{name}: device memory changed"
        # ... and the same arguments without the fault run (a COEFFICIENT message with ns = q_0 + 1 on limb 0 alone too)
        assert pk() == 0 and sk() == 0 and spk() == 0 and ssk() == 0 and spk(fmt=1) == 0 and ssk(fmt=1) == 0
        assert pk(c0=e0, c1=e1) == 0 and sk(c0=e0, c1=v) == 0
        assert ssk(nl=1, ns=int(qs[0]) + 1, fmt=1) == 0
        ctx.sync()
    finally:
        ctx.close()


@pytest.mark.parametrize("v_dist", [fh.TERNARY, fh.GAUSSIAN])
def test_bgv_round_trip_on_the_device(backend, oracle, v_dist):
    """N = 2^10, 3 limbs, t = 65537: the secret from fhe_sample_ternary_blake2, the public key from public_key, fhe_encrypt_pk_blake2 with
    ns = t, fhe_bgv_decrypt: the residues modulo t are the message.  (Noise: |t * (e_pk * v + e0 + e1 * s)| < 65537 * (2 * 1024 * 39 * 39
    + 39) < 2^38 for either v, far below q_0 / 2.)"""
    o, logN, n_limbs, batch = oracle, 10, 3, 3
    # q_i = 1 modulo 2N * t, as the reference chooses BGV's moduli: ModReduce then leaves the message unscaled
    M = (2 << logN) * T
    qs = [o.orc_last_prime(60, M), o.orc_last_prime(50, M)]
    qs = np.array(qs + [o.orc_previous_prime(qs[1], M)], np.uint64)
    assert all(o.orc_is_prime(int(q)) and int(q) % M == 1 for q in qs) and len(set(qs.tolist())) == n_limbs
    ctx = fh.Context(backend, logN, qs, roots(o, logN, qs))
    rng = np.random.default_rng(2026)
    N = ctx.N
    try:
        s = ctx.sample("ternary", 1, n_limbs, generator="blake2", key=KEY, counter0=0).SwitchFormat()
        a = ctx.sample("uniform", 1, n_limbs, generator="blake2", key=KEY, counter0=100)
        a.fmt = fh.EVALUATION
        e = ctx.sample("gaussian", 1, n_limbs, generator="blake2", key=KEY, counter0=200).SwitchFormat()
        pk_b = fh.public_key(ctx, s, a, e, T)
        msg = rng.integers(0, T, size=(batch, N), dtype=np.uint64)
        m = ctx.tower(np.repeat(msg[:, None, :], n_limbs, axis=1), fmt=fh.COEFFICIENT).SwitchFormat()
        c0, c1 = fh.encrypt_pk_blake2(ctx, pk_b, a, batch, KEY, 300, 400, msg=m, ns=T, v_dist=v_dist)
        assert np.array_equal(fh.bgv_decrypt(ctx, [c0, c1], s, T), msg)
        # two rows of the three-row key: a plaintext one level down
        m2 = ctx.tower(np.repeat(msg[:, None, :], 2, axis=1), fmt=fh.COEFFICIENT).SwitchFormat()
        c0, c1 = fh.encrypt_pk_blake2(ctx, pk_b, a, batch, KEY, 300, 400, n_limbs=2, msg=m2, ns=T, v_dist=v_dist, contiguous=False)
        s2 = ctx.tower(s.to_host()[:, :2])
        assert np.array_equal(fh.bgv_decrypt(ctx, [c0, c1], s2, T), msg)
        # and the secret-key form
        c0, c1 = fh.encrypt_sk_blake2(ctx, s, batch, KEY, 500, 600, msg=m, ns=T)
        assert np.array_equal(fh.bgv_decrypt(ctx, [c0, c1], s, T), msg)
    finally:
        ctx.close()
