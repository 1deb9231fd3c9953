"""BV evaluation keys on the device (KeySwitchBV::KeySwitchGenInternal, keyswitch-bv.cpp:49-225): the factor table, the secret-key form
(the kernel of fhe_keygen_combine with that table) and the public-key form (keygen_pk_combine_kernel), word for word against expectations
built from the oracle's element-wise members (orc_vec_mul / _neg / _mul_const / _add, orc_automorph_eval_k, orc_ntt_*_tower) and Python
integers:

  secret key   b[key][d][i] = ns * e[key][d][i] - a[key][d][i] * sigma_kNew[key](sNew[i]) + f[d][i] * sigma_kOld[key](sOld[i])   mod q_i
  public key   b[key][d][i] = p0[key][i] * u[key][d][i] + ns * e0[key][d][i] + f[d][i] * sOld[i]
               a[key][d][i] = p1[key][i] * u[key][d][i] + ns * e1[key][d][i]                                                   mod q_i

The shapes are the smallest at which the code can go wrong: N = 2^4 and 2^5 (less than one 16-byte pair per lane), 2^10, 2^12 (two tiles
per row); 1 and 3 keys with different automorphism indices; ns in {1, 65537, 2^40 + 15}; operands at q - 1; in place; one public key and
one per key; enough keys that the tower walk of the public-key kernel is whole and few enough that it is cut, with a short last piece.  A BV table has a non-zero factor in every limb row (limb i's own windows), so no row of sOld can be left out: what the
formula parity shows instead is that sOld never enters a tower at a row whose factor is zero.  A wrapped window of the slabs switches a
tower exactly as the same words uploaded through fhe_bv_key_upload, and the switch is correct up to the derived noise bound; a rotation
key rotates; the seeded forms equal their compositions with the stated launch counts; every error leaves the outputs untouched."""
import ctypes as C
import functools

import numpy as np
import pytest

import libs
from openfhe_amd import fhe_hip as fh
from test_parity_edges import primes_of, roots
from test_parity_keygen import KEY, T_BIG, expect_combine, index_sets, towers

u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)
FHE_ERR_ARG, FHE_ERR_UNSUPPORTED = 1, 4


@functools.lru_cache(maxsize=None)
def chain(logN, bits):
    """distinct primes of the given sizes, = 1 mod 2N, with their roots; read-only"""
    o = libs.load_oracle()
    q = []
    for b in bits:
        q.append(primes_of(o, logN, b, 1, avoid=q)[0])
    q = np.array(q, np.uint64)
    assert tuple(int(v).bit_length() for v in q) == tuple(bits)
    psi = roots(o, logN, q)
    q.setflags(write=False), psi.setflags(write=False)
    return q, psi


def factors(q, r):
    """the table with python integers, written out here once more (not through the library's own helper)"""
    rows = []
    for i, qi in enumerate(int(v) for v in q):
        for k in range(1 if r == 0 else -(-qi.bit_length() // r)):
            rows.append([pow(2, r * k, qi) if j == i else 0 for j in range(len(q))])
    return np.array(rows, np.uint64)


# ---- 1. the factor table --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,r,per_limb", [((60, 60, 60), 0, (1, 1, 1)), ((60, 60, 60), 10, (6, 6, 6)), ((60, 50, 51), 10, (6, 5, 6)),
                                              ((60, 60, 60), 31, (2, 2, 2)), ((60, 25, 50), 10, (6, 3, 5)), ((60, 25, 50), 0, (1, 1, 1))])
def test_factor_table(backend, bits, r, per_limb):
    q, psi = chain(4, bits)
    ctx = fh.Context(backend, 4, q, psi)
    L = backend.L
    try:
        want = factors(q, r)
        D0 = L.fhe_bv_keygen_factors(ctx.h, 3, r, None)
        assert D0 == sum(per_limb) == len(want) == L.fhe_crt_decompose_towers(ctx.h, None, 3, r)
        got = np.full((D0, 3), 77, np.uint64)
        assert L.fhe_bv_keygen_factors(ctx.h, 3, r, got.ctypes.data_as(u64p)) == D0
        assert np.array_equal(got, want)
        assert np.array_equal(np.array(fh.bv_keygen_factors(q, r), np.uint64), want)
        for d in range(D0):  # one non-zero entry per tower, at the tower's own limb, limb after limb
            assert np.count_nonzero(got[d]) == 1 and np.nonzero(got[d])[0][0] == np.searchsorted(np.cumsum(per_limb), d, side="right")
        # a level below: the first D_l towers, their first sizeQl columns
        Dl = L.fhe_bv_keygen_factors(ctx.h, 2, r, None)
        low = np.zeros((Dl, 2), np.uint64)
        assert Dl == sum(per_limb[:2]) and L.fhe_bv_keygen_factors(ctx.h, 2, r, low.ctypes.data_as(u64p)) == Dl
        assert np.array_equal(low, want[:Dl, :2])
    finally:
        ctx.close()


def test_digit_size_32_is_unsupported(backend):
    q, psi = chain(4, (60, 60, 60))
    ctx = fh.Context(backend, 4, q, psi)
    L = backend.L
    try:
        assert L.fhe_crt_decompose_towers(ctx.h, None, 3, 32) == 0 and L.fhe_bv_keygen_factors(ctx.h, 3, 32, None) == 0
        assert L.fhe_bv_keygen_workspace_bytes(ctx.h, 3, 32, 1) == 0
        n0, ne = C.c_uint64(), C.c_uint64()
        assert L.fhe_bv_keygen_counters(ctx.h, 3, 32, 1, 0, C.byref(n0), C.byref(ne)) == FHE_ERR_UNSUPPORTED
        assert "digit size" in L.fhe_last_error().decode()
    finally:
        ctx.close()


# ---- 2. the secret-key form ------------------------------------------------------------------------------------------------------------
# (logN, limb sizes, digit size): 17 towers with different window counts per limb; the chain with a limb below ns; two tiles per row
SK_SHAPES = [(4, (60, 50, 51), 10), (5, (60, 25, 50), 20), (10, (60, 50, 51), 20), (12, (60, 60, 60), 0)]


@pytest.mark.parametrize("logN,bits,r", SK_SHAPES)
def test_secret_key_form_matches_the_formula(backend, oracle, logN, bits, r):
    q, psi = chain(logN, bits)
    ctx = fh.Context(backend, logN, q, psi)
    N, f = 1 << logN, factors(q, r)
    D0 = len(f)
    rng = np.random.default_rng(300 + logN)
    try:
        for K, ns, top in ((1, 1, False), (3, 65537, False), (3, T_BIG, True), (1, T_BIG, False)):
            k_new, k_old = index_sets(N, K)
            a, e = towers(rng, q, N, K * D0, top), towers(rng, q, N, K * D0, top)
            s_new, s_old = towers(rng, q, N, 1, top), towers(rng, q, N, 1, top)
            want = expect_combine(oracle, q, N, a, e, s_new[0], k_new, s_old[0], k_old, f, ns)
            ta, te, tsn, tso = ctx.tower(a), ctx.tower(e), ctx.tower(s_new), ctx.tower(s_old)
            b, _, keys = fh.BvKey.keygen(ctx, r, tsn, tso, ta, te, K, k_new, k_old, ns=ns)
            assert np.array_equal(b.to_host(), want), f"K={K} ns={ns} top={top}"
            assert np.array_equal(te.to_host(), e) and np.array_equal(ta.to_host(), a), "operands modified"
            assert np.array_equal(tsn.to_host(), s_new) and np.array_equal(tso.to_host(), s_old), "secrets modified"
            assert len(keys) == K and all(k.digits(3) == D0 for k in keys)
            for k in keys:
                k.close()
            b2, _, keys = fh.BvKey.keygen(ctx, r, tsn, tso, ta, te, K, k_new, k_old, ns=ns, in_place=True)
            assert b2 is te and np.array_equal(te.to_host(), want), f"in place: K={K} ns={ns} top={top}"
            for k in keys:
                k.close()
    finally:
        ctx.close()


# ---- 3. the public-key form ------------------------------------------------------------------------------------------------------------
def expect_pk(o, qs, N, p0, p1, s_old, u, e0, e1, factor, ns, K):
    """u, e0, e1 [K * D0][L][N]; p0, p1 [1 or K][L][N]; s_old [L][N]; factor [D0][L]"""
    D0 = u.shape[0] // K
    b, a = np.empty_like(u), np.empty_like(u)
    t, w = np.empty(N, np.uint64), np.empty(N, np.uint64)
    for key in range(K):
        pk = key if p0.shape[0] > 1 else 0
        for i, q in enumerate(int(v) for v in qs):
            for d in range(D0):
                x = key * D0 + d
                for out, p, e in ((b, p0, e0), (a, p1, e1)):
                    o.orc_vec_mul(t, np.ascontiguousarray(p[pk, i]), np.ascontiguousarray(u[x, i]), N, q)
                    o.orc_vec_mul_const(w, np.ascontiguousarray(e[x, i]), ns % q, N, q)
                    o.orc_vec_add(t, t.copy(), w, N, q)
                    if out is b and int(factor[d][i]):
                        o.orc_vec_mul_const(w, np.ascontiguousarray(s_old[i]), int(factor[d][i]), N, q)
                        o.orc_vec_add(t, t.copy(), w, N, q)
                    out[x, i] = t
    return b, a


# The tower walk is cut into pieces when keys x rows x tiles alone leave fewer than four workgroups per compute unit (1024 on a device of
# 256 compute units, 12 on the lane emulator, which reports 3).  The last three shapes: 512 keys of 2 limbs and 2 towers, 1024 workgroups,
# so that the walk is whole on the device too; one key of two limbs with 11 towers: pieces of two towers and a last one of one on the
# emulator, of one tower each on the device; 25 keys of 17 towers, 75 workgroups: the walk is whole on the emulator, on the device 9
# pieces of two towers, the last of one
PK_SHAPES = [(4, (60, 50, 51), 10, (1, 3)), (5, (60, 25, 50), 20, (1, 3)), (10, (60, 50, 51), 20, (1, 3)), (12, (60, 60, 60), 0, (1, 3)),
             (4, (60, 50), 0, (512,)), (5, (60, 50), 10, (1,)), (4, (60, 50, 51), 10, (25,))]


@pytest.mark.parametrize("logN,bits,r,key_counts", PK_SHAPES)
def test_public_key_form_matches_the_formula(backend, oracle, logN, bits, r, key_counts):
    q, psi = chain(logN, bits)
    ctx = fh.Context(backend, logN, q, psi)
    N, f = 1 << logN, factors(q, r)
    D0 = len(f)
    rng = np.random.default_rng(400 + logN)
    try:
        for n, K in enumerate(key_counts):
            for ns, top, per_key in ((1, False, False), (65537, False, True), (T_BIG, True, True), (T_BIG, False, False))[n:]:
                u, e0, e1 = (towers(rng, q, N, K * D0, top) for _ in range(3))
                p0, p1 = (towers(rng, q, N, K if per_key else 1, top) for _ in range(2))
                s_old = towers(rng, q, N, 1, top)
                wb, wa = expect_pk(oracle, q, N, p0, p1, s_old[0], u, e0, e1, f, ns, K)
                tu, t0, t1, tp0, tp1, ts = (ctx.tower(x) for x in (u, e0, e1, p0, p1, s_old))
                b, a, keys = fh.BvKey.keygen_pk(ctx, r, tp0, tp1, ts, tu, t0, t1, K, ns=ns)
                what = f"K={K} ns={ns} top={top} per_key={per_key}"
                assert np.array_equal(b.to_host(), wb), "b: " + what
                assert np.array_equal(a.to_host(), wa), "a: " + what
                for t, x in ((tu, u), (t0, e0), (t1, e1), (tp0, p0), (tp1, p1), (ts, s_old)):
                    assert np.array_equal(t.to_host(), x), "operands modified: " + what
                assert len(keys) == K
                for k in keys:
                    k.close()
                b2, a2, keys = fh.BvKey.keygen_pk(ctx, r, tp0, tp1, ts, tu, t0, t1, K, ns=ns, in_place=True)
                assert b2 is t0 and a2 is t1 and np.array_equal(t0.to_host(), wb) and np.array_equal(t1.to_host(), wa), "in place: " + what
                for k in keys:
                    k.close()
    finally:
        ctx.close()


# ---- 4. a wrapped window switches, 5. a rotation key rotates ---------------------------------------------------------------------------
def small_eval(o, octx, rng, q, N, batch, bound):
    """towers of integer polynomials with coefficients in [-bound, bound], EVALUATION; also the integers"""
    ints = rng.integers(-bound, bound + 1, size=(batch, N))
    x = np.stack([np.stack([(ints[b] % int(v)).astype(np.uint64) for v in q]) for b in range(batch)])
    o.orc_ntt_fwd_tower(octx, x, None, len(q), batch, 1)
    return x, ints


def centred(o, octx, x, q):
    """the integer polynomial of one EVALUATION tower x [L][N] over Q = prod q, centred"""
    c = np.ascontiguousarray(x[None].copy())
    o.orc_ntt_inv_tower(octx, c, None, len(q), 1, 1)
    Q = 1
    for v in q:
        Q *= int(v)
    acc = np.zeros(x.shape[1], object)
    for i, v in enumerate(int(v) for v in q):
        Qi = Q // v
        acc = (acc + c[0, i].astype(object) * (Qi * pow(Qi, -1, v))) % Q
    return np.array([int(v) - Q if int(v) > Q // 2 else int(v) for v in acc], object)


def mul_rows(o, a, b, q, N):
    out = np.empty_like(a)
    for i, v in enumerate(int(v) for v in q):
        o.orc_vec_mul(out[i], np.ascontiguousarray(a[i]), np.ascontiguousarray(b[i]), N, v)
    return out


def add_rows(o, a, b, q, N, sub=False):
    out = np.empty_like(a)
    for i, v in enumerate(int(v) for v in q):
        (o.orc_vec_sub if sub else o.orc_vec_add)(out[i], np.ascontiguousarray(a[i]), np.ascontiguousarray(b[i]), N, v)
    return out


@pytest.mark.parametrize("logN,r", [(12, 0), (5, 0), (5, 20)])
def test_a_wrapped_window_switches(backend, oracle, logN, r):
    """window 1 of a two-key set: the same words as an uploaded key, at the full level and one below; and the switch is correct:
    o0 + o1 * sNew - c * sOld = ns * sum_d digit_d * e_d, whose coefficients are below ns * D_l * N * W * max|e|"""
    o = oracle
    q, psi = chain(logN, (60, 60, 60))
    ctx = fh.Context(backend, logN, q, psi)
    N, f, ns, K, E = 1 << logN, factors(q, r), 65537, 2, 8
    D0 = len(f)
    rng = np.random.default_rng(500 + logN + r)
    octx = o.orc_ctx_create(N, 3, q, psi)
    try:
        a = towers(rng, q, N, K * D0)
        e, _ = small_eval(o, octx, rng, q, N, K * D0, E)
        (s_new, s_old), _ = small_eval(o, octx, rng, q, N, 2, 1)
        b, ta, keys = fh.BvKey.keygen(ctx, r, ctx.tower(s_new), ctx.tower(s_old), ctx.tower(a), ctx.tower(e), K, [5, 1], [25, 1], ns=ns)
        hb, ha = b.to_host(), ta.to_host()
        up = fh.BvKey(ctx, 3, r, hb[D0:], ha[D0:])
        for sizeQl in (3, 2):
            ql = q[:sizeQl]
            Dl = keys[1].digits(sizeQl)
            lctx = o.orc_ctx_create(N, sizeQl, np.ascontiguousarray(ql), np.ascontiguousarray(psi[:sizeQl]))
            c = towers(rng, ql, N, 1)
            o0, o1 = keys[1].KeySwitchCore(ctx.tower(c))
            w0, w1 = up.KeySwitchCore(ctx.tower(c))
            g0, g1 = o0.to_host()[0], o1.to_host()[0]
            assert np.array_equal(g0, w0.to_host()[0]) and np.array_equal(g1, w1.to_host()[0]), f"sizeQl={sizeQl}"
            left = add_rows(o, g0, mul_rows(o, g1, s_new[:sizeQl], ql, N), ql, N)
            noise = centred(o, lctx, add_rows(o, left, mul_rows(o, c[0], s_old[:sizeQl], ql, N), ql, N, sub=True), ql)
            W = (1 << r) if r else max(int(v) for v in ql)
            worst = max(abs(int(v)) for v in noise)
            assert 0 < worst <= ns * Dl * N * W * E, (sizeQl, worst)
            o.orc_ctx_destroy(lctx)
        up.close()
        for k in keys:
            k.close()
    finally:
        o.orc_ctx_destroy(octx)
        ctx.close()


@pytest.mark.parametrize("logN,r", [(5, 0), (10, 20)])
def test_a_rotation_key_rotates(backend, oracle, logN, r):
    """kNew = k^-1, kOld = 1: fhe_bv_eval_automorphism on (c0, c1) with c0 + c1 * s = m gives o0 + o1 * s = sigma_k(m) up to the bound"""
    o = oracle
    q, psi = chain(logN, (60, 60, 60))
    ctx = fh.Context(backend, logN, q, psi)
    N, f, E = 1 << logN, factors(q, r), 8
    D0 = len(f)
    rng = np.random.default_rng(600 + logN)
    octx = o.orc_ctx_create(N, 3, q, psi)
    try:
        k = 5
        k_inv = pow(k, -1, 2 * N)
        a = towers(rng, q, N, D0)
        e, _ = small_eval(o, octx, rng, q, N, D0, E)
        (s,), _ = small_eval(o, octx, rng, q, N, 1, 1)
        ts = ctx.tower(s)
        _, _, keys = fh.BvKey.keygen(ctx, r, ts, ts, ctx.tower(a), ctx.tower(e), 1, [k_inv], [1])
        m, c1 = towers(rng, q, N, 1)[0], towers(rng, q, N, 1)[0]
        c0 = add_rows(o, m, mul_rows(o, c1, s, q, N), q, N, sub=True)
        o0, o1 = keys[0].Automorphism(ctx.tower(c0), ctx.tower(c1), k)
        got = add_rows(o, o0.to_host()[0], mul_rows(o, o1.to_host()[0], s, q, N), q, N)
        want = np.empty_like(m)
        for i in range(3):
            o.orc_automorph_eval_k(want[i], np.ascontiguousarray(m[i]), N, k)
        noise = centred(o, octx, add_rows(o, got, want, q, N, sub=True), q)
        W = (1 << r) if r else max(int(v) for v in q)
        assert max(abs(int(v)) for v in noise) <= D0 * N * W * E
        keys[0].close()
    finally:
        o.orc_ctx_destroy(octx)
        ctx.close()


# ---- 6. the seeded forms ---------------------------------------------------------------------------------------------------------------
def launches(lib):
    total = C.c_uint64()
    lib.L.fhe_launch_stats(None, 0, C.byref(total))
    return total.value


@pytest.mark.parametrize("logN,sizeQ,r,K,five", [(13, 2, 0, 1, True), (10, 3, 20, 2, False)])
def test_seeded_forms_are_their_compositions(backend, oracle, logN, sizeQ, r, K, five):
    q, psi = chain(logN, (60, 50, 51)[:sizeQ])
    ctx = fh.Context(backend, logN, q, psi)
    N, ns, sigma = 1 << logN, 65537, 3.19
    D0 = len(factors(q, r))
    T = K * D0
    rng = np.random.default_rng(700 + logN)
    k_new, k_old = index_sets(N, K) if K == 1 else ([5, 2 * N - 1], [1, 25])
    try:
        tsn, tso = ctx.tower(towers(rng, q, N, 1)), ctx.tower(towers(rng, q, N, 1))
        p0, p1 = ctx.tower(towers(rng, q, N, K)), ctx.tower(towers(rng, q, N, K))
        # secret-key form
        na, ne = fh.bv_keygen_counters(ctx, sizeQ, r, K)
        assert na == -(-2 * T * sizeQ * N // 512) and ne == -(-T * N // 512)
        ca, ce = 11, 11 + na
        a = ctx.sample("uniform", T, sizeQ, generator="blake2", key=KEY, counter0=ca)
        a.fmt = fh.EVALUATION  # used as drawn
        e = ctx.sample("gaussian", T, sizeQ, sigma=sigma, generator="blake2", key=KEY, counter0=ce).SwitchFormat()
        ctx.sync()
        t0 = launches(backend)
        wb, wa, keys = fh.BvKey.keygen(ctx, r, tsn, tso, a, e, K, k_new, k_old, ns=ns)
        ctx.sync()
        one_combine = launches(backend) - t0
        t0 = launches(backend)
        a2 = ctx.sample("uniform", T, sizeQ, generator="blake2", key=KEY, counter0=ca)
        e2 = ctx.sample("gaussian", T, sizeQ, sigma=sigma, generator="blake2", key=KEY, counter0=ce).SwitchFormat()
        ctx.sync()
        composed = launches(backend) - t0 + one_combine
        t0 = launches(backend)
        b, a3, keys2 = fh.BvKey.keygen_blake2(ctx, r, tsn, tso, K, KEY, ca, ce, k_new, k_old, ns=ns, sigma=sigma)
        ctx.sync()
        spent = launches(backend) - t0
        assert one_combine == 1 and spent == composed and (not five or spent == 5), (spent, composed)
        assert np.array_equal(a3.to_host(), wa.to_host()) and np.array_equal(b.to_host(), wb.to_host())
        # the counters give the first unused ones: a second call from them regenerates a with the uniform sampler alone
        b4, a4, keys4 = fh.BvKey.keygen_blake2(ctx, r, tsn, tso, K, KEY, ca + na + ne, ca + 2 * na + ne, k_new, k_old, ns=ns, sigma=sigma)
        again = ctx.sample("uniform", T, sizeQ, generator="blake2", key=KEY, counter0=ca + na + ne)
        assert np.array_equal(a4.to_host(), again.to_host()) and not np.array_equal(a4.to_host(), a3.to_host())
        for k in keys + keys2 + keys4:
            k.close()
        # public-key form: u from cu, e0 from ce, e1 from the block after e0's last
        nu, ne2 = fh.bv_keygen_counters(ctx, sizeQ, r, K, fh.PUBLIC_KEY_FORM)
        assert nu == -(-T * N // 512) and ne2 == 2 * nu
        cu, ce = 5, 5 + nu
        u = ctx.sample("ternary", T, sizeQ, generator="blake2", key=KEY, counter0=cu).SwitchFormat()
        e0 = ctx.sample("gaussian", T, sizeQ, sigma=sigma, generator="blake2", key=KEY, counter0=ce).SwitchFormat()
        e1 = ctx.sample("gaussian", T, sizeQ, sigma=sigma, generator="blake2", key=KEY, counter0=ce + ne2 // 2).SwitchFormat()
        ctx.sync()
        t0 = launches(backend)
        wb, wa, keys = fh.BvKey.keygen_pk(ctx, r, p0, p1, tso, u, e0, e1, K, ns=ns)
        ctx.sync()
        one_combine = launches(backend) - t0
        t0 = launches(backend)
        ctx.sample("gaussian", 2 * T, sizeQ, sigma=sigma, generator="blake2", key=KEY, counter0=ce)
        ctx.sample("ternary", T, sizeQ, generator="blake2", key=KEY, counter0=cu)
        ctx.sample("gaussian", 3 * T, sizeQ, sigma=sigma, generator="blake2", key=KEY, counter0=ce).SwitchFormat()
        ctx.sync()
        composed = launches(backend) - t0 - 1 + one_combine  # (the third sample only feeds the one transform call over 3 T towers)
        t0 = launches(backend)
        b, a5, keys2 = fh.BvKey.keygen_pk_blake2(ctx, r, p0, p1, tso, K, KEY, cu, ce, ns=ns, sigma=sigma)
        spent = launches(backend) - t0
        assert one_combine == 1 and spent == composed and (not five or spent == 5), (spent, composed)
        assert np.array_equal(b.to_host(), wb.to_host()) and np.array_equal(a5.to_host(), wa.to_host()), "contiguous"
        b6, a6, keys3 = fh.BvKey.keygen_pk_blake2(ctx, r, p0, p1, tso, K, KEY, cu, ce, ns=ns, sigma=sigma, contiguous=False)
        assert np.array_equal(b6.to_host(), wb.to_host()) and np.array_equal(a6.to_host(), wa.to_host()), "scattered"
        for k in keys + keys2 + keys3:
            k.close()
    finally:
        ctx.close()


def test_seeded_public_key_form_on_a_ring_below_one_block(backend):
    """N = 2^4 with 3 towers: 48 coefficients per error block, e1 starts at the next blake2 block whether the buffers touch or not"""
    q, psi = chain(4, (60, 50, 51))
    ctx = fh.Context(backend, 4, q, psi)
    rng = np.random.default_rng(44)
    try:
        ts, p0, p1 = (ctx.tower(towers(rng, q, 16, 1)) for _ in range(3))
        u = ctx.sample("gaussian", 3, 3, sigma=3.19, generator="blake2", key=KEY, counter0=9).SwitchFormat()
        e0 = ctx.sample("gaussian", 3, 3, sigma=3.19, generator="blake2", key=KEY, counter0=20).SwitchFormat()
        e1 = ctx.sample("gaussian", 3, 3, sigma=3.19, generator="blake2", key=KEY, counter0=21).SwitchFormat()
        assert fh.bv_keygen_counters(ctx, 3, 0, 1, fh.PUBLIC_KEY_FORM) == (1, 2)
        wb, wa, keys = fh.BvKey.keygen_pk(ctx, 0, p0, p1, ts, u, e0, e1, 1, ns=3)
        for contiguous in (True, False):
            b, a, more = fh.BvKey.keygen_pk_blake2(ctx, 0, p0, p1, ts, 1, KEY, 9, 20, ns=3, u_dist=fh.GAUSSIAN, contiguous=contiguous)
            assert np.array_equal(b.to_host(), wb.to_host()) and np.array_equal(a.to_host(), wa.to_host()), contiguous
            keys += more
        for k in keys:
            k.close()
    finally:
        ctx.close()


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_untouched(backend):
    logN, r, K = 5, 20, 2
    q, psi = chain(logN, (60, 50, 51))
    ctx = fh.Context(backend, logN, q, psi)
    L, N = backend.L, 1 << logN
    D0 = len(factors(q, r))
    words = K * D0 * 3 * N
    rng = np.random.default_rng(55)
    try:
        # a | e (e0) | e1 | b | outA | ws | spare, contiguous; then the keys: sNew | sOld | p0 [K] | p1 [K]
        buf = ctx.upload(rng.integers(0, 1 << 20, size=7 * words + (2 + 2 * K) * 3 * N, dtype=np.uint64))
        total = 7 * words + (2 + 2 * K) * 3 * N
        before = ctx.download(buf, (total,))
        at = lambda w: C.c_void_p(buf.value + 8 * w)
        a, e0, e1, ob, oa, ws = (at(i * words) for i in range(6))
        sn, so, p0, p1 = at(7 * words), at(7 * words + 3 * N), at(7 * words + 6 * N), at(7 * words + (6 + 3 * K) * N)
        ks = lambda *v: np.array(v, np.uint32).ctypes.data_as(u32p)
        key = np.frombuffer(KEY, dtype="<u4").astype(np.uint32).ctypes.data_as(u32p)
        wsb = L.fhe_bv_keygen_workspace_bytes(ctx.h, 3, r, K)
        assert wsb == 8 * words

        def sk(sizeQ=3, r=r, nKeys=K, kNew=None, kOld=None, sNew=sn, sOld=so, ns=1, a=a, e=e0, out=ob):
            return L.fhe_bv_keygen(ctx.h, sizeQ, r, nKeys, kNew, kOld, sNew, sOld, ns, a, e, out, None)

        def sk_seeded(sizeQ=3, r=r, nKeys=K, kNew=None, sNew=sn, sOld=so, ns=1, sigma=3.19, key=key, b=ob, a=oa):
            return L.fhe_bv_keygen_blake2(ctx.h, sizeQ, r, nKeys, kNew, None, sNew, sOld, ns, sigma, key, 0, 1 << 20, b, a, None)

        def pk(sizeQ=3, r=r, nKeys=K, p0=p0, p1=p1, per_key=1, sOld=so, ns=1, u=a, e0=e0, e1=e1, b=ob, a=oa):
            return L.fhe_bv_keygen_pk(ctx.h, sizeQ, r, nKeys, p0, p1, per_key, sOld, ns, u, e0, e1, b, a, None)

        def pk_seeded(sizeQ=3, r=r, nKeys=K, p0=p0, p1=p1, sOld=so, uDist=0, ns=1, sigma=3.19, key=key, b=ob, a=oa, ws=ws, wsb=wsb):
            return L.fhe_bv_keygen_pk_blake2(ctx.h, sizeQ, r, nKeys, p0, p1, 1, sOld, uDist, ns, sigma, key, 0, 1 << 20, b, a, ws, wsb, None)

        n0, ne = C.c_uint64(), C.c_uint64()
        counters = lambda **kw: L.fhe_bv_keygen_counters(ctx.h, kw.get("sizeQ", 3), kw.get("r", r), kw.get("nKeys", K), kw.get("form", 0),
                                                         C.byref(n0), C.byref(ne))
        cases = {
            "sk: nKeys == 0": (lambda: sk(nKeys=0), "nKeys"),
            "sk: even index": (lambda: sk(kNew=ks(1, 4)), "Automorphism index not odd"),
            "sk: even old index": (lambda: sk(kOld=ks(2, 1)), "Automorphism index not odd"),
            "sk: index 2N + 1": (lambda: sk(kNew=ks(2 * N + 1, 1)), "out of range"),
            "sk: null a": (lambda: sk(a=None), "null"),
            "sk: null e": (lambda: sk(e=None), "null"),
            "sk: null sNew": (lambda: sk(sNew=None), "null"),
            "sk: null sOld": (lambda: sk(sOld=None), "null"),
            "sk: null out": (lambda: sk(out=None), "null"),
            "sk: ns == 0": (lambda: sk(ns=0), "noise scale"),
            "sk: sizeQ == 0": (lambda: sk(sizeQ=0), "sizeQ"),
            "sk: sizeQ == 4": (lambda: sk(sizeQ=4), "sizeQ"),
            "sk: out over a": (lambda: sk(out=at(N)), "overlap"),
            "sk: out half over e": (lambda: sk(out=at(words + N)), "overlap"),
            "sk: out over sOld": (lambda: sk(sOld=at(4 * words - N)), "overlap"),
            "sk seeded: nKeys == 0": (lambda: sk_seeded(nKeys=0), "nKeys"),
            "sk seeded: even index": (lambda: sk_seeded(kNew=ks(3, 2)), "Automorphism index not odd"),
            "sk seeded: sigma 0.5": (lambda: sk_seeded(sigma=0.5), "sigma"),
            "sk seeded: sigma 300": (lambda: sk_seeded(sigma=300.0), "sigma"),
            "sk seeded: ns == 0": (lambda: sk_seeded(ns=0), "noise scale"),
            "sk seeded: null key": (lambda: sk_seeded(key=None), "null"),
            "sk seeded: sizeQ == 4": (lambda: sk_seeded(sizeQ=4), "sizeQ"),
            "sk seeded: b over a": (lambda: sk_seeded(b=at(4 * words + N)), "overlap"),
            "sk seeded: a over sNew": (lambda: sk_seeded(sNew=at(5 * words - N)), "overlap"),
            "pk: nKeys == 0": (lambda: pk(nKeys=0), "nKeys"),
            "pk: null p0": (lambda: pk(p0=None), "null"),
            "pk: null p1": (lambda: pk(p1=None), "null"),
            "pk: null sOld": (lambda: pk(sOld=None), "null"),
            "pk: null u": (lambda: pk(u=None), "null"),
            "pk: null e0": (lambda: pk(e0=None), "null"),
            "pk: null e1": (lambda: pk(e1=None), "null"),
            "pk: null b": (lambda: pk(b=None), "null"),
            "pk: null a": (lambda: pk(a=None), "null"),
            "pk: ns == 0": (lambda: pk(ns=0), "noise scale"),
            "pk: sizeQ == 0": (lambda: pk(sizeQ=0), "sizeQ"),
            "pk: sizeQ == 4": (lambda: pk(sizeQ=4), "sizeQ"),
            "pk: b over a": (lambda: pk(a=at(3 * words + N)), "overlap"),
            "pk: b half over e0": (lambda: pk(b=at(words + N), a=at(5 * words)), "overlap"),
            "pk: a half over e1": (lambda: pk(a=at(2 * words + N), b=at(5 * words)), "overlap"),
            "pk: b is e1": (lambda: pk(b=e1, a=at(5 * words)), "overlap"),
            "pk: a is e0": (lambda: pk(a=e0), "overlap"),
            "pk: b over u": (lambda: pk(b=at(N), a=at(5 * words)), "overlap"),
            "pk: a over the public key": (lambda: pk(p1=at(5 * words - N)), "overlap"),
            "pk: b over the second public key": (lambda: pk(p0=at(3 * words - 4 * N)), "overlap"),
            "pk: b over sOld": (lambda: pk(sOld=at(4 * words - N)), "overlap"),
            "pk seeded: nKeys == 0": (lambda: pk_seeded(nKeys=0), "nKeys"),
            "pk seeded: sigma 1": (lambda: pk_seeded(sigma=1.0), "sigma"),
            "pk seeded: sigma 300": (lambda: pk_seeded(sigma=300.0), "sigma"),
            "pk seeded: uDist 2": (lambda: pk_seeded(uDist=2), "uDist"),
            "pk seeded: ns == 0": (lambda: pk_seeded(ns=0), "noise scale"),
            "pk seeded: null key": (lambda: pk_seeded(key=None), "null"),
            "pk seeded: null ws": (lambda: pk_seeded(ws=None), "null"),
            "pk seeded: null b": (lambda: pk_seeded(b=None), "null"),
            "pk seeded: sizeQ == 4": (lambda: pk_seeded(sizeQ=4), "sizeQ"),
            "pk seeded: short workspace": (lambda: pk_seeded(wsb=wsb - 8), "workspace too small"),
            "pk seeded: ws over b": (lambda: pk_seeded(ws=at(4 * words - N)), "workspace overlaps a key block"),
            "pk seeded: ws over a": (lambda: pk_seeded(ws=at(4 * words + N)), "workspace overlaps a key block"),
            "pk seeded: ws over the public key": (lambda: pk_seeded(p0=at(6 * words - N)), "workspace overlaps the public key"),
            "pk seeded: ws over sOld": (lambda: pk_seeded(sOld=at(5 * words + N)), "workspace overlaps the public key or sOld"),
            "pk seeded: b over a": (lambda: pk_seeded(a=at(3 * words + N)), "overlap"),
            "counters: nKeys == 0": (lambda: counters(nKeys=0), "nKeys"),
            "counters: form 2": (lambda: counters(form=2), "form"),
            "counters: sizeQ == 4": (lambda: counters(sizeQ=4), "sizeQ"),
        }
        for name, (call, text) in cases.items():
            assert call() == FHE_ERR_ARG, f"{name}: FHE_ERR_ARG expected"
            assert text in L.fhe_last_error().decode(), (name, L.fhe_last_error().decode())
        for name, call in (("sk", lambda: sk(r=32)), ("sk seeded", lambda: sk_seeded(r=32)), ("pk", lambda: pk(r=32)),
                           ("pk seeded", lambda: pk_seeded(r=32)), ("counters", lambda: counters(r=32))):
            assert call() == FHE_ERR_UNSUPPORTED, f"{name}: FHE_ERR_UNSUPPORTED expected for a 32-bit digit"
            assert "digit size" in L.fhe_last_error().decode(), name
        ctx.sync()
        assert np.array_equal(ctx.download(buf, (total,)), before), "device memory changed"
        # ... and the same arguments without the fault run, in place as well
        assert sk(kNew=ks(5, 2 * N - 1)) == 0 and sk(out=e0) == 0 and sk_seeded() == 0
        assert pk() == 0 and pk(b=e0, a=e1) == 0 and pk_seeded() == 0 and counters() == 0 and counters(form=1) == 0
        ctx.sync()
    finally:
        ctx.close()
