"""Key generation on the device: keygen_combine_kernel and the entry points on it, word for word against expectations built from the
oracle's element-wise members (orc_vec_mul / _neg / _mul_const / _add, orc_automorph_eval_k, orc_switch_modulus, orc_ntt_*_tower).

  out[key][j][i] = ns * e[key][j][i] - a[key][j][i] * sigma_kNew[key](sNew[i]) + f[j][i] * sigma_kOld[key](sOld[i])   mod q_i

The shapes are the smallest at which the kernel can go wrong: N = 2^4 and 2^5 (a workgroup holds less than one 16-byte pair per lane,
most lanes idle), N = 2^10 (two pairs per lane), N = 2^12 (two tiles per row, emulator and GPU alike); digit partitions with a short last
digit, one limb per digit and a single digit; 1 and 3 keys with different automorphism indices per key; the 60/25/50-bit chain with a noise
scale above its 25-bit limb; operands at q - 1; in place; a limb subset; no sOld term (the public key); every error with the output
untouched; the secret's extension; the seeded form against its composition, with the launch counts."""
import ctypes as C

import numpy as np
import pytest

import libs
from openfhe_amd import fhe_hip as fh
from test_parity import ckks_like_params
from test_parity_edges import primes_of, roots

u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)
T_BIG = (1 << 40) + 15  # above the 25-bit limb of the mixed chain
SHAPES = [(3, 2, 2), (4, 1, 4), (3, 3, 1)]  # (sizeQ, sizeP, dnum): a short last digit, one limb per digit, one digit
KEY = bytes(range(64))


def permuted(o, row, k, N):
    if k == 1:
        return row
    out = np.empty_like(row)
    o.orc_automorph_eval_k(out, np.ascontiguousarray(row), N, k)
    return out


def expect_combine(o, qs, N, a, e, s_new, k_new, s_old, k_old, factor, ns):
    """a, e [K * nParts][L][N]; s_new [L][N]; s_old [>= rows with a factor][N] or None; factor [nParts][L] or None"""
    K, L = len(k_new), len(qs)
    nP = a.shape[0] // K
    out = np.empty_like(a)
    t, u = np.empty(N, np.uint64), np.empty(N, np.uint64)
    for key in range(K):
        for i, q in enumerate(int(v) for v in qs):
            sn = permuted(o, s_new[i], int(k_new[key]), N)
            so = permuted(o, s_old[i], int(k_old[key]), N) if factor is not None and i < len(s_old) else None
            for j in range(nP):
                b = key * nP + j
                o.orc_vec_mul(t, np.ascontiguousarray(a[b, i]), sn, N, q)
                o.orc_vec_neg(t, t.copy(), N, q)
                o.orc_vec_mul_const(u, np.ascontiguousarray(e[b, i]), ns % q, N, q)
                o.orc_vec_add(t, t.copy(), u, N, q)
                f = int(factor[j][i]) % q if factor is not None else 0
                if f:
                    o.orc_vec_mul_const(u, so, f, N, q)
                    o.orc_vec_add(t, t.copy(), u, N, q)
                out[b, i] = t
    return out


def hybrid_factors(qs, sizeQ, sizeP, dnum):
    """[P]_{q_i} on the limbs of digit j, 0 elsewhere (keyswitch-hybrid.cpp:105-119), with python integers"""
    alpha = -(-sizeQ // dnum)
    P = 1
    for v in qs[sizeQ:]:
        P *= int(v)
    f = np.zeros((dnum, sizeQ + sizeP), np.uint64)
    for j in range(dnum):
        for i in range(alpha * j, min(alpha * (j + 1), sizeQ)):
            f[j, i] = P % int(qs[i])
    return f


def towers(rng, qs, N, batch, top=False):
    if top:
        return np.broadcast_to((qs - np.uint64(1))[None, :, None], (batch, len(qs), N)).copy()
    return libs.rand_tower(rng, qs, N, batch)


class Hybrid:
    def __init__(self, backend, o, logN, shape):
        sizeQ, sizeP, dnum = shape
        q, psiQ, p, psiP = ckks_like_params(o, logN, sizeQ, dnum)
        assert len(p) == sizeP, (shape, len(p))
        self.logN, self.N, self.sizeQ, self.sizeP, self.dnum = logN, 1 << logN, sizeQ, sizeP, dnum
        self.qs, self.psi = np.concatenate([q, p]), np.concatenate([psiQ, psiP])
        self.ctx = fh.Context(backend, logN, self.qs, self.psi)
        self.plan = fh.KeySwitchPlan(self.ctx, sizeQ, sizeP, dnum)
        self.f = hybrid_factors(self.qs, sizeQ, sizeP, dnum)

    def close(self):
        self.plan.close()
        self.ctx.close()


def index_sets(N, K):
    """automorphism indices from {1, 5, 25, 2N - 1}: different per key, and kNew != kOld in every key"""
    return ([25], [2 * N - 1]) if K == 1 else ([5, 1, 2 * N - 1], [1, 25, 5])


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("logN", [4, 5, 10])
def test_hybrid_keygen_matches_the_formula(backend, oracle, logN, shape):
    h = Hybrid(backend, oracle, logN, shape)
    rng = np.random.default_rng(1000 * logN + shape[0] * 10 + shape[2])
    N, L = h.N, h.sizeQ + h.sizeP
    try:
        for K, ns, top in ((1, 1, False), (3, 65537, False), (3, 2, True), (1, T_BIG, False)):
            k_new, k_old = index_sets(N, K)
            a, e = towers(rng, h.qs, N, K * h.dnum, top), towers(rng, h.qs, N, K * h.dnum, top)
            s_new, s_old = towers(rng, h.qs, N, 1, top), towers(rng, h.qs[:h.sizeQ], N, 1, top)
            want = expect_combine(oracle, h.qs, N, a, e, s_new[0], k_new, s_old[0], k_old, h.f, ns)
            ta, te = h.ctx.tower(a), h.ctx.tower(e)
            tsn, tso = h.ctx.tower(s_new), h.ctx.tower(s_old)  # (s_old has sizeQ rows only: the P rows carry no factor and are never read)
            b, _, keys = h.plan.keygen(tsn, tso, ta, te, k_new, k_old, ns=ns)
            assert np.array_equal(b.to_host(), want), f"K={K} ns={ns} top={top}"
            assert np.array_equal(te.to_host(), e) and np.array_equal(ta.to_host(), a), "operands modified"
            assert len(keys) == K
            h.plan.destroy_keys(keys)
            b2, _, keys = h.plan.keygen(tsn, tso, ta, te, k_new, k_old, ns=ns, in_place=True)
            assert b2 is te and np.array_equal(te.to_host(), want), f"in place: K={K} ns={ns} top={top}"
            h.plan.destroy_keys(keys)
    finally:
        h.close()


def test_two_tiles_per_row_and_a_wrapped_key_switches(backend, oracle):
    """N = 2^12: a limb row is two tiles of the kernel; window 1 of the slabs, adopted by fhe_ks_key_wrap, is the key the oracle's
    KeySwitchCore sees at that place"""
    o = oracle
    h = Hybrid(backend, o, 12, (3, 2, 2))
    rng = np.random.default_rng(12)
    N, K = h.N, 2
    k_new, k_old = [5, 2 * N - 1], [1, 25]
    try:
        a, e = towers(rng, h.qs, N, K * h.dnum), towers(rng, h.qs, N, K * h.dnum)
        s_new, s_old = towers(rng, h.qs, N, 1), towers(rng, h.qs[:h.sizeQ], N, 1)
        want = expect_combine(o, h.qs, N, a, e, s_new[0], k_new, s_old[0], k_old, h.f, 1)
        b, ta, keys = h.plan.keygen(h.ctx.tower(s_new), h.ctx.tower(s_old), h.ctx.tower(a), h.ctx.tower(e), k_new, k_old)
        assert np.array_equal(b.to_host(), want)
        hy = o.orc_hybrid_create(N, h.sizeQ, h.qs[:h.sizeQ].copy(), h.psi[:h.sizeQ].copy(), h.sizeP, h.qs[h.sizeQ:].copy(),
                                 h.psi[h.sizeQ:].copy(), h.dnum)
        c = towers(rng, h.qs[:h.sizeQ], N, 1)
        w0, w1 = np.empty_like(c[0]), np.empty_like(c[0])
        o.orc_hybrid_key_switch(hy, c[0], h.sizeQ, np.ascontiguousarray(want[h.dnum:]), np.ascontiguousarray(a[h.dnum:]), w0, w1)
        o.orc_hybrid_destroy(hy)
        h.plan.key = keys[1]
        o0, o1 = h.plan.KeySwitchCore(h.ctx.tower(c))
        assert np.array_equal(o0.to_host()[0], w0) and np.array_equal(o1.to_host()[0], w1)
        h.plan.key = None
        h.plan.destroy_keys(keys)
    finally:
        h.close()


def mixed_context(backend, o, logN):
    """60-, 25-, 50- and 59-bit limbs: the mixed chain with one limb more, so that a subset can leave one out"""
    q = np.array([primes_of(o, logN, b, 1)[0] for b in (60, 25, 50, 59)], np.uint64)
    assert [int(v).bit_length() for v in q] == [60, 25, 50, 59] and T_BIG > int(q[1])
    return q, fh.Context(backend, logN, q, roots(o, logN, q))


@pytest.mark.parametrize("logN", [4, 10])
def test_limb_subset_on_the_mixed_chain(backend, oracle, logN):
    """fhe_keygen_combine over context limbs (2, 0, 1), a factor table with absent terms, every operand at q - 1 and uniform"""
    q, ctx = mixed_context(backend, oracle, logN)
    N, idx = 1 << logN, np.array([2, 0, 1], np.uint32)
    qs = q[idx]
    rng = np.random.default_rng(60 + logN)
    try:
        for ns, top in ((T_BIG, True), (T_BIG, False), (1, True), (65537, False)):
            K, nP = 3, 2
            k_new, k_old = index_sets(N, K)
            a, e = towers(rng, qs, N, K * nP, top), towers(rng, qs, N, K * nP, top)
            s_new, s_old = towers(rng, qs, N, 1, top), towers(rng, qs, N, 1, top)
            factor = np.array([[int(qs[0]) - 1, 0, 7], [0, 0, T_BIG]], np.uint64)  # row 1 has no sOld term at all; T_BIG is reduced inside
            want = expect_combine(oracle, qs, N, a, e, s_new[0], k_new, s_old[0], k_old, factor, ns)
            got = fh.keygen_combine(ctx, ctx.tower(a, idx), ctx.tower(e, idx), ctx.tower(s_new, idx), K, k_new, ctx.tower(s_old, idx), k_old,
                                    factor, ns)
            assert np.array_equal(got.to_host(), want), f"ns={ns} top={top}"
    finally:
        ctx.close()


@pytest.mark.parametrize("logN", [5, 10])
def test_public_key_has_no_old_secret_term(backend, oracle, logN):
    """factor == NULL: b = ns * e - a * s (PKEBase::KeyGenInternal); sOld and kOld are not looked at"""
    q, ctx = mixed_context(backend, oracle, logN)
    N = 1 << logN
    rng = np.random.default_rng(70 + logN)
    try:
        for ns in (1, 65537, T_BIG):
            a, e, s = towers(rng, q, N, 2), towers(rng, q, N, 2), towers(rng, q, N, 1)
            want = expect_combine(oracle, q, N, a, e, s[0], [1, 1], None, [1, 1], None, ns)
            assert np.array_equal(fh.public_key(ctx, ctx.tower(s), ctx.tower(a), ctx.tower(e), ns).to_host(), want), f"ns={ns}"
        # an automorphism of the secret without an sOld term
        want = expect_combine(oracle, q, N, a, e, s[0], [5, 25], None, [1, 1], None, 2)
        assert np.array_equal(fh.keygen_combine(ctx, ctx.tower(a), ctx.tower(e), ctx.tower(s), 2, [5, 25], ns=2).to_host(), want)
    finally:
        ctx.close()


def test_errors_leave_the_output_untouched(backend, oracle):
    h = Hybrid(backend, oracle, 5, (3, 2, 2))
    ctx, plan, L = h.ctx, h.plan, backend.L
    rng = np.random.default_rng(5)
    N, QP, K = h.N, h.sizeQ + h.sizeP, 2
    words = K * h.dnum * QP * N
    try:
        buf = ctx.upload(rng.integers(0, 1 << 20, size=4 * words, dtype=np.uint64))  # a | e | out | spare, contiguous
        before = ctx.download(buf, (4 * words,))
        at = lambda w: C.c_void_p(buf.value + 8 * w)
        a, e, out = at(0), at(words), at(2 * words)
        sn, so = ctx.tower(towers(rng, h.qs, N, 1)), ctx.tower(towers(rng, h.qs[:h.sizeQ], N, 1))
        f = np.ascontiguousarray(h.f)
        fp = f.ctypes.data_as(u64p)
        ks = lambda *v: np.array(v, np.uint32).ctypes.data_as(u32p)

        def combine(nKeys=K, a=a, e=e, sNew=sn.ptr, kNew=None, sOld=so.ptr, kOld=None, factor=fp, ns=1, out=out, nParts=h.dnum):
            return L.fhe_keygen_combine(ctx.h, None, QP, nKeys, nParts, a, e, sNew, kNew, sOld, kOld, factor, ns, out, None)

        def hybrid(nKeys=K, kNew=None, kOld=None, sNew=sn.ptr, sOld=so.ptr, ns=1, a=a, e=e, out=out):
            return L.fhe_ks_keygen_hybrid(plan.h, nKeys, kNew, kOld, sNew, sOld, ns, a, e, out, None)

        key = np.frombuffer(KEY, dtype="<u4").astype(np.uint32).ctypes.data_as(u32p)

        def seeded(nKeys=K, kNew=None, ns=1, sigma=3.19, key=key, b=out, a=a):
            return L.fhe_ks_keygen_hybrid_blake2(plan.h, nKeys, kNew, None, sn.ptr, so.ptr, ns, sigma, key, 0, 1 << 20, b, a, None)

        cases = {
            "nKeys == 0": (lambda: combine(nKeys=0), "nKeys"),
            "nParts == 0": (lambda: combine(nParts=0), "nParts"),
            "even index": (lambda: combine(kNew=ks(1, 4)), "Automorphism index not odd"),
            "even old index": (lambda: combine(kOld=ks(2, 1)), "Automorphism index not odd"),
            "index 2N + 1": (lambda: combine(kNew=ks(2 * N + 1, 1)), "out of range"),
            "null a": (lambda: combine(a=None), "null"),
            "null e": (lambda: combine(e=None), "null"),
            "null sNew": (lambda: combine(sNew=None), "null"),
            "null sOld with a factor": (lambda: combine(sOld=None), "null"),
            "null out": (lambda: combine(out=None), "null"),
            "ns == 0": (lambda: combine(ns=0), "noise scale"),
            "out over a": (lambda: combine(out=at(N)), "overlap"),
            "out half over e": (lambda: combine(out=at(words + N)), "overlap"),
            "out over sNew": (lambda: combine(sNew=at(2 * words + 2 * N)), "overlap"),
            "out over sOld": (lambda: combine(sOld=at(3 * words - N)), "overlap"),
            "hybrid: nKeys == 0": (lambda: hybrid(nKeys=0), "nKeys"),
            "hybrid: even index": (lambda: hybrid(kOld=ks(1, 6)), "Automorphism index not odd"),
            "hybrid: null sOld": (lambda: hybrid(sOld=None), "null"),
            "hybrid: ns == 0": (lambda: hybrid(ns=0), "noise scale"),
            "hybrid: out over a": (lambda: hybrid(out=a), "overlap"),
            "seeded: nKeys == 0": (lambda: seeded(nKeys=0), "nKeys"),
            "seeded: even index": (lambda: seeded(kNew=ks(3, 2)), "Automorphism index not odd"),
            "seeded: sigma 0.5": (lambda: seeded(sigma=0.5), "sigma"),
            "seeded: sigma 300": (lambda: seeded(sigma=300.0), "sigma"),
            "seeded: ns == 0": (lambda: seeded(ns=0), "noise scale"),
            "seeded: null key": (lambda: seeded(key=None), "null"),
            "seeded: b over a": (lambda: seeded(b=at(N)), "overlap"),
        }
        for name, (call, text) in cases.items():
            assert call() == 1, f"{name}: FHE_ERR_ARG expected"
            assert text in L.fhe_last_error().decode(), (name, L.fhe_last_error().decode())
            ctx.sync()
            assert np.array_equal(ctx.download(buf, (4 * words,)), before), f"{name}: device memory changed"
        na, ne = C.c_uint64(), C.c_uint64()
        assert L.fhe_ks_keygen_counters(plan.h, 0, C.byref(na), C.byref(ne)) == 1
        # ... and the same arguments without the fault run
        assert combine(kNew=ks(5, 2 * N - 1)) == 0 and hybrid() == 0 and seeded() == 0
        ctx.sync()
    finally:
        h.close()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("logN", [4, 10])
def test_secret_extend(backend, oracle, logN, shape):
    """Q rows as they are; P rows = limb 0 in COEFFICIENT format, centre-switched to p_j, transformed (keyswitch-hybrid.cpp:59-83)"""
    o = oracle
    h = Hybrid(backend, o, logN, shape)
    rng = np.random.default_rng(80 + logN)
    N, sizeQ, sizeP = h.N, h.sizeQ, h.sizeP
    octx = o.orc_ctx_create(N, sizeQ + sizeP, h.qs, h.psi)
    try:
        # a ternary secret (as the reference's), and uniform residues: limb 0 then takes values on both sides of q_0 / 2
        tern = rng.integers(-1, 2, size=N)
        for coef in (np.stack([(tern % int(q)).astype(np.uint64) for q in h.qs[:sizeQ]]), libs.rand_tower(rng, h.qs[:sizeQ], N)):
            s = coef.copy()[None]
            o.orc_ntt_fwd_tower(octx, s, None, sizeQ, 1, 0)
            want = np.empty((sizeQ + sizeP, N), np.uint64)
            want[:sizeQ] = s[0]
            for j in range(sizeP):
                row = coef[0].copy()
                o.orc_switch_modulus(row, N, int(h.qs[0]), int(h.qs[sizeQ + j]))
                row = row[None, None].copy()
                o.orc_ntt_fwd_tower(octx, row, np.array([sizeQ + j], np.uint32).ctypes.data_as(C.c_void_p), 1, 1, 0)
                want[sizeQ + j] = row[0, 0]
            ts = h.ctx.tower(s)
            assert np.array_equal(h.plan.extend_secret(ts).to_host()[0], want)
            assert np.array_equal(ts.to_host(), s), "the secret was modified"
    finally:
        o.orc_ctx_destroy(octx)
        h.close()


def launches(lib):
    total = C.c_uint64()
    lib.L.fhe_launch_stats(None, 0, C.byref(total))
    return total.value, lib.launch_count("keygen_combine_kernel")


@pytest.mark.parametrize("shape,logN,ns", [((3, 2, 2), 10, 1), ((4, 1, 4), 5, 65537), ((3, 3, 1), 12, 1)])
def test_seeded_form_is_its_composition_and_its_launches_do_not_grow(backend, oracle, shape, logN, ns):
    """fhe_ks_keygen_hybrid_blake2 == fhe_sample_uniform_blake2 (a, as drawn) + fhe_sample_gaussian_blake2 -> fhe_ntt_fwd (e) ->
    fhe_ks_keygen_hybrid, word for word; the same number of launches for 1 and for 3 keys, one of them the combine"""
    h = Hybrid(backend, oracle, logN, shape)
    rng = np.random.default_rng(90 + logN)
    N, QP = h.N, h.sizeQ + h.sizeP
    try:
        tsn, tso = h.ctx.tower(towers(rng, h.qs, N, 1)), h.ctx.tower(towers(rng, h.qs[:h.sizeQ], N, 1))
        spent = {}
        for K in (1, 3):
            k_new, k_old = index_sets(N, K)
            na, ne = h.plan.keygen_counters(K)
            assert na == -(-2 * K * h.dnum * QP * N // 512) and ne == -(-K * h.dnum * N // 512)
            ca, ce = 7, 7 + na  # disjoint counter ranges, laid out with the counts
            a = h.ctx.sample("uniform", K * h.dnum, QP, generator="blake2", key=KEY, counter0=ca)
            a.fmt = fh.EVALUATION  # used as drawn
            e = h.ctx.sample("gaussian", K * h.dnum, QP, sigma=3.19, generator="blake2", key=KEY, counter0=ce).SwitchFormat()
            wb, wa, keys = h.plan.keygen(tsn, tso, a, e, k_new, k_old, ns=ns)
            h.plan.destroy_keys(keys)
            h.ctx.sync()
            t0, c0 = launches(backend)
            b, a2, keys = h.plan.keygen_blake2(tsn, tso, K, KEY, ca, ce, k_new, k_old, ns=ns, sigma=3.19)
            h.ctx.sync()
            t1, c1 = launches(backend)
            h.plan.destroy_keys(keys)
            spent[K] = t1 - t0
            assert c1 - c0 == 1, "exactly one combine launch"
            assert np.array_equal(a2.to_host(), wa.to_host()), f"K={K}: the a half is not the uniform sampler's words"
            assert np.array_equal(b.to_host(), wb.to_host()), f"K={K}: the b half differs from the composition"
        assert spent[1] == spent[3], spent
    finally:
        h.close()


def test_rotation_key_indices(backend, oracle):
    """kNew = (5^r)^-1 mod 2N, kOld = 1 (EvalAutomorphismKeyGen: the new secret is the permuted one)"""
    N = 64
    k_new, k_old = fh.rotation_key_indices(backend, [1, -1, 5], N)
    for r, kn, ko in zip([1, -1, 5], k_new, k_old):
        k = oracle.orc_find_automorphism_index_2n_complex(r, 2 * N)
        assert (int(kn) * k) % (2 * N) == 1 and ko == 1
