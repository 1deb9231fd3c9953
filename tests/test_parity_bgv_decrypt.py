"""BGV decryption on the device: the ModReduce chain of a COEFFICIENT tower in one launch per 16 limbs, its residues modulo t, and
PKEBGVRNS::Decrypt as one call.

  * fhe_mod_reduce_chain against the oracle's restatement of DCRTPolyImpl::ModReduce (dcrtpoly-impl.h:736-755, evalFormat 0) applied step by
    step; fhe_mod_reduce_to_t against the same loop down to one limb and (x_0 > floor(q_0/2) ? x_0 - q_0 : x_0) mod t with Python integers
    (NativeVector::Mod, mubintvecnat.cpp:145-161, 351-356);
  * fhe_bgv_decrypt against orc_vec_mul / orc_vec_add (PKERNS::DecryptCore), orc_ntt_inv_tower, and the two above;
  * the launches of each call, and every argument error with the output left as it was.
Every comparison is word for word."""
import ctypes as C

import numpy as np
import pytest

import libs
from openfhe_amd import fhe_hip as fh
from test_parity import ckks_like_params, params
from test_parity_bgv import T_BIG, T_SMALL, delta_targets, edge_tower, mixed_chain
from test_parity_edges import pattern, primes_of, roots

u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)


def loop_of_mod_reduce(o, octx, x, levels, t):
    """`levels` calls of DCRTPolyImpl::ModReduce on the COEFFICIENT towers x [batch][sizeQl][N] -> [batch][sizeQl - levels][N]"""
    cur = np.ascontiguousarray(x)
    for _ in range(levels):
        n = cur.shape[1]
        nxt = np.zeros((cur.shape[0], n - 1, cur.shape[2]), np.uint64)
        for b in range(cur.shape[0]):
            o.orc_mod_reduce(octx, np.ascontiguousarray(cur[b]), n, t, 0, nxt[b])
        cur = nxt
    return cur


def residues_mod_t(x0, q0, t):
    """DecryptionCRTInterpolate(t) of one limb x0 [batch][N] modulo q0, with Python integers"""
    q0, h = int(q0), int(q0) // 2
    return np.array([[(int(v) - q0 if int(v) > h else int(v)) % t for v in row] for row in x0], np.uint64)


def chain_case(backend, o, logN, q, psi, levels, B, ts, seed, x_of=None):
    N, sizeQl = 1 << logN, len(q)
    rng = np.random.default_rng(seed)
    ctx = fh.Context(backend, logN, q, psi)
    octx = o.orc_ctx_create(N, sizeQl, q, psi)
    try:
        for t in ts:
            x = x_of(rng, octx, t) if x_of else np.stack([pattern(rng, ("mix", "max", "uniform")[b % 3], q, N) for b in range(B)])
            want = loop_of_mod_reduce(o, octx, x, levels, t)
            xt = ctx.tower(x, fmt=fh.COEFFICIENT)
            got = fh.mod_reduce_chain(ctx, xt, levels, t).to_host()
            assert np.array_equal(got, want), f"chain logN={logN} sizeQl={sizeQl} levels={levels} t={t}"
            if levels == sizeQl - 1:
                got_t = fh.mod_reduce_to_t(ctx, xt, t)
                assert np.array_equal(got_t, residues_mod_t(want[:, 0], q[0], t)), f"to_t logN={logN} sizeQl={sizeQl} t={t}"
    finally:
        o.orc_ctx_destroy(octx)
        ctx.close()


# (logN, sizeQl, levels, batch): batch 3 at N = 16 is a partial workgroup; 15 / 16 / 17 levels around the chunk boundary; 33 levels are two
# full chunks and a rest; 2^12 and 2^13 whole workgroups
CHAIN_SHAPES = [(4, 3, 1, 2), (4, 5, 4, 3), (10, 18, 15, 1), (10, 18, 16, 1), (10, 18, 17, 2), (4, 34, 33, 1), (12, 4, 3, 2), (13, 3, 2, 1)]


@pytest.mark.parametrize("logN,sizeQl,levels,B", CHAIN_SHAPES)
def test_mod_reduce_chain_shapes(backend, oracle, logN, sizeQl, levels, B):
    q, psi = params(oracle, logN, sizeQl)
    chain_case(backend, oracle, logN, q, psi, levels, B, T_SMALL, 300 + logN + sizeQl)


@pytest.mark.parametrize("logN,levels", [(4, 1), (4, 2), (12, 2)])
def test_chain_on_the_mixed_chain_switches_both_ways(backend, oracle, logN, levels):
    q, psi = mixed_chain(oracle, logN)
    assert T_BIG > int(q[1]) and [int(v).bit_length() for v in q] == [60, 25, 50]
    chain_case(backend, oracle, logN, q, psi, levels, 2, (T_BIG, 65537), 400 + logN)


def check_first_delta(x, q, t):
    """the first delta of every tower of x takes the branch points of SwitchModulus at both ends of the row"""
    ql = int(q[-1])
    negt_inv = (-pow(t % ql, -1, ql)) % ql
    tg = delta_targets(ql)
    for b in range(x.shape[0]):
        row = x[b, -1]
        assert [(int(v) * negt_inv) % ql for v in list(row[:5]) + list(row[-5:])] == tg + tg[::-1]


@pytest.mark.parametrize("logN,sizeQl", [(4, 3), (10, 5), (12, 3)])
def test_branch_points_of_the_first_step(backend, oracle, logN, sizeQl):
    """the dropped limb is built so that the first delta is 0, 1, floor(q/2), floor(q/2) + 1, q - 1"""
    o = oracle
    q, psi = params(o, logN, sizeQl)

    def edges(rng, octx, t):
        x = edge_tower(o, rng, octx, q, 1 << logN, t, ("max", "mix"), 0)
        check_first_delta(x, q, t)
        return x

    for levels in (1, sizeQl - 1):
        chain_case(backend, o, logN, q, psi, levels, 2, T_SMALL, 500 + logN, edges)


@pytest.mark.parametrize("pair", [0, 1])
def test_branch_points_on_adjacent_pairs_of_the_mixed_chain(backend, oracle, pair):
    """sizeQl = 2 over (60-bit, 25-bit) and (25-bit, 50-bit): the one step switches down, then up"""
    o, logN = oracle, 6
    q3, psi3 = mixed_chain(o, logN)
    q, psi = q3[pair:pair + 2].copy(), psi3[pair:pair + 2].copy()

    def edges(rng, octx, t):
        x = edge_tower(o, rng, octx, q, 1 << logN, t, ("max", "mix"), 0)
        check_first_delta(x, q, t)
        return x

    chain_case(backend, o, logN, q, psi, 1, 2, (T_BIG, 65537, 2), 600 + pair, edges)


@pytest.mark.parametrize("t", [2, 65537, T_BIG])
def test_mod_reduce_to_t_on_one_limb(backend, oracle, t):
    """sizeQl == 1: no step, only the centred residue modulo t; a 25-bit limb, so that T_BIG is a t above q_0"""
    o, logN = oracle, 6
    N = 1 << logN
    q = np.array(primes_of(o, logN, 25, 1), np.uint64)
    q0 = int(q[0])
    assert (t > q0) == (t == T_BIG)
    ctx = fh.Context(backend, logN, q, roots(o, logN, q))
    x = np.random.default_rng(7).integers(0, q0, size=(2, 1, N), dtype=np.uint64)
    x[0, 0, :5] = [0, 1, q0 // 2, q0 // 2 + 1, q0 - 1]
    x[1, 0, -5:] = [q0 - 1, q0 // 2 + 1, q0 // 2, 1, 0]
    got = fh.mod_reduce_to_t(ctx, ctx.tower(x, fmt=fh.COEFFICIENT), t)
    ctx.close()
    assert np.array_equal(got, residues_mod_t(x[:, 0], q0, t))
    assert got.max() < t


def decrypt_want(o, sub, qs, N, elems, s, t):
    """PKEBGVRNS::Decrypt of ONE ciphertext: elems [nElem][sizeQl][N], s [sizeQl][N], EVALUATION"""
    sizeQl = len(qs)
    b, tmp, sp = elems[0].copy(), np.empty_like(s), s.copy()
    for e in range(1, len(elems)):
        for i in range(sizeQl):
            if e > 1:
                o.orc_vec_mul(sp[i], sp[i].copy(), s[i], N, int(qs[i]))
            o.orc_vec_mul(tmp[i], np.ascontiguousarray(elems[e][i]), sp[i], N, int(qs[i]))
            o.orc_vec_add(b[i], b[i].copy(), tmp[i], N, int(qs[i]))
    o.orc_ntt_inv_tower(sub, b, None, sizeQl, 1, 0)
    last = loop_of_mod_reduce(o, sub, b[None], sizeQl - 1, t)
    return residues_mod_t(last[:, 0], qs[0], t)[0]


@pytest.mark.parametrize("nElem", [2, 3])
@pytest.mark.parametrize("logN,sizeQl", [(4, 3), (12, 3), (13, 4)])
def test_bgv_decrypt(backend, oracle, logN, sizeQl, nElem):
    """batch 1 and 3 over the leading limbs, then over a limb list that is not the leading one"""
    o = oracle
    N, t = 1 << logN, 65537
    rng = np.random.default_rng(700 + logN + nElem)
    q, psi, _, _ = ckks_like_params(o, logN, sizeQl + 3, 2)
    ctx = fh.Context(backend, logN, q, psi)
    scattered = [sizeQl + 2, 0, sizeQl, 1, 2][:sizeQl]
    for limbs, batches in ((None, (1, 3)), (scattered, (3,))):
        idx = list(range(sizeQl)) if limbs is None else limbs
        qs = np.array([int(q[i]) for i in idx], np.uint64)
        sub = o.orc_ctx_create(N, sizeQl, qs, np.array([int(psi[i]) for i in idx], np.uint64))
        s = libs.rand_tower(rng, qs, N)
        for B in batches:
            elems = [libs.rand_tower(rng, qs, N, B) for _ in range(nElem)]
            want = np.stack([decrypt_want(o, sub, qs, N, [e[b] for e in elems], s, t) for b in range(B)])
            got = fh.bgv_decrypt(ctx, [ctx.tower(e, limbs) for e in elems], ctx.tower(s, limbs), t)
            assert np.array_equal(got, want), f"decrypt logN={logN} sizeQl={sizeQl} nElem={nElem} batch={B} limbs={limbs}"
        o.orc_ctx_destroy(sub)
    ctx.close()


COUNTED = ("mod_reduce_chain_kernel", "switch_modulus_kernel", "elemwise_kernel", "elemwise_cv_kernel")


def launches(lib, names=COUNTED):
    return np.array([lib.launch_count(k) for k in names], np.int64)


def ntt_launches(lib):
    buf = C.create_string_buffer(1 << 16)
    lib.L.fhe_launch_stats(buf, len(buf), None)
    return sum(int(line.rsplit(" ", 1)[1]) for line in buf.value.decode().splitlines() if "ntt_" in line.rsplit(" ", 1)[0])


def test_chain_launches(backend, oracle):
    """up to 16 levels are ONE launch of the chain kernel and nothing else; 17 levels are two"""
    o, logN, sizeQl, t = oracle, 6, 18, 65537
    q, psi = params(o, logN, sizeQl)
    ctx = fh.Context(backend, logN, q, psi)
    x = ctx.tower(libs.rand_tower(np.random.default_rng(9), q, 1 << logN, 2), fmt=fh.COEFFICIENT)
    for levels, chain in ((1, 1), (5, 1), (16, 1), (17, 2)):
        before, ntt = launches(backend), ntt_launches(backend)
        fh.mod_reduce_chain(ctx, x, levels, t)
        assert list(launches(backend) - before) == [chain, 0, 0, 0] and ntt_launches(backend) == ntt, levels
    before = launches(backend)
    fh.mod_reduce_to_t(ctx, x, t)
    assert list(launches(backend) - before) == [2, 0, 0, 0]
    ctx.close()


@pytest.mark.parametrize("nElem,elementwise", [(2, 2), (3, 4)])
def test_bgv_decrypt_launches(backend, oracle, nElem, elementwise):
    """N = 2^13: DecryptCore's element-wise launches, the two passes of ONE inverse transform, one chain launch"""
    o, logN, sizeQl, t = oracle, 13, 3, 65537
    N = 1 << logN
    q, psi = params(o, logN, sizeQl)
    ctx = fh.Context(backend, logN, q, psi)
    rng = np.random.default_rng(10)
    elems = [ctx.tower(libs.rand_tower(rng, q, N, 2)) for _ in range(nElem)]
    s = ctx.tower(libs.rand_tower(rng, q, N))
    before, ntt = launches(backend), ntt_launches(backend)
    fh.bgv_decrypt(ctx, elems, s, t)
    assert list(launches(backend) - before) == [1, 0, elementwise, 0]
    assert ntt_launches(backend) - ntt == 2
    ctx.close()


def test_argument_errors_leave_the_output_untouched(backend, oracle):
    o, logN, L, t = oracle, 6, 20, 65537
    N = 1 << logN
    q, psi = params(o, logN, L)
    ctx = fh.Context(backend, logN, q, psi)
    lib = backend.L
    mark = np.full((1, L, N), 0x5A5A5A5A, np.uint64)
    x, out, s = ctx.tower(np.zeros((1, L, N), np.uint64), fmt=fh.COEFFICIENT), ctx.tower(mark), ctx.tower(np.zeros((1, L, N), np.uint64))
    wsb = lib.fhe_bgv_decrypt_workspace_bytes(ctx.h, 3, L, 1)
    assert wsb >= lib.fhe_mod_reduce_chain_workspace_bytes(ctx.h, L, L - 1, 1) > 0 == lib.fhe_mod_reduce_chain_workspace_bytes(ctx.h, L, 16, 1)
    ws = ctx.malloc(wsb)
    far = np.array(list(range(L - 1)) + [L], np.uint32).ctypes.data_as(u32p)
    twice = np.array([0] + list(range(L - 1)), np.uint32).ctypes.data_as(u32p)
    ql, qk = int(q[L - 1]), int(q[L - 3])
    chain = lambda xx, li, n, lv, tt, b, oo, w, wb: lib.fhe_mod_reduce_chain(ctx.h, xx, li, n, lv, tt, b, oo, w, wb, None)
    to_t = lambda xx, li, n, tt, b, oo, w, wb: lib.fhe_mod_reduce_to_t(ctx.h, xx, li, n, tt, b, oo, w, wb, None)
    elems = (C.c_void_p * 3)(x.ptr.value, x.ptr.value, x.ptr.value)
    dec = lambda cc, ne, ss, li, n, tt, b, oo, w, wb: lib.fhe_bgv_decrypt(ctx.h, cc, ne, ss, li, n, tt, b, oo, w, wb, None)

    def bad(status, text):
        assert status != 0 and text in lib.fhe_last_error().decode(), (status, lib.fhe_last_error())

    bad(chain(None, None, L, 3, t, 1, out.ptr, ws, wsb), "fhe_mod_reduce_chain: null argument")
    bad(chain(x.ptr, None, L, 3, t, 1, None, ws, wsb), "fhe_mod_reduce_chain: null argument")
    bad(chain(x.ptr, None, L, L - 1, t, 1, out.ptr, None, 0), "fhe_mod_reduce_chain: null argument")  # (more than 16 levels need ws)
    bad(chain(x.ptr, None, L, 0, t, 1, out.ptr, ws, wsb), "levels must be in [1, sizeQl)")
    bad(chain(x.ptr, None, L, L, t, 1, out.ptr, ws, wsb), "levels must be in [1, sizeQl)")
    bad(chain(x.ptr, None, 1, 1, t, 1, out.ptr, ws, wsb), "Removing last element")
    bad(chain(x.ptr, None, L + 1, 3, t, 1, out.ptr, ws, wsb), "Removing last element")
    bad(chain(x.ptr, far, L, 3, t, 1, out.ptr, ws, wsb), "limb index exceeds context size")
    bad(chain(x.ptr, None, L, 3, 1, 1, out.ptr, ws, wsb), "t must be in [2, 2^63)")
    bad(chain(x.ptr, None, L, 3, 5 * ql, 1, out.ptr, ws, wsb), "invertible modulo every dropped limb")
    bad(chain(x.ptr, None, L, 3, qk, 1, out.ptr, ws, wsb), "invertible modulo every dropped limb")
    assert chain(x.ptr, None, L, 2, qk, 1, out.ptr, ws, wsb) == 0  # (a multiple of a KEPT limb is legal)
    ctx.sync()
    ctx.lib.check(lib.fhe_memcpy_h2d(ctx.h, out.ptr, mark.ctypes.data_as(C.c_void_p), mark.nbytes, None))
    ctx.sync()
    bad(chain(x.ptr, twice, L, L - 1, t, 1, out.ptr, ws, wsb), "the moduli of a tower must be distinct")
    bad(chain(x.ptr, None, L, L - 1, t, 1, out.ptr, ws, 8), "workspace too small")
    bad(chain(x.ptr, None, L, 3, t, 0, out.ptr, ws, wsb), "workspace too small")  # (batch 0)
    bad(chain(x.ptr, None, L, 3, t, 1, x.ptr, ws, wsb), "out must not alias x")
    bad(to_t(None, None, L, t, 1, out.ptr, ws, wsb), "fhe_mod_reduce_to_t: null argument")
    bad(to_t(x.ptr, None, 0, t, 1, out.ptr, ws, wsb), "sizeQl must be at least 1")
    bad(to_t(x.ptr, None, 1, t, 1, None, ws, wsb), "fhe_mod_reduce_to_t: null argument")
    bad(to_t(x.ptr, far, L, t, 1, out.ptr, ws, wsb), "limb index exceeds context size")
    bad(to_t(x.ptr, None, L, 0, 1, out.ptr, ws, wsb), "t must be in [2, 2^63)")
    bad(to_t(x.ptr, None, L, 1 << 63, 1, out.ptr, ws, wsb), "t must be in [2, 2^63)")
    bad(to_t(x.ptr, None, L, int(q[1]), 1, out.ptr, ws, wsb), "invertible modulo every dropped limb")
    bad(to_t(x.ptr, None, L, t, 1, out.ptr, ws, 8), "workspace too small")
    bad(to_t(x.ptr, None, L, t, 1, x.ptr, ws, wsb), "out must not alias x")
    bad(dec(None, 2, s.ptr, None, L, t, 1, out.ptr, ws, wsb), "fhe_bgv_decrypt: null argument")
    bad(dec(elems, 2, None, None, L, t, 1, out.ptr, ws, wsb), "fhe_bgv_decrypt: null argument")
    bad(dec((C.c_void_p * 3)(x.ptr.value, None, None), 2, s.ptr, None, L, t, 1, out.ptr, ws, wsb), "fhe_bgv_decrypt: null argument")
    bad(dec((C.c_void_p * 3)(x.ptr.value, out.ptr.value, None), 2, s.ptr, None, L, t, 1, out.ptr, ws, wsb), "fhe_bgv_decrypt: null argument")
    bad(dec(elems, 1, s.ptr, None, L, t, 1, out.ptr, ws, wsb), "2 or 3 elements")
    bad(dec(elems, 4, s.ptr, None, L, t, 1, out.ptr, ws, wsb), "2 or 3 elements")
    bad(dec(elems, 2, s.ptr, None, L + 1, t, 1, out.ptr, ws, wsb), "sizeQl exceeds context size")
    bad(dec(elems, 2, s.ptr, far, L, t, 1, out.ptr, ws, wsb), "limb index exceeds context size")
    bad(dec(elems, 2, s.ptr, None, L, 1, 1, out.ptr, ws, wsb), "t must be in [2, 2^63)")
    bad(dec(elems, 2, s.ptr, None, L, ql, 1, out.ptr, ws, wsb), "invertible modulo every dropped limb")
    bad(dec(elems, 2, s.ptr, twice, L, t, 1, out.ptr, ws, wsb), "the moduli of a tower must be distinct")
    bad(dec(elems, 3, s.ptr, None, L, t, 1, out.ptr, ws, wsb - 8), "workspace too small")
    ctx.sync()
    assert np.array_equal(out.to_host(), mark), "a refused call wrote to its output"
    assert to_t(x.ptr, None, L, t, 1, out.ptr, ws, wsb) == 0 and dec(elems, 3, s.ptr, None, L, t, 1, out.ptr, ws, wsb) == 0
    ctx.sync()
    ctx.close()


@pytest.mark.gpu
def test_full_size_chain_against_the_member_loop_on_the_device(hip):
    """the smallest shape of tools/bgv_decrypt_bench.py (N = 2^14, sizeQl = 8, batch 2): the loop of fhe_mod_reduce on COEFFICIENT towers, run on
    the same device, gives the words of the chain"""
    backend = hip
    logN, sizeQl, B, t = 14, 8, 2, 65537
    q, psi = backend.dcrt_chain(logN, sizeQl, 60)
    ctx = fh.Context(backend, logN, q, psi)
    x = ctx.tower(libs.rand_tower(np.random.default_rng(11), q, 1 << logN, B), fmt=fh.COEFFICIENT)
    cur, steps = x, {}
    for n in range(sizeQl, 1, -1):
        cur = fh.mod_reduce(ctx, cur, t)
        steps[sizeQl - n + 1] = cur
    for levels in (1, 3, sizeQl - 1):
        assert np.array_equal(fh.mod_reduce_chain(ctx, x, levels, t).to_host(), steps[levels].to_host()), levels
    assert np.array_equal(fh.mod_reduce_to_t(ctx, x, t), residues_mod_t(cur.to_host()[:, 0], q[0], t))
    ctx.close()
