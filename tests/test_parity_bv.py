"""BV key switching (KeySwitchBV, keyswitch-bv.cpp) as device composites: fhe_bv_precompute, fhe_bv_fast_keyswitch, fhe_keyswitch_bv and
fhe_bfv_eval_mult_relin_hps_bv, word for word against the digits of orc_crt_decompose (pinned on DCRTPolyImpl::CRTDecompose by
tests/test_oracle_vs_ref.py) and exact Python-integer sums  out_e[i] = sum_d digit[d][i] * key_e[d][i] mod q_i.
`backend` = the lane emulator on the CPU, the product library with -m gpu."""
import ctypes as C
import functools

import numpy as np
import pytest

import hps_ref
import libs
from openfhe_amd import fhe_hip as fh

FHE_ERR_ARG, FHE_ERR_UNSUPPORTED = 1, 4


def params(o, logN, L, bits):
    q, psi = np.zeros(L, np.uint64), np.zeros(L, np.uint64)
    o.orc_dcrt_params(2 << logN, L, bits, q, psi)
    return q, psi


def windows(q, base_bits):
    return 1 if base_bits == 0 else -(-int(q).bit_length() // base_bits)


def digits_of(o, octx, x, base_bits):
    """orc_crt_decompose of every tower of x [batch][L][N] (COEFFICIENT) -> [batch][D][L][N] EVALUATION"""
    B, L, N = x.shape
    D = o.orc_crt_decompose(octx, x[0].ctypes.data, L, base_bits, None)
    out = np.zeros((B, D, L, N), np.uint64)
    for b in range(B):
        assert o.orc_crt_decompose(octx, np.ascontiguousarray(x[b]).ctypes.data, L, base_bits, out[b].ctypes.data) == D
    return out


def exact_sums(dig, key, q):
    """dig [batch][D][L][N], key [>= D][>= L][N] -> [batch][L][N]: sum_d dig[b][d][i] * key[d][i] mod q_i over Python integers"""
    B, D, L, N = dig.shape
    out = np.zeros((B, L, N), np.uint64)
    for i in range(L):
        k = key[:D, i].astype(object)
        for b in range(B):
            out[b, i] = ((dig[b, :, i].astype(object) * k).sum(axis=0) % int(q[i])).astype(np.uint64)
    return out


def add_mod(a, b, q):
    """(a + b) mod q_i per limb, towers [batch][L][N] of residues below 2^60"""
    s = a + b
    qq = q[None, :len(q), None]
    return np.where(s >= qq, s - qq, s)


# (logN, sizeQ, bits, baseBits, batch, sizeQl): what each shape stresses
SHAPES = [
    (4, 3, 60, 0, 1, 3),    # N below a tile; D = 3 < 8
    (5, 4, 60, 4, 2, 3),    # D_l = 45: six chunks, the last partial; level below sizeQ: key row stride sizeQ, tower stride sizeQl, key prefix
    (5, 3, 60, 1, 1, 2),    # D_l = 120
    (10, 3, 30, 8, 2, 3),   # moduli below 36 bits
    (5, 5, 45, 3, 3, 4),    # odd batch; group count not a multiple of 8
    (12, 2, 50, 7, 2, 2),   # one full tile
    (12, 2, 60, 30, 1, 2),  # widest window
    (13, 3, 60, 0, 2, 3),   # two tiles per row; the two-pass NTT
]


@functools.lru_cache(maxsize=None)
def case(logN, sizeQ, bits, base_bits, batch, sizeQl, worst=False):
    """operands and expected words of one shape, computed once and shared by the backends and the tests; read-only"""
    o = libs.load_oracle()
    N = 1 << logN
    q, psi = params(o, logN, sizeQ, bits)
    rng = np.random.default_rng(7000 + 100 * logN + 10 * sizeQ + base_bits)
    ql = q[:sizeQl]
    D0 = sum(windows(v, base_bits) for v in q)
    Dl = sum(windows(v, base_bits) for v in ql)
    x = libs.rand_tower(rng, ql, N, batch)  # COEFFICIENT form
    x[:, :, 0] = 0
    x[:, :, 1] = ql - np.uint64(1)
    x[:, :, 2] = ql >> np.uint64(1)
    x[:, :, 3] = (ql >> np.uint64(1)) + np.uint64(1)
    keys = []
    for _ in range(2):  # two keys (hoisting), each (b, a)
        kb, ka = (np.stack([libs.rand_tower(rng, q, N) for _ in range(D0)]) for _ in range(2))
        kb[:, :, 5] = q - np.uint64(1)
        ka[:, :, 5] = q - np.uint64(1)
        keys.append((kb, ka))
    if worst:  # every window all ones in every limb / q - 1, against keys of q - 1: the largest column sums
        for i, v in enumerate(ql):
            nW = windows(v, base_bits)
            x[:, i, :] = (1 << (base_bits * (nW - 1))) - 1
            x[:, i, 1::2] = v - np.uint64(1)
        for kb, ka in keys:
            kb[:] = q[None, :, None] - np.uint64(1)
            ka[:] = q[None, :, None] - np.uint64(1)
    octx = o.orc_ctx_create(N, sizeQl, np.ascontiguousarray(ql), np.ascontiguousarray(psi[:sizeQl]))
    dig = digits_of(o, octx, x, base_bits)
    assert dig.shape[1] == Dl
    xe = x.copy()
    o.orc_ntt_fwd_tower(octx, xe, None, sizeQl, batch, 1)
    o.orc_ctx_destroy(octx)
    want = [(exact_sums(dig, kb, ql), exact_sums(dig, ka, ql)) for kb, ka in keys]
    acc = (libs.rand_tower(rng, ql, N, batch), libs.rand_tower(rng, ql, N, batch))
    for a in [q, psi, x, xe, dig, *acc] + [v for k in keys for v in k] + [v for w in want for v in w]:
        a.setflags(write=False)
    return dict(q=q, psi=psi, x=x, xe=xe, dig=dig, keys=keys, want=want, acc=acc, D0=D0, Dl=Dl)


def ws_digits(ctx, key, Dl, batch, sizeQl):
    ws, _ = key.workspace(sizeQl, batch)
    return ctx.download(ws, (Dl, batch, sizeQl, ctx.N))


# ---- 1. parity over the shapes, from both input formats ------------------------------------------------------------------------------
@pytest.mark.parametrize("ev", [0, 1], ids=["coef", "eval"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "logN%d-Q%d-%db-r%d-b%d-l%d" % s)
def test_parity(backend, shape, ev):
    logN, sizeQ, bits, base_bits, batch, sizeQl = shape
    z = case(*shape)
    ctx = fh.Context(backend, logN, z["q"], z["psi"])
    key = fh.BvKey(ctx, sizeQ, base_bits, *z["keys"][0])
    assert key.digits(sizeQ) == z["D0"] and key.digits(sizeQl) == z["Dl"]
    xin = z["xe"] if ev else z["x"]
    c = ctx.tower(xin, fmt=fh.EVALUATION if ev else fh.COEFFICIENT)
    key.Precompute(c)
    o0, o1 = key.FastKeySwitch(sizeQl, batch)
    assert np.array_equal(o0.to_host(), z["want"][0][0]) and np.array_equal(o1.to_host(), z["want"][0][1])
    got = ws_digits(ctx, key, z["Dl"], batch, sizeQl)
    for b in range(batch):
        assert np.array_equal(got[:, b], z["dig"][b]), f"digit-major digits of ciphertext {b}"
    assert np.array_equal(c.to_host(), xin), "the input is only read"
    if ev:  # KeySwitchCore = the two calls
        ctx.lib.check(ctx.lib.L.fhe_memset_zero(ctx.h, key.workspace(sizeQl, batch)[0], key.workspace(sizeQl, batch)[1], None))
        p0, p1 = key.KeySwitchCore(c)
        assert np.array_equal(p0.to_host(), z["want"][0][0]) and np.array_equal(p1.to_host(), z["want"][0][1])
        assert np.array_equal(c.to_host(), xin)
    key.close()
    ctx.close()


# ---- 2. worst-case column sums ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 3, 60, 1, 1, 3), (5, 4, 60, 4, 1, 4)], ids=lambda s: "logN%d-Q%d-%db-r%d-b%d-l%d" % s)
def test_worst_case_column_sums(backend, shape):
    logN, sizeQ, bits, base_bits, batch, sizeQl = shape
    z = case(*shape, worst=True)
    ctx = fh.Context(backend, logN, z["q"], z["psi"])
    key = fh.BvKey(ctx, sizeQ, base_bits, *z["keys"][0])
    o0, o1 = key.KeySwitchCore(ctx.tower(z["xe"]))
    assert np.array_equal(o0.to_host(), z["want"][0][0]) and np.array_equal(o1.to_host(), z["want"][0][1])
    key.close()
    ctx.close()


# ---- 3. accumulate ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4], SHAPES[5]], ids=lambda s: "logN%d-Q%d-%db-r%d-b%d-l%d" % s)
def test_accumulate(backend, shape):
    logN, sizeQ, bits, base_bits, batch, sizeQl = shape
    z = case(*shape)
    ql = z["q"][:sizeQl]
    ctx = fh.Context(backend, logN, z["q"], z["psi"])
    key = fh.BvKey(ctx, sizeQ, base_bits, *z["keys"][0])
    a0, a1 = ctx.tower(z["acc"][0]), ctx.tower(z["acc"][1])
    r0, r1 = key.KeySwitchCore(ctx.tower(z["xe"]), a0, a1)
    assert r0 is a0 and r1 is a1
    assert np.array_equal(a0.to_host(), add_mod(z["acc"][0], z["want"][0][0], ql))
    assert np.array_equal(a1.to_host(), add_mod(z["acc"][1], z["want"][0][1], ql))
    key.close()
    ctx.close()


# ---- 4. hoisting: one Precompute, two keys ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[7]], ids=lambda s: "logN%d-Q%d-%db-r%d-b%d-l%d" % s)
def test_hoisting(backend, shape):
    logN, sizeQ, bits, base_bits, batch, sizeQl = shape
    z = case(*shape)
    ctx = fh.Context(backend, logN, z["q"], z["psi"])
    k0 = fh.BvKey(ctx, sizeQ, base_bits, *z["keys"][0])
    k1 = fh.BvKey(ctx, sizeQ, base_bits, *z["keys"][1])
    c = ctx.tower(z["xe"])
    k0.Precompute(c)
    before = backend.launch_count("crt_digits_kernel")
    fast = [k.FastKeySwitch(sizeQl, batch, ws_of=k0) for k in (k0, k1)]
    assert backend.launch_count("crt_digits_kernel") == before
    core = [k.KeySwitchCore(c) for k in (k0, k1)]
    for t in range(2):
        for e in range(2):
            assert np.array_equal(fast[t][e].to_host(), core[t][e].to_host())
            assert np.array_equal(fast[t][e].to_host(), z["want"][t][e])
    k0.close()
    k1.close()
    ctx.close()


# ---- 5. launch counts ---------------------------------------------------------------------------------------------------------------
def test_launch_counts(backend):
    shape = SHAPES[1]
    logN, sizeQ, bits, base_bits, batch, sizeQl = shape
    z = case(*shape)
    ctx = fh.Context(backend, logN, z["q"], z["psi"])
    key = fh.BvKey(ctx, sizeQ, base_bits, *z["keys"][0])
    c = ctx.tower(z["xe"])
    names = ("crt_digits_kernel", "bv_inner_product_kernel", "inner_rows_kernel")
    before = [backend.launch_count(k) for k in names]
    key.KeySwitchCore(c)
    assert [backend.launch_count(k) - b for k, b in zip(names, before)] == [1, 1, 0]
    # fhe_crt_decompose at 4 limbs: one launch cuts every source limb
    x4 = libs.rand_tower(np.random.default_rng(5), z["q"], ctx.N, 1)
    before = backend.launch_count("crt_digits_kernel")
    got = ctx.tower(x4, fmt=fh.COEFFICIENT).CRTDecompose(base_bits)
    assert got is not None and got.batch == z["D0"]
    assert backend.launch_count("crt_digits_kernel") == before + 1
    key.close()
    ctx.close()


# ---- 6. errors enqueue nothing ------------------------------------------------------------------------------------------------------
def test_errors(backend):
    shape = SHAPES[1]
    logN, sizeQ, bits, base_bits, batch, sizeQl = shape
    z = case(*shape)
    L = backend.L
    ctx = fh.Context(backend, logN, z["q"], z["psi"])
    key = fh.BvKey(ctx, sizeQ, base_bits, *z["keys"][0])
    c = ctx.tower(z["xe"])
    mark = np.full((batch, sizeQl, ctx.N), 0x5A5A5A5A5A5A5A5A, np.uint64)
    o0, o1 = ctx.tower(mark), ctx.tower(mark)
    ws, wsb = key.workspace(sizeQl, batch)
    assert wsb == L.fhe_bv_workspace_bytes(ctx.h, sizeQl, base_bits, batch)
    names = ("crt_digits_kernel", "bv_inner_product_kernel")
    before = [backend.launch_count(k) for k in names]

    def untouched():
        ctx.sync()
        return (np.array_equal(o0.to_host(), mark) and np.array_equal(o1.to_host(), mark) and
                [backend.launch_count(k) for k in names] == before)

    # a workspace one byte short
    assert L.fhe_keyswitch_bv(key.h, c.ptr, sizeQl, batch, o0.ptr, o1.ptr, 0, ws, wsb - 1, None) == FHE_ERR_ARG
    assert L.fhe_bv_precompute(ctx.h, c.ptr, 1, sizeQl, base_bits, batch, ws, wsb - 1, None) == FHE_ERR_ARG
    assert L.fhe_bv_fast_keyswitch(key.h, sizeQl, batch, o0.ptr, o1.ptr, 0, ws, wsb - 1, None) == FHE_ERR_ARG
    assert untouched()
    # sizeQl = sizeQ + 1
    big = ctx.malloc(L.fhe_bv_workspace_bytes(ctx.h, sizeQ, base_bits, batch) * 2)
    assert L.fhe_keyswitch_bv(key.h, c.ptr, sizeQ + 1, batch, o0.ptr, o1.ptr, 0, big, 1 << 40, None) == FHE_ERR_ARG
    assert L.fhe_bv_workspace_bytes(ctx.h, sizeQ + 1, base_bits, batch) == 0
    assert untouched()
    # a null argument
    assert L.fhe_keyswitch_bv(key.h, None, sizeQl, batch, o0.ptr, o1.ptr, 0, ws, wsb, None) == FHE_ERR_ARG
    assert L.fhe_keyswitch_bv(None, c.ptr, sizeQl, batch, o0.ptr, o1.ptr, 0, ws, wsb, None) == FHE_ERR_ARG
    assert untouched()
    # a key of another baseBits: its digits do not fit the workspace of the digits that were cut
    zeros = np.zeros((sum(windows(v, base_bits - 1) for v in z["q"]), sizeQ, ctx.N), np.uint64)
    other = fh.BvKey(ctx, sizeQ, base_bits - 1, zeros, zeros)
    assert L.fhe_bv_fast_keyswitch(other.h, sizeQl, batch, o0.ptr, o1.ptr, 0, ws, wsb, None) == FHE_ERR_ARG
    assert untouched()
    other.close()
    # baseBits = 25 on 60-bit moduli: three windows of 25 bits leave the word
    kB = np.zeros((3 * sizeQ, sizeQ, ctx.N), np.uint64)
    h = fh.vp()
    assert L.fhe_bv_key_upload(ctx.h, sizeQ, 25, kB.ctypes.data_as(fh.u64p), kB.ctypes.data_as(fh.u64p), C.byref(h)) == FHE_ERR_UNSUPPORTED
    assert not h.value
    assert L.fhe_bv_precompute(ctx.h, c.ptr, 1, sizeQl, 25, batch, big, 1 << 40, None) == FHE_ERR_UNSUPPORTED
    assert L.fhe_bv_workspace_bytes(ctx.h, sizeQl, 25, batch) == 0
    assert untouched()
    # and the same handles still work
    r0, r1 = key.KeySwitchCore(c)
    assert np.array_equal(r0.to_host(), z["want"][0][0]) and np.array_equal(r1.to_host(), z["want"][0][1])
    key.close()
    ctx.close()


# ---- 7. the BFV default path: EvalMult of the HPS family + BV relinearisation --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bfv_operands(logN, numQ, tech):
    o = libs.load_oracle()
    N = 1 << logN
    q, psiQ = hps_ref.chain(o, logN, 60, numQ)
    r, cur = [], int(q[-1])
    for _ in range(numQ):
        cur = o.orc_previous_prime(cur, 2 * N)
        r.append(cur)
    r = np.array(r, np.uint64)
    psiR = np.array([o.orc_root_of_unity(2 * N, int(v)) for v in r], np.uint64)
    rng = np.random.default_rng(4100 + tech)
    ops = [libs.rand_tower(rng, q, N, 2) for _ in range(4)]
    keys = {}
    for base_bits in (0, 10):
        D0 = sum(windows(v, base_bits) for v in q)
        keys[base_bits] = tuple(np.stack([libs.rand_tower(rng, q, N) for _ in range(D0)]) for _ in range(2))
    return q, psiQ, r, psiR, ops, keys


@pytest.mark.parametrize("base_bits", [0, 10])
@pytest.mark.parametrize("tech,drop", [(fh.HPSPOVERQ, 0), (fh.HPSPOVERQLEVELED, 0), (fh.HPSPOVERQLEVELED, 1)],
                         ids=["HPSPOVERQ", "LEVELED", "LEVELED-dropped"])
def test_bfv_eval_mult_relin(backend, oracle, tech, drop, base_bits):
    logN, numQ, t = 6, 3, 65537
    N = 1 << logN
    q, psiQ, r, psiR, ops, keys = bfv_operands(logN, numQ, tech)
    ctx = fh.Context(backend, logN, np.concatenate([q, r]), np.concatenate([psiQ, psiR]))
    plan = fh.Hps(ctx, np.arange(numQ), np.arange(numQ, 2 * numQ), t, tech)
    key = fh.BvKey(ctx, numQ, base_bits, *keys[base_bits])
    size_ql = numQ - drop
    T = [ctx.tower(x, limb_idx=np.arange(numQ)) for x in ops]
    d = [x.to_host() for x in plan.EvalMultNoRelin(*T, size_ql=size_ql, out_eval=True)]
    d2c = plan.EvalMultNoRelin(*T, size_ql=size_ql, out_eval=False)[2].to_host()
    if drop:
        assert not d2c[:, size_ql:].any(), "the product has zero rows above Q_l; the key switch still runs at numQ"
    octx = oracle.orc_ctx_create(N, numQ, q, psiQ)
    dig = digits_of(oracle, octx, d2c, base_bits)
    oracle.orc_ctx_destroy(octx)
    want0 = add_mod(d[0], exact_sums(dig, keys[base_bits][0], q), q)
    want1 = add_mod(d[1], exact_sums(dig, keys[base_bits][1], q), q)
    names = ("crt_digits_kernel", "bv_inner_product_kernel")
    before = [backend.launch_count(k) for k in names]
    c0, c1 = plan.EvalMult(key, *T, size_ql=size_ql)
    assert [backend.launch_count(k) - b for k, b in zip(names, before)] == [1, 1]
    assert np.array_equal(c0.to_host(), want0) and np.array_equal(c1.to_host(), want1)
    for x, h in zip(T, ops):
        assert np.array_equal(x.to_host(), h)
    key.close()
    plan.close()
    ctx.close()
