"""BGV level alignment in one fused pass (fhe_mod_reduce_multi, fhe_mod_reduce_multi_limbs, fhe_mod_reduce_multi_limbs_pair).

The expected words are the steps of LeveledSHEBGVRNS::AdjustLevelsAndDepthInPlace (bgvrns-leveledshe.cpp:83-233) on one operand: the
scalar multiplied in with Python integers, rows discarded in numpy, and the oracle's restatement of DCRTPolyImpl::ModReduce
(dcrtpoly-impl.h:736-755) called step by step on the rows that are left (the oracle reads the leading sizeQl limbs of its context, which
are the moduli left at that step).  Every comparison is word for word, on every path of the dispatch: the small kernels and the single
pass (step by step), the two-pass rings with both swizzle branches of the column pass, a single kept limb, adjacent and non-adjacent
dropped rows, chunks of four, the 12-stage row passes and the 5-stage column pass."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import libs
from openfhe_amd import fhe_hip as fh
from test_parity import ckks_like_params, is_emu, params
from test_parity_bgv import member_formula, mixed_chain
from test_parity_edges import pattern

u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)

T_BIG = (1 << 40) + 15  # larger than the 25-bit limb of the mixed chain
PRO3 = "ntt_static_kernel<PRO3>"


def big_emu():
    return bool(os.environ.get("FHE_TEST_BIG_EMU"))


def unfused_env():
    return os.environ.get("FHE_MOD_REDUCE_UNFUSED", "0") != "0"


def sm(v, qs, qn):
    """centred SwitchModulus of one residue (mubintvecnat.cpp:109-122) over Python integers"""
    v = int(v)
    return (v - qs if v > qs // 2 else v) % qn


def tower_names(B):
    return tuple(("max", "mix", "uniform")[i % 3] for i in range(B)) if B > 1 else ("mix",)


def rows_of(sizeQl, levels, drop):
    return [sizeQl - 1 - k for k in range(levels)] if drop is None else list(drop)


def steps_of_the_reference(o, octx, x, qs, t, scalar, drop, n_out, ev=1):
    """x [B][sizeQl][N] over the leading limbs of octx -> [B][n_out][N]: rows times scalar, then for every row r of `drop` the rows above
    it discarded and orc_mod_reduce on the r + 1 rows that are left"""
    B, sizeQl, N = x.shape
    out = np.empty((B, n_out, N), np.uint64)
    for b in range(B):
        cur = np.ascontiguousarray(x[b])
        if scalar != 1:
            cur = np.stack([((cur[i].astype(object) * (scalar % int(qs[i]))) % int(qs[i])).astype(np.uint64) for i in range(sizeQl)])
        for r in drop:
            nxt = np.empty((r, N), np.uint64)
            o.orc_mod_reduce(octx, np.ascontiguousarray(cur[:r + 1]), r + 1, t, ev, nxt)
            cur = nxt
        out[b] = cur[:n_out]
    return out


def takes_the_fused_form(logN, ev, scalar, drop, n_out, qs):
    plain = len(drop) == 1 and scalar == 1 and n_out == drop[0]
    zero = any(scalar % int(v) == 0 for v in qs)
    return logN >= 13 and ev == 1 and not plain and not zero and not unfused_env()


def run_case(backend, o, logN, q, psi, B, t, scalar, levels, drop, n_out, seed=0, x=None, ev=1):
    N, sizeQl = 1 << logN, len(q)
    rng = np.random.default_rng(seed)
    rows = rows_of(sizeQl, levels, drop)
    n_out = rows[-1] if n_out is None else n_out
    ctx = fh.Context(backend, logN, q, psi)
    octx = o.orc_ctx_create(N, sizeQl, q, psi)
    try:
        if x is None:
            x = np.stack([pattern(rng, n, q, N) for n in tower_names(B)])
        want = steps_of_the_reference(o, octx, x, q, t, scalar, rows, n_out, ev)
        xt = ctx.tower(x, fmt=fh.EVALUATION if ev else fh.COEFFICIENT)
        before = backend.launch_count(PRO3)
        got = fh.mod_reduce_multi(ctx, xt, t, levels, scalar, drop, n_out).to_host()
        moved = backend.launch_count(PRO3) - before
        assert got.shape == want.shape and np.array_equal(got, want), f"logN={logN} sizeQl={sizeQl} t={t} s={scalar} rows={rows} nOut={n_out}"
        fused = takes_the_fused_form(logN, ev, scalar, rows, n_out, q)
        assert (moved > 0) == fused, f"prologue mode 3 ran {moved} times, fused form expected: {fused}"
    finally:
        o.orc_ctx_destroy(octx)
        ctx.close()


S60 = (1 << 59) + 12345  # a scalar that is reduced modulo no limb of the 60-bit chains in the same way

# id: (logN, sizeQl, levels, dropRows, nOut, scalar, batch, t, GPU only)
CASES = {
    # the small kernels and the single pass: step by step
    "l4-scalar1": (4, 4, 1, None, None, 3, 2, 65537, False),
    "l4-adjacent2": (4, 5, 2, None, None, S60, 2, 65537, False),
    "l4-gap1": (4, 6, 2, (5, 3), None, S60, 2, 2, False),
    "l4-gapfront": (4, 5, 1, (2,), None, 1, 1, 65537, False),
    "l4-chunks5": (4, 7, 5, None, None, 7, 1, 65537, False),
    "l12-gap2": (12, 6, 2, (5, 2), 1, S60, 2, 65537, False),
    "l12-adjacent2": (12, 4, 2, None, None, 1, 1, 2, False),
    # two-pass rings.  At 2^13 a row has two tiles: 3 kept limbs give 6 (limb, tile) groups, not a multiple of 8, 4 give 8
    "l13-k3-scalar1": (13, 4, 1, None, None, S60, 1, 65537, False),
    "l13-k3-adjacent2": (13, 5, 2, None, None, 1, 1, 65537, False),
    "l13-k3-gap1": (13, 6, 2, (5, 3), None, S60, 2, 2, False),
    "l13-k4-gap2": (13, 8, 2, (7, 4), None, S60, 3, 65537, False),
    "l13-k4-adjacent2": (13, 6, 2, None, None, S60, 1, 2, False),
    "l13-k4-gapfront": (13, 6, 1, (4,), None, 1, 1, 65537, False),
    "l13-k3-gapfront-scalar": (13, 6, 1, (3,), None, 5, 1, 65537, False),
    "l13-k1-adjacent3": (13, 4, 3, None, None, S60, 1, 65537, False),
    "l13-k1-gap1": (13, 5, 2, (4, 2), 1, 1, 2, 65537, False),
    "l13-nout-below": (13, 6, 2, (5, 4), 2, S60, 1, 65537, False),
    "l13-three-runs": (13, 7, 3, (6, 4, 2), None, S60, 1, 65537, False),
    "l13-chunks5": (13, 7, 5, None, None, S60, 2, 65537, False),
    # the 12-stage row passes and the 5-stage column pass
    "l16-gap1": (16, 4, 2, (3, 1), None, S60, 1, 65537, True),
    "l16-gap1-b4": (16, 5, 2, (4, 2), None, S60, 4, 65537, True),  # enough towers for the hand-over pair of the inverse transform
    "l17-adjacent2": (17, 4, 2, None, None, S60, 1, 65537, True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_mod_reduce_multi_cases(backend, oracle, name):
    logN, sizeQl, levels, drop, n_out, scalar, B, t, gpu_only = CASES[name]
    if gpu_only and is_emu(backend) and not big_emu():
        pytest.skip("emulator: the 12-stage row passes run on the GPU (FHE_TEST_BIG_EMU=1 runs them here too)")
    q, psi = params(oracle, logN, sizeQl)
    run_case(backend, oracle, logN, q, psi, B, t, scalar, levels, drop, n_out, 700 + logN + sizeQl)


@pytest.mark.parametrize("logN", [4, 12, 13])
def test_coefficient_towers_run_step_by_step(backend, oracle, logN):
    q, psi = params(oracle, logN, 5)
    run_case(backend, oracle, logN, q, psi, 2, 65537, S60, 2, (4, 2), None, 720 + logN, ev=0)


@pytest.mark.parametrize("logN", [4, 12, 13])
def test_t_above_a_limb_on_the_mixed_chain(backend, oracle, logN):
    """60, 25 and 50 bits: the dropped rows are switched up and down, and t exceeds the 25-bit limb"""
    q, psi = mixed_chain(oracle, logN)
    assert T_BIG > int(q[1]) and [int(v).bit_length() for v in q] == [60, 25, 50]
    for t in (T_BIG, 65537, 2):
        run_case(backend, oracle, logN, q, psi, 2, t, S60, 2, None, None, 740 + logN)
        run_case(backend, oracle, logN, q, psi, 1, t, 1, 1, (1,), None, 750 + logN)  # a gap in front, down into the 60-bit limb alone
        run_case(backend, oracle, logN, q, psi, 1, t, 3, 1, None, 1, 760 + logN)


@pytest.mark.parametrize("logN", [4, 13])
def test_zero_scalar_residue_takes_the_members_steps(backend, oracle, logN):
    """a scalar that is a multiple of one modulus: that row's words are all zero, by the member's own steps"""
    q, psi = params(oracle, logN, 5)
    run_case(backend, oracle, logN, q, psi, 1, 65537, 3 * int(q[1]), 2, None, None, 770 + logN)


def targets(q):
    h = q // 2
    return [0, 1, h, h + 1, q - 1]


def edge_tower(o, rng, octx, qs, N, t, scalar, r0, r1, names):
    """towers [len(names)][len(qs)][N], EVALUATION, for the two steps on rows r0 > r1: the other rows follow the named patterns; the two dropped
    rows are built from COEFFICIENT rows for which rho_0 AND rho_1 of the chain take 0, 1, floor(q/2), floor(q/2) + 1, q - 1 at coefficients
    0..4 and, in reverse order, at N-5..N-1 (rho_1's targets run the other way round, so that the pairs differ); checked here with Python
    integers"""
    q0, q1 = int(qs[r0]), int(qs[r1])
    sg0 = scalar % q0 * pow(t % q0, -1, q0) % q0
    sg1 = scalar % q1 * pow(t % q1, -1, q1) % q1
    t0, t1 = targets(q0), targets(q1)[::-1]
    li = lambda i: np.array([i], np.uint32).ctypes.data_as(C.c_void_p)
    x = np.stack([pattern(rng, n, qs, N) for n in names])
    for b in range(len(names)):
        e0 = rng.integers(0, q0, size=N, dtype=np.uint64)
        e1 = rng.integers(0, q1, size=N, dtype=np.uint64)
        for j in range(5):
            for pos in (j, N - 1 - j):
                e0[pos] = t0[j] * pow(sg0, -1, q0) % q0
                e1[pos] = (t1[j] * q0 + sm(t0[j], q0, q1)) * pow(sg1, -1, q1) % q1
        inv = pow(q0 % q1, -1, q1)
        pos = list(range(5)) + list(range(N - 5, N))
        rho0 = [int(e0[p]) * sg0 % q0 for p in pos]
        rho1 = [((int(e1[p]) * sg1 - sm(rho0[n], q0, q1)) * inv) % q1 for n, p in enumerate(pos)]
        assert rho0 == t0 + t0[::-1] and rho1 == t1 + t1[::-1], (rho0, rho1)
        for m, e in ((r0, e0), (r1, e1)):
            row = e.reshape(1, N).copy()
            o.orc_ntt_fwd_tower(octx, row, li(m), 1, 1, 0)
            x[b, m] = row[0]
    return x


@pytest.mark.parametrize("logN,sizeQl,drop,scalar,t", [(4, 4, (3, 2), 1, 65537), (12, 4, (3, 2), S60, 65537), (13, 5, (4, 3), 1, 2),
                                                        (13, 6, (5, 3), S60, 65537), (13, 3, (2, 1), S60, T_BIG)])
def test_rounding_edges_of_the_chain(backend, oracle, logN, sizeQl, drop, scalar, t):
    o = oracle
    q, psi = mixed_chain(o, logN) if sizeQl == 3 else params(o, logN, sizeQl)
    N = 1 << logN
    octx = o.orc_ctx_create(N, len(q), q, psi)
    x = edge_tower(o, np.random.default_rng(800 + logN), octx, q, N, t, scalar, drop[0], drop[1], ("max", "mix", "uniform"))
    o.orc_ctx_destroy(octx)
    run_case(backend, o, logN, q, psi, 3, t, scalar, 2, drop, None, 0, x)


@pytest.mark.parametrize("logN", [4, 12, 13])
def test_one_plain_level_equals_fhe_mod_reduce(backend, oracle, logN):
    o = oracle
    N, sizeQl, t = 1 << logN, 4, 65537
    q, psi = params(o, logN, sizeQl)
    ctx = fh.Context(backend, logN, q, psi)
    x = ctx.tower(libs.rand_tower(np.random.default_rng(21), q, N, 2))
    one = fh.mod_reduce(ctx, x, t).to_host()
    assert np.array_equal(fh.mod_reduce_multi(ctx, x, t).to_host(), one)
    assert np.array_equal(fh.mod_reduce_multi(ctx, x, t, 1, 1, None, 2).to_host(), one[:, :2])  # (the fused form of one level on two-pass rings)
    ctx.close()


def scattered(o, logN, backend, n):
    q, psiQ, _, _ = ckks_like_params(o, logN, 9, 2)
    ctx = fh.Context(backend, logN, q, psiQ)
    limbs = [5, 0, 3, 6, 2, 8, 1][:n]
    qs = np.array([int(q[i]) for i in limbs], np.uint64)
    sub = o.orc_ctx_create(1 << logN, n, qs, np.array([int(psiQ[i]) for i in limbs], np.uint64))
    return ctx, limbs, qs, sub


@pytest.mark.parametrize("logN,drop,gpu_only", [(8, (4, 2), False), (13, (4, 2), False), (13, (5, 4, 3), False), (17, (3, 2), True)])
def test_pair_equals_two_single_calls(backend, oracle, logN, drop, gpu_only):
    """fhe_mod_reduce_multi_limbs_pair on the two elements of a ciphertext, each a buffer of its own (in either address order), over
    scattered limbs of the context"""
    if gpu_only and is_emu(backend) and not big_emu():
        pytest.skip("emulator: the 5-stage column pass with separately allocated towers runs on the GPU; N = 2^13 covers the emulator")
    o = oracle
    rng = np.random.default_rng(67)
    N, t, scalar = 1 << logN, 65537, S60
    ctx, limbs, qs, sub = scattered(o, logN, backend, drop[0] + 2)
    h0, h1 = np.stack([pattern(rng, "max", qs, N)]), np.stack([pattern(rng, "mix", qs, N)])
    negt, inv = fh.mod_reduce_multi_tables(qs, t, drop)
    for order in (0, 1):
        if order:
            a1, a0 = ctx.tower(h1, limbs), ctx.tower(h0, limbs)
        else:
            a0, a1 = ctx.tower(h0, limbs), ctx.tower(h1, limbs)
        r0, r1 = fh.mod_reduce_multi_pair(ctx, a0, a1, t, negt, inv, scalar=scalar, drop_rows=drop)
        assert np.array_equal(r0.to_host(), fh.mod_reduce_multi_limbs(ctx, a0, t, negt, inv, scalar=scalar, drop_rows=drop).to_host())
        assert np.array_equal(r1.to_host(), fh.mod_reduce_multi_limbs(ctx, a1, t, negt, inv, scalar=scalar, drop_rows=drop).to_host())
    assert np.array_equal(r1.to_host(), steps_of_the_reference(o, sub, h1, qs, t, scalar, drop, drop[-1]))
    o.orc_ctx_destroy(sub)
    ctx.close()


@pytest.mark.parametrize("logN", [4, 13])
def test_limbs_entry_with_the_references_tables_and_with_foreign_ones(backend, oracle, logN):
    """the reference's tables take the fused form on the two-pass ring; one perturbed entry runs the member's formula with the caller's
    values, step by step (the expected words are that formula on the host)"""
    o = oracle
    rng = np.random.default_rng(71)
    N, t, drop = 1 << logN, 65537, (4, 2)
    ctx, limbs, qs, sub = scattered(o, logN, backend, 5)
    x = np.stack([pattern(rng, n, qs, N) for n in ("mix", "uniform")])
    xt = ctx.tower(x, limbs)
    negt, inv = fh.mod_reduce_multi_tables(qs, t, drop)
    before = backend.launch_count(PRO3)
    got = fh.mod_reduce_multi_limbs(ctx, xt, t, negt, inv, drop_rows=drop).to_host()
    assert (backend.launch_count(PRO3) > before) == (logN >= 13 and not unfused_env())
    assert np.array_equal(got, steps_of_the_reference(o, sub, x, qs, t, 1, drop, 2))
    for what, at in (("negtInvModq", 1), ("qlInvModq", 1), ("qlInvModq", 4 + 1)):  # step 1's negtInv, an inverse of step 0, one of step 1
        n2, i2 = negt.copy(), inv.copy()
        if what == "negtInvModq":
            n2[at] = (int(n2[at]) + 1) % int(qs[drop[at]])
        else:
            i2[at] = (3 * int(i2[at]) + 1) % int(qs[1])
        before = backend.launch_count(PRO3)
        got = fh.mod_reduce_multi_limbs(ctx, xt, t, n2, i2, drop_rows=drop).to_host()
        assert backend.launch_count(PRO3) == before, f"altered {what}: the fused form ran"
        for b in range(len(x)):
            step0 = member_formula(o, sub, qs[:5], N, x[b], t, int(n2[0]), [int(v) for v in i2[:4]], 1)
            want = member_formula(o, sub, qs[:3], N, step0[:3], t, int(n2[1]), [int(v) for v in i2[4:]], 1)
            assert np.array_equal(got[b], want), f"altered {what}[{at}], tower {b}"
    o.orc_ctx_destroy(sub)
    ctx.close()


COUNTED = (PRO3, "ntt_static_kernel<EPI>", "rescale_chain_kernel", "switch_modulus_kernel", "elemwise_kernel", "elemwise_cv_kernel")


def launches(lib):
    total = C.c_uint64(0)
    lib.L.fhe_launch_stats(None, 0, C.byref(total))
    return np.array([total.value] + [lib.launch_count(k) for k in COUNTED], np.int64)


@pytest.mark.parametrize("drop,want_total", [(None, 5), ((7,), 5), ((7, 6, 5, 4), 5), ((7, 4), 7), ((7, 6, 3), 7), ((7, 5, 3), 9)])
def test_launches_of_the_fused_form(backend, oracle, drop, want_total):
    """five launches for adjacent dropped rows, two more for every further run of adjacent rows (its inverse transform)"""
    if unfused_env():
        pytest.skip("FHE_MOD_REDUCE_UNFUSED=1: no fused form in this process")
    o = oracle
    logN, sizeQl = 13, 8
    N = 1 << logN
    q, psi = params(o, logN, sizeQl)
    ctx = fh.Context(backend, logN, q, psi)
    x = ctx.tower(libs.rand_tower(np.random.default_rng(5), q, N, 1))
    before = launches(backend)
    fh.mod_reduce_multi(ctx, x, 65537, 2, S60, drop)
    total, pro, epi, chain, sw, el, elcv = launches(backend) - before
    assert (total, pro, epi, chain) == (want_total, 1, 1, 1), (total, pro, epi, chain)
    assert sw == 0 and el + elcv == 0, "a stand-alone modulus switch or an element-wise kernel ran"
    ctx.close()


def test_argument_errors_leave_the_output_alone(backend, oracle):
    o = oracle
    logN, L, levels, t = 6, 5, 2, 65537
    N = 1 << logN
    q, psi = params(o, logN, L)
    ctx = fh.Context(backend, logN, q, psi)
    x0, x1 = ctx.tower(np.zeros((1, L, N), np.uint64)), ctx.tower(np.zeros((1, L, N), np.uint64))
    mark = np.random.default_rng(9).integers(0, 1 << 63, size=(1, L, N), dtype=np.uint64)
    o0, o1 = ctx.tower(mark), ctx.tower(mark)
    negt, inv = fh.mod_reduce_multi_tables(q, t, (4, 3))
    ap, bp = negt.ctypes.data_as(u64p), inv.ctypes.data_as(u64p)
    Lb = backend.L
    wsb = Lb.fhe_mod_reduce_multi_workspace_bytes(ctx.h, L, levels, 2)
    assert wsb > 0 and Lb.fhe_mod_reduce_multi_workspace_bytes(ctx.h, L, 0, 2) == 0 and Lb.fhe_mod_reduce_multi_workspace_bytes(ctx.h, L, L, 2) == 0
    ws = ctx.malloc(wsb)
    f, g, h = Lb.fhe_mod_reduce_multi, Lb.fhe_mod_reduce_multi_limbs, Lb.fhe_mod_reduce_multi_limbs_pair
    total = C.c_uint64(0)
    Lb.fhe_launch_stats(None, 0, C.byref(total))
    before = total.value

    def bad(status, text):
        assert status != 0 and text in Lb.fhe_last_error().decode(), (status, Lb.fhe_last_error())
        assert np.array_equal(o0.to_host(), mark) and np.array_equal(o1.to_host(), mark), "an erroneous call wrote to out"

    rows = lambda *r: np.array(r, np.uint32).ctypes.data_as(u32p)
    n = L - levels
    bad(f(ctx.h, None, L, t, 1, None, levels, n, 1, 1, o0.ptr, ws, wsb, None), "null argument")
    bad(f(ctx.h, x0.ptr, L, t, 1, None, levels, n, 1, 1, None, ws, wsb, None), "null argument")
    bad(f(ctx.h, x0.ptr, L, t, 1, None, levels, n, 1, 1, o0.ptr, None, wsb, None), "null argument")
    bad(g(ctx.h, x0.ptr, None, L, t, 1, None, levels, n, None, bp, 1, 1, o0.ptr, ws, wsb, None), "null argument")
    bad(g(ctx.h, x0.ptr, None, L, t, 1, None, levels, n, ap, None, 1, 1, o0.ptr, ws, wsb, None), "null argument")
    bad(h(ctx.h, x0.ptr, None, None, L, t, 1, None, levels, n, ap, bp, 1, o0.ptr, o1.ptr, ws, wsb, None), "null argument")
    bad(h(ctx.h, x0.ptr, x1.ptr, None, L, t, 1, None, levels, n, ap, bp, 1, o0.ptr, None, ws, wsb, None), "null argument")
    bad(h(ctx.h, x0.ptr, x0.ptr, None, L, t, 1, None, levels, n, ap, bp, 1, o0.ptr, o1.ptr, ws, wsb, None), "two distinct towers")
    bad(f(ctx.h, x0.ptr, L, t, 1, None, 0, n, 1, 1, o0.ptr, ws, wsb, None), "levels must be in [1, sizeQl)")
    bad(f(ctx.h, x0.ptr, L, t, 1, None, L, 1, 1, 1, o0.ptr, ws, wsb, None), "levels must be in [1, sizeQl)")
    bad(f(ctx.h, x0.ptr, 1, t, 1, None, 1, 1, 1, 1, o0.ptr, ws, wsb, None), "Removing last element")
    bad(f(ctx.h, x0.ptr, L + 1, t, 1, None, levels, n, 1, 1, o0.ptr, ws, wsb, None), "Removing last element")
    for r in ((3, 4), (4, 4), (5, 3), (4, 0)):  # increasing, repeated, beyond the tower, the first row
        bad(f(ctx.h, x0.ptr, L, t, 1, rows(*r), 2, 1, 1, 1, o0.ptr, ws, wsb, None), "dropRows must be strictly decreasing")
    q9, psi9 = params(o, logN, 9)
    ctx9 = fh.Context(backend, logN, q9, psi9)
    x9 = ctx9.tower(np.zeros((1, 9, N), np.uint64))
    ws9 = ctx9.malloc(Lb.fhe_mod_reduce_multi_workspace_bytes(ctx9.h, 9, 5, 1))
    bad(f(ctx9.h, x9.ptr, 9, t, 1, rows(8, 7, 6, 5, 4), 5, 1, 1, 1, o0.ptr, ws9, Lb.fhe_mod_reduce_multi_workspace_bytes(ctx9.h, 9, 5, 1), None),
        "a row list takes at most 4 levels")
    ctx9.close()
    bad(f(ctx.h, x0.ptr, L, t, 1, None, levels, 0, 1, 1, o0.ptr, ws, wsb, None), "nOut must be in [1, sizeQl - levels]")
    bad(f(ctx.h, x0.ptr, L, t, 1, None, levels, n + 1, 1, 1, o0.ptr, ws, wsb, None), "nOut must be in [1, sizeQl - levels]")
    bad(f(ctx.h, x0.ptr, L, t, 1, rows(4, 2), 2, 3, 1, 1, o0.ptr, ws, wsb, None), "nOut must be in [1, dropRows[levels - 1]]")
    far = np.array([0, 1, 2, 3, L], np.uint32)
    bad(g(ctx.h, x0.ptr, far.ctypes.data_as(u32p), L, t, 1, None, levels, n, ap, bp, 1, 1, o0.ptr, ws, wsb, None), "limb index exceeds context size")
    bad(f(ctx.h, x0.ptr, L, 1, 1, None, levels, n, 1, 1, o0.ptr, ws, wsb, None), "t must be invertible modulo the dropped limbs")
    bad(f(ctx.h, x0.ptr, L, 3 * int(q[3]), 1, None, levels, n, 1, 1, o0.ptr, ws, wsb, None), "t must be invertible modulo the dropped limbs")
    same = np.array([0, 1, 2, 1, 4], np.uint32)  # the row dropped second has the modulus of row 1
    bad(g(ctx.h, x0.ptr, same.ctypes.data_as(u32p), L, t, 1, None, levels, n, ap, bp, 1, 1, o0.ptr, ws, wsb, None),
        "the moduli of a tower must be distinct")
    n2 = negt.copy()
    n2[1] = q[3]
    bad(g(ctx.h, x0.ptr, None, L, t, 1, None, levels, n, n2.ctypes.data_as(u64p), bp, 1, 1, o0.ptr, ws, wsb, None),
        "table entry is not reduced modulo its limb")
    i2 = inv.copy()
    i2[4 + 1] = q[1]  # an entry of step 1
    bad(g(ctx.h, x0.ptr, None, L, t, 1, None, levels, n, ap, i2.ctypes.data_as(u64p), 1, 1, o0.ptr, ws, wsb, None),
        "table entry is not reduced modulo its limb")
    bad(f(ctx.h, x0.ptr, L, t, 1, None, levels, n, 1, 1, o0.ptr, ws, 8, None), "workspace too small")
    bad(f(ctx.h, x0.ptr, L, t, 1, None, levels, n, 1, 0, o0.ptr, ws, wsb, None), "workspace too small")  # (batch 0)
    bad(f(ctx.h, x0.ptr, L, t, 1, None, levels, n, 1, 1, x0.ptr, ws, wsb, None), "out must not alias x")
    bad(h(ctx.h, x0.ptr, x1.ptr, None, L, t, 1, None, levels, n, ap, bp, 1, o0.ptr, x0.ptr, ws, wsb, None), "out must not alias x")
    Lb.fhe_launch_stats(None, 0, C.byref(total))
    assert total.value == before, "an erroneous call launched a kernel"
    assert f(ctx.h, x0.ptr, L, t, 1, None, levels, n, 1, 1, o0.ptr, ws, wsb, None) == 0
    ctx.sync(None)
    assert not np.array_equal(o0.to_host()[:, :n], mark[:, :n])
    ctx.free(ws)
    ctx.close()


def test_unfused_knob_gives_the_same_words(backend):
    """FHE_MOD_REDUCE_UNFUSED is read once per process: two-pass shapes again in a child process, where every call runs the member step by
    step (run_case checks there that prologue mode 3 stays idle; the expected words are the same steps of the oracle, so fused and unfused
    words are equal)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FHE_MOD_REDUCE_UNFUSED="1")
    emu = is_emu(backend)
    sel = "test_mod_reduce_multi_cases and (l13-k3-gap1 or l13-k4-adjacent2 or l13-chunks5)"
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-p", "no:cacheprovider", "-m",
                          "not gpu" if emu else "gpu", "-k", sel if emu else f"hip and {sel}"],
                         env=env, capture_output=True, text=True, timeout=900, cwd=root)
    assert out.returncode == 0 and " passed" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
