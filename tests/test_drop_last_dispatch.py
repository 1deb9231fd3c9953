"""Which kernels every path of the drop-the-last-limbs family launches (fhe_rescale*, fhe_mod_reduce*, fhe_rescale_multi*).

The family shares one host path; this file pins its dispatch.  Every case runs one entry point between two readings of the library's launch
counters and compares (total, the prologue instances of modes 1, 2 and 3, the epilogue instance, rescale_chain_kernel,
switch_modulus_kernel, elemwise_kernel, elemwise_cv_kernel) with EXPECTED.  The expected counts were observed on the emulator at commit
1b9191a ("CKKS rescale by several limbs in one fused pass"), before the family was collapsed into one path; a count is a condition, not a
tolerance.  Every case also compares its words with the oracle (or, for tables the reference would not produce, with the member's formula
over Python integers): a count is never the only assertion.

Shapes: 30-bit primes, sizeQl = 3 over a context of 7 limbs and batch 2 unless a case says otherwise; logN 13 is a ring of two passes, 12 the
single static pass, 8 the small-ring kernel."""
import ctypes as C

import numpy as np
import pytest

import libs
from openfhe_amd import fhe_hip as fh
from test_parity import params
from test_parity_bgv import member_formula as mod_reduce_formula
from test_parity_bgv import ref_tables as bgv_tables
from test_parity_rescale_multi import loop_of_the_reference
from test_parity_rescale_multi import member_formula as rescale_formula
from test_parity_rescale_multi import ref_tables as ckks_tables

u64p = C.POINTER(C.c_uint64)

COUNTED = ("ntt_static_kernel<PRO>", "ntt_static_kernel<PRO2>", "ntt_static_kernel<PRO3>", "ntt_static_kernel<EPI>",
           "rescale_chain_kernel", "switch_modulus_kernel", "elemwise_kernel", "elemwise_cv_kernel")
T = 65537
CTX_LIMBS = 7
SCATTERED = [5, 0, 3]  # the tower's limbs in its own order: context limb 3 is dropped

# case -> (total, PRO, PRO2, PRO3, EPI, chain, switch, elemwise, elemwise_cv)
EXPECTED = {
    "rescale-13": (4, 1, 0, 0, 1, 0, 0, 0, 0),
    "rescale-12": (3, 0, 0, 0, 1, 0, 1, 0, 0),
    "rescale-8": (4, 0, 0, 0, 0, 0, 1, 1, 0),
    "rescale_limbs-13-scattered": (4, 1, 0, 0, 1, 0, 0, 0, 0),
    "rescale_limbs-13-A-is-not-minus-B": (6, 0, 0, 0, 0, 0, 1, 1, 0),
    "rescale_limbs-13-B-doubled": (4, 1, 0, 0, 1, 0, 0, 0, 0),
    "rescale_limbs_pair-13": (4, 1, 0, 0, 1, 0, 0, 0, 0),
    "rescale_limbs_pair-8": (8, 0, 0, 0, 0, 0, 2, 2, 0),
    "mod_reduce-13": (5, 0, 1, 0, 1, 0, 0, 1, 0),
    "mod_reduce-12": (4, 0, 0, 0, 1, 0, 1, 1, 0),
    "mod_reduce-8": (5, 0, 0, 0, 0, 0, 1, 2, 0),
    "mod_reduce-13-coefficient": (3, 0, 0, 0, 0, 0, 1, 2, 0),
    "mod_reduce_limbs-13-altered-qlInvModq": (7, 0, 0, 0, 0, 0, 1, 2, 0),
    "mod_reduce_limbs-13-altered-negtInvModq": (7, 0, 0, 0, 0, 0, 1, 2, 0),
    "mod_reduce_limbs_pair-13": (5, 0, 1, 0, 1, 0, 0, 1, 0),
    "mod_reduce_limbs_pair-8": (10, 0, 0, 0, 0, 0, 2, 4, 0),
    "rescale_multi-13-one-level": (4, 1, 0, 0, 1, 0, 0, 0, 0),
    "rescale_multi-13-two-levels": (5, 0, 0, 1, 1, 1, 0, 0, 0),
    "rescale_multi-13-five-levels-two-chunks": (9, 0, 0, 2, 2, 1, 0, 0, 0),
    "rescale_multi-13-zero-scale-residue": (9, 2, 0, 0, 2, 0, 0, 1, 0),
    "rescale_multi-13-foreign-tables": (10, 1, 0, 0, 1, 0, 1, 1, 0),
}


def launches(lib):
    total = C.c_uint64(0)
    lib.L.fhe_launch_stats(None, 0, C.byref(total))
    return np.array([total.value] + [lib.launch_count(k) for k in COUNTED], np.int64)


class Ring:
    """one context of CTX_LIMBS 30-bit limbs, the oracle's context over the same limbs, and oracle contexts over sub-towers"""

    def __init__(self, lib, o, logN):
        self.lib, self.o, self.logN, self.N = lib, o, logN, 1 << logN
        self.q, self.psi = params(o, logN, CTX_LIMBS, 30)
        assert all(int(v).bit_length() == 30 for v in self.q) and len(set(int(v) for v in self.q)) == CTX_LIMBS
        self.ctx = fh.Context(lib, logN, self.q, self.psi)
        self.subs = {}

    def sub(self, limbs):
        """(moduli of the tower, oracle context over them)"""
        key = tuple(limbs)
        if key not in self.subs:
            qs = np.array([int(self.q[i]) for i in limbs], np.uint64)
            ps = np.array([int(self.psi[i]) for i in limbs], np.uint64)
            self.subs[key] = (qs, self.o.orc_ctx_create(self.N, len(limbs), qs, ps))
        return self.subs[key]

    def counted(self, fn):
        before = launches(self.lib)
        r = fn()
        return r, tuple(int(v) for v in launches(self.lib) - before)

    def close(self):
        for _, octx in self.subs.values():
            self.o.orc_ctx_destroy(octx)
        self.ctx.close()


@pytest.fixture(scope="module")
def rings(backend, oracle):
    made = {}

    def get(logN):
        if logN not in made:
            made[logN] = Ring(backend, oracle, logN)
        return made[logN]

    yield get
    for r in made.values():
        r.close()


def rescaled(r, qs, octx, x):
    """DropLastElementAndScale of every tower of x [B][n][N] by the oracle"""
    want = np.empty((x.shape[0], x.shape[1] - 1, r.N), np.uint64)
    for b in range(x.shape[0]):
        r.o.orc_drop_last_element_and_scale(octx, np.ascontiguousarray(x[b]), x.shape[1], want[b])
    return want


def mod_reduced(r, octx, x, ev):
    want = np.empty((x.shape[0], x.shape[1] - 1, r.N), np.uint64)
    for b in range(x.shape[0]):
        r.o.orc_mod_reduce(octx, np.ascontiguousarray(x[b]), x.shape[1], T, ev, want[b])
    return want


def inv_tables(qs):
    inv = [pow(int(qs[-1]) % int(qi), -1, int(qi)) for qi in qs[:-1]]
    return [(int(qi) - v) % int(qi) for v, qi in zip(inv, qs[:-1])], inv


# ---- fhe_rescale, fhe_rescale_limbs, fhe_rescale_limbs_pair ------------------------------------------------------------------------
def rescale_case(r, seed):
    qs, octx = r.sub(range(3))
    x = libs.rand_tower(np.random.default_rng(seed), qs, r.N, 2)
    xt = r.ctx.tower(x)
    got, n = r.counted(lambda: fh.rescale(r.ctx, xt))
    assert np.array_equal(got.to_host(), rescaled(r, qs, octx, x))
    return n


def rescale_limbs_case(r, tables, seed):
    """tables: 'ref' the reference's; 'foreign' A = 2 * (-q_l^-1), B = q_l^-1; 'doubled' B = 2 * q_l^-1, A = -B"""
    qs, octx = r.sub(SCATTERED)
    x = libs.rand_tower(np.random.default_rng(seed), qs, r.N, 2)
    xt = r.ctx.tower(x, SCATTERED)
    neg, inv = inv_tables(qs)
    want = rescaled(r, qs, octx, x)
    if tables == "foreign":  # x_i * inv_i + NTT(sm * 2 neg_i) = 2 * want - x_i * inv_i
        neg = [(2 * v) % int(qi) for v, qi in zip(neg, qs)]
        want = np.stack([(2 * want[:, i].astype(object) - x[:, i].astype(object) * inv[i]) % int(qs[i]) for i in range(2)], 1)
    if tables == "doubled":  # (x_i - r_i) * 2 inv_i = 2 * want
        inv = [(2 * v) % int(qi) for v, qi in zip(inv, qs)]
        neg = [(int(qi) - v) % int(qi) for v, qi in zip(inv, qs)]
        want = np.stack([(2 * want[:, i].astype(object)) % int(qs[i]) for i in range(2)], 1)
    got, n = r.counted(lambda: fh.rescale_limbs(r.ctx, xt, neg, inv))
    assert np.array_equal(got.to_host().astype(object), want.astype(object)), tables
    return n


def rescale_pair_case(r, seed):
    qs, octx = r.sub(SCATTERED)
    x = libs.rand_tower(np.random.default_rng(seed), qs, r.N, 2)
    x0, x1 = r.ctx.tower(x[0], SCATTERED), r.ctx.tower(x[1], SCATTERED)
    neg, inv = inv_tables(qs)
    (r0, r1), n = r.counted(lambda: fh.rescale_limbs_pair(r.ctx, x0, x1, neg, inv))
    want = rescaled(r, qs, octx, x)
    assert np.array_equal(r0.to_host()[0], want[0]) and np.array_equal(r1.to_host()[0], want[1])
    return n


# ---- fhe_mod_reduce, fhe_mod_reduce_limbs, fhe_mod_reduce_limbs_pair ---------------------------------------------------------------
def mod_reduce_case(r, ev, seed):
    qs, octx = r.sub(range(3))
    x = libs.rand_tower(np.random.default_rng(seed), qs, r.N, 2)
    xt = r.ctx.tower(x, fmt=fh.EVALUATION if ev else fh.COEFFICIENT)
    got, n = r.counted(lambda: fh.mod_reduce(r.ctx, xt, T))
    assert np.array_equal(got.to_host(), mod_reduced(r, octx, x, ev))
    return n


def mod_reduce_limbs_case(r, altered, seed):
    qs, octx = r.sub(range(3))
    x = libs.rand_tower(np.random.default_rng(seed), qs, r.N, 2)
    xt = r.ctx.tower(x)
    negt_inv, ql_inv = bgv_tables(qs, T)
    if altered == "qlInvModq":
        ql_inv[1] = (3 * ql_inv[1] + 1) % int(qs[1])
    else:
        negt_inv = (negt_inv + 1) % int(qs[-1])
    got, n = r.counted(lambda: fh.mod_reduce_limbs(r.ctx, xt, T, negt_inv, ql_inv))
    got = got.to_host()
    for b in range(2):
        assert np.array_equal(got[b], mod_reduce_formula(r.o, octx, qs, r.N, x[b], T, negt_inv, ql_inv, 1)), (altered, b)
    return n


def mod_reduce_pair_case(r, seed):
    qs, octx = r.sub(range(3))
    x = libs.rand_tower(np.random.default_rng(seed), qs, r.N, 2)
    x0, x1 = r.ctx.tower(x[0]), r.ctx.tower(x[1])
    negt_inv, ql_inv = bgv_tables(qs, T)
    (r0, r1), n = r.counted(lambda: fh.mod_reduce_pair(r.ctx, x0, x1, T, negt_inv, ql_inv))
    want = mod_reduced(r, octx, x, 1)
    assert np.array_equal(r0.to_host()[0], want[0]) and np.array_equal(r1.to_host()[0], want[1])
    return n


# ---- fhe_rescale_multi, fhe_rescale_multi_limbs ------------------------------------------------------------------------------------
def rescale_multi_case(r, sizeQl, levels, zero_scale, seed):
    qs, octx = r.sub(range(sizeQl))
    rng = np.random.default_rng(seed)
    x = libs.rand_tower(rng, qs, r.N, 2)
    xt = r.ctx.tower(x)
    scale = None
    if zero_scale:
        scale = np.array([int(rng.integers(1, int(q))) for q in qs], np.uint64)
        scale[1] = 0
    got, n = r.counted(lambda: fh.rescale_multi(r.ctx, xt, levels, None, scale))
    assert np.array_equal(got.to_host(), loop_of_the_reference(r.o, octx, x, levels, None, scale, qs))
    return n


def rescale_multi_foreign_case(r, seed):
    """an entry of step 1's second table altered: the member's formula with the caller's values, step by step"""
    qs, octx = r.sub(range(3))
    x = libs.rand_tower(np.random.default_rng(seed), qs, r.N, 2)
    xt = r.ctx.tower(x)
    ta, tb = ckks_tables(qs, 2)
    tb[2] = (3 * int(tb[2]) + 1) % int(qs[0])
    got, n = r.counted(lambda: fh.rescale_multi_limbs(r.ctx, xt, 2, ta, tb))
    got = got.to_host()
    for b in range(2):
        step0 = rescale_formula(r.o, octx, qs, r.N, x[b], ta[:2], tb[:2])
        assert np.array_equal(got[b], rescale_formula(r.o, octx, qs, r.N, step0, ta[2:], tb[2:])), b
    return n


CASES = {
    "rescale-13": lambda g: rescale_case(g(13), 1),
    "rescale-12": lambda g: rescale_case(g(12), 2),
    "rescale-8": lambda g: rescale_case(g(8), 3),
    "rescale_limbs-13-scattered": lambda g: rescale_limbs_case(g(13), "ref", 4),
    "rescale_limbs-13-A-is-not-minus-B": lambda g: rescale_limbs_case(g(13), "foreign", 5),
    "rescale_limbs-13-B-doubled": lambda g: rescale_limbs_case(g(13), "doubled", 6),
    "rescale_limbs_pair-13": lambda g: rescale_pair_case(g(13), 7),
    "rescale_limbs_pair-8": lambda g: rescale_pair_case(g(8), 8),
    "mod_reduce-13": lambda g: mod_reduce_case(g(13), 1, 9),
    "mod_reduce-12": lambda g: mod_reduce_case(g(12), 1, 10),
    "mod_reduce-8": lambda g: mod_reduce_case(g(8), 1, 11),
    "mod_reduce-13-coefficient": lambda g: mod_reduce_case(g(13), 0, 12),
    "mod_reduce_limbs-13-altered-qlInvModq": lambda g: mod_reduce_limbs_case(g(13), "qlInvModq", 13),
    "mod_reduce_limbs-13-altered-negtInvModq": lambda g: mod_reduce_limbs_case(g(13), "negtInvModq", 14),
    "mod_reduce_limbs_pair-13": lambda g: mod_reduce_pair_case(g(13), 15),
    "mod_reduce_limbs_pair-8": lambda g: mod_reduce_pair_case(g(8), 16),
    "rescale_multi-13-one-level": lambda g: rescale_multi_case(g(13), 3, 1, False, 17),
    "rescale_multi-13-two-levels": lambda g: rescale_multi_case(g(13), 3, 2, False, 18),
    "rescale_multi-13-five-levels-two-chunks": lambda g: rescale_multi_case(g(13), 7, 5, False, 19),
    "rescale_multi-13-zero-scale-residue": lambda g: rescale_multi_case(g(13), 3, 2, True, 20),
    "rescale_multi-13-foreign-tables": lambda g: rescale_multi_foreign_case(g(13), 21),
}


@pytest.mark.parametrize("case", list(CASES))
def test_launches_of_every_path(backend, oracle, rings, case):
    got = CASES[case](rings)
    print(f'    "{case}": {got},')
    assert got == EXPECTED[case], (case, dict(zip(("total",) + COUNTED, got)))


def test_the_members_are_the_same_launches():
    """one level without a scalar and without a level drop is fhe_rescale itself; the pair entry is the single entry over both towers"""
    assert EXPECTED["rescale_multi-13-one-level"] == EXPECTED["rescale-13"]
    assert EXPECTED["rescale_limbs_pair-13"] == EXPECTED["rescale_limbs-13-scattered"]


# ---- caches ------------------------------------------------------------------------------------------------------------------------
def free_bytes(r):
    fr, tot = C.c_size_t(0), C.c_size_t(0)
    r.lib.check(r.lib.L.fhe_mem_info(r.ctx.h, C.byref(fr), C.byref(tot)))
    return fr.value


@pytest.mark.parametrize("entry", ["fhe_rescale", "fhe_mod_reduce"])
def test_steady_state_call_allocates_nothing(backend, oracle, rings, entry):
    """the per-level tables are derived and uploaded once: between the second and a third call with the same arguments the device's free
    memory does not move (the library exposes no allocation counter; workspace and output are allocated here, once)"""
    r = rings(13)
    sizeQl = 4  # (a level no other case of this file has asked for)
    qs, octx = r.sub(range(sizeQl))
    x = libs.rand_tower(np.random.default_rng(30), qs, r.N, 1)
    xt, out = r.ctx.tower(x), r.ctx.empty(1, sizeQl - 1)
    wsb = r.lib.L.fhe_rescale_workspace_bytes(r.ctx.h, sizeQl, 1)
    ws = r.ctx.malloc(wsb)

    def call():
        if entry == "fhe_rescale":
            r.lib.check(r.lib.L.fhe_rescale(r.ctx.h, xt.ptr, sizeQl, 1, out.ptr, ws, wsb, None))
        else:
            r.lib.check(r.lib.L.fhe_mod_reduce(r.ctx.h, xt.ptr, sizeQl, T, 1, 1, out.ptr, ws, wsb, None))
        r.ctx.sync(None)

    call()
    call()
    after_second = free_bytes(r)
    call()
    assert free_bytes(r) == after_second, f"{entry}: a steady-state call allocated device memory"
    want = rescaled(r, qs, octx, x) if entry == "fhe_rescale" else mod_reduced(r, octx, x, 1)
    assert np.array_equal(out.to_host(), want)
    r.ctx.free(ws)
