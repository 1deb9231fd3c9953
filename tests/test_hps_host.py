"""Host side of the BFV HPS-family composite: the auxiliary basis, every derived table bit for bit against Python integers
(hps_ref.tables, the reference's big-integer formulas), the expected-value composition against the live reference, error returns."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import hps_ref
import libs
from openfhe_amd import fhe_hip as fh

TECHS = (fh.HPS, fh.HPSPOVERQ, fh.HPSPOVERQLEVELED)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("tech", TECHS)
@pytest.mark.parametrize("logN,bits,numQ", [(4, 60, 2), (10, 55, 3), (13, 60, 4), (6, 30, 5)])
def test_param_hps_r(backend, oracle, logN, bits, numQ, tech):
    o, M = oracle, 2 << logN
    q, _ = hps_ref.chain(o, logN, bits, numQ)
    r, psi = backend.hps_r(logN, q, tech)
    assert len(r) == (numQ + 1 if tech == fh.HPS else numQ)
    cur = int(q[-1])
    for j in range(len(r)):
        cur = o.orc_previous_prime(cur, M)
        assert int(r[j]) == cur and int(psi[j]) == o.orc_root_of_unity(M, cur)
    with pytest.raises(fh.FheError):
        backend.hps_r(logN, q, 0)
    with pytest.raises(fh.FheError):
        backend.hps_r(logN, q, 4)


def make_plan(lib, o, logN, bits, numQ, t, tech):
    q, psiQ = hps_ref.chain(o, logN, bits, numQ)
    r, psiR = lib.hps_r(logN, q, tech)
    ctx = fh.Context(lib, logN, np.concatenate([q, r]), np.concatenate([psiQ, psiR]))
    plan = fh.Hps(ctx, np.arange(numQ), np.arange(numQ, numQ + len(r)), t, tech)
    return q, psiQ, r, psiR, ctx, plan


@pytest.mark.parametrize("tech", TECHS)
@pytest.mark.parametrize("logN,bits,numQ,t", [(4, 60, 2, 65537), (10, 55, 3, 786433), (6, 30, 5, 65537), (13, 60, 4, 65537),
                                              (5, 60, 17, 65537), (4, 45, 1, 2)])
def test_tables_bit_for_bit(backend, oracle, logN, bits, numQ, t, tech):
    """every (table, level) of the plan equals the Python-integer value — integers and the bit patterns of the doubles —
    and the plan has no table beyond those"""
    q, _, r, _, ctx, plan = make_plan(backend, oracle, logN, bits, numQ, t, tech)
    T = hps_ref.tables(q, r, t, tech)
    assert {n for n, _ in T} <= set(fh.Hps.TABLES)
    for name in fh.Hps.TABLES:
        for level in range(numQ + 1):
            got = hps_ref.table_of(plan, name, level)
            want = T.get((name, level))
            if want is None:
                assert got is None, f"{name}({level}) is not a table of technique {tech}"
                continue
            assert got is not None and got.dtype == want.dtype and got.shape == want.shape, f"{name}({level})"
            assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), f"{name}({level}) differs"
    plan.close()
    ctx.close()


def test_tables_equal_the_references_own(backend):
    """every table of every level against what the reference's CryptoParametersBFVRNS getters returned (recorded by
    tests/golden/gen_hps_leveled.cpp for an HPSPOVERQLEVELED context with 7 limbs of 30 bits), and hps_ref.tables against the same"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_vectors_hps.npz"))
    g = lambda k: z["hpslev_" + k]
    ring, t, numQ = (int(v) for v in g("meta")[:3])
    q, psiQ, r, psiR = g("q"), g("psiQ"), g("r"), g("psiR")
    rr, pp = backend.hps_r(ring.bit_length() - 1, q, fh.HPSPOVERQLEVELED)
    assert np.array_equal(rr, r) and np.array_equal(pp, psiR)
    ctx = fh.Context(backend, ring.bit_length() - 1, np.concatenate([q, r]), np.concatenate([psiQ, psiR]))
    plan = fh.Hps(ctx, np.arange(numQ), np.arange(numQ, 2 * numQ), t, fh.HPSPOVERQLEVELED)
    T = hps_ref.tables(q, r, t, fh.HPSPOVERQLEVELED)
    recorded = {k[len("hpslev_tab_"):] for k in z.files if k.startswith("hpslev_tab_")}
    assert recorded == {f"{n}_{l}" for n, l in T}, "the recorded tables are the plan's table set"
    for name, level in T:
        want = g(f"tab_{name}_{level}")
        got = hps_ref.table_of(plan, name, level)
        assert got is not None and got.dtype == want.dtype and np.array_equal(got.view(np.uint64), want.view(np.uint64)), f"{name}({level})"
        assert np.array_equal(T[name, level].view(np.uint64), want.view(np.uint64)), f"hps_ref.tables {name}({level})"
    plan.close()
    ctx.close()


def test_composition_matches_recorded_dropped_level(oracle):
    """hps_ref.Composer at sizeQl < numQ against the reference's recorded product with a dropped level"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "ref_vectors_hps.npz"))
    g = lambda k: z["hpslev_" + k]
    ring, t, numQ, size_ql = (int(v) for v in g("meta")[:4])
    comp = hps_ref.Composer(oracle, ring, g("q"), g("psiQ"), g("r"), g("psiR"), t, fh.HPSPOVERQLEVELED)
    got = comp.eval_mult(g("a"), g("b"), size_ql)
    comp.close()
    assert np.array_equal(got, g("d"))


def _golden_module():
    spec = importlib.util.spec_from_file_location("make_golden_hps", os.path.join(ROOT, "tests", "golden", "make_golden_hps.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("tech", TECHS)
@pytest.mark.parametrize("ring,t,depth,sms", [(64, 65537, 2, 60), (1024, 786433, 3, 55)])
def test_composition_matches_live_reference(oracle, ref, ring, t, depth, sms, tech):
    """hps_ref.Composer (the expected-value generator of test_parity_hps.py) reproduces cc->EvalMultNoRelin word for word;
    the reference's Q chain is the one rebuilt from the limb count, its R basis the one fhe_param_hps_r's oracle chain gives"""
    S = _golden_module().session(ref, tech, ring, t, depth, sms)
    q, psiQ = hps_ref.chain(oracle, ring.bit_length() - 1, sms, len(S["q"]))
    assert np.array_equal(q, S["q"]) and np.array_equal(psiQ, S["psiQ"])
    comp = hps_ref.Composer(oracle, ring, S["q"], S["psiQ"], S["r"], S["psiR"], t, tech)
    got = comp.eval_mult(S["a"], S["b"])
    comp.close()
    assert np.array_equal(got, S["d"])


def total_launches(lib):
    tot = C.c_uint64(0)
    lib.L.fhe_launch_stats(None, 0, C.byref(tot))
    return tot.value


def test_error_returns(backend, oracle):
    logN, numQ, t = 4, 3, 65537
    q, psiQ = hps_ref.chain(oracle, logN, 60, numQ)
    N = 1 << logN
    for tech in TECHS:
        q, psiQ, r, psiR, ctx, plan = make_plan(backend, oracle, logN, 60, numQ, t, tech)
        x = [ctx.tower(libs.rand_tower(np.random.default_rng(1), q, N, 1), limb_idx=np.arange(numQ)) for _ in range(4)]
        before = total_launches(backend)
        for bad in (0, numQ + 1) + ((numQ - 1,) if tech != fh.HPSPOVERQLEVELED else ()):
            assert plan.workspace_bytes(bad, 1) == 0
            with pytest.raises(fh.FheError):
                plan.EvalMultNoRelin(*x, size_ql=bad)
        wsb = plan.workspace_bytes(numQ, 1)
        assert wsb > 0
        ws = ctx.malloc(wsb)
        d = [x[0].like() for _ in range(3)]
        st = backend.L.fhe_bfv_eval_mult_hps(plan.h, x[0].ptr, x[1].ptr, x[2].ptr, x[3].ptr, d[0].ptr, d[1].ptr, d[2].ptr, numQ, 0, 1,
                                             ws, wsb - 8, None)
        assert st != 0, "too small a workspace must be refused"
        assert total_launches(backend) == before, "a refused call enqueues nothing"
        ctx.free(ws)
        plan.close()
        # unknown technique, wrong size of R, too many rows
        for bad_tech, nR in ((0, len(r)), (4, len(r)), (tech, len(r) + 1)):
            with pytest.raises(fh.FheError):
                fh.Hps(ctx, np.arange(numQ), np.arange(numQ, numQ + nR) % (numQ + len(r)), t, bad_tech)
        ctx.close()
