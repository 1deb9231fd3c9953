#!/usr/bin/env python3
"""BFV rotations and relinearisation on a HYBRID key at the shape of DESIGN 7.9 (N = 2^15, 7 Q limbs of 60 bits, batch 64), dnum 3,
HPSPOVERQLEVELED, for the levels sizeQl = 7 and 4, on one GPU:

  (a) fhe_bfv_eval_fast_rotation_hybrid after one fhe_bfv_fast_rotation_precompute_hybrid (the fast key switch and the tail kernel),
  (b) the whole fhe_bfv_eval_automorphism_hybrid,
  (c) fhe_bfv_relinearize_hybrid from COEFFICIENT elements,

each against the same words composed in the same process from existing public calls: fhe_ntt_inv_oop, fhe_scale_and_round,
fhe_ntt_fwd_oop, fhe_ks_precompute, fhe_ks_fast_keyswitch, fhe_expand_crt_basis_ql_hat x 2, fhe_add, fhe_automorph x 2.
Every variant is recorded once into a graph and replayed; composite and baseline alternate after warm-up, `--repeats` times, and the
table reports median and spread.  The outputs must be identical (fhe_checksum of both elements) before anything is timed.
A tool, not a test: it fails without a GPU.   python tools/bfv_hybrid_bench.py [--out profiles/FILE.md]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openfhe_amd import fhe_hip as fh  # noqa: E402

u32p, u64p, vp = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_void_p


def capture(lib, ctx, st, call):
    call()
    lib.check(lib.L.fhe_stream_sync(ctx.h, st))
    g = vp()
    lib.check(lib.L.fhe_graph_begin(ctx.h, st))
    call()
    lib.check(lib.L.fhe_graph_end(ctx.h, st, C.byref(g)))
    return g


def timed(lib, ctx, st, g, n):
    lib.check(lib.L.fhe_stream_sync(ctx.h, st))
    t0 = time.perf_counter()
    for _ in range(n):
        lib.check(lib.L.fhe_graph_launch(ctx.h, g, st))
    lib.check(lib.L.fhe_stream_sync(ctx.h, st))
    return (time.perf_counter() - t0) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logN", type=int, default=15)
    ap.add_argument("--limbs", type=int, default=7)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--dnum", type=int, default=3)
    ap.add_argument("--levels", type=int, nargs="+", default=[7, 4])
    ap.add_argument("--k", type=int, default=5, help="automorphism index")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10, help="graph launches per timed repeat")
    ap.add_argument("--out", default=None, help="write the table (markdown) to this file")
    a = ap.parse_args()
    assert a.repeats >= 5
    lib = fh.Lib()
    if "emulator" in lib.version() or lib.device_count() < 1:
        raise SystemExit("bfv_hybrid_bench: needs the HIP build and a GPU")
    L_ = lib.L
    logN, nQ, B, k, dnum = a.logN, a.limbs, a.batch, a.k, a.dnum
    N, M = 1 << logN, 2 << logN
    q = [L_.fhe_param_last_prime(60, M)]
    while len(q) < nQ:
        q.append(L_.fhe_param_previous_prime(q[-1], M))
    q = np.array(q, np.uint64)
    psi = np.array([L_.fhe_param_root_of_unity(M, int(v)) for v in q], np.uint64)
    p, psiP = lib.select_p(logN, q, dnum)
    r, psiR = lib.hps_r(logN, q, fh.HPSPOVERQLEVELED)
    # the context: Q, then P, then the limbs of R that P does not hold (a modulus common to P and R is one limb)
    mods, psis = [int(v) for v in q] + [int(v) for v in p], [int(v) for v in psi] + [int(v) for v in psiP]
    r_idx = []
    for v, w in zip(r, psiR):
        if int(v) not in mods:
            mods.append(int(v))
            psis.append(int(w))
        r_idx.append(mods.index(int(v)))
    ctx = fh.Context(lib, logN, np.array(mods, np.uint64), np.array(psis, np.uint64))
    hps = fh.Hps(ctx, np.arange(nQ), r_idx, 65537, fh.HPSPOVERQLEVELED)
    ks = fh.KeySwitchPlan(ctx, nQ, len(p), dnum)
    plan = fh.BfvHybrid(hps, ks)
    st = vp()
    lib.check(L_.fhe_stream_create(ctx.h, C.byref(st)))
    rng = np.random.default_rng(11)

    def rand(rows, moduli):
        x = np.empty((rows, len(moduli), N), np.uint64)
        for i, qi in enumerate(moduli):
            x[:, i, :] = rng.integers(0, int(qi), size=(rows, N), dtype=np.uint64)
        return x

    qi_all = np.arange(nQ)
    c0, c1, d0, d1 = (ctx.tower(rand(B, q), limb_idx=qi_all) for _ in range(4))  # c0, c1 EVALUATION; d0, d1 and d2 = c1's words COEFFICIENT
    out = [ctx.empty(B, nQ, qi_all) for _ in range(4)]                           # composite 0 / 1, baseline 0 / 1
    coef, e0, e1 = (ctx.empty(B, nQ, qi_all) for _ in range(3))
    tower_bytes = B * nQ * N * 8
    qp = np.concatenate([q, p])
    kb, ka = ctx.upload(rand(dnum, qp)), ctx.upload(rand(dnum, qp))
    key = vp()
    lib.check(L_.fhe_ks_key_wrap(ks.h, kb, ka, C.byref(key)))
    chk = lambda s: lib.check(s)
    rows = []
    for L in a.levels:
        wsb, bwsb = L_.fhe_bfv_hybrid_workspace_bytes(plan.h, L, B), L_.fhe_ks_workspace_bytes(ks.h, L, B)
        assert wsb > 0 and bwsb > 0
        ws, wsBase = ctx.malloc(wsb), ctx.malloc(bwsb)
        scaled, se, t0, t1 = (ctx.empty(B, L) for _ in range(4))
        sr = hat = None
        if L < nQ:
            tab = hps.table("QlQHatInvModqDivqModq", L - 1).reshape(L, nQ - L + 1)
            sr = fh.ScaleAndRoundPlan(ctx, nQ - L, np.arange(L), tab, hps.table("QlQHatInvModqDivqFrac", L - 1).view(np.float64))
            hat = np.ascontiguousarray(hps.table("QlHatModq", L - 1))

        def base_digits(x, ev):  # x [B][nQ][N] -> digits at L limbs in wsBase; returns the EVALUATION tower over Q_l they were cut from
            if L == nQ and ev:
                chk(L_.fhe_ks_precompute(ks.h, x, L, B, wsBase, bwsb, st))
                return x
            if L < nQ:
                if ev:
                    chk(L_.fhe_ntt_inv_oop(ctx.h, x, coef.ptr, None, nQ, B, st))
                    x = coef.ptr
                chk(L_.fhe_scale_and_round(sr.h, x, 1, scaled.ptr, B, st))
                x = scaled.ptr
            chk(L_.fhe_ntt_fwd_oop(ctx.h, x, se.ptr, None, L, B, st))
            chk(L_.fhe_ks_precompute(ks.h, se.ptr, L, B, wsBase, bwsb, st))
            return se.ptr

        def base_switch(cin):  # -> the two key-switch results over Q: (pointer0, pointer1)
            chk(L_.fhe_ks_fast_keyswitch(ks.h, key, cin, L, B, t0.ptr, t1.ptr, wsBase, bwsb, st))
            if L == nQ:
                return t0.ptr, t1.ptr
            chk(L_.fhe_expand_crt_basis_ql_hat(ctx.h, t0.ptr, L, hat.ctypes.data_as(u64p), None, nQ, B, e0.ptr, st))
            chk(L_.fhe_expand_crt_basis_ql_hat(ctx.h, t1.ptr, L, hat.ctypes.data_as(u64p), None, nQ, B, e1.ptr, st))
            return e0.ptr, e1.ptr

        def base_rotation(cin=None):
            p0, p1 = base_switch(cin if cin is not None else (c1.ptr if L == nQ else se.ptr))
            chk(L_.fhe_add(ctx.h, p0, p0, c0.ptr, None, nQ, B, st))
            chk(L_.fhe_automorph(ctx.h, out[2].ptr, p0, k, 1, None, nQ, B, st))
            chk(L_.fhe_automorph(ctx.h, out[3].ptr, p1, k, 1, None, nQ, B, st))

        def base_automorphism():
            base_rotation(base_digits(c1.ptr, 1))

        def base_relinearize():
            p0, p1 = base_switch(base_digits(c1.ptr, 0))
            chk(L_.fhe_ntt_fwd_oop(ctx.h, d0.ptr, out[2].ptr, None, nQ, B, st))
            chk(L_.fhe_ntt_fwd_oop(ctx.h, d1.ptr, out[3].ptr, None, nQ, B, st))
            chk(L_.fhe_add(ctx.h, out[2].ptr, out[2].ptr, p0, None, nQ, B, st))
            chk(L_.fhe_add(ctx.h, out[3].ptr, out[3].ptr, p1, None, nQ, B, st))

        new_rotation = lambda: chk(L_.fhe_bfv_eval_fast_rotation_hybrid(plan.h, key, c0.ptr, c1.ptr, k, L, B, out[0].ptr, out[1].ptr, ws, wsb, st))
        new_automorphism = lambda: chk(L_.fhe_bfv_eval_automorphism_hybrid(plan.h, key, c0.ptr, c1.ptr, k, L, B, out[0].ptr, out[1].ptr, ws, wsb,
                                                                           st))
        new_relinearize = lambda: chk(L_.fhe_bfv_relinearize_hybrid(plan.h, key, d0.ptr, d1.ptr, c1.ptr, 0, L, B, out[0].ptr, out[1].ptr, ws, wsb,
                                                                    st))
        row = {"sizeQl": L, "digits": min((L + (nQ + dnum - 1) // dnum - 1) // ((nQ + dnum - 1) // dnum), dnum)}
        for name, new, base in (("a", new_rotation, base_rotation), ("b", new_automorphism, base_automorphism),
                                ("c", new_relinearize, base_relinearize)):
            if name == "a":  # the digits both variants of (a) work on ((b) and (c) cut their own)
                chk(L_.fhe_bfv_fast_rotation_precompute_hybrid(plan.h, c1.ptr, L, B, ws, wsb, st))
                base_digits(c1.ptr, 1)
            for o in out:
                chk(L_.fhe_memset_zero(ctx.h, o.ptr, tower_bytes, st))
            gn, gb = capture(lib, ctx, st, new), capture(lib, ctx, st, base)
            sums = [ctx.checksum(o, st) for o in out]
            assert np.array_equal(sums[0], sums[2]) and np.array_equal(sums[1], sums[3]), f"({name}) sizeQl {L}: differs"
            timed(lib, ctx, st, gn, a.inner), timed(lib, ctx, st, gb, a.inner)  # warm-up
            tn, tb = [], []
            for _ in range(a.repeats):
                tn.append(timed(lib, ctx, st, gn, a.inner))
                tb.append(timed(lib, ctx, st, gb, a.inner))
            row[name + "_new_ms"], row[name + "_base_ms"] = tn, tb
            L_.fhe_graph_destroy(gn), L_.fhe_graph_destroy(gb)
        rows.append(row)
        if sr is not None:
            sr.close()
        for t in (scaled, se, t0, t1):
            t.free()
        ctx.free(ws), ctx.free(wsBase)
    med = lambda v: float(np.median(v))
    fmt = lambda v: f"{med(v):.3f} ({min(v):.3f} .. {max(v):.3f})"
    titles = {"a": "(a) fast rotation", "b": "(b) automorphism", "c": "(c) relinearise"}
    lines = [f"BFV rotations and relinearisation on a HYBRID key, HPSPOVERQLEVELED, N = 2^{logN}, {nQ} Q limbs of 60 bits, {len(p)} P limbs, "
             f"dnum {dnum}, batch {B}, k = {k}; ms per batch, median (min .. max) of {a.repeats} repeats of {a.inner} graph launches, composite "
             "and baseline alternating; outputs identical (fhe_checksum)", "",
             "| sizeQl | digits | what | composite | existing public calls | baseline / composite | gain > baseline's spread |",
             "|---|---|---|---|---|---|---|"]
    for r_ in rows:
        for n in "abc":
            tn, tb = r_[n + "_new_ms"], r_[n + "_base_ms"]
            lines.append(f"| {r_['sizeQl']} | {r_['digits']} | {titles[n]} | {fmt(tn)} | {fmt(tb)} | {med(tb) / med(tn):.3f} | "
                         f"{'yes' if med(tb) - med(tn) > max(tb) - min(tb) else 'no'} |")
    lines += ["", "Command: `python tools/bfv_hybrid_bench.py " + " ".join(sys.argv[1:]) + "`"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"rows": rows}))
    L_.fhe_ks_key_destroy(key)
    lib.check(L_.fhe_stream_destroy(ctx.h, st))
    plan.close()
    ks.close()
    hps.close()
    ctx.close()


if __name__ == "__main__":
    main()
