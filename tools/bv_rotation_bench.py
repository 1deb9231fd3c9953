#!/usr/bin/env python3
"""BFV rotations and relinearisation on a BV key at the shape of DESIGN 7.8 (N = 2^15, 7 Q limbs of 60 bits, batch 64), HPSPOVERQLEVELED,
for the digit sizes 0 and 20 and the levels sizeQl = 7 and 4, on one GPU:

  (a) fhe_bfv_eval_fast_rotation_bv after one fhe_bfv_fast_rotation_precompute_bv (the inner product with the output stage alone),
  (b) the whole fhe_bfv_eval_automorphism_bv,
  (c) fhe_bfv_relinearize_bv from COEFFICIENT elements,

each against the same words composed in the same process from the separate entry points: fhe_ntt_inv_oop, fhe_scale_and_round,
fhe_bv_precompute, fhe_bv_fast_keyswitch, fhe_expand_crt_basis_ql_hat, fhe_add, fhe_automorph x 2 (and fhe_ntt_fwd_oop for (c)).
Every variant is recorded once into a graph and replayed; composite and baseline alternate after warm-up, `--repeats` times, and the
table reports median and spread.  The outputs must be identical (fhe_checksum of both elements) before anything is timed.
A tool, not a test: it fails without a GPU.   python tools/bv_rotation_bench.py [--out profiles/FILE.md]
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
    ap.add_argument("--base-bits", type=int, nargs="+", default=[0, 20])
    ap.add_argument("--levels", type=int, nargs="+", default=[7, 4])
    ap.add_argument("--k", type=int, default=5, help="automorphism index")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10, help="graph launches per timed repeat")
    ap.add_argument("--out", default=None, help="write the table (markdown) to this file")
    a = ap.parse_args()
    assert a.repeats >= 5
    lib = fh.Lib()
    if "emulator" in lib.version() or lib.device_count() < 1:
        raise SystemExit("bv_rotation_bench: needs the HIP build and a GPU")
    L_ = lib.L
    logN, nQ, B, k = a.logN, a.limbs, a.batch, a.k
    N, M = 1 << logN, 2 << logN
    q = [L_.fhe_param_last_prime(60, M)]
    while len(q) < nQ:
        q.append(L_.fhe_param_previous_prime(q[-1], M))
    q = np.array(q, np.uint64)
    psi = np.array([L_.fhe_param_root_of_unity(M, int(v)) for v in q], np.uint64)
    r, psiR = lib.hps_r(logN, q, fh.HPSPOVERQLEVELED)
    ctx = fh.Context(lib, logN, np.concatenate([q, r]), np.concatenate([psi, psiR]))
    plan = fh.Hps(ctx, np.arange(nQ), np.arange(nQ, 2 * nQ), 65537, fh.HPSPOVERQLEVELED)
    st = vp()
    lib.check(L_.fhe_stream_create(ctx.h, C.byref(st)))
    rng = np.random.default_rng(11)

    def rand(rows):
        x = np.empty((rows, nQ, N), np.uint64)
        for i, qi in enumerate(q):
            x[:, i, :] = rng.integers(0, int(qi), size=(rows, N), dtype=np.uint64)
        return x

    qi_all = np.arange(nQ)
    c0, c1, d0, d1 = (ctx.tower(rand(B), limb_idx=qi_all) for _ in range(4))  # c0, c1 EVALUATION; d0, d1 and d2 = c1's words COEFFICIENT
    out = [ctx.empty(B, nQ, qi_all) for _ in range(4)]                        # composite 0 / 1, baseline 0 / 1
    coef, e0, e1 = (ctx.empty(B, nQ, qi_all) for _ in range(3))
    tower_bytes = B * nQ * N * 8
    rows = []
    for rbits in a.base_bits:
        D0 = L_.fhe_crt_decompose_towers(ctx.h, None, nQ, rbits)
        assert D0 > 0
        kb, ka = ctx.upload(rand(D0)), ctx.upload(rand(D0))
        key = vp()
        lib.check(L_.fhe_bv_key_wrap(ctx.h, nQ, rbits, kb, ka, C.byref(key)))
        for L in a.levels:
            wsb = L_.fhe_bfv_bv_workspace_bytes(plan.h, L, rbits, B)
            assert wsb > 0
            ws, wsBase = ctx.malloc(wsb), ctx.malloc(wsb)
            D = L_.fhe_crt_decompose_towers(ctx.h, None, L, rbits)
            scaled, t0, t1 = (ctx.empty(B, L) for _ in range(3))
            sr = hat = None
            if L < nQ:
                tab = plan.table("QlQHatInvModqDivqModq", L - 1).reshape(L, nQ - L + 1)
                sr = fh.ScaleAndRoundPlan(ctx, nQ - L, np.arange(L), tab, plan.table("QlQHatInvModqDivqFrac", L - 1).view(np.float64))
                hat = np.ascontiguousarray(plan.table("QlHatModq", L - 1))
            chk = lambda s: lib.check(s)

            def base_digits(x, ev):  # x [B][nQ][N] -> digits at L limbs at the start of wsBase
                if L == nQ:
                    return chk(L_.fhe_bv_precompute(ctx.h, x, ev, L, rbits, B, wsBase, wsb, st))
                if ev:
                    chk(L_.fhe_ntt_inv_oop(ctx.h, x, coef.ptr, None, nQ, B, st))
                    x = coef.ptr
                chk(L_.fhe_scale_and_round(sr.h, x, 1, scaled.ptr, B, st))
                chk(L_.fhe_bv_precompute(ctx.h, scaled.ptr, 0, L, rbits, B, wsBase, wsb, st))

            def base_switch():  # -> the two key-switch results over Q: (pointer0, pointer1)
                chk(L_.fhe_bv_fast_keyswitch(key, L, B, t0.ptr, t1.ptr, 0, wsBase, wsb, st))
                if L == nQ:
                    return t0.ptr, t1.ptr
                chk(L_.fhe_expand_crt_basis_ql_hat(ctx.h, t0.ptr, L, hat.ctypes.data_as(u64p), None, nQ, B, e0.ptr, st))
                chk(L_.fhe_expand_crt_basis_ql_hat(ctx.h, t1.ptr, L, hat.ctypes.data_as(u64p), None, nQ, B, e1.ptr, st))
                return e0.ptr, e1.ptr

            def base_rotation():
                p0, p1 = base_switch()
                chk(L_.fhe_add(ctx.h, p0, p0, c0.ptr, None, nQ, B, st))
                chk(L_.fhe_automorph(ctx.h, out[2].ptr, p0, k, 1, None, nQ, B, st))
                chk(L_.fhe_automorph(ctx.h, out[3].ptr, p1, k, 1, None, nQ, B, st))

            def base_automorphism():
                base_digits(c1.ptr, 1)
                base_rotation()

            def base_relinearize():
                base_digits(c1.ptr, 0)
                p0, p1 = base_switch()
                chk(L_.fhe_ntt_fwd_oop(ctx.h, d0.ptr, out[2].ptr, None, nQ, B, st))
                chk(L_.fhe_ntt_fwd_oop(ctx.h, d1.ptr, out[3].ptr, None, nQ, B, st))
                chk(L_.fhe_add(ctx.h, out[2].ptr, out[2].ptr, p0, None, nQ, B, st))
                chk(L_.fhe_add(ctx.h, out[3].ptr, out[3].ptr, p1, None, nQ, B, st))

            new_rotation = lambda: chk(L_.fhe_bfv_eval_fast_rotation_bv(plan.h, key, c0.ptr, k, L, B, out[0].ptr, out[1].ptr, ws, wsb, st))
            new_automorphism = lambda: chk(L_.fhe_bfv_eval_automorphism_bv(plan.h, key, c0.ptr, c1.ptr, k, L, B, out[0].ptr, out[1].ptr, ws, wsb,
                                                                           st))
            new_relinearize = lambda: chk(L_.fhe_bfv_relinearize_bv(plan.h, key, d0.ptr, d1.ptr, c1.ptr, 0, L, B, out[0].ptr, out[1].ptr, ws,
                                                                    wsb, st))
            # the digits both variants of (a) work on ((b) leaves the same ones behind, (c) cuts its own)
            chk(L_.fhe_bfv_fast_rotation_precompute_bv(plan.h, c1.ptr, L, rbits, B, ws, wsb, st))
            base_digits(c1.ptr, 1)
            row = {"baseBits": rbits, "sizeQl": L, "digits": D}
            for name, new, base in (("a", new_rotation, base_rotation), ("b", new_automorphism, base_automorphism),
                                    ("c", new_relinearize, base_relinearize)):
                for o in out:
                    chk(L_.fhe_memset_zero(ctx.h, o.ptr, tower_bytes, st))
                gn, gb = capture(lib, ctx, st, new), capture(lib, ctx, st, base)
                sums = [ctx.checksum(o, st) for o in out]
                assert np.array_equal(sums[0], sums[2]) and np.array_equal(sums[1], sums[3]), f"({name}) baseBits {rbits}, sizeQl {L}: differs"
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
            for t in (scaled, t0, t1):
                t.free()
            ctx.free(ws), ctx.free(wsBase)
        L_.fhe_bv_key_destroy(key)
        ctx.free(kb), ctx.free(ka)
    med = lambda v: float(np.median(v))
    fmt = lambda v: f"{med(v):.3f} ({min(v):.3f} .. {max(v):.3f})"
    titles = {"a": "(a) fast rotation", "b": "(b) automorphism", "c": "(c) relinearise"}
    lines = [f"BFV rotations and relinearisation on a BV key, HPSPOVERQLEVELED, N = 2^{logN}, {nQ} Q limbs of 60 bits, batch {B}, k = {k}; ms per "
             f"batch, median (min .. max) of {a.repeats} repeats of {a.inner} graph launches, composite and baseline alternating; outputs "
             "identical (fhe_checksum)", "",
             "| baseBits | sizeQl | digits | what | composite | separate entry points | baseline / composite | gain > baseline's spread |",
             "|---|---|---|---|---|---|---|---|"]
    for r_ in rows:
        for n in "abc":
            tn, tb = r_[n + "_new_ms"], r_[n + "_base_ms"]
            lines.append(f"| {r_['baseBits']} | {r_['sizeQl']} | {r_['digits']} | {titles[n]} | {fmt(tn)} | {fmt(tb)} | {med(tb) / med(tn):.3f} | "
                         f"{'yes' if med(tb) - med(tn) > max(tb) - min(tb) else 'no'} |")
    lines += ["", "Command: `python tools/bv_rotation_bench.py " + " ".join(sys.argv[1:]) + "`"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"rows": rows}))
    lib.check(L_.fhe_stream_destroy(ctx.h, st))
    plan.close()
    ctx.close()


if __name__ == "__main__":
    main()
