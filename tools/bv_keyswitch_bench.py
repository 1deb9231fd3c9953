#!/usr/bin/env python3
"""BV key switching at config 5's shape (N = 2^15, 7 Q limbs of 60 bits, batch 64) for the digit sizes 0, 20 and 6 (7, 21 and 70
digits), on one GPU:

  (a) the composite fhe_keyswitch_bv (one inverse NTT, one crt_digits_kernel launch, one forward NTT over all digits of the batch,
      one bv_inner_product_kernel launch),
  (b) what a caller had before the composite, run on the library given with --baseline-lib (a build of the parent commit): per
      ciphertext fhe_ntt_inv_oop + fhe_crt_decompose + fhe_inner_product,
  (c) fhe_bv_precompute followed by the existing fhe_inner_product over the same digits and key towers (one launch per 8 terms):
      isolates the new inner-product kernel.

Every variant is recorded once into a graph and replayed; the variants alternate in one process after warm-up, `--repeats` times,
and the table reports median and spread.  The outputs of all variants must be identical (fhe_checksum of both elements).
--only a --no-graph runs the composite alone with plain launches: the run to put under a kernel trace for the NTT's share.
A tool, not a test: it fails without a GPU.   python tools/bv_keyswitch_bench.py [--baseline-lib PATH] [--out profiles/FILE.md]
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


def timed(lib, ctx, st, g, n, call=None):
    lib.check(lib.L.fhe_stream_sync(ctx.h, st))
    t0 = time.perf_counter()
    for _ in range(n):
        if call is not None:
            call()
        else:
            lib.check(lib.L.fhe_graph_launch(ctx.h, g, st))
    lib.check(lib.L.fhe_stream_sync(ctx.h, st))
    return (time.perf_counter() - t0) / n * 1e3


def ptrs(base, count, stride_bytes):
    a = (vp * count)()
    for i in range(count):
        a[i] = base + i * stride_bytes
    return a


class Side:
    """one library's context with the input batch, the key towers and two output towers on its device"""

    def __init__(self, lib, logN, q, psi, c_host, kb_host, ka_host):
        self.lib, self.ctx = lib, fh.Context(lib, logN, q, psi)
        self.c = self.ctx.tower(c_host)
        self.kb, self.ka = self.ctx.upload(kb_host), self.ctx.upload(ka_host)
        self.o0, self.o1 = self.c.like(), self.c.like()
        self.st = vp()
        lib.check(lib.L.fhe_stream_create(self.ctx.h, C.byref(self.st)))

    def sums(self):
        return np.concatenate([self.ctx.checksum(self.o0, self.st), self.ctx.checksum(self.o1, self.st)])

    def clear(self):
        for o in (self.o0, self.o1):
            self.lib.check(self.lib.L.fhe_memset_zero(self.ctx.h, o.ptr, o.batch * o.n_limbs * self.ctx.N * 8, self.st))

    def close(self):
        self.lib.check(self.lib.L.fhe_stream_destroy(self.ctx.h, self.st))
        self.ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logN", type=int, default=15)
    ap.add_argument("--limbs", type=int, default=7)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--base-bits", type=int, nargs="+", default=[0, 20, 6])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10, help="graph launches per timed repeat")
    ap.add_argument("--baseline-lib", default=None, help="libfhe_hip.so of the parent commit for row (b); without it the row is left out")
    ap.add_argument("--only", default=None, choices=["a"], help="run the composite alone (for a kernel trace)")
    ap.add_argument("--no-graph", action="store_true", help="plain launches instead of graph replays")
    ap.add_argument("--out", default=None, help="write the table (markdown) to this file")
    a = ap.parse_args()
    assert a.repeats >= 5 or a.only
    lib = fh.Lib()
    if "emulator" in lib.version() or lib.device_count() < 1:
        raise SystemExit("bv_keyswitch_bench: needs the HIP build and a GPU")
    old = fh.Lib(a.baseline_lib, may_lack=("fhe_bv_", "fhe_keyswitch_bv", "fhe_bfv_eval_mult_relin_hps_bv")) if a.baseline_lib and not a.only else None
    logN, nQ, B = a.logN, a.limbs, a.batch
    N, M = 1 << logN, 2 << logN
    q = [lib.L.fhe_param_last_prime(60, M)]
    while len(q) < nQ:
        q.append(lib.L.fhe_param_previous_prime(q[-1], M))
    q = np.array(q, np.uint64)
    psi = np.array([lib.L.fhe_param_root_of_unity(M, int(v)) for v in q], np.uint64)
    rng = np.random.default_rng(9)
    c_host = np.empty((B, nQ, N), np.uint64)
    for i, qi in enumerate(q):
        c_host[:, i, :] = rng.integers(0, int(qi), size=(B, N), dtype=np.uint64)
    tower_bytes, row_bytes = nQ * N * 8, N * 8
    rows = []
    for r in a.base_bits:
        probe = fh.Context(lib, logN, q, psi)
        D = lib.L.fhe_crt_decompose_towers(probe.h, None, nQ, r)
        probe.close()
        assert D > 0
        kb_host, ka_host = np.empty((D, nQ, N), np.uint64), np.empty((D, nQ, N), np.uint64)
        for k in (kb_host, ka_host):
            for i, qi in enumerate(q):
                k[:, i, :] = rng.integers(0, int(qi), size=(D, N), dtype=np.uint64)
        new = Side(lib, logN, q, psi, c_host, kb_host, ka_host)
        L_, ctx, st = lib.L, new.ctx, new.st
        key = vp()
        lib.check(L_.fhe_bv_key_wrap(ctx.h, nQ, r, new.kb, new.ka, C.byref(key)))
        wsb = L_.fhe_bv_workspace_bytes(ctx.h, nQ, r, B)
        ws = ctx.malloc(wsb)
        call_a = lambda: lib.check(L_.fhe_keyswitch_bv(key, new.c.ptr, nQ, B, new.o0.ptr, new.o1.ptr, 0, ws, wsb, st))
        if a.only:
            t = [timed(lib, ctx, st, None if a.no_graph else capture(lib, ctx, st, call_a), a.inner, call_a if a.no_graph else None)
                 for _ in range(max(a.repeats, 1))]
            print(f"baseBits {r}: D = {D}, composite {np.median(t):.3f} ms")
            L_.fhe_bv_key_destroy(key)
            new.close()
            continue
        # (c) the batched precompute, then one inner_rows_kernel launch per 8 terms over the digit-major towers
        xs, k0, k1 = ptrs(ws.value, D, B * tower_bytes), ptrs(new.kb.value, D, tower_bytes), ptrs(new.ka.value, D, tower_bytes)

        def call_c():
            lib.check(L_.fhe_bv_precompute(ctx.h, new.c.ptr, 1, nQ, r, B, ws, wsb, st))
            lib.check(L_.fhe_inner_product(ctx.h, D, xs, k0, k1, None, None, nQ, B, new.o0.ptr, new.o1.ptr, st))

        variants = [("a", lib, ctx, st, call_a, new), ("c", lib, ctx, st, call_c, new)]
        if old is not None:  # (b) per ciphertext on the parent's library
            base = Side(old, logN, q, psi, c_host, kb_host, ka_host)
            O_, octx, ost = old.L, base.ctx, base.st
            coef, dig = octx.malloc(tower_bytes), octx.malloc(D * tower_bytes)
            bx, b0, b1 = ptrs(dig.value, D, tower_bytes), ptrs(base.kb.value, D, tower_bytes), ptrs(base.ka.value, D, tower_bytes)

            def call_b():
                for b in range(B):
                    off = b * tower_bytes
                    old.check(O_.fhe_ntt_inv_oop(octx.h, base.c.ptr.value + off, coef, None, nQ, 1, ost))
                    old.check(O_.fhe_crt_decompose(octx.h, coef, None, nQ, r, dig, ost))
                    old.check(O_.fhe_inner_product(octx.h, D, bx, b0, b1, None, None, nQ, 1, base.o0.ptr.value + off, base.o1.ptr.value + off,
                                                   ost))

            variants.insert(1, ("b", old, octx, ost, call_b, base))
        graphs, sums = {}, {}
        for name, lb, cx, s, call, side in variants:
            side.clear()
            graphs[name] = capture(lb, cx, s, call)
            sums[name] = side.sums()
        for name in sums:
            assert np.array_equal(sums[name], sums["a"]), f"baseBits {r}: variant ({name}) differs from the composite"
        times = {name: [] for name, *_ in variants}
        for name, lb, cx, s, call, _ in variants:  # warm-up
            timed(lb, cx, s, graphs[name], a.inner)
        for _ in range(a.repeats):
            for name, lb, cx, s, call, _ in variants:
                times[name].append(timed(lb, cx, s, graphs[name], a.inner))
        rows.append({"baseBits": r, "digits": D, **{k + "_ms": v for k, v in times.items()}})
        for name, lb, *_ in variants:
            lb.L.fhe_graph_destroy(graphs[name])
        L_.fhe_bv_key_destroy(key)
        new.close()
        if old is not None:
            base.close()
    if a.only:
        return
    med = lambda v: float(np.median(v))
    fmt = lambda v: f"{med(v):.3f} ({min(v):.3f} .. {max(v):.3f})" if v else "not run"
    lines = [f"BV key switch, N = 2^{logN}, {nQ} Q limbs of 60 bits, batch {B}; ms per batch, median (min .. max) of {a.repeats} repeats of "
             f"{a.inner} graph launches, variants alternating; outputs identical (fhe_checksum)", "",
             "| baseBits | digits | (a) fhe_keyswitch_bv | (b) parent, per ciphertext | (c) precompute + fhe_inner_product | (b) / (a) | (c) / (a) |",
             "|---|---|---|---|---|---|---|"]
    for r_ in rows:
        ta, tb, tc = r_["a_ms"], r_.get("b_ms", []), r_["c_ms"]
        lines.append(f"| {r_['baseBits']} | {r_['digits']} | {fmt(ta)} | {fmt(tb)} | {fmt(tc)} | "
                     f"{(med(tb) / med(ta)) if tb else float('nan'):.3f} | {med(tc) / med(ta):.3f} |")
    lines += ["", "Command: `python tools/bv_keyswitch_bench.py " + " ".join(sys.argv[1:]) + "`"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"rows": rows}))


if __name__ == "__main__":
    main()
