#!/usr/bin/env python3
"""Times evaluation-key generation on the device: the seeded composite fhe_ks_keygen_hybrid_blake2 against the same keys made member by
member through the entry points that existed before it (per key fhe_automorph of the secret; per key and digit fhe_sample_uniform_blake2,
fhe_sample_gaussian_blake2, fhe_ntt_fwd, fhe_mul, fhe_sub, fhe_mul_const, fhe_add -- the steps of KeySwitchHYBRID::KeySwitchGenInternal,
keyswitch-hybrid.cpp:98-123, with ns = 1), at two shapes:
  boot    the bootstrap leg's key set: N = 2^17, 24 Q limbs, dnum 3 (P as PrecomputeCRTTables picks it: 8 limbs), 63 rotation keys
  relin   one relinearisation key at config 3's shape: N = 2^16, 21 Q limbs, dnum 3
Both sides run on one stream with warmed caches (tables, the Gaussian inversion table, code objects) and are timed with events on that
stream (torch.cuda.Event on the library's stream where torch sees the device, else a host clock around a stream synchronise: --clock), alternating, `--repeats` times;
the two key sets are compared word for word inside the run (fhe_checksum of every limb row of both slabs: the baseline draws its words
from the same counters).  Also timed: the combine alone (fhe_ks_keygen_hybrid in place) and fhe_lincomb of two terms over the same slabs,
which moves the same bytes (two reads, one write).
GB/s is against the bytes the call MUST move, counted in slabs of nKeys * dnum * (sizeQ + sizeP) * N words: a written once (1), e written
once (1), every pass of its transform read + write (2 per pass), the combine reading a and e and writing b (3).
usage (on an MI355X): python tools/keygen_bench.py [--out profiles/keygen_bench.md] [--shapes boot,relin] [--repeats 5]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openfhe_amd import fhe_hip as fh  # noqa: E402

vp, u64p, u32p = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
SHAPES = {"boot": (17, 24, 3, 63), "relin": (16, 21, 3, 1), "tiny": (10, 3, 2, 3)}  # logN, sizeQ, dnum, keys ("tiny": rehearsal only)
KEY = bytes(range(64))
SIGMA = 3.19


class Clock:
    def __init__(self, kind, ctx, st):
        self.kind, self.ctx, self.st = kind, ctx, st
        if kind == "event":
            import torch
            self.torch, self.stream = torch, torch.cuda.ExternalStream(st.value, device=torch.device("cuda", 0))

    def time(self, fn):
        """milliseconds of fn() on the stream"""
        if self.kind == "event":
            e0, e1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
            self.ctx.sync(self.st)
            e0.record(self.stream)
            fn()
            e1.record(self.stream)
            e1.synchronize()
            return e0.elapsed_time(e1)
        self.ctx.sync(self.st)
        t0 = time.perf_counter()
        fn()
        self.ctx.sync(self.st)
        return (time.perf_counter() - t0) * 1e3


def launches(lib):
    total = C.c_uint64()
    lib.L.fhe_launch_stats(None, 0, C.byref(total))
    return total.value


def spread(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"


def run_shape(lib, name, clock_kind, repeats):
    logN, sizeQ, dnum, K = SHAPES[name]
    N = 1 << logN
    q, psiQ = lib.ckks_like_chain(logN, sizeQ, 60, 59)
    p, psiP = lib.select_p(logN, q, dnum)
    sizeP, QP, alpha = len(p), sizeQ + len(p), -(-sizeQ // dnum)
    ctx = fh.Context(lib, logN, np.concatenate([q, p]), np.concatenate([psiQ, psiP]))
    plan = fh.KeySwitchPlan(ctx, sizeQ, sizeP, dnum)
    L, st = lib.L, vp()
    lib.check(L.fhe_stream_create(ctx.h, C.byref(st)))
    clock = Clock(clock_kind, ctx, st)
    qs = [int(v) for v in np.concatenate([q, p])]
    P = 1
    for v in p:
        P *= int(v)
    pmodq = np.array([P % qi for qi in qs[:sizeQ]], np.uint64)
    # secrets: a ternary s (drawn on the device), its extension, and s itself as the old key (rotation keys) / a uniform tower (relin)
    s = ctx.sample("ternary", 1, sizeQ, generator="blake2", key=KEY, counter0=1 << 40).SwitchFormat()
    s_ext = plan.extend_secret(s)
    s_old = s if K > 1 else ctx.sample("uniform", 1, sizeQ, generator="blake2", key=KEY, counter0=1 << 41)
    rots = [r for i in range(1, K // 2 + 2) for r in (i, -i)][:K] if K > 1 else None
    k_new = fh.rotation_key_indices(lib, rots, N)[0] if K > 1 else np.ones(1, np.uint32)
    k_old = np.ones(K, np.uint32)
    na, ne = plan.keygen_counters(K)
    cA, cE = 0, na
    slab = K * dnum * QP * N  # words
    bufs = {n: ctx.malloc(slab * 8) for n in ("b", "a", "bb", "ba")}
    tmp, perm = ctx.malloc(QP * N * 8), ctx.malloc(QP * N * 8)
    keyw = np.frombuffer(KEY, dtype="<u4").astype(np.uint32)
    kp, knp, kop = keyw.ctypes.data_as(u32p), k_new.ctypes.data_as(u32p), k_old.ctypes.data_as(u32p)
    at = lambda base, words: vp(base.value + 8 * words)

    def seeded():
        lib.check(L.fhe_ks_keygen_hybrid_blake2(plan.h, K, knp, kop, s_ext.ptr, s_old.ptr, 1, SIGMA, kp, cA, cE, bufs["b"], bufs["a"], st))

    def baseline():
        b, a = bufs["bb"], bufs["ba"]
        for k in range(K):
            sn = s_ext.ptr
            if k_new[k] != 1:
                lib.check(L.fhe_automorph(ctx.h, perm, s_ext.ptr, int(k_new[k]), 1, None, QP, 1, st))
                sn = perm
            for j in range(dnum):
                t = k * dnum + j
                pa, pb = at(a, t * QP * N), at(b, t * QP * N)
                lib.check(L.fhe_sample_uniform_blake2(ctx.h, pa, None, QP, 1, kp, cA + t * QP * N // 256, st))
                lib.check(L.fhe_sample_gaussian_blake2(ctx.h, pb, None, QP, 1, SIGMA, kp, cE + t * N // 512, st))
                lib.check(L.fhe_ntt_fwd(ctx.h, pb, None, QP, 1, st))
                lib.check(L.fhe_mul(ctx.h, tmp, pa, sn, None, QP, 1, st))
                lib.check(L.fhe_sub(ctx.h, pb, pb, tmp, None, QP, 1, st))
                lo, hi = alpha * j, min(alpha * (j + 1), sizeQ)
                idx = np.arange(lo, hi, dtype=np.uint32)
                lib.check(L.fhe_mul_const(ctx.h, tmp, at(s_old.ptr, lo * N), pmodq[lo:hi].ctypes.data_as(u64p), idx.ctypes.data_as(u32p),
                                          hi - lo, 1, st))
                lib.check(L.fhe_add(ctx.h, at(pb, lo * N), at(pb, lo * N), tmp, idx.ctypes.data_as(u32p), hi - lo, 1, st))

    def combine_only():  # a, e -> e in place on the baseline's slabs (their words no longer matter by then)
        lib.check(L.fhe_ks_keygen_hybrid(plan.h, K, knp, kop, s_ext.ptr, s_old.ptr, 1, bufs["ba"], bufs["bb"], bufs["bb"], st))

    ones = np.ones(2 * QP, np.uint64)
    xs = (vp * 2)(bufs["ba"], bufs["bb"])

    def lincomb():  # the same bytes: two slabs read, one written
        lib.check(L.fhe_lincomb(ctx.h, bufs["bb"], xs, ones.ctypes.data_as(u64p), 2, None, QP, K * dnum, 0, st))

    # warm-up of both (tables, the Gaussian table, code objects), the launch counts, and the comparison of the two key sets
    n0 = launches(lib)
    seeded()
    n1 = launches(lib)
    baseline()
    n2 = launches(lib)
    ctx.sync(st)
    same = all(np.array_equal(ctx.checksum(fh.Tower(ctx, bufs[x], K * dnum, QP), st), ctx.checksum(fh.Tower(ctx, bufs[y], K * dnum, QP), st))
               for x, y in (("b", "bb"), ("a", "ba")))
    if not same:
        raise SystemExit(f"{name}: the composite's keys differ from the member-by-member keys")
    ts, tb = [], []
    for _ in range(repeats):
        ts.append(clock.time(seeded))
        tb.append(clock.time(baseline))
    combine_only(), lincomb()
    tc, tl = [], []
    for _ in range(repeats):
        tc.append(clock.time(combine_only))
        tl.append(clock.time(lincomb))
    passes = 1 if logN < 13 else 2
    must = (1 + 1 + 2 * passes + 3) * slab * 8
    ms, mb, mc, ml = (statistics.median(v) for v in (ts, tb, tc, tl))
    row = {"shape": name, "logN": logN, "sizeQ": sizeQ, "sizeP": sizeP, "dnum": dnum, "keys": K, "key_set_GB": 2 * slab * 8 / 1e9,
           "seeded_ms": ms, "seeded_ms_all": ts, "baseline_ms": mb, "baseline_ms_all": tb, "ratio": mb / ms,
           "must_move_GB": must / 1e9, "seeded_GBps": must / 1e6 / ms, "launches_seeded": n1 - n0, "launches_baseline": n2 - n1,
           "combine_ms": mc, "combine_ms_all": tc, "combine_GBps": 3 * slab * 8 / 1e6 / mc, "lincomb_ms": ml, "lincomb_ms_all": tl,
           "lincomb_GBps": 3 * slab * 8 / 1e6 / ml, "clock": clock_kind, "keys_identical": same}
    for b in list(bufs.values()) + [tmp, perm]:
        ctx.free(b)
    lib.check(L.fhe_stream_destroy(ctx.h, st))
    plan.close()
    ctx.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keygen_bench.md"))
    ap.add_argument("--shapes", default="boot,relin")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--clock", choices=("auto", "event", "host"), default="auto",
                    help="event: torch.cuda.Event on the library's stream; host: a host clock around a stream synchronise; auto: events "
                         "when torch sees the device, else the host clock (the table says which)")
    ap.add_argument("--lib", default=None, help="library to load (default: the product build)")
    a = ap.parse_args()
    if a.clock != "host":  # torch's runtime is initialised before the library's
        try:
            import torch
            torch.cuda.init()
            a.clock = "event"
        except Exception as e:
            if a.clock == "event":
                raise
            print(f"no device events (torch: {e}): timing with the host clock around a stream synchronise", flush=True)
            a.clock = "host"
    lib = fh.Lib(a.lib)
    rows = []
    for name in a.shapes.split(","):
        rows.append(run_shape(lib, name, a.clock, a.repeats))
        print(json.dumps(rows[-1]), flush=True)
    lines = [f"Evaluation-key generation on the device, {lib.version()}; ms, median (min .. max) of {a.repeats} repeats, composite and "
             f"baseline alternating on one stream ({a.clock} clock), warmed; the two key sets identical word for word (fhe_checksum of every "
             "limb row of both slabs)", "",
             "| shape | N | Q + P limbs, dnum | keys | key set GB | seeded composite ms | member by member ms | baseline / composite | "
             "launches composite / baseline | must-move GB | composite GB/s |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['shape']} | 2^{r['logN']} | {r['sizeQ']} + {r['sizeP']}, {r['dnum']} | {r['keys']} | {r['key_set_GB']:.2f} | "
                     f"{spread(r['seeded_ms_all'])} | {spread(r['baseline_ms_all'])} | {r['ratio']:.2f} | "
                     f"{r['launches_seeded']} / {r['launches_baseline']} | {r['must_move_GB']:.2f} | {r['seeded_GBps']:.0f} |")
    lines += ["", "The combine alone (fhe_ks_keygen_hybrid in place) against fhe_lincomb of two terms over the same slabs (both read two slabs "
              "and write one):", "", "| shape | combine ms | combine GB/s | fhe_lincomb ms | fhe_lincomb GB/s |", "|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['shape']} | {spread(r['combine_ms_all'])} | {r['combine_GBps']:.0f} | {spread(r['lincomb_ms_all'])} | "
                     f"{r['lincomb_GBps']:.0f} |")
    lines += ["", f"Command: `python tools/keygen_bench.py --shapes {a.shapes} --repeats {a.repeats} --clock {a.clock}`", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
