#!/usr/bin/env python3
"""Times encryption on the device: the seeded public-key composite fhe_encrypt_pk_blake2 (workspace behind the ciphertexts, an EVALUATION
message) against the same ciphertexts made member by member through the entry points that existed before it: three sampler calls over the
batch (fhe_sample_ternary_blake2 for v, fhe_sample_gaussian_blake2 for e0 and for e1), fhe_ntt_fwd per block, then the arithmetic of
PKERNS::EncryptZeroCore / Encrypt (rns-pke.cpp:56-70, 148-197): per ciphertext fhe_mul of v with pkB and with pkA (one key tower meets one
ciphertext per call), and over the batch fhe_mul_const by ns (left out when ns = 1, which favours the baseline: the reference multiplies
anyway), fhe_add of the products to e0 and e1, fhe_add of the message.  Shapes:
  cfg3    config 3's ring: N = 2^16, 21 limbs, batch 64, ns = 1
  small   launch-bound: N = 2^13, 3 limbs, batch 4, ns = 65537
Both sides draw from the same counters, run on one stream with warmed caches (tables, the Gaussian inversion table, code objects) and are
timed with events on that stream (torch.cuda.Event on the library's stream where torch sees the device, else a host clock around a stream
synchronise: --clock), alternating, `--repeats` times; the two results are compared word for word inside the run (fhe_checksum of every
limb row of c0 and c1).  Also timed: the combine alone (fhe_encrypt_pk_combine in place, no message: three slabs read, two written) and
fhe_lincomb of three terms over the same three slabs (three read, one written); each rate is against its own bytes.
GB/s of the composite is against the bytes the call MUST move, in slabs of batch * nLimbs * N words: v, e0, e1 written once (3), every pass
of their transform read + write (6 per pass), the combine reading v, e0, e1 and the message and writing c0, c1 (6).
usage (on an MI355X): python tools/encrypt_bench.py [--out profiles/encrypt_bench.md] [--shapes cfg3,small] [--repeats 5]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from openfhe_amd import fhe_hip as fh  # noqa: E402
from keygen_bench import Clock, launches, spread  # noqa: E402

vp, u64p, u32p = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
SHAPES = {"cfg3": (16, 21, 64, 1), "small": (13, 3, 4, 65537), "tiny": (10, 3, 4, 65537)}  # logN, limbs, batch, ns ("tiny": rehearsal only)
KEY = bytes(range(64))
SIGMA = 3.19


def run_shape(lib, name, clock_kind, repeats):
    logN, nl, B, ns = SHAPES[name]
    N = 1 << logN
    q, psi = lib.ckks_like_chain(logN, nl, 60, 59)
    ctx = fh.Context(lib, logN, q, psi)
    L, st = lib.L, vp()
    lib.check(L.fhe_stream_create(ctx.h, C.byref(st)))
    clock = Clock(clock_kind, ctx, st)
    assert (B * N) % 512 == 0  # e1's counters start on a block boundary
    # a public key made on the device (its words do not matter to the timing), and a message
    s = ctx.sample("ternary", 1, nl, generator="blake2", key=KEY, counter0=1 << 40).SwitchFormat()
    pk_a = ctx.sample("uniform", 1, nl, generator="blake2", key=KEY, counter0=1 << 41)
    pk_b = fh.public_key(ctx, s, pk_a, ctx.sample("gaussian", 1, nl, generator="blake2", key=KEY, counter0=1 << 42).SwitchFormat(), ns)
    msg = ctx.sample("uniform", B, nl, generator="blake2", key=KEY, counter0=1 << 43)
    nv, ne = fh.encrypt_counters(ctx, nl, B)
    cV, cE = 0, nv
    slab = B * nl * N  # words
    tower = nl * N
    ct = ctx.malloc(3 * slab * 8)  # c0 | c1 | workspace
    bv, be, tmp = ctx.malloc(slab * 8), ctx.malloc(2 * slab * 8), ctx.malloc(2 * slab * 8)
    keyw = np.frombuffer(KEY, dtype="<u4").astype(np.uint32)
    kp = keyw.ctypes.data_as(u32p)
    at = lambda base, words: vp(base.value + 8 * words)
    nsv = np.array([ns % int(v) for v in q], np.uint64)

    def seeded():
        lib.check(L.fhe_encrypt_pk_blake2(ctx.h, None, nl, B, pk_b.ptr, pk_a.ptr, 0, ns, SIGMA, kp, cV, cE, msg.ptr, 0, ct, at(ct, 2 * slab),
                                          slab * 8, st))

    def baseline():
        e0, e1 = be, at(be, slab)
        lib.check(L.fhe_sample_ternary_blake2(ctx.h, bv, None, nl, B, kp, cV, st))
        lib.check(L.fhe_sample_gaussian_blake2(ctx.h, e0, None, nl, B, SIGMA, kp, cE, st))
        lib.check(L.fhe_sample_gaussian_blake2(ctx.h, e1, None, nl, B, SIGMA, kp, cE + B * N // 512, st))
        for x in (bv, e0, e1):
            lib.check(L.fhe_ntt_fwd(ctx.h, x, None, nl, B, st))
        for t in range(B):
            lib.check(L.fhe_mul(ctx.h, at(tmp, t * tower), at(bv, t * tower), pk_b.ptr, None, nl, 1, st))
            lib.check(L.fhe_mul(ctx.h, at(tmp, slab + t * tower), at(bv, t * tower), pk_a.ptr, None, nl, 1, st))
        if ns != 1:
            lib.check(L.fhe_mul_const(ctx.h, e0, e0, nsv.ctypes.data_as(u64p), None, nl, B, st))
            lib.check(L.fhe_mul_const(ctx.h, e1, e1, nsv.ctypes.data_as(u64p), None, nl, B, st))
        lib.check(L.fhe_add(ctx.h, e0, tmp, e0, None, nl, B, st))
        lib.check(L.fhe_add(ctx.h, e1, at(tmp, slab), e1, None, nl, B, st))
        lib.check(L.fhe_add(ctx.h, e0, e0, msg.ptr, None, nl, B, st))

    def combine_only():  # v, e0, e1 -> e0, e1 in place on the baseline's slabs (their words no longer matter by then)
        lib.check(L.fhe_encrypt_pk_combine(ctx.h, None, nl, B, pk_b.ptr, pk_a.ptr, bv, be, at(be, slab), None, ns, be, at(be, slab), st))

    ones = np.ones(3 * nl, np.uint64)
    xs = (vp * 3)(bv, be, at(be, slab))

    def lincomb():  # three slabs read, one written
        lib.check(L.fhe_lincomb(ctx.h, tmp, xs, ones.ctypes.data_as(u64p), 3, None, nl, B, 0, st))

    # warm-up of both (tables, the Gaussian table, code objects), the launch counts, and the comparison of the two results
    seeded(), baseline()
    n0 = launches(lib)
    seeded()
    n1 = launches(lib)
    baseline()
    n2 = launches(lib)
    ctx.sync(st)
    same = np.array_equal(ctx.checksum(fh.Tower(ctx, ct, 2 * B, nl), st), ctx.checksum(fh.Tower(ctx, be, 2 * B, nl), st))
    if not same:
        raise SystemExit(f"{name}: the composite's ciphertexts differ from the member-by-member ciphertexts")
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
    must = (3 + 6 * passes + 6) * slab * 8
    ms, mb, mc, ml = (statistics.median(v) for v in (ts, tb, tc, tl))
    row = {"shape": name, "logN": logN, "limbs": nl, "batch": B, "ns": ns, "ciphertexts_GB": 2 * slab * 8 / 1e9, "seeded_ms": ms,
           "seeded_ms_all": ts, "baseline_ms": mb, "baseline_ms_all": tb, "ratio": mb / ms, "must_move_GB": must / 1e9,
           "seeded_GBps": must / 1e6 / ms, "launches_seeded": n1 - n0, "launches_baseline": n2 - n1, "combine_ms": mc, "combine_ms_all": tc,
           "combine_GBps": 5 * slab * 8 / 1e6 / mc, "lincomb_ms": ml, "lincomb_ms_all": tl, "lincomb_GBps": 4 * slab * 8 / 1e6 / ml,
           "chunk": L.fhe_encrypt_chunk(ctx.h, nl, B), "clock": clock_kind, "identical": bool(same)}
    for b in (ct, bv, be, tmp):
        ctx.free(b)
    lib.check(L.fhe_stream_destroy(ctx.h, st))
    ctx.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encrypt_bench.md"))
    ap.add_argument("--shapes", default="cfg3,small")
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
    lines = [f"Encryption on the device, {lib.version()}; ms, median (min .. max) of {a.repeats} repeats, composite and baseline alternating "
             f"on one stream ({a.clock} clock), warmed; the two sets of ciphertexts identical word for word (fhe_checksum of every limb row of "
             "c0 and c1)", "",
             "| shape | N | limbs | batch | ns | ciphertexts GB | seeded composite ms | member by member ms | baseline / composite | "
             "launches composite / baseline | must-move GB | composite GB/s |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['shape']} | 2^{r['logN']} | {r['limbs']} | {r['batch']} | {r['ns']} | {r['ciphertexts_GB']:.3f} | "
                     f"{spread(r['seeded_ms_all'])} | {spread(r['baseline_ms_all'])} | {r['ratio']:.2f} | "
                     f"{r['launches_seeded']} / {r['launches_baseline']} | {r['must_move_GB']:.3f} | {r['seeded_GBps']:.0f} |")
    lines += ["", "The combine alone (fhe_encrypt_pk_combine in place, no message: three slabs read, two written) against fhe_lincomb of three "
              "terms over the same three slabs (three read, one written); each rate against its own bytes:", "",
              "| shape | ciphertexts per workgroup | combine ms | combine GB/s | fhe_lincomb ms | fhe_lincomb GB/s |", "|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['shape']} | {r['chunk']} | {spread(r['combine_ms_all'])} | {r['combine_GBps']:.0f} | {spread(r['lincomb_ms_all'])} | "
                     f"{r['lincomb_GBps']:.0f} |")
    lines += ["", f"Command: `python tools/encrypt_bench.py --shapes {a.shapes} --repeats {a.repeats} --clock {a.clock}`", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
