#!/usr/bin/env python3
"""Times BV evaluation-key generation on the device: the seeded composites fhe_bv_keygen_blake2 and fhe_bv_keygen_pk_blake2 against the
same keys made member by member through entry points that existed before them, drawing from the same blake2 counters:
  secret-key form   per key fhe_automorph of the secret; per key and tower fhe_sample_uniform_blake2, fhe_sample_gaussian_blake2,
                    fhe_ntt_fwd, fhe_mul, fhe_sub, fhe_mul_const, fhe_add (KeySwitchBV::KeySwitchGenInternal, keyswitch-bv.cpp:49-103)
  public-key form   the message tower factor[d][i] * sOld[i] materialised once ([D_0][sizeQ][N], all but D_0 rows zero); per key
                    fhe_sample_ternary_blake2, two fhe_sample_gaussian_blake2, three fhe_ntt_fwd and fhe_encrypt_pk_combine with that
                    message (keyswitch-bv.cpp:162-225 as D_0 encryptions)
at BFV's benchmark shape N = 2^15, 7 limbs, digit size 0 (7 towers of 7 limbs per key half):
  relin   one relinearisation key            rot64   64 rotation keys
  pre1    one re-encryption key              pre64   64 re-encryption keys, one public key per key
Both sides run on one stream with warmed caches and are timed with events on that stream (torch.cuda.Event on the library's stream where
torch sees the device, else a host clock around a stream synchronise: --clock), alternating, `--repeats` times; the two key sets are
compared word for word inside the run (fhe_checksum of every limb row of both halves).  Also timed: the combine alone, in place, and
fhe_lincomb over the same number of slabs read and written (secret key: one call of two terms, 2 reads + 1 write; public key: one call of
two terms and one of one term, 3 reads + 2 writes).
GB/s is against the bytes the call MUST move, in slabs of nKeys * D_0 * sizeQ * N words.  Secret key: a written (1), e written (1), every
pass of its transform read + write (2 per pass), the combine 2 reads + 1 write (3).  Public key: u, e0, e1 written (3), every pass of their
transform (6 per pass), the combine 3 reads + 2 writes (5).
usage (on an MI355X): python tools/bv_keygen_bench.py [--out profiles/bv_keygen_bench.md] [--shapes relin,rot64,pre1,pre64] [--repeats 5]"""
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
from keygen_bench import KEY, SIGMA, Clock, launches, spread  # noqa: E402

vp, u64p, u32p = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
# logN, sizeQ, digit size, keys, public-key form ("tiny*": rehearsal only)
SHAPES = {"relin": (15, 7, 0, 1, False), "rot64": (15, 7, 0, 64, False), "pre1": (15, 7, 0, 1, True), "pre64": (15, 7, 0, 64, True),
          "tiny": (10, 3, 20, 3, False), "tinypre": (10, 3, 20, 3, True)}


def run_shape(lib, name, clock_kind, repeats):
    logN, sizeQ, r, K, pk_form = SHAPES[name]
    N = 1 << logN
    q, psi = lib.dcrt_chain(logN, sizeQ, 60)
    ctx = fh.Context(lib, logN, q, psi)
    L, st = lib.L, vp()
    lib.check(L.fhe_stream_create(ctx.h, C.byref(st)))
    clock = Clock(clock_kind, ctx, st)
    f = fh.bv_keygen_factors(q, r)
    D0 = len(f)
    row, tower = N, sizeQ * N  # words
    slab = K * D0 * tower
    s = ctx.sample("ternary", 1, sizeQ, generator="blake2", key=KEY, counter0=1 << 40).SwitchFormat()
    s_old = s if K > 1 or pk_form else ctx.sample("uniform", 1, sizeQ, generator="blake2", key=KEY, counter0=1 << 41)
    rots = [x for i in range(1, K // 2 + 2) for x in (i, -i)][:K] if K > 1 else None
    k_new = fh.rotation_key_indices(lib, rots, N)[0] if K > 1 and not pk_form else np.ones(K, np.uint32)
    k_old = np.ones(K, np.uint32)
    keyw = np.frombuffer(KEY, dtype="<u4").astype(np.uint32)
    kp, knp, kop = keyw.ctypes.data_as(u32p), k_new.ctypes.data_as(u32p), k_old.ctypes.data_as(u32p)
    at = lambda base, words: vp(base.value + 8 * words)
    n0c, ne = fh.bv_keygen_counters(ctx, sizeQ, r, K, 1 if pk_form else 0)
    c0, cE = 0, n0c
    own = ctx.malloc(3 * slab * 8)  # the composite's b | a | workspace, contiguous
    base = ctx.malloc(3 * slab * 8)  # the baseline's b | a | u
    tmp, perm, msg = ctx.malloc(tower * 8), ctx.malloc(tower * 8), ctx.malloc(D0 * tower * 8)
    pk = ctx.sample("uniform", 2 * K, sizeQ, generator="blake2", key=KEY, counter0=1 << 42) if pk_form else None  # p0 [K] | p1 [K]
    fac = [np.array([max(rw)], np.uint64) for rw in f]  # the one non-zero factor of tower d ...
    lim = [np.array([int(np.argmax(rw))], np.uint32) for rw in f]  # ... and its limb

    if pk_form:
        def seeded():
            lib.check(L.fhe_bv_keygen_pk_blake2(ctx.h, sizeQ, r, K, pk.ptr, at(pk.ptr, K * tower), 1, s_old.ptr, 0, 1, SIGMA, kp, c0, cE,
                                                own, at(own, slab), at(own, 2 * slab), slab * 8, st))

        def baseline():
            b, a, u = base, at(base, slab), at(base, 2 * slab)
            lib.check(L.fhe_memset_zero(ctx.h, msg, D0 * tower * 8, st))
            for d in range(D0):
                i = int(lim[d][0])
                lib.check(L.fhe_mul_const(ctx.h, at(msg, d * tower + i * row), at(s_old.ptr, i * row), fac[d].ctypes.data_as(u64p),
                                          lim[d].ctypes.data_as(u32p), 1, 1, st))
            per = D0 * N // 512  # blocks of one key's towers in a one-word-per-coefficient stream
            for k in range(K):
                o = k * D0 * tower
                lib.check(L.fhe_sample_ternary_blake2(ctx.h, at(u, o), None, sizeQ, D0, kp, c0 + k * per, st))
                lib.check(L.fhe_sample_gaussian_blake2(ctx.h, at(b, o), None, sizeQ, D0, SIGMA, kp, cE + k * per, st))
                lib.check(L.fhe_sample_gaussian_blake2(ctx.h, at(a, o), None, sizeQ, D0, SIGMA, kp, cE + ne // 2 + k * per, st))
                for x in (u, b, a):
                    lib.check(L.fhe_ntt_fwd(ctx.h, at(x, o), None, sizeQ, D0, st))
                lib.check(L.fhe_encrypt_pk_combine(ctx.h, None, sizeQ, D0, at(pk.ptr, k * tower), at(pk.ptr, (K + k) * tower), at(u, o),
                                                   at(b, o), at(a, o), msg, 1, at(b, o), at(a, o), st))

        def combine_only():  # in place on the baseline's slabs (their words no longer matter by then)
            lib.check(L.fhe_bv_keygen_pk(ctx.h, sizeQ, r, K, pk.ptr, at(pk.ptr, K * tower), 1, s_old.ptr, 1, at(base, 2 * slab), base,
                                         at(base, slab), base, at(base, slab), st))
    else:
        def seeded():
            lib.check(L.fhe_bv_keygen_blake2(ctx.h, sizeQ, r, K, knp, kop, s.ptr, s_old.ptr, 1, SIGMA, kp, c0, cE, own, at(own, slab), st))

        def baseline():
            b, a = base, at(base, slab)
            for k in range(K):
                sn = s.ptr
                if k_new[k] != 1:
                    lib.check(L.fhe_automorph(ctx.h, perm, s.ptr, int(k_new[k]), 1, None, sizeQ, 1, st))
                    sn = perm
                for d in range(D0):
                    t = k * D0 + d
                    pa, pb, i = at(a, t * tower), at(b, t * tower), int(lim[d][0])
                    lib.check(L.fhe_sample_uniform_blake2(ctx.h, pa, None, sizeQ, 1, kp, c0 + t * tower // 256, st))
                    lib.check(L.fhe_sample_gaussian_blake2(ctx.h, pb, None, sizeQ, 1, SIGMA, kp, cE + t * N // 512, st))
                    lib.check(L.fhe_ntt_fwd(ctx.h, pb, None, sizeQ, 1, st))
                    lib.check(L.fhe_mul(ctx.h, tmp, pa, sn, None, sizeQ, 1, st))
                    lib.check(L.fhe_sub(ctx.h, pb, pb, tmp, None, sizeQ, 1, st))
                    lib.check(L.fhe_mul_const(ctx.h, tmp, at(s_old.ptr, i * row), fac[d].ctypes.data_as(u64p), lim[d].ctypes.data_as(u32p), 1,
                                              1, st))
                    lib.check(L.fhe_add(ctx.h, at(pb, i * row), at(pb, i * row), tmp, lim[d].ctypes.data_as(u32p), 1, 1, st))

        def combine_only():
            lib.check(L.fhe_bv_keygen(ctx.h, sizeQ, r, K, knp, kop, s.ptr, s_old.ptr, 1, at(base, slab), base, base, st))

    ones = np.ones(2 * sizeQ, np.uint64)
    xs2, xs1 = (vp * 2)(at(base, slab), base), (vp * 1)(at(base, 2 * slab))

    def lincomb():  # the same slabs read and written: 2 + 1, and for the public-key form 1 + 1 more
        lib.check(L.fhe_lincomb(ctx.h, base, xs2, ones.ctypes.data_as(u64p), 2, None, sizeQ, K * D0, 0, st))
        if pk_form:
            lib.check(L.fhe_lincomb(ctx.h, at(base, slab), xs1, ones.ctypes.data_as(u64p), 1, None, sizeQ, K * D0, 0, st))

    n0 = launches(lib)
    seeded()
    n1 = launches(lib)
    baseline()
    n2 = launches(lib)
    ctx.sync(st)
    half = lambda p, i: fh.Tower(ctx, at(p, i * slab), K * D0, sizeQ)
    same = all(np.array_equal(ctx.checksum(half(own, i), st), ctx.checksum(half(base, i), st)) for i in (0, 1))
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
    comb_slabs = 5 if pk_form else 3
    must = ((3 + 6 * passes if pk_form else 2 + 2 * passes) + comb_slabs) * slab * 8
    ms, mb, mc, ml = (statistics.median(v) for v in (ts, tb, tc, tl))
    out = {"shape": name, "form": "public key" if pk_form else "secret key", "logN": logN, "sizeQ": sizeQ, "r": r, "D0": D0, "keys": K,
           "key_set_GB": 2 * slab * 8 / 1e9, "seeded_ms": ms, "seeded_ms_all": ts, "baseline_ms": mb, "baseline_ms_all": tb, "ratio": mb / ms,
           "beats_spread": min(tb) > max(ts), "must_move_GB": must / 1e9, "seeded_GBps": must / 1e6 / ms, "launches_seeded": n1 - n0,
           "launches_baseline": n2 - n1, "combine_ms": mc, "combine_ms_all": tc, "combine_GBps": comb_slabs * slab * 8 / 1e6 / mc,
           "lincomb_ms": ml, "lincomb_ms_all": tl, "lincomb_GBps": comb_slabs * slab * 8 / 1e6 / ml, "clock": clock_kind,
           "keys_identical": same}
    for p in (own, base, tmp, perm, msg):
        ctx.free(p)
    lib.check(L.fhe_stream_destroy(ctx.h, st))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bv_keygen_bench.md"))
    ap.add_argument("--shapes", default="relin,rot64,pre1,pre64")
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
    lines = [f"BV evaluation-key generation on the device, {lib.version()}; ms, median (min .. max) of {a.repeats} repeats, composite and "
             f"baseline alternating on one stream ({a.clock} clock), warmed; the two key sets identical word for word (fhe_checksum of every "
             "limb row of both halves)", "",
             "| shape | form | N | limbs, r, towers | keys | key set GB | seeded composite ms | member by member ms | baseline / composite | "
             "beats the spread | launches composite / baseline | must-move GB | composite GB/s |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['shape']} | {r['form']} | 2^{r['logN']} | {r['sizeQ']}, {r['r']}, {r['D0']} | {r['keys']} | "
                     f"{r['key_set_GB']:.3f} | {spread(r['seeded_ms_all'])} | {spread(r['baseline_ms_all'])} | {r['ratio']:.2f} | "
                     f"{'yes' if r['beats_spread'] else 'NO'} | {r['launches_seeded']} / {r['launches_baseline']} | {r['must_move_GB']:.3f} | "
                     f"{r['seeded_GBps']:.0f} |")
    lines += ["", "\"beats the spread\": the baseline's fastest repeat is slower than the composite's slowest.", "",
              "The combine alone, in place, against fhe_lincomb over the same number of slabs read and written (secret key 2 + 1, public key "
              "3 + 2 in two calls):", "", "| shape | combine ms | combine GB/s | fhe_lincomb ms | fhe_lincomb GB/s |", "|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['shape']} | {spread(r['combine_ms_all'])} | {r['combine_GBps']:.0f} | {spread(r['lincomb_ms_all'])} | "
                     f"{r['lincomb_GBps']:.0f} |")
    lines += ["", f"Command: `python tools/bv_keygen_bench.py --shapes {a.shapes} --repeats {a.repeats} --clock {a.clock}`", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        fo.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
