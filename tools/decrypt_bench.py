#!/usr/bin/env python3
"""Times decryption on the device against the member-by-member sequence on the entry points that existed before it.

  combine   fhe_decrypt_core (EVALUATION output: ONE launch of decrypt_combine_kernel) against PKERNS::DecryptCore (rns-pke.cpp:199-225)
            written with the element-wise entry points: fhe_mul(b, c1, s), fhe_add(b, b, c0) and, for three elements, fhe_mul(s2, s, s),
            fhe_mul_add(b, c2, s2): 2 or 4 launches.  Those entry points meet towers of one shape, so the baseline reads the secret key
            from a slab that holds one copy of it per ciphertext, replicated OUTSIDE the timed window (a caller on the parent commit pays
            for that copy, or for one launch per ciphertext; neither is charged here, which favours the baseline).
  bfv       fhe_bfv_decrypt (the combine into the workspace, one inverse transform, the scaling kernel with the plan's tables) against
            that sequence, fhe_ntt_inv and fhe_scale_and_round_native with the caller's tables (the plan's own, read back).
Shapes:
  cfg3    config 3's ring: N = 2^16, 21 limbs, batch 64   (combine, two and three elements)
  cfg5    config 5's ring: N = 2^15, 7 limbs, batch 64    (combine and bfv)
  small   launch-bound: N = 2^13, 3 limbs, batch 4        (combine and bfv)
Both sides run on one stream with warmed caches and are timed with events on that stream (torch.cuda.Event on the library's stream where
torch sees the device, else a host clock around a stream synchronise: --clock), alternating, `--repeats` windows of `--inner` calls each;
the table holds milliseconds per call.  The two results are compared word for word inside the run (fhe_checksum of every limb row).
GB/s of the combine is against the bytes the call MUST move, in slabs of batch * nLimbs * N words: nElem read, one written (the key adds
1 / chunk of a slab and is not counted).
usage (on an MI355X): python tools/decrypt_bench.py [--out profiles/decrypt_bench.md] [--shapes cfg3,cfg5,small] [--repeats 5] [--inner 8]"""
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

vp, u64p, f64p = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double)
SHAPES = {"cfg3": (16, 21, 64, False), "cfg5": (15, 7, 64, True), "small": (13, 3, 4, True), "tiny": (10, 3, 4, True)}  # logN, limbs, batch, bfv
KEY = bytes(range(64))
T = 65537


def run_shape(lib, name, clock_kind, repeats, inner):
    logN, nl, B, with_bfv = SHAPES[name]
    N = 1 << logN
    q, psi = lib.dcrt_chain(logN, nl, 60)
    ctx = fh.Context(lib, logN, q, psi)
    L, st = lib.L, vp()
    lib.check(L.fhe_stream_create(ctx.h, C.byref(st)))
    clock = Clock(clock_kind, ctx, st)
    slab, tower = B * nl * N, nl * N  # words
    s = ctx.sample("ternary", 1, nl, generator="blake2", key=KEY, counter0=1 << 40).SwitchFormat()
    c = [ctx.sample("uniform", B, nl, generator="blake2", key=KEY, counter0=(e + 1) << 41) for e in range(3)]
    for e in c:
        e.fmt = fh.EVALUATION  # used as drawn
    s_rep, s2_rep, out_new, out_old = (ctx.empty(B, nl) for _ in range(4))
    for t in range(B):  # the baseline's copy of the key per ciphertext, made once, outside every timed window
        lib.check(L.fhe_memcpy_d2d(ctx.h, vp(s_rep.ptr.value + 8 * t * tower), s.ptr, 8 * tower, st))
    ctx.sync(st)
    rows = []

    def timed(new, old, same):
        new(), old()  # warm-up: code objects, tables
        n0 = launches(lib)
        new()
        n1 = launches(lib)
        old()
        n2 = launches(lib)
        ctx.sync(st)
        if not same():
            raise SystemExit(f"{name}: the two results differ")
        tn, to = [], []
        many = lambda f: [f() for _ in range(inner)]
        for _ in range(repeats):
            tn.append(clock.time(lambda: many(new)) / inner)
            to.append(clock.time(lambda: many(old)) / inner)
        return tn, to, n1 - n0, n2 - n1

    for n_elem in (2, 3):
        ptrs = fh._elem_ptrs(c[:n_elem])

        def combine():
            lib.check(L.fhe_decrypt_core(ctx.h, ptrs, n_elem, s.ptr, None, nl, B, None, 1, 1, 0, out_new.ptr, st))

        def members():
            lib.check(L.fhe_mul(ctx.h, out_old.ptr, c[1].ptr, s_rep.ptr, None, nl, B, st))
            lib.check(L.fhe_add(ctx.h, out_old.ptr, out_old.ptr, c[0].ptr, None, nl, B, st))
            if n_elem == 3:
                lib.check(L.fhe_mul(ctx.h, s2_rep.ptr, s_rep.ptr, s_rep.ptr, None, nl, B, st))
                lib.check(L.fhe_mul_add(ctx.h, out_old.ptr, c[2].ptr, s2_rep.ptr, None, nl, B, st))

        tn, to, ln, lo = timed(combine, members, lambda: np.array_equal(ctx.checksum(out_new, st), ctx.checksum(out_old, st)))
        must = (n_elem + 1) * slab * 8
        rows.append({"shape": name, "what": "combine", "logN": logN, "limbs": nl, "batch": B, "nElem": n_elem, "new_ms_all": tn,
                     "old_ms_all": to, "ratio": statistics.median(to) / statistics.median(tn), "launches_new": ln, "launches_old": lo,
                     "must_move_GB": must / 1e9, "new_GBps": must / 1e6 / statistics.median(tn),
                     "old_moves_slabs": 6 if n_elem == 2 else 13, "chunk": L.fhe_decrypt_chunk(ctx.h, nl, B)})
    if with_bfv:
        plan = fh.BfvDecrypt(ctx, T, fh.BfvDecrypt.HPS)
        ta, tb = plan.table("tQHatInvModqDivqModt"), plan.table("tQHatInvModqBDivqModt")
        fr, bf = plan.table("tQHatInvModqDivqFrac").view(np.float64), plan.table("tQHatInvModqBDivqFrac").view(np.float64)
        wsb = plan.workspace_bytes(B)
        ws, m_new, m_old = ctx.malloc(wsb), ctx.malloc(B * N * 8), ctx.malloc(B * N * 8)
        for n_elem in (2, 3):
            ptrs = fh._elem_ptrs(c[:n_elem])

            def composite():
                lib.check(L.fhe_bfv_decrypt(plan.h, ptrs, n_elem, s.ptr, B, m_new, ws, wsb, st))

            def members():
                lib.check(L.fhe_mul(ctx.h, out_old.ptr, c[1].ptr, s_rep.ptr, None, nl, B, st))
                lib.check(L.fhe_add(ctx.h, out_old.ptr, out_old.ptr, c[0].ptr, None, nl, B, st))
                if n_elem == 3:
                    lib.check(L.fhe_mul(ctx.h, s2_rep.ptr, s_rep.ptr, s_rep.ptr, None, nl, B, st))
                    lib.check(L.fhe_mul_add(ctx.h, out_old.ptr, c[2].ptr, s2_rep.ptr, None, nl, B, st))
                lib.check(L.fhe_ntt_inv(ctx.h, out_old.ptr, None, nl, B, st))
                lib.check(L.fhe_scale_and_round_native(ctx.h, out_old.ptr, None, nl, T, ta.ctypes.data_as(u64p), tb.ctypes.data_as(u64p),
                                                       fr.ctypes.data_as(f64p), bf.ctypes.data_as(f64p), B, m_old, st))

            same = lambda: np.array_equal(ctx.checksum(fh.Tower(ctx, m_new, B, 1), st), ctx.checksum(fh.Tower(ctx, m_old, B, 1), st))
            tn, to, ln, lo = timed(composite, members, same)
            rows.append({"shape": name, "what": "bfv", "logN": logN, "limbs": nl, "batch": B, "nElem": n_elem, "new_ms_all": tn,
                         "old_ms_all": to, "ratio": statistics.median(to) / statistics.median(tn), "launches_new": ln, "launches_old": lo})
        for b in (ws, m_new, m_old):
            ctx.free(b)
        plan.close()
    lib.check(L.fhe_stream_destroy(ctx.h, st))
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decrypt_bench.md"))
    ap.add_argument("--shapes", default="cfg3,cfg5,small")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=8, help="calls per timed window")
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
        for r in run_shape(lib, name, a.clock, a.repeats, a.inner):
            rows.append(r)
            print(json.dumps(r), flush=True)
    lines = [f"Decryption on the device, {lib.version()}; ms per call, median (min .. max) of {a.repeats} windows of {a.inner} calls, the new "
             f"entry point and the member-by-member sequence alternating on one stream ({a.clock} clock), warmed; the two results identical "
             "word for word (fhe_checksum of every limb row)", "",
             "The combine alone: `fhe_decrypt_core`, EVALUATION output, against `fhe_mul`, `fhe_add` (three elements: `fhe_mul` for s², "
             "`fhe_mul_add`) reading the key from a slab replicated per ciphertext outside the timed window:", "",
             "| shape | N | limbs | batch | nElem | ciphertexts per workgroup | combine ms | element-wise ms | element-wise / combine | "
             "launches | must-move GB | combine GB/s | slabs moved, element-wise |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in (r for r in rows if r["what"] == "combine"):
        lines.append(f"| {r['shape']} | 2^{r['logN']} | {r['limbs']} | {r['batch']} | {r['nElem']} | {r['chunk']} | {spread(r['new_ms_all'])} | "
                     f"{spread(r['old_ms_all'])} | {r['ratio']:.2f} | {r['launches_new']} / {r['launches_old']} | {r['must_move_GB']:.3f} | "
                     f"{r['new_GBps']:.0f} | {r['old_moves_slabs']} |")
    lines += ["", "BFV decryption: `fhe_bfv_decrypt` (HPS, t = 65537) against the same element-wise sequence, `fhe_ntt_inv` and "
              "`fhe_scale_and_round_native` with the caller's tables:", "",
              "| shape | N | limbs | batch | nElem | fhe_bfv_decrypt ms | member by member ms | baseline / composite | launches |",
              "|---|---|---|---|---|---|---|---|---|"]
    for r in (r for r in rows if r["what"] == "bfv"):
        lines.append(f"| {r['shape']} | 2^{r['logN']} | {r['limbs']} | {r['batch']} | {r['nElem']} | {spread(r['new_ms_all'])} | "
                     f"{spread(r['old_ms_all'])} | {r['ratio']:.2f} | {r['launches_new']} / {r['launches_old']} |")
    lines += ["", f"Command: `python tools/decrypt_bench.py --shapes {a.shapes} --repeats {a.repeats} --inner {a.inner} --clock {a.clock}`", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
