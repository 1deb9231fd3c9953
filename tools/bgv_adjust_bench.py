#!/usr/bin/env python3
"""BGV level alignment (LeveledSHEBGVRNS::AdjustLevelsAndDepthInPlace on one operand) on one GPU, device-resident EVALUATION towers of
uniform residues, three plans:

  a   scalar, ModReduce                                  dropRows = [n-1]
  b   scalar, ModReduce, LevelReduce(2), ModReduce       dropRows = [n-1, n-4]
  c   ModReduce twice, no scalar                         dropRows = [n-1, n-2]

each in two forms, in this process on the same input, alternating:

  new           one fhe_mod_reduce_multi call
  composition   what a caller of the C ABI had before: fhe_mul_const over the whole tower (a, b), fhe_mod_reduce, then (b) one
                fhe_memcpy_d2d per tower to bring the n-3 rows that are left together (fhe_mod_reduce reads dense towers), and fhe_mod_reduce
                again (b, c)

hipEvent timing on a stream of the library: `--inner` calls between two events (>= 20), `--repeats` repeats (>= 5) after a warm-up; the table
reports the median and the spread.  Both forms must give identical towers (fhe_checksum).  The kernels of one call come from
fhe_launch_stats.

A tool, not a test: it fails without a GPU.   python tools/bgv_adjust_bench.py [--shape 16,8,2] [--out profiles/FILE.md]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from openfhe_amd import fhe_hip as fh  # noqa: E402
from rescale_multi_bench import Events, chain, fmt, kernels_of  # noqa: E402

vp = C.c_void_p
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
T = 65537
SCALAR = (1 << 59) + 12345


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="16,8,2", help="logN,sizeQl,batch")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 5 and a.inner >= 20
    lib = fh.Lib()
    if "emulator" in lib.version() or lib.device_count() < 1:
        raise SystemExit("bgv_adjust_bench: needs the HIP build and a GPU")
    ev = Events()
    logN, n, B = (int(v) for v in a.shape.split(","))
    assert n >= 5
    q, psi = chain(lib, logN, n)
    ctx = fh.Context(lib, logN, q, psi)
    x = ctx.sample("uniform", B, n, seed=11)
    x.fmt = fh.EVALUATION  # (uniform residues: any format)
    st = vp()
    lib.check(lib.L.fhe_stream_create(ctx.h, C.byref(st)))
    sync = lambda: lib.check(lib.L.fhe_stream_sync(ctx.h, st))
    L = lib.L
    row = 8 << logN
    consts = np.array([SCALAR % int(v) for v in q], np.uint64)
    cp = consts.ctypes.data_as(u64p)
    plans = (("a", SCALAR, [n - 1]), ("b", SCALAR, [n - 1, n - 4]), ("c", 1, [n - 1, n - 2]))
    lines = [f"BGV level alignment of one operand, N = 2^{logN}, sizeQl = {n}, batch {B}, t = {T}, uniform device-resident EVALUATION towers; ms "
             f"per call, median (min .. max) of {a.repeats} repeats of {a.inner} calls between two hipEvents, after a warm-up, the two forms "
             "alternating; outputs identical (fhe_checksum).  new = one fhe_mod_reduce_multi; composition = fhe_mul_const, fhe_mod_reduce, "
             "(b: one fhe_memcpy_d2d per tower,) fhe_mod_reduce.", "",
             "| plan | new ms | composition ms | new / composition |", "|---|---|---|---|"]
    rows, kern = [], []
    wsb = L.fhe_mod_reduce_multi_workspace_bytes(ctx.h, n, 2, B)
    ws = ctx.malloc(wsb)
    wsb1 = L.fhe_rescale_workspace_bytes(ctx.h, n, B)
    ws1 = ctx.malloc(wsb1)
    scaled, step = ctx.empty(B, n), ctx.empty(B, n - 1)
    dense = ctx.empty(B, n - 3)
    for name, scalar, drop in plans:
        n_out = drop[-1]
        dr = np.array(drop, np.uint32)
        out, out2 = ctx.empty(B, n_out), ctx.empty(B, n_out)

        def new():
            lib.check(L.fhe_mod_reduce_multi(ctx.h, x.ptr, n, T, scalar, dr.ctypes.data_as(u32p), len(drop), n_out, 1, B, out.ptr, ws, wsb, st))

        def composition():
            cur = x
            if scalar != 1:
                lib.check(L.fhe_mul_const(ctx.h, scaled.ptr, x.ptr, cp, None, n, B, st))
                cur = scaled
            last = len(drop) == 1
            lib.check(L.fhe_mod_reduce(ctx.h, cur.ptr, n, T, 1, B, (out2 if last else step).ptr, ws1, wsb1, st))
            if last:
                return
            cur, rows_left = step, drop[1] + 1
            if rows_left != n - 1:  # LevelReduce: the rows that are left of every tower, brought together
                for b in range(B):
                    lib.check(L.fhe_memcpy_d2d(ctx.h, vp(dense.ptr.value + b * rows_left * row), vp(step.ptr.value + b * (n - 1) * row),
                                               rows_left * row, st))
                cur = dense
            lib.check(L.fhe_mod_reduce(ctx.h, cur.ptr, rows_left, T, 1, B, out2.ptr, ws1, wsb1, st))

        forms = (("new", new), ("composition", composition))
        for form, f in forms:
            kern.append((name, form, kernels_of(lib, f, sync)))
        assert np.array_equal(ctx.checksum(out, st), ctx.checksum(out2, st)), f"plan {name}: the two forms differ"
        times = {form: [] for form, _ in forms}
        for form, f in forms:
            ev.time(st, a.inner, f)  # warm-up
        for _ in range(a.repeats):
            for form, f in forms:
                times[form].append(ev.time(st, a.inner, f))
        tn, tc = times["new"], times["composition"]
        lines.append(f"| {name} | {fmt(tn)} | {fmt(tc)} | {np.median(tn) / np.median(tc):.3f} |")
        rows.append({"plan": name, "new_ms": tn, "composition_ms": tc})
        out.free(), out2.free()
    lines += ["", "Kernel launches of one call (fhe_launch_stats; a labelled instance is listed with its family and once more under its label):", ""]
    for name, form, k in kern:
        lines.append(f"- {name} {form}: " + ", ".join(f"{c} x {kk}" for kk, c in sorted(k.items())))
    lines += ["", "Command: `python tools/bgv_adjust_bench.py " + " ".join(sys.argv[1:]) + "`"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"shape": [logN, n, B], "rows": rows}))
    lib.check(L.fhe_stream_destroy(ctx.h, st))
    ctx.close()


if __name__ == "__main__":
    main()
