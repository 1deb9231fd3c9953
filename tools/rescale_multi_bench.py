#!/usr/bin/env python3
"""CKKS rescale by `levels` limbs on one GPU, device-resident towers of uniform residues:

  fused      one fhe_rescale_multi call (five launches for levels <= 4 on a two-pass ring)
  loop       `levels` successive fhe_rescale calls, each one limb shorter (the reference's ModReduceInternalInPlace loop,
             ckksrns-leveledshe.cpp:172-191, on the member this library already had)

both in this process on the same input, alternating.  hipEvent timing on a stream of the library: `--inner` calls between two events
(>= 20), `--repeats` repeats (>= 5) after a warm-up; the table reports the median and the spread.  Both forms must give identical towers
(fhe_checksum).  The kernels of one call come from fhe_launch_stats.  The HBM rows each form moves are counted by construction (rows_moved).

A tool, not a test: it fails without a GPU.   python tools/rescale_multi_bench.py [--levels 2,3,4] [--out profiles/FILE.md]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openfhe_amd import fhe_hip as fh  # noqa: E402

vp = C.c_void_p


class Events:
    """hipEventRecord / hipEventElapsedTime of the HIP runtime the library itself is linked against"""

    def __init__(self):
        self.rt = C.CDLL("libamdhip64.so")
        self.e0, self.e1 = vp(), vp()
        for e in (self.e0, self.e1):
            assert self.rt.hipEventCreate(C.byref(e)) == 0

    def time(self, stream, n, call):
        assert self.rt.hipEventRecord(self.e0, stream) == 0
        for _ in range(n):
            call()
        assert self.rt.hipEventRecord(self.e1, stream) == 0
        assert self.rt.hipEventSynchronize(self.e1) == 0
        ms = C.c_float()
        assert self.rt.hipEventElapsedTime(C.byref(ms), self.e0, self.e1) == 0
        return ms.value / n


def stats(lib):
    buf = C.create_string_buffer(1 << 16)
    lib.L.fhe_launch_stats(buf, len(buf), None)
    return {k: int(n) for k, n in (line.rsplit(" ", 1) for line in buf.value.decode().splitlines())}


def kernels_of(lib, call, sync):
    before = stats(lib)
    call()
    sync()
    after = stats(lib)
    return {k: v - before.get(k, 0) for k, v in after.items() if v - before.get(k, 0)}


def rows_moved(n, d):
    """rows of N words per tower that the kernels of each form read and write, every distinct row counted once per kernel that touches it
    (the d chain rows a column pass re-reads for every kept limb stay in cache: counted once).  Returns (fused, loop) as (read, written)."""
    k = n - d
    # fused: INTT of d rows (two passes), the chain in place, the column pass (d rows in, k out), the row pass (k + k of x in, k out)
    fused = (2 * d + d + d + 2 * k, 2 * d + d + k + k)
    rd = wr = 0
    for s in range(d):
        m = n - 1 - s  # kept limbs of this step: INTT of one row (two passes), column pass (1 in, m out), row pass (m + m in, m out)
        rd += 2 + 1 + 2 * m
        wr += 2 + m + m
    return fused, (rd, wr)


def chain(lib, logN, n):
    M = 2 << logN
    q = [lib.L.fhe_param_last_prime(60, M)]
    while len(q) < n:
        q.append(lib.L.fhe_param_previous_prime(q[-1], M))
    q = np.array(q, np.uint64)
    return q, np.array([lib.L.fhe_param_root_of_unity(M, int(v)) for v in q], np.uint64)


def fmt(v):
    return f"{np.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="16,24,16", help="logN,sizeQl,batch")
    ap.add_argument("--levels", default="2,3,4")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 5 and a.inner >= 20
    lib = fh.Lib()
    if "emulator" in lib.version() or lib.device_count() < 1:
        raise SystemExit("rescale_multi_bench: needs the HIP build and a GPU")
    ev = Events()
    logN, n, B = (int(v) for v in a.shape.split(","))
    q, psi = chain(lib, logN, n)
    ctx = fh.Context(lib, logN, q, psi)
    x = ctx.sample("uniform", B, n, seed=11)
    x.fmt = fh.EVALUATION  # (uniform residues: any format)
    st = vp()
    lib.check(lib.L.fhe_stream_create(ctx.h, C.byref(st)))
    sync = lambda: lib.check(lib.L.fhe_stream_sync(ctx.h, st))
    rowBytes = 8 << logN
    lines = [f"CKKS rescale by d limbs, N = 2^{logN}, sizeQl = {n}, batch {B}, uniform device-resident towers; ms per call, median "
             f"(min .. max) of {a.repeats} repeats of {a.inner} calls between two hipEvents, after a warm-up, the two forms alternating; outputs "
             "identical (fhe_checksum).  fused = one fhe_rescale_multi; loop = d successive fhe_rescale calls.  MiB: what the kernels of "
             "one call read + write by construction (every distinct row once per kernel that touches it).", "",
             "| d | fused ms | loop ms | fused / loop | fused MiB read + written | loop MiB read + written |", "|---|---|---|---|---|---|"]
    rows, kern = [], []
    for d in (int(v) for v in a.levels.split(",")):
        out = ctx.empty(B, n - d)
        wsb = lib.L.fhe_rescale_multi_workspace_bytes(ctx.h, n, d, B)
        ws = ctx.malloc(wsb)
        tmp = [ctx.empty(B, n - 1), ctx.empty(B, n - 1)]
        out2 = ctx.empty(B, n - d)
        wsb1 = lib.L.fhe_rescale_workspace_bytes(ctx.h, n, B)
        ws1 = ctx.malloc(wsb1)

        def fused():
            lib.check(lib.L.fhe_rescale_multi(ctx.h, x.ptr, n, d, n - d, None, B, out.ptr, ws, wsb, st))

        def loop():
            cur = x
            for s in range(d):
                dst = out2 if s == d - 1 else tmp[s & 1]
                lib.check(lib.L.fhe_rescale(ctx.h, cur.ptr, n - s, B, dst.ptr, ws1, wsb1, st))
                cur = dst

        forms = (("fused", fused), ("loop", loop))
        for name, f in forms:
            kern.append((d, name, kernels_of(lib, f, sync)))
        assert np.array_equal(ctx.checksum(out, st), ctx.checksum(out2, st)), f"d = {d}: the two forms differ"
        times = {name: [] for name, _ in forms}
        for name, f in forms:
            ev.time(st, a.inner, f)  # warm-up
        for _ in range(a.repeats):
            for name, f in forms:
                times[name].append(ev.time(st, a.inner, f))
        (fr, fw), (lr, lw) = rows_moved(n, d)
        mib = lambda r: r * B * rowBytes / 2**20
        tf, tl = times["fused"], times["loop"]
        lines.append(f"| {d} | {fmt(tf)} | {fmt(tl)} | {np.median(tf) / np.median(tl):.3f} | {mib(fr):.0f} + {mib(fw):.0f} | "
                     f"{mib(lr):.0f} + {mib(lw):.0f} |")
        rows.append({"d": d, "fused_ms": tf, "loop_ms": tl, "fused_rows": [fr, fw], "loop_rows": [lr, lw]})
        for t in (out, out2, tmp[0], tmp[1]):
            t.free()
        ctx.free(ws)
        ctx.free(ws1)
    lines += ["", "Kernel launches of one call (fhe_launch_stats; a labelled instance is listed with its family and once more under its label):", ""]
    for d, name, k in kern:
        lines.append(f"- d = {d} {name}: " + ", ".join(f"{c} x {kk}" for kk, c in sorted(k.items())))
    lines += ["", "Command: `python tools/rescale_multi_bench.py " + " ".join(sys.argv[1:]) + "`"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"rows": rows}))
    lib.check(lib.L.fhe_stream_destroy(ctx.h, st))
    ctx.close()


if __name__ == "__main__":
    main()
