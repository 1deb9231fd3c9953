#!/usr/bin/env python3
"""EVALUATION fhe_mod_reduce (DCRTPoly::ModReduce, BGV's modulus switch) on one GPU, device-resident towers of uniform residues:

  N = 2^16, sizeQl = 21, batch 64   and   N = 2^15, sizeQl = 8, batch 256

on this build and, with --baseline-lib, on a build of the parent commit in the same process (the variants alternate).  hipEvent timing on a
stream of the library: `--inner` calls between two events (>= 20), `--repeats` repeats (>= 5) after a warm-up; the table reports the median
and the spread.  Both builds must give identical towers (fhe_checksum).  The kernels of one call come from fhe_launch_stats.
FHE_MOD_REDUCE_UNFUSED=1 in the environment makes this build run the launch-by-launch sequence (the A/B switch of the dispatch).

As information only: one timing of fhe_bgv_eval_mult beside fhe_ckks_eval_mult at config 3's shape (N = 2^16, l = 21, dnum = 3) with
--evalmult-batch ciphertexts.

A tool, not a test: it fails without a GPU.   python tools/bgv_mod_reduce_bench.py [--baseline-lib PATH] [--out profiles/FILE.md]
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
T = 65537


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


class Side:
    """one library's context, input tower, output tower and workspace for one shape"""

    def __init__(self, lib, logN, q, psi, B):
        self.lib, self.ctx, self.B, self.L = lib, fh.Context(lib, logN, q, psi), B, len(q)
        self.x = self.ctx.sample("uniform", B, self.L, seed=11)
        self.x.fmt = fh.EVALUATION  # (uniform residues: any format)
        self.out = self.ctx.empty(B, self.L - 1)
        self.wsb = lib.L.fhe_rescale_workspace_bytes(self.ctx.h, self.L, B)
        self.ws = self.ctx.malloc(self.wsb)
        self.st = vp()
        lib.check(lib.L.fhe_stream_create(self.ctx.h, C.byref(self.st)))

    def call(self):
        self.lib.check(self.lib.L.fhe_mod_reduce(self.ctx.h, self.x.ptr, self.L, T, 1, self.B, self.out.ptr, self.ws, self.wsb, self.st))

    def sync(self):
        self.lib.check(self.lib.L.fhe_stream_sync(self.ctx.h, self.st))

    def close(self):
        self.lib.check(self.lib.L.fhe_stream_destroy(self.ctx.h, self.st))
        self.ctx.close()


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
    ap.add_argument("--shapes", default="16,21,64;15,8,256", help="logN,sizeQl,batch;...")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--baseline-lib", default=None, help="libfhe_hip.so of the parent commit; without it only this build is timed")
    ap.add_argument("--evalmult-batch", type=int, default=16, help="0: skip the EvalMult timing")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 5 and a.inner >= 20
    lib = fh.Lib()
    if "emulator" in lib.version() or lib.device_count() < 1:
        raise SystemExit("bgv_mod_reduce_bench: needs the HIP build and a GPU")
    old = fh.Lib(a.baseline_lib, may_lack=("fhe_mod_reduce_limbs", "fhe_bgv_")) if a.baseline_lib else None
    ev = Events()
    forced = os.environ.get("FHE_MOD_REDUCE_UNFUSED", "0") not in ("", "0")
    lines = ["EVALUATION fhe_mod_reduce, t = 65537, uniform device-resident towers; ms per call, median (min .. max) of "
             f"{a.repeats} repeats of {a.inner} calls between two hipEvents, after a warm-up, variants alternating; outputs identical "
             "(fhe_checksum)" + ("; FHE_MOD_REDUCE_UNFUSED=1: this build runs the launch-by-launch sequence" if forced else ""), "",
             "| N | sizeQl | batch | this build | parent | this / parent |", "|---|---|---|---|---|---|"]
    rows, kern = [], []
    for shape in a.shapes.split(";"):
        logN, L, B = (int(v) for v in shape.split(","))
        q, psi = chain(lib, logN, L)
        sides = [("new", Side(lib, logN, q, psi, B))] + ([("parent", Side(old, logN, q, psi, B))] if old else [])
        sums = {}
        for name, s in sides:
            kern.append((shape, name, kernels_of(s.lib, s.call, s.sync)))
            sums[name] = s.ctx.checksum(s.out, s.st)
            ev.time(s.st, a.inner, s.call)  # warm-up
        assert all(np.array_equal(v, sums["new"]) for v in sums.values()), f"{shape}: the builds differ"
        times = {name: [] for name, _ in sides}
        for _ in range(a.repeats):
            for name, s in sides:
                times[name].append(ev.time(s.st, a.inner, s.call))
        tn, tp = times["new"], times.get("parent")
        lines.append(f"| 2^{logN} | {L} | {B} | {fmt(tn)} | {fmt(tp) if tp else 'not run'} | "
                     f"{np.median(tn) / np.median(tp) if tp else float('nan'):.3f} |")
        rows.append({"shape": shape, **{k + "_ms": v for k, v in times.items()}})
        for _, s in sides:
            s.close()
    lines += ["", "Kernel launches of one call (fhe_launch_stats; a labelled instance is listed with its family and once more under its label):", ""]
    for shape, name, k in kern:
        lines.append(f"- {shape} {name}: " + ", ".join(f"{n} x {kk}" for kk, n in sorted(k.items())))
    if a.evalmult_batch:
        logN, sizeQ, dnum, B = 16, 21, 3, a.evalmult_batch
        q, psiQ = lib.ckks_like_chain(logN, sizeQ)
        p, psiP = lib.select_p(logN, q, dnum, 60)
        allq = np.concatenate([q, p])
        ctx = fh.Context(lib, logN, allq, np.concatenate([psiQ, psiP]))
        plan = fh.KeySwitchPlan(ctx, sizeQ, len(p), dnum)
        rng = np.random.default_rng(3)
        key = [np.empty((dnum, len(allq), ctx.N), np.uint64) for _ in range(2)]
        for k in key:
            for i, qi in enumerate(allq):
                k[:, i, :] = rng.integers(0, int(qi), size=(dnum, ctx.N), dtype=np.uint64)
        plan.upload_key(*key)
        tw = [ctx.sample("uniform", B, sizeQ, seed=20 + i) for i in range(4)]
        c0, c1 = ctx.empty(B, sizeQ), ctx.empty(B, sizeQ)
        ws, wsb = plan.workspace(sizeQ, B)
        st = vp()
        lib.check(lib.L.fhe_stream_create(ctx.h, C.byref(st)))
        calls = {
            "fhe_ckks_eval_mult": lambda: lib.check(lib.L.fhe_ckks_eval_mult(plan.h, plan.key, tw[0].ptr, tw[1].ptr, tw[2].ptr, tw[3].ptr, sizeQ, B,
                                                                             c0.ptr, c1.ptr, ws, wsb, st)),
            "fhe_bgv_eval_mult": lambda: lib.check(lib.L.fhe_bgv_eval_mult(plan.h, plan.key, tw[0].ptr, tw[1].ptr, tw[2].ptr, tw[3].ptr, sizeQ, T, B,
                                                                           c0.ptr, c1.ptr, ws, wsb, st)),
        }
        em = {k: [] for k in calls}
        for k, f in calls.items():
            ev.time(st, 2, f)
        for _ in range(a.repeats):
            for k, f in calls.items():
                em[k].append(ev.time(st, 5, f))
        lines += ["", f"Information only: EvalMult + HYBRID key switch at config 3's shape (N = 2^16, l = {sizeQ}, k = {len(p)}, dnum = {dnum}), "
                  f"batch {B}, ms per call, median (min .. max) of {a.repeats} repeats of 5 calls:", ""]
        lines += [f"- {k}: {fmt(v)}" for k, v in em.items()]
        rows.append({"evalmult_batch": B, **{k + "_ms": v for k, v in em.items()}})
        lib.check(lib.L.fhe_stream_destroy(ctx.h, st))
        plan.close()
        ctx.close()
    lines += ["", "Command: `python tools/bgv_mod_reduce_bench.py " + " ".join(sys.argv[1:]) + "`"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"rows": rows}))


if __name__ == "__main__":
    main()
