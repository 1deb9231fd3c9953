#!/usr/bin/env python3
"""BGV decryption on one GPU, device-resident towers of uniform residues, t = 65537:

  fhe_mod_reduce_to_t   against   sizeQl - 1 calls of fhe_mod_reduce on the COEFFICIENT tower (the path of the parent commit; that entry is
                                  unchanged), whose last limb the host would still have to reduce modulo t
  fhe_bgv_decrypt       against   fhe_mul + fhe_add (DecryptCore, the secret key copied once per ciphertext), fhe_ntt_inv and the same loop

at N = 2^14 and 2^15, sizeQl = 4, 8, 16, 24, batch 16 and 64.  Before any timing the words are compared: the loop's last limb, reduced modulo t
on the host, must equal the output of fhe_mod_reduce_to_t, and both decryptions must agree.  hipEvent timing on a stream of the library:
at least `--inner` calls and about `--window-ms` of work between two events, `--repeats` repeats after a warm-up of every variant at every
shape, the variants alternating; the table reports the median and the spread of the milliseconds per call.  The clocks the device reports
before and after go into the record.

A tool, not a test: it fails without a GPU.   python tools/bgv_decrypt_bench.py [--out profiles/bgv_decrypt.md]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from openfhe_amd import fhe_hip as fh  # noqa: E402
from bgv_mod_reduce_bench import Events, chain, fmt, kernels_of  # noqa: E402

vp = C.c_void_p
T = 65537


def clocks():
    """the lines of `rocm-smi --showclocks` that name the shader and memory clocks (reading only), or a note that it could not be read"""
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        got = [" ".join(line.split()) for line in out.splitlines() if "sclk" in line or "mclk" in line]
        return got[:4] or ["rocm-smi printed no clock lines"]
    except (OSError, subprocess.SubprocessError) as e:
        return [f"rocm-smi not available ({type(e).__name__})"]


class Shape:
    """the towers, outputs and workspaces of one shape, and the four variants as calls on one stream"""

    def __init__(self, lib, logN, sizeQl, B):
        q, psi = chain(lib, logN, sizeQl)
        self.lib, self.q, self.B, self.L = lib, q, B, sizeQl
        ctx = self.ctx = fh.Context(lib, logN, q, psi)
        L = lib.L
        self.x = ctx.sample("uniform", B, sizeQl, seed=11)  # COEFFICIENT
        self.c = [ctx.sample("uniform", B, sizeQl, seed=12 + e) for e in range(2)]  # (uniform residues: any format)
        self.s = ctx.sample("uniform", 1, sizeQl, seed=15)
        self.sB = ctx.empty(B, sizeQl)  # the parent's element-wise kernels want one copy of s per ciphertext
        words = sizeQl * ctx.N * 8
        for b in range(B):
            lib.check(L.fhe_memcpy_d2d(ctx.h, vp(self.sB.ptr.value + b * words), self.s.ptr, words, None))
        self.out = [ctx.malloc(B * ctx.N * 8) for _ in range(2)]  # chain, decrypt
        self.pp = [ctx.empty(B, sizeQl), ctx.empty(B, sizeQl)]  # the loop's towers between steps
        self.b = ctx.empty(B, sizeQl)
        self.wsb = [L.fhe_mod_reduce_chain_workspace_bytes(ctx.h, sizeQl, sizeQl - 1, B), L.fhe_bgv_decrypt_workspace_bytes(ctx.h, 2, sizeQl, B),
                    L.fhe_rescale_workspace_bytes(ctx.h, sizeQl, B)]
        self.ws = [ctx.malloc(max(n, 8)) for n in self.wsb]
        self.elems = (vp * 2)(self.c[0].ptr.value, self.c[1].ptr.value)
        self.st = vp()
        lib.check(L.fhe_stream_create(ctx.h, C.byref(self.st)))
        ctx.sync()

    def loop(self, src):
        """sizeQl - 1 calls of fhe_mod_reduce on COEFFICIENT towers; returns the tower that holds the last limb"""
        L, cur = self.lib.L, src
        for k, n in enumerate(range(self.L, 1, -1)):
            dst = self.pp[k & 1]
            self.lib.check(L.fhe_mod_reduce(self.ctx.h, cur.ptr, n, T, 0, self.B, dst.ptr, self.ws[2], self.wsb[2], self.st))
            cur = dst
        return cur

    def to_t(self):
        self.lib.check(self.lib.L.fhe_mod_reduce_to_t(self.ctx.h, self.x.ptr, None, self.L, T, self.B, self.out[0], self.ws[0], self.wsb[0], self.st))

    def decrypt(self):
        self.lib.check(self.lib.L.fhe_bgv_decrypt(self.ctx.h, self.elems, 2, self.s.ptr, None, self.L, T, self.B, self.out[1], self.ws[1],
                                                  self.wsb[1], self.st))

    def decrypt_loop(self):
        L, h = self.lib.L, self.ctx.h
        self.lib.check(L.fhe_mul(h, self.b.ptr, self.c[1].ptr, self.sB.ptr, None, self.L, self.B, self.st))
        self.lib.check(L.fhe_add(h, self.b.ptr, self.b.ptr, self.c[0].ptr, None, self.L, self.B, self.st))
        self.lib.check(L.fhe_ntt_inv(h, self.b.ptr, None, self.L, self.B, self.st))
        return self.loop(self.b)

    def sync(self):
        self.lib.check(self.lib.L.fhe_stream_sync(self.ctx.h, self.st))

    def last_limb_mod_t(self, tower):
        """the loop's last limb, centred and reduced modulo t on the host (DecryptionCRTInterpolate)"""
        self.sync()
        v = self.ctx.download(tower.ptr, (self.B, self.ctx.N), self.st).astype(np.int64)  # (tower [B][1][N] after the last step)
        q0 = int(self.q[0])
        return np.mod(np.where(v > q0 // 2, v - q0, v), T).astype(np.uint64)

    def check_words(self):
        want = self.last_limb_mod_t(self.loop(self.x))
        self.to_t()
        self.sync()
        assert np.array_equal(self.ctx.download(self.out[0], (self.B, self.ctx.N), self.st), want), "fhe_mod_reduce_to_t differs from the loop"
        want = self.last_limb_mod_t(self.decrypt_loop())
        self.decrypt()
        self.sync()
        assert np.array_equal(self.ctx.download(self.out[1], (self.B, self.ctx.N), self.st), want), "fhe_bgv_decrypt differs from the loop"

    def close(self):
        self.lib.check(self.lib.L.fhe_stream_destroy(self.ctx.h, self.st))
        self.ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", default="14,15")
    ap.add_argument("--sizes", default="4,8,16,24")
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--window-ms", type=float, default=40.0, help="work between two events: calls = max(inner, window / time of one call)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.repeats >= 5 and a.inner >= 5
    lib = fh.Lib()
    if "emulator" in lib.version() or lib.device_count() < 1:
        raise SystemExit("bgv_decrypt_bench: needs the HIP build and a GPU")
    ev = Events()
    before = clocks()
    lines = [f"BGV decryption, t = {T}, uniform device-resident towers; ms per call, median (min .. max) of {a.repeats} repeats of at least {a.inner} calls "
             f"and about {a.window_ms:g} ms of work between two hipEvents, after a warm-up of every variant, the variants alternating.  chain = fhe_mod_reduce_to_t; loop = sizeQl - 1 "
             "calls of fhe_mod_reduce on the COEFFICIENT tower (the parent commit's path, without the residues modulo t that it leaves to the "
             "host); decrypt = fhe_bgv_decrypt; decrypt by loop = fhe_mul, fhe_add, fhe_ntt_inv and the loop.  At every shape the words of the "
             "new entries were compared with the loop's before the timing.", "",
             "| N | sizeQl | batch | chain | loop | loop / chain | decrypt | decrypt by loop | by loop / decrypt |", "|---|---|---|---|---|---|---|---|---|"]
    rows, kern, lost = [], [], []
    for logN in (int(v) for v in a.logn.split(",")):
        for sizeQl in (int(v) for v in a.sizes.split(",")):
            for B in (int(v) for v in a.batches.split(",")):
                s = Shape(lib, logN, sizeQl, B)
                s.check_words()
                variants = {"chain": s.to_t, "loop": lambda: s.loop(s.x), "decrypt": s.decrypt, "decrypt_loop": s.decrypt_loop}
                if B == int(a.batches.split(",")[0]):
                    kern.append((f"2^{logN}, {sizeQl}", {k: kernels_of(lib, f, s.sync) for k, f in variants.items()}))
                # warm-up; it also sizes the timed window: at least --inner calls and about --window-ms of work between the two events
                calls = {k: max(a.inner, min(4000, int(a.window_ms / ev.time(s.st, max(2, a.inner // 4), f)))) for k, f in variants.items()}
                times = {k: [] for k in variants}
                for _ in range(a.repeats):
                    for k, f in variants.items():
                        times[k].append(ev.time(s.st, calls[k], f))
                med = {k: float(np.median(v)) for k, v in times.items()}
                lines.append(f"| 2^{logN} | {sizeQl} | {B} | {fmt(times['chain'])} | {fmt(times['loop'])} | {med['loop'] / med['chain']:.2f} | "
                             f"{fmt(times['decrypt'])} | {fmt(times['decrypt_loop'])} | {med['decrypt_loop'] / med['decrypt']:.2f} |")
                if med["chain"] > med["loop"]:
                    lost.append(f"2^{logN} / {sizeQl} / {B}: chain")
                if med["decrypt"] > med["decrypt_loop"]:
                    lost.append(f"2^{logN} / {sizeQl} / {B}: decrypt")
                rows.append({"logN": logN, "sizeQl": sizeQl, "batch": B, **{k + "_ms": v for k, v in times.items()}})
                s.close()
    lines += ["", "Shapes at which a new entry was SLOWER than the loop (median): " + ("; ".join(lost) if lost else "none") + ".", "",
              f"Kernel launches of one call at batch {a.batches.split(',')[0]} (fhe_launch_stats; a labelled instance is listed with its family and once more under its label):", ""]
    for shape, per in kern:
        for k, d in per.items():
            lines.append(f"- {shape} {k}: {sum(n for kk, n in d.items() if '<' not in kk)} launches: " + ", ".join(f"{n} x {kk}" for kk, n in sorted(d.items())))
    lines += ["", "Clocks reported by the device before the run: " + "; ".join(before) + ".  After: " + "; ".join(clocks()) + ".", "",
              "Command: `python tools/bgv_decrypt_bench.py " + " ".join(sys.argv[1:]) + "`"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps({"rows": rows}))


if __name__ == "__main__":
    main()
