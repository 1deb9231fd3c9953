#!/usr/bin/env python3
"""Throughput of the blake2xb stream kernel (fhe_blake2xb_stream, csrc/blake2_kernels.h): `reps` launches of 4 GiB each (2^20 blocks of
4 KiB) into one device buffer, timed by wall clock around a stream sync.  For the kernel's own time run it under
`rocprofv3 --kernel-trace --stats -- python tools/blake2_stream_probe.py`.
usage (on an MI355X): python tools/blake2_stream_probe.py [reps]"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from openfhe_amd import fhe_hip as fh  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
lib = fh.Lib()
ctx = fh.Context(lib, 4, [97], [19])
n_blocks = 1 << 20
key = fh._key_words(bytes(range(64)))
kp = key.ctypes.data_as(fh.u32p)
d = ctx.malloc(n_blocks * 4096)
lib.check(lib.L.fhe_blake2xb_stream(ctx.h, d, 64, kp, 0, None))  # (first launch: code object load)
ctx.sync()
t0 = time.perf_counter()
for r in range(reps):
    lib.check(lib.L.fhe_blake2xb_stream(ctx.h, d, n_blocks, kp, r * n_blocks, None))
ctx.sync()
dt = (time.perf_counter() - t0) / reps
print("RESULT", json.dumps({"bytes_per_launch": n_blocks * 4096, "reps": reps, "s_per_launch": dt, "GB_per_s": n_blocks * 4096 / dt / 1e9}))
ctx.free(d)
ctx.close()
