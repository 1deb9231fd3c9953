"""Records blake2xb_kats.json: the reference's own blake2xb, called the way default_prng::Blake2Engine::Generate() calls it
(blake2engine.cpp: out = its 1024-word buffer (4096 bytes), in = its 64-bit counter (8 bytes), key = its 16-word seed (64 bytes)).

Needs the reference's core library, built by the recipe under oracle/ (./build.sh ref -> oracle/_ref/libOPENFHEcore.so).
    python tests/golden/make_blake2_kats.py
Each entry keeps the key, the counter, the sha256 of the 4096 bytes and their first and last 16 words (uint32, little-endian)."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libOPENFHEcore.so"))
    lib.blake2xb.restype = C.c_int
    lib.blake2xb.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    rng = np.random.default_rng(20261016)
    rand_key = rng.integers(0, 1 << 32, 16, dtype=np.uint64).astype(np.uint32)
    cases = [(np.zeros(16, np.uint32), 0), (np.zeros(16, np.uint32), 1), (rand_key, 0), (rand_key, (1 << 32) - 1),
             (rand_key, 1 << 32), (rand_key, (1 << 64) - 1)]
    out = []
    for key, ctr in cases:
        buf = np.zeros(1024, np.uint32)
        c = C.c_uint64(ctr)
        key = np.ascontiguousarray(key, np.uint32)
        assert lib.blake2xb(buf.ctypes.data, 4096, C.addressof(c), 8, key.ctypes.data, 64) == 0
        out.append({"key": key.astype("<u4").tobytes().hex(), "counter": ctr,
                    "sha256": hashlib.sha256(buf.astype("<u4").tobytes()).hexdigest(),
                    "first16": [int(v) for v in buf[:16]], "last16": [int(v) for v in buf[-16:]]})
    with open(os.path.join(HERE, "blake2xb_kats.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
