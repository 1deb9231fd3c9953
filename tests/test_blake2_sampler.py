"""blake2xb counter mode on the device (fhe_blake2xb_stream, fhe_sample_*_blake2; csrc/blake2_kernels.h).

What is pinned on what:
 * a numpy restatement of BLAKE2b (RFC 7693) against hashlib.blake2b, for every parameter block hashlib accepts;
 * the restatement's blake2xb against the reference's own blake2xb, called the way Blake2Engine::Generate() calls it
   (tests/golden/blake2xb_kats.json, recorded by tests/golden/make_blake2_kats.py: hashlib refuses depth = 0, the leaves' parameter);
 * the stream kernel against the KATs and the restatement, across the 32-bit carry of the counter;
 * the fused samplers against the restatement word for word, and their distributions against the reference's;
 * the gfx950 code object: no kernel of blake2_kernels.h has a private segment or spills VGPRs."""
import hashlib
import json
import math
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from openfhe_amd import fhe_hip as fh

from test_sampler import reference_dgg_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = os.path.join(ROOT, "tests", "golden", "blake2xb_kats.json")
M64 = (1 << 64) - 1

# ---- the restatement: BLAKE2b over numpy uint64 lanes ----------------------------------------------------------------------------
IV = np.array([0x6a09e667f3bcc908, 0xbb67ae8584caa73b, 0x3c6ef372fe94f82b, 0xa54ff53a5f1d36f1,
               0x510e527fade682d1, 0x9b05688c2b3e6c1f, 0x1f83d9abfb41bd6b, 0x5be0cd19137e2179], np.uint64)
SIGMA = [[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15], [14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3],
         [11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4], [7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8],
         [9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13], [2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9],
         [12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11], [13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10],
         [6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5], [10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0]]


def _rotr(x, s):
    return (x >> np.uint64(s)) | (x << np.uint64(64 - s))


def compress(h, m, t, last):
    """F (RFC 7693 3.2): h [8][lanes], m [16][lanes] uint64; t the byte counter (< 2^64)"""
    v = [h[i].copy() for i in range(8)] + [np.full(h.shape[1:], IV[i], np.uint64) for i in range(8)]
    v[12] = v[12] ^ np.uint64(t)
    if last:
        v[14] = ~v[14]
    for r in range(12):
        s = SIGMA[r % 10]
        for i, (a, b, c, d) in enumerate(((0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15),
                                          (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14))):
            v[a] = v[a] + v[b] + m[s[2 * i]]
            v[d] = _rotr(v[d] ^ v[a], 32)
            v[c] = v[c] + v[d]
            v[b] = _rotr(v[b] ^ v[c], 24)
            v[a] = v[a] + v[b] + m[s[2 * i + 1]]
            v[d] = _rotr(v[d] ^ v[a], 16)
            v[c] = v[c] + v[d]
            v[b] = _rotr(v[b] ^ v[c], 63)
    return np.stack([h[i] ^ v[i] ^ v[i + 8] for i in range(8)])


def param_words(digest=64, key=0, fanout=1, depth=1, leaf=0, node_offset=0, node_depth=0, inner=0):
    """words 0..2 of the parameter block (salt and personalisation zero); node_offset is 64-bit here (BLAKE2X: offset | xof << 32)"""
    return [digest | key << 8 | fanout << 16 | depth << 24 | leaf << 32, node_offset, node_depth | inner << 8]


def blake2b(p, data, key=b""):
    """BLAKE2b-512 of the byte string `data` under parameter words p (scalars or [lanes] arrays) and key: [8][lanes] uint64"""
    lanes = max(np.size(w) for w in p)
    h = np.repeat(IV[:, None], lanes, axis=1)
    for i, w in enumerate(p):
        h[i] ^= np.asarray(w, np.uint64)
    blocks = ([key + bytes(128 - len(key))] if key else []) + [data[i:i + 128] for i in range(0, len(data), 128)]
    if not blocks:
        blocks = [b""]
    t = 0
    for bi, blk in enumerate(blocks):
        t += len(blk) if (bi or not key) else 128
        m = np.frombuffer(blk + bytes(128 - len(blk)), "<u8").astype(np.uint64)
        h = compress(h, np.repeat(m[:, None], lanes, axis=1), t, bi == len(blocks) - 1)
    return h


def blake2xb_blocks(key, counters):
    """the 4 KiB blocks blake2xb(4096 bytes, in = counter (8 bytes little-endian), key (64 bytes)): uint32 [len(counters)][1024]"""
    counters = np.asarray(counters, np.uint64)
    n = counters.size
    kw = np.frombuffer(key, "<u8").astype(np.uint64)
    h = np.repeat(IV[:, None], n, axis=1)
    p = param_words(key=64, node_offset=4096 << 32)
    for i, w in enumerate(p):
        h[i] ^= np.uint64(w)
    m = np.zeros((16, n), np.uint64)
    m[:8] = kw[:, None]
    h = compress(h, m, 128, False)
    m = np.zeros((16, n), np.uint64)
    m[0] = counters
    h0 = compress(h, m, 136, True)  # [8][n]
    # leaves: lane (block, leaf)
    leaf = np.tile(np.arange(64, dtype=np.uint64), n)
    p = param_words(fanout=0, depth=0, leaf=64, inner=64)
    h = np.repeat(IV[:, None], n * 64, axis=1)
    h[0] ^= np.uint64(p[0])
    h[1] ^= leaf | np.uint64(4096 << 32)
    h[2] ^= np.uint64(p[2])
    m = np.zeros((16, n * 64), np.uint64)
    m[:8] = np.repeat(h0, 64, axis=1)
    out = compress(h, m, 64, True)  # [8][n * 64]
    return np.ascontiguousarray(out.T).reshape(n, 512).view(np.uint32)


def stream64(key, counter0, words64):
    """R[0 .. words64): the 64-bit words of S(key, counter0)"""
    nb = (words64 + 511) // 512
    ctr = (np.arange(nb, dtype=np.uint64) + np.uint64(counter0 & M64))  # (wraps mod 2^64)
    return blake2xb_blocks(key, ctr).view(np.uint64).ravel()[:words64]


def mod128(hi, lo, q):
    """(hi * 2^64 + lo) mod q for uint64 arrays, q < 2^60: four bits of lo at a time"""
    q = np.uint64(q)
    r = hi % q
    for s in range(60, -4, -4):
        r = ((r << np.uint64(4)) | ((lo >> np.uint64(s)) & np.uint64(15))) % q
    return r


def mulhi3(x):
    """floor(3 x / 2^64)"""
    lo = ((x & np.uint64(0xffffffff)) * np.uint64(3)) >> np.uint64(32)
    return (((x >> np.uint64(32)) * np.uint64(3)) + lo) >> np.uint64(32)


def peikert(x, sigma):
    vals, a = reference_dgg_table(sigma)
    s = (x >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0) - 0.5
    tmp = np.abs(s) - a / 2
    idx = np.minimum(np.searchsorted(np.array(vals), tmp, side="left"), len(vals) - 1)
    k = (idx + 1).astype(np.int64)
    k = np.where(s > 0.0, k, -k)
    return np.where(tmp <= 0.0, 0, k)


def sample_want(kind, key, counter0, q_sel, batch, N, sigma=3.19):
    """the samplers restated: uint64 [batch][nLimbs][N]"""
    L = len(q_sel)
    if kind == "uniform":
        R = stream64(key, counter0, 2 * batch * L * N).reshape(batch, L, N, 2)
        return np.stack([mod128(R[:, l, :, 1], R[:, l, :, 0], q_sel[l]) for l in range(L)], axis=1)
    R = stream64(key, counter0, batch * N).reshape(batch, N)
    k = peikert(R, sigma) if kind == "gaussian" else mulhi3(R).astype(np.int64) - 1
    return np.stack([np.where(k < 0, np.uint64(q) - np.abs(k).astype(np.uint64), k.astype(np.uint64)) for q in q_sel], axis=1)


def kats():
    with open(KATS) as f:
        return json.load(f)


def kat_key(k):
    return bytes.fromhex(k["key"])


# ---- (a) the restatement ---------------------------------------------------------------------------------------------------------
def test_restatement_is_blake2b():
    rng = np.random.default_rng(1)
    for klen, dlen in ((0, 0), (0, 3), (64, 8), (64, 0), (17, 128), (0, 129), (64, 300), (32, 256)):
        key, data = rng.bytes(klen), rng.bytes(dlen)
        for kw in (dict(), dict(fanout=1, depth=1), dict(fanout=0, depth=1, leaf_size=64, node_offset=5 | 4096 << 32, inner_size=64),
                   dict(fanout=3, depth=7, leaf_size=1 << 20, node_offset=(1 << 64) - 2, node_depth=3, inner_size=64, last_node=False)):
            want = hashlib.blake2b(data, key=key, digest_size=64, **kw).digest()
            p = param_words(key=klen, fanout=kw.get("fanout", 1), depth=kw.get("depth", 1), leaf=kw.get("leaf_size", 0),
                            node_offset=kw.get("node_offset", 0), node_depth=kw.get("node_depth", 0), inner=kw.get("inner_size", 0))
            got = blake2b(p, data, key)[:, 0].astype("<u8").tobytes()
            assert got == want, (klen, dlen, kw)


def test_restatement_is_the_references_blake2xb():
    for k in kats():
        blk = blake2xb_blocks(kat_key(k), [k["counter"]])[0]
        assert hashlib.sha256(blk.astype("<u4").tobytes()).hexdigest() == k["sha256"]
        assert blk[:16].tolist() == k["first16"] and blk[-16:].tolist() == k["last16"]


# ---- (b) the stream kernel -------------------------------------------------------------------------------------------------------
def test_stream_kernel_is_the_references(backend):
    for k in kats():
        blk = backend.blake2xb_stream(kat_key(k), k["counter"], 1)[0]
        assert hashlib.sha256(blk.astype("<u4").tobytes()).hexdigest() == k["sha256"]
    # consecutive counters: one call = successive Generate() calls (the KATs of the carry are adjacent counters)
    by_ctr = {(k["key"], k["counter"]): k for k in kats()}
    for (key, ctr), k in by_ctr.items():
        nxt = by_ctr.get((key, (ctr + 1) & M64))
        if nxt:
            two = backend.blake2xb_stream(kat_key(k), ctr, 2)
            assert two[1][:16].tolist() == nxt["first16"] and two[1][-16:].tolist() == nxt["last16"]


def test_stream_kernel_equals_the_restatement(backend):
    rng = np.random.default_rng(7)
    emu = "emulator" in backend.version()
    for n, c0 in ((1, 0), (63, 5), (65, (1 << 32) - 3), (257 if emu else 300, (1 << 32) - 100), (3, (1 << 64) - 2)):
        key = rng.bytes(64)
        got = backend.blake2xb_stream(key, c0, n)
        assert np.array_equal(got, blake2xb_blocks(key, (np.arange(n, dtype=np.uint64) + np.uint64(c0)))), (n, c0)
    assert backend.blake2xb_stream(rng.bytes(64), 0, 0).shape == (0, 1024)


def test_stream_kernel_is_independent_of_the_walk(backend):
    """the host shortens the walk of a wave (counters per wave, 64 down to 1) for calls too small to fill the device: calls of every walk
    length agree with the restatement (the emulator reports 3 compute units, the MI355X 256)"""
    rng = np.random.default_rng(8)
    emu = "emulator" in backend.version()
    for n in ((30, 50, 100, 200, 400, 800, 1600) if emu else (3000, 5000, 9000, 20000, 40000, 70000, (1 << 17) + 5)):
        key, c0 = rng.bytes(64), int(rng.integers(0, 1 << 63))
        got = backend.blake2xb_stream(key, c0, n)
        idx = np.arange(n) if n <= 5000 else np.unique(np.concatenate([np.arange(300), np.arange(n - 300, n), rng.integers(0, n, 400)]))
        want = blake2xb_blocks(key, idx.astype(np.uint64) + np.uint64(c0))
        assert np.array_equal(got[idx], want), n


# ---- (c) the samplers word for word ----------------------------------------------------------------------------------------------
def _small_prime(lib, N):
    """the first prime = 1 mod 2N from 2^16 on (65537, 17 bits, up to N = 2^15)"""
    m = 2 * N
    base = ((1 << 16) // m) * m + 1
    return int(lib.L.fhe_param_next_prime(base - m if base > m else base, m))


def _context(lib, logN, L):
    """L moduli near 2^60 and, at limb 1, a small one"""
    N = 1 << logN
    q, _ = lib.dcrt_chain(logN, L, 60)
    q = [int(v) for v in q]
    q[1] = _small_prime(lib, N)
    q = np.array(q, np.uint64)
    psi = np.array([lib.L.fhe_param_root_of_unity(2 * N, int(v)) for v in q], np.uint64)
    return fh.Context(lib, logN, q, psi), q


SHAPES_EMU = [(11, 1, 1), (11, 3, 3), (11, 30, 1)]
SHAPES_GPU = [(14, 1, 3), (14, 30, 3), (17, 3, 1), (17, 30, 1)]


@pytest.mark.parametrize("kind", ["uniform", "gaussian", "ternary"])
def test_samplers_equal_the_restatement(backend, kind):
    rng = np.random.default_rng(11)
    emu = "emulator" in backend.version()
    for logN, nl, batch in (SHAPES_EMU if emu else SHAPES_GPU):
        N = 1 << logN
        ctx, q = _context(backend, logN, 32)
        sel = None if nl == 1 else (np.array([5, 1, 0], np.uint32) if nl == 3 else np.array([1] + list(range(31, 2, -1)), np.uint32))
        qs = q[sel] if sel is not None else q[:1]
        key = rng.bytes(64)
        c0 = int(rng.integers(0, 1 << 63)) if nl != 3 else (1 << 32) - 1
        for sigma in ((3.19, 25.0) if kind == "gaussian" else (3.19,)):
            got = ctx.sample(kind, batch, nl, limb_idx=sel, sigma=sigma, generator="blake2", key=key, counter0=c0).to_host()
            want = sample_want(kind, key, c0, qs, batch, N, sigma)
            assert np.array_equal(got, want), (kind, logN, nl, batch, sigma)
            assert np.all(got < qs[None, :, None])
        ctx.close()


def test_sampler_ending_mid_block(backend):
    """N = 16, one limb: a uniform call covers 16 of a block's 256 coefficients, a ternary call 48 of 512 (batch 3): the lanes past
    the end store nothing"""
    lib = backend
    q = np.array([int(lib.L.fhe_param_last_prime(60, 32))], np.uint64)
    ctx = fh.Context(lib, 4, q, np.array([lib.L.fhe_param_root_of_unity(32, int(q[0]))], np.uint64))
    key = bytes(range(64))
    for kind, batch in (("uniform", 1), ("ternary", 3), ("gaussian", 2)):
        t = ctx.empty(batch + 8, 1, fmt=fh.COEFFICIENT)
        guard = np.full((batch + 8, 1, 16), 0xABCDEF, np.uint64)
        lib.check(lib.L.fhe_memcpy_h2d(ctx.h, t.ptr, guard.ctypes.data_as(fh.vp), guard.nbytes, None))
        kp = fh._key_words(key).ctypes.data_as(fh.u32p)
        fn = {"uniform": lambda: lib.L.fhe_sample_uniform_blake2(ctx.h, t.ptr, None, 1, batch, kp, 9, None),
              "ternary": lambda: lib.L.fhe_sample_ternary_blake2(ctx.h, t.ptr, None, 1, batch, kp, 9, None),
              "gaussian": lambda: lib.L.fhe_sample_gaussian_blake2(ctx.h, t.ptr, None, 1, batch, 3.19, kp, 9, None)}[kind]
        lib.check(fn())
        got = t.to_host()
        assert np.array_equal(got[:batch], sample_want(kind, key, 9, q, batch, 16)), kind
        assert np.all(got[batch:] == 0xABCDEF), kind
    ctx.close()


# ---- (d) distributions -----------------------------------------------------------------------------------------------------------
def test_distributions_are_the_references(backend):
    emu = "emulator" in backend.version()
    logN, B = (12, 16) if emu else (14, 16)
    N = 1 << logN
    ctx, q = _context(backend, logN, 3)
    key = bytes(range(1, 65))
    x = ctx.sample("uniform", B, 3, generator="blake2", key=key, counter0=1).to_host()
    for l in range(3):
        v = x[:, l, :].ravel().astype(np.float64) / float(q[l])
        assert np.all(x[:, l, :] < q[l])
        hist = np.histogram(v, bins=16, range=(0, 1))[0]
        exp = v.size / 16
        assert np.sum((hist - exp) ** 2 / exp) < 16 + 6 * math.sqrt(2 * 16)  # chi-square, 6 sigma
    sigma = 3.19
    y = ctx.sample("gaussian", B, 1, sigma=sigma, generator="blake2", key=key, counter0=1 << 40).to_host()[:, 0, :].ravel()
    ints = np.where(y > q[0] // 2, -(q[0] - y).astype(np.int64), y.astype(np.int64))
    vals, a = reference_dgg_table(sigma)
    n = ints.size
    assert abs((ints == 0).mean() - a) < 6 * math.sqrt(a * (1 - a) / n)
    prev = 0.0
    for k in range(1, 9):
        pk = vals[k - 1] - prev
        prev = vals[k - 1]
        for sgn in (1, -1):
            f = (ints == sgn * k).mean()
            assert abs(f - pk) < 6 * math.sqrt(pk * (1 - pk) / n), (k, sgn, f, pk)
    z = ctx.sample("ternary", B, 1, generator="blake2", key=key, counter0=1 << 41).to_host()[:, 0, :].ravel()
    ints = np.where(z == q[0] - np.uint64(1), -1, z.astype(np.int64))
    assert set(np.unique(ints)) <= {-1, 0, 1}
    for v in (-1, 0, 1):
        assert abs((ints == v).mean() - 1 / 3) < 6 * math.sqrt(2 / 9 / n)
    ctx.close()


# ---- (e) key and counter separate the blocks -------------------------------------------------------------------------------------
def test_key_and_counter_change_every_block(backend):
    key = bytearray(range(64))
    a = backend.blake2xb_stream(bytes(key), 1000, 64)
    key[63] ^= 1
    b = backend.blake2xb_stream(bytes(key), 1000, 64)
    c = backend.blake2xb_stream(bytes(range(64)), 1001, 64)
    for other in (b, c):
        # every block differs, and in about half of its bits
        assert all(not np.array_equal(a[i], other[i]) for i in range(64))
        bits = np.unpackbits((a ^ other).view(np.uint8), axis=1).sum(axis=1, dtype=np.int64)
        assert np.all(np.abs(bits - 16384) < 6 * math.sqrt(8192))
    assert np.array_equal(a[1:], c[:-1])  # (counter0 + 1 is the same stream, one block later)


# ---- (f) the gfx950 code object --------------------------------------------------------------------------------------------------
def _code_object_notes():
    so = os.path.join(ROOT, "openfhe-development_amd", "csrc", "libfhe_hip.so")
    assert os.path.exists(so), "libfhe_hip.so is not built (python __graft_entry__.py)"
    # the ROCm installation that provides hipcc (build.sh compiles with it) also provides the LLVM binary tools
    hipcc = shutil.which("hipcc")
    assert hipcc, "hipcc is not on PATH"
    llvm = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin")
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fatbin")
        subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", so, os.path.join(d, "x")])
        co = os.path.join(d, "gfx950.co")
        subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"])
        return subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", co], text=True)


def test_blake2_kernels_keep_everything_in_registers():
    notes = _code_object_notes()
    # one metadata map per kernel: split at each kernel's ".name" entry and keep the keys of that map
    kernels = {}
    for chunk in re.split(r"\n\s+- \.", notes):
        name = re.search(r"\.name:\s+(\S+)", chunk)
        if name and "blake2xb_kernel" in name.group(1) and ".symbol:" in chunk:
            kernels[name.group(1)] = chunk
    assert len(kernels) == 4, sorted(kernels)
    for name, chunk in kernels.items():
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", chunk), name
        assert re.search(r"\.vgpr_spill_count:\s+0\b", chunk), name
