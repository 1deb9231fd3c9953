"""The 6 + 10 split of the forward transform at N = 2^16: the column pass runs the transform's first six stages (ntt_static.h,
ntt_col6_fwd_body: 4 + 2 around one LDS exchange) and the batched row pass ten stages inside its 12-stage tile (ntt_row8.h, SPLIT).  The
intermediate tower differs from the one every other kernel exchanges, the transform's words must not: every case is compared word for word
with the oracle AND with the same calls under FHE_NTT_SPLIT6=0, on the lane emulator (its C++ butterflies check every lazy bound the new
schedule promises and abort on a violation) and on the GPU, and asserts the launches of the pair's own tag (<SPLIT6>), which are 0 where the
pair must not run: inverse transforms (the inverse pair was measured slower and is not part of the library), batch 1, and the switch at 0.

FHE_NTT_SPLIT6 is read once per process, so every setting runs in a child process, which writes its results to a file; the parent compares
the files of the two settings.

Shapes: N = 2^16 is the only ring with this pair.  Three limbs: the ring's last 60-bit prime (the top of the lazy ranges: 16 q just fits a
word), 36-bit prime (the smallest size on the quotient-estimate reductions) and 33-bit prime (the ladder reductions).  Batch 2 is all new
pair, batch 3 a group and a remainder on the 4 + 12 kernels in one call (one column launch serves both), batch 1 has no new pair.  In place,
out of place (the input must stay untouched), through ApproxModUp over a reversed limb subset (strided views), and the round trip.
Operands (test_parity_edges.pattern): all q-1, `mix`, the input whose transform is all q-1, and uniform residues."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libfhe_emu.so")
HIP = os.path.join(ROOT, "openfhe-development_amd", "csrc", "libfhe_hip.so")

PRELUDE = r"""
import ctypes as C, os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np, libs
from openfhe_amd import fhe_hip as fh
from test_parity_edges import pattern, roots
lib = fh.Lib({so!r})
o = libs.load_oracle()
SPLIT, P = {split}, 2
results = {{}}
logN = 16
N = 1 << logN
def limbs(sizes=(60, 36, 33)):
    M = 2 << logN
    q = np.array([o.orc_last_prime(s, M) for s in sizes], np.uint64)
    assert [int(v).bit_length() for v in q] == list(sizes)
    return q, roots(o, logN, q)
def towers(rng, octx, names, q, inverse, sel=None):
    # one tower per name; "pre": the input whose transform (in the direction under test) is all q-1
    out = []
    for n in names:
        if n == "pre":
            t = pattern(rng, "max", q, N)[None].copy()
            (o.orc_ntt_fwd_tower if inverse else o.orc_ntt_inv_tower)(octx, t, None if sel is None else sel.ctypes.data, len(q), 1, 0)
            out.append(t[0])
        else:
            out.append(pattern(rng, n, q, N))
    return np.stack(out)
def split_counts():
    # launches of the pair's instances since the library was loaded: (row pass, column pass)
    return np.array([lib.launch_count("ntt_row8_batched_kernel<SPLIT6>"), lib.launch_count("ntt_static_kernel<SPLIT6>")], np.int64)
def by_kernel():
    # every line of fhe_launch_stats but the pair's own tag
    buf = C.create_string_buffer(1 << 16)
    lib.L.fhe_launch_stats(buf, len(buf), None)
    out = {{}}
    for line in buf.value.decode().splitlines():
        k, n = line.rsplit(" ", 1)
        if "<SPLIT6>" not in k:
            out[k] = int(n)
    return out
def expect(B, inverse):
    return np.array([1, 1] if SPLIT and not inverse and B >= P else [0, 0], np.int64)
"""

NTT_CHILD = PRELUDE + r"""
rng = np.random.default_rng(1601)
q, psi = limbs()
L = len(q)
ctx = fh.Context(lib, logN, q, psi)
octx = o.orc_ctx_create(N, L, q, psi)
for ci, (B, mode, names) in enumerate({cases!r}):
    assert len(names) == B
    for inverse in (False, True):
        x = towers(rng, octx, names, q, inverse)
        want = x.copy()
        (o.orc_ntt_inv_tower if inverse else o.orc_ntt_fwd_tower)(octx, want, None, L, B, 0)
        if "pre" in names:
            assert np.array_equal(want[names.index("pre")], pattern(rng, "max", q, N)), "the oracle's transforms are inverse to each other"
        before = split_counts()
        t = ctx.tower(x, fmt=fh.EVALUATION if inverse else fh.COEFFICIENT)
        if mode == "inplace":
            t.SwitchFormat()
            got = t.to_host()
        else:
            out = ctx.empty(B, L)
            f = lib.L.fhe_ntt_inv_oop if inverse else lib.L.fhe_ntt_fwd_oop
            lib.check(f(ctx.h, t.ptr, out.ptr, None, L, B, None))
            got = out.to_host()
            assert np.array_equal(t.to_host(), x), "an out-of-place transform must not touch its input"
            out.fmt = fh.COEFFICIENT if inverse else fh.EVALUATION
            t = out
        ran = split_counts() - before
        tag = f"B={{B}} {{mode}} {{'inverse' if inverse else 'forward'}}"
        for b in range(B):
            for l in range(L):
                assert np.array_equal(got[b, l], want[b, l]), f"{{tag}}: tower {{names[b]}} limb {{q[l]}} differs from the oracle"
        assert np.array_equal(ran, expect(B, inverse)), f"{{tag}}: <SPLIT6> launches {{ran}}, expected {{expect(B, inverse)}}"
        results[f"{{ci}}_{{int(inverse)}}"] = got
        before = split_counts()
        t.SwitchFormat()  # the way back
        assert np.array_equal(t.to_host(), x), f"{{tag}}: round trip"
        assert np.array_equal(split_counts() - before, expect(B, not inverse)), f"{{tag}}: <SPLIT6> launches of the way back"
o.orc_ctx_destroy(octx)
ctx.close()
np.savez({dump!r}, **results)
print("ok")
"""

# ApproxModUp over the source limbs (2, 1) of a three-limb context, batch 3: the transforms run on strided views (inStride / outStride) of the
# result tower, over a limb subset in reversed order; COEFFICIENT input transforms source and target rows forward (two plain forward
# transforms: a group of two on the new pair and a remainder each), EVALUATION input the source rows inverse and the target rows forward
VIEWS_CHILD = PRELUDE + r"""
rng = np.random.default_rng(1602)
B = 3
q, psi = limbs()
ctx = fh.Context(lib, logN, q, psi)
src, dst = np.array([2, 1], np.uint32), np.array([0], np.uint32)
order = np.concatenate([src, dst])
octx = o.orc_ctx_create(N, 3, q[order], psi[order])  # the oracle's source basis is its first limbs
hatInv, hatPre, hatMod, _, _, mu = libs.crt_tables(q[src], q[dst])
conv = fh.Conv(ctx, src, dst)
for fmt, inEval in ((fh.COEFFICIENT, 0), (fh.EVALUATION, 1)):
    x = towers(rng, octx, ("max", "mix", "pre"), q[src], bool(inEval), sel=np.arange(2, dtype=np.uint32))
    want = np.empty((B, 3, N), np.uint64)
    for bb in range(B):
        o.orc_approx_mod_up(octx, 2, 1, x[bb], inEval, hatInv, hatPre, hatMod, mu, want[bb])
    before = split_counts()
    got = conv.ApproxModUp(ctx.tower(x, limb_idx=src, fmt=fmt)).to_host()
    ran = split_counts() - before
    assert np.array_equal(got, want), f"ApproxModUp inEval={{inEval}} differs from the oracle"
    nfwd = 1 if inEval else 2
    assert np.array_equal(ran, [nfwd, nfwd] if SPLIT else [0, 0]), f"ApproxModUp inEval={{inEval}}: <SPLIT6> launches {{ran}}"
    results[f"modup_{{inEval}}"] = got
conv.close()
o.orc_ctx_destroy(octx)
ctx.close()
np.savez({dump!r}, **results)
print("ok")
"""

# The other consumers of the intermediate tower, at batch 2: fhe_poly_mul (its fused row kernels read what the plain column pass wrote) and a
# HYBRID key switch.  Both match the oracle; their launches by kernel name are compared between the two settings by the parent: equal apart
# from the pair's own tag, so no pass was split or re-routed.  fhe_poly_mul launches no kernel of the pair at all.
CALLERS_CHILD = PRELUDE + r"""
from test_parity_edges import chain, limit_pair
rng = np.random.default_rng(1603)
B = 2
q, psi = limbs()
ctx = fh.Context(lib, logN, q, psi)
octx = o.orc_ctx_create(N, 3, q, psi)
a, b = limit_pair(rng, q, N), limit_pair(rng, q, N)
wa, wb = a.copy(), b.copy()
o.orc_ntt_fwd_tower(octx, wa, None, 3, B, 0)
o.orc_ntt_fwd_tower(octx, wb, None, 3, B, 0)
want = np.empty_like(a)
for bb in range(B):
    for l in range(3):
        o.orc_vec_mul(want[bb, l], wa[bb, l], wb[bb, l], N, q[l])
o.orc_ntt_inv_tower(octx, want, None, 3, B, 0)
before, names0 = split_counts(), by_kernel()
got = ctx.tower(a, fmt=fh.COEFFICIENT).PolyMul(ctx.tower(b, fmt=fh.COEFFICIENT)).to_host()
assert np.array_equal(got, want), "fhe_poly_mul differs from the oracle"
assert not (split_counts() - before).any(), f"fhe_poly_mul ran the 6 + 10 pair: {{split_counts() - before}}"
names1 = by_kernel()
results["poly_mul"] = got
results["poly_mul_launches"] = np.array(sorted((k, n - names0.get(k, 0)) for k, n in names1.items() if n - names0.get(k, 0)), dtype=str)
o.orc_ctx_destroy(octx)
ctx.close()
sizeQ, dnum = 2, 1
qq, psiQ, p, psiP = chain(o, logN, sizeQ, dnum, (60, 36, 60))
hy = o.orc_hybrid_create(N, sizeQ, qq, psiQ, len(p), p, psiP, dnum)
allq = np.concatenate([qq, p])
ctx = fh.Context(lib, logN, allq, np.concatenate([psiQ, psiP]))
plan = fh.KeySwitchPlan(ctx, sizeQ, len(p), dnum)
keyB = np.stack([pattern(rng, "max", allq, N) for _ in range(dnum)])
keyA = np.stack([pattern(rng, "mix", allq, N) for _ in range(dnum)])
plan.upload_key(keyB, keyA)
a0 = limit_pair(rng, qq, N)
w0, w1 = np.empty_like(a0), np.empty_like(a0)
for bb in range(B):
    o.orc_hybrid_key_switch(hy, a0[bb], sizeQ, keyB, keyA, w0[bb], w1[bb])
ta0 = ctx.tower(a0)
names0 = by_kernel()
g0, g1 = plan.KeySwitchCore(ta0)
names1 = by_kernel()
assert np.array_equal(g0.to_host(), w0) and np.array_equal(g1.to_host(), w1), "KeySwitchCore differs from the oracle"
results["ks0"], results["ks1"] = g0.to_host(), g1.to_host()
results["ks_launches"] = np.array(sorted((k, n - names0.get(k, 0)) for k, n in names1.items() if n - names0.get(k, 0)), dtype=str)
plan.close()
ctx.close()
o.orc_hybrid_destroy(hy)
np.savez({dump!r}, **results)
print("ok")
"""

# (batch, mode, one operand pattern per tower)
CASES = [(2, "inplace", ("max", "pre")), (3, "inplace", ("mix", "uniform", "max")), (1, "inplace", ("mix",)),
         (3, "oop", ("pre", "mix", "max"))]


def run_child(code, so, split, dump, **kw):
    env = dict(os.environ, FHE_NTT_SPLIT6=str(split))
    for k in ("FHE_NTT_ROW8", "FHE_NTT_ROW8_BATCH", "FHE_NTT_ROW8_X1", "FHE_NTT_T1", "FHE_NTT_HANDOVER"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", code.format(root=ROOT, so=so, split=split, dump=str(dump), **kw)], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def both_settings(code, so, tmp_path, **kw):
    """the child with the pair and without: each checks the oracle and the pair's launch counts, the results of the two are the same words
    (and, where the child records them, the same launches by kernel name)"""
    files = []
    for split in (1, 0):
        files.append(tmp_path / f"split{split}.npz")
        run_child(code, so, split, files[-1], **kw)
    on, off = np.load(files[0]), np.load(files[1])
    assert sorted(on.files) == sorted(off.files) and on.files
    for k in on.files:
        assert np.array_equal(on[k], off[k]), f"{k}: FHE_NTT_SPLIT6=1 and =0 differ"


def test_transforms_on_emulator(tmp_path):
    both_settings(NTT_CHILD, EMU, tmp_path, cases=CASES)


def test_strided_views_of_a_reversed_limb_subset_on_emulator(tmp_path):
    both_settings(VIEWS_CHILD, EMU, tmp_path)


def test_poly_mul_and_key_switch_on_emulator(tmp_path):
    both_settings(CALLERS_CHILD, EMU, tmp_path)


@pytest.mark.gpu
def test_transforms_on_gpu(tmp_path):
    both_settings(NTT_CHILD, HIP, tmp_path, cases=CASES)


@pytest.mark.gpu
def test_strided_views_of_a_reversed_limb_subset_on_gpu(tmp_path):
    both_settings(VIEWS_CHILD, HIP, tmp_path)


@pytest.mark.gpu
def test_poly_mul_and_key_switch_on_gpu(tmp_path):
    both_settings(CALLERS_CHILD, HIP, tmp_path)
