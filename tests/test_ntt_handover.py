"""Hand-over between the two passes of an inverse 4 + 12-stage transform: the batched row pass (ntt_row8.h, HAND) stores the
differences of its last stage unmultiplied and the column pass (ntt_static.h, HAND) does that stage's twiddle products on its way in.  The
intermediate tower differs from the one every other kernel exchanges, the transform's words must not: every case is compared word for word
with the oracle AND with the same calls under FHE_NTT_HANDOVER=0, on the lane emulator (its C++ butterflies follow the generated plans and
abort on a lazy-range violation) and on the GPU.  Forward transforms have no hand-over: every case runs them as well (a round trip pairs the
plain forward kernels with the inverse hand-over pair) and asserts that they launch the plain kernels only.

FHE_NTT_HANDOVER and FHE_NTT_ROW8_BATCH are read once per process, so every setting runs in a child process, which writes its results to
a file; the parent compares the files of the two settings.

Shapes: N = 2^16 is the smallest ring with a 12-stage row pass.  Three limbs: the ring's largest 60-bit prime (the top of the lazy
ranges: 16 q just fits a word), a 36-bit prime (the smallest size on the quotient-estimate reductions) and a 33-bit prime (the
ladder reductions).  Batch 2 is all hand-over, batch 3 a hand-over group and a remainder on the plain pair in one call, batch 4 one group of
FHE_NTT_ROW8_BATCH=4, batch 1 no hand-over at all.  In place, out of place, and through ApproxModUp, which transforms strided views of a
limb subset given in reversed order.  Operands: all q-1, `mix`, the input whose transform is all q-1 (test_parity_edges.py) and uniform
residues.  The 5-stage column kernels of N = 2^17 have no hand-over: that ring must run the plain pair."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libfhe_emu.so")
HIP = os.path.join(ROOT, "openfhe-development_amd", "csrc", "libfhe_hip.so")

PRELUDE = r"""
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np, libs
from openfhe_amd import fhe_hip as fh
from test_parity_edges import pattern, roots
lib = fh.Lib({so!r})
o = libs.load_oracle()
HAND, P = {hand}, {P}
results = {{}}
def limbs(logN, sizes=(60, 36, 33)):
    M = 2 << logN
    q = np.array([o.orc_last_prime(s, M) for s in sizes], np.uint64)
    assert [int(v).bit_length() for v in q] == list(sizes)
    return q, roots(o, logN, q)
def towers(rng, octx, names, q, N, inverse, sel=None):
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
def launches():
    return np.array(lib.handover_counts() + (lib.launch_count("ntt_static_kernel"), lib.launch_count("ntt_row8_batched_kernel"),
                                             lib.launch_count("ntt_row8_kernel")), np.int64)
def expect(B, inverse, ring16=True):
    # launches of ONE transform: (hand-over row, hand-over column, static, batched row, unbatched row8); the hand-over instances are
    # counted under their kernels' names as well
    group = ring16 and B >= P
    hand = bool(group and HAND and inverse)
    rest = B % P if group else B  # polynomials on the plain kernels: their column and their (static, 12-stage) row pass
    if not ring16:
        static = 1 + (1 if B % P or B < P else 0)
    elif hand:
        static = 1 + (2 if rest else 0)  # the hand-over column launch; the remainder's column and row launches
    else:
        static = 1 + (1 if rest else 0)  # one column launch for the whole batch, one row launch for what the batched kernel leaves
    return np.array([int(hand), int(hand), static, 1 if (group or (not ring16 and B >= P)) else 0, 0], np.int64)
"""

NTT_CHILD = PRELUDE + r"""
rng = np.random.default_rng(1201)
for ci, (logN, B, mode, names) in enumerate({cases!r}):
    N = 1 << logN
    q, psi = limbs(logN) if logN == 16 else limbs(logN, (60, 33))
    L = len(q)
    ctx = fh.Context(lib, logN, q, psi)
    octx = o.orc_ctx_create(N, L, q, psi)
    assert len(names) == B
    for inverse in (False, True):
        x = towers(rng, octx, names, q, N, inverse)
        want = x.copy()
        (o.orc_ntt_inv_tower if inverse else o.orc_ntt_fwd_tower)(octx, want, None, L, B, 0)
        if "pre" in names:
            assert np.array_equal(want[names.index("pre")], pattern(rng, "max", q, N)), "the oracle's transforms are inverse to each other"
        fmt = fh.EVALUATION if inverse else fh.COEFFICIENT
        before = launches()
        t = ctx.tower(x, fmt=fmt)
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
        ran = launches() - before
        tag = f"logN={{logN}} B={{B}} {{mode}} {{'inverse' if inverse else 'forward'}}"
        for b in range(B):
            for l in range(L):
                assert np.array_equal(got[b, l], want[b, l]), f"{{tag}}: tower {{names[b]}} limb {{q[l]}} differs from the oracle"
        assert np.array_equal(ran, expect(B, inverse, logN == 16)), f"{{tag}}: launches {{ran}}, expected {{expect(B, inverse, logN == 16)}}"
        results[f"{{ci}}_{{int(inverse)}}"] = got
        before = launches()
        t.SwitchFormat()  # the way back
        assert np.array_equal(t.to_host(), x), f"{{tag}}: round trip"
        assert np.array_equal(launches() - before, expect(B, not inverse, logN == 16)), f"{{tag}}: launches of the way back"
    o.orc_ctx_destroy(octx)
    ctx.close()
np.savez({dump!r}, **results)
print("ok")
"""

# ApproxModUp over the source limbs (2, 1) of a three-limb context, batch 3: the transforms run on strided views (inStride / outStride) of the
# result tower, over a limb subset in reversed order; COEFFICIENT input transforms source and target rows forward, EVALUATION input the
# source rows inverse (dense) and the target rows forward
VIEWS_CHILD = PRELUDE + r"""
rng = np.random.default_rng(1202)
logN, B = 16, 3
N = 1 << logN
q, psi = limbs(logN)
ctx = fh.Context(lib, logN, q, psi)
src, dst = np.array([2, 1], np.uint32), np.array([0], np.uint32)
order = np.concatenate([src, dst])
octx = o.orc_ctx_create(N, 3, q[order], psi[order])  # the oracle's source basis is its first limbs
hatInv, hatPre, hatMod, _, _, mu = libs.crt_tables(q[src], q[dst])
conv = fh.Conv(ctx, src, dst)
for fmt, inEval in ((fh.COEFFICIENT, 0), (fh.EVALUATION, 1)):
    x = towers(rng, octx, ("max", "mix", "pre"), q[src], N, bool(inEval), sel=np.arange(2, dtype=np.uint32))
    want = np.empty((B, 3, N), np.uint64)
    for bb in range(B):
        o.orc_approx_mod_up(octx, 2, 1, x[bb], inEval, hatInv, hatPre, hatMod, mu, want[bb])
    before = launches()
    got = conv.ApproxModUp(ctx.tower(x, limb_idx=src, fmt=fmt)).to_host()
    ran = launches() - before
    assert np.array_equal(got, want), f"ApproxModUp inEval={{inEval}} differs from the oracle"
    # two transforms either way (COEFFICIENT: source rows and target rows forward; EVALUATION: source rows inverse, target rows forward)
    assert np.array_equal(ran[:2], [1, 1] if HAND and inEval else [0, 0]), ran
    assert ran[3] == 2 and ran[4] == 0, ran
    results[f"modup_{{inEval}}"] = got
conv.close()
o.orc_ctx_destroy(octx)
ctx.close()
np.savez({dump!r}, **results)
print("ok")
"""

# The other consumers of the intermediate tower, at N = 2^16 and batch 2: fhe_poly_mul (the fused row kernels read what the plain column pass
# wrote and write what the plain inverse column pass reads) and a HYBRID key switch (its forward transforms carry the load prologue and the
# fused epilogue).  Neither may meet a hand-over tower: fhe_poly_mul launches no hand-over kernel at all, the key switch only for its two
# plain inverse transforms, and both match the oracle.
CALLERS_CHILD = PRELUDE + r"""
from test_parity_edges import chain, limit_pair
rng = np.random.default_rng(1203)
logN, B = 16, 2
N = 1 << logN
q, psi = limbs(logN)
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
before = launches()
fused = lib.launch_count("poly_mul_row_b_kernel")
got = ctx.tower(a, fmt=fh.COEFFICIENT).PolyMul(ctx.tower(b, fmt=fh.COEFFICIENT)).to_host()
assert np.array_equal(got, want), "fhe_poly_mul differs from the oracle"
ran = launches() - before
assert lib.launch_count("poly_mul_row_b_kernel") == fused + 1 and not ran[:2].any() and ran[3] == 0, f"fhe_poly_mul: {{ran}}"
results["poly_mul"] = got
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
before = launches()
g0, g1 = plan.KeySwitchCore(ta0)
ran = launches() - before
assert np.array_equal(g0.to_host(), w0) and np.array_equal(g1.to_host(), w1), "KeySwitchCore differs from the oracle"
# The key switch has two PLAIN inverse transforms with canonical output, both over whole groups: the ciphertext's Q rows before the digit
# decomposition (batch 2) and the P rows of the two accumulators in ApproxModDown (4 towers).  Only they may take the hand-over pair.  Its
# forward transforms -- the digits' (lazy output, load prologue where the ring has one) and ApproxModDown's (fused epilogue) -- keep the
# plain kernels: the launches by kernel name (`ks_launches`, compared between the two settings by the parent) are the same with and
# without hand-over, so no transform was split or re-routed, and all of them are accounted for by the static and batched row kernels.
assert np.array_equal(ran[:2], [2, 2] if HAND else [0, 0]), f"KeySwitchCore: hand-over launches {{ran}}"
assert ran[2] > 2 and ran[3] >= 2 and ran[4] == 0, f"KeySwitchCore: {{ran}}"
results["ks0"], results["ks1"], results["ks_launches"] = g0.to_host(), g1.to_host(), ran[2:]
plan.close()
ctx.close()
o.orc_hybrid_destroy(hy)
np.savez({dump!r}, **results)
print("ok")
"""

# (logN, batch, mode, one operand pattern per tower)
CASES_P2 = [(16, 2, "inplace", ("max", "pre")), (16, 3, "inplace", ("mix", "uniform", "max")), (16, 1, "inplace", ("mix",)),
            (16, 3, "oop", ("pre", "mix", "max")), (17, 2, "inplace", ("max", "mix"))]
CASES_P4 = [(16, 4, "inplace", ("max", "mix", "pre", "uniform"))]


def run_child(code, so, hand, P, dump, forceP=False, **kw):
    env = dict(os.environ, FHE_NTT_HANDOVER=str(hand))
    env.pop("FHE_NTT_ROW8", None)
    env.pop("FHE_NTT_ROW8_BATCH", None)
    if forceP:
        env["FHE_NTT_ROW8_BATCH"] = str(P)
    r = subprocess.run([sys.executable, "-c", code.format(root=ROOT, so=so, hand=hand, P=P, dump=str(dump), **kw)], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def both_settings(code, so, tmp_path, P=2, forceP=False, **kw):
    """the child with hand-over and without: each checks the oracle and its launch counts, the results of the two are the same words"""
    files = []
    for hand in (1, 0):
        files.append(tmp_path / f"hand{hand}.npz")
        run_child(code, so, hand, P, files[-1], forceP, **kw)
    on, off = np.load(files[0]), np.load(files[1])
    assert sorted(on.files) == sorted(off.files) and on.files
    for k in on.files:
        assert np.array_equal(on[k], off[k]), f"{k}: FHE_NTT_HANDOVER=1 and =0 give different words"


def test_transforms_on_emulator(tmp_path):
    both_settings(NTT_CHILD, EMU, tmp_path, cases=CASES_P2)


def test_groups_of_four_on_emulator(tmp_path):
    both_settings(NTT_CHILD, EMU, tmp_path, P=4, forceP=True, cases=CASES_P4)


def test_strided_views_of_a_reversed_limb_subset_on_emulator(tmp_path):
    both_settings(VIEWS_CHILD, EMU, tmp_path)


def test_poly_mul_and_key_switch_keep_the_plain_tower_on_emulator(tmp_path):
    both_settings(CALLERS_CHILD, EMU, tmp_path)


@pytest.mark.gpu
def test_transforms_on_gpu(tmp_path):
    both_settings(NTT_CHILD, HIP, tmp_path, cases=CASES_P2)


@pytest.mark.gpu
def test_groups_of_four_on_gpu(tmp_path):
    both_settings(NTT_CHILD, HIP, tmp_path, P=4, forceP=True, cases=CASES_P4)


@pytest.mark.gpu
def test_strided_views_of_a_reversed_limb_subset_on_gpu(tmp_path):
    both_settings(VIEWS_CHILD, HIP, tmp_path)


@pytest.mark.gpu
def test_poly_mul_and_key_switch_keep_the_plain_tower_on_gpu(tmp_path):
    both_settings(CALLERS_CHILD, HIP, tmp_path)
