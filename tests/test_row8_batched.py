"""The batched 8-residues-per-lane row pass (ntt_row8.h, ntt_row8_batched_kernel: one workgroup transforms the same tile of P
consecutive polynomials of the batch with one fetch of the twiddles) against the oracle, word for word, on the lane emulator (CPU: its
C++ butterflies follow the generated plan and abort on a lazy-range violation) and on the GPU.

FHE_NTT_ROW8_BATCH = 1 / 2 / 4 forces P and FHE_NTT_ROW8_X1 = 0 / 1 the form of the exchange between waves; both are read once per
process, so the forced settings run in a child process.  The P-aligned part of a batch goes to the batched kernel and the other
batch % P polynomials to the unbatched row pass in a second launch: batches 1, 2, 3, 4, 5 and 7 cover no batched launch at all, exact
multiples and remainders 1 and 3.  One tower of all q-1 and one of zeros sit at different positions of one P-group, so that a mix-up of
the register banks cannot cancel."""
import os
import subprocess
import sys

import numpy as np
import pytest

import libs
from openfhe_amd import fhe_hip as fh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libfhe_emu.so")
HIP = os.path.join(ROOT, "openfhe-development_amd", "csrc", "libfhe_hip.so")
KERNEL = "ntt_row8_batched_kernel"
SMALL = (60, 35, 33, 30)  # limbs on the ladder reductions (below 36 bits) next to a 60-bit one

PRELUDE = r"""
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np, libs
from openfhe_amd import fhe_hip as fh
lib = fh.Lib({so!r})
o = libs.load_oracle()
P = {P}
def chain(logN, sizes):  # the last prime of every size asked for; a repeated size descends
    M, q = 2 << logN, []
    for s in sizes:
        v = o.orc_last_prime(s, M)
        while v in q:
            v = o.orc_previous_prime(v, M)
        assert int(v).bit_length() == s and v % M == 1, (logN, s, v)
        q.append(v)
    q = np.array(q, np.uint64)
    return q, np.array([o.orc_root_of_unity(M, int(v)) for v in q], np.uint64)
def edge_towers(x, q):  # zeros and all q-1 at different positions of one P-group (the batch's last whole group, else its first towers)
    B = x.shape[0]
    if B >= 2:
        g = (B // P - 1) * P if B >= P > 1 else 0
        x[g] = 0
        x[g + 1] = (q - np.uint64(1))[:, None]
"""

NTT_CHILD = PRELUDE + r"""
rng = np.random.default_rng(71)
for logN, sizes, B in {shapes!r}:
    N, L = 1 << logN, len(sizes)
    q, psi = chain(logN, sizes)
    ctx = fh.Context(lib, logN, q, psi)
    octx = o.orc_ctx_create(N, L, q, psi)
    before = lib.launch_count({kernel!r})
    x = libs.rand_tower(rng, q, N, B)
    edge_towers(x, q)
    want = x.copy()
    o.orc_ntt_fwd_tower(octx, want, None, L, B, 0)
    t = ctx.tower(x, fmt=fh.COEFFICIENT)
    t.SwitchFormat()
    assert np.array_equal(t.to_host(), want), f"forward mismatch logN={{logN}} sizes={{sizes}} B={{B}}"
    t.SwitchFormat()
    assert np.array_equal(t.to_host(), x), f"round trip mismatch logN={{logN}} sizes={{sizes}} B={{B}}"
    y = libs.rand_tower(rng, q, N, B)  # independent EVALUATION input
    edge_towers(y, q)
    wanti = y.copy()
    o.orc_ntt_inv_tower(octx, wanti, None, L, B, 0)
    t2 = ctx.tower(y, fmt=fh.EVALUATION)
    t2.SwitchFormat()
    assert np.array_equal(t2.to_host(), wanti), f"inverse mismatch logN={{logN}} sizes={{sizes}} B={{B}}"
    n = lib.launch_count({kernel!r}) - before
    assert n == (3 if P > 1 and B >= P else 0), f"the batched kernel ran {{n}} times at logN={{logN}} B={{B}} P={{P}}"
    o.orc_ctx_destroy(octx)
    ctx.close()
print("ok")
"""

# a limb subset, out of place (batch 3), and ApproxModUp, which enters the row pass through strided views (batch 3)
VIEWS_CHILD = PRELUDE + r"""
rng = np.random.default_rng(72)
logN = 16
N = 1 << logN
q, psi = chain(logN, (60, 59, 58))
ctx = fh.Context(lib, logN, q, psi)
octx = o.orc_ctx_create(N, 3, q, psi)
before = lib.launch_count({kernel!r})
sel = np.array([2, 0], np.uint32)
x = libs.rand_tower(rng, q[sel], N, 3)
edge_towers(x, q[sel])
want = x.copy()
o.orc_ntt_fwd_tower(octx, want, sel.ctypes.data, 2, 3, 0)
t = ctx.tower(x, limb_idx=sel, fmt=fh.COEFFICIENT)
out = ctx.empty(3, 2, sel)
lib.check(lib.L.fhe_ntt_fwd_oop(ctx.h, t.ptr, out.ptr, sel.ctypes.data_as(fh.u32p), 2, 3, None))
assert np.array_equal(out.to_host(), want), "out-of-place forward on a limb subset differs"
assert np.array_equal(t.to_host(), x), "out-of-place transform must not touch its input"
assert lib.launch_count({kernel!r}) - before == 1
nQ, nP = 1, 2
src, dst = q[:nQ], q[nQ:]
hatInv, hatPre, hatMod, _, _, mu = libs.crt_tables(src, dst)
conv = fh.Conv(ctx, np.arange(nQ), np.arange(nQ, nQ + nP))
for fmt, inEval in ((fh.EVALUATION, 1), (fh.COEFFICIENT, 0)):
    before = lib.launch_count({kernel!r})
    x = libs.rand_tower(rng, src, N, 3)
    edge_towers(x, src)
    want = np.empty((3, nQ + nP, N), np.uint64)
    for bb in range(3):
        o.orc_approx_mod_up(octx, nQ, nP, x[bb], inEval, hatInv, hatPre, hatMod, mu, want[bb])
    got = conv.ApproxModUp(ctx.tower(x, limb_idx=np.arange(nQ), fmt=fmt))
    assert np.array_equal(got.to_host(), want), f"ApproxModUp inEval={{inEval}}"
    assert lib.launch_count({kernel!r}) - before >= 1, "ApproxModUp took no batched row pass"
conv.close()
o.orc_ctx_destroy(octx)
ctx.close()
print("ok")
"""


def run_child(code, so, P, x1=None, **kw):
    env = dict(os.environ, FHE_NTT_ROW8_BATCH=str(P))
    if x1 is not None:
        env["FHE_NTT_ROW8_X1"] = str(x1)
    r = subprocess.run([sys.executable, "-c", code.format(root=ROOT, so=so, P=P, kernel=KERNEL, **kw)], env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


BATCHES = (1, 2, 3, 4, 5, 7)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("sizes", [(60, 60), SMALL], ids=["60x2", "ladder"])
@pytest.mark.parametrize("P", [2, 4])
def test_batch_remainders_on_emulator(P, sizes, B):
    run_child(NTT_CHILD, EMU, P, shapes=[(16, sizes, B)])


@pytest.mark.parametrize("x1", [0, 1])
def test_both_exchange_forms_and_2_17_on_emulator(x1):
    """both forms of the exchange between waves at P = 2 and P = 4 (batch 5: a whole group and a remainder), and the 2^17 ring"""
    run_child(NTT_CHILD, EMU, 2, x1, shapes=[(16, (60, 33), 3), (17, (60,), 3)])
    run_child(NTT_CHILD, EMU, 4, x1, shapes=[(16, (60, 33), 5)])


def test_views_on_emulator():
    run_child(VIEWS_CHILD, EMU, 2)


def test_forced_unbatched_runs_no_batched_kernel_on_emulator():
    run_child(NTT_CHILD, EMU, 1, shapes=[(16, (60,), 2)])


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [(60, 60), SMALL], ids=["60x2", "ladder"])
@pytest.mark.parametrize("P", [2, 4])
def test_batch_remainders_on_gpu(P, sizes):
    run_child(NTT_CHILD, HIP, P, shapes=[(16, sizes, B) for B in BATCHES])


@pytest.mark.gpu
@pytest.mark.parametrize("x1", [0, 1])
def test_both_exchange_forms_and_2_17_on_gpu(x1):
    run_child(NTT_CHILD, HIP, 2, x1, shapes=[(16, (60, 33), 3), (17, SMALL, 3)])
    run_child(NTT_CHILD, HIP, 4, x1, shapes=[(16, (60, 33), 5)])


@pytest.mark.gpu
def test_views_on_gpu():
    run_child(VIEWS_CHILD, HIP, 2)  # (batch 3: one group of two and a remainder)


def default_path(backend, o):
    """N = 2^16, batch 4, default settings: the row kernel launch_pass names for 12 stages is the one that runs"""
    counts = {k: backend.launch_count(k) for k in (KERNEL, "ntt_row8_kernel", "ntt_static_kernel")}
    logN, N, M = 16, 1 << 16, 2 << 16
    q = np.array([o.orc_last_prime(60, M), o.orc_last_prime(45, M)], np.uint64)
    psi = np.array([o.orc_root_of_unity(M, int(v)) for v in q], np.uint64)
    ctx = fh.Context(backend, logN, q, psi)
    octx = o.orc_ctx_create(N, 2, q, psi)
    x = libs.rand_tower(np.random.default_rng(73), q, N, 4)
    x[1] = 0
    x[2] = (q - np.uint64(1))[:, None]
    want = x.copy()
    o.orc_ntt_fwd_tower(octx, want, None, 2, 4, 0)
    t = ctx.tower(x, fmt=fh.COEFFICIENT)
    t.SwitchFormat()
    assert np.array_equal(t.to_host(), want)
    t.SwitchFormat()
    assert np.array_equal(t.to_host(), x)
    o.orc_ctx_destroy(octx)
    ctx.close()
    ran = {k: backend.launch_count(k) - v for k, v in counts.items()}
    # the default of launch_pass for 12 stages (fhe_hip.cpp: kRow8BatchDefault = 2, batch 4 = two whole groups): the batched kernel for
    # both row passes, the static kernel for the two column passes, and no unbatched row pass
    assert ran == {KERNEL: 2, "ntt_row8_kernel": 0, "ntt_static_kernel": 2}, ran


def test_default_path_on_emulator():
    default_path(fh.Lib(EMU), libs.load_oracle())


@pytest.mark.gpu
def test_default_path_on_gpu():
    default_path(fh.Lib(HIP), libs.load_oracle())
