"""The N>1 path on CPU: world_size 2, gloo backend.  Each rank shards the ciphertext batch, receives the
evaluation key through the broadcast (the design's only collective) and runs EvalMult + key switching on its
slice; rank results are gathered and compared bit-for-bit with the oracle on the full batch.
The ranks use the TEST-ONLY lane-emulator build (CPU tensors are its "device" memory); on GPUs the same code
runs with backend nccl (= RCCL) and the HIP library."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# TEST-ONLY: hal/bootstrap_batch.cpp compiled against the stock libraries of oracle/_ref (the byte-for-byte reference)
STOCK_BOOT_SO = os.path.join(ROOT, "tests", "hal", "_build", "libfhe_boot_batch_stock.so")
HIP_LIB = os.path.join(ROOT, "openfhe-development_amd", "csrc", "libfhe_hip.so")
EMU_LIB = os.path.join(ROOT, "tests", "emu", "libfhe_emu.so")

WORKER = r'''
import os, sys
import numpy as np
ROOT = sys.argv[1]; out = sys.argv[2]
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, torch.distributed as dist
from openfhe_amd import fhe_hip as fh
from openfhe_amd import shard
import libs
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
lib = fh.Lib(os.path.join(ROOT, "tests", "emu", "libfhe_emu.so"))
o = libs.load_oracle()
logN, sizeQ, dnum, B = 10, 4, 2, 5
N = 1 << logN
q, psiQ = lib.ckks_like_chain(logN, sizeQ, 60, 50)
p, psiP = lib.select_p(logN, q, dnum)
allq = np.concatenate([q, p])
ctx = fh.Context(lib, logN, allq, np.concatenate([psiQ, psiP]))
plan = fh.KeySwitchPlan(ctx, sizeQ, len(p), dnum)
rng = np.random.default_rng(99)          # same seed on every rank: the full batch is known everywhere,
keyB = libs.rand_tower(rng, allq, N, dnum)  # but only rank 0's key copy is used
keyA = libs.rand_tower(rng, allq, N, dnum)
ops = [libs.rand_tower(rng, q, N, B) for _ in range(4)]
keep = shard.broadcast_key(plan, keyB if rank == 0 else None, keyA if rank == 0 else None, "cpu")
lo, hi = shard.shard_range(B, rank, world)
mine = [ctx.tower(x[lo:hi]) for x in ops]
c0, c1 = plan.EvalMult(*mine)
np.savez(out + f".{rank}.npz", lo=lo, hi=hi, c0=c0.to_host(), c1=c1.to_host())
dist.barrier()
if rank == 0:
    hy = o.orc_hybrid_create(N, sizeQ, q, psiQ, len(p), p, psiP, dnum)
    w0 = np.empty_like(ops[0]); w1 = np.empty_like(ops[0])
    for b in range(B):
        o.orc_ckks_eval_mult_relin(hy, ops[0][b], ops[1][b], ops[2][b], ops[3][b], sizeQ, keyB, keyA, w0[b], w1[b])
    got0 = np.empty_like(w0); got1 = np.empty_like(w1); covered = np.zeros(B, bool)
    for r in range(world):
        z = np.load(out + f".{r}.npz")
        got0[z["lo"]:z["hi"]] = z["c0"]; got1[z["lo"]:z["hi"]] = z["c1"]; covered[z["lo"]:z["hi"]] = True
    assert covered.all(), "shards do not cover the batch"
    assert np.array_equal(got0, w0) and np.array_equal(got1, w1), "sharded EvalMult differs from the oracle"
    open(out + ".ok", "w").write("ok")
dist.destroy_process_group()
'''


def test_shard_range_partitions():
    from openfhe_amd import shard
    for total in (0, 1, 5, 8, 1024, 1025):
        for world in (1, 2, 3, 8):
            spans = [shard.shard_range(total, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == total
            assert all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1


def test_two_rank_sharded_eval_mult_with_key_broadcast(tmp_path, backend):
    if "emulator" not in backend.version():
        import pytest
        pytest.skip("CPU (gloo) variant only; the GPU variant is bench.py --gpus N")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    worker = tmp_path / "worker.py"
    worker.write_text(WORKER)
    out = str(tmp_path / "res")
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen([sys.executable, str(worker), ROOT, out], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    assert os.path.exists(out + ".ok"), "\n".join(logs)


WORKER_LT = r"""
import os, sys
import numpy as np
ROOT = sys.argv[1]; out = sys.argv[2]
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch, torch.distributed as dist
from openfhe_amd import fhe_hip as fh
from openfhe_amd import shard
import libs
from test_parity_lt import run_oracle
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
lib = fh.Lib(os.path.join(ROOT, "tests", "emu", "libfhe_emu.so"))
o = libs.load_oracle()
logN, sizeQ, dnum, B, bStep, gStep = 8, 3, 3, 3, 2, 2
N = 1 << logN
q, psiQ = lib.ckks_like_chain(logN, sizeQ, 60, 50)
p, psiP = lib.select_p(logN, q, dnum)
allq = np.concatenate([q, p])
ctx = fh.Context(lib, logN, allq, np.concatenate([psiQ, psiP]))
plan = fh.KeySwitchPlan(ctx, sizeQ, len(p), dnum)
rng = np.random.default_rng(7)   # same seed everywhere: rank 0's copies are the ones that travel
rots = [1, bStep]                # baby step 1, giant step bStep
keys = [(libs.rand_tower(rng, allq, N, dnum), libs.rand_tower(rng, allq, N, dnum)) for _ in rots]
diag = np.stack([libs.rand_tower(rng, allq, N) for _ in range(bStep * gStep)])
c0, c1 = libs.rand_tower(rng, q, N, B), libs.rand_tower(rng, q, N, B)
handles, keep_k = shard.broadcast_rotation_keys(plan, keys if rank == 0 else [None] * len(rots), "cpu")
dt = shard.broadcast_rows(diag if rank == 0 else None, diag.shape, "cpu")
ks = [lib.find_automorphism_index(r, 2 * N) for r in rots]
row = diag[0].size * 8
dptr = [[dt.data_ptr() + (i * bStep + j) * row for j in range(bStep)] for i in range(gStep)]
lo, hi = shard.shard_range(B, rank, world)
g0, g1 = plan.BsgsTransform(ctx.tower(c0[lo:hi]), ctx.tower(c1[lo:hi]), [None, (ks[0], handles[0])], [None, (ks[1], handles[1])], dptr)
np.savez(out + f".{rank}.npz", lo=lo, hi=hi, c0=g0.to_host(), c1=g1.to_host())
dist.barrier()
if rank == 0:
    hy = o.orc_hybrid_create(N, sizeQ, q, psiQ, len(p), p, psiP, dnum)
    want = run_oracle(o, hy, c0, c1, sizeQ, [None, (ks[0],) + keys[0]], [None, (ks[1],) + keys[1]],
                      [[diag[i * bStep + j] for j in range(bStep)] for i in range(gStep)])
    got = np.empty_like(want); covered = np.zeros(B, bool)
    for r in range(world):
        z = np.load(out + f".{r}.npz")
        got[0, z["lo"]:z["hi"]] = z["c0"]; got[1, z["lo"]:z["hi"]] = z["c1"]; covered[z["lo"]:z["hi"]] = True
    assert covered.all() and np.array_equal(got, want), "sharded linear transform differs from the oracle"
    open(out + ".ok", "w").write("ok")
dist.destroy_process_group()
"""


def run_two_ranks(tmp_path, source):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    worker = tmp_path / "worker.py"
    worker.write_text(source)
    out = str(tmp_path / "res")
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS="2")
        procs.append(subprocess.Popen([sys.executable, str(worker), ROOT, out], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=600)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    assert os.path.exists(out + ".ok"), "\n".join(logs)


def test_two_rank_sharded_linear_transform_with_key_and_diagonal_broadcast(tmp_path, backend):
    """config 4's shape of parallelism: ciphertexts sharded over the ranks, the rotation keys and the encoded diagonals
    replicated with one broadcast each, no collective on the data path"""
    if "emulator" not in backend.version():
        import pytest
        pytest.skip("CPU (gloo) variant only")
    run_two_ranks(tmp_path, WORKER_LT)


def test_bench_self_launches_two_ranks_on_gloo(backend):
    """`python bench.py --gpus 2`, invoked exactly like the N=1 run (no torchrun), starts its own ranks; rehearsed on CPU with
    the gloo backend and the test-only emulator build at small sizes (FHE_BENCH_BACKEND / FHE_HIP_LIB).  The JSON line must
    carry n_gpus = 2, per-rank times, the key broadcast to 2 ranks, the scatter + all-gather replication record and the
    per-leg parity fields."""
    import json
    if "emulator" not in backend.version():
        import pytest
        pytest.skip("CPU (gloo) variant only; on GPUs the same command runs with RCCL")
    env = dict(os.environ, FHE_BENCH_BACKEND="gloo", FHE_HIP_LIB=os.path.join(ROOT, "tests", "emu", "libfhe_emu.so"))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--logn", "12", "--limbs", "2",
           "--batch", "4", "--evalmult-logn", "10", "--evalmult-limbs", "5", "--evalmult-batch", "3", "--no-bfv", "--no-lt",
           "--no-hadamard", "--no-cpu-baseline", "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and len(d["ms_per_step_per_rank"]) == 2 and d["scaling"] == "weak"
    assert "2 rank(s)" in d["evalmult"]["eval_key"] and d["evalmult"]["ops_per_s_total"] >= d["evalmult"]["ops_per_s_per_gpu"]
    assert d["evalmult"]["parity"].startswith("bit-exact vs oracle")
    assert d["parity_at_full_size"].startswith("forward NTT of ALL 4 towers")
    assert "scatter" in d["rotation_key_replication"]["how"] and d["rotation_key_replication"]["keys"] == 14
    # the line verifies its own process group: backend and world size as torch.distributed reports them, one record per rank
    dd = d["distributed"]
    assert dd["process_group"]["backend"] == "gloo" and dd["process_group"]["world_size"] == 2 and dd["launcher_world_size"] == 2
    assert sorted(r["rank"] for r in dd["ranks"]) == [0, 1] and len({r["pid"] for r in dd["ranks"]}) == 2
    assert dd["key_replication_GB_per_s"] == d["rotation_key_replication"]["GB_per_s"]


def _bench_on_gloo(world, extra_env=None, extra_args=(), timeout=2400):
    env = dict(os.environ, FHE_BENCH_BACKEND="gloo", FHE_HIP_LIB=os.path.join(ROOT, "tests", "emu", "libfhe_emu.so"))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "OMP_NUM_THREADS"):
        env.pop(k, None)
    env.update(extra_env or {})
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "1", "--warmup", "0", "--logn", "12", "--limbs", "2",
           "--batch", "4", "--evalmult-logn", "10", "--evalmult-limbs", "5", "--evalmult-batch", "3", "--no-bfv", "--no-lt",
           "--no-hadamard", "--no-cpu-baseline", "--full", *extra_args]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)


def test_bench_eight_ranks_on_gloo_with_sharded_bootstrap(backend):
    """The 8-GPU run rehearsed on CPU: `python bench.py --gpus 8` starts eight ranks itself (gloo, the lane emulator,
    small rings).  Checked: the JSON line carries n_gpus = 8 and eight per-rank times; the relinearisation key reaches 8 ranks; the
    rotation-key replication (scatter + all-gather) works with a key count that does not divide by 8 (14 keys: ragged slices); the
    bootstrap leg — config 4 in miniature, 2 ciphertexts per rank = 16 sharded over the ranks, keys generated on rank 0 only and adopted
    from the gathered tensor by the other seven — decrypts correctly on every rank with lockstep == narrow word for word; every rank's
    OpenMP team and stream threads are capped at cores / 8."""
    import json
    if "emulator" not in backend.version():
        pytest.skip("CPU (gloo) variant only; on GPUs the same command runs with RCCL")
    sys.path.insert(0, ROOT)
    from openfhe_amd import boot_batch as bb
    boot = os.path.exists(bb.HIP_SO)
    extra = ["--bootstrap-logn", "8", "--bootstrap-batch", "2", "--bootstrap-threads", "2", "--bootstrap-group", "2", "--bootstrap-wide-threads", "1"]
    out = _bench_on_gloo(8, {"FHE_BENCH_EMU_BOOTSTRAP": "1" if boot else "", "FHE_BENCH_BOOTSTRAP_LIMIT_S": "2000"}, extra if boot else ["--no-bootstrap"])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 8 and len(d["ms_per_step_per_rank"]) == 8 and d["scaling"] == "weak"
    assert d["config"]["global_batch"] == 32 and "x8" in d["config"]["parallelism"]
    assert "8 rank(s)" in d["evalmult"]["eval_key"] and d["evalmult"]["parity"].startswith("bit-exact vs oracle")
    assert d["evalmult"]["ops_per_s_total"] >= d["evalmult"]["ops_per_s_per_gpu"]
    rep = d["rotation_key_replication"]
    assert rep["keys"] == 14 and "8 rank(s)" in rep["how"] and "scatter" in rep["how"]
    if boot:
        b = d["evalbootstrap"]
        assert "error" not in b, b
        cores = os.cpu_count() or 1
        assert b["host_threads"] == {"cores": cores, "ranks": 8, "cap_per_rank": max(1, cores // 8), "stream_threads": min(2, max(1, cores // 8)),
                                     "openmp_team_during_setup": min(8, max(1, cores // 8))}
        assert "8 rank(s)" in b["workload"] and b["max_abs_error_vs_message"] < 1e-2
        assert b["lockstep"]["parity"].startswith("all 2 outputs identical word for word")
        assert b["key_set_GB"] > 0 and b["bootstraps_per_s_total"] >= b["bootstraps_per_s_per_gpu"]


def test_bench_rank_that_stalls_in_the_bootstrap_leg_fails_the_run(backend):
    """a rank that never reaches the leg's first collective: every rank's watchdog ends its process after the limit, rank 0 prints the headline
    line (without the leg's figures) first, and the run's exit status is NOT zero"""
    import json
    if "emulator" not in backend.version():
        pytest.skip("CPU (gloo) variant only")
    sys.path.insert(0, ROOT)
    from openfhe_amd import boot_batch as bb
    if not os.path.exists(bb.HIP_SO):
        pytest.skip("hal/_build/libfhe_boot_batch_hip.so not built")
    out = _bench_on_gloo(3, {"FHE_BENCH_EMU_BOOTSTRAP": "1", "FHE_BENCH_BOOTSTRAP_LIMIT_S": "25", "FHE_BENCH_TEST_STALL_RANK": "2"},
                         ["--bootstrap-logn", "8", "--bootstrap-batch", "1", "--bootstrap-threads", "1"], timeout=900)
    assert out.returncode != 0, "a stalled rank must fail the run"
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert lines, out.stdout[-1500:] + out.stderr[-1500:]
    d = json.loads(lines[-1])
    assert d["n_gpus"] == 3 and "did not finish within 25 s" in d["evalbootstrap"]["error"]


def test_allgather_replication_matches_broadcast(tmp_path, backend):
    """shard.allgather_words (scatter + all-gather) delivers the same words to every rank as the one-shot broadcast, also when
    the table does not divide by the world size"""
    if "emulator" not in backend.version():
        import pytest
        pytest.skip("CPU (gloo) variant only")
    worker = tmp_path / "w.py"
    worker.write_text(r'''
import os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import torch, torch.distributed as dist
from openfhe_amd import shard
dist.init_process_group("gloo")
rank = dist.get_rank()
for shape in [(3, 2, 1031), (7,), (2, 4096)]:
    want = (np.arange(int(np.prod(shape)), dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).reshape(shape)
    got = shard.allgather_words(want if rank == 0 else None, shape, "cpu")
    assert np.array_equal(got.numpy().view(np.uint64), want), (rank, shape)
    ref = shard.broadcast_rows(want if rank == 0 else None, shape, "cpu")
    assert torch.equal(ref, got)
dist.barrier()
if rank == 0:
    open(sys.argv[2], "w").write("ok")
dist.destroy_process_group()
''')
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ok = tmp_path / "ok"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(worker), ROOT, str(ok)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and ok.exists(), out.stdout[-2000:] + out.stderr[-3000:]


WORKER_BOOT = r"""
import os, sys
ROOT = sys.argv[1]; out = sys.argv[2]
sys.path.insert(0, ROOT)
import torch, torch.distributed as dist
from openfhe_amd import boot_batch as bb
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
os.environ["FHE_HIP_LIB"] = os.path.join(ROOT, "tests", "emu", "libfhe_emu.so")   # the lane emulator: CPU tensors are its device memory
os.environ["FHE_HAL_REQUIRE_DEVICE"] = "1"
prng = os.path.join(ROOT, "tests", "hal", "_build", "libdetprng.so")
r = bb.run_rank(8, 8, 2, 1, 1, 0, prng, dist=dist, torch_device="cpu", budget=(1, 1), levels_after=1, dump_path=out + f".rank{rank}.bin", warmup=0)
assert r["ciphertexts"] == 1 and r["max_abs_error"] < 1e-3, r
assert r["key_set_GB"] > 0 and r["key_replication_s"] >= 0
if rank != 0:
    assert r["keygen_s"] < 0.5, "a rank other than 0 generated keys"   # (its key objects are shells: the words arrived by all-gather)
dist.barrier()
dist.destroy_process_group()
"""


def test_two_rank_sharded_bootstrap_batch_with_replicated_keys(tmp_path):
    """BASELINE configs[3] in miniature (N = 2^8, gloo, the lane emulator): 2 ciphertexts, one per rank; rank 0 generates the relinearisation
    and rotation keys, the packed key words reach rank 1 by scatter + all-gather and become the device words of key objects that never had
    any; every rank's cc->EvalBootstrap output is identical, byte for byte, to the stock backend's bootstrap of the same ciphertext"""
    import pytest
    sys.path.insert(0, ROOT)
    from openfhe_amd import boot_batch as bb
    if not (os.path.exists(bb.HIP_SO) and os.path.exists(STOCK_BOOT_SO)):
        pytest.skip("hal/_build/libfhe_boot_batch_hip.so not built (./build.sh hal needs the reference sources)")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    worker = tmp_path / "worker_boot.py"
    worker.write_text(WORKER_BOOT)
    out = str(tmp_path / "boot")
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="1")
        env.pop("FHE_HAL_ALLOW_HOST", None)
        procs.append(subprocess.Popen([sys.executable, str(worker), ROOT, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = [p.communicate(timeout=1200)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)
    # the stock backend, one process, the whole batch
    ref = subprocess.run([sys.executable, "-c", f"""
import sys; sys.path.insert(0, {ROOT!r})
from openfhe_amd import boot_batch as bb
r = bb.run_rank(8, 8, 2, 1, 1, 0, {os.path.join(ROOT, 'tests', 'hal', '_build', 'libdetprng.so')!r}, budget=(1, 1), levels_after=1,
                dump_path={out + '.stock.bin'!r}, warmup=0, so={STOCK_BOOT_SO!r})
"""], env=dict(os.environ, OMP_NUM_THREADS="1"), capture_output=True, text=True, timeout=600)
    assert ref.returncode == 0, ref.stdout + ref.stderr
    stock = open(out + ".stock.bin", "rb").read()
    got = open(out + ".rank0.bin", "rb").read() + open(out + ".rank1.bin", "rb").read()
    assert len(stock) > 10000 and got == stock, "a rank's bootstrapped ciphertext differs from the stock backend's"


def wide_bootstrap(tmp_path, logN, slots, device_lib, timeout=1500, cases=(("g3", 0, 1), ("g2t", 2, 2))):
    """K ciphertexts with equal metadata as ONE ciphertext whose towers hold K towers each (hal/bootstrap_batch.cpp fbb_bootstrap_wide):
    cc->EvalBootstrap runs once, every launch works on K towers.  Fully packed (the CoeffsToSlots / SlotsToCoeffs transforms, the
    conjugation, MultByMonomial and both Chebyshev evaluations): every output identical, byte for byte, to the stock backend's
    bootstrap of the same ciphertext — in one group of 3 and in groups of 2 + 1 on two host threads — and, inside the backend's process, word for word to
    the narrow pass's outputs (fbb_compare_saved: the comparison bench.py's lockstep leg makes)."""
    import pytest
    sys.path.insert(0, ROOT)
    from openfhe_amd import boot_batch as bb
    if not (os.path.exists(bb.HIP_SO) and os.path.exists(STOCK_BOOT_SO)):
        pytest.skip("hal/_build/libfhe_boot_batch_hip.so not built (./build.sh hal needs the reference sources)")
    prng = os.path.join(ROOT, "tests", "hal", "_build", "libdetprng.so")
    out = str(tmp_path / "wide")
    code = f"""
import sys, os; sys.path.insert(0, {ROOT!r})
from openfhe_amd import boot_batch as bb
if len(sys.argv) > 1:
    r = bb.run_rank({logN}, {slots}, 3, 1, 1, 0, {prng!r}, dump_path={out + '.stock.bin'!r}, warmup=0, so={STOCK_BOOT_SO!r})
    sys.exit(0)
r = bb.run_rank({logN}, {slots}, 3, 1, 1, 0, {prng!r}, warmup=0)  # (the narrow pass: first use of every composite, checked against the members)
h = r.pop("handle")
h.save_outputs()
for tag, group, threads in {cases!r}:  # (g2t: groups of 2 + 1 on two host threads / streams, bench.py's way; g2: the same groups one after the other on one thread)
    h.bootstrap_wide(group, 0, threads)
    print(tag, "differing", h.compare_saved())
    h.dump({out!r} + "." + tag + ".bin", 0, 3)
    print(tag, "errors", [h.check(i)[0] for i in range(3)])
h.close()
"""
    env = dict(os.environ, OMP_NUM_THREADS="1", FHE_HIP_LIB=device_lib, FHE_HAL_REQUIRE_DEVICE="1")
    env.pop("FHE_HAL_ALLOW_HOST", None)
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert all(f"{t} differing 0" in p.stdout for t, _, _ in cases), p.stdout[-600:]
    ref = subprocess.run([sys.executable, "-c", code, "stock"], env=dict(os.environ, OMP_NUM_THREADS="1"), capture_output=True, text=True, timeout=timeout)
    assert ref.returncode == 0, ref.stdout + ref.stderr
    stock = open(out + ".stock.bin", "rb").read()
    assert len(stock) > 10000
    for tag, _, _ in cases:
        assert open(out + "." + tag + ".bin", "rb").read() == stock, f"wide bootstrap ({tag}) differs from the stock backend's"


def test_wide_bootstrap_in_lockstep_matches_the_stock_backend(tmp_path):
    """N = 2^8, fully packed, on the lane emulator: one group of 3, groups of 2 + 1 on two host threads, and (back since round 6: the
    round-5 advisor noticed the case had been dropped) groups of 2 + 1 one after the other on ONE host thread"""
    wide_bootstrap(tmp_path, 8, 128, EMU_LIB, cases=(("g3", 0, 1), ("g2t", 2, 2), ("g2", 2, 1)))




@pytest.mark.gpu
def test_wide_bootstrap_in_lockstep_matches_the_stock_backend_on_gpu(tmp_path):
    """N = 2^13, fully packed (4096 slots), on the MI355X: the path behind bench.py's headline config-4 figure"""
    wide_bootstrap(tmp_path, 13, 4096, HIP_LIB)
