"""bench.py's plain run and --dump-outputs at a small size: one JSON line with the headline fields only, `--steps` timed steps, and
the dumped sample equal to what the last step computed (the seeded input after fwd + inv, and its forward transform by the oracle).
`emu` runs the TEST-ONLY lane emulator build on the CPU; `hip` the product library on the GPU."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _words(a):
    """float64 [..., 2] = (high 32 bits, low 32 bits) -> uint64 [...]"""
    assert a.dtype == np.float64 and a.shape[-1] == 2
    return (a[..., 0].astype(np.uint64) << np.uint64(32)) | a[..., 1].astype(np.uint64)


def test_bench_plain_run_dumps_the_last_step(tmp_path, backend, oracle):
    import bench  # (the repository root is on sys.path: tests/conftest.py)
    logN, L, B, steps = 12, 3, 5, 3
    N = 1 << logN
    env = dict(os.environ, FHE_HIP_LIB=backend.path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "FHE_BENCH_FORCE_DIST"):
        env.pop(k, None)
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--logn", str(logN),
           "--limbs", str(L), "--batch", str(B), "--dump-outputs", str(out)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["steps"] == steps and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["full"] is False
    assert r["unit"] == "GB/s" and r["higher_is_better"] is True and r["dtype"] == "u64" and r["value"] >= 0
    assert r["metric"].startswith("NTT GB/s") and r["n_gpus"] == 1
    for extra in ("evalmult", "roofline", "cpu_baseline", "parity_at_full_size", "hadamard", "power"):
        assert extra not in r, extra

    rows = np.load(out / "sample_rows.npy")
    assert rows.dtype == np.float64
    rows = rows.astype(np.int64)
    assert len(rows) == B * L and len(set(rows.tolist())) == len(rows)  # a small batch is dumped whole
    rt, fw = _words(np.load(out / "ntt_roundtrip.npy")), _words(np.load(out / "ntt_forward.npy"))
    assert rt.shape == fw.shape == (len(rows), N)
    q, psi = backend.dcrt_chain(logN, L, 60)
    host = bench.host_seed_towers(q, N, B, 2, 8)  # the bench's seeded input (rank 0): tower t is seed tower t % 8
    fwd = host.copy()
    octx = oracle.orc_ctx_create(N, L, q, psi)
    oracle.orc_ntt_fwd_tower(octx, fwd, None, L, fwd.shape[0], 0)
    oracle.orc_ctx_destroy(octx)
    seed = (rows // L) % host.shape[0]
    assert np.array_equal(rt, host[seed, rows % L]), "dumped round trip differs from the seeded input"
    assert np.array_equal(fw, fwd[seed, rows % L]), "dumped forward transform differs from the oracle"
