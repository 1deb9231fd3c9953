"""FHE_HAL_DEVICE_SAMPLER=blake2: the sampling constructors of DCRTPoly (key generation, encryption) on the device, drawing from the
reference's blake2xb construction in counter mode (csrc/blake2_kernels.h) keyed by 512 bits from the reference's PRNG.

The shim programs of test_hal_shim.py run under the option.  The keys are new (they differ from the default backend's and from the
Philox option's), the computation is the reference's: every decrypted value is right; two runs under the same seeded PRNG write the same
bytes; the sampler ran on the device inside key generation under its own scope (DeviceSamplerBlake2) with no host-mirror execution; and
that scope holds the sampling kernels only: the uniform towers are labelled with the requested format and never transformed, the
Gaussian and ternary towers are transformed outside it."""
import os

import pytest

from test_hal_shim import BFV, BOOT, CKKS_MEMBERS, EMU, HIP, LEVELED, PROGS, assert_ran_on_device, ensure_built, run, setup_stats, values


def run_with(prog, out, mode, logN, device_lib, sampler, extra=()):
    saved = os.environ.get("FHE_HAL_DEVICE_SAMPLER")
    os.environ["FHE_HAL_DEVICE_SAMPLER"] = sampler
    try:
        return run(prog, out, mode, logN, device_lib, extra=extra)
    finally:
        if saved is None:
            os.environ.pop("FHE_HAL_DEVICE_SAMPLER", None)
        else:
            os.environ["FHE_HAL_DEVICE_SAMPLER"] = saved


def blake2_check(tmp_path, mode, logN, device_lib, expect, extra=()):
    ensure_built()
    paths = {n: str(tmp_path / f"{n}.bin") for n in ("stock", "philox", "blake2", "blake2_again")}
    run(PROGS[0], paths["stock"], mode, logN, extra=extra)
    out_philox = run_with(PROGS[1], paths["philox"], mode, logN, device_lib, "1", extra)
    out = run_with(PROGS[1], paths["blake2"], mode, logN, device_lib, "blake2", extra)
    run_with(PROGS[1], paths["blake2_again"], mode, logN, device_lib, "blake2", extra)
    data = {n: open(p, "rb").read() for n, p in paths.items()}
    assert len(data["blake2"]) == len(data["stock"]) > 1000
    assert data["blake2"] != data["stock"], "blake2-sampled keys must not reproduce the reference PRNG's sequential words"
    assert data["blake2"] != data["philox"], "FHE_HAL_DEVICE_SAMPLER=blake2 drew the same words as the Philox option"
    assert data["blake2"] == data["blake2_again"], "the blake2 sampler is deterministic under a seeded reference PRNG (its key is drawn from it)"
    for name, want in expect.items():
        got = values(out, name)
        assert len(got) == len(want) and all(abs(g - w) < 1e-3 for g, w in zip(got, want)), (name, got, want)
    st = setup_stats(out)
    ops, mirror, _ = st.get("DeviceSamplerBlake2", (0, 0, 0))
    assert ops >= 3 and mirror == 0, f"set-up: DeviceSamplerBlake2 {st.get('DeviceSamplerBlake2')}"  # (KeyGen alone: s, a, e)
    assert "DeviceSampler" not in st, "the Philox sampler ran under FHE_HAL_DEVICE_SAMPLER=blake2"
    return out, out_philox


def check_scope(out, out_philox):
    """Set-up window of a program whose samplers all ask for EVALUATION towers.  Under Philox every call is one kernel and one forward
    transform inside the DeviceSampler scope.  Under blake2 the DeviceSamplerBlake2 scope holds one kernel per call and nothing else; the
    Gaussian and ternary towers are transformed outside it (SwitchFormat), the uniform ones not at all (fewer transforms in total, fewer
    device operations inside KeySwitchGenInternal, whose `a` towers are uniform)."""
    b, p = setup_stats(out), setup_stats(out_philox)
    calls, odd = divmod(p["DeviceSampler"][0], 2)
    assert odd == 0 and calls >= 3, p["DeviceSampler"]
    assert b["DeviceSamplerBlake2"][0] == calls, (b["DeviceSamplerBlake2"], calls)
    moved = b.get("SwitchFormat", (0,))[0] - p.get("SwitchFormat", (0,))[0]
    assert 0 < moved < calls, (moved, calls)
    assert b["KeySwitchGenInternal"][0] < p["KeySwitchGenInternal"][0], (b["KeySwitchGenInternal"], p["KeySwitchGenInternal"])


def test_shim_blake2_sampler_on_emulator(tmp_path):
    out, out_philox = blake2_check(tmp_path, "leveled", 11, EMU, LEVELED)
    assert_ran_on_device(out, CKKS_MEMBERS)
    check_scope(out, out_philox)


@pytest.mark.gpu
def test_shim_blake2_sampler_on_gpu(tmp_path):
    out, out_philox = blake2_check(tmp_path, "leveled", 14, HIP, LEVELED)
    assert_ran_on_device(out, CKKS_MEMBERS)
    check_scope(out, out_philox)
    blake2_check(tmp_path, "bootstrap", 12, HIP, BOOT)


@pytest.mark.gpu
def test_shim_blake2_sampler_bfv_on_gpu(tmp_path):
    blake2_check(tmp_path, "bfv", 13, HIP, BFV, extra=("BEHZ", 2))
