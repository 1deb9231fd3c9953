"""BV evaluation-key generation through the C++ host mirror (hal/dcrtpoly_hip.h: BvKeySet, KeyGenBv, KeyGenBvBlake2, KeyGenBvPk,
KeyGenBvPkBlake2) compared word for word with the oracle by tests/hal_keygen_bv.cpp: on CPU linked against the TEST-ONLY emulator build,
with -m gpu against the HIP library."""
import os

import pytest

from test_hal_cpp import ROOT, _run


def test_hal_cpp_keygen_bv_with_oracle_on_emulator(backend, oracle, tmp_path):
    if "emulator" not in backend.version():
        pytest.skip("emulator variant")
    _run(os.path.join(ROOT, "tests", "emu"), "fhe_emu", tmp_path, "hal_keygen_bv", with_oracle=True)


@pytest.mark.gpu
def test_hal_cpp_keygen_bv_with_oracle_on_gpu(hip, oracle, tmp_path):
    _run(os.path.join(ROOT, "openfhe-development_amd", "csrc"), "fhe_hip", tmp_path, "hal_keygen_bv", with_oracle=True)
