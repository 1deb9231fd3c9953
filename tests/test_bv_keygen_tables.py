"""host::bv_keygen_factors (csrc/host_math.h), the factor table of a BV evaluation key, as a stand-alone host program under the
sanitizers: tests/bv_keygen_tables_san.cpp (its own main, host_math.h only) is built with -fsanitize=address,undefined and run on the CPU
over the chains of tests/test_parity_keygen_bv.py (60/60/60, 60/50/51, 60/25/50 bits) plus a one-limb chain, digit sizes 0, 1, 4, 10, 20,
30 and 31, every level of each chain, and the refusals outside the device path.  Host code only: nothing is launched, no device is needed,
nothing is loaded into Python."""
import os
import subprocess


def test_stand_alone_host_program_under_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "bv_keygen_tables_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(root, "tests", "bv_keygen_tables_san.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "bv_keygen_tables_san OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
