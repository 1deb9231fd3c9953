"""The host constants of the fused BGV level alignment (host_math.h mod_reduce_multi_tables, through fhe_mod_reduce_multi_host_tables)
against their closed forms over Python integers.  Host code only: nothing is launched, no device is needed.

  B[j][k] = q_{r_j}^-1 mod q_{r_k}, j < k          the triangle of the chain
  S[k]    = s * t^-1 mod q_{r_k}                   sigma_k, the chain's scalar slot
  W[k][i] = (t mod q_i) * s^-1 * prod_{j<k} q_{r_j} mod q_i
  C[i]    = s * prod_k q_{r_k}^-1 mod q_i
and the identity the pass rests on, W[k][i] * C[i] = t * prod_{j>=k} q_{r_j}^-1, which is what step k's delta is multiplied by on its way
through the remaining steps of the member (dcrtpoly-impl.h:736-755)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

u64p = C.POINTER(C.c_uint64)


def is_prime(n):  # Miller-Rabin with the bases that decide every n < 2^64
    if n < 2:
        return False
    d, r = n - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if a % n == 0:
            continue
        y = pow(a, d, n)
        if y in (1, n - 1):
            continue
        for _ in range(r - 1):
            y = y * y % n
            if y == n - 1:
                break
        else:
            return False
    return True


def prime_below(n):
    n -= 1
    while not is_prime(n):
        n -= 1
    return n


# the 60-bit chain of the parity tests' shape, and the 60 / 25 / 50-bit mix with further sizes around it
QD = [prime_below(1 << 60), prime_below(1 << 50), prime_below(1 << 25), prime_below(1 << 59)]
QK = [prime_below(1 << 61), prime_below(1 << 40), prime_below(1 << 17), prime_below(1 << 36)]
TS = (2, 3, 65537, 786433, (1 << 31) - 1, (1 << 40) + 15, QK[0] + 2)


@pytest.fixture
def lib(backend):
    """the emulator build of the library's host code without a GPU, the product library with one: the same host_math.h"""
    return backend


def tables(lib, drop, keep, t, sd, sk):
    d = len(drop)
    arr = lambda v: np.array(v, np.uint64)
    p = lambda a: a.ctypes.data_as(u64p)
    B, W = np.zeros((d, d, 2), np.uint64), np.zeros((d, len(keep), 2), np.uint64)
    Cc, S = np.zeros((len(keep), 2), np.uint64), np.zeros((d, 2), np.uint64)
    a_d, a_k = arr(drop), arr(keep)
    a_sd, a_sk = (arr(sd), arr(sk)) if sd is not None else (None, None)
    st = lib.L.fhe_mod_reduce_multi_host_tables(p(a_d), d, p(a_k), len(keep), t, p(a_sd) if sd is not None else None,
                                                p(a_sk) if sk is not None else None, p(B), p(W), p(Cc), p(S))
    return st, B, W, Cc, S


@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("scaled", [False, True])
def test_tables_against_the_closed_forms(lib, d, scaled):
    rng = np.random.default_rng(3 + d)
    shoup = lambda v, m: (v << 64) // m
    for t in TS:
        drop, keep = QD[:d], QK
        s = int(rng.integers(2, 1 << 62)) if scaled else 1
        sd = [s % v for v in drop] if scaled else None
        sk = [s % v for v in keep] if scaled else None
        st, B, W, Cc, S = tables(lib, drop, keep, t, sd, sk)
        assert st == 0, lib.L.fhe_last_error()
        for k in range(d):
            sigma = s * pow(t, -1, drop[k]) % drop[k]
            assert (int(S[k, 0]), int(S[k, 1])) == (sigma, shoup(sigma, drop[k])), (t, k)
            for j in range(d):
                v = pow(drop[k], -1, drop[j]) if k < j else 0
                assert (int(B[k, j, 0]), int(B[k, j, 1])) == (v, shoup(v, drop[j]) if k < j else 0)
        for i, m in enumerate(keep):
            prod = 1
            for k in range(d):
                w = t * pow(s, -1, m) * prod % m
                assert (int(W[k, i, 0]), int(W[k, i, 1])) == (w, shoup(w, m)), (t, d, k, i)
                prod = prod * drop[k] % m
            c = s * pow(prod, -1, m) % m
            assert (int(Cc[i, 0]), int(Cc[i, 1])) == (c, shoup(c, m))
            for k in range(d):
                tail = t
                for j in range(k, d):
                    tail = tail * pow(drop[j], -1, m) % m
                assert int(W[k, i, 0]) * c % m == tail % m


def test_the_fused_form_equals_the_members_steps_on_integers(lib):
    """the identity itself, pointwise in the coefficient domain, with the library's constants: random residues and the rounding edges of
    SwitchModulus, against DCRTPolyImpl::ModReduce applied step by step"""
    rng = np.random.default_rng(11)

    def sm(v, qs, qn):
        return (v - qs if v > qs // 2 else v) % qn

    for trial in range(200):
        d = 1 + trial % 3
        drop, keep = [QD[(trial + k) % 4] for k in range(d)], QK[:1 + trial % 4]
        t = TS[trial % len(TS)]
        s = int(rng.integers(2, 1 << 62)) if trial % 2 else 1
        st, B, W, Cc, S = tables(lib, drop, keep, t, [s % v for v in drop] if s != 1 else None, [s % v for v in keep] if s != 1 else None)
        assert st == 0
        edge = lambda q: [0, 1, q // 2, q // 2 + 1, q - 1][int(rng.integers(0, 5))]
        xd = [edge(q) if trial % 5 == 0 else int(rng.integers(0, q)) for q in drop]
        xk = [int(rng.integers(0, q)) for q in keep]
        # the member, step by step: rows keep + the rows still to drop, times the scalar first
        rows = [(v * s) % q for v, q in zip(xk + xd[::-1], keep + drop[::-1])]
        mods = keep + drop[::-1]
        for k in range(d):
            ql, last = mods[-1], rows[-1]
            delta = last * ((-pow(t, -1, ql)) % ql) % ql
            rows = [((v + t * sm(delta, ql, q)) * pow(ql, -1, q)) % q for v, q in zip(rows[:-1], mods[:-1])]
            mods = mods[:-1]
        # the fused form with the tables
        rho = []
        for k in range(d):
            v = xd[k] * int(S[k, 0]) % drop[k]
            for j in range(k):
                v = (v - sm(rho[j], drop[j], drop[k])) * int(B[j, k, 0]) % drop[k]
            rho.append(v)
        for i, q in enumerate(keep):
            r = sum(sm(rho[k], drop[k], q) * int(W[k, i, 0]) for k in range(d)) % q
            assert (xk[i] - r) * int(Cc[i, 0]) % q == rows[i], (trial, i)


def test_argument_errors(lib):
    drop, keep = QD[:2], QK[:2]

    def bad(st, text):
        assert st != 0 and text in lib.L.fhe_last_error().decode()

    bad(tables(lib, drop, keep, 1, None, None)[0], "t must be invertible")
    bad(tables(lib, drop, keep, 3 * drop[1], None, None)[0], "t must be invertible")
    bad(tables(lib, drop, keep, 65537, [1, 1], [1, 0])[0], "a zero scalar residue has no inverse")
    bad(tables(lib, QD + QD[:1], keep, 65537, None, None)[0], "bad sizes")


def test_stand_alone_host_program_under_sanitizers(tmp_path):
    """tests/mod_reduce_multi_tables_san.cpp (its own main, host_math.h only) built with -fsanitize=address,undefined and run on the CPU
    over the same modulus sets"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "mod_reduce_multi_tables_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(root, "tests", "mod_reduce_multi_tables_san.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mod_reduce_multi_tables_san OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
