// TEST: a stand-alone host program for the sanitizers.  It includes the product's host_math.h, calls host::mod_reduce_multi_tables (and,
// through it, rescale_multi_tables) over the modulus sets of tests/test_mod_reduce_multi_tables.py with exactly-sized heap buffers, and
// checks the identity the fused pass rests on, W[k][i] * C[i] = t * prod_{j>=k} qDrop[j]^-1 mod qKeep[i], and S[k] * t = s mod qDrop[k].
// Built with -fsanitize=address,undefined and run on the CPU (test_mod_reduce_multi_tables.py); nothing touches a device.
#include <cstdio>
#include <vector>

#include "../openfhe-development_amd/csrc/host_math.h"

using namespace fhe::host;

static bool prime(uint64_t n) {  // Miller-Rabin with the bases that decide every n < 2^64
    if (n < 2)
        return false;
    for (uint64_t p : {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37}) {
        if (n == p)
            return true;
        if (n % p == 0)
            return false;
    }
    uint64_t d = n - 1;
    int r      = 0;
    for (; d % 2 == 0; d /= 2)
        ++r;
    for (uint64_t a : {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37}) {
        uint64_t y = powmod(a, d, n);
        if (y == 1 || y == n - 1)
            continue;
        bool composite = true;
        for (int i = 1; i < r && composite; ++i) {
            y = mulmod(y, y, n);
            composite = y != n - 1;
        }
        if (composite)
            return false;
    }
    return true;
}
static uint64_t prime_below(uint64_t n) {
    for (--n; !prime(n); --n) {
    }
    return n;
}

int main() {
    const std::vector<uint64_t> qd = {prime_below(1ull << 60), prime_below(1ull << 50), prime_below(1ull << 25), prime_below(1ull << 59)};
    const std::vector<uint64_t> qk = {prime_below(1ull << 61), prime_below(1ull << 40), prime_below(1ull << 17), prime_below(1ull << 36)};
    const std::vector<uint64_t> ts = {2, 3, 65537, 786433, (1ull << 31) - 1, (1ull << 40) + 15, qk[0] + 2};
    int checked = 0;
    for (uint32_t d = 1; d <= 4; ++d)
        for (uint32_t nKeep = 1; nKeep <= qk.size(); ++nKeep)
            for (uint64_t t : ts)
                for (int scaled = 0; scaled < 2; ++scaled) {
                    const uint64_t s = scaled ? (1ull << 59) + 12345 + d : 1;
                    std::vector<uint64_t> sd(d), sk(nKeep);
                    for (uint32_t k = 0; k < d; ++k)
                        sd[k] = s % qd[k];
                    for (uint32_t i = 0; i < nKeep; ++i)
                        sk[i] = s % qk[i];
                    // exactly-sized buffers: a write past any of them is the sanitizer's to report
                    std::vector<uint64_t> B(2 * d * d), W(2 * (size_t)d * nKeep), C(2 * nKeep), S(2 * d);
                    mod_reduce_multi_tables(qd.data(), d, qk.data(), nKeep, t, scaled ? sd.data() : nullptr, scaled ? sk.data() : nullptr,
                                            B.data(), W.data(), C.data(), S.data());
                    for (uint32_t k = 0; k < d; ++k) {
                        if (mulmod(S[2 * k], t % qd[k], qd[k]) != s % qd[k] || S[2 * k + 1] != shoup(S[2 * k], qd[k])) {
                            std::printf("mod_reduce_multi_tables_san: S[%u] wrong (d %u, t %llu)\n", k, d, (unsigned long long)t);
                            return 1;
                        }
                        for (uint32_t j = k + 1; j < d; ++j)
                            if (mulmod(B[2 * (k * d + j)], qd[k] % qd[j], qd[j]) != 1) {
                                std::printf("mod_reduce_multi_tables_san: B[%u][%u] wrong\n", k, j);
                                return 2;
                            }
                    }
                    for (uint32_t i = 0; i < nKeep; ++i)
                        for (uint32_t k = 0; k < d; ++k) {
                            uint64_t tail = t % qk[i];
                            for (uint32_t j = k; j < d; ++j)
                                tail = mulmod(tail, invmod(qd[j] % qk[i], qk[i]), qk[i]);
                            if (mulmod(W[2 * ((size_t)k * nKeep + i)], C[2 * i], qk[i]) != tail) {
                                std::printf("mod_reduce_multi_tables_san: W[%u][%u] * C wrong (d %u, t %llu)\n", k, i, d, (unsigned long long)t);
                                return 3;
                            }
                        }
                    ++checked;
                }
    std::printf("mod_reduce_multi_tables_san OK (%d table sets)\n", checked);
    return 0;
}
