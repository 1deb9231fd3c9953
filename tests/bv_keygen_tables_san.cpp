// TEST: a stand-alone host program for the sanitizers.  It includes the product's host_math.h, calls host::bv_keygen_factors over the
// chains of tests/test_parity_keygen_bv.py plus a one-limb chain and digit size 1, and checks every entry of the table against
// 2^(baseBits * k) mod q_i computed by repeated doubling, the tower order (limb after limb, least significant window first), the window
// counts, and that nothing is returned outside the device path (baseBits > 31, a window beyond the word, no limbs).
// Built with -fsanitize=address,undefined and run on the CPU (test_bv_keygen_tables.py); nothing touches a device.
#include <cstdio>
#include <vector>

#include "../openfhe-development_amd/csrc/host_math.h"

using namespace fhe::host;

static int fail(const char* what, uint32_t r, uint32_t d, uint32_t i) {
    std::printf("bv_keygen_tables_san: %s (baseBits %u, tower %u, limb %u)\n", what, r, d, i);
    return 1;
}

int main() {
    // moduli of 60/60/60, 60/50/51, 60/25/50 bits and one limb alone (the table needs odd moduli of these sizes, not primes)
    const std::vector<std::vector<uint64_t>> chains = {
        {(1ull << 60) - 93, (1ull << 60) - 107, (1ull << 60) - 173},
        {(1ull << 60) - 93, (1ull << 50) - 27, (1ull << 51) - 129},
        {(1ull << 60) - 93, (1ull << 25) - 39, (1ull << 50) - 27},
        {(1ull << 59) - 55},
    };
    int checked = 0;
    for (const auto& q : chains)
        for (uint32_t sizeQ = 1; sizeQ <= q.size(); ++sizeQ)
            for (uint32_t r : {0u, 1u, 4u, 10u, 20u, 30u, 31u}) {
                std::vector<uint64_t> f(7, 99);  // (is cleared and resized inside)
                const uint32_t D0 = bv_keygen_factors(q.data(), sizeQ, r, f);
                uint32_t want = 0;
                for (uint32_t i = 0; i < sizeQ; ++i)
                    want += r ? (bitlen(q[i]) + r - 1) / r : 1;
                if (D0 != want || f.size() != (size_t)D0 * sizeQ)
                    return fail("tower count", r, D0, sizeQ);
                uint32_t d = 0;
                for (uint32_t i = 0; i < sizeQ; ++i) {
                    const uint32_t nW = r ? (bitlen(q[i]) + r - 1) / r : 1;
                    uint64_t power    = 1;  // 2^(r k) mod q_i by doubling
                    for (uint32_t k = 0; k < nW; ++k, ++d) {
                        for (uint32_t j = 0; j < sizeQ; ++j)
                            if (f[(size_t)d * sizeQ + j] != (j == i ? power : 0))
                                return fail("entry", r, d, j);
                        for (uint32_t s = 0; s < r; ++s)
                            power = (power * 2) % q[i];
                    }
                }
                ++checked;
            }
    // outside the device path: no towers and no table
    std::vector<uint64_t> f(3, 1);
    if (bv_keygen_factors(chains[0].data(), 3, 32, f) != 0 || !f.empty())
        return fail("baseBits 32 accepted", 32, 0, 0);
    f.assign(3, 1);
    if (bv_keygen_factors(chains[0].data(), 0, 10, f) != 0 || !f.empty())
        return fail("no limbs accepted", 10, 0, 0);
    f.assign(3, 1);
    if (bv_keygen_factors(nullptr, 3, 10, f) != 0 || !f.empty())
        return fail("null chain accepted", 10, 0, 0);
    const uint64_t wide = ~0ull - 58;  // 64 bits at 31 bits a window: three windows, 93 bits, beyond the word
    f.assign(3, 1);
    if (bv_keygen_factors(&wide, 1, 31, f) != 0 || !f.empty())
        return fail("a window beyond the word accepted", 31, 0, 0);
    std::printf("bv_keygen_tables_san OK (%d tables)\n", checked);
    return 0;
}
