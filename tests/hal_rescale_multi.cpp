// TEST: DCRTPolyHip::DropLastElementsAndScale of the C++ host mirror (openfhe-development_amd/hal/dcrtpoly_hip.h) against the oracle's
// DropLastElementAndScale applied `levels` times (oracle/fhe_oracle.h), with and without the scalar and the level drop, on a small ring
// (the member's loop) and on a ring of two passes (the fused form).  Linked against the TEST-ONLY emulator build on CPU or the HIP
// library on a GPU box.
#include <cstdio>
#include <random>

#include "../openfhe-development_amd/hal/dcrtpoly_hip.h"
#include "../oracle/fhe_oracle.h"

using namespace fhehip;
typedef std::vector<uint64_t> Vec;

static std::mt19937_64 gen(20261020);
#define REQUIRE(cond, code)                                                    \
    if (!(cond)) {                                                             \
        std::printf("hal_rescale_multi: check %d failed (%s)\n", code, #cond); \
        return code;                                                           \
    }

static int one_ring(uint32_t logN, int base) {
    const uint32_t N = 1u << logN, L = 5, levels = 2, B = 2;
    Vec q(L), psi(L);
    check(fhe_param_dcrt_chain(2 * N, L, 55, q.data(), psi.data()));
    auto params   = std::make_shared<Params>(2 * N, q, psi);
    orc_ctx* octx = orc_ctx_create(N, L, q.data(), psi.data());
    Vec x((size_t)B * L * N), scale(L);
    for (uint32_t b = 0; b < B; ++b)
        for (uint32_t l = 0; l < L; ++l)
            for (uint32_t i = 0; i < N; ++i)
                x[((size_t)b * L + l) * N + i] = gen() % q[l];
    for (uint32_t l = 0; l < L; ++l)
        scale[l] = 1 + gen() % (q[l] - 1);
    // the loop of the reference on the host: the scalar's residues first, then one limb at a time
    auto loop = [&](bool scaled, uint32_t nOut) {
        Vec out((size_t)B * nOut * N);
        for (uint32_t b = 0; b < B; ++b) {
            Vec cur(x.begin() + (size_t)b * L * N, x.begin() + (size_t)(b + 1) * L * N);
            if (scaled)
                for (uint32_t l = 0; l < L; ++l)
                    for (uint32_t i = 0; i < N; ++i)
                        cur[(size_t)l * N + i] = (uint64_t)((unsigned __int128)cur[(size_t)l * N + i] * scale[l] % q[l]);
            for (uint32_t k = 0; k < levels; ++k) {
                Vec nxt((size_t)(L - 1 - k) * N);
                orc_drop_last_element_and_scale(octx, cur.data(), L - k, nxt.data());
                cur = nxt;
            }
            std::copy(cur.begin(), cur.begin() + (size_t)nOut * N, out.begin() + (size_t)b * nOut * N);
        }
        return out;
    };
    auto fresh = [&]() {
        DCRTPolyHip t(params, L, EVALUATION, B);
        t.SetValues(x, EVALUATION);
        return t;
    };
    auto a = fresh();
    a.DropLastElementsAndScale(levels);
    REQUIRE(a.GetNumOfElements() == L - levels && a.GetValues() == loop(false, L - levels), base + 1);
    auto b = fresh();
    b.DropLastElementsAndScale(levels, scale);
    REQUIRE(b.GetValues() == loop(true, L - levels), base + 2);
    auto c = fresh();
    c.DropLastElementsAndScale(levels, scale, 2);
    REQUIRE(c.GetNumOfElements() == 2 && c.GetValues() == loop(true, 2), base + 3);
    bool threw = false;
    try {
        auto d = fresh();
        d.DropLastElementsAndScale(L);
    }
    catch (const Error&) {
        threw = true;
    }
    REQUIRE(threw, base + 4);
    orc_ctx_destroy(octx);
    return 0;
}

int main() {
    if (int rc = one_ring(8, 100))
        return rc;
    if (int rc = one_ring(13, 200))
        return rc;
    std::printf("hal_rescale_multi OK\n");
    return 0;
}
