// TEST: the decryption members of the C++ host mirror (openfhe-development_amd/hal/dcrtpoly_hip.h) against the oracle (oracle/fhe_oracle.h):
// ModReduceChain and ModReduceToT against the loop of orc_mod_reduce on COEFFICIENT towers, BgvDecrypt against DecryptCore with orc_vec_mul /
// orc_vec_add, orc_ntt_inv_tower and that loop.  Linked against the TEST-ONLY emulator build on CPU or the HIP library on a GPU box.
#include <cstdio>
#include <random>

#include "../openfhe-development_amd/hal/dcrtpoly_hip.h"
#include "../oracle/fhe_oracle.h"

using namespace fhehip;
typedef std::vector<uint64_t> Vec;

static std::mt19937_64 gen(20261019);
static Vec randTower(const Vec& mods, uint32_t N, uint32_t lead) {
    Vec v((size_t)lead * mods.size() * N);
    for (uint32_t t = 0; t < lead; ++t)
        for (size_t l = 0; l < mods.size(); ++l)
            for (uint32_t i = 0; i < N; ++i)
                v[((size_t)t * mods.size() + l) * N + i] = gen() % mods[l];
    return v;
}
static DCRTPolyHip upload(const std::shared_ptr<Params>& p, const Vec& v, uint32_t limbs, uint32_t batch, Format f) {
    DCRTPolyHip x(p, limbs, f, batch);
    x.SetValues(v, f);
    return x;
}
#define REQUIRE(cond, code)                                                  \
    if (!(cond)) {                                                           \
        std::printf("hal_bgv_decrypt: check %d failed (%s)\n", code, #cond); \
        return code;                                                         \
    }

int main() {
    const uint32_t logN = 8, N = 1u << logN, L = 19, B = 2;
    const uint64_t t = 65537;
    Vec q(L), psi(L);
    check(fhe_param_dcrt_chain(2 * N, L, 55, q.data(), psi.data()));
    auto params   = std::make_shared<Params>(2 * N, q, psi);
    orc_ctx* octx = orc_ctx_create(N, L, q.data(), psi.data());

    // `levels` calls of the member on every tower of x [B][n][N], COEFFICIENT
    auto loop = [&](Vec x, uint32_t n, uint32_t levels) {
        for (uint32_t k = 0; k < levels; ++k, --n) {
            Vec y((size_t)B * (n - 1) * N);
            for (uint32_t b = 0; b < B; ++b)
                orc_mod_reduce(octx, &x[(size_t)b * n * N], n, t, 0, &y[(size_t)b * (n - 1) * N]);
            x.swap(y);
        }
        return x;
    };
    auto modT = [&](const Vec& x0) {  // x0 [B][1][N] modulo q[0]
        Vec r(x0.size());
        for (size_t i = 0; i < x0.size(); ++i)
            r[i] = x0[i] > q[0] / 2 ? (t - (q[0] - x0[i]) % t) % t : x0[i] % t;
        return r;
    };

    {  // 17 of 18 limbs go: one full chunk of 16 and a rest; then 3 levels of 19
        const uint32_t n = 18;
        const Vec ql(q.begin(), q.begin() + n);
        const Vec x = randTower(ql, N, B);
        auto X = upload(params, x, n, B, COEFFICIENT);
        const Vec last = loop(x, n, n - 1);
        REQUIRE(X.ModReduceToT(t) == modT(last), 101);
        X.ModReduceChain(n - 1, t);
        REQUIRE(X.GetNumOfElements() == 1 && X.GetFormat() == COEFFICIENT && X.GetValues() == last, 102);
        const Vec y = randTower(q, N, B);
        auto Y = upload(params, y, L, B, COEFFICIENT);
        Y.ModReduceChain(3, t);
        REQUIRE(Y.GetNumOfElements() == L - 3 && Y.GetValues() == loop(y, L, 3), 103);
        bool thrown = false;
        try {
            Y.ModReduceChain(L - 3, t);
        } catch (const Error&) {
            thrown = true;
        }
        REQUIRE(thrown && Y.GetNumOfElements() == L - 3, 104);
    }
    for (uint32_t nElem = 2; nElem <= 3; ++nElem) {  // b = c0 + c1*s (+ c2*s^2), INTT, the chain, the residues modulo t
        const uint32_t n = 4;
        const Vec ql(q.begin(), q.begin() + n);
        const Vec s = randTower(ql, N, 1);
        std::vector<Vec> c;
        for (uint32_t e = 0; e < nElem; ++e)
            c.push_back(randTower(ql, N, B));
        Vec b = c[0], sp = s, tmp(N);
        for (uint32_t e = 1; e < nElem; ++e)
            for (uint32_t i = 0; i < n; ++i) {
                if (e > 1)
                    orc_vec_mul(&sp[(size_t)i * N], &sp[(size_t)i * N], &s[(size_t)i * N], N, q[i]);
                for (uint32_t bb = 0; bb < B; ++bb) {
                    const size_t off = ((size_t)bb * n + i) * N;
                    orc_vec_mul(tmp.data(), &c[e][off], &sp[(size_t)i * N], N, q[i]);
                    orc_vec_add(&b[off], &b[off], tmp.data(), N, q[i]);
                }
            }
        orc_ntt_inv_tower(octx, b.data(), nullptr, n, B, 0);
        std::vector<DCRTPolyHip> dev;
        for (uint32_t e = 0; e < nElem; ++e)
            dev.push_back(upload(params, c[e], n, B, EVALUATION));
        std::vector<const DCRTPolyHip*> elems;
        for (auto& d : dev)
            elems.push_back(&d);
        auto S = upload(params, s, n, 1, EVALUATION);
        REQUIRE(DCRTPolyHip::BgvDecrypt(elems, S, t) == modT(loop(b, n, n - 1)), 104 + (int)nElem);
        REQUIRE(dev[0].GetValues() == c[0] && dev[1].GetValues() == c[1], 106 + (int)nElem);  // (the operands are left as they were)
    }
    orc_ctx_destroy(octx);
    std::printf("hal_bgv_decrypt OK\n");
    return 0;
}
