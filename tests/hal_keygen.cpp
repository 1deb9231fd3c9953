// TEST: evaluation-key generation through the C++ host mirror (openfhe-development_amd/hal/dcrtpoly_hip.h: KeySwitchSecretExtend,
// KeyGenHybrid, KeyGenHybridBlake2, HybridKeySet) against the oracle (oracle/fhe_oracle.h).  Expected words of the explicit form:
// orc_automorph_eval_k, orc_vec_mul / _neg / _mul_const / _add on every limb of every digit; of the extension: orc_ntt_inv_tower,
// orc_switch_modulus, orc_ntt_fwd_tower.  The seeded form must equal the explicit form fed with the two blake2 samplers and a forward
// transform, and a key of the set must switch keys like the same words uploaded by hand (orc_hybrid_key_switch).  Linked against the
// TEST-ONLY emulator build on CPU or the HIP library on a GPU box.
#include <cstdio>
#include <random>

#include "../openfhe-development_amd/hal/dcrtpoly_hip.h"
#include "../oracle/fhe_oracle.h"

using namespace fhehip;
typedef std::vector<uint64_t> Vec;

static std::mt19937_64 gen(20261020);
static Vec randTower(const Vec& mods, uint32_t N, uint32_t lead) {
    Vec v((size_t)lead * mods.size() * N);
    for (uint32_t t = 0; t < lead; ++t)
        for (size_t l = 0; l < mods.size(); ++l)
            for (uint32_t i = 0; i < N; ++i)
                v[((size_t)t * mods.size() + l) * N + i] = gen() % mods[l];
    return v;
}
static DCRTPolyHip upload(const std::shared_ptr<Params>& p, const Vec& v, uint32_t limbs, uint32_t batch, Format f = EVALUATION) {
    DCRTPolyHip x(p, limbs, f, batch);
    x.SetValues(v, f);
    return x;
}
#define REQUIRE(cond, code)                                             \
    if (!(cond)) {                                                      \
        std::printf("hal_keygen: check %d failed (%s)\n", code, #cond); \
        return code;                                                    \
    }

int main() {
    const uint32_t logN = 6, N = 1u << logN, numQ = 3, dnum = 2, alpha = 2, K = 3;
    const uint64_t t = 65537;
    Vec q(numQ), psiQ(numQ), p(64), psiP(64);
    q[0] = fhe_param_last_prime(60, 2 * N);
    for (uint32_t i = 1; i < numQ; ++i)
        q[i] = fhe_param_previous_prime(q[i - 1], 2 * N);
    for (uint32_t i = 0; i < numQ; ++i)
        psiQ[i] = fhe_param_root_of_unity(2 * N, q[i]);
    const uint32_t sizeP = fhe_param_select_p(logN, numQ, q.data(), dnum, 60, p.data(), psiP.data());
    REQUIRE(sizeP > 0, 100);
    p.resize(sizeP), psiP.resize(sizeP);
    Vec qp = q, psi = psiQ;
    qp.insert(qp.end(), p.begin(), p.end()), psi.insert(psi.end(), psiP.begin(), psiP.end());
    const uint32_t QP = numQ + sizeP;
    auto params = std::make_shared<Params>(2 * N, qp, psi);
    KeySwitchHybrid ks(params, numQ, sizeP, dnum);
    orc_ctx* octx = orc_ctx_create(N, QP, qp.data(), psi.data());

    // ---- the secret's extension ----
    Vec sCoef((size_t)numQ * N);  // a ternary secret
    for (uint32_t i = 0; i < N; ++i) {
        const int v = (int)(gen() % 3) - 1;
        for (uint32_t l = 0; l < numQ; ++l)
            sCoef[(size_t)l * N + i] = v < 0 ? q[l] - 1 : (uint64_t)v;
    }
    Vec s = sCoef;
    orc_ntt_fwd_tower(octx, s.data(), nullptr, numQ, 1, 1);
    Vec sExt((size_t)QP * N);
    std::copy(s.begin(), s.end(), sExt.begin());
    for (uint32_t j = 0; j < sizeP; ++j) {
        uint64_t* row = &sExt[(size_t)(numQ + j) * N];
        std::copy(sCoef.begin(), sCoef.begin() + N, row);
        orc_switch_modulus(row, N, q[0], p[j]);
        const uint32_t limb = numQ + j;
        orc_ntt_fwd_tower(octx, row, &limb, 1, 1, 1);
    }
    DCRTPolyHip dS      = upload(params, s, numQ, 1);
    DCRTPolyHip dSExt   = KeySwitchSecretExtend(ks, dS, sizeP);
    REQUIRE(dSExt.GetValues() == sExt, 1);
    REQUIRE(dS.GetValues() == s, 2);

    // ---- the explicit form: K keys with different automorphism indices, the BGV noise scale ----
    const std::vector<uint32_t> kNew = {5, 1, 2 * N - 1}, kOld = {1, 25, 5};
    Vec factor((size_t)dnum * QP, 0);
    for (uint32_t j = 0; j < dnum; ++j)
        for (uint32_t i = alpha * j; i < std::min(alpha * (j + 1), numQ); ++i) {
            uint64_t P = 1;
            for (uint64_t pj : p)
                P = orc_mulmod(P, pj % q[i], q[i]);
            factor[(size_t)j * QP + i] = P;
        }
    const Vec sOld = randTower(q, N, 1), a = randTower(qp, N, K * dnum), e = randTower(qp, N, K * dnum);
    Vec want(a.size()), sn(N), so(N), x(N), y(N);
    for (uint32_t k = 0; k < K; ++k)
        for (uint32_t i = 0; i < QP; ++i) {
            orc_automorph_eval_k(sn.data(), &sExt[(size_t)i * N], N, kNew[k]);
            if (i < numQ)
                orc_automorph_eval_k(so.data(), &sOld[(size_t)i * N], N, kOld[k]);
            for (uint32_t j = 0; j < dnum; ++j) {
                const size_t at = (((size_t)k * dnum + j) * QP + i) * N;
                orc_vec_mul(x.data(), &a[at], sn.data(), N, qp[i]);
                orc_vec_neg(x.data(), x.data(), N, qp[i]);
                orc_vec_mul_const(y.data(), &e[at], t % qp[i], N, qp[i]);
                orc_vec_add(x.data(), x.data(), y.data(), N, qp[i]);
                if (factor[(size_t)j * QP + i]) {
                    orc_vec_mul_const(y.data(), so.data(), factor[(size_t)j * QP + i], N, qp[i]);
                    orc_vec_add(x.data(), x.data(), y.data(), N, qp[i]);
                }
                std::copy(x.begin(), x.end(), want.begin() + at);
            }
        }
    DCRTPolyHip dSOld = upload(params, sOld, numQ, 1);
    auto set          = KeyGenHybrid(ks, dSExt, dSOld, kNew, kOld, t, upload(params, a, QP, K * dnum), upload(params, e, QP, K * dnum));
    REQUIRE(set->keys.size() == K, 10);
    REQUIRE(set->b.GetValues() == want, 11);
    REQUIRE(set->a.GetValues() == a, 12);

    // ---- a handle of the set is the key of its window: KeySwitchCore with key 1 against the oracle on the same words ----
    {
        orc_hybrid* hy = orc_hybrid_create(N, numQ, q.data(), psiQ.data(), sizeP, p.data(), psiP.data(), dnum);
        const Vec c    = randTower(q, N, 1);
        const size_t kw = (size_t)dnum * QP * N;
        Vec w0((size_t)numQ * N), w1((size_t)numQ * N);
        orc_hybrid_key_switch(hy, c.data(), numQ, &want[kw], &a[kw], w0.data(), w1.data());
        orc_hybrid_destroy(hy);
        DCRTPolyHip dC = upload(params, c, numQ, 1), o0(params, numQ, EVALUATION), o1(params, numQ, EVALUATION);
        const size_t wsb = fhe_ks_workspace_bytes(ks.plan(), numQ, 1);
        void* ws         = nullptr;
        check(fhe_malloc(params->ctx(), wsb, &ws));
        check(fhe_keyswitch_hybrid(ks.plan(), set->keys[1], dC.data(), numQ, 1, o0.data(), o1.data(), ws, wsb, nullptr));
        REQUIRE(o0.GetValues() == w0 && o1.GetValues() == w1, 20);
        fhe_free(params->ctx(), ws);
    }

    // ---- the seeded form is its composition ----
    uint32_t key[16];
    for (uint32_t i = 0; i < 16; ++i)
        key[i] = 0x9e3779b9u * (i + 1);
    const double sigma = 3.19;
    uint64_t nA = 0, nE = 0;
    check(fhe_ks_keygen_counters(ks.plan(), K, &nA, &nE));
    REQUIRE(nA == ((uint64_t)2 * K * dnum * QP * N + 511) / 512 && nE == ((uint64_t)K * dnum * N + 511) / 512, 30);
    const uint64_t cA = 11, cE = cA + nA;
    uint64_t nextA = 0, nextE = 0;
    auto seeded = KeyGenHybridBlake2(ks, dnum, dSExt, dSOld, kNew, kOld, t, sigma, key, cA, cE, &nextA, &nextE);
    REQUIRE(nextA == cA + nA && nextE == cE + nE, 31);
    DCRTPolyHip da(params, QP, EVALUATION, K * dnum), de(params, QP, COEFFICIENT, K * dnum);
    check(fhe_sample_uniform_blake2(params->ctx(), da.data(), nullptr, QP, K * dnum, key, cA, nullptr));
    check(fhe_sample_gaussian_blake2(params->ctx(), de.data(), nullptr, QP, K * dnum, sigma, key, cE, nullptr));
    de.SwitchFormat();
    auto byHand = KeyGenHybrid(ks, dSExt, dSOld, kNew, kOld, t, std::move(da), std::move(de));
    REQUIRE(seeded->a.GetValues() == byHand->a.GetValues(), 32);
    REQUIRE(seeded->b.GetValues() == byHand->b.GetValues(), 33);

    // ---- errors surface as exceptions with the library's text ----
    bool threw = false;
    try {
        KeyGenHybridBlake2(ks, dnum, dSExt, dSOld, {2}, {1}, t, sigma, key, 0, 0);
    } catch (const Error& err) {
        threw = std::string(err.what()).find("Automorphism index not odd") != std::string::npos;
    }
    REQUIRE(threw, 40);
    orc_ctx_destroy(octx);
    std::printf("hal_keygen OK\n");
    return 0;
}
