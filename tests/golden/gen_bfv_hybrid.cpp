// TEST INFRASTRUCTURE — generator of tests/golden/ref_vectors_bfv_hybrid.npz (run by make_golden_bfv_hybrid.py).
// Links the reference's stock libraries (oracle/_ref), the way gen_bfv_rotate_bv.cpp does.  Rotations and leveled relinearisation of BFV
// ciphertexts on HYBRID keys through the reference's scheme layer: ring dimension 64, t = 65537, limbs of 60 bits, the default
// multiplication technique (HPSPOVERQLEVELED), numLargeDigits 2 (4 limbs: the dropped level has a partial last digit) and 3 (3 limbs:
// alpha = 1).  Per case, prefix bfvh<dnum>_:
//   q, psiQ, p_q, p_psiQ, r_q, r_psiQ   moduli and roots of Q, P and R
//   a, b                       two fresh ciphertexts
//   rotB<j>, rotA<j>           the automorphism keys of the rotation indices 1 and 2 (j = 0, 1), mulB / mulA the relinearisation key, each
//                              [numPartQ][sizeQ + sizeP][N]
//   dig, rot<j>                EvalFastRotationPrecompute(a)'s digits [numPartQl][sizeQl + sizeP][N] and cc->EvalRotate(a, index_j);
//                              EvalFastRotation on the digits is CHECKED here to give the same words
//   digL, rotL<j>              the same for a with its noiseScaleDeg raised until the reference drops a level for the key switch
//   d, m                       cc->EvalMultNoRelin and cc->EvalMult of a, b with their noiseScaleDeg raised until both the product and
//                              its relinearisation run below numQ
//   meta                       ring, t, numQ, sizeP, numPartQ, autoIndex_0, autoIndex_1, sizeQl of the fresh rotation (= numQ), noiseScaleDeg
//                              and sizeQl of the dropped rotation, noiseScaleDeg of the product's operands, sizeQl of the product, sizeQl
//                              of its relinearisation
// The levels are what FindLevelsToDrop answers here (with HYBRID's noiseKS they differ from the BV file's); the generator FAILS unless the
// dropped cases drop and the fresh ones do not, and unless the digit shapes are the ones named above.
// Record format: u32 name length, name, u32 type (0 = u64), u64 count, data.
#include <cstdint>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "openfhe.h"

using namespace lbcrypto;

namespace lbcrypto {
uint32_t FindLevelsToDrop(uint32_t multiplicativeDepth, std::shared_ptr<CryptoParametersBase<DCRTPoly>> cryptoParams, uint32_t dcrtBits,
                          bool keySwitch);
}

static FILE* g_out;
static void put_u64(const std::string& name, const std::vector<uint64_t>& v) {
    const uint32_t n = name.size(), type = 0;
    const uint64_t count = v.size();
    fwrite(&n, 4, 1, g_out);
    fwrite(name.data(), 1, n, g_out);
    fwrite(&type, 4, 1, g_out);
    fwrite(&count, 8, 1, g_out);
    fwrite(v.data(), 8, count, g_out);
}
static std::vector<uint64_t> words(const std::vector<DCRTPoly>& v) {
    std::vector<uint64_t> o;
    for (const auto& e : v)
        for (size_t i = 0; i < e.GetNumOfElements(); ++i)
            for (size_t k = 0; k < e.GetRingDimension(); ++k)
                o.push_back(e.GetElementAtIndex(i)[k].ConvertToInt<uint64_t>());
    return o;
}
static void put_polys(const std::string& name, const std::vector<DCRTPoly>& v) { put_u64(name, words(v)); }
static void put_params(const std::string& pre, const std::shared_ptr<DCRTPoly::Params>& p) {
    std::vector<uint64_t> q, psi;
    for (const auto& l : p->GetParams()) {
        q.push_back(l->GetModulus().ConvertToInt<uint64_t>());
        psi.push_back(l->GetRootOfUnity().ConvertToInt<uint64_t>());
    }
    put_u64(pre + "q", q), put_u64(pre + "psiQ", psi);
}
static bool all_format(const std::vector<DCRTPoly>& v, Format f) {
    for (const auto& e : v)
        if (e.GetFormat() != f)
            return false;
    return true;
}
#define REQUIRE(cond)                                                      \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "gen_bfv_hybrid: %s does not hold\n", #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

// wantPartial: the dropped rotation's level must leave a partial last digit; otherwise alpha must be 1
static int bfv_case(uint32_t dnum, uint32_t depth, bool wantPartial) {
    const uint32_t ring = 64;
    const uint64_t t    = 65537;
    const std::string pre = "bfvh" + std::to_string(dnum) + "_";
    const std::vector<int32_t> indices = {1, 2};
    CCParams<CryptoContextBFVRNS> parameters;
    parameters.SetSecurityLevel(HEStd_NotSet);
    parameters.SetRingDim(ring);
    parameters.SetPlaintextModulus(t);
    parameters.SetMultiplicativeDepth(depth);
    parameters.SetScalingModSize(60);
    parameters.SetKeySwitchTechnique(HYBRID);
    parameters.SetNumLargeDigits(dnum);
    auto cc = GenCryptoContext(parameters);
    cc->Enable(PKE);
    cc->Enable(KEYSWITCH);
    cc->Enable(LEVELEDSHE);
    auto kp = cc->KeyGen();
    cc->EvalMultKeyGen(kp.secretKey);
    cc->EvalRotateKeyGen(kp.secretKey, indices);
    std::mt19937_64 gen(53 + dnum);
    auto fresh = [&]() {
        std::vector<int64_t> v(ring);
        for (auto& e : v)
            e = static_cast<int64_t>(gen() % 5) - 2;
        return cc->Encrypt(kp.publicKey, cc->MakePackedPlaintext(v));
    };
    const auto cp        = std::dynamic_pointer_cast<CryptoParametersBFVRNS>(cc->GetCryptoParameters());
    const uint32_t numQ  = cp->GetElementParams()->GetParams().size();
    const uint32_t sizeP = cp->GetParamsP()->GetParams().size();
    const uint32_t alpha = cp->GetNumPerPartQ();
    REQUIRE(cp->GetMultiplicationTechnique() == HPSPOVERQLEVELED && cp->GetKeySwitchTechnique() == HYBRID && numQ >= 3);
    REQUIRE(cp->GetNumPartQ() == dnum);
    auto a = fresh(), b = fresh();
    REQUIRE(all_format(a->GetElements(), Format::EVALUATION) && all_format(b->GetElements(), Format::EVALUATION));
    const uint32_t dcrtBits = a->GetElements()[0].GetElementAtIndex(0).GetModulus().GetMSB();
    auto drop = [&](uint32_t noiseScaleDeg, bool keySwitch) {
        return FindLevelsToDrop(noiseScaleDeg - 1, cc->GetCryptoParameters(), dcrtBits, keySwitch);
    };
    auto raised = [&](const Ciphertext<DCRTPoly>& c, uint32_t deg) {
        auto o = c->Clone();
        o->SetNoiseScaleDeg(deg);
        return o;
    };
    // keys
    const auto mulKey  = cc->GetEvalMultKeyVector(a->GetKeyTag())[0];
    const auto& rotMap = cc->GetEvalAutomorphismKeyMap(a->GetKeyTag());
    REQUIRE(mulKey->GetBVector().size() == dnum && mulKey->GetBVector()[0].GetNumOfElements() == numQ + sizeP);
    std::vector<uint64_t> autoIdx;
    for (size_t j = 0; j < indices.size(); ++j) {
        const uint32_t k = cc->FindAutomorphismIndex(indices[j]);
        const auto key   = rotMap.at(k);
        REQUIRE(all_format(key->GetBVector(), Format::EVALUATION) && key->GetBVector()[0].GetNumOfElements() == numQ + sizeP &&
                key->GetBVector().size() == dnum);
        autoIdx.push_back(k);
        put_polys(pre + "rotB" + std::to_string(j), key->GetBVector()), put_polys(pre + "rotA" + std::to_string(j), key->GetAVector());
    }
    put_polys(pre + "mulB", mulKey->GetBVector()), put_polys(pre + "mulA", mulKey->GetAVector());
    put_params(pre, cp->GetElementParams());
    put_params(pre + "p_", cp->GetParamsP());
    put_params(pre + "r_", cp->GetParamsRl(numQ - 1));
    put_polys(pre + "a", a->GetElements()), put_polys(pre + "b", b->GetElements());

    // rotations: fresh (nothing dropped) and with the noiseScaleDeg raised until the key switch drops a level
    REQUIRE(a->GetNoiseScaleDeg() == 1 && drop(1, true) == 0);
    uint32_t degRot = 2;
    while (degRot < 64 && drop(degRot, true) == 0)
        ++degRot;
    const uint32_t dropRot = drop(degRot, true);
    REQUIRE(dropRot >= 1 && dropRot < numQ);
    printf("BFV HYBRID dnum = %u, depth %u: numQ = %u, alpha = %u, the key switch drops %u at noiseScaleDeg %u\n", dnum, depth, numQ, alpha,
           dropRot, degRot);
    if (wantPartial)
        REQUIRE(alpha >= 2 && (numQ - dropRot) % alpha != 0);
    else
        REQUIRE(alpha == 1);
    const struct {
        Ciphertext<DCRTPoly> ct;
        uint32_t sizeQl;
        const char* tag;
    } rots[2] = {{a, numQ, ""}, {raised(a, degRot), numQ - dropRot, "L"}};
    for (const auto& c : rots) {
        const auto digits = cc->EvalFastRotationPrecompute(c.ct);
        REQUIRE(all_format(*digits, Format::EVALUATION) && (*digits)[0].GetNumOfElements() == c.sizeQl + sizeP);
        REQUIRE(digits->size() == std::min<size_t>((c.sizeQl + alpha - 1) / alpha, dnum));
        put_polys(pre + "dig" + c.tag, *digits);
        for (size_t j = 0; j < indices.size(); ++j) {
            const auto rot  = cc->EvalRotate(c.ct, indices[j]);
            const auto fast = cc->EvalFastRotation(c.ct, indices[j], 2 * ring, digits);
            REQUIRE(rot->GetElements().size() == 2 && all_format(rot->GetElements(), Format::EVALUATION) &&
                    rot->GetElements()[0].GetNumOfElements() == numQ);
            REQUIRE(words(rot->GetElements()) == words(fast->GetElements()));
            put_polys(pre + "rot" + c.tag + std::to_string(j), rot->GetElements());
        }
    }

    // EvalMult with both the product and its relinearisation at a dropped level
    REQUIRE(drop(1, false) == 0);
    uint32_t degMul = 2;
    while (degMul < 64 && drop(degMul, false) == 0)
        ++degMul;
    auto a2 = raised(a, degMul), b2 = raised(b, degMul);
    const uint32_t dropMul = drop(degMul, false);
    auto d                 = cc->EvalMultNoRelin(a2, b2);
    const uint32_t dropRel = drop(d->GetNoiseScaleDeg(), false);  // (RelinearizeCore on three elements: isKeySwitch is false, :894)
    REQUIRE(dropMul >= 1 && dropMul < numQ && dropRel >= 1 && dropRel < numQ);
    REQUIRE(d->GetElements().size() == 3 && all_format(d->GetElements(), Format::COEFFICIENT));
    auto m = cc->EvalMult(a2, b2);
    REQUIRE(m->GetElements().size() == 2 && all_format(m->GetElements(), Format::EVALUATION));
    put_polys(pre + "d", d->GetElements()), put_polys(pre + "m", m->GetElements());

    put_u64(pre + "meta", {ring, t, numQ, sizeP, dnum, autoIdx[0], autoIdx[1], numQ, degRot, numQ - dropRot, degMul, numQ - dropMul,
                           numQ - dropRel});
    printf("BFV HYBRID dnum = %u: numQ = %u, sizeP = %u, alpha = %u, automorphism indices %u %u; rotation drops %u at noiseScaleDeg %u; "
           "product drops %u at noiseScaleDeg %u, its relinearisation %u at %zu\n",
           dnum, numQ, sizeP, alpha, (unsigned)autoIdx[0], (unsigned)autoIdx[1], dropRot, degRot, dropMul, degMul, dropRel,
           (size_t)d->GetNoiseScaleDeg());
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2)
        return 2;
    g_out = fopen(argv[1], "wb");
    if (!g_out)
        return 1;
    int rc = 0;
    rc |= bfv_case(2, 8, true);
    rc |= bfv_case(3, 4, false);
    fclose(g_out);
    return rc;
}
