// TEST INFRASTRUCTURE — generator of tests/golden/ref_vectors_ckks_composite.npz (run by make_golden_ckks_composite.py).
// Links the reference's stock libraries (oracle/_ref), the way gen_bgv_hybrid.cpp does.  CKKS under COMPOSITESCALINGMANUAL, where every
// rescale drops compositeDegree limbs (LeveledSHECKKSRNS::ModReduceInternalInPlace(ct, compositeDegree), ckksrns-leveledshe.cpp:172-191).
// Chosen values (accepted by the reference's validation at the smallest ring tried): ring dimension 64, HEStd_NotSet, multiplicative depth 2,
// HYBRID key switching, register word size 32; composite degree 2 with firstModSize 60 / scalingModSize 50, composite degree 3 with
// firstModSize 72 / scalingModSize 66 (the validation wants scalingModSize >= 60 above degree 2, and firstModSize above it).
// Outside FIXEDMANUAL the public cc->Rescale is a no-op (LeveledSHERNS::ModReduceInPlace, rns-leveledshe.cpp:317-321: the rescale happens
// by itself before the next multiplication, :148-155); the generator CHECKS that and records the call the reference makes there,
// scheme->ModReduceInternal(ct, compositeDegree), on the product of two fresh ciphertexts.
// Per case <d> = 2, 3:
//   q_d<d>, psi_d<d>           moduli and roots of Q
//   x_d<d>                     both elements of cc->EvalMult(a, b) before the rescale:   [2][sizeQl][ring]
//   y_d<d>                     both elements after it:                                    [2][sizeQl - d][ring]
//   tabA_d<d>, tabB_d<d>       GetQlQlInvModqlDivqlModq(diffQl + i) / GetqlInvModq(diffQl + i), i = 0 .. d-1, one after the other
//   meta_d<d>                  ring, composite degree, sizeQ, sizeQl before, sizeQl after
// The generator FAILS unless the call dropped exactly compositeDegree limbs.
// Record format: u32 name length, name, u32 type (0 = u64), u64 count, data.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "openfhe.h"

using namespace lbcrypto;

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
static bool shaped(const Ciphertext<DCRTPoly>& c, size_t limbs) {
    if (c->GetElements().size() != 2)
        return false;
    for (const auto& e : c->GetElements())
        if (e.GetFormat() != Format::EVALUATION || e.GetNumOfElements() != limbs)
            return false;
    return true;
}
#define REQUIRE(cond)                                                          \
    do {                                                                       \
        if (!(cond)) {                                                         \
            fprintf(stderr, "gen_ckks_composite: %s does not hold\n", #cond); \
            return 1;                                                          \
        }                                                                      \
    } while (0)

static int one_case(uint32_t degree, uint32_t firstMod, uint32_t scaleMod) {
    const uint32_t ring = 64;
    const std::string sfx = "_d" + std::to_string(degree);
    CCParams<CryptoContextCKKSRNS> parameters;
    parameters.SetSecurityLevel(HEStd_NotSet);
    parameters.SetRingDim(ring);
    parameters.SetMultiplicativeDepth(2);
    parameters.SetFirstModSize(firstMod);
    parameters.SetScalingModSize(scaleMod);
    parameters.SetScalingTechnique(COMPOSITESCALINGMANUAL);
    parameters.SetRegisterWordSize(32);
    parameters.SetCompositeDegree(degree);
    parameters.SetKeySwitchTechnique(HYBRID);
    auto cc = GenCryptoContext(parameters);
    cc->Enable(PKE);
    cc->Enable(KEYSWITCH);
    cc->Enable(LEVELEDSHE);
    auto kp = cc->KeyGen();
    cc->EvalMultKeyGen(kp.secretKey);
    const auto cp = std::dynamic_pointer_cast<CryptoParametersCKKSRNS>(cc->GetCryptoParameters());
    REQUIRE(cp->GetScalingTechnique() == COMPOSITESCALINGMANUAL && cp->GetCompositeDegree() == degree);
    const uint32_t sizeQ = cp->GetElementParams()->GetParams().size();
    std::vector<double> v1(ring / 2), v2(ring / 2);
    for (uint32_t i = 0; i < ring / 2; ++i)
        v1[i] = 0.25 * (i % 7) - 0.5, v2[i] = 1.0 - 0.125 * (i % 5);
    auto a = cc->Encrypt(kp.publicKey, cc->MakeCKKSPackedPlaintext(v1));
    auto b = cc->Encrypt(kp.publicKey, cc->MakeCKKSPackedPlaintext(v2));
    auto m = cc->EvalMult(a, b);
    const uint32_t sizeQl = m->GetElements()[0].GetNumOfElements();
    REQUIRE(shaped(m, sizeQl) && sizeQl > degree && m->GetNoiseScaleDeg() == 2);
    REQUIRE(shaped(cc->Rescale(m), sizeQl));  // the public call leaves the ciphertext alone outside FIXEDMANUAL
    auto r = cc->GetScheme()->ModReduceInternal(m, degree);
    REQUIRE(shaped(r, sizeQl - degree));  // exactly compositeDegree limbs
    std::vector<uint64_t> qs, roots, tabA, tabB;
    for (const auto& l : cp->GetElementParams()->GetParams()) {
        qs.push_back(l->GetModulus().ConvertToInt<uint64_t>());
        roots.push_back(l->GetRootOfUnity().ConvertToInt<uint64_t>());
    }
    const uint32_t diffQl = sizeQ - sizeQl;
    for (uint32_t i = 0; i < degree; ++i) {
        const auto& A = cp->GetQlQlInvModqlDivqlModq(diffQl + i);
        const auto& B = cp->GetqlInvModq(diffQl + i);
        REQUIRE(A.size() >= sizeQl - 1 - i && B.size() >= sizeQl - 1 - i);
        for (uint32_t k = 0; k < sizeQl - 1 - i; ++k)
            tabA.push_back(A[k].ConvertToInt<uint64_t>()), tabB.push_back(B[k].ConvertToInt<uint64_t>());
    }
    put_u64("q" + sfx, qs), put_u64("psi" + sfx, roots);
    put_u64("x" + sfx, words(m->GetElements())), put_u64("y" + sfx, words(r->GetElements()));
    put_u64("tabA" + sfx, tabA), put_u64("tabB" + sfx, tabB);
    put_u64("meta" + sfx, {ring, degree, sizeQ, sizeQl, sizeQl - degree});
    printf("CKKS COMPOSITESCALINGMANUAL: degree %u, sizeQ = %u, sizeQl %u -> %u\n", degree, sizeQ, sizeQl, sizeQl - degree);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2)
        return 2;
    g_out = fopen(argv[1], "wb");
    if (!g_out)
        return 1;
    if (int rc = one_case(2, 60, 50))
        return rc;
    if (int rc = one_case(3, 72, 66))
        return rc;
    fclose(g_out);
    return 0;
}
