// TEST INFRASTRUCTURE — generator of tests/golden/ref_vectors_bgv.npz (run by make_golden_bgv.py).
// Links the reference's stock libraries (oracle/_ref), the way gen_bfv_rotate_bv.cpp does.  BGV on HYBRID keys through the reference's
// scheme layer: ring dimension 64, t = 65537, multiplicative depth 3, FIXEDMANUAL, HYBRID key switching with 2 digits, HEStd_NotSet.
//   q, psiQ, p, psiP           moduli and roots of Q and of the auxiliary basis P
//   mulB, mulA, rotB, rotA     the relinearisation key and the automorphism key of the rotation index 1: [dnum][numQ + numP][ring]
//   a, b                       two fresh ciphertexts
//   m                          cc->EvalMult(a, b)              (KeySwitchCore with ApproxModDown's t > 0)
//   r                          cc->ModReduce(m)                (DCRTPoly::ModReduce on both elements)
//   rot                        cc->EvalRotate(a, 1); EvalFastRotationPrecompute / EvalFastRotation is CHECKED here to give the same words
//   rotL, mL                   cc->EvalRotate(r, 1) and cc->EvalMult(r, r): the same composites one level down
//   meta                       ring, t, numQ, numP, dnum, automorphism index, sizeQl of m, sizeQl of r
// The generator FAILS unless the product sits at the full level and ModReduce drops exactly one limb.
// Record format: u32 name length, name, u32 type (0 = u64), u64 count, data.
#include <cstdint>
#include <cstdio>
#include <random>
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
static void put_polys(const std::string& name, const std::vector<DCRTPoly>& v) { put_u64(name, words(v)); }
static void put_params(const std::string& q, const std::string& psi, const std::shared_ptr<DCRTPoly::Params>& p) {
    std::vector<uint64_t> qs, roots;
    for (const auto& l : p->GetParams()) {
        qs.push_back(l->GetModulus().ConvertToInt<uint64_t>());
        roots.push_back(l->GetRootOfUnity().ConvertToInt<uint64_t>());
    }
    put_u64(q, qs), put_u64(psi, roots);
}
static bool shaped(const Ciphertext<DCRTPoly>& c, size_t limbs) {
    if (c->GetElements().size() != 2)
        return false;
    for (const auto& e : c->GetElements())
        if (e.GetFormat() != Format::EVALUATION || e.GetNumOfElements() != limbs)
            return false;
    return true;
}
#define REQUIRE(cond)                                                      \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "gen_bgv_hybrid: %s does not hold\n", #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

int main(int argc, char** argv) {
    if (argc < 2)
        return 2;
    g_out = fopen(argv[1], "wb");
    if (!g_out)
        return 1;
    const uint32_t ring = 64, dnum = 2;
    const uint64_t t    = 65537;
    const int32_t index = 1;
    CCParams<CryptoContextBGVRNS> parameters;
    parameters.SetSecurityLevel(HEStd_NotSet);
    parameters.SetRingDim(ring);
    parameters.SetPlaintextModulus(t);
    parameters.SetMultiplicativeDepth(3);
    parameters.SetScalingTechnique(FIXEDMANUAL);
    parameters.SetKeySwitchTechnique(HYBRID);
    parameters.SetNumLargeDigits(dnum);
    auto cc = GenCryptoContext(parameters);
    cc->Enable(PKE);
    cc->Enable(KEYSWITCH);
    cc->Enable(LEVELEDSHE);
    auto kp = cc->KeyGen();
    cc->EvalMultKeyGen(kp.secretKey);
    cc->EvalRotateKeyGen(kp.secretKey, {index});
    std::mt19937_64 gen(47);
    auto fresh = [&]() {
        std::vector<int64_t> v(ring);
        for (auto& e : v)
            e = static_cast<int64_t>(gen() % 5) - 2;
        return cc->Encrypt(kp.publicKey, cc->MakePackedPlaintext(v));
    };
    const auto cp       = std::dynamic_pointer_cast<CryptoParametersBGVRNS>(cc->GetCryptoParameters());
    const uint32_t numQ = cp->GetElementParams()->GetParams().size(), numP = cp->GetParamsP()->GetParams().size();
    REQUIRE(cp->GetScalingTechnique() == FIXEDMANUAL && cp->GetKeySwitchTechnique() == HYBRID && cp->GetNumPartQ() == dnum && numQ >= 3);
    REQUIRE(cp->GetPlaintextModulus() == t);
    auto a = fresh(), b = fresh();
    REQUIRE(shaped(a, numQ) && shaped(b, numQ));

    const auto mulKey = cc->GetEvalMultKeyVector(a->GetKeyTag())[0];
    const uint32_t k  = cc->FindAutomorphismIndex(index);
    const auto rotKey = cc->GetEvalAutomorphismKeyMap(a->GetKeyTag()).at(k);
    for (const auto& key : {mulKey, rotKey})
        REQUIRE(key->GetBVector().size() == dnum && key->GetBVector()[0].GetNumOfElements() == numQ + numP &&
                key->GetBVector()[0].GetFormat() == Format::EVALUATION);
    put_params("q", "psiQ", cp->GetElementParams());
    put_params("p", "psiP", cp->GetParamsP());
    put_polys("mulB", mulKey->GetBVector()), put_polys("mulA", mulKey->GetAVector());
    put_polys("rotB", rotKey->GetBVector()), put_polys("rotA", rotKey->GetAVector());
    put_polys("a", a->GetElements()), put_polys("b", b->GetElements());

    auto m = cc->EvalMult(a, b);
    REQUIRE(shaped(m, numQ));  // FIXEDMANUAL: the product sits at the full level
    auto r = cc->ModReduce(m);
    REQUIRE(shaped(r, numQ - 1));  // ... and ModReduce drops exactly one limb
    put_polys("m", m->GetElements()), put_polys("r", r->GetElements());

    auto rot          = cc->EvalRotate(a, index);
    const auto digits = cc->EvalFastRotationPrecompute(a);
    const auto fast   = cc->EvalFastRotation(a, index, 2 * ring, digits);
    REQUIRE(shaped(rot, numQ) && words(rot->GetElements()) == words(fast->GetElements()));
    put_polys("rot", rot->GetElements());

    auto rotL = cc->EvalRotate(r, index);
    auto mL   = cc->EvalMult(r, r);
    REQUIRE(shaped(rotL, numQ - 1) && shaped(mL, numQ - 1));
    put_polys("rotL", rotL->GetElements()), put_polys("mL", mL->GetElements());

    put_u64("meta", {ring, t, numQ, numP, dnum, k, numQ, numQ - 1});
    printf("BGV FIXEDMANUAL + HYBRID: numQ = %u, numP = %u, dnum = %u, automorphism index %u\n", numQ, numP, dnum, k);
    fclose(g_out);
    return 0;
}
