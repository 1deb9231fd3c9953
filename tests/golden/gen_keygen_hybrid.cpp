// TEST INFRASTRUCTURE — generator of tests/golden/ref_vectors_keygen.npz (run by make_golden_keygen.py).
// Links the reference's stock libraries (oracle/_ref), the way gen_bgv_hybrid.cpp does.  The keys the reference's own KeyGen,
// EvalMultKeyGen and EvalRotateKeyGen make on HYBRID key switching, ring dimension 64, HEStd_NotSet, for two parameter sets:
//   ckks_*   CKKS, FIXEDMANUAL, depth 2 (3 limbs of Q), 2 digits: the last digit is shorter than the first
//   bgv_*    BGV, FIXEDMANUAL, t = 65537, depth 3, 2 digits
// Per set (prefix omitted):
//   q, psiQ, p, psiP           moduli and roots of Q and of the auxiliary basis P
//   s                          the secret key [numQ][ring], EVALUATION
//   pkB, pkA                   the public key's two elements [numQ][ring]
//   mulB, mulA                 the EvalMultKeyGen key [dnum][numQ + numP][ring]
//   rotPB, rotPA, rotMB, rotMA the EvalRotateKeyGen keys of the index +1 and of the index -1
//   meta                       ring, noise scale, numQ, numP, dnum, limbs per digit, automorphism index of +1, of -1, 100 * sigma
// The generator FAILS unless the shapes are what the meta block says.
// Record format: u32 name length, name, u32 type (0 = u64), u64 count, data.
#include <cmath>
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
static void put_polys(const std::string& name, const std::vector<DCRTPoly>& v) {
    std::vector<uint64_t> o;
    for (const auto& e : v)
        for (size_t i = 0; i < e.GetNumOfElements(); ++i)
            for (size_t k = 0; k < e.GetRingDimension(); ++k)
                o.push_back(e.GetElementAtIndex(i)[k].ConvertToInt<uint64_t>());
    put_u64(name, o);
}
static void put_params(const std::string& q, const std::string& psi, const std::shared_ptr<DCRTPoly::Params>& p) {
    std::vector<uint64_t> qs, roots;
    for (const auto& l : p->GetParams()) {
        qs.push_back(l->GetModulus().ConvertToInt<uint64_t>());
        roots.push_back(l->GetRootOfUnity().ConvertToInt<uint64_t>());
    }
    put_u64(q, qs), put_u64(psi, roots);
}
static bool shaped(const DCRTPoly& e, size_t limbs, uint32_t ring) {
    return e.GetFormat() == Format::EVALUATION && e.GetNumOfElements() == limbs && e.GetRingDimension() == ring;
}
#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "gen_keygen_hybrid: %s does not hold\n", #cond); \
            return false;                                                    \
        }                                                                    \
    } while (0)

static bool record(const std::string& pre, CryptoContext<DCRTPoly> cc, uint32_t ring, uint32_t dnum, uint64_t ns, bool shortLast) {
    cc->Enable(PKE);
    cc->Enable(KEYSWITCH);
    cc->Enable(LEVELEDSHE);
    auto kp = cc->KeyGen();
    cc->EvalMultKeyGen(kp.secretKey);
    cc->EvalRotateKeyGen(kp.secretKey, {1, -1});
    const auto cp       = std::dynamic_pointer_cast<CryptoParametersRNS>(cc->GetCryptoParameters());
    const uint32_t numQ = cp->GetElementParams()->GetParams().size(), numP = cp->GetParamsP()->GetParams().size();
    const uint32_t per  = cp->GetNumPerPartQ();
    REQUIRE(cp->GetKeySwitchTechnique() == HYBRID && cp->GetNumPartQ() == dnum && cp->GetNoiseScale() == ns);
    REQUIRE(cp->GetElementParams()->GetRingDimension() == ring);
    REQUIRE(per * (dnum - 1) < numQ && numQ <= per * dnum && (numQ < per * dnum) == shortLast);
    const auto& s = kp.secretKey->GetPrivateElement();
    REQUIRE(shaped(s, numQ, ring));
    const auto& pk = kp.publicKey->GetPublicElements();
    REQUIRE(pk.size() == 2 && shaped(pk[0], numQ, ring) && shaped(pk[1], numQ, ring));
    const uint32_t kP = cc->FindAutomorphismIndex(1), kM = cc->FindAutomorphismIndex(-1);
    REQUIRE(kP != kM && (uint64_t)kP * kM % (2 * ring) == 1);
    const auto mulKey = cc->GetEvalMultKeyVector(kp.secretKey->GetKeyTag())[0];
    const auto& rots  = cc->GetEvalAutomorphismKeyMap(kp.secretKey->GetKeyTag());
    const auto rotP = rots.at(kP), rotM = rots.at(kM);
    for (const auto& key : {mulKey, rotP, rotM}) {
        REQUIRE(key->GetBVector().size() == dnum && key->GetAVector().size() == dnum);
        for (uint32_t j = 0; j < dnum; ++j)
            REQUIRE(shaped(key->GetBVector()[j], numQ + numP, ring) && shaped(key->GetAVector()[j], numQ + numP, ring));
    }
    put_params(pre + "q", pre + "psiQ", cp->GetElementParams());
    put_params(pre + "p", pre + "psiP", cp->GetParamsP());
    put_polys(pre + "s", {s});
    put_polys(pre + "pkB", {pk[0]}), put_polys(pre + "pkA", {pk[1]});
    put_polys(pre + "mulB", mulKey->GetBVector()), put_polys(pre + "mulA", mulKey->GetAVector());
    put_polys(pre + "rotPB", rotP->GetBVector()), put_polys(pre + "rotPA", rotP->GetAVector());
    put_polys(pre + "rotMB", rotM->GetBVector()), put_polys(pre + "rotMA", rotM->GetAVector());
    const uint64_t sigma100 = (uint64_t)std::llround(100.0 * cp->GetDistributionParameter());
    put_u64(pre + "meta", {ring, ns, numQ, numP, dnum, per, kP, kM, sigma100});
    printf("%s HYBRID: numQ = %u, numP = %u, dnum = %u (%u limbs per digit), ns = %llu, automorphism indices %u / %u\n", pre.c_str(), numQ,
           numP, dnum, per, (unsigned long long)ns, kP, kM);
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2)
        return 2;
    g_out = fopen(argv[1], "wb");
    if (!g_out)
        return 1;
    const uint32_t ring = 64, dnum = 2;
    {
        CCParams<CryptoContextCKKSRNS> parameters;
        parameters.SetSecurityLevel(HEStd_NotSet);
        parameters.SetRingDim(ring);
        parameters.SetMultiplicativeDepth(2);
        parameters.SetScalingModSize(50);
        parameters.SetFirstModSize(60);
        parameters.SetScalingTechnique(FIXEDMANUAL);
        parameters.SetKeySwitchTechnique(HYBRID);
        parameters.SetNumLargeDigits(dnum);
        if (!record("ckks_", GenCryptoContext(parameters), ring, dnum, 1, true))
            return 1;
    }
    {
        const uint64_t t = 65537;
        CCParams<CryptoContextBGVRNS> parameters;
        parameters.SetSecurityLevel(HEStd_NotSet);
        parameters.SetRingDim(ring);
        parameters.SetPlaintextModulus(t);
        parameters.SetMultiplicativeDepth(3);
        parameters.SetScalingTechnique(FIXEDMANUAL);
        parameters.SetKeySwitchTechnique(HYBRID);
        parameters.SetNumLargeDigits(dnum);
        if (!record("bgv_", GenCryptoContext(parameters), ring, dnum, t, false))
            return 1;
    }
    fclose(g_out);
    return 0;
}
