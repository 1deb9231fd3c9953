// TEST INFRASTRUCTURE — generator of tests/golden/ref_vectors_keygen_bv.npz (run by make_golden_keygen_bv.py).
// Links the reference's stock libraries (oracle/_ref), the way gen_keygen_hybrid.cpp does.  The keys the reference's own KeyGen,
// EvalMultKeyGen, EvalRotateKeyGen and ReKeyGen make on BV key switching (KeySwitchBV::KeySwitchGenInternal, keyswitch-bv.cpp:49-225),
// ring dimension 64, HEStd_NotSet, for three parameter sets:
//   bfv0_, bfv10_   BFV, t = 65537, multiplicative depth 4 (3 limbs of 60 bits), digit sizes r = 0 and r = 10
//   ckks10_         CKKS, FIXEDMANUAL, depth 2, first modulus 60 bits, scaling 50 bits (limbs of 60 / 50 / 51 bits), r = 10
// Per set (prefix omitted):
//   q, psiQ                    moduli and roots of Q
//   s, pkB, pkA                the secret key and the public key [numQ][ring], EVALUATION
//   mulB, mulA                 the EvalMultKeyGen key [D_0][numQ][ring]
//   rotPB, rotPA, rotMB, rotMA the EvalRotateKeyGen keys of the index +1 and of the index -1
//   s2, pk2B, pk2A             a second key pair (the delegatee's)
//   reB, reA                   ReKeyGen(secret key, second public key) [D_0][numQ][ring]
//   meta                       ring, noise scale, numQ, r, D_0, automorphism index of +1, of -1, 100 * sigma, t (0: CKKS), the limbs' bits
// BFV sets also: r_q, r_psiQ (the auxiliary basis of the multiplication), ct a fresh ciphertext under the public key [2][numQ][ring],
// m the NativePoly the reference decrypts it to [ring], reM what it decrypts ReEncrypt(ct, reKey) to under the second secret key.
// The generator FAILS unless the shapes are what the meta block says and unless re-encryption decrypts to the encrypted values.
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
static void put_native(const std::string& name, const NativePoly& m) {
    std::vector<uint64_t> o;
    for (size_t k = 0; k < m.GetLength(); ++k)
        o.push_back(m[k].ConvertToInt<uint64_t>());
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
#define REQUIRE(cond)                                                    \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "gen_keygen_bv: %s does not hold\n", #cond); \
            return false;                                                \
        }                                                                \
    } while (0)

static bool record(const std::string& pre, CryptoContext<DCRTPoly> cc, uint32_t ring, uint32_t r, uint64_t t,
                   const std::vector<uint32_t>& bits) {
    cc->Enable(PKE);
    cc->Enable(KEYSWITCH);
    cc->Enable(LEVELEDSHE);
    cc->Enable(PRE);
    auto kp = cc->KeyGen();
    cc->EvalMultKeyGen(kp.secretKey);
    cc->EvalRotateKeyGen(kp.secretKey, {1, -1});
    auto kp2   = cc->KeyGen();
    auto reKey = cc->ReKeyGen(kp.secretKey, kp2.publicKey);
    const auto cp       = std::dynamic_pointer_cast<CryptoParametersRNS>(cc->GetCryptoParameters());
    const uint32_t numQ = cp->GetElementParams()->GetParams().size();
    REQUIRE(cp->GetKeySwitchTechnique() == BV && cp->GetDigitSize() == r && cp->GetNoiseScale() == 1);
    REQUIRE(cp->GetElementParams()->GetRingDimension() == ring && numQ == bits.size());
    REQUIRE(cp->GetSecretKeyDist() == UNIFORM_TERNARY);
    uint32_t D0 = 0;
    std::vector<uint64_t> meta_bits;
    for (uint32_t i = 0; i < numQ; ++i) {
        const uint32_t msb = cp->GetElementParams()->GetParams()[i]->GetModulus().GetMSB();
        REQUIRE(msb == bits[i]);
        D0 += r ? (msb + r - 1) / r : 1;
        meta_bits.push_back(msb);
    }
    const auto& s  = kp.secretKey->GetPrivateElement();
    const auto& s2 = kp2.secretKey->GetPrivateElement();
    REQUIRE(shaped(s, numQ, ring) && shaped(s2, numQ, ring));
    const auto& pk  = kp.publicKey->GetPublicElements();
    const auto& pk2 = kp2.publicKey->GetPublicElements();
    REQUIRE(pk.size() == 2 && shaped(pk[0], numQ, ring) && shaped(pk[1], numQ, ring));
    REQUIRE(pk2.size() == 2 && shaped(pk2[0], numQ, ring) && shaped(pk2[1], numQ, ring));
    const uint32_t kP = cc->FindAutomorphismIndex(1), kM = cc->FindAutomorphismIndex(-1);
    REQUIRE(kP != kM && (uint64_t)kP * kM % (2 * ring) == 1);
    const auto mulKey = cc->GetEvalMultKeyVector(kp.secretKey->GetKeyTag())[0];
    const auto& rots  = cc->GetEvalAutomorphismKeyMap(kp.secretKey->GetKeyTag());
    const auto rotP = rots.at(kP), rotM = rots.at(kM);
    for (const auto& key : {mulKey, rotP, rotM, reKey}) {
        REQUIRE(key->GetBVector().size() == D0 && key->GetAVector().size() == D0);
        for (uint32_t j = 0; j < D0; ++j)
            REQUIRE(shaped(key->GetBVector()[j], numQ, ring) && shaped(key->GetAVector()[j], numQ, ring));
    }
    put_params(pre + "q", pre + "psiQ", cp->GetElementParams());
    put_polys(pre + "s", {s});
    put_polys(pre + "pkB", {pk[0]}), put_polys(pre + "pkA", {pk[1]});
    put_polys(pre + "mulB", mulKey->GetBVector()), put_polys(pre + "mulA", mulKey->GetAVector());
    put_polys(pre + "rotPB", rotP->GetBVector()), put_polys(pre + "rotPA", rotP->GetAVector());
    put_polys(pre + "rotMB", rotM->GetBVector()), put_polys(pre + "rotMA", rotM->GetAVector());
    put_polys(pre + "s2", {s2});
    put_polys(pre + "pk2B", {pk2[0]}), put_polys(pre + "pk2A", {pk2[1]});
    put_polys(pre + "reB", reKey->GetBVector()), put_polys(pre + "reA", reKey->GetAVector());
    if (t) {
        const auto bfv = std::dynamic_pointer_cast<CryptoParametersBFVRNS>(cc->GetCryptoParameters());
        REQUIRE(bfv && bfv->GetMultiplicationTechnique() == HPSPOVERQLEVELED && bfv->GetPlaintextModulus() == t);
        put_params(pre + "r_q", pre + "r_psiQ", bfv->GetParamsRl(numQ - 1));
        std::vector<int64_t> v(ring);
        for (uint32_t i = 0; i < ring; ++i)
            v[i] = (int64_t)((i * 7 + r) % 5) - 2;
        auto ct = cc->Encrypt(kp.publicKey, cc->MakePackedPlaintext(v));
        REQUIRE(ct->GetElements().size() == 2 && shaped(ct->GetElements()[0], numQ, ring) && shaped(ct->GetElements()[1], numQ, ring));
        ConstCiphertext<DCRTPoly> cct = ct;
        NativePoly m, m2;
        cc->GetScheme()->Decrypt(cct, kp.secretKey, &m);
        REQUIRE(m.GetLength() == ring && m.GetFormat() == Format::COEFFICIENT && m.GetModulus() == NativeInteger(t));
        auto re = cc->ReEncrypt(ct, reKey);
        REQUIRE(re->GetElements().size() == 2 && shaped(re->GetElements()[0], numQ, ring));
        ConstCiphertext<DCRTPoly> cre = re;
        cc->GetScheme()->Decrypt(cre, kp2.secretKey, &m2);
        Plaintext pt;
        cc->Decrypt(kp2.secretKey, re, &pt);
        pt->SetLength(v.size());
        REQUIRE(pt->GetPackedValue() == v);
        for (uint32_t i = 0; i < ring; ++i)
            REQUIRE(m[i] == m2[i]);
        put_polys(pre + "ct", ct->GetElements());
        put_native(pre + "m", m), put_native(pre + "reM", m2);
    }
    const uint64_t sigma100 = (uint64_t)std::llround(100.0 * cp->GetDistributionParameter());
    std::vector<uint64_t> meta = {ring, 1, numQ, r, D0, kP, kM, sigma100, t};
    meta.insert(meta.end(), meta_bits.begin(), meta_bits.end());
    put_u64(pre + "meta", meta);
    printf("%s BV: numQ = %u, r = %u, D_0 = %u, automorphism indices %u / %u\n", pre.c_str(), numQ, r, D0, kP, kM);
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2)
        return 2;
    g_out = fopen(argv[1], "wb");
    if (!g_out)
        return 1;
    const uint32_t ring = 64;
    for (uint32_t r : {0u, 10u}) {
        const uint64_t t = 65537;
        CCParams<CryptoContextBFVRNS> parameters;
        parameters.SetSecurityLevel(HEStd_NotSet);
        parameters.SetRingDim(ring);
        parameters.SetPlaintextModulus(t);
        parameters.SetMultiplicativeDepth(4);
        parameters.SetScalingModSize(60);
        parameters.SetKeySwitchTechnique(BV);
        parameters.SetDigitSize(r);
        if (!record("bfv" + std::to_string(r) + "_", GenCryptoContext(parameters), ring, r, t, {60, 60, 60}))
            return 1;
    }
    {
        CCParams<CryptoContextCKKSRNS> parameters;
        parameters.SetSecurityLevel(HEStd_NotSet);
        parameters.SetRingDim(ring);
        parameters.SetMultiplicativeDepth(2);
        parameters.SetScalingModSize(50);
        parameters.SetFirstModSize(60);
        parameters.SetScalingTechnique(FIXEDMANUAL);
        parameters.SetKeySwitchTechnique(BV);
        parameters.SetDigitSize(10);
        if (!record("ckks10_", GenCryptoContext(parameters), ring, 10, 0, {60, 50, 51}))
            return 1;
    }
    fclose(g_out);
    return 0;
}
