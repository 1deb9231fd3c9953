// TEST INFRASTRUCTURE — generator of tests/golden/ref_vectors_encrypt.npz (run by make_golden_encrypt.py).
// Links the reference's stock libraries (oracle/_ref), the way gen_keygen_hybrid.cpp does.  Fresh ciphertexts of the reference's own
// Encrypt under the secret key and under the public key (PKERNS::Encrypt, rns-pke.cpp:40-70; PKEBFVRNS::Encrypt, bfvrns-pke.cpp:99-213),
// ring dimension 64, HEStd_NotSet, for four parameter sets:
//   ckks_   CKKS, FIXEDMANUAL, depth 2 (3 limbs): one plaintext at full level and one encoded one level down (2 limbs)
//   ckksg_  the same with SecretKeyDist = GAUSSIAN (v of the public-key form is Gaussian)
//   bgv_    BGV, FIXEDMANUAL, t = 65537, depth 2
//   bfv_    BFV, HPS multiplication, STANDARD encryption, t = 65537, depth 2
// Per set (prefix omitted):
//   q, psi          moduli and roots of Q
//   s, pkB, pkA     the secret key and the public key's two elements [numQ][ring], EVALUATION
//   pt              the plaintext DCRTPoly handed to Encrypt [limbs][ring], in the format Encrypt first puts it in: EVALUATION (CKKS, BGV),
//                   COEFFICIENT (BFV)
//   sk0, sk1        the two elements of Encrypt(pt, secretKey) [limbs][ring], EVALUATION;  pk0, pk1: of Encrypt(pt, publicKey)
//   ptd, skd0, skd1, pkd0, pkd1   the same for the plaintext encoded one level down (ckks_ only)
//   negQModt, tInvModq            GetNegQModt(0), GettInvModq() (bfv_ only)
//   meta            ring, noise scale, numQ, t (0: none), 100 * sigma, 1 if the secret is Gaussian, limbs of the level-down plaintext (0: none)
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
static void put_poly(const std::string& name, const DCRTPoly& e) {
    std::vector<uint64_t> o;
    for (size_t i = 0; i < e.GetNumOfElements(); ++i)
        for (size_t k = 0; k < e.GetRingDimension(); ++k)
            o.push_back(e.GetElementAtIndex(i)[k].ConvertToInt<uint64_t>());
    put_u64(name, o);
}
static bool shaped(const DCRTPoly& e, size_t limbs, uint32_t ring, Format f = Format::EVALUATION) {
    return e.GetFormat() == f && e.GetNumOfElements() == limbs && e.GetRingDimension() == ring;
}
#define REQUIRE(cond)                                                  \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "gen_encrypt: %s does not hold\n", #cond); \
            return false;                                              \
        }                                                              \
    } while (0)

// Encrypt(pt) under both keys; records pt and the four elements under the names pt<tag>, sk<tag>0 ...
static bool encrypt_both(const std::string& pre, const std::string& tag, CryptoContext<DCRTPoly> cc, const KeyPair<DCRTPoly>& kp,
                         Plaintext pt, size_t limbs, uint32_t ring, Format ptFormat) {
    DCRTPoly handed = pt->GetElement<DCRTPoly>();
    REQUIRE(handed.GetNumOfElements() == limbs && handed.GetRingDimension() == ring);
    handed.SetFormat(ptFormat);  // (the first thing Encrypt does to its copy)
    auto ctS = cc->Encrypt(kp.secretKey, pt);
    auto ctP = cc->Encrypt(kp.publicKey, pt);
    for (const auto& ct : {ctS, ctP}) {
        REQUIRE(ct->GetElements().size() == 2);
        REQUIRE(shaped(ct->GetElements()[0], limbs, ring) && shaped(ct->GetElements()[1], limbs, ring));
    }
    put_poly(pre + "pt" + tag, handed);
    put_poly(pre + "sk" + tag + "0", ctS->GetElements()[0]), put_poly(pre + "sk" + tag + "1", ctS->GetElements()[1]);
    put_poly(pre + "pk" + tag + "0", ctP->GetElements()[0]), put_poly(pre + "pk" + tag + "1", ctP->GetElements()[1]);
    return true;
}

// kind: 0 CKKS, 1 BGV, 2 BFV
static bool record(const std::string& pre, CryptoContext<DCRTPoly> cc, int kind, uint32_t ring, uint64_t ns, uint64_t t, bool gaussian,
                   bool levelDown) {
    cc->Enable(PKE);
    cc->Enable(LEVELEDSHE);
    auto kp             = cc->KeyGen();
    const auto cp       = std::dynamic_pointer_cast<CryptoParametersRNS>(cc->GetCryptoParameters());
    const uint32_t numQ = cp->GetElementParams()->GetParams().size();
    REQUIRE(cp->GetNoiseScale() == ns && cp->GetElementParams()->GetRingDimension() == ring);
    REQUIRE((cp->GetSecretKeyDist() == GAUSSIAN) == gaussian);
    REQUIRE(numQ >= (levelDown ? 2u : 1u));
    const auto& s = kp.secretKey->GetPrivateElement();
    REQUIRE(shaped(s, numQ, ring));
    const auto& pk = kp.publicKey->GetPublicElements();
    REQUIRE(pk.size() == 2 && shaped(pk[0], numQ, ring) && shaped(pk[1], numQ, ring));
    std::vector<uint64_t> qs, roots;
    for (const auto& l : cp->GetElementParams()->GetParams()) {
        qs.push_back(l->GetModulus().ConvertToInt<uint64_t>());
        roots.push_back(l->GetRootOfUnity().ConvertToInt<uint64_t>());
    }
    put_u64(pre + "q", qs), put_u64(pre + "psi", roots);
    put_poly(pre + "s", s), put_poly(pre + "pkB", pk[0]), put_poly(pre + "pkA", pk[1]);
    if (kind == 0) {
        std::vector<double> x;
        for (uint32_t i = 0; i < ring / 2; ++i)
            x.push_back(0.25 * std::sin(0.7 * i) + 0.001 * i);
        if (!encrypt_both(pre, "", cc, kp, cc->MakeCKKSPackedPlaintext(x), numQ, ring, Format::EVALUATION))
            return false;
        if (levelDown && !encrypt_both(pre, "d", cc, kp, cc->MakeCKKSPackedPlaintext(x, 1, 1), numQ - 1, ring, Format::EVALUATION))
            return false;
    } else {
        std::vector<int64_t> x;
        for (uint32_t i = 0; i < ring; ++i)
            x.push_back((int64_t)((i * 7919u + 13u) % t) - (int64_t)(t / 2));  // both signs, within [-t/2, t/2]
        if (!encrypt_both(pre, "", cc, kp, cc->MakePackedPlaintext(x), numQ, ring, kind == 2 ? Format::COEFFICIENT : Format::EVALUATION))
            return false;
    }
    if (kind == 2) {
        const auto bfv = std::dynamic_pointer_cast<CryptoParametersBFVRNS>(cc->GetCryptoParameters());
        REQUIRE(bfv->GetEncryptionTechnique() == STANDARD && bfv->GetMultiplicationTechnique() == HPS);
        std::vector<uint64_t> tInv;
        for (const auto& v : bfv->GettInvModq())
            tInv.push_back(v.ConvertToInt<uint64_t>());
        REQUIRE(tInv.size() == numQ);
        put_u64(pre + "negQModt", {bfv->GetNegQModt(0).ConvertToInt<uint64_t>()});
        put_u64(pre + "tInvModq", tInv);
    }
    const uint64_t sigma100 = (uint64_t)std::llround(100.0 * cp->GetDistributionParameter());
    put_u64(pre + "meta", {ring, ns, numQ, t, sigma100, gaussian ? 1u : 0u, levelDown ? numQ - 1 : 0u});
    printf("%s numQ = %u, ns = %llu, t = %llu, sigma = %.2f, Gaussian secret: %d, level-down limbs: %u\n", pre.c_str(), numQ,
           (unsigned long long)ns, (unsigned long long)t, sigma100 / 100.0, (int)gaussian, levelDown ? numQ - 1 : 0u);
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2)
        return 2;
    g_out = fopen(argv[1], "wb");
    if (!g_out)
        return 1;
    const uint32_t ring = 64;
    const uint64_t t    = 65537;
    for (int gaussian = 0; gaussian < 2; ++gaussian) {
        CCParams<CryptoContextCKKSRNS> parameters;
        parameters.SetSecurityLevel(HEStd_NotSet);
        parameters.SetRingDim(ring);
        parameters.SetMultiplicativeDepth(2);
        parameters.SetScalingModSize(50);
        parameters.SetFirstModSize(60);
        parameters.SetScalingTechnique(FIXEDMANUAL);
        if (gaussian)
            parameters.SetSecretKeyDist(GAUSSIAN);
        if (!record(gaussian ? "ckksg_" : "ckks_", GenCryptoContext(parameters), 0, ring, 1, 0, gaussian, !gaussian))
            return 1;
    }
    {
        CCParams<CryptoContextBGVRNS> parameters;
        parameters.SetSecurityLevel(HEStd_NotSet);
        parameters.SetRingDim(ring);
        parameters.SetPlaintextModulus(t);
        parameters.SetMultiplicativeDepth(2);
        parameters.SetScalingTechnique(FIXEDMANUAL);
        if (!record("bgv_", GenCryptoContext(parameters), 1, ring, t, t, false, false))
            return 1;
    }
    {
        CCParams<CryptoContextBFVRNS> parameters;
        parameters.SetSecurityLevel(HEStd_NotSet);
        parameters.SetRingDim(ring);
        parameters.SetPlaintextModulus(t);
        parameters.SetMultiplicativeDepth(2);
        parameters.SetMultiplicationTechnique(HPS);
        parameters.SetEncryptionTechnique(STANDARD);
        if (!record("bfv_", GenCryptoContext(parameters), 2, ring, 1, t, false, false))
            return 1;
    }
    fclose(g_out);
    return 0;
}
