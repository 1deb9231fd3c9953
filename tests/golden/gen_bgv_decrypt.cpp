// TEST INFRASTRUCTURE — generator of tests/golden/ref_vectors_bgv_decrypt.npz (run by make_golden_bgv_decrypt.py).
// Links the reference's stock libraries (oracle/_ref), the way gen_bgv_hybrid.cpp does.  BGV decryption through the reference's scheme
// layer (PKEBGVRNS::Decrypt, bgvrns-pke.cpp:44-99) at ring dimension 64, t = 65537, multiplicative depth 3, HEStd_NotSet.  Two contexts:
// FIXEDMANUAL (prefix "fm_") and the default FLEXIBLEAUTOEXT (prefix "fx_").  Per context
//   <p>q, <p>psi       moduli and roots of Q
//   <p>s               the secret key, [numQ][ring], EVALUATION
// and per case <c> (fm_fresh: a fresh ciphertext; fm_prod: the three-element product cc->EvalMultNoRelin(a, b); fm_reduced: cc->ModReduce of a
// fresh ciphertext; fx_fresh: a fresh ciphertext under FLEXIBLEAUTOEXT)
//   <c>_c              the elements, [nElem][sizeQl][ring], EVALUATION
//   <c>_m              the NativePoly that PKEBGVRNS::Decrypt hands back before decoding, [ring], values in [0, t)
//   <c>_meta           nElem, sizeQl
// meta: ring, t.
// The generator FAILS unless every case has sizeQl >= 2 and its elements in EVALUATION, and cc->Decrypt of it decodes to the encoded values.
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
#define REQUIRE(cond)                                                       \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "gen_bgv_decrypt: %s does not hold\n", #cond); \
            return false;                                                   \
        }                                                                   \
    } while (0)

static const uint32_t kRing = 64;
static const uint64_t kT    = 65537;

// one case: the elements, the NativePoly of the scheme's Decrypt, and the check that the context's Decrypt decodes to `want`
static bool put_case(const std::string& name, CryptoContext<DCRTPoly> cc, const PrivateKey<DCRTPoly>& sk, const Ciphertext<DCRTPoly>& ct,
                     size_t nElem, const std::vector<int64_t>& want) {
    const auto& cv = ct->GetElements();
    REQUIRE(cv.size() == nElem && cv[0].GetNumOfElements() >= 2);
    for (const auto& e : cv)
        REQUIRE(e.GetFormat() == Format::EVALUATION && e.GetNumOfElements() == cv[0].GetNumOfElements());
    ConstCiphertext<DCRTPoly> cct = ct;
    NativePoly m;
    cc->GetScheme()->Decrypt(cct, sk, &m);
    REQUIRE(m.GetLength() == kRing && m.GetFormat() == Format::COEFFICIENT);
    std::vector<uint64_t> mw;
    for (size_t k = 0; k < kRing; ++k)
        mw.push_back(m[k].ConvertToInt<uint64_t>());
    Plaintext pt;
    cc->Decrypt(sk, ct, &pt);
    pt->SetLength(want.size());
    REQUIRE(pt->GetPackedValue() == want);
    put_u64(name + "_c", words(cv));
    put_u64(name + "_m", mw);
    put_u64(name + "_meta", {nElem, cv[0].GetNumOfElements()});
    printf("%s: %zu elements, sizeQl = %zu\n", name.c_str(), nElem, (size_t)cv[0].GetNumOfElements());
    return true;
}

static bool context(const std::string& prefix, bool fixedManual) {
    CCParams<CryptoContextBGVRNS> parameters;
    parameters.SetSecurityLevel(HEStd_NotSet);
    parameters.SetRingDim(kRing);
    parameters.SetPlaintextModulus(kT);
    parameters.SetMultiplicativeDepth(3);
    if (fixedManual)
        parameters.SetScalingTechnique(FIXEDMANUAL);
    auto cc = GenCryptoContext(parameters);
    cc->Enable(PKE);
    cc->Enable(KEYSWITCH);
    cc->Enable(LEVELEDSHE);
    const auto cp = std::dynamic_pointer_cast<CryptoParametersBGVRNS>(cc->GetCryptoParameters());
    REQUIRE(cp->GetScalingTechnique() == (fixedManual ? FIXEDMANUAL : FLEXIBLEAUTOEXT) && cp->GetPlaintextModulus() == kT);
    auto kp = cc->KeyGen();
    std::mt19937_64 gen(fixedManual ? 53 : 59);
    auto values = [&]() {
        std::vector<int64_t> v(kRing / 2);
        for (auto& e : v)
            e = static_cast<int64_t>(gen() % 7) - 3;
        return v;
    };
    std::vector<uint64_t> qs, roots;
    for (const auto& l : cp->GetElementParams()->GetParams()) {
        qs.push_back(l->GetModulus().ConvertToInt<uint64_t>());
        roots.push_back(l->GetRootOfUnity().ConvertToInt<uint64_t>());
    }
    const DCRTPoly& s = kp.secretKey->GetPrivateElement();
    REQUIRE(s.GetFormat() == Format::EVALUATION && s.GetNumOfElements() == qs.size());
    put_u64(prefix + "q", qs), put_u64(prefix + "psi", roots), put_u64(prefix + "s", words({s}));

    const auto va = values(), vb = values();
    auto a = cc->Encrypt(kp.publicKey, cc->MakePackedPlaintext(va));
    if (!put_case(prefix + "fresh", cc, kp.secretKey, a, 2, va))
        return false;
    if (!fixedManual)
        return true;
    auto b = cc->Encrypt(kp.publicKey, cc->MakePackedPlaintext(vb));
    std::vector<int64_t> vab(va.size());
    for (size_t i = 0; i < va.size(); ++i)
        vab[i] = va[i] * vb[i];
    if (!put_case(prefix + "prod", cc, kp.secretKey, cc->EvalMultNoRelin(a, b), 3, vab))
        return false;
    auto r = cc->ModReduce(b);
    REQUIRE(r->GetElements()[0].GetNumOfElements() + 1 == b->GetElements()[0].GetNumOfElements());
    return put_case(prefix + "reduced", cc, kp.secretKey, r, 2, vb);
}

int main(int argc, char** argv) {
    if (argc < 2)
        return 2;
    g_out = fopen(argv[1], "wb");
    if (!g_out)
        return 1;
    if (!context("fm_", true) || !context("fx_", false))
        return 1;
    put_u64("meta", {kRing, kT});
    fclose(g_out);
    return 0;
}
