// TEST INFRASTRUCTURE — generator of tests/golden/ref_vectors_decrypt.npz (run by make_golden_decrypt.py).
// Links the reference's stock libraries (oracle/_ref), the way gen_bgv_decrypt.cpp does.  Decryption through the reference's scheme layer
// for BFV and CKKS, single-key and two-party threshold, at ring dimension 64, HEStd_NotSet.  Parameter sets (prefix):
//   hps_    BFV, HPSPOVERQLEVELED, t = 65537, default 60-bit moduli: the split ("B") branch of the decryption ScaleAndRound
//   hpsu_   BFV, HPS, t = 65537, 45-bit moduli: the unsplit branch (qMSB + sizeQMSB < 52).  (The reference's parameter generation does
//           produce such a set at this ring with SetScalingModSize(45); the generator fails if the branch is not the unsplit one.)
//   behz_   BFV, BEHZ, t = 65537
//   ckks_   CKKS, FIXEDMANUAL, 50-bit scaling, depth 2 (3 limbs)
//   tbfv_   BFV, HPS, t = 65537, two parties;   tckks_  CKKS as ckks_, two parties
// Per set: <p>q, <p>psi (moduli and roots of Q), <p>s (the secret key [numQ][ring], EVALUATION; the threshold sets: <p>s1, <p>s2, the two
// shares), <p>meta (ring, numQ, t or 0, technique: 0 BEHZ, 1 HPS, 2 HPSPOVERQ, 3 HPSPOVERQLEVELED, 9 CKKS; noise scale).
// BFV tables as CryptoParametersBFVRNS holds them: <p>tQHatInvModqDivqModt, <p>tQHatInvModqDivqFrac and, on the split branch,
// <p>tQHatInvModqBDivqModt, <p>tQHatInvModqBDivqFrac (doubles as their 64 bits); behz_tgamma, behz_tgammaQHatInvModq,
// behz_negInvqModtgamma.
// Cases <c>: hps_fresh, hps_prod (cc->EvalMultNoRelin, three elements), hpsu_fresh, hpsu_prod, behz_fresh; ckks_fresh, ckks_rescaled (EvalMult by
// 1.0 and Rescale: 2 limbs), ckks_prod (three elements), ckks_one (LevelReduce to one limb).  Per case
//   <c>_c      the elements [nElem][sizeQl][ring], in the format the reference holds them in (BFV's product: COEFFICIENT; PKERNS::DecryptCore
//              puts its copies into EVALUATION first, rns-pke.cpp:212-218)
//   <c>_m      BFV: the NativePoly of GetScheme()->Decrypt(ct, sk, NativePoly*) [ring], values in [0, t)
//   <c>_b      CKKS: the Poly of GetScheme()->Decrypt(ct, sk, Poly*) reduced modulo every q_i with the reference's big integers
//              [sizeQl][ring]; ckks_one: the NativePoly of Decrypt(ct, sk, NativePoly*) [1][ring]
//   <c>_meta   nElem, sizeQl, format of the elements (0 EVALUATION, 1 COEFFICIENT)
// Threshold sets: <p>c the joint ciphertext [2][numQ][ring]; <p>lead, <p>main the one element of MultipartyDecryptLead(ct, s1) and
// MultipartyDecryptMain(ct, s2) [numQ][ring], EVALUATION; <p>fusion the result of GetScheme()->MultipartyDecryptFusion: the NativePoly
// [ring] (tbfv_), the Poly's residues [numQ][ring] (tckks_).
// The generator FAILS unless every shape is what its meta block says and unless every case decodes to the encoded values.
// Record format: u32 name length, name, u32 type (0 = u64), u64 count, data.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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
static std::vector<uint64_t> words(const NativePoly& m) {
    std::vector<uint64_t> o;
    for (size_t k = 0; k < m.GetLength(); ++k)
        o.push_back(m[k].ConvertToInt<uint64_t>());
    return o;
}
static std::vector<uint64_t> words(const std::vector<NativeInteger>& v) {
    std::vector<uint64_t> o;
    for (const auto& x : v)
        o.push_back(x.ConvertToInt<uint64_t>());
    return o;
}
static std::vector<uint64_t> bits(const std::vector<double>& v) {
    std::vector<uint64_t> o(v.size());
    if (!v.empty())
        std::memcpy(o.data(), v.data(), 8 * v.size());
    return o;
}
// the residues of a Poly's coefficients modulo every q_i, with the reference's own big integers: [sizeQl][ring]
static std::vector<uint64_t> residues(const Poly& p, const std::vector<uint64_t>& qs, size_t sizeQl) {
    std::vector<uint64_t> o;
    for (size_t i = 0; i < sizeQl; ++i) {
        const BigInteger qi(qs[i]);
        for (size_t k = 0; k < p.GetLength(); ++k)
            o.push_back(p[k].Mod(qi).ConvertToInt<uint64_t>());
    }
    return o;
}
#define REQUIRE(cond)                                                  \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "gen_decrypt: %s does not hold\n", #cond); \
            return false;                                              \
        }                                                              \
    } while (0)

static const uint32_t kRing = 64;
static const uint64_t kT    = 65537;

static bool put_params(const std::string& pre, CryptoContext<DCRTPoly> cc, std::vector<uint64_t>& qs) {
    const auto cp = std::dynamic_pointer_cast<CryptoParametersRNS>(cc->GetCryptoParameters());
    REQUIRE(cp->GetElementParams()->GetRingDimension() == kRing);
    std::vector<uint64_t> roots;
    qs.clear();
    for (const auto& l : cp->GetElementParams()->GetParams()) {
        qs.push_back(l->GetModulus().ConvertToInt<uint64_t>());
        roots.push_back(l->GetRootOfUnity().ConvertToInt<uint64_t>());
    }
    put_u64(pre + "q", qs), put_u64(pre + "psi", roots);
    return true;
}
static bool put_key(const std::string& name, const PrivateKey<DCRTPoly>& sk, size_t numQ) {
    const DCRTPoly& s = sk->GetPrivateElement();
    REQUIRE(s.GetFormat() == Format::EVALUATION && s.GetNumOfElements() == numQ && s.GetRingDimension() == kRing);
    put_u64(name, words({s}));
    return true;
}
static bool shaped(const std::vector<DCRTPoly>& cv, size_t nElem, size_t sizeQl, Format f = Format::EVALUATION) {
    REQUIRE(cv.size() == nElem);
    for (const auto& e : cv)
        REQUIRE(e.GetFormat() == f && e.GetNumOfElements() == sizeQl && e.GetRingDimension() == kRing);
    return true;
}
static std::vector<int64_t> bfv_values(uint32_t salt) {
    std::vector<int64_t> v(kRing);
    for (uint32_t i = 0; i < kRing; ++i)
        v[i] = (int64_t)((i * 7919u + salt) % 201u) - 100;  // both signs; products stay within [-t/2, t/2]
    return v;
}
static std::vector<double> ckks_values(double phase) {
    std::vector<double> x;
    for (uint32_t i = 0; i < kRing / 2; ++i)
        x.push_back(0.25 * std::sin(0.7 * i + phase) + 0.001 * i);
    return x;
}
static bool close_to(Plaintext pt, const std::vector<double>& want, double tol) {
    pt->SetLength(want.size());
    const auto got = pt->GetRealPackedValue();
    REQUIRE(got.size() == want.size());
    for (size_t i = 0; i < want.size(); ++i)
        REQUIRE(std::fabs(got[i] - want[i]) < tol);
    return true;
}

// ---- BFV ----
static bool bfv_case(const std::string& name, CryptoContext<DCRTPoly> cc, const PrivateKey<DCRTPoly>& sk, const Ciphertext<DCRTPoly>& ct,
                     size_t nElem, size_t numQ, const std::vector<int64_t>& want) {
    const Format f = ct->GetElements()[0].GetFormat();  // (the product's elements are COEFFICIENT: DecryptCore transforms its copies)
    if (!shaped(ct->GetElements(), nElem, numQ, f))
        return false;
    ConstCiphertext<DCRTPoly> cct = ct;
    NativePoly m;
    cc->GetScheme()->Decrypt(cct, sk, &m);
    REQUIRE(m.GetLength() == kRing && m.GetFormat() == Format::COEFFICIENT && m.GetModulus() == NativeInteger(kT));
    Plaintext pt;
    cc->Decrypt(sk, ct, &pt);
    pt->SetLength(want.size());
    REQUIRE(pt->GetPackedValue() == want);
    put_u64(name + "_c", words(ct->GetElements()));
    put_u64(name + "_m", words(m));
    put_u64(name + "_meta", {nElem, numQ, f == Format::EVALUATION ? 0u : 1u});
    printf("%s: %zu elements, sizeQl = %zu, format %d\n", name.c_str(), nElem, numQ, (int)f);
    return true;
}
static bool put_bfv_tables(const std::string& pre, const std::shared_ptr<CryptoParametersBFVRNS>& cp, size_t numQ, bool behz, int split) {
    if (behz) {
        REQUIRE(cp->GettgammaQHatInvModq().size() == numQ && cp->GetNegInvqModtgamma().size() == numQ);
        put_u64(pre + "tgamma", {cp->Gettgamma().ConvertToInt<uint64_t>()});
        put_u64(pre + "tgammaQHatInvModq", words(cp->GettgammaQHatInvModq()));
        put_u64(pre + "negInvqModtgamma", words(cp->GetNegInvqModtgamma()));
        return true;
    }
    REQUIRE(cp->GettQHatInvModqDivqModt().size() == numQ && cp->GettQHatInvModqDivqFrac().size() == numQ);
    REQUIRE(cp->GettQHatInvModqBDivqModt().size() == (split ? numQ : 0) && cp->GettQHatInvModqBDivqFrac().size() == (split ? numQ : 0));
    put_u64(pre + "tQHatInvModqDivqModt", words(cp->GettQHatInvModqDivqModt()));
    put_u64(pre + "tQHatInvModqDivqFrac", bits(cp->GettQHatInvModqDivqFrac()));
    if (split) {
        put_u64(pre + "tQHatInvModqBDivqModt", words(cp->GettQHatInvModqBDivqModt()));
        put_u64(pre + "tQHatInvModqBDivqFrac", bits(cp->GettQHatInvModqBDivqFrac()));
    }
    return true;
}
static CryptoContext<DCRTPoly> bfv_context(MultiplicationTechnique tech, uint32_t modSize, bool threshold) {
    CCParams<CryptoContextBFVRNS> parameters;
    parameters.SetSecurityLevel(HEStd_NotSet);
    parameters.SetRingDim(kRing);
    parameters.SetPlaintextModulus(kT);
    parameters.SetMultiplicativeDepth(2);
    parameters.SetMultiplicationTechnique(tech);
    parameters.SetEncryptionTechnique(STANDARD);
    if (modSize)
        parameters.SetScalingModSize(modSize);
    auto cc = GenCryptoContext(parameters);
    cc->Enable(PKE);
    cc->Enable(KEYSWITCH);
    cc->Enable(LEVELEDSHE);
    if (threshold)
        cc->Enable(MULTIPARTY);
    return cc;
}
// technique id of the meta block and of fhe_bfv_decrypt_create
static uint64_t technique_id(MultiplicationTechnique t) {
    return t == BEHZ ? 0 : t == HPS ? 1 : t == HPSPOVERQ ? 2 : 3;
}
static bool bfv_set(const std::string& pre, MultiplicationTechnique tech, uint32_t modSize, int wantSplit, bool withProduct) {
    auto cc       = bfv_context(tech, modSize, false);
    const auto cp = std::dynamic_pointer_cast<CryptoParametersBFVRNS>(cc->GetCryptoParameters());
    REQUIRE(cp->GetMultiplicationTechnique() == tech && cp->GetPlaintextModulus() == kT && cp->GetNoiseScale() == 1);
    std::vector<uint64_t> qs;
    if (!put_params(pre, cc, qs))
        return false;
    const size_t numQ = qs.size();
    uint64_t qmax     = 0;
    for (uint64_t q : qs)
        qmax = std::max(qmax, q);
    const int split = (GetMSB64(qmax) + GetMSB64(numQ) < 52) ? 0 : 1;  // bfvrns-cryptoparameters.cpp:438-445
    REQUIRE(tech == BEHZ || split == wantSplit);
    auto kp = cc->KeyGen();
    if (!put_key(pre + "s", kp.secretKey, numQ) || !put_bfv_tables(pre, cp, numQ, tech == BEHZ, split))
        return false;
    const auto va = bfv_values(13), vb = bfv_values(101);
    auto a = cc->Encrypt(kp.publicKey, cc->MakePackedPlaintext(va));
    if (!bfv_case(pre + "fresh", cc, kp.secretKey, a, 2, numQ, va))
        return false;
    if (withProduct) {
        auto b = cc->Encrypt(kp.publicKey, cc->MakePackedPlaintext(vb));
        std::vector<int64_t> vab(va.size());
        for (size_t i = 0; i < va.size(); ++i)
            vab[i] = va[i] * vb[i];
        if (!bfv_case(pre + "prod", cc, kp.secretKey, cc->EvalMultNoRelin(a, b), 3, numQ, vab))
            return false;
    }
    put_u64(pre + "meta", {kRing, numQ, kT, technique_id(tech), 1});
    printf("%s numQ = %zu, qMSB = %u, split = %d\n", pre.c_str(), numQ, (unsigned)GetMSB64(qmax), split);
    return true;
}

// ---- CKKS ----
static CryptoContext<DCRTPoly> ckks_context(bool threshold) {
    CCParams<CryptoContextCKKSRNS> parameters;
    parameters.SetSecurityLevel(HEStd_NotSet);
    parameters.SetRingDim(kRing);
    parameters.SetMultiplicativeDepth(2);
    parameters.SetScalingModSize(50);
    parameters.SetFirstModSize(60);
    parameters.SetScalingTechnique(FIXEDMANUAL);
    auto cc = GenCryptoContext(parameters);
    cc->Enable(PKE);
    cc->Enable(KEYSWITCH);
    cc->Enable(LEVELEDSHE);
    if (threshold)
        cc->Enable(MULTIPARTY);
    return cc;
}
static bool ckks_case(const std::string& name, CryptoContext<DCRTPoly> cc, const PrivateKey<DCRTPoly>& sk, const Ciphertext<DCRTPoly>& ct,
                      size_t nElem, size_t sizeQl, const std::vector<uint64_t>& qs, const std::vector<double>& want) {
    if (!shaped(ct->GetElements(), nElem, sizeQl))
        return false;
    ConstCiphertext<DCRTPoly> cct = ct;
    std::vector<uint64_t> b;
    if (sizeQl == 1) {
        NativePoly m;
        cc->GetScheme()->Decrypt(cct, sk, &m);
        REQUIRE(m.GetLength() == kRing && m.GetFormat() == Format::COEFFICIENT && m.GetModulus() == NativeInteger(qs[0]));
        b = words(m);
    } else {
        Poly p;
        cc->GetScheme()->Decrypt(cct, sk, &p);
        REQUIRE(p.GetLength() == kRing && p.GetFormat() == Format::COEFFICIENT);
        b = residues(p, qs, sizeQl);
    }
    Plaintext pt;
    cc->Decrypt(sk, ct, &pt);
    if (!close_to(pt, want, 1e-6))
        return false;
    put_u64(name + "_c", words(ct->GetElements()));
    put_u64(name + "_b", b);
    put_u64(name + "_meta", {nElem, sizeQl, 0});
    printf("%s: %zu elements, sizeQl = %zu\n", name.c_str(), nElem, sizeQl);
    return true;
}
static bool ckks_set(const std::string& pre) {
    auto cc       = ckks_context(false);
    const auto cp = std::dynamic_pointer_cast<CryptoParametersCKKSRNS>(cc->GetCryptoParameters());
    REQUIRE(cp->GetScalingTechnique() == FIXEDMANUAL && cp->GetNoiseScale() == 1);
    REQUIRE(cp->GetDecryptionNoiseMode() == FIXED_NOISE_DECRYPT);
    std::vector<uint64_t> qs;
    if (!put_params(pre, cc, qs))
        return false;
    const size_t numQ = qs.size();
    REQUIRE(numQ == 3);
    auto kp = cc->KeyGen();
    if (!put_key(pre + "s", kp.secretKey, numQ))
        return false;
    const auto xa = ckks_values(0.0), xb = ckks_values(1.0);
    auto a = cc->Encrypt(kp.publicKey, cc->MakeCKKSPackedPlaintext(xa));
    auto b = cc->Encrypt(kp.publicKey, cc->MakeCKKSPackedPlaintext(xb));
    if (!ckks_case(pre + "fresh", cc, kp.secretKey, a, 2, 3, qs, xa))
        return false;
    auto r = cc->Rescale(cc->EvalMult(a, 1.0));
    if (!ckks_case(pre + "rescaled", cc, kp.secretKey, r, 2, 2, qs, xa))
        return false;
    std::vector<double> xab(xa.size());
    for (size_t i = 0; i < xa.size(); ++i)
        xab[i] = xa[i] * xb[i];
    if (!ckks_case(pre + "prod", cc, kp.secretKey, cc->EvalMultNoRelin(a, b), 3, 3, qs, xab))
        return false;
    if (!ckks_case(pre + "one", cc, kp.secretKey, cc->LevelReduce(b, nullptr, 2), 2, 1, qs, xb))
        return false;
    put_u64(pre + "meta", {kRing, numQ, 0, 9, 1});
    return true;
}

// ---- two-party threshold decryption ----
static bool threshold_set(const std::string& pre, bool ckks) {
    auto cc       = ckks ? ckks_context(true) : bfv_context(HPS, 0, true);
    const auto cp = std::dynamic_pointer_cast<CryptoParametersRNS>(cc->GetCryptoParameters());
    REQUIRE(cp->GetNoiseScale() == 1 && cp->GetMultipartyMode() == FIXED_NOISE_MULTIPARTY);
    REQUIRE(cp->GetDecryptionNoiseMode() == FIXED_NOISE_DECRYPT);
    std::vector<uint64_t> qs;
    if (!put_params(pre, cc, qs))
        return false;
    const size_t numQ = qs.size();
    auto kp1 = cc->KeyGen();
    auto kp2 = cc->MultipartyKeyGen(kp1.publicKey);
    if (!put_key(pre + "s1", kp1.secretKey, numQ) || !put_key(pre + "s2", kp2.secretKey, numQ))
        return false;
    const auto vi = bfv_values(7);
    const auto vx = ckks_values(0.5);
    Plaintext in = ckks ? cc->MakeCKKSPackedPlaintext(vx) : cc->MakePackedPlaintext(vi);
    auto ct      = cc->Encrypt(kp2.publicKey, in);  // under the joint key
    if (!shaped(ct->GetElements(), 2, numQ))
        return false;
    auto lead = cc->MultipartyDecryptLead({ct}, kp1.secretKey);
    auto main = cc->MultipartyDecryptMain({ct}, kp2.secretKey);
    REQUIRE(lead.size() == 1 && main.size() == 1);
    if (!shaped(lead[0]->GetElements(), 1, numQ) || !shaped(main[0]->GetElements(), 1, numQ))
        return false;
    const std::vector<Ciphertext<DCRTPoly>> partials{lead[0], main[0]};
    Plaintext pt;
    cc->MultipartyDecryptFusion(partials, &pt);
    if (ckks) {
        if (!close_to(pt, vx, 1e-4))
            return false;
        Poly p;
        cc->GetScheme()->MultipartyDecryptFusion(partials, &p);
        REQUIRE(p.GetLength() == kRing && p.GetFormat() == Format::COEFFICIENT);
        put_u64(pre + "fusion", residues(p, qs, numQ));
    } else {
        pt->SetLength(vi.size());
        REQUIRE(pt->GetPackedValue() == vi);
        NativePoly m;
        cc->GetScheme()->MultipartyDecryptFusion(partials, &m);
        REQUIRE(m.GetLength() == kRing && m.GetModulus() == NativeInteger(kT));
        put_u64(pre + "fusion", words(m));
        const auto bfv = std::dynamic_pointer_cast<CryptoParametersBFVRNS>(cc->GetCryptoParameters());
        REQUIRE(bfv->GetMultiplicationTechnique() == HPS);
    }
    put_u64(pre + "c", words(ct->GetElements()));
    put_u64(pre + "lead", words(lead[0]->GetElements()));
    put_u64(pre + "main", words(main[0]->GetElements()));
    put_u64(pre + "meta", {kRing, numQ, ckks ? 0 : kT, ckks ? 9u : 1u, 1});
    printf("%s numQ = %zu\n", pre.c_str(), numQ);
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2)
        return 2;
    g_out = fopen(argv[1], "wb");
    if (!g_out)
        return 1;
    if (!bfv_set("hps_", HPSPOVERQLEVELED, 0, 1, true) || !bfv_set("hpsu_", HPS, 45, 0, true) || !bfv_set("behz_", BEHZ, 0, 1, false))
        return 1;
    if (!ckks_set("ckks_"))
        return 1;
    if (!threshold_set("tbfv_", false) || !threshold_set("tckks_", true))
        return 1;
    fclose(g_out);
    return 0;
}
