// TEST INFRASTRUCTURE — generator of tests/golden/ref_vectors_bv.npz (run by make_golden_bv.py).
// Links the reference's stock libraries (oracle/_ref), the way gen_hps_leveled.cpp does.  BV key switching (KeySwitchBV,
// keyswitch-bv.cpp) through the reference's scheme layer at ring dimension 64, digit sizes r = 0 and r = 10:
//   bfv<r>_*   BFV, multiplicative depth 4 (3 limbs of 60 bits), the default multiplication technique (HPSPOVERQLEVELED): two fresh
//              ciphertexts, the evaluation key's b and a vectors, cc->EvalMultNoRelin, KeySwitchCore of its third element in EVALUATION
//              format, and cc->EvalMult;
//   ckks<r>_*  CKKS, depth 2, FIXEDMANUAL (limbs of 60, 50, 51 bits: the window counts differ per limb): the key, the third element of
//              an EvalMultNoRelin after one EvalMult + Rescale (2 of 3 limbs) and its KeySwitchCore.
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
static void append(std::vector<uint64_t>& o, const DCRTPoly& e) {
    for (size_t i = 0; i < e.GetNumOfElements(); ++i)
        for (size_t k = 0; k < e.GetRingDimension(); ++k)
            o.push_back(e.GetElementAtIndex(i)[k].ConvertToInt<uint64_t>());
}
static void put_polys(const std::string& name, const std::vector<DCRTPoly>& v) {
    std::vector<uint64_t> o;
    for (const auto& e : v)
        append(o, e);
    put_u64(name, o);
}
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

static int bfv_case(uint32_t r) {
    const uint32_t ring = 64;
    const uint64_t t    = 65537;
    const std::string pre = "bfv" + std::to_string(r) + "_";
    CCParams<CryptoContextBFVRNS> parameters;
    parameters.SetSecurityLevel(HEStd_NotSet);
    parameters.SetRingDim(ring);
    parameters.SetPlaintextModulus(t);
    parameters.SetMultiplicativeDepth(4);
    parameters.SetScalingModSize(60);
    parameters.SetKeySwitchTechnique(BV);
    parameters.SetDigitSize(r);
    auto cc = GenCryptoContext(parameters);
    cc->Enable(PKE);
    cc->Enable(KEYSWITCH);
    cc->Enable(LEVELEDSHE);
    auto kp = cc->KeyGen();
    cc->EvalMultKeyGen(kp.secretKey);
    std::mt19937_64 gen(11 + r);
    auto fresh = [&]() {
        std::vector<int64_t> v(ring);
        for (auto& e : v)
            e = static_cast<int64_t>(gen() % 5) - 2;
        return cc->Encrypt(kp.publicKey, cc->MakePackedPlaintext(v));
    };
    const auto cp       = std::dynamic_pointer_cast<CryptoParametersBFVRNS>(cc->GetCryptoParameters());
    const uint32_t numQ = cp->GetElementParams()->GetParams().size();
    if (cp->GetMultiplicationTechnique() != HPSPOVERQLEVELED || cp->GetDigitSize() != r)
        return 1;
    auto a = fresh(), b = fresh();
    const uint32_t dcrtBit = a->GetElements()[0].GetElementAtIndex(0).GetModulus().GetMSB();
    const uint32_t dropped = FindLevelsToDrop(std::max(a->GetNoiseScaleDeg(), b->GetNoiseScaleDeg()) - 1, cc->GetCryptoParameters(), dcrtBit, false);
    if (dropped >= numQ || !all_format(a->GetElements(), Format::EVALUATION) || !all_format(b->GetElements(), Format::EVALUATION))
        return 1;
    const auto key = cc->GetEvalMultKeyVector(a->GetKeyTag())[0];
    auto d         = cc->EvalMultNoRelin(a, b);
    if (d->GetElements().size() != 3 || !all_format(d->GetElements(), Format::COEFFICIENT))
        return 1;
    DCRTPoly e2 = d->GetElements()[2];
    e2.SetFormat(Format::EVALUATION);
    const auto ks = cc->GetScheme()->KeySwitchCore(e2, key);
    auto m        = cc->EvalMult(a, b);
    if (m->GetElements().size() != 2 || !all_format(m->GetElements(), Format::EVALUATION) || !all_format(*ks, Format::EVALUATION) ||
        !all_format(key->GetBVector(), Format::EVALUATION) || key->GetBVector()[0].GetNumOfElements() != numQ)
        return 1;
    put_u64(pre + "meta", {ring, t, numQ, numQ - dropped, r, key->GetBVector().size()});
    put_params(pre, cp->GetElementParams());
    put_params(pre + "r_", cp->GetParamsRl(numQ - 1));
    put_polys(pre + "a", a->GetElements()), put_polys(pre + "b", b->GetElements());
    put_polys(pre + "keyB", key->GetBVector()), put_polys(pre + "keyA", key->GetAVector());
    put_polys(pre + "d", d->GetElements()), put_polys(pre + "ks", *ks), put_polys(pre + "m", m->GetElements());
    printf("BFV  r = %2u: numQ = %u, levels dropped = %u, digits = %zu\n", r, numQ, dropped, key->GetBVector().size());
    return 0;
}

static int ckks_case(uint32_t r) {
    const uint32_t ring = 64;
    const std::string pre = "ckks" + std::to_string(r) + "_";
    CCParams<CryptoContextCKKSRNS> parameters;
    parameters.SetSecurityLevel(HEStd_NotSet);
    parameters.SetRingDim(ring);
    parameters.SetMultiplicativeDepth(2);
    parameters.SetScalingModSize(50);
    parameters.SetFirstModSize(60);
    parameters.SetScalingTechnique(FIXEDMANUAL);
    parameters.SetKeySwitchTechnique(BV);
    parameters.SetDigitSize(r);
    auto cc = GenCryptoContext(parameters);
    cc->Enable(PKE);
    cc->Enable(KEYSWITCH);
    cc->Enable(LEVELEDSHE);
    auto kp = cc->KeyGen();
    cc->EvalMultKeyGen(kp.secretKey);
    std::mt19937_64 gen(23 + r);
    auto fresh = [&]() {
        std::vector<double> v(ring / 2);
        for (auto& e : v)
            e = static_cast<double>(gen() % 1000) / 500.0 - 1.0;
        return cc->Encrypt(kp.publicKey, cc->MakeCKKSPackedPlaintext(v));
    };
    const auto cp        = std::dynamic_pointer_cast<CryptoParametersRNS>(cc->GetCryptoParameters());
    const uint32_t sizeQ = cp->GetElementParams()->GetParams().size();
    auto x = fresh(), y = fresh();
    auto a = cc->Rescale(cc->EvalMult(x, y));
    auto b = cc->Rescale(cc->EvalMult(y, y));
    auto d = cc->EvalMultNoRelin(a, b);
    const auto key = cc->GetEvalMultKeyVector(a->GetKeyTag())[0];
    if (d->GetElements().size() != 3 || !all_format(d->GetElements(), Format::EVALUATION) || cp->GetDigitSize() != r ||
        key->GetBVector()[0].GetNumOfElements() != sizeQ)
        return 1;
    const DCRTPoly& e2    = d->GetElements()[2];
    const uint32_t sizeQl = e2.GetNumOfElements();
    if (sizeQl + 1 != sizeQ)
        return 1;
    const auto ks = cc->GetScheme()->KeySwitchCore(e2, key);
    if (!all_format(*ks, Format::EVALUATION) || (*ks)[0].GetNumOfElements() != sizeQl)
        return 1;
    put_u64(pre + "meta", {ring, 0, sizeQ, sizeQl, r, key->GetBVector().size()});
    put_params(pre, cp->GetElementParams());
    put_polys(pre + "keyB", key->GetBVector()), put_polys(pre + "keyA", key->GetAVector());
    put_polys(pre + "c", {e2}), put_polys(pre + "ks", *ks);
    printf("CKKS r = %2u: sizeQ = %u, sizeQl = %u, digits = %zu\n", r, sizeQ, sizeQl, key->GetBVector().size());
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2)
        return 2;
    g_out = fopen(argv[1], "wb");
    if (!g_out)
        return 1;
    int rc = 0;
    for (uint32_t r : {0u, 10u})
        rc |= bfv_case(r) | ckks_case(r);
    fclose(g_out);
    return rc;
}
