// TEST INFRASTRUCTURE — generator of the dropped-level case of tests/golden/ref_vectors_hps.npz (run by make_golden_hps.py).
// Links the reference's stock libraries (oracle/_ref), the way tests/hal/Makefile links shim_ckks.  In an HPSPOVERQLEVELED context a
// chain of cc->EvalMult is deepened until LeveledSHEBFVRNS::EvalMult drops at least one level for the next product
// (bfvrns-leveledshe.cpp:263-272; FindLevelsToDrop has external linkage and is called here with the same arguments to record the
// level).  Dumps: moduli, the two operands, sizeQl, the EvalMultNoRelin product and the reference's own tables of every level through
// the CryptoParametersBFVRNS getters, flattened row-major in the layout of fhe_hps_table.
// Record format: u32 name length, name, u32 type (0 = u64, 1 = double), u64 count, data.
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
static void put(const std::string& name, uint32_t type, const void* data, uint64_t count) {
    uint32_t n = name.size();
    fwrite(&n, 4, 1, g_out);
    fwrite(name.data(), 1, n, g_out);
    fwrite(&type, 4, 1, g_out);
    fwrite(&count, 8, 1, g_out);
    fwrite(data, 8, count, g_out);
}
static void put_u64(const std::string& name, const std::vector<uint64_t>& v) { put(name, 0, v.data(), v.size()); }
static void put_f64(const std::string& name, const std::vector<double>& v) { put(name, 1, v.data(), v.size()); }
static std::vector<uint64_t> vec(const std::vector<NativeInteger>& v, size_t n) {
    std::vector<uint64_t> o;
    for (size_t i = 0; i < n; ++i)
        o.push_back(v[i].ConvertToInt<uint64_t>());
    return o;
}
// m[a][b] for a < na, b < nb, row-major; transposed: m[b][a]
static std::vector<uint64_t> mat(const std::vector<std::vector<NativeInteger>>& m, size_t na, size_t nb, bool transposed) {
    std::vector<uint64_t> o;
    for (size_t a = 0; a < na; ++a)
        for (size_t b = 0; b < nb; ++b)
            o.push_back((transposed ? m[b][a] : m[a][b]).ConvertToInt<uint64_t>());
    return o;
}
static void put_ct(const std::string& name, ConstCiphertext<DCRTPoly> ct) {
    std::vector<uint64_t> o;
    for (const auto& e : ct->GetElements())
        for (size_t i = 0; i < e.GetNumOfElements(); ++i)
            for (size_t k = 0; k < e.GetRingDimension(); ++k)
                o.push_back(e.GetElementAtIndex(i)[k].ConvertToInt<uint64_t>());
    put_u64(name, o);
}

int main(int argc, char** argv) {
    if (argc < 2)
        return 2;
    const uint32_t ring = 1024, bits = 30;
    const uint64_t t = 65537;
    CCParams<CryptoContextBFVRNS> parameters;
    parameters.SetSecurityLevel(HEStd_NotSet);
    parameters.SetRingDim(ring);
    parameters.SetPlaintextModulus(t);
    parameters.SetMultiplicativeDepth(6);
    parameters.SetScalingModSize(bits);
    parameters.SetMultiplicationTechnique(HPSPOVERQLEVELED);
    auto cc = GenCryptoContext(parameters);
    cc->Enable(PKE);
    cc->Enable(KEYSWITCH);
    cc->Enable(LEVELEDSHE);
    auto kp = cc->KeyGen();
    cc->EvalMultKeyGen(kp.secretKey);
    std::mt19937_64 gen(7);
    auto fresh = [&]() {
        std::vector<int64_t> v(ring);
        for (auto& e : v)
            e = static_cast<int64_t>(gen() % 5) - 2;
        return cc->Encrypt(kp.publicKey, cc->MakePackedPlaintext(v));
    };
    const auto cp = std::dynamic_pointer_cast<CryptoParametersBFVRNS>(cc->GetCryptoParameters());
    const uint32_t numQ = cp->GetElementParams()->GetParams().size();
    // deepen a chain of EvalMult (with relinearisation: 2-element ciphertexts) until the next product drops a level
    Ciphertext<DCRTPoly> a = fresh(), b = fresh();
    uint32_t dropped = 0;
    for (int depth = 0; depth < 8; ++depth) {
        const uint32_t levels  = std::max(a->GetNoiseScaleDeg(), b->GetNoiseScaleDeg()) - 1;
        const uint32_t dcrtBit = a->GetElements()[0].GetElementAtIndex(0).GetModulus().GetMSB();
        dropped                = FindLevelsToDrop(levels, cc->GetCryptoParameters(), dcrtBit, false);
        if (dropped > 0)
            break;
        a = cc->EvalMult(a, b);
        b = cc->EvalMult(b, fresh());
    }
    if (dropped == 0 || dropped >= numQ) {
        fprintf(stderr, "no usable level drop observed (dropped = %u, numQ = %u)\n", dropped, numQ);
        return 1;
    }
    if (a->GetElements()[0].GetNumOfElements() != numQ || a->GetElements()[0].GetFormat() != Format::EVALUATION ||
        b->GetElements()[0].GetFormat() != Format::EVALUATION || a->GetElements().size() != 2 || b->GetElements().size() != 2) {
        fprintf(stderr, "operands are not 2-element EVALUATION ciphertexts over all of Q\n");
        return 1;
    }
    auto d = cc->EvalMultNoRelin(a, b);
    if (d->GetElements()[0].GetFormat() != Format::COEFFICIENT || d->GetElements().size() != 3)
        return 1;
    g_out = fopen(argv[1], "wb");
    if (!g_out)
        return 1;
    const uint32_t sizeQl = numQ - dropped;
    put_u64("meta", {ring, t, numQ, sizeQl, a->GetNoiseScaleDeg(), b->GetNoiseScaleDeg()});
    std::vector<uint64_t> q, psiQ, r, psiR;
    for (const auto& p : cp->GetElementParams()->GetParams()) {
        q.push_back(p->GetModulus().ConvertToInt<uint64_t>());
        psiQ.push_back(p->GetRootOfUnity().ConvertToInt<uint64_t>());
    }
    for (const auto& p : cp->GetParamsRl(numQ - 1)->GetParams()) {
        r.push_back(p->GetModulus().ConvertToInt<uint64_t>());
        psiR.push_back(p->GetRootOfUnity().ConvertToInt<uint64_t>());
    }
    put_u64("q", q), put_u64("psiQ", psiQ), put_u64("r", r), put_u64("psiR", psiR);
    put_ct("a", a), put_ct("b", b), put_ct("d", d);
    const size_t nQ = numQ, nR = r.size();
    put_f64("tab_qInv_0", cp->GetqInv());
    put_f64("tab_rInv_0", cp->GetrInv());
    put_u64("tab_qInvModr_0", mat(cp->GetqInvModr(), nQ, nR, false));
    put_u64("tab_tRSHatInvModsDivsModr_0", mat(cp->GettRSHatInvModsDivsModr(), nR, nQ + 1, false));
    put_f64("tab_tRSHatInvModsDivsFrac_0", cp->GettRSHatInvModsDivsFrac());
    for (uint32_t l = 0; l < numQ; ++l) {
        const size_t L = l + 1;
        const std::string s = "_" + std::to_string(l);
        put_u64("tab_QlHatInvModq" + s, vec(cp->GetQlHatInvModq(l), L));
        put_u64("tab_QlHatModr" + s, mat(cp->GetQlHatModr(l), L, L, true));          // reference [j][i] -> [i][j], j over R_l
        put_u64("tab_alphaQlModr" + s, mat(cp->GetalphaQlModr(l), L + 1, L, false));  // [a][j], j over R_l
        put_u64("tab_RlHatInvModr" + s, vec(cp->GetRlHatInvModr(l), L));
        put_u64("tab_RlHatModq" + s, mat(cp->GetRlHatModq(l), L, L, true));          // reference [i][j] -> [j][i]
        put_u64("tab_alphaRlModq" + s, mat(cp->GetalphaRlModq(l), L + 1, L, false));  // [a][i], i over Q_l
        put_u64("tab_tQlSlHatInvModsDivsModq" + s, mat(cp->GettQlSlHatInvModsDivsModq(l), L, L + 1, false));
        put_f64("tab_tQlSlHatInvModsDivsFrac" + s, cp->GettQlSlHatInvModsDivsFrac(l));
        put_u64("tab_negRlQHatInvModq" + s, vec(cp->GetmNegRlQHatInvModq(l), nQ));
        put_u64("tab_negRlQlHatInvModq" + s, vec(cp->GetmNegRlQlHatInvModq(l), L));
        put_u64("tab_QlQHatInvModqDivqModq" + s, mat(cp->GetQlQHatInvModqDivqModq(l), L, nQ - L + 1, false));
        if (L < nQ)
            put_f64("tab_QlQHatInvModqDivqFrac" + s, cp->GetQlQHatInvModqDivqFrac(l));
        put_u64("tab_QlHatModq" + s, vec(cp->GetQlHatModq(l), L));
    }
    fclose(g_out);
    printf("numQ = %u, levels dropped = %u, sizeQl = %u, noiseScaleDeg = (%u, %u)\n", numQ, dropped, sizeQl,
           (unsigned)a->GetNoiseScaleDeg(), (unsigned)b->GetNoiseScaleDeg());
    return 0;
}
