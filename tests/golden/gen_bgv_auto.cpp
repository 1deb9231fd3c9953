// TEST INFRASTRUCTURE — generator of tests/golden/ref_vectors_bgv_auto.npz (run by make_golden_bgv_auto.py).
// Links the reference's stock libraries (oracle/_ref), the way gen_bgv_decrypt.cpp does.  BGV on HYBRID keys (2 digits) at ring dimension 64,
// t = 65537, multiplicative depth 4, HEStd_NotSet, once under FLEXIBLEAUTO (prefix "fa_") and once under the default FLEXIBLEAUTOEXT ("fx_"):
// the level alignment of the automatic scaling modes, LeveledSHEBGVRNS::AdjustLevelsAndDepthInPlace and AdjustLevelsAndDepthToOneInPlace
// (bgvrns-leveledshe.cpp:83-233), on ciphertext pairs that reach every branch of the case table.
//
// Operands come from a pool: for k = 0 .. 3 (FLEXIBLEAUTOEXT: .. 4) a ciphertext of noise degree 1 and one of noise degree 2, k levels below a
// fresh one.  Degree 2 is cc->EvalMult of two degree-1 ciphertexts of that level; degree 1 one level further down is
// scheme->ModReduceInternalInPlace of such a product, which is what the next EvalMult of the reference does to it
// (AdjustLevelsAndDepthToOneInPlace).  cc->ModReduce itself is a no-op outside FIXEDMANUAL, so the pool cannot be built through it.
// What public calls cannot produce: under FLEXIBLEAUTOEXT a ciphertext of noise degree 1 at level 0 -- a fresh ciphertext there has degree 2
// and the Big scaling factor (cryptocontext.h:194-199, 441-444), and every degree-1 ciphertext is a ModReduce of something.  The pairs whose
// lower operand has degree 1 therefore start at level 1 in that context; every branch of the table is still reached.  (A ciphertext of noise
// degree 3 or more never reaches the table: every operation leaves degree 1 or 2.)
//
// Per context <p>:
//   <p>q, <p>psiQ, <p>p, <p>psiP      moduli and roots of Q and P
//   <p>mulB, <p>mulA                  the relinearisation key, [dnum][numQ + numP][ring]
//   <p>mrf, <p>big                    GetModReduceFactorInt(i) and GetScalingFactorIntBig(i), i < numQ
//   <p>pool<j>, <p>pool<j>_meta       pool ciphertext j = 2 * level + degree - 1: [2][sizeQl][ring]; level, noiseScaleDeg, sizeQl, scalingFactorInt
//   <p>cases                          per case: pool index of ct1, of ct2, branch id
// per case <p>c<n>, for which in {"adj" (AdjustLevelsAndDepthInPlace), "one" (AdjustLevelsAndDepthToOneInPlace)} and operand o in {1, 2}:
//   <p>c<n>_<which>_meta              level, noiseScaleDeg, sizeQl, scalingFactorInt of ct1 then of ct2, after the call
//   <p>c<n>_<which><o>                the operand after the call, [2][sizeQl][ring] -- present only when its words or row count changed
// whole operations on operands of different levels:
//   <p>add, <p>add_meta               cc->EvalAdd(pool[a], pool[b]): [2][sizeQl][ring]; a, b, level, noiseScaleDeg, sizeQl, scalingFactorInt
//   <p>mul, <p>mul_meta               cc->EvalMult(pool[a], pool[b]) (relinearised), likewise
// meta: ring, t, dnum.
// Branch ids: 10 * side + kind, side 0: ct1 is the lower level, 1: ct2, 2: equal levels.  kind, by (noise degree of the lower, of the higher):
//   0 (2,2) ModReduce            1 (2,2) ModReduce + LevelReduce     2 (2,1) gap 1: ModReduce alone
//   3 (2,1) ModReduce twice      4 (2,1) ModReduce, LevelReduce, ModReduce
//   5 (1,2) scalar + LevelReduce 6 (1,1) scalar + ModReduce          7 (1,1) scalar + LevelReduce + ModReduce
// equal levels: 20 nothing, 21 scalar on ct1, 22 scalar on ct2.  The generator FAILS unless all 19 ids were reached, every (degree, degree)
// combination was seen with level differences 1, 2 and 3, and the metadata after each call is what the label says.
// Record format: u32 name length, name, u32 type (0 = u64), u64 count, data.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
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
static void put_params(const std::string& q, const std::string& psi, const std::shared_ptr<DCRTPoly::Params>& p) {
    std::vector<uint64_t> qs, roots;
    for (const auto& l : p->GetParams()) {
        qs.push_back(l->GetModulus().ConvertToInt<uint64_t>());
        roots.push_back(l->GetRootOfUnity().ConvertToInt<uint64_t>());
    }
    put_u64(q, qs), put_u64(psi, roots);
}
static std::vector<uint64_t> meta_of(const Ciphertext<DCRTPoly>& c) {
    return {c->GetLevel(), c->GetNoiseScaleDeg(), c->GetElements()[0].GetNumOfElements(), c->GetScalingFactorInt().ConvertToInt<uint64_t>()};
}
#define REQUIRE(cond)                                                    \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "gen_bgv_auto: %s does not hold\n", #cond); \
            return false;                                                \
        }                                                                \
    } while (0)

static const uint32_t kRing = 64, kDnum = 2;
static const uint64_t kT = 65537;

static bool context(const std::string& p, ScalingTechnique st) {
    CCParams<CryptoContextBGVRNS> parameters;
    parameters.SetSecurityLevel(HEStd_NotSet);
    parameters.SetRingDim(kRing);
    parameters.SetPlaintextModulus(kT);
    parameters.SetMultiplicativeDepth(4);
    parameters.SetScalingTechnique(st);
    parameters.SetKeySwitchTechnique(HYBRID);
    parameters.SetNumLargeDigits(kDnum);
    auto cc = GenCryptoContext(parameters);
    cc->Enable(PKE);
    cc->Enable(KEYSWITCH);
    cc->Enable(LEVELEDSHE);
    const auto cp       = std::dynamic_pointer_cast<CryptoParametersBGVRNS>(cc->GetCryptoParameters());
    const uint32_t numQ = cp->GetElementParams()->GetParams().size(), numP = cp->GetParamsP()->GetParams().size();
    REQUIRE(cp->GetScalingTechnique() == st && cp->GetKeySwitchTechnique() == HYBRID && cp->GetNumPartQ() == kDnum);
    REQUIRE(cp->GetPlaintextModulus() == kT);
    auto kp = cc->KeyGen();
    cc->EvalMultKeyGen(kp.secretKey);
    const auto scheme = cc->GetScheme();
    std::mt19937_64 gen(st == FLEXIBLEAUTO ? 61 : 67);
    auto fresh = [&]() {
        std::vector<int64_t> v(kRing);
        for (auto& e : v)
            e = static_cast<int64_t>(gen() % 5) - 2;
        return cc->Encrypt(kp.publicKey, cc->MakePackedPlaintext(v));
    };
    // the pool: pool[2k] of noise degree 1, pool[2k+1] of noise degree 2, k levels below a fresh ciphertext.  Under FLEXIBLEAUTOEXT a fresh
    // ciphertext has noise degree 2 (cryptocontext.h:441-444) and pool[0] stays empty (see the head of the file)
    const bool ext         = st == FLEXIBLEAUTOEXT;
    const uint32_t nLevels = ext ? 5 : 4;
    std::vector<Ciphertext<DCRTPoly>> pool(2 * nLevels);
    auto x = fresh(), y = fresh();
    REQUIRE(x->GetLevel() == 0 && x->GetNoiseScaleDeg() == (ext ? 2u : 1u) && x->GetElements()[0].GetNumOfElements() == numQ && numQ >= nLevels + 1);
    for (uint32_t k = 0; k < nLevels; ++k) {
        Ciphertext<DCRTPoly> prod, prodY;
        if (ext && k == 0)
            prod = x, prodY = y;
        else {
            REQUIRE(x->GetLevel() == k && y->GetLevel() == k && x->GetNoiseScaleDeg() == 1 && y->GetNoiseScaleDeg() == 1);
            pool[2 * k] = x;
            prod = cc->EvalMult(x, y), prodY = k + 1 < nLevels ? cc->EvalMult(y, y) : prod;
        }
        REQUIRE(prod->GetLevel() == k && prod->GetNoiseScaleDeg() == 2 && prod->GetElements().size() == 2);
        pool[2 * k + 1] = prod;
        if (k + 1 == nLevels)
            break;
        auto nx = prod->Clone(), ny = prodY->Clone();
        scheme->ModReduceInternalInPlace(nx, 1), scheme->ModReduceInternalInPlace(ny, 1);
        x = nx, y = ny;
    }
    const auto mulKey = cc->GetEvalMultKeyVector(pool[1]->GetKeyTag())[0];
    REQUIRE(mulKey->GetBVector().size() == kDnum && mulKey->GetBVector()[0].GetNumOfElements() == numQ + numP);
    put_params(p + "q", p + "psiQ", cp->GetElementParams());
    put_params(p + "p", p + "psiP", cp->GetParamsP());
    put_u64(p + "mulB", words(mulKey->GetBVector())), put_u64(p + "mulA", words(mulKey->GetAVector()));
    std::vector<uint64_t> mrf, big;
    for (uint32_t i = 0; i < numQ; ++i) {
        mrf.push_back(cp->GetModReduceFactorInt(i).ConvertToInt<uint64_t>());
        big.push_back(cp->GetScalingFactorIntBig(i).ConvertToInt<uint64_t>());
    }
    put_u64(p + "mrf", mrf), put_u64(p + "big", big);
    for (size_t j = 0; j < pool.size(); ++j) {
        if (!pool[j])
            continue;
        for (const auto& e : pool[j]->GetElements())
            REQUIRE(e.GetFormat() == Format::EVALUATION);
        put_u64(p + "pool" + std::to_string(j), words(pool[j]->GetElements()));
        put_u64(p + "pool" + std::to_string(j) + "_meta", meta_of(pool[j]));
    }

    // the pairs: the lower operand at the first level the pool has for its degree, the higher one `gap` levels below it
    struct Pair {
        uint32_t a, b;
    };
    std::vector<Pair> pairs;
    auto idx = [](uint32_t level, uint32_t degree) { return 2 * level + (degree - 1); };
    for (uint32_t dlo = 1; dlo <= 2; ++dlo)
        for (uint32_t dhi = 1; dhi <= 2; ++dhi)
            for (uint32_t gap = 1; gap <= 3; ++gap) {
                const uint32_t lo = pool[idx(0, dlo)] ? 0 : 1;
                pairs.push_back({idx(lo, dlo), idx(lo + gap, dhi)});  // ct1 is the lower level: every gap
                if (gap != 2 || (dlo == 2 && dhi == 1))               // ct2 is: every branch of the table
                    pairs.push_back({idx(lo + gap, dhi), idx(lo, dlo)});
            }
    pairs.push_back({idx(1, 1), idx(1, 1)}), pairs.push_back({idx(1, 2), idx(1, 2)});
    pairs.push_back({idx(1, 1), idx(1, 2)}), pairs.push_back({idx(1, 2), idx(1, 1)});

    std::vector<uint64_t> cases;
    std::set<uint64_t> reached;
    std::set<std::vector<uint32_t>> gaps;
    for (size_t n = 0; n < pairs.size(); ++n) {
        const auto &c1 = pool[pairs[n].a], &c2 = pool[pairs[n].b];
        const uint32_t l1 = c1->GetLevel(), l2 = c2->GetLevel(), d1 = c1->GetNoiseScaleDeg(), d2 = c2->GetNoiseScaleDeg();
        const uint32_t gap = l1 < l2 ? l2 - l1 : l1 - l2, dlo = l1 < l2 ? d1 : d2, dhi = l1 < l2 ? d2 : d1;
        uint64_t id;
        if (l1 == l2)
            id = 20 + (d1 < d2 ? 1 : d2 < d1 ? 2 : 0);
        else {
            const uint64_t kind = dlo == 2 ? (dhi == 2 ? (gap > 1 ? 1 : 0) : (gap == 1 ? 2 : gap == 2 ? 3 : 4))
                                           : (dhi == 2 ? 5 : (gap > 1 ? 7 : 6));
            id = 10 * (l1 < l2 ? 0 : 1) + kind;
            gaps.insert({dlo, dhi, gap});
        }
        reached.insert(id);
        cases.insert(cases.end(), {pairs[n].a, pairs[n].b, id});
        const std::string name = p + "c" + std::to_string(n);
        for (int one = 0; one < 2; ++one) {
            auto a = c1->Clone(), b = c2->Clone();
            if (one)
                scheme->AdjustLevelsAndDepthToOneInPlace(a, b);
            else
                scheme->AdjustLevelsAndDepthInPlace(a, b);
            // what the label says: both end at the higher level with the degree of the higher operand (equal levels: the larger degree),
            // and AdjustLevelsAndDepthToOneInPlace takes a pair of degree 2 one level further down
            const uint32_t deg = l1 == l2 ? std::max(d1, d2) : dhi;
            REQUIRE(a->GetLevel() == b->GetLevel() && a->GetElements()[0].GetNumOfElements() == b->GetElements()[0].GetNumOfElements());
            REQUIRE(a->GetNoiseScaleDeg() == b->GetNoiseScaleDeg() && a->GetNoiseScaleDeg() == (one ? 1u : deg));
            REQUIRE(a->GetLevel() == std::max(l1, l2) + (one && deg == 2 ? 1u : 0u));
            REQUIRE(a->GetScalingFactorInt() == b->GetScalingFactorInt() || l1 == l2);
            const std::string which = one ? "_one" : "_adj";
            auto m = meta_of(a);
            const auto mb = meta_of(b);
            m.insert(m.end(), mb.begin(), mb.end());
            put_u64(name + which + "_meta", m);
            if (words(a->GetElements()) != words(c1->GetElements()))
                put_u64(name + which + "1", words(a->GetElements()));
            if (words(b->GetElements()) != words(c2->GetElements()))
                put_u64(name + which + "2", words(b->GetElements()));
        }
        printf("%s: (%u,%u) x (%u,%u) -> branch %llu\n", name.c_str(), l1, d1, l2, d2, (unsigned long long)id);
    }
    put_u64(p + "cases", cases);
    const std::set<uint64_t> all = {0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 12, 13, 14, 15, 16, 17, 20, 21, 22};
    REQUIRE(reached == all);
    REQUIRE(gaps.size() == 12);  // 2 x 2 degree combinations x level differences 1, 2, 3

    // whole operations on operands of different levels (and degrees)
    {
        const uint32_t a = idx(0, 2), b = idx(2, 1);
        auto s = cc->EvalAdd(pool[a], pool[b]);
        REQUIRE(s->GetElements().size() == 2 && s->GetLevel() == pool[b]->GetLevel());
        auto ms = meta_of(s);
        ms.insert(ms.begin(), {a, b});
        put_u64(p + "add", words(s->GetElements())), put_u64(p + "add_meta", ms);
        const uint32_t c = idx(1, 1), d = idx(2, 2);
        auto m = cc->EvalMult(pool[c], pool[d]);
        REQUIRE(m->GetElements().size() == 2 && m->GetLevel() == pool[d]->GetLevel() + 1 && m->GetNoiseScaleDeg() == 2);
        auto mm = meta_of(m);
        mm.insert(mm.begin(), {c, d});
        put_u64(p + "mul", words(m->GetElements())), put_u64(p + "mul_meta", mm);
    }
    printf("%s: numQ = %u, numP = %u, %zu pool ciphertexts, %zu cases\n", p.c_str(), numQ, numP, pool.size(), pairs.size());
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2)
        return 2;
    g_out = fopen(argv[1], "wb");
    if (!g_out)
        return 1;
    if (!context("fa_", FLEXIBLEAUTO) || !context("fx_", FLEXIBLEAUTOEXT))
        return 1;
    put_u64("meta", {kRing, kT, kDnum});
    fclose(g_out);
    return 0;
}
