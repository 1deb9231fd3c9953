// dcrtpoly_hip.h — header-only C++ host side over the C ABI (include/fhe_hip.h).
//
// Mirrors the part of the reference class surface that lies on the hot path, with the reference's names,
// argument meaning and error behaviour (errors are thrown as exceptions carrying the library's message, the way
// OPENFHE_THROW does in src/core/include/utils/exception.h):
//   lbcrypto::DCRTPolyImpl  (src/core/include/lattice/hal/default/dcrtpoly.h:59-398, dcrtpoly-impl.h)
//   ILDCRTParams             (src/core/include/lattice/hal/default/ildcrtparams.h:70-372)
//   KeySwitchHYBRID          (src/pke/lib/keyswitch/keyswitch-hybrid.cpp:308-435)
// A tower object owns ONE device allocation uint64_t[batch][limbs][N]; `batch` > 1 is the extension over the
// reference (a DCRTPoly is batch == 1): every method applies to all towers of the batch in one launch.
// This header is a convenience binding for stand-alone C++ programs that want the BATCHED composites (tests/hal_smoke.cpp,
// tests/hal_parity.cpp).  It is NOT what the drop-in backend uses: lbcrypto::DCRTPolyHipImpl (lattice/hal/hip/dcrtpoly-hip.h)
// binds the C ABI itself through hip-runtime.cpp.
#ifndef FHE_HAL_DCRTPOLY_HIP_H
#define FHE_HAL_DCRTPOLY_HIP_H
#include <cstdint>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/fhe_hip.h"

namespace fhehip {

enum Format { EVALUATION = 0, COEFFICIENT = 1 };  // lbcrypto::Format, utils/inttypes.h:65

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};
inline void check(fhe_status s) {
    if (s != FHE_OK)
        throw Error(std::string(fhe_last_error()));
}

// ILDCRTParams + device twiddle tables (shared, immutable)
class Params {
public:
    // ILDCRTParams(corder, moduli, rootsOfUnity)  ildcrtparams.h:130-145
    Params(uint32_t cyclotomicOrder, const std::vector<uint64_t>& moduli, const std::vector<uint64_t>& roots, int device = 0)
        : m_moduli(moduli), m_roots(roots) {
        if (moduli.size() != roots.size())
            throw Error("sizes of moduli and roots of unity do not match 1");
        uint32_t logN = 0;
        while ((2u << logN) < cyclotomicOrder)
            ++logN;
        check(fhe_ctx_create(logN, (uint32_t)moduli.size(), moduli.data(), roots.data(), device, &m_ctx));
    }
    // ILDCRTParams(corder, depth, bits)  ildcrtparams.h:100-117
    static std::shared_ptr<Params> Generate(uint32_t cyclotomicOrder, uint32_t depth, uint32_t bits, int device = 0) {
        std::vector<uint64_t> q(depth), psi(depth);
        check(fhe_param_dcrt_chain(cyclotomicOrder, depth, bits, q.data(), psi.data()));
        return std::make_shared<Params>(cyclotomicOrder, q, psi, device);
    }
    ~Params() { fhe_ctx_destroy(m_ctx); }
    Params(const Params&)            = delete;
    Params& operator=(const Params&) = delete;
    uint32_t GetRingDimension() const { return 1u << fhe_ctx_logn(m_ctx); }
    uint32_t GetCyclotomicOrder() const { return 2u << fhe_ctx_logn(m_ctx); }
    const std::vector<uint64_t>& GetModuli() const { return m_moduli; }
    const std::vector<uint64_t>& GetRoots() const { return m_roots; }
    fhe_ctx* ctx() const { return m_ctx; }

private:
    fhe_ctx* m_ctx = nullptr;
    std::vector<uint64_t> m_moduli, m_roots;
};

class DCRTPolyHip {
public:
    // towers over the context limbs limbIdx (empty = limbs [0, nLimbs))
    DCRTPolyHip(std::shared_ptr<Params> params, uint32_t nLimbs, Format format, uint32_t batch = 1,
                std::vector<uint32_t> limbIdx = {})
        : m_params(std::move(params)), m_limbs(nLimbs), m_batch(batch), m_format(format), m_idx(std::move(limbIdx)) {
        if (!m_idx.empty() && m_idx.size() != nLimbs)
            throw Error("limb index list does not match the number of towers");
        void* p = nullptr;
        check(fhe_malloc(m_params->ctx(), bytes(), &p));
        m_data = static_cast<uint64_t*>(p);
    }
    ~DCRTPolyHip() {
        if (m_data)
            fhe_free(m_params->ctx(), m_data);
    }
    DCRTPolyHip(DCRTPolyHip&& o) noexcept { *this = std::move(o); }
    DCRTPolyHip& operator=(DCRTPolyHip&& o) noexcept {
        if (this != &o) {
            if (m_data)
                fhe_free(m_params->ctx(), m_data);
            m_params = std::move(o.m_params);
            m_limbs = o.m_limbs, m_batch = o.m_batch, m_format = o.m_format, m_idx = std::move(o.m_idx);
            m_data   = o.m_data;
            o.m_data = nullptr;
        }
        return *this;
    }
    DCRTPolyHip(const DCRTPolyHip& o) : DCRTPolyHip(o.m_params, o.m_limbs, o.m_format, o.m_batch, o.m_idx) {
        check(fhe_memcpy_d2d(m_params->ctx(), m_data, o.m_data, bytes(), nullptr));
    }

    // host <-> device (SetValues / GetValues of the limbs, poly.h:166-195)
    void SetValues(const std::vector<uint64_t>& host, Format format) {
        if (host.size() != words())
            throw Error("SetValues: size mismatch");
        check(fhe_memcpy_h2d(m_params->ctx(), m_data, host.data(), bytes(), nullptr));
        check(fhe_stream_sync(m_params->ctx(), nullptr));
        m_format = format;
    }
    std::vector<uint64_t> GetValues() const {
        std::vector<uint64_t> h(words());
        check(fhe_memcpy_d2h(m_params->ctx(), h.data(), m_data, bytes(), nullptr));
        check(fhe_stream_sync(m_params->ctx(), nullptr));
        return h;
    }

    Format GetFormat() const { return m_format; }
    uint32_t GetNumOfElements() const { return m_limbs; }
    uint32_t GetRingDimension() const { return m_params->GetRingDimension(); }
    uint32_t GetBatch() const { return m_batch; }
    const std::shared_ptr<Params>& GetParams() const { return m_params; }
    uint64_t* data() { return m_data; }
    const uint64_t* data() const { return m_data; }

    // DCRTPolyImpl::SwitchFormat (dcrtpoly-impl.h:1932-1940), SetFormat (ilelement.h:447-450)
    void SwitchFormat(void* stream = nullptr) {
        if (m_format == COEFFICIENT)
            check(fhe_ntt_fwd(m_params->ctx(), m_data, idx(), m_limbs, m_batch, stream));
        else
            check(fhe_ntt_inv(m_params->ctx(), m_data, idx(), m_limbs, m_batch, stream));
        m_format = m_format == COEFFICIENT ? EVALUATION : COEFFICIENT;
    }
    void SetFormat(Format f, void* stream = nullptr) {
        if (f != m_format)
            SwitchFormat(stream);
    }

    // Plus / Minus / Times and the in-place operators (dcrtpoly.h:131-189, dcrtpoly-impl.h:362-408)
    DCRTPolyHip Plus(const DCRTPolyHip& r) const { return bin(fhe_add, r); }
    DCRTPolyHip Minus(const DCRTPolyHip& r) const { return bin(fhe_sub, r); }
    DCRTPolyHip Times(const DCRTPolyHip& r) const { return bin(fhe_mul, r); }
    DCRTPolyHip& operator+=(const DCRTPolyHip& r) { return binEq(fhe_add, r); }
    DCRTPolyHip& operator-=(const DCRTPolyHip& r) { return binEq(fhe_sub, r); }
    DCRTPolyHip& operator*=(const DCRTPolyHip& r) { return binEq(fhe_mul, r); }
    // Times(const std::vector<NativeInteger>&)  dcrtpoly-impl.h:582-601
    DCRTPolyHip Times(const std::vector<uint64_t>& perLimb) const {
        if (perLimb.size() != m_limbs)
            throw Error("tower size mismatch; cannot multiply");
        DCRTPolyHip out(m_params, m_limbs, m_format, m_batch, m_idx);
        check(fhe_mul_const(m_params->ctx(), out.m_data, m_data, perLimb.data(), idx(), m_limbs, m_batch, nullptr));
        return out;
    }
    DCRTPolyHip Negate() const {  // dcrtpoly-impl.h:347-354
        DCRTPolyHip out(m_params, m_limbs, m_format, m_batch, m_idx);
        check(fhe_neg(m_params->ctx(), out.m_data, m_data, idx(), m_limbs, m_batch, nullptr));
        return out;
    }
    // AutomorphismTransform(k)  dcrtpoly-impl.h:314-333 ("Automorphism index not odd" is thrown for even k)
    DCRTPolyHip AutomorphismTransform(uint32_t k) const {
        DCRTPolyHip out(m_params, m_limbs, m_format, m_batch, m_idx);
        check(fhe_automorph(m_params->ctx(), out.m_data, m_data, k, m_format == EVALUATION, idx(), m_limbs, m_batch, nullptr));
        return out;
    }
    // DropLastElementAndScale (CKKS rescale)  dcrtpoly-impl.h:693-712; tower must use context limbs [0, limbs)
    void DropLastElementAndScale() {
        if (!m_idx.empty())
            throw Error("DropLastElementAndScale: tower must use the leading context limbs");
        if (m_format != EVALUATION)
            throw Error("DropLastElementAndScale: EVALUATION format expected");
        DCRTPolyHip out(m_params, m_limbs - 1, m_format, m_batch);
        size_t wsb = fhe_rescale_workspace_bytes(m_params->ctx(), m_limbs, m_batch);
        void* ws   = nullptr;
        check(fhe_malloc(m_params->ctx(), wsb, &ws));
        fhe_status s = fhe_rescale(m_params->ctx(), m_data, m_limbs, m_batch, out.m_data, ws, wsb, nullptr);
        fhe_stream_sync(m_params->ctx(), nullptr);
        fhe_free(m_params->ctx(), ws);
        check(s);
        *this = std::move(out);
    }
    // DropLastElementAndScale `levels` times in one fused pass: what LeveledSHECKKSRNS::ModReduceInternalInPlace(ct, levels)
    // (ckksrns-leveledshe.cpp:172-191) does to an element, levels = compositeDegree under composite scaling.  scale: empty, or one residue per
    // limb the tower is multiplied by first (EvalMultCoreInPlace's integer); nOut: 0 = every remaining limb, else the leading nOut of them
    // (the LevelReduceInternalInPlace that follows in AdjustLevelsAndDepthInPlace).  fhe_rescale_multi
    void DropLastElementsAndScale(uint32_t levels, const std::vector<uint64_t>& scale = {}, uint32_t nOut = 0) {
        if (!m_idx.empty())
            throw Error("DropLastElementsAndScale: tower must use the leading context limbs");
        if (m_format != EVALUATION)
            throw Error("DropLastElementsAndScale: EVALUATION format expected");
        if (levels < 1 || levels >= m_limbs)
            throw Error("DropLastElementsAndScale: levels must be in [1, limbs)");
        if (!scale.empty() && scale.size() < m_limbs)
            throw Error("DropLastElementsAndScale: one scale residue per limb expected");
        if (nOut == 0)
            nOut = m_limbs - levels;
        if (nOut > m_limbs - levels)
            throw Error("DropLastElementsAndScale: nOut exceeds the remaining limbs");
        DCRTPolyHip out(m_params, nOut, m_format, m_batch);
        size_t wsb = fhe_rescale_multi_workspace_bytes(m_params->ctx(), m_limbs, levels, m_batch);
        void* ws   = nullptr;
        check(fhe_malloc(m_params->ctx(), wsb, &ws));
        fhe_status s = fhe_rescale_multi(m_params->ctx(), m_data, m_limbs, levels, nOut, scale.empty() ? nullptr : scale.data(), m_batch,
                                         out.m_data, ws, wsb, nullptr);
        fhe_stream_sync(m_params->ctx(), nullptr);
        fhe_free(m_params->ctx(), ws);
        check(s);
        *this = std::move(out);
    }
    // ModReduce (BGV modulus switch by the last limb, plaintext modulus t)  dcrtpoly-impl.h:736-755
    void ModReduce(uint64_t t) {
        if (!m_idx.empty())
            throw Error("ModReduce: tower must use the leading context limbs");
        DCRTPolyHip out(m_params, m_limbs - 1, m_format, m_batch);
        size_t wsb = fhe_rescale_workspace_bytes(m_params->ctx(), m_limbs, m_batch);
        void* ws   = nullptr;
        check(fhe_malloc(m_params->ctx(), wsb, &ws));
        fhe_status s = fhe_mod_reduce(m_params->ctx(), m_data, m_limbs, t, m_format == EVALUATION, m_batch, out.m_data, ws, wsb, nullptr);
        fhe_stream_sync(m_params->ctx(), nullptr);
        fhe_free(m_params->ctx(), ws);
        check(s);
        *this = std::move(out);
    }
    // ... over any limbs of the context with the caller's tables, as DCRTPoly::ModReduce receives them (dcrtpoly-impl.h:736-738):
    // negtInvModq = -t^-1 mod q_l, qlInvModq[i] = q_l^-1 mod q_i for the limbs that stay (fhe_mod_reduce_limbs)
    void ModReduce(uint64_t t, uint64_t negtInvModq, const std::vector<uint64_t>& qlInvModq) {
        if (qlInvModq.size() + 1 < m_limbs)
            throw Error("ModReduce: one qlInvModq entry per remaining limb expected");
        std::vector<uint32_t> kept(m_idx.begin(), m_idx.empty() ? m_idx.end() : m_idx.end() - 1);
        DCRTPolyHip out(m_params, m_limbs - 1, m_format, m_batch, kept);
        size_t wsb = fhe_rescale_workspace_bytes(m_params->ctx(), m_limbs, m_batch);
        void* ws   = nullptr;
        check(fhe_malloc(m_params->ctx(), wsb, &ws));
        fhe_status s = fhe_mod_reduce_limbs(m_params->ctx(), m_data, idx(), m_limbs, t, negtInvModq, qlInvModq.data(), m_format == EVALUATION,
                                            m_batch, out.m_data, ws, wsb, nullptr);
        fhe_stream_sync(m_params->ctx(), nullptr);
        fhe_free(m_params->ctx(), ws);
        check(s);
        *this = std::move(out);
    }
    // ... of the two elements of one ciphertext (batch 1 each, allocated on their own) in the same launches
    // (LeveledSHEBGVRNS::ModReduceInternalInPlace, bgvrns-leveledshe.cpp:44-75; fhe_mod_reduce_limbs_pair)
    static void ModReducePair(DCRTPolyHip& x0, DCRTPolyHip& x1, uint64_t t, uint64_t negtInvModq, const std::vector<uint64_t>& qlInvModq) {
        if (x0.m_batch != 1 || x1.m_batch != 1 || x0.m_limbs != x1.m_limbs || x0.m_format != x1.m_format || x0.m_idx != x1.m_idx)
            throw Error("ModReducePair: two single towers over the same limbs in the same format expected");
        if (qlInvModq.size() + 1 < x0.m_limbs)
            throw Error("ModReduce: one qlInvModq entry per remaining limb expected");
        const auto& P = x0.m_params;
        std::vector<uint32_t> kept(x0.m_idx.begin(), x0.m_idx.empty() ? x0.m_idx.end() : x0.m_idx.end() - 1);
        DCRTPolyHip o0(P, x0.m_limbs - 1, x0.m_format, 1, kept), o1(P, x0.m_limbs - 1, x0.m_format, 1, kept);
        size_t wsb = fhe_rescale_workspace_bytes(P->ctx(), x0.m_limbs, 2);
        void* ws   = nullptr;
        check(fhe_malloc(P->ctx(), wsb, &ws));
        fhe_status s = fhe_mod_reduce_limbs_pair(P->ctx(), x0.m_data, x1.m_data, x0.idx(), x0.m_limbs, t, negtInvModq, qlInvModq.data(),
                                                 x0.m_format == EVALUATION, o0.m_data, o1.m_data, ws, wsb, nullptr);
        fhe_stream_sync(P->ctx(), nullptr);
        fhe_free(P->ctx(), ws);
        check(s);
        x0 = std::move(o0);
        x1 = std::move(o1);
    }
    // The level alignment of BGV's automatic scaling modes on one operand (LeveledSHEBGVRNS::AdjustLevelsAndDepthInPlace,
    // bgvrns-leveledshe.cpp:83-233) as one call: every row times `scalar` (1: none), then ModReduce (dcrtpoly-impl.h:736-755) on the rows
    // dropRows (strictly decreasing; empty: the last row) with the rows above each discarded, of which the leading nOut rows (0: all below the
    // lowest dropped row) are left.  Tables derived from the moduli and t; the tower must use the leading context limbs (fhe_mod_reduce_multi)
    void ModReduceMulti(uint64_t t, uint64_t scalar = 1, std::vector<uint32_t> dropRows = {}, uint32_t nOut = 0) {
        if (!m_idx.empty())
            throw Error("ModReduceMulti: tower must use the leading context limbs");
        if (dropRows.empty())
            dropRows.push_back(m_limbs - 1);
        if (nOut == 0)
            nOut = dropRows.back();
        if (nOut < 1 || nOut >= m_limbs)
            throw Error("ModReduceMulti: nOut out of range");
        const uint32_t levels = (uint32_t)dropRows.size();
        DCRTPolyHip out(m_params, nOut, m_format, m_batch);
        size_t wsb = fhe_mod_reduce_multi_workspace_bytes(m_params->ctx(), m_limbs, levels, m_batch);
        void* ws   = nullptr;
        check(fhe_malloc(m_params->ctx(), wsb ? wsb : 8, &ws));
        fhe_status s = fhe_mod_reduce_multi(m_params->ctx(), m_data, m_limbs, t, scalar, dropRows.data(), levels, nOut, m_format == EVALUATION,
                                            m_batch, out.m_data, ws, wsb, nullptr);
        fhe_stream_sync(m_params->ctx(), nullptr);
        fhe_free(m_params->ctx(), ws);
        check(s);
        *this = std::move(out);
    }
    // ... of the two elements of one ciphertext (batch 1 each, allocated on their own, over any limbs of the context) in the same launches,
    // with the caller's tables: negtInvModq[k] of row dropRows[k] and, one after the other, the rows' qlInvModq (dropRows[k] residues each)
    // (fhe_mod_reduce_multi_limbs_pair)
    static void ModReduceMultiPair(DCRTPolyHip& x0, DCRTPolyHip& x1, uint64_t t, uint64_t scalar, const std::vector<uint32_t>& dropRows,
                                   uint32_t nOut, const std::vector<uint64_t>& negtInvModq, const std::vector<uint64_t>& qlInvModq) {
        if (x0.m_batch != 1 || x1.m_batch != 1 || x0.m_limbs != x1.m_limbs || x0.m_format != x1.m_format || x0.m_idx != x1.m_idx)
            throw Error("ModReduceMultiPair: two single towers over the same limbs in the same format expected");
        size_t entries = 0;
        for (uint32_t r : dropRows)
            entries += r;
        if (dropRows.empty() || negtInvModq.size() < dropRows.size() || qlInvModq.size() < entries)
            throw Error("ModReduceMultiPair: one negtInvModq entry per dropped row and dropRows[k] qlInvModq entries per step expected");
        if (nOut < 1 || nOut > dropRows.back())
            throw Error("ModReduceMultiPair: nOut out of range");
        const auto& P = x0.m_params;
        std::vector<uint32_t> kept(x0.m_idx.begin(), x0.m_idx.empty() ? x0.m_idx.end() : x0.m_idx.begin() + nOut);
        DCRTPolyHip o0(P, nOut, x0.m_format, 1, kept), o1(P, nOut, x0.m_format, 1, kept);
        const uint32_t levels = (uint32_t)dropRows.size();
        size_t wsb = fhe_mod_reduce_multi_workspace_bytes(P->ctx(), x0.m_limbs, levels, 2);
        void* ws   = nullptr;
        check(fhe_malloc(P->ctx(), wsb ? wsb : 8, &ws));
        fhe_status s = fhe_mod_reduce_multi_limbs_pair(P->ctx(), x0.m_data, x1.m_data, x0.idx(), x0.m_limbs, t, scalar, dropRows.data(), levels,
                                                       nOut, negtInvModq.data(), qlInvModq.data(), x0.m_format == EVALUATION, o0.m_data,
                                                       o1.m_data, ws, wsb, nullptr);
        fhe_stream_sync(P->ctx(), nullptr);
        fhe_free(P->ctx(), ws);
        check(s);
        x0 = std::move(o0);
        x1 = std::move(o1);
    }
    // the leading nOut rows of the two elements of one ciphertext times `scalar`: the EvalMultCoreInPlace and LevelReduceInternalInPlace of
    // a plan without a ModReduce (fhe_mul_const_pair on nOut rows)
    static void TimesScalarPair(DCRTPolyHip& x0, DCRTPolyHip& x1, uint64_t scalar, uint32_t nOut) {
        if (x0.m_batch != 1 || x1.m_batch != 1 || x0.m_limbs != x1.m_limbs || x0.m_format != x1.m_format || x0.m_idx != x1.m_idx)
            throw Error("TimesScalarPair: two single towers over the same limbs in the same format expected");
        if (nOut < 1 || nOut > x0.m_limbs)
            throw Error("TimesScalarPair: nOut out of range");
        const auto& P = x0.m_params;
        std::vector<uint32_t> kept(x0.m_idx.begin(), x0.m_idx.empty() ? x0.m_idx.end() : x0.m_idx.begin() + nOut);
        std::vector<uint64_t> consts(nOut);
        for (uint32_t i = 0; i < nOut; ++i)
            consts[i] = scalar % P->GetModuli()[x0.m_idx.empty() ? i : x0.m_idx[i]];
        DCRTPolyHip o0(P, nOut, x0.m_format, 1, kept), o1(P, nOut, x0.m_format, 1, kept);
        check(fhe_mul_const_pair(P->ctx(), o0.m_data, o1.m_data, x0.m_data, x1.m_data, consts.data(), o0.idx(), nOut, nullptr));
        check(fhe_stream_sync(P->ctx(), nullptr));
        x0 = std::move(o0);
        x1 = std::move(o1);
    }
    // the moduli of the tower's rows
    std::vector<uint64_t> GetRowModuli() const {
        std::vector<uint64_t> qs(m_limbs);
        for (uint32_t i = 0; i < m_limbs; ++i)
            qs[i] = m_params->GetModuli()[m_idx.empty() ? i : m_idx[i]];
        return qs;
    }
    // ModReduce `levels` times on a COEFFICIENT tower, its last limb first, in one launch per 16 limbs: what the COEFFICIENT branch of
    // PKEBGVRNS::Decrypt (bgvrns-pke.cpp:73-81) does to every element (fhe_mod_reduce_chain; the tables are derived from the moduli and t)
    void ModReduceChain(uint32_t levels, uint64_t t) {
        if (m_format != COEFFICIENT)
            throw Error("ModReduceChain: COEFFICIENT format expected");
        if (levels < 1 || levels >= m_limbs)
            throw Error("ModReduceChain: levels must be in [1, limbs)");
        std::vector<uint32_t> kept(m_idx.begin(), m_idx.empty() ? m_idx.end() : m_idx.end() - levels);
        DCRTPolyHip out(m_params, m_limbs - levels, m_format, m_batch, kept);
        size_t wsb = fhe_mod_reduce_chain_workspace_bytes(m_params->ctx(), m_limbs, levels, m_batch);
        void* ws   = nullptr;
        if (wsb)
            check(fhe_malloc(m_params->ctx(), wsb, &ws));
        fhe_status s = fhe_mod_reduce_chain(m_params->ctx(), m_data, idx(), m_limbs, levels, t, m_batch, out.m_data, ws, wsb, nullptr);
        fhe_stream_sync(m_params->ctx(), nullptr);
        if (ws)
            fhe_free(m_params->ctx(), ws);
        check(s);
        *this = std::move(out);
    }
    // the whole chain down to one limb and DecryptionCRTInterpolate(t) of it: the NativePoly words, [batch][N] in [0, t), of PKEBGVRNS::Decrypt
    // (bgvrns-pke.cpp:56-60, 96) and MultipartyDecryptFusion (bgvrns-multiparty.cpp:79-83, 94) for b in COEFFICIENT format (fhe_mod_reduce_to_t)
    std::vector<uint64_t> ModReduceToT(uint64_t t) const {
        if (m_format != COEFFICIENT)
            throw Error("ModReduceToT: COEFFICIENT format expected");
        return toT([&](uint64_t* out, void* ws, size_t wsb) {
            return fhe_mod_reduce_to_t(m_params->ctx(), m_data, idx(), m_limbs, t, m_batch, out, ws, wsb, nullptr);
        }, fhe_mod_reduce_chain_workspace_bytes(m_params->ctx(), m_limbs, m_limbs - 1, m_batch));
    }
    // PKEBGVRNS::Decrypt of `batch` EVALUATION ciphertexts of 2 or 3 elements under the secret key s (one tower over the same limbs): the
    // NativePoly words before decoding, [batch][N] (fhe_bgv_decrypt)
    static std::vector<uint64_t> BgvDecrypt(const std::vector<const DCRTPolyHip*>& elements, const DCRTPolyHip& s, uint64_t t) {
        if (elements.size() < 2 || elements.size() > 3)
            throw Error("BgvDecrypt: a ciphertext of 2 or 3 elements expected");
        const DCRTPolyHip& c0 = *elements[0];
        std::vector<const uint64_t*> ptrs;
        for (const DCRTPolyHip* e : elements) {
            if (e->m_limbs != c0.m_limbs || e->m_batch != c0.m_batch || e->m_idx != c0.m_idx || e->m_format != EVALUATION)
                throw Error("BgvDecrypt: EVALUATION elements over the same limbs expected");
            ptrs.push_back(e->m_data);
        }
        if (s.m_limbs != c0.m_limbs || s.m_batch != 1 || s.m_idx != c0.m_idx || s.m_format != EVALUATION)
            throw Error("BgvDecrypt: the secret key must be one EVALUATION tower over the elements' limbs");
        const uint32_t nElem = (uint32_t)elements.size();
        return c0.toT([&](uint64_t* out, void* ws, size_t wsb) {
            return fhe_bgv_decrypt(c0.m_params->ctx(), ptrs.data(), nElem, s.m_data, c0.idx(), c0.m_limbs, t, c0.m_batch, out, ws, wsb, nullptr);
        }, fhe_bgv_decrypt_workspace_bytes(c0.m_params->ctx(), nElem, c0.m_limbs, c0.m_batch));
    }
    // ExpandCRTBasis / ExpandCRTBasisReverseOrder to this basis + the context limbs `extra` (dcrtpoly-impl.h:1088-1148)
    DCRTPolyHip ExpandCRTBasis(const std::vector<uint32_t>& extra, Format resultFormat, bool reverseOrder = false) const {
        std::vector<uint32_t> src = m_idx;
        if (src.empty())
            for (uint32_t i = 0; i < m_limbs; ++i)
                src.push_back(i);
        fhe_conv* cv = nullptr;
        check(fhe_conv_create(m_params->ctx(), src.data(), m_limbs, extra.data(), (uint32_t)extra.size(), &cv));
        std::vector<uint32_t> all = reverseOrder ? extra : src;
        all.insert(all.end(), reverseOrder ? src.begin() : extra.begin(), reverseOrder ? src.end() : extra.end());
        DCRTPolyHip out(m_params, (uint32_t)all.size(), resultFormat, m_batch, all);
        size_t wsb = fhe_expand_crt_basis_workspace_bytes(cv, m_batch);
        void* ws   = nullptr;
        check(fhe_malloc(m_params->ctx(), wsb, &ws));
        fhe_status s = fhe_expand_crt_basis(cv, m_data, m_format == EVALUATION, out.m_data, resultFormat == EVALUATION,
                                            reverseOrder, m_batch, ws, wsb, nullptr);
        fhe_stream_sync(m_params->ctx(), nullptr);
        fhe_free(m_params->ctx(), ws);
        fhe_conv_destroy(cv);
        check(s);
        return out;
    }
    // ApproxSwitchCRTBasis / SwitchCRTBasis to the context limbs `target` (dcrtpoly-impl.h:888-932, 1008-1085)
    DCRTPolyHip SwitchCRTBasis(const std::vector<uint32_t>& target, bool exact) const {
        if (m_format != COEFFICIENT)
            throw Error("SwitchCRTBasis: COEFFICIENT format expected");
        std::vector<uint32_t> src = m_idx;
        if (src.empty())
            for (uint32_t i = 0; i < m_limbs; ++i)
                src.push_back(i);
        fhe_conv* cv = nullptr;
        check(fhe_conv_create(m_params->ctx(), src.data(), m_limbs, target.data(), (uint32_t)target.size(), &cv));
        DCRTPolyHip out(m_params, (uint32_t)target.size(), COEFFICIENT, m_batch, target);
        fhe_status s = exact ? fhe_switch_basis_exact(cv, m_data, m_limbs, 0, out.m_data, (uint32_t)target.size(), 0, m_batch, nullptr)
                             : fhe_approx_switch_basis(cv, m_data, m_limbs, 0, out.m_data, (uint32_t)target.size(), 0, m_batch, nullptr);
        fhe_stream_sync(m_params->ctx(), nullptr);
        fhe_conv_destroy(cv);
        check(s);
        return out;
    }

private:
    typedef fhe_status (*BinFn)(fhe_ctx*, uint64_t*, const uint64_t*, const uint64_t*, const uint32_t*, uint32_t, uint32_t, void*);
    void compatible(const DCRTPolyHip& r) const {
        if (r.m_limbs != m_limbs || r.m_batch != m_batch)
            throw Error("tower size mismatch");  // dcrtpoly.h:154-162
        if (r.m_format != m_format)
            throw Error("format mismatch");
    }
    DCRTPolyHip bin(BinFn f, const DCRTPolyHip& r) const {
        compatible(r);
        DCRTPolyHip out(m_params, m_limbs, m_format, m_batch, m_idx);
        check(f(m_params->ctx(), out.m_data, m_data, r.m_data, idx(), m_limbs, m_batch, nullptr));
        return out;
    }
    DCRTPolyHip& binEq(BinFn f, const DCRTPolyHip& r) {
        compatible(r);
        check(f(m_params->ctx(), m_data, m_data, r.m_data, idx(), m_limbs, m_batch, nullptr));
        return *this;
    }
    // one [batch][N] result of `run(out, ws, wsBytes)` brought to the host (ModReduceToT, BgvDecrypt)
    template <typename Run>
    std::vector<uint64_t> toT(Run run, size_t wsb) const {
        fhe_ctx* c       = m_params->ctx();
        const size_t outb = (size_t)m_batch * GetRingDimension() * sizeof(uint64_t);
        void *ws = nullptr, *out = nullptr;
        check(fhe_malloc(c, outb, &out));
        if (wsb && fhe_malloc(c, wsb, &ws) != FHE_OK) {
            fhe_free(c, out);
            throw Error(fhe_last_error());
        }
        std::vector<uint64_t> h(outb / sizeof(uint64_t));
        fhe_status s = run(static_cast<uint64_t*>(out), ws, wsb);
        if (s == FHE_OK)
            s = fhe_memcpy_d2h(c, h.data(), out, outb, nullptr);
        fhe_stream_sync(c, nullptr);
        if (ws)
            fhe_free(c, ws);
        fhe_free(c, out);
        check(s);
        return h;
    }
    const uint32_t* idx() const { return m_idx.empty() ? nullptr : m_idx.data(); }
    size_t words() const { return (size_t)m_batch * m_limbs * m_params->GetRingDimension(); }
    size_t bytes() const { return words() * sizeof(uint64_t); }

    std::shared_ptr<Params> m_params;
    uint32_t m_limbs = 0, m_batch = 0;
    Format m_format  = EVALUATION;
    std::vector<uint32_t> m_idx;
    uint64_t* m_data = nullptr;
};

// ---- BGV automatic scaling: the case table of LeveledSHEBGVRNS::AdjustLevelsAndDepth[ToOne]InPlace (bgvrns-leveledshe.cpp:83-233) as a plan
// (host arithmetic modulo t only), and its executor.
// What the reference reads of a ciphertext, and what the plan decides for it.
struct BgvOperand {
    uint32_t level = 0, noiseScaleDeg = 1, sizeQl = 0;
    uint64_t scalingFactorInt = 1;
    // the plan: scalar (1: none), the rows ModReduce is called on (strictly decreasing), the rows that are left
    uint64_t scalar = 1;
    std::vector<uint32_t> dropRows;
    uint32_t nOut = 0;
    BgvOperand() = default;
    BgvOperand(uint32_t lvl, uint32_t depth, uint32_t rows, uint64_t scf)
        : level(lvl), noiseScaleDeg(depth), sizeQl(rows), scalingFactorInt(scf), nOut(rows) {}
    bool Untouched() const { return scalar == 1 && dropRows.empty() && nOut == sizeQl; }
};
namespace bgvplan {
inline uint64_t mulmod(uint64_t a, uint64_t b, uint64_t t) { return (uint64_t)((unsigned __int128)(a % t) * (b % t) % t); }
inline uint64_t invmod(uint64_t a, uint64_t t) {  // NativeInteger::ModInverse: extended Euclid, t need not be prime
    __int128 r0 = t, r1 = a % t, s0 = 0, s1 = 1;
    while (r1) {
        const __int128 qt = r0 / r1, r2 = r0 - qt * r1, s2 = s0 - qt * s1;
        r0 = r1, r1 = r2, s0 = s1, s1 = s2;
    }
    if (r0 != 1)
        throw Error("BgvAdjustPlan: a scaling factor is not invertible modulo t");
    return (uint64_t)((s0 % (__int128)t + t) % t);
}
// the three members as bookkeeping (bgvrns-leveledshe.cpp:44-81, 235-247)
inline void evalMultCore(BgvOperand& c, uint64_t scalar, uint64_t t) {
    if (!c.Untouched())
        throw Error("BgvAdjustPlan: the scalar product comes first");
    c.scalar = scalar;
    c.noiseScaleDeg += 1;
    c.scalingFactorInt = mulmod(c.scalingFactorInt, scalar, t);
}
inline void modReduce(BgvOperand& c, uint64_t t, const std::vector<uint64_t>& modReduceFactorInt) {
    if (c.nOut < 2)
        throw Error("Too few towers to support ModReduce.");
    const uint32_t r = c.nOut - 1;
    c.dropRows.push_back(r);
    c.nOut = r, c.level += 1, c.noiseScaleDeg -= 1;
    c.scalingFactorInt = mulmod(c.scalingFactorInt, invmod(modReduceFactorInt.at(r), t), t);
}
inline void levelReduce(BgvOperand& c, uint32_t levels) { c.nOut -= levels, c.level += levels; }
}  // namespace bgvplan
// modReduceFactorInt[i] = CryptoParametersBGVRNS::GetModReduceFactorInt(i), scalingFactorIntBig[i] = GetScalingFactorIntBig(i); ct1 / ct2 come
// in with (level, noiseScaleDeg, sizeQl, scalingFactorInt) and leave with the new values and their plans.  toOne: AdjustLevelsAndDepthToOneInPlace.
inline void BgvAdjustPlan(BgvOperand& ct1, BgvOperand& ct2, uint64_t t, const std::vector<uint64_t>& modReduceFactorInt,
                          const std::vector<uint64_t>& scalingFactorIntBig, bool toOne = false) {
    using namespace bgvplan;
    const auto& mrf = modReduceFactorInt;
    if (ct1.level != ct2.level) {
        // the branches for c1lvl > c2lvl are those for c1lvl < c2lvl with the names swapped
        BgvOperand &lo = ct1.level < ct2.level ? ct1 : ct2, &hi = ct1.level < ct2.level ? ct2 : ct1;
        const uint32_t gap = hi.level - lo.level;
        const uint64_t scf1Inv = invmod(lo.scalingFactorInt, t);
        if (lo.noiseScaleDeg == 2) {
            if (hi.noiseScaleDeg == 2) {
                evalMultCore(lo, mulmod(mulmod(hi.scalingFactorInt, scf1Inv, t), mrf.at(lo.sizeQl - 1), t), t);
                modReduce(lo, t, mrf);
                if (gap > 1)
                    levelReduce(lo, gap - 1);
                lo.scalingFactorInt = hi.scalingFactorInt;
            }
            else if (gap == 1)
                modReduce(lo, t, mrf);
            else {
                evalMultCore(lo, mulmod(mulmod(scalingFactorIntBig.at(hi.level - 1), scf1Inv, t), mrf.at(lo.sizeQl - 1), t), t);
                modReduce(lo, t, mrf);
                if (gap > 2)
                    levelReduce(lo, gap - 2);
                modReduce(lo, t, mrf);
                lo.scalingFactorInt = hi.scalingFactorInt;
            }
        }
        else if (hi.noiseScaleDeg == 2) {
            evalMultCore(lo, mulmod(hi.scalingFactorInt, scf1Inv, t), t);
            levelReduce(lo, gap);
            lo.scalingFactorInt = hi.scalingFactorInt;
        }
        else {
            evalMultCore(lo, mulmod(scalingFactorIntBig.at(hi.level - 1), scf1Inv, t), t);
            if (gap > 1)
                levelReduce(lo, gap - 1);
            modReduce(lo, t, mrf);
            lo.scalingFactorInt = hi.scalingFactorInt;
        }
    }
    else if (ct1.noiseScaleDeg < ct2.noiseScaleDeg)
        evalMultCore(ct1, ct1.scalingFactorInt, t);
    else if (ct2.noiseScaleDeg < ct1.noiseScaleDeg)
        evalMultCore(ct2, ct2.scalingFactorInt, t);
    if (toOne && ct1.noiseScaleDeg == 2) {
        modReduce(ct1, t, mrf);
        modReduce(ct2, t, mrf);
    }
}
// runs one operand's plan on the two elements of its ciphertext: nothing, fhe_mul_const on the nOut rows that are left when no ModReduce is in
// the plan, else ONE fhe_mod_reduce_multi_limbs_pair with the tables of CryptoParametersBGVRNS (GetNegtInvModq / GetqlInvModq) derived here
inline void BgvAdjust(DCRTPolyHip& c0, DCRTPolyHip& c1, const BgvOperand& plan, uint64_t t) {
    if (plan.Untouched())
        return;
    if (plan.dropRows.empty())
        return DCRTPolyHip::TimesScalarPair(c0, c1, plan.scalar, plan.nOut);
    const std::vector<uint64_t> qs = c0.GetRowModuli();
    std::vector<uint64_t> negt, inv;
    for (uint32_t r : plan.dropRows) {
        const uint64_t ql = qs.at(r);
        negt.push_back((ql - bgvplan::invmod(t % ql, ql)) % ql);
        for (uint32_t i = 0; i < r; ++i)
            inv.push_back(bgvplan::invmod(ql % qs[i], qs[i]));
    }
    DCRTPolyHip::ModReduceMultiPair(c0, c1, t, plan.scalar, plan.dropRows, plan.nOut, negt, inv);
}

// KeySwitchHYBRID over a context holding Q then P limbs (keyswitch-hybrid.cpp:308-435)
class KeySwitchHybrid {
public:
    KeySwitchHybrid(std::shared_ptr<Params> params, uint32_t sizeQ, uint32_t sizeP, uint32_t numPartQ)
        : m_params(std::move(params)), m_sizeQ(sizeQ), m_sizeP(sizeP) {
        check(fhe_ks_plan_create(m_params->ctx(), sizeQ, sizeP, numPartQ, &m_plan));
    }
    ~KeySwitchHybrid() {
        for (auto& kv : m_rot)
            fhe_ks_key_destroy(kv.second.second);
        for (void* d : m_diag)
            fhe_free(m_params->ctx(), d);
        fhe_ks_key_destroy(m_key);
        if (m_ws)
            fhe_free(m_params->ctx(), m_ws);
        fhe_ks_plan_destroy(m_plan);
    }
    // EvalKeyRelin b/a vectors, host uint64[numPartQ][sizeQ+sizeP][N] (evalkeyrelin.h:141,171)
    void SetEvalKey(const std::vector<uint64_t>& keyB, const std::vector<uint64_t>& keyA) {
        fhe_ks_key_destroy(m_key);
        m_key = nullptr;
        check(fhe_ks_key_upload(m_plan, keyB.data(), keyA.data(), &m_key));
    }
    // t = 0: CKKS / BFV; t >= 2: BGV, ApproxModDown with the plaintext modulus (the fhe_bgv_* twin of the entry point)
    // KeySwitchCore(a, evalKey)
    std::pair<DCRTPolyHip, DCRTPolyHip> KeySwitchCore(const DCRTPolyHip& a, uint64_t t = 0) {
        const uint32_t sizeQl = a.GetNumOfElements(), batch = a.GetBatch();
        DCRTPolyHip o0(m_params, sizeQl, EVALUATION, batch), o1(m_params, sizeQl, EVALUATION, batch);
        reserve(sizeQl, batch);
        check(t ? fhe_bgv_keyswitch_hybrid(m_plan, m_key, a.data(), sizeQl, t, batch, o0.data(), o1.data(), m_ws, m_wsBytes, nullptr)
                : fhe_keyswitch_hybrid(m_plan, m_key, a.data(), sizeQl, batch, o0.data(), o1.data(), m_ws, m_wsBytes, nullptr));
        return {std::move(o0), std::move(o1)};
    }
    // acc += KeySwitchCore(a), in place (base-leveledshe.cpp:207-211)
    void KeySwitchCoreAcc(const DCRTPolyHip& a, DCRTPolyHip& acc0, DCRTPolyHip& acc1, uint64_t t = 0) {
        const uint32_t sizeQl = a.GetNumOfElements(), batch = a.GetBatch();
        reserve(sizeQl, batch);
        check(t ? fhe_bgv_keyswitch_hybrid_acc(m_plan, m_key, a.data(), sizeQl, t, batch, acc0.data(), acc1.data(), m_ws, m_wsBytes, nullptr)
                : fhe_keyswitch_hybrid_acc(m_plan, m_key, a.data(), sizeQl, batch, acc0.data(), acc1.data(), m_ws, m_wsBytes, nullptr));
    }
    // LeveledSHEBase::EvalMult(ct1, ct2, evalKey) for 2-element ciphertexts (base-leveledshe.cpp:201-214)
    std::pair<DCRTPolyHip, DCRTPolyHip> EvalMult(const DCRTPolyHip& a0, const DCRTPolyHip& a1, const DCRTPolyHip& b0, const DCRTPolyHip& b1,
                                                 uint64_t t = 0) {
        const uint32_t sizeQl = a0.GetNumOfElements(), batch = a0.GetBatch();
        DCRTPolyHip c0(m_params, sizeQl, EVALUATION, batch), c1(m_params, sizeQl, EVALUATION, batch);
        reserve(sizeQl, batch);
        check(t ? fhe_bgv_eval_mult(m_plan, m_key, a0.data(), a1.data(), b0.data(), b1.data(), sizeQl, t, batch, c0.data(), c1.data(), m_ws,
                                    m_wsBytes, nullptr)
                : fhe_ckks_eval_mult(m_plan, m_key, a0.data(), a1.data(), b0.data(), b1.data(), sizeQl, batch, c0.data(), c1.data(), m_ws,
                                     m_wsBytes, nullptr));
        return {std::move(c0), std::move(c1)};
    }

    // DCRTPolyImpl::ApproxModDown with the context's P (dcrtpoly-impl.h:966-1005; t > 0: the BGV form): x over Q_l u P
    DCRTPolyHip ApproxModDown(const DCRTPolyHip& x, uint32_t sizeQl, uint64_t t = 0) {
        DCRTPolyHip out(m_params, sizeQl, EVALUATION, x.GetBatch());
        reserve(sizeQl, x.GetBatch());
        check(t ? fhe_approx_mod_down_bgv(m_plan, x.data(), sizeQl, t, x.GetBatch(), out.data(), m_ws, m_wsBytes, nullptr)
                : fhe_approx_mod_down(m_plan, x.data(), sizeQl, x.GetBatch(), out.data(), m_ws, m_wsBytes, nullptr));
        return out;
    }
    // KeySwitchHYBRID::KeySwitchExt for one element (keyswitch-hybrid.cpp:217-243): c * [P] on the Q_l limbs, zeros on P
    DCRTPolyHip KeySwitchExt(const DCRTPolyHip& c) {
        DCRTPolyHip out(m_params, c.GetNumOfElements() + m_sizeP, EVALUATION, c.GetBatch(), extLimbs(c.GetNumOfElements()));
        check(fhe_ks_ext(m_plan, c.data(), c.GetNumOfElements(), c.GetBatch(), out.data(), nullptr));
        return out;
    }
    // KeySwitchHYBRID::KeySwitchDown (keyswitch-hybrid.cpp:245-278)
    std::pair<DCRTPolyHip, DCRTPolyHip> KeySwitchDown(const DCRTPolyHip& x0, const DCRTPolyHip& x1) {
        const uint32_t sizeQl = x0.GetNumOfElements() - m_sizeP;
        DCRTPolyHip o0(m_params, sizeQl, EVALUATION, x0.GetBatch()), o1(m_params, sizeQl, EVALUATION, x0.GetBatch());
        reserve(sizeQl, x0.GetBatch());
        check(fhe_ks_down(m_plan, x0.data(), x1.data(), sizeQl, x0.GetBatch(), o0.data(), o1.data(), m_ws, m_wsBytes, nullptr));
        return {std::move(o0), std::move(o1)};
    }
    // LeveledSHEBase::EvalAutomorphism / EvalRotate (base-leveledshe.cpp:381-422) with the key set by SetRotationKey
    std::pair<DCRTPolyHip, DCRTPolyHip> EvalRotate(const DCRTPolyHip& c0, const DCRTPolyHip& c1, int32_t index, uint64_t t = 0) {
        auto it = m_rot.find(index);
        if (it == m_rot.end())
            throw Error("EvalRotate: no rotation key for index " + std::to_string(index));
        const uint32_t sizeQl = c0.GetNumOfElements(), batch = c0.GetBatch();
        DCRTPolyHip o0(m_params, sizeQl, EVALUATION, batch), o1(m_params, sizeQl, EVALUATION, batch);
        reserve(sizeQl, batch);
        check(t ? fhe_bgv_eval_automorphism(m_plan, it->second.second, c0.data(), c1.data(), it->second.first, sizeQl, t, batch, o0.data(),
                                            o1.data(), m_ws, m_wsBytes, nullptr)
                : fhe_eval_automorphism(m_plan, it->second.second, c0.data(), c1.data(), it->second.first, sizeQl, batch, o0.data(),
                                        o1.data(), m_ws, m_wsBytes, nullptr));
        return {std::move(o0), std::move(o1)};
    }
    // hoisted rotations: EvalFastRotationPrecompute once (base-leveledshe.cpp:425-430), then EvalFastRotation per index
    // (:432-463); the digits live in this object's workspace until the next call that uses it
    void EvalFastRotationPrecompute(const DCRTPolyHip& c1) {
        reserve(c1.GetNumOfElements(), c1.GetBatch());
        check(fhe_ks_precompute(m_plan, c1.data(), c1.GetNumOfElements(), c1.GetBatch(), m_ws, m_wsBytes, nullptr));
    }
    std::pair<DCRTPolyHip, DCRTPolyHip> EvalFastRotation(const DCRTPolyHip& c0, const DCRTPolyHip& c1, int32_t index, uint64_t t = 0) {
        auto it = m_rot.find(index);
        if (it == m_rot.end())
            throw Error("EvalFastRotation: no rotation key for index " + std::to_string(index));
        const uint32_t sizeQl = c0.GetNumOfElements(), batch = c0.GetBatch();
        DCRTPolyHip o0(m_params, sizeQl, EVALUATION, batch), o1(m_params, sizeQl, EVALUATION, batch);
        check(t ? fhe_bgv_eval_fast_rotation(m_plan, it->second.second, c0.data(), c1.data(), it->second.first, sizeQl, t, batch, o0.data(),
                                             o1.data(), m_ws, m_wsBytes, nullptr)
                : fhe_eval_fast_rotation(m_plan, it->second.second, c0.data(), c1.data(), it->second.first, sizeQl, batch, o0.data(),
                                         o1.data(), m_ws, m_wsBytes, nullptr));
        return {std::move(o0), std::move(o1)};
    }
    // EvalFastKeySwitchCore (keyswitch-hybrid.cpp:381-400) with the rotation key of `index` on the digits EvalFastRotationPrecompute left
    std::pair<DCRTPolyHip, DCRTPolyHip> FastKeySwitch(const DCRTPolyHip& c1, int32_t index, uint64_t t = 0) {
        auto it = m_rot.find(index);
        if (it == m_rot.end())
            throw Error("FastKeySwitch: no rotation key for index " + std::to_string(index));
        const uint32_t sizeQl = c1.GetNumOfElements(), batch = c1.GetBatch();
        DCRTPolyHip o0(m_params, sizeQl, EVALUATION, batch), o1(m_params, sizeQl, EVALUATION, batch);
        check(t ? fhe_bgv_ks_fast_keyswitch(m_plan, it->second.second, c1.data(), sizeQl, t, batch, o0.data(), o1.data(), m_ws, m_wsBytes, nullptr)
                : fhe_ks_fast_keyswitch(m_plan, it->second.second, c1.data(), sizeQl, batch, o0.data(), o1.data(), m_ws, m_wsBytes, nullptr));
        return {std::move(o0), std::move(o1)};
    }
    uint32_t AutomorphismIndex(int32_t index) const { return m_rot.at(index).first; }
    const fhe_ks_key* RotationKey(int32_t index) const { return m_rot.at(index).second; }
    fhe_ks_plan* plan() const { return m_plan; }
    const fhe_ks_key* key() const { return m_key; }

    // ---- BSGS linear transform with double hoisting (FHECKKSRNS::EvalLinearTransform, ckksrns-fhe.cpp:1832-1882) ----
    // rotation key of `index` slots (EvalRotateKeyGen's key for FindAutomorphismIndex2nComplex(index, 2N))
    void SetRotationKey(int32_t index, const std::vector<uint64_t>& keyB, const std::vector<uint64_t>& keyA) {
        const uint32_t k = fhe_param_find_automorphism_index_2n_complex(index, 2u * m_params->GetRingDimension());
        if (k == 0)
            throw Error("m should be a power of two.");
        fhe_ks_key* h = nullptr;
        check(fhe_ks_key_upload(m_plan, keyB.data(), keyA.data(), &h));
        auto it = m_rot.find(index);
        if (it != m_rot.end())
            fhe_ks_key_destroy(it->second.second);
        m_rot[index] = {k, h};
    }
    // an encoded diagonal (EvalLinearTransformPrecompute's aux plaintext): host rows [sizeQl+sizeP][N], EVALUATION
    // format over the limbs {0..sizeQl-1, sizeQ..sizeQ+sizeP-1}; stays on the device until the object dies
    const uint64_t* UploadDiagonal(const std::vector<uint64_t>& rows) {
        void* d = nullptr;
        check(fhe_malloc(m_params->ctx(), rows.size() * sizeof(uint64_t), &d));
        m_diag.push_back(d);
        check(fhe_memcpy_h2d(m_params->ctx(), d, rows.data(), rows.size() * sizeof(uint64_t), nullptr));
        check(fhe_stream_sync(m_params->ctx(), nullptr));  // the copy reads the caller's vector: it may die right after the call
        return static_cast<const uint64_t*>(d);
    }
    // A[i] = diagonal i (nullptr = absent); baby step bStep, giant steps ceil(|A| / bStep)
    std::pair<DCRTPolyHip, DCRTPolyHip> EvalLinearTransform(const std::vector<const uint64_t*>& A, uint32_t bStep,
                                                             const DCRTPolyHip& c0, const DCRTPolyHip& c1) {
        const uint32_t slots = (uint32_t)A.size(), gStep = (slots + bStep - 1) / bStep;
        std::vector<uint32_t> inK(bStep, 0), outK(gStep, 0);
        std::vector<const fhe_ks_key*> inKeys(bStep, nullptr), outKeys(gStep, nullptr);
        auto key = [&](int32_t index, uint32_t& k, const fhe_ks_key*& h) {
            auto it = m_rot.find(index);
            if (it == m_rot.end())
                throw Error("EvalLinearTransform: no rotation key for index " + std::to_string(index));
            k = it->second.first, h = it->second.second;
        };
        for (uint32_t j = 1; j < bStep; ++j)
            key((int32_t)j, inK[j], inKeys[j]);
        for (uint32_t i = 1; i < gStep; ++i)
            key((int32_t)(bStep * i), outK[i], outKeys[i]);
        std::vector<const uint64_t*> diag((size_t)gStep * bStep, nullptr);
        for (uint32_t i = 0; i < slots; ++i)
            diag[i] = A[i];
        const uint32_t sizeQl = c0.GetNumOfElements(), batch = c0.GetBatch();
        DCRTPolyHip o0(m_params, sizeQl, EVALUATION, batch), o1(m_params, sizeQl, EVALUATION, batch);
        const size_t need = fhe_ckks_bsgs_workspace_bytes(m_plan, sizeQl, batch, bStep, gStep);
        void* ws          = nullptr;
        check(fhe_malloc(m_params->ctx(), need, &ws));
        const fhe_status st = fhe_ckks_bsgs_transform(m_plan, c0.data(), c1.data(), sizeQl, batch, bStep, inK.data(), inKeys.data(),
                                                      gStep, outK.data(), outKeys.data(), diag.data(), o0.data(), o1.data(), ws,
                                                      need, nullptr);
        fhe_stream_sync(m_params->ctx(), nullptr);
        fhe_free(m_params->ctx(), ws);
        check(st);
        return {std::move(o0), std::move(o1)};
    }

private:
    void reserve(uint32_t sizeQl, uint32_t batch) {
        size_t need = fhe_ks_workspace_bytes(m_plan, sizeQl, batch);
        if (need > m_wsBytes) {
            if (m_ws)
                fhe_free(m_params->ctx(), m_ws);
            check(fhe_malloc(m_params->ctx(), need, &m_ws));
            m_wsBytes = need;
        }
    }
    std::vector<uint32_t> extLimbs(uint32_t sizeQl) const {  // context limbs of Q_l u P
        std::vector<uint32_t> v;
        for (uint32_t i = 0; i < sizeQl; ++i)
            v.push_back(i);
        for (uint32_t j = 0; j < m_sizeP; ++j)
            v.push_back(m_sizeQ + j);
        return v;
    }
    std::shared_ptr<Params> m_params;
    uint32_t m_sizeQ, m_sizeP;
    fhe_ks_plan* m_plan = nullptr;
    fhe_ks_key* m_key   = nullptr;
    std::map<int32_t, std::pair<uint32_t, fhe_ks_key*>> m_rot;  // rotation index -> (automorphism index, key)
    std::vector<void*> m_diag;
    void* m_ws          = nullptr;
    size_t m_wsBytes    = 0;
};

// BFV multiplication in the BEHZ RNS variant (CryptoParametersBFVRNS's BEHZ tables, bfvrns-cryptoparameters.cpp:673-850;
// DCRTPolyImpl::FastBaseConvqToBskMontgomery / FastRNSFloorq / FastBaseConvSK, dcrtpoly-impl.h:1694-1929;
// LeveledSHEBFVRNS::EvalMult, bfvrns-leveledshe.cpp:198-445).  The context holds Q (qLimbs) and Bsk (bskLimbs, m_sk last).
class BfvBehz {
public:
    // the Bsk moduli / roots the reference picks for (N, Q, t) (bfvrns-cryptoparameters.cpp:682-711)
    static void SelectBsk(uint32_t cyclotomicOrder, const std::vector<uint64_t>& q, uint64_t t, std::vector<uint64_t>& bsk,
                          std::vector<uint64_t>& psi) {
        uint32_t logN = 0;
        while ((2u << logN) < cyclotomicOrder)
            ++logN;
        bsk.assign(q.size() + 1, 0), psi.assign(q.size() + 1, 0);
        if (fhe_param_behz_bsk(logN, (uint32_t)q.size(), q.data(), t, bsk.data(), psi.data()) != q.size() + 1)
            throw Error("BEHZ: no auxiliary basis for these parameters");
    }
    BfvBehz(std::shared_ptr<Params> params, const std::vector<uint32_t>& qLimbs, const std::vector<uint32_t>& bskLimbs, uint64_t t)
        : m_params(std::move(params)), m_numQ((uint32_t)qLimbs.size()) {
        if (bskLimbs.size() != qLimbs.size() + 1)
            throw Error("BEHZ: Bsk must hold one limb more than Q");
        check(fhe_behz_create(m_params->ctx(), qLimbs.data(), m_numQ, bskLimbs.data(), t, &m_plan));
    }
    ~BfvBehz() { fhe_behz_destroy(m_plan); }
    BfvBehz(const BfvBehz&)            = delete;
    BfvBehz& operator=(const BfvBehz&) = delete;
    // EvalMultNoRelin: (a0, a1) x (b0, b1) -> (d0, d1, d2), inputs EVALUATION over Q, outputs COEFFICIENT like the reference's
    std::vector<DCRTPolyHip> EvalMultNoRelin(const DCRTPolyHip& a0, const DCRTPolyHip& a1, const DCRTPolyHip& b0, const DCRTPolyHip& b1) {
        const uint32_t batch = a0.GetBatch();
        std::vector<DCRTPolyHip> d;
        for (int i = 0; i < 3; ++i)
            d.emplace_back(m_params, m_numQ, COEFFICIENT, batch);
        const size_t need = fhe_bfv_eval_mult_behz_workspace_bytes(m_plan, batch);
        void* ws          = nullptr;
        check(fhe_malloc(m_params->ctx(), need, &ws));
        const fhe_status st = fhe_bfv_eval_mult_behz(m_plan, a0.data(), a1.data(), b0.data(), b1.data(), d[0].data(), d[1].data(),
                                                     d[2].data(), 0, batch, ws, need, nullptr);
        fhe_stream_sync(m_params->ctx(), nullptr);
        fhe_free(m_params->ctx(), ws);
        check(st);
        return d;
    }
    // cc->EvalMult: EvalMultNoRelin + HYBRID relinearisation with `ks`'s evaluation key (base-leveledshe.cpp:201-214)
    std::pair<DCRTPolyHip, DCRTPolyHip> EvalMult(KeySwitchHybrid& ks, const DCRTPolyHip& a0, const DCRTPolyHip& a1,
                                                 const DCRTPolyHip& b0, const DCRTPolyHip& b1) {
        const uint32_t batch = a0.GetBatch();
        DCRTPolyHip c0(m_params, m_numQ, EVALUATION, batch), c1(m_params, m_numQ, EVALUATION, batch);
        const size_t need = fhe_bfv_eval_mult_relin_workspace_bytes(m_plan, ks.plan(), batch);
        void* ws          = nullptr;
        check(fhe_malloc(m_params->ctx(), need, &ws));
        const fhe_status st = fhe_bfv_eval_mult_relin_behz(m_plan, ks.plan(), ks.key(), a0.data(), a1.data(), b0.data(), b1.data(),
                                                           c0.data(), c1.data(), batch, ws, need, nullptr);
        fhe_stream_sync(m_params->ctx(), nullptr);
        fhe_free(m_params->ctx(), ws);
        check(st);
        return {std::move(c0), std::move(c1)};
    }

private:
    std::shared_ptr<Params> m_params;
    uint32_t m_numQ;
    fhe_behz* m_plan = nullptr;
};

// BFV multiplication in the HPS family — technique 1 = HPS, 2 = HPSPOVERQ, 3 = HPSPOVERQLEVELED (the reference's default) —
// LeveledSHEBFVRNS::EvalMult, bfvrns-leveledshe.cpp:198-302, 354-412, with the tables of CryptoParametersBFVRNS's HPS block
// (bfvrns-cryptoparameters.cpp:143-665) derived by the plan.  The context holds Q (qLimbs) and the auxiliary basis R (rLimbs).
class HpsPlan {
public:
    // the R moduli / roots the reference picks for (N, Q, technique) (bfvrns-cryptoparameters.cpp:75, 126-139)
    static void SelectR(uint32_t cyclotomicOrder, const std::vector<uint64_t>& q, int technique, std::vector<uint64_t>& r,
                        std::vector<uint64_t>& psi) {
        uint32_t logN = 0;
        while ((2u << logN) < cyclotomicOrder)
            ++logN;
        r.assign(q.size() + 1, 0), psi.assign(q.size() + 1, 0);
        const uint32_t n = fhe_param_hps_r(logN, (uint32_t)q.size(), q.data(), technique, r.data(), psi.data());
        if (n == 0)
            throw Error("HPS: no auxiliary basis for these parameters");
        r.resize(n), psi.resize(n);
    }
    HpsPlan(std::shared_ptr<Params> params, const std::vector<uint32_t>& qLimbs, const std::vector<uint32_t>& rLimbs, uint64_t t,
            int technique)
        : m_params(std::move(params)), m_numQ((uint32_t)qLimbs.size()) {
        check(fhe_hps_create(m_params->ctx(), qLimbs.data(), m_numQ, rLimbs.data(), (uint32_t)rLimbs.size(), t, technique, &m_plan));
    }
    ~HpsPlan() { fhe_hps_destroy(m_plan); }
    HpsPlan(const HpsPlan&)            = delete;
    HpsPlan& operator=(const HpsPlan&) = delete;
    // EvalMultNoRelin: (a0, a1) x (b0, b1) -> (d0, d1, d2), inputs EVALUATION over Q; outputs COEFFICIENT like the reference's, or
    // EVALUATION (outEval) for the relinearisation that follows.  sizeQl = numQ - levelsDropped (HPSPOVERQLEVELED; 0 = numQ).
    std::vector<DCRTPolyHip> EvalMultNoRelin(const DCRTPolyHip& a0, const DCRTPolyHip& a1, const DCRTPolyHip& b0, const DCRTPolyHip& b1,
                                             uint32_t sizeQl = 0, bool outEval = false) {
        const uint32_t batch = a0.GetBatch();
        if (sizeQl == 0)
            sizeQl = m_numQ;
        std::vector<DCRTPolyHip> d;
        for (int i = 0; i < 3; ++i)
            d.emplace_back(m_params, m_numQ, outEval ? EVALUATION : COEFFICIENT, batch);
        const size_t need = fhe_bfv_eval_mult_hps_workspace_bytes(m_plan, sizeQl, batch);
        if (need == 0)
            throw Error("HPS: sizeQl does not fit the technique");
        void* ws = nullptr;
        check(fhe_malloc(m_params->ctx(), need, &ws));
        const fhe_status st = fhe_bfv_eval_mult_hps(m_plan, a0.data(), a1.data(), b0.data(), b1.data(), d[0].data(), d[1].data(),
                                                    d[2].data(), sizeQl, outEval ? 1 : 0, batch, ws, need, nullptr);
        fhe_stream_sync(m_params->ctx(), nullptr);
        fhe_free(m_params->ctx(), ws);
        check(st);
        return d;
    }
    fhe_hps* plan() const { return m_plan; }

private:
    std::shared_ptr<Params> m_params;
    uint32_t m_numQ;
    fhe_hps* m_plan = nullptr;
};

// BFV of the HPS family on HYBRID keys: rotations and relinearisation at the level the reference drops to (LeveledSHEBFVRNS::
// EvalFastRotationPrecompute / EvalFastRotation / EvalAutomorphism / RelinearizeCore / EvalMult, bfvrns-leveledshe.cpp:735-938, with
// KeySwitchHYBRID).  Pairs an HpsPlan with a KeySwitchHybrid of the same context (Q the context's leading limbs, the key-switch plan's
// sizeQ == numQ); both must outlive this object.  All towers are [batch][numQ][N]; sizeQl = numQ - levelsDropped for the KEY SWITCH
// (1 ... numQ for HPSPOVERQLEVELED, numQ otherwise; 0 = numQ).  Keys are the KeySwitchHybrid's (key() / RotationKey(index)), k is the
// automorphism index (AutomorphismIndex(index)).
class BfvHybrid {
public:
    BfvHybrid(std::shared_ptr<Params> params, HpsPlan& hps, KeySwitchHybrid& ks, uint32_t numQ)
        : m_params(std::move(params)), m_numQ(numQ) {
        check(fhe_bfv_hybrid_create(hps.plan(), ks.plan(), &m_plan));
    }
    ~BfvHybrid() {
        fhe_bfv_hybrid_destroy(m_plan);
        if (m_ws)
            fhe_free(m_params->ctx(), m_ws);
    }
    BfvHybrid(const BfvHybrid&)            = delete;
    BfvHybrid& operator=(const BfvHybrid&) = delete;
    // the digits of c1 at sizeQl limbs; they live in this object's workspace until the next precompute, automorphism or relinearisation
    void FastRotationPrecompute(const DCRTPolyHip& c1, uint32_t sizeQl = 0) {
        sizeQl = level(sizeQl);
        reserve(sizeQl, c1.GetBatch());
        check(fhe_bfv_fast_rotation_precompute_hybrid(m_plan, c1.data(), sizeQl, c1.GetBatch(), m_ws, m_wsBytes, nullptr));
    }
    std::pair<DCRTPolyHip, DCRTPolyHip> FastRotation(const fhe_ks_key* key, const DCRTPolyHip& c0, const DCRTPolyHip& c1, uint32_t k,
                                                     uint32_t sizeQl = 0) {
        const uint32_t batch = c0.GetBatch();
        DCRTPolyHip o0(m_params, m_numQ, EVALUATION, batch), o1(m_params, m_numQ, EVALUATION, batch);
        check(fhe_bfv_eval_fast_rotation_hybrid(m_plan, key, c0.data(), c1.data(), k, level(sizeQl), batch, o0.data(), o1.data(), m_ws,
                                                m_wsBytes, nullptr));
        return {std::move(o0), std::move(o1)};
    }
    std::pair<DCRTPolyHip, DCRTPolyHip> Automorphism(const fhe_ks_key* key, const DCRTPolyHip& c0, const DCRTPolyHip& c1, uint32_t k,
                                                     uint32_t sizeQl = 0) {
        const uint32_t batch = c0.GetBatch();
        sizeQl = level(sizeQl);
        DCRTPolyHip o0(m_params, m_numQ, EVALUATION, batch), o1(m_params, m_numQ, EVALUATION, batch);
        reserve(sizeQl, batch);
        check(fhe_bfv_eval_automorphism_hybrid(m_plan, key, c0.data(), c1.data(), k, sizeQl, batch, o0.data(), o1.data(), m_ws, m_wsBytes,
                                               nullptr));
        return {std::move(o0), std::move(o1)};
    }
    // (d0 + Expand(ks0(d2)), d1 + Expand(ks1(d2))), EVALUATION; the three inputs share one format (COEFFICIENT as EvalMultNoRelin leaves
    // them, or EVALUATION)
    std::pair<DCRTPolyHip, DCRTPolyHip> Relinearize(const fhe_ks_key* key, const DCRTPolyHip& d0, const DCRTPolyHip& d1,
                                                    const DCRTPolyHip& d2, uint32_t sizeQl = 0) {
        const uint32_t batch = d0.GetBatch();
        sizeQl = level(sizeQl);
        DCRTPolyHip c0(m_params, m_numQ, EVALUATION, batch), c1(m_params, m_numQ, EVALUATION, batch);
        reserve(sizeQl, batch);
        check(fhe_bfv_relinearize_hybrid(m_plan, key, d0.data(), d1.data(), d2.data(), d2.GetFormat() == EVALUATION ? 1 : 0, sizeQl, batch,
                                         c0.data(), c1.data(), m_ws, m_wsBytes, nullptr));
        return {std::move(c0), std::move(c1)};
    }
    // cc->EvalMult: the product at sizeQlMult limbs, the relinearisation at sizeQlRelin
    std::pair<DCRTPolyHip, DCRTPolyHip> EvalMult(const fhe_ks_key* key, const DCRTPolyHip& a0, const DCRTPolyHip& a1, const DCRTPolyHip& b0,
                                                 const DCRTPolyHip& b1, uint32_t sizeQlMult = 0, uint32_t sizeQlRelin = 0) {
        const uint32_t batch = a0.GetBatch();
        sizeQlMult = level(sizeQlMult), sizeQlRelin = level(sizeQlRelin);
        DCRTPolyHip c0(m_params, m_numQ, EVALUATION, batch), c1(m_params, m_numQ, EVALUATION, batch);
        const size_t need = fhe_bfv_eval_mult_relin_hps_hybrid_workspace_bytes(m_plan, sizeQlMult, sizeQlRelin, batch);
        if (need == 0)
            throw Error("BFV on HYBRID keys: a level does not fit the technique");
        void* ws = nullptr;
        check(fhe_malloc(m_params->ctx(), need, &ws));
        const fhe_status st = fhe_bfv_eval_mult_relin_hps_hybrid(m_plan, key, a0.data(), a1.data(), b0.data(), b1.data(), c0.data(),
                                                                 c1.data(), sizeQlMult, sizeQlRelin, batch, ws, need, nullptr);
        fhe_stream_sync(m_params->ctx(), nullptr);
        fhe_free(m_params->ctx(), ws);
        check(st);
        return {std::move(c0), std::move(c1)};
    }
    fhe_bfv_hybrid* plan() const { return m_plan; }

private:
    uint32_t level(uint32_t sizeQl) const { return sizeQl ? sizeQl : m_numQ; }
    void reserve(uint32_t sizeQl, uint32_t batch) {
        const size_t need = fhe_bfv_hybrid_workspace_bytes(m_plan, sizeQl, batch);
        if (need == 0)
            throw Error("BFV on HYBRID keys: sizeQl does not fit the technique");
        if (need > m_wsBytes) {
            if (m_ws)
                fhe_free(m_params->ctx(), m_ws);
            m_ws = nullptr, m_wsBytes = 0;
            check(fhe_malloc(m_params->ctx(), need, &m_ws));
            m_wsBytes = need;
        }
    }
    std::shared_ptr<Params> m_params;
    uint32_t m_numQ;
    fhe_bfv_hybrid* m_plan = nullptr;
    void* m_ws             = nullptr;
    size_t m_wsBytes       = 0;
};

// ---- evaluation keys made on the device (KeySwitchHYBRID::KeySwitchGenInternal, keyswitch-hybrid.cpp:51-130) ----
// The two slabs of a key set, [nKeys * numPartQ][sizeQ+sizeP][N] in EVALUATION format, and one handle per key that fhe_ks_key_wrap laid
// over its window of them: what the composites of KeySwitchHybrid / BfvHybrid take as `key`.  The handles die with the set.
struct HybridKeySet {
    DCRTPolyHip b, a;
    std::vector<fhe_ks_key*> keys;
    HybridKeySet(fhe_ks_plan* plan, DCRTPolyHip&& b_, DCRTPolyHip&& a_, uint32_t nKeys) : b(std::move(b_)), a(std::move(a_)) {
        const size_t words = (size_t)b.GetBatch() / nKeys * b.GetNumOfElements() * b.GetRingDimension();
        for (uint32_t k = 0; k < nKeys; ++k) {
            fhe_ks_key* h = nullptr;
            check(fhe_ks_key_wrap(plan, b.data() + k * words, a.data() + k * words, &h));
            keys.push_back(h);
        }
    }
    ~HybridKeySet() {
        for (auto* k : keys)
            fhe_ks_key_destroy(k);
    }
    HybridKeySet(const HybridKeySet&)            = delete;
    HybridKeySet& operator=(const HybridKeySet&) = delete;
};
// the sNewExt block (:59-83): s over Q, EVALUATION -> Q u P (fhe_ks_secret_extend)
inline DCRTPolyHip KeySwitchSecretExtend(KeySwitchHybrid& ks, const DCRTPolyHip& s, uint32_t sizeP) {
    const auto& params = s.GetParams();
    DCRTPolyHip out(params, s.GetNumOfElements() + sizeP, EVALUATION);
    const size_t wsb = (size_t)s.GetRingDimension() * 8;
    void* ws         = nullptr;
    check(fhe_malloc(params->ctx(), wsb, &ws));
    const fhe_status st = fhe_ks_secret_extend(ks.plan(), s.data(), out.data(), ws, wsb, nullptr);
    fhe_stream_sync(params->ctx(), nullptr);
    fhe_free(params->ctx(), ws);
    check(st);
    return out;
}
// nKeys = kNew.size() keys from the caller's a and e (both [nKeys * numPartQ][sizeQ+sizeP][N], EVALUATION); e's buffer becomes b.
// key k switches sigma_kOld[k](sOld) to sigma_kNew[k](sNew): EvalMultKeyGen is (1, 1) with sOld = s * s, EvalAutomorphismKeyGen of the
// automorphism index i is (i^-1 mod 2N, 1) with sOld = s (base-leveledshe.cpp:146-154, 336-379).  ns = GetNoiseScale().
inline std::unique_ptr<HybridKeySet> KeyGenHybrid(KeySwitchHybrid& ks, const DCRTPolyHip& sNewExt, const DCRTPolyHip& sOld,
                                                  const std::vector<uint32_t>& kNew, const std::vector<uint32_t>& kOld, uint64_t ns,
                                                  DCRTPolyHip&& a, DCRTPolyHip&& e) {
    if (kNew.empty() || kNew.size() != kOld.size())
        throw Error("KeyGenHybrid: one automorphism index pair per key");
    check(fhe_ks_keygen_hybrid(ks.plan(), (uint32_t)kNew.size(), kNew.data(), kOld.data(), sNewExt.data(), sOld.data(), ns, a.data(),
                               e.data(), e.data(), nullptr));
    return std::make_unique<HybridKeySet>(ks.plan(), std::move(e), std::move(a), (uint32_t)kNew.size());
}
// the seeded form (fhe_ks_keygen_hybrid_blake2): a = the uniform blake2 sampler's words from counterA, e = the Gaussian sampler's from
// counterE; *nextA / *nextE, when given, receive the first counters the call did not use (fhe_ks_keygen_counters)
inline std::unique_ptr<HybridKeySet> KeyGenHybridBlake2(KeySwitchHybrid& ks, uint32_t numPartQ, const DCRTPolyHip& sNewExt,
                                                        const DCRTPolyHip& sOld, const std::vector<uint32_t>& kNew,
                                                        const std::vector<uint32_t>& kOld, uint64_t ns, double sigma, const uint32_t key[16],
                                                        uint64_t counterA, uint64_t counterE, uint64_t* nextA = nullptr,
                                                        uint64_t* nextE = nullptr) {
    if (kNew.empty() || kNew.size() != kOld.size())
        throw Error("KeyGenHybridBlake2: one automorphism index pair per key");
    const uint32_t nKeys = (uint32_t)kNew.size();
    const auto& params   = sNewExt.GetParams();
    DCRTPolyHip b(params, sNewExt.GetNumOfElements(), EVALUATION, nKeys * numPartQ), a(params, sNewExt.GetNumOfElements(), EVALUATION,
                                                                                        nKeys * numPartQ);
    check(fhe_ks_keygen_hybrid_blake2(ks.plan(), nKeys, kNew.data(), kOld.data(), sNewExt.data(), sOld.data(), ns, sigma, key, counterA,
                                      counterE, b.data(), a.data(), nullptr));
    uint64_t nA = 0, nE = 0;
    check(fhe_ks_keygen_counters(ks.plan(), nKeys, &nA, &nE));
    if (nextA)
        *nextA = counterA + nA;
    if (nextE)
        *nextE = counterE + nE;
    return std::make_unique<HybridKeySet>(ks.plan(), std::move(b), std::move(a), nKeys);
}

// ---- BV evaluation keys made on the device (KeySwitchBV::KeySwitchGenInternal, keyswitch-bv.cpp:49-225) ----
// The two halves of a key set, [nKeys * D_0][sizeQ][N] each in EVALUATION format, and one handle per key that fhe_bv_key_wrap laid over
// its window of them: what fhe_keyswitch_bv, fhe_bv_eval_fast_rotation and the BFV composites on BV keys take as `key`.  The halves live
// in `slabs` (two towers, or one that holds b | a | workspace for the seeded public-key form); the handles die with the set.
struct BvKeySet {
    std::vector<DCRTPolyHip> slabs;
    uint64_t *b = nullptr, *a = nullptr;
    size_t halfWords = 0;
    std::vector<fhe_bv_key*> keys;
    BvKeySet(std::vector<DCRTPolyHip>&& s, uint64_t* b_, uint64_t* a_, uint32_t sizeQ, uint32_t baseBits, uint32_t nKeys)
        : slabs(std::move(s)), b(b_), a(a_) {
        fhe_ctx* ctx       = slabs[0].GetParams()->ctx();
        const size_t words = (size_t)fhe_crt_decompose_towers(ctx, nullptr, sizeQ, baseBits) * sizeQ * slabs[0].GetRingDimension();
        halfWords          = words * nKeys;
        for (uint32_t k = 0; k < nKeys; ++k) {
            fhe_bv_key* h = nullptr;
            check(fhe_bv_key_wrap(ctx, sizeQ, baseBits, b + k * words, a + k * words, &h));
            keys.push_back(h);
        }
    }
    ~BvKeySet() {
        for (auto* k : keys)
            fhe_bv_key_destroy(k);
    }
    BvKeySet(const BvKeySet&)            = delete;
    BvKeySet& operator=(const BvKeySet&) = delete;
    std::vector<uint64_t> GetValues(int half) const {  // [nKeys * D_0][sizeQ][N] of b (0) or a (1)
        std::vector<uint64_t> out(halfWords);
        fhe_ctx* ctx = slabs[0].GetParams()->ctx();
        check(fhe_memcpy_d2h(ctx, out.data(), half ? a : b, halfWords * 8, nullptr));
        check(fhe_stream_sync(ctx, nullptr));
        return out;
    }
};
inline std::unique_ptr<BvKeySet> MakeBvKeySet(DCRTPolyHip&& b, DCRTPolyHip&& a, uint32_t baseBits, uint32_t nKeys) {
    const uint32_t sizeQ = b.GetNumOfElements();
    uint64_t *pb = b.data(), *pa = a.data();
    std::vector<DCRTPolyHip> slabs;
    slabs.push_back(std::move(b)), slabs.push_back(std::move(a));
    return std::make_unique<BvKeySet>(std::move(slabs), pb, pa, sizeQ, baseBits, nKeys);
}
// the secret-key form (:49-160) from the caller's a and e (both [nKeys * D_0][sizeQ][N], EVALUATION); e's buffer becomes b.  Key k
// switches sigma_kOld[k](sOld) to sigma_kNew[k](sNew), as in KeyGenHybrid; a taken from another key is MultiKeySwitchGen's overload.
inline std::unique_ptr<BvKeySet> KeyGenBv(uint32_t baseBits, const DCRTPolyHip& sNew, const DCRTPolyHip& sOld, const std::vector<uint32_t>& kNew,
                                          const std::vector<uint32_t>& kOld, uint64_t ns, DCRTPolyHip&& a, DCRTPolyHip&& e) {
    if (kNew.empty() || kNew.size() != kOld.size())
        throw Error("KeyGenBv: one automorphism index pair per key");
    check(fhe_bv_keygen(sNew.GetParams()->ctx(), sNew.GetNumOfElements(), baseBits, (uint32_t)kNew.size(), kNew.data(), kOld.data(),
                        sNew.data(), sOld.data(), ns, a.data(), e.data(), e.data(), nullptr));
    return MakeBvKeySet(std::move(e), std::move(a), baseBits, (uint32_t)kNew.size());
}
// the seeded form (fhe_bv_keygen_blake2); *nextA / *nextE: the first counters the call did not use (fhe_bv_keygen_counters)
inline std::unique_ptr<BvKeySet> KeyGenBvBlake2(uint32_t baseBits, const DCRTPolyHip& sNew, const DCRTPolyHip& sOld,
                                                const std::vector<uint32_t>& kNew, const std::vector<uint32_t>& kOld, uint64_t ns, double sigma,
                                                const uint32_t key[16], uint64_t counterA, uint64_t counterE, uint64_t* nextA = nullptr,
                                                uint64_t* nextE = nullptr) {
    if (kNew.empty() || kNew.size() != kOld.size())
        throw Error("KeyGenBvBlake2: one automorphism index pair per key");
    const uint32_t nKeys = (uint32_t)kNew.size(), sizeQ = sNew.GetNumOfElements();
    const auto& params   = sNew.GetParams();
    uint64_t nA = 0, nE = 0;
    check(fhe_bv_keygen_counters(params->ctx(), sizeQ, baseBits, nKeys, 0, &nA, &nE));  // (refuses what the key generation would)
    const uint32_t towers = nKeys * fhe_crt_decompose_towers(params->ctx(), nullptr, sizeQ, baseBits);
    DCRTPolyHip b(params, sizeQ, EVALUATION, towers), a(params, sizeQ, EVALUATION, towers);
    check(fhe_bv_keygen_blake2(params->ctx(), sizeQ, baseBits, nKeys, kNew.data(), kOld.data(), sNew.data(), sOld.data(), ns, sigma, key,
                               counterA, counterE, b.data(), a.data(), nullptr));
    if (nextA)
        *nextA = counterA + nA;
    if (nextE)
        *nextE = counterE + nE;
    return MakeBvKeySet(std::move(b), std::move(a), baseBits, nKeys);
}
// the public-key form (:162-225, PREBase::ReKeyGen) from the caller's u, e0, e1 ([nKeys * D_0][sizeQ][N], EVALUATION); e0's and e1's
// buffers become b and a.  p0, p1: the new public key, [1][sizeQ][N], or [nKeys][sizeQ][N] for one public key per key.
inline std::unique_ptr<BvKeySet> KeyGenBvPk(uint32_t baseBits, uint32_t nKeys, const DCRTPolyHip& p0, const DCRTPolyHip& p1,
                                            const DCRTPolyHip& sOld, uint64_t ns, const DCRTPolyHip& u, DCRTPolyHip&& e0, DCRTPolyHip&& e1) {
    if (p0.GetBatch() != p1.GetBatch() || (p0.GetBatch() != 1 && p0.GetBatch() != nKeys))
        throw Error("KeyGenBvPk: one public key, or one per key");
    check(fhe_bv_keygen_pk(sOld.GetParams()->ctx(), sOld.GetNumOfElements(), baseBits, nKeys, p0.data(), p1.data(), p0.GetBatch() > 1 ? 1 : 0,
                           sOld.data(), ns, u.data(), e0.data(), e1.data(), e0.data(), e1.data(), nullptr));
    return MakeBvKeySet(std::move(e0), std::move(e1), baseBits, nKeys);
}
// its seeded form (fhe_bv_keygen_pk_blake2) in one slab b | a | workspace: one Gaussian call and one transform call; gaussianU: u from the
// Gaussian sampler (SecretKeyDist == GAUSSIAN); *nextU / *nextE: the first counters the call did not use
inline std::unique_ptr<BvKeySet> KeyGenBvPkBlake2(uint32_t baseBits, uint32_t nKeys, const DCRTPolyHip& p0, const DCRTPolyHip& p1,
                                                  const DCRTPolyHip& sOld, bool gaussianU, uint64_t ns, double sigma, const uint32_t key[16],
                                                  uint64_t counterU, uint64_t counterE, uint64_t* nextU = nullptr,
                                                  uint64_t* nextE = nullptr) {
    if (p0.GetBatch() != p1.GetBatch() || (p0.GetBatch() != 1 && p0.GetBatch() != nKeys))
        throw Error("KeyGenBvPkBlake2: one public key, or one per key");
    const auto& params   = sOld.GetParams();
    const uint32_t sizeQ = sOld.GetNumOfElements();
    uint64_t nU = 0, nE = 0;
    check(fhe_bv_keygen_counters(params->ctx(), sizeQ, baseBits, nKeys, 1, &nU, &nE));
    const uint32_t towers = nKeys * fhe_crt_decompose_towers(params->ctx(), nullptr, sizeQ, baseBits);
    std::vector<DCRTPolyHip> slabs;
    slabs.emplace_back(params, sizeQ, EVALUATION, 3 * towers);
    const size_t wsb = fhe_bv_keygen_workspace_bytes(params->ctx(), sizeQ, baseBits, nKeys);
    uint64_t* b      = slabs[0].data();
    check(fhe_bv_keygen_pk_blake2(params->ctx(), sizeQ, baseBits, nKeys, p0.data(), p1.data(), p0.GetBatch() > 1 ? 1 : 0, sOld.data(),
                                  gaussianU ? 1 : 0, ns, sigma, key, counterU, counterE, b, b + wsb / 8, b + 2 * (wsb / 8), wsb, nullptr));
    if (nextU)
        *nextU = counterU + nU;
    if (nextE)
        *nextE = counterE + nE;
    return std::make_unique<BvKeySet>(std::move(slabs), b, b + wsb / 8, sizeQ, baseBits, nKeys);
}

// ---- encryption on the device (PKERNS::EncryptZeroCore + Encrypt, rns-pke.cpp:40-70, 111-197; PKEBFVRNS::Encrypt, bfvrns-pke.cpp:99-213)
// All towers over the leading context limbs.  The key towers may have more rows than the plaintext's level: their first rows are used.
// `batch` fresh ciphertexts in one slab [2][batch][sizeQl][N], EVALUATION: the c0 block, then the c1 block (what the seeded calls fill).
struct FreshCiphertexts {
    DCRTPolyHip ct;  // [2 * batch (+ batch of workspace behind them)][sizeQl][N]
    uint32_t batch;
    size_t blockWords() const { return (size_t)batch * ct.GetNumOfElements() * ct.GetRingDimension(); }
    uint64_t* c0() { return ct.data(); }
    uint64_t* c1() { return ct.data() + blockWords(); }
    std::vector<uint64_t> GetValues(int element) const {  // [batch][sizeQl][N] of c0 (0) or c1 (1)
        const std::vector<uint64_t> all = ct.GetValues();
        return std::vector<uint64_t>(all.begin() + element * blockWords(), all.begin() + (element + 1) * blockWords());
    }
};
// c0 = pkB * v + ns * e0 (+ msg), c1 = pkA * v + ns * e1 with the caller's randomness, in place: returns {e0's buffer, e1's buffer}
inline std::pair<DCRTPolyHip, DCRTPolyHip> EncryptPk(const DCRTPolyHip& pkB, const DCRTPolyHip& pkA, const DCRTPolyHip& v, DCRTPolyHip&& e0,
                                                      DCRTPolyHip&& e1, const DCRTPolyHip* msg, uint64_t ns) {
    if (pkB.GetNumOfElements() < v.GetNumOfElements() || pkA.GetNumOfElements() < v.GetNumOfElements())
        throw Error("EncryptPk: the public key has fewer towers than the plaintext");
    check(fhe_encrypt_pk_combine(v.GetParams()->ctx(), nullptr, v.GetNumOfElements(), v.GetBatch(), pkB.data(), pkA.data(), v.data(),
                                 e0.data(), e1.data(), msg ? msg->data() : nullptr, ns, e0.data(), e1.data(), nullptr));
    return {std::move(e0), std::move(e1)};
}
// c0 = a * s + ns * e (+ msg), c1 = -a, in place: returns {e's buffer, a's buffer}
inline std::pair<DCRTPolyHip, DCRTPolyHip> EncryptSk(const DCRTPolyHip& s, DCRTPolyHip&& a, DCRTPolyHip&& e, const DCRTPolyHip* msg,
                                                      uint64_t ns) {
    if (s.GetNumOfElements() < a.GetNumOfElements())
        throw Error("EncryptSk: the secret key has fewer towers than the plaintext");
    check(fhe_encrypt_sk_combine(a.GetParams()->ctx(), nullptr, a.GetNumOfElements(), a.GetBatch(), s.data(), a.data(), e.data(),
                                 msg ? msg->data() : nullptr, ns, e.data(), a.data(), nullptr));
    return {std::move(e), std::move(a)};
}
// the seeded forms; msg: [batch][sizeQl][N] in either format (COEFFICIENT needs ns = 1 modulo every limb) or null; gaussianV: v from the
// Gaussian sampler (SecretKeyDist == GAUSSIAN); *nextV / *nextA, *nextE: the first counters the call did not use (fhe_encrypt_counters)
inline FreshCiphertexts EncryptPkBlake2(const DCRTPolyHip& pkB, const DCRTPolyHip& pkA, uint32_t sizeQl, uint32_t batch, bool gaussianV,
                                        uint64_t ns, double sigma, const uint32_t key[16], uint64_t counterV, uint64_t counterE,
                                        const DCRTPolyHip* msg = nullptr, uint64_t* nextV = nullptr, uint64_t* nextE = nullptr) {
    const auto& params = pkB.GetParams();
    FreshCiphertexts out{DCRTPolyHip(params, sizeQl, EVALUATION, 3 * batch), batch};  // the workspace follows ct: one forward transform
    const size_t wsb = fhe_encrypt_workspace_bytes(params->ctx(), sizeQl, batch);
    check(fhe_encrypt_pk_blake2(params->ctx(), nullptr, sizeQl, batch, pkB.data(), pkA.data(), gaussianV ? 1 : 0, ns, sigma, key, counterV,
                                counterE, msg ? msg->data() : nullptr, msg ? (int)msg->GetFormat() : 0, out.ct.data(),
                                out.ct.data() + 2 * out.blockWords(), wsb, nullptr));
    uint64_t nV = 0, nE = 0;
    check(fhe_encrypt_counters(params->ctx(), sizeQl, batch, 0, &nV, &nE));
    if (nextV)
        *nextV = counterV + nV;
    if (nextE)
        *nextE = counterE + nE;
    return out;
}
inline FreshCiphertexts EncryptSkBlake2(const DCRTPolyHip& s, uint32_t sizeQl, uint32_t batch, uint64_t ns, double sigma,
                                        const uint32_t key[16], uint64_t counterA, uint64_t counterE, const DCRTPolyHip* msg = nullptr,
                                        uint64_t* nextA = nullptr, uint64_t* nextE = nullptr) {
    const auto& params = s.GetParams();
    FreshCiphertexts out{DCRTPolyHip(params, sizeQl, EVALUATION, 2 * batch), batch};
    check(fhe_encrypt_sk_blake2(params->ctx(), nullptr, sizeQl, batch, s.data(), ns, sigma, key, counterA, counterE,
                                msg ? msg->data() : nullptr, msg ? (int)msg->GetFormat() : 0, out.ct.data(), nullptr));
    uint64_t nA = 0, nE = 0;
    check(fhe_encrypt_counters(params->ctx(), sizeQl, batch, 1, &nA, &nE));
    if (nextA)
        *nextA = counterA + nA;
    if (nextE)
        *nextE = counterE + nE;
    return out;
}
// DCRTPoly::TimesQovert (dcrtpoly-impl.h:868-885) of a COEFFICIENT plaintext: the message of PKEBFVRNS::Encrypt with the STANDARD technique
inline DCRTPolyHip BfvScaledMessage(const DCRTPolyHip& ptxt, uint64_t t, uint64_t negQModt, const std::vector<uint64_t>& tInvModq) {
    if (ptxt.GetFormat() != COEFFICIENT)
        throw Error("BfvScaledMessage: COEFFICIENT format expected");
    if (tInvModq.size() < ptxt.GetNumOfElements())
        throw Error("BfvScaledMessage: one tInvModq residue per limb expected");
    DCRTPolyHip m(ptxt.GetParams(), ptxt.GetNumOfElements(), COEFFICIENT, ptxt.GetBatch());
    check(fhe_times_q_over_t(ptxt.GetParams()->ctx(), m.data(), ptxt.data(), t, negQModt, tInvModq.data(), nullptr, ptxt.GetNumOfElements(),
                             ptxt.GetBatch(), nullptr));
    return m;
}
// PKEBFVRNS::Encrypt(ptxt, publicKey / privateKey), STANDARD: negQModt = GetNegQModt(level), tInvModq = GettInvModq()
inline FreshCiphertexts BfvEncryptPkBlake2(const DCRTPolyHip& pkB, const DCRTPolyHip& pkA, const DCRTPolyHip& ptxt, uint64_t t,
                                           uint64_t negQModt, const std::vector<uint64_t>& tInvModq, bool gaussianV, double sigma,
                                           const uint32_t key[16], uint64_t counterV, uint64_t counterE) {
    const DCRTPolyHip m = BfvScaledMessage(ptxt, t, negQModt, tInvModq);
    return EncryptPkBlake2(pkB, pkA, ptxt.GetNumOfElements(), ptxt.GetBatch(), gaussianV, 1, sigma, key, counterV, counterE, &m);
}
inline FreshCiphertexts BfvEncryptSkBlake2(const DCRTPolyHip& s, const DCRTPolyHip& ptxt, uint64_t t, uint64_t negQModt,
                                           const std::vector<uint64_t>& tInvModq, double sigma, const uint32_t key[16], uint64_t counterA,
                                           uint64_t counterE) {
    const DCRTPolyHip m = BfvScaledMessage(ptxt, t, negQModt, tInvModq);
    return EncryptSkBlake2(s, ptxt.GetNumOfElements(), ptxt.GetBatch(), 1, sigma, key, counterA, counterE, &m);
}

// ---- decryption on the device (PKERNS::DecryptCore, rns-pke.cpp:199-225; MultipartyDecryptLead / Main, rns-multiparty.cpp:46-171;
// PKEBFVRNS::Decrypt, bfvrns-pke.cpp:215-245).  All towers over the leading context limbs; the key may have more rows than the ciphertext.
// b = [c0] + s * c1 + s^2 * c2 + s^3 * c3 [+ ns * noise] for 2 to 4 EVALUATION elements [batch][sizeQl][N] in one launch, in outFormat
// (COEFFICIENT: what PKECKKSRNS::Decrypt interpolates, ckksrns-pke.cpp:44-96).  withC0 = false (two elements, elements[0] may be null) is
// MultipartyDecryptMain.  noise: the flooding term, EVALUATION, or null.
inline DCRTPolyHip DecryptCore(const std::vector<const DCRTPolyHip*>& elements, const DCRTPolyHip& s, const DCRTPolyHip* noise = nullptr,
                               uint64_t ns = 1, bool withC0 = true, Format outFormat = EVALUATION) {
    if (elements.size() < 2 || !elements[1])
        throw Error("DecryptCore: a ciphertext of 2 to 4 elements expected");
    const DCRTPolyHip& c1 = *elements[1];
    std::vector<const uint64_t*> ptrs;
    for (const DCRTPolyHip* e : elements) {
        if (e && (e->GetNumOfElements() != c1.GetNumOfElements() || e->GetBatch() != c1.GetBatch() || e->GetFormat() != EVALUATION))
            throw Error("DecryptCore: EVALUATION elements of one shape expected");
        ptrs.push_back(e ? e->data() : nullptr);
    }
    if (s.GetNumOfElements() < c1.GetNumOfElements() || s.GetFormat() != EVALUATION)
        throw Error("DecryptCore: the secret key has fewer towers than the ciphertext");
    DCRTPolyHip b(c1.GetParams(), c1.GetNumOfElements(), outFormat, c1.GetBatch());
    check(fhe_decrypt_core(c1.GetParams()->ctx(), ptrs.data(), (uint32_t)ptrs.size(), s.data(), nullptr, c1.GetNumOfElements(), c1.GetBatch(),
                           noise ? noise->data() : nullptr, ns, withC0 ? 1 : 0, (int)outFormat, b.data(), nullptr));
    return b;
}
// PKEBFVRNS::Decrypt at sizeQl == sizeQ over the context's leading sizeQ limbs: technique 0 = BEHZ, 1 = HPS, 2 = HPSPOVERQ,
// 3 = HPSPOVERQLEVELED; the tables of CryptoParametersBFVRNS's decryption blocks are derived by the plan (fhe_bfv_decrypt_create).
class BfvDecrypt {
public:
    BfvDecrypt(std::shared_ptr<Params> params, uint32_t sizeQ, uint64_t t, int technique) : m_params(std::move(params)), m_sizeQ(sizeQ) {
        check(fhe_bfv_decrypt_create(m_params->ctx(), nullptr, sizeQ, t, technique, &m_plan));
    }
    ~BfvDecrypt() { fhe_bfv_decrypt_destroy(m_plan); }
    BfvDecrypt(const BfvDecrypt&)            = delete;
    BfvDecrypt& operator=(const BfvDecrypt&) = delete;
    // a derived table (ids: fhe_bfv_decrypt_table; doubles as their 64 bits); empty when the plan has none
    std::vector<uint64_t> Table(int id) const {
        std::vector<uint64_t> t(fhe_bfv_decrypt_table(m_plan, id, nullptr, 0));
        fhe_bfv_decrypt_table(m_plan, id, t.data(), t.size());
        return t;
    }
    // the NativePoly words modulo t, [batch][N], of `batch` EVALUATION ciphertexts of 2 to 4 elements under the secret key s
    std::vector<uint64_t> Decrypt(const std::vector<const DCRTPolyHip*>& elements, const DCRTPolyHip& s) const {
        if (elements.size() < 2 || !elements[0])
            throw Error("BfvDecrypt: a ciphertext of 2 to 4 elements expected");
        std::vector<const uint64_t*> ptrs;
        for (const DCRTPolyHip* e : elements) {
            if (!e || e->GetNumOfElements() != m_sizeQ || e->GetBatch() != elements[0]->GetBatch() || e->GetFormat() != EVALUATION)
                throw Error("BfvDecrypt: EVALUATION elements over the plan's limbs expected");
            ptrs.push_back(e->data());
        }
        if (s.GetNumOfElements() != m_sizeQ || s.GetFormat() != EVALUATION)
            throw Error("BfvDecrypt: the secret key must be one EVALUATION tower over the plan's limbs");
        const uint32_t batch = elements[0]->GetBatch();
        return run(batch, [&](uint64_t* out, void* ws, size_t wsb) {
            return fhe_bfv_decrypt(m_plan, ptrs.data(), (uint32_t)ptrs.size(), s.data(), batch, out, ws, wsb, nullptr);
        });
    }
    // the tail alone on b [batch][sizeQ][N] in either format (MultipartyBFVRNS::MultipartyDecryptFusion after its sum); b is only read
    std::vector<uint64_t> DecryptB(const DCRTPolyHip& b) const {
        if (b.GetNumOfElements() != m_sizeQ)
            throw Error("BfvDecrypt: b over the plan's limbs expected");
        return run(b.GetBatch(), [&](uint64_t* out, void* ws, size_t wsb) {
            return fhe_bfv_decrypt_b(m_plan, b.data(), b.GetFormat() == EVALUATION ? 1 : 0, b.GetBatch(), out, ws, wsb, nullptr);
        });
    }
    fhe_bfv_dec* plan() const { return m_plan; }

private:
    template <typename Run>
    std::vector<uint64_t> run(uint32_t batch, Run f) const {
        fhe_ctx* c        = m_params->ctx();
        const size_t outb = (size_t)batch * m_params->GetRingDimension() * sizeof(uint64_t), wsb = fhe_bfv_decrypt_workspace_bytes(m_plan, batch);
        void *ws = nullptr, *out = nullptr;
        check(fhe_malloc(c, outb, &out));
        if (fhe_malloc(c, wsb, &ws) != FHE_OK) {
            fhe_free(c, out);
            throw Error(fhe_last_error());
        }
        std::vector<uint64_t> h(outb / sizeof(uint64_t));
        fhe_status s = f(static_cast<uint64_t*>(out), ws, wsb);
        if (s == FHE_OK)
            s = fhe_memcpy_d2h(c, h.data(), out, outb, nullptr);
        fhe_stream_sync(c, nullptr);
        fhe_free(c, ws);
        fhe_free(c, out);
        check(s);
        return h;
    }
    std::shared_ptr<Params> m_params;
    uint32_t m_sizeQ;
    fhe_bfv_dec* m_plan = nullptr;
};

}  // namespace fhehip
#endif
