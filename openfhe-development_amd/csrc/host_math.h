// host_math.h — host-side number theory and table builders of the HIP backend (product code).
//
// Builds, with 64-bit modular arithmetic only, the constant operands the kernels consume:
//  * twiddle tables of ChineseRemainderTransformFTTNat::PreCompute
//    (src/core/include/math/hal/intnat/transformnat-impl.h:714-756),
//  * CRT conversion tables of CryptoParametersRNS::PrecomputeCRTTables
//    (src/pke/lib/schemerns/rns-cryptoparameters.cpp:199-349) — the reference forms them from BigInteger
//    products and quotients; every stored value is a residue of a product of moduli, so modular products
//    give identical numbers,
//  * CKKS rescale tables (src/pke/lib/scheme/ckksrns/ckksrns-cryptoparameters.cpp:60-81),
//  * modulus chains / roots for self-contained benchmarks (nbtheory-impl.h:183-231, 329-393;
//    ildcrtparams.h:100-117).
#ifndef FHE_HOST_MATH_H
#define FHE_HOST_MATH_H
#include <cstdint>
#include <vector>

namespace fhe {
namespace host {

typedef unsigned __int128 u128;

inline uint64_t mulmod(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)(((u128)a * b) % q); }
inline uint64_t powmod(uint64_t a, uint64_t e, uint64_t q) {
    uint64_t r = 1 % q;
    a %= q;
    for (; e; e >>= 1) {
        if (e & 1)
            r = mulmod(r, a, q);
        a = mulmod(a, a, q);
    }
    return r;
}
inline uint64_t invmod(uint64_t a, uint64_t q) { return powmod(a % q, q - 2, q); }  // q prime
inline uint32_t bitlen(uint64_t x) {
    uint32_t r = 0;
    for (; x; x >>= 1)
        ++r;
    return r;
}
inline uint64_t shoup(uint64_t w, uint64_t q) { return (uint64_t)((((u128)w) << 64) / q); }  // PrepModMulConst
inline uint64_t barrett_mu(uint64_t q) { return (uint64_t)(((u128)1 << (2 * bitlen(q) + 3)) / q); }  // ComputeMu
inline void mu128(uint64_t q, uint64_t* out2) {  // floor(2^128/q), q odd
    u128 m  = (~(u128)0) / q;
    out2[0] = (uint64_t)m;
    out2[1] = (uint64_t)(m >> 64);
}
inline uint32_t bitrev(uint32_t x, uint32_t nbits) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < nbits; ++i)
        r |= ((x >> i) & 1u) << (nbits - 1 - i);
    return r;
}

bool is_prime(uint64_t n);
bool is_primitive_root_2n(uint64_t psi, uint64_t twoN, uint64_t q);
uint64_t first_prime(uint32_t bits, uint64_t m);
uint64_t last_prime(uint32_t bits, uint64_t m);
uint64_t previous_prime(uint64_t q, uint64_t m);
uint64_t next_prime(uint64_t q, uint64_t m);
uint64_t min_root_of_unity(uint64_t m, uint64_t q);

// product of mods[k] (k in sel, k != skip) reduced mod `mod`
uint64_t prod_mod(const std::vector<uint64_t>& mods, int skip, uint64_t mod);

// ---- the reference's per-level tables of dropping the last limb of a tower over moduli q[0..n) ----
// q_l^-1 mod q_i, the one value all of them are made of.  0 when q_i == q_l: equal moduli have no inverse, and no table holds a zero otherwise.
inline uint64_t dropped_inv(uint64_t ql, uint64_t qi) { return invmod(ql % qi, qi); }
// CKKS (ckksrns-cryptoparameters.cpp:60-81), for the first `levels` steps, step k dropping q[n-1-k]: its n-1-k residues follow those of
// step k-1 (the layout of fhe_rescale_multi_limbs).  B = qlInvModq[i] = q_l^-1 mod q_i;
// A = QlQlInvModqlDivqlModq[i] = floor(Q' * (Q'^-1 mod q_l) / q_l) mod q_i = -(q_l^-1) mod q_i   
inline void rescale_step_tables(const uint64_t* q, uint32_t n, uint32_t levels, std::vector<uint64_t>& A, std::vector<uint64_t>& B) {
    A.clear(), B.clear();
    for (uint32_t k = 0; k < levels; ++k)
        for (uint32_t i = 0; i + 1 + k < n; ++i) {
            B.push_back(dropped_inv(q[n - 1 - k], q[i]));
            A.push_back((q[i] - B.back()) % q[i]);
        }
}
// BGV with plaintext modulus t (bgvrns-cryptoparameters.cpp, DCRTPolyImpl::ModReduce): B = qlInvModq[i], T[i] = t mod q_i (t > q_i: its
// residue), tInv = t^-1 mod q_l, negtInv = negtInvModq = -tInv mod q_l, and A[i] = t * inv_i mod q_i, where inv is callerB (the inverses a
// caller handed in, reduced) or, when that is null, B.
struct ModReduceTables {
    std::vector<uint64_t> A, B, T;
    uint64_t tInv, negtInv;
};
inline ModReduceTables mod_reduce_tables(const uint64_t* q, uint32_t n, uint64_t t, const uint64_t* callerB) {
    const uint32_t l  = n - 1;
    const uint64_t ql = q[l];
    ModReduceTables r{std::vector<uint64_t>(l), std::vector<uint64_t>(l), std::vector<uint64_t>(l), invmod(t % ql, ql), 0};
    r.negtInv = (ql - r.tInv) % ql;
    for (uint32_t i = 0; i < l; ++i) {
        r.B[i] = dropped_inv(ql, q[i]);
        r.T[i] = t % q[i];
        r.A[i] = mulmod(r.T[i], callerB ? callerB[i] : r.B[i], q[i]);
    }
    return r;
}
// `d` consecutive ModReduce steps on a COEFFICIENT tower over moduli q[0..n) as ONE pass (mod_reduce_chain_kernel): step k
// drops limb n-1-k, modulus qd_k.  Unrolling v <- (v + T * SM(delta_k)) * B_k, with SM(delta_k) = delta_k - c_k * qd_k as a residue
// (c_k = 1 when delta_k > floor(qd_k / 2)), gives for a row modulo q that sees the first s steps
//   v_s = x * X + sum_{k<s} (delta_k * W_k + c_k * Cn_k)   mod q,
//   X = M * prod_{j<s} B_j,   W_k = M * (t mod q) * prod_{k<=j<s} B_j,   Cn_k = -(qd_k * W_k),   B_j = qd_j^-1 mod q,
// M = 1 for a kept limb (s = d) and M = negtInvModq = -t^-1 mod q for the limb dropped at step s, whose v_s is delta_s.
// Layout, in words: row r at r * (3 + 3d), rows 0..d-1 the dropped limbs in the order of the steps, rows d..n-1 the kept limbs 0..n-d-1;
// a row holds q, X, Shoup(X), then for k < d: W_k, Shoup(W_k), Cn_k (zero beyond the row's own s).  modT: three more words at the end,
// t, floor(2^64 / t) and q[0] mod t, for the centred residue modulo t of the one limb that is left (NativeVector::Mod).
inline std::vector<uint64_t> mod_reduce_chain_table(const uint64_t* q, uint32_t n, uint32_t d, uint64_t t, bool modT) {
    const size_t stride = 3 + 3 * (size_t)d;
    std::vector<uint64_t> tab(n * stride + (modT ? 3 : 0), 0);
    std::vector<uint64_t> suffix(d + 1);
    for (uint32_t r = 0; r < n; ++r) {
        const bool dropped = r < d;
        const uint32_t s   = dropped ? r : d;
        const uint64_t qr  = q[dropped ? n - 1 - r : r - d];
        const uint64_t M   = dropped ? (qr - invmod(t % qr, qr)) % qr : 1;
        const uint64_t MT  = mulmod(M, t % qr, qr);
        suffix[s]          = 1;  // prod_{k<=j<s} B_j
        for (uint32_t k = s; k-- > 0;)
            suffix[k] = mulmod(suffix[k + 1], dropped_inv(q[n - 1 - k], qr), qr);
        uint64_t* row = &tab[r * stride];
        const uint64_t X = mulmod(M, suffix[0], qr);
        row[0] = qr, row[1] = X, row[2] = shoup(X, qr);
        for (uint32_t k = 0; k < s; ++k) {
            const uint64_t W = mulmod(MT, suffix[k], qr);
            row[3 + 3 * k] = W, row[4 + 3 * k] = shoup(W, qr);
            row[5 + 3 * k] = (qr - mulmod(q[n - 1 - k] % qr, W, qr)) % qr;
        }
    }
    if (modT) {
        uint64_t* tail = &tab[n * stride];
        tail[0] = t, tail[1] = shoup(1, t), tail[2] = q[0] % t;
    }
    return tab;
}
// A[i] == -B[i] mod q[i], B reduced: the pair for which x*B + r*A == (x - r)*B
inline bool negated_pair(const uint64_t* q, const uint64_t* A, const uint64_t* B, uint32_t n) {
    bool ok = true;
    for (uint32_t i = 0; i < n; ++i)
        ok = ok && B[i] < q[i] && A[i] == (q[i] - B[i]) % q[i];
    return ok;
}
// B holds the true inverses `own` (dropped_inv of the same moduli), none of them the zero of an equal modulus
inline bool true_inverses(const uint64_t* own, const uint64_t* B, uint32_t n) {
    bool ok = true;
    for (uint32_t i = 0; i < n; ++i)
        ok = ok && own[i] != 0 && B[i] == own[i];
    return ok;
}

// Constants of a rescale by d limbs in one pass (LeveledSHECKKSRNS::ModReduceInternalInPlace, ckksrns-leveledshe.cpp:172-191, as one
// step).  qDrop[k]: the modulus dropped at step k (the last limb first), qKeep[i]: the limbs that are produced,
// sKeep / sDrop: residues of the scalar the tower is multiplied by first (null: none; every sKeep[i] must be non-zero).
//   B[k][j]  = qDrop[k]^-1 mod qDrop[j], k < j                       the triangle of the coefficient-domain chain
//   W[k][i]  = sKeep[i]^-1 * prod_{j<k} qDrop[j] mod qKeep[i]        weight of chain row k in the column pass's load
//   C[i]     = sKeep[i] * prod_k qDrop[k]^-1 mod qKeep[i]            constant of the row pass's store (A - r) * C
// so that (x_i - NTT(sum_k SM(r_k) * W[k][i])) * C[i] = x_i * s_i * prod_k B[k][i] - NTT(sum_k SM(r_k) * prod_{j>=k} B[j][i]).
// Every entry comes with its Shoup companion: out arrays hold {value, shoup(value)} pairs, B as [d][d] (entries k >= j zero), W as [d][nKeep].
inline void rescale_multi_tables(const uint64_t* qDrop, uint32_t d, const uint64_t* qKeep, uint32_t nKeep, const uint64_t* sDrop,
                                 const uint64_t* sKeep, uint64_t* B, uint64_t* W, uint64_t* C, uint64_t* S) {
    for (uint32_t k = 0; k < d; ++k) {
        for (uint32_t j = 0; j < d; ++j) {
            const uint64_t v       = k < j ? invmod(qDrop[k] % qDrop[j], qDrop[j]) : 0;
            B[2 * (k * d + j)]     = v;
            B[2 * (k * d + j) + 1] = k < j ? shoup(v, qDrop[j]) : 0;
        }
        const uint64_t s = sDrop ? sDrop[k] : 1;
        S[2 * k] = s, S[2 * k + 1] = shoup(s, qDrop[k]);
    }
    for (uint32_t i = 0; i < nKeep; ++i) {
        const uint64_t qi = qKeep[i];
        uint64_t w        = sKeep ? invmod(sKeep[i], qi) : 1 % qi;
        uint64_t cst      = sKeep ? sKeep[i] : 1 % qi;
        for (uint32_t k = 0; k < d; ++k) {
            W[2 * ((size_t)k * nKeep + i)]     = w;
            W[2 * ((size_t)k * nKeep + i) + 1] = shoup(w, qi);
            w                                  = mulmod(w, qDrop[k] % qi, qi);
            cst                                = mulmod(cst, invmod(qDrop[k] % qi, qi), qi);
        }
        C[2 * i] = cst, C[2 * i + 1] = shoup(cst, qi);
    }
}
// The BGV twin: d DCRTPolyImpl::ModReduce steps (dcrtpoly-impl.h:736-755) with plaintext modulus t as one pass, the scalar s of
// LeveledSHEBGVRNS::AdjustLevelsAndDepthInPlace (bgvrns-leveledshe.cpp:83-233) in front.  The tables above with two changes:
//   S[k]    = sDrop[k] * t^-1 mod qDrop[k]                           the chain's rows are the canonical residues of -delta_k
//   W[k][i] = (t mod qKeep[i]) * sKeep[i]^-1 * prod_{j<k} qDrop[j]   the switched rows enter the sum times t
// B and C are unchanged.  t must be invertible modulo every qDrop[k].
inline void mod_reduce_multi_tables(const uint64_t* qDrop, uint32_t d, const uint64_t* qKeep, uint32_t nKeep, uint64_t t,
                                    const uint64_t* sDrop, const uint64_t* sKeep, uint64_t* B, uint64_t* W, uint64_t* C, uint64_t* S) {
    rescale_multi_tables(qDrop, d, qKeep, nKeep, sDrop, sKeep, B, W, C, S);
    for (uint32_t k = 0; k < d; ++k) {
        S[2 * k]     = mulmod(S[2 * k], invmod(t % qDrop[k], qDrop[k]), qDrop[k]);
        S[2 * k + 1] = shoup(S[2 * k], qDrop[k]);
    }
    for (uint32_t k = 0; k < d; ++k)
        for (uint32_t i = 0; i < nKeep; ++i) {
            uint64_t* w = &W[2 * ((size_t)k * nKeep + i)];
            w[0] = mulmod(w[0], t % qKeep[i], qKeep[i]), w[1] = shoup(w[0], qKeep[i]);
        }
}

// The factor table of a BV evaluation key over moduli q[0..sizeQ) with digit size baseBits (KeySwitchBV::KeySwitchGenInternal,
// keyswitch-bv.cpp:49-225): tower d of the key carries sOld's limb i times one power of the base at row i and nothing of sOld elsewhere,
//   factor[d][i] = 2^(baseBits * k) mod q_i   when tower d is window k of limb i (PolyImpl::PowersOfBase, poly-impl.h:559-571),   else 0,
// towers in the order of DCRTPolyImpl::CRTDecompose (limb 0's windows, least significant first, then limb 1's ...), ceil(GetMSB(q_i) /
// baseBits) windows per limb; baseBits == 0: one tower per limb with factor 1.  Returns the tower count D_0 and fills factor [D_0][sizeQ];
// 0 and an empty table outside the device path of fhe_crt_decompose_towers (baseBits > 31, a window beyond the 64-bit word, no limbs).
inline uint32_t bv_keygen_factors(const uint64_t* q, uint32_t sizeQ, uint32_t baseBits, std::vector<uint64_t>& factor) {
    factor.clear();
    if (!q || sizeQ < 1 || baseBits > 31)
        return 0;
    std::vector<uint32_t> windows(sizeQ);
    uint32_t towers = 0;
    for (uint32_t i = 0; i < sizeQ; ++i) {
        const uint32_t nBits = bitlen(q[i]);
        windows[i]           = baseBits ? nBits / baseBits + (nBits % baseBits != 0) : 1;
        if ((uint64_t)windows[i] * baseBits > 64)
            return 0;
        towers += windows[i];
    }
    factor.assign((size_t)towers * sizeQ, 0);
    for (uint32_t i = 0, d = 0; i < sizeQ; ++i)
        for (uint32_t k = 0; k < windows[i]; ++k, ++d)
            factor[(size_t)d * sizeQ + i] = powmod(2, (uint64_t)baseBits * k, q[i]);
    return towers;
}

}  // namespace host
}  // namespace fhe
#endif
