// keygen_kernels.h — the streaming pass of key generation (an HBM-bound stream like those of elemwise_kernels.h).
//
// Replaces the per-digit, per-limb loop of KeySwitchHYBRID::KeySwitchGenInternal (src/pke/lib/keyswitch/keyswitch-hybrid.cpp:98-123:
// `b.SetElementAtIndex(i, (-ai * sni) + (ns * ei) [+ (PModq[i] * soi)])`), the permuted secret of
// LeveledSHEBase::EvalAutomorphismKeyGen (src/pke/lib/schemebase/base-leveledshe.cpp:336-379) and `b = ns*e - a*s` of
// PKEBase::KeyGenInternal (src/pke/lib/schemebase/base-pke.cpp:47-98) for any number of keys in ONE launch:
//
//   out[key][j][i][n] = ns_i * e[key][j][i][n] - a[key][j][i][n] * sNew[i][pi_kNew[key](n)] + f[j][i] * sOld[i][pi_kOld[key](n)]   mod q_i
//
// All towers EVALUATION, all residues canonical on entry and on return.  pi_k is the EVALUATION-format automorphism map of
// automorph_kernel (elemwise_kernels.h: automorph_source); k = 1 reads the secret row in place.
//
// Work decomposition: a workgroup owns one (key, limb row, tile of 2048 coefficients) and walks the nParts digits inside it.  A lane
// holds 4 pairs of coefficients: it gathers its words of the two secret rows ONCE, keeps them in registers, and then streams a, e and
// out of every digit with 16-byte accesses (a full wave instruction is 1 KiB, coalesced).  The gather moves 16-byte pairs as well: for
// an even n the sources of n and n + 1 are the two words of one aligned pair (bitrev(n + 1) = bitrev(n) + N/2, and N/2 * k = N/2 mod N
// for odd k flips the top bit of the index, i.e. the bottom bit of its bit reversal), possibly swapped.
// A lane reads its words of e before it writes its words of out and no other lane touches them: out may be e itself.
#ifndef FHE_KEYGEN_KERNELS_H
#define FHE_KEYGEN_KERNELS_H
#include "elemwise_kernels.h"

namespace fhe {

constexpr int kKeygenTileLog = 11;                                  // coefficients of a limb row per workgroup (rings below that: the row)
constexpr int kKeygenPairs   = (1 << kKeygenTileLog) / (2 * kThreads);  // 16-byte pairs per lane
constexpr int kKeygenKeys    = 256;  // keys per launch: their automorphism indices travel by value (2 KiB of the 4 KiB of kernel arguments)

struct KeygenArgs {
    uint64_t* out;                     // [nKeys][nParts][nLimbs][N]
    const uint64_t *a, *e;             // [nKeys][nParts][nLimbs][N]
    const uint64_t *sNew, *sOld;       // [nLimbs][N]; sOld is read only in rows that have a non-zero factor
    const LimbConst* lc;               // [ctxLimbs]
    // Shoup pairs (device): HAS_OLD: f[nParts][nLimbs]; then, unless NS1, ns mod q_i [nLimbs]
    const TwPair* tab;
    uint32_t logN, nLimbs, nParts, nKeys;
    uint32_t kNew[kKeygenKeys], kOld[kKeygenKeys];
    LimbSel sel;
};

// the words pi_k(n), pi_k(n + 1) of a secret row for an even n
FHE_HD void keygen_secret_pair(const uint64_t* row, uint32_t n, uint32_t k, uint32_t logN, uint64_t& s0, uint64_t& s1) {
    // (64-bit indices: p + 1 cannot wrap, so the two words are one 16-byte access)
    const uint32_t src = k == 1u ? n : automorph_source(bitrev32(n, logN), k, logN);
    const uint64_t p   = src & ~1u;
    const uint64_t lo = row[p], hi = row[p + 1];
    s0 = (src & 1u) ? hi : lo;
    s1 = (src & 1u) ? lo : hi;
}

template <bool NS1, bool HAS_OLD>
FHE_GLOBAL void FHE_LAUNCH_BOUNDS(kThreads) keygen_combine_kernel(const KeygenArgs g) {
    const uint32_t t           = FHE_TID;
    const uint32_t tileLog     = g.logN < (uint32_t)kKeygenTileLog ? g.logN : (uint32_t)kKeygenTileLog;
    const uint32_t tilesPerRow = 1u << (g.logN - tileLog);
    const uint32_t tile        = FHE_BID & (tilesPerRow - 1u);
    const uint32_t keyRow      = FHE_BID >> (g.logN - tileLog);
    const uint32_t row = keyRow % g.nLimbs, key = keyRow / g.nLimbs;
    if (key >= g.nKeys)
        return;
    const LimbConst lc = g.lc[g.sel.idx[row]];
    const uint64_t q   = lc.q;
    const int msb      = (int)lc.msb;
    const TwPair* f    = g.tab + row;  // f[j * nLimbs]: the factor of digit j
    bool old           = false;
    if (HAS_OLD)
        for (uint32_t j = 0; j < g.nParts; ++j)
            old |= f[(size_t)j * g.nLimbs].w != 0;
    const TwPair ns = NS1 ? TwPair{1, 0} : g.tab[(size_t)(HAS_OLD ? g.nParts : 0u) * g.nLimbs + row];
    const uint32_t kN = g.kNew[key], kO = g.kOld[key];
    const uint64_t* sN = g.sNew + ((uint64_t)row << g.logN);
    const uint64_t* sO = g.sOld + ((uint64_t)row << g.logN);

    uint64_t sn[kKeygenPairs][2], so[kKeygenPairs][2];
#pragma unroll
    for (int m = 0; m < kKeygenPairs; ++m) {
        const uint32_t in = ((uint32_t)m * kThreads + t) << 1;
        sn[m][0] = sn[m][1] = so[m][0] = so[m][1] = 0;
        if (in >= (1u << tileLog))
            continue;
        const uint32_t n = (tile << tileLog) + in;
        keygen_secret_pair(sN, n, kN, g.logN, sn[m][0], sn[m][1]);
        if (HAS_OLD && old)
            keygen_secret_pair(sO, n, kO, g.logN, so[m][0], so[m][1]);
    }
    for (uint32_t j = 0; j < g.nParts; ++j) {
        const uint64_t base = ((((uint64_t)key * g.nParts + j) * g.nLimbs + row) << g.logN) + ((uint64_t)tile << tileLog);
        TwPair fj           = {0, 0};
        if (HAS_OLD)
            fj = f[(size_t)j * g.nLimbs];
#pragma unroll
        for (int m = 0; m < kKeygenPairs; ++m) {
            const uint32_t in = ((uint32_t)m * kThreads + t) << 1;
            if (in >= (1u << tileLog))
                continue;
            const uint64_t off = base + in;
            const uint64_t a0 = g.a[off], a1 = g.a[off + 1];
            uint64_t e0 = g.e[off], e1 = g.e[off + 1];
            if (!NS1) {
                e0 = mul_shoup(e0, ns.w, ns.wp, q);
                e1 = mul_shoup(e1, ns.w, ns.wp, q);
            }
            uint64_t r0 = sub_mod(e0, mul_mod_barrett(a0, sn[m][0], q, lc.mu, msb), q);
            uint64_t r1 = sub_mod(e1, mul_mod_barrett(a1, sn[m][1], q, lc.mu, msb), q);
            if (HAS_OLD && fj.w != 0) {
                r0 = add_mod(r0, mul_shoup(so[m][0], fj.w, fj.wp, q), q);
                r1 = add_mod(r1, mul_shoup(so[m][1], fj.w, fj.wp, q), q);
            }
            g.out[off]     = r0;
            g.out[off + 1] = r1;
        }
    }
}

}  // namespace fhe
#endif
