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

// ---- the public-key form of a BV evaluation key ----
// KeySwitchBV::KeySwitchGenInternal(oldSk, newPk) (src/pke/lib/keyswitch/keyswitch-bv.cpp:162-225), what PREBase::ReKeyGen
// (src/pke/lib/schemebase/base-pre.cpp:42-45) calls, for any number of keys in ONE launch: for key < nKeys, tower d < nParts, row i, word n
//
//   outB[key][d][i][n] = p0[key][i][n] * u[key][d][i][n] + ns_i * e0[key][d][i][n] + f[d][i] * sOld[i][n]
//   outA[key][d][i][n] = p1[key][i][n] * u[key][d][i][n] + ns_i * e1[key][d][i][n]                             mod q_i
//
// (one public key for all keys when !pkPerKey).  It is an encryption of f[d] * sOld under the new public key, tower by tower, whose
// "message" is non-zero in one row per tower only and therefore never materialised.  The work decomposition of the kernel above: a
// workgroup owns one (key, limb row, tile of 2048 coefficients), holds its words of p0, p1 and sOld in registers (4 pairs per lane: 24
// words) and walks the towers, streaming u, e0, e1 in and outB, outA out with 16-byte accesses.  sOld is read only in rows where some tower
// of the walk has a non-zero factor.  When keys x rows x tiles alone would leave fewer than four workgroups per compute unit the host cuts
// the walk into `pieces` (towers [piece * chunk, piece * chunk + chunk) per workgroup; the key rows then come from L2 once per piece);
// pieces == 1 is the whole walk.
// A lane reads its words of u, e0, e1 before it writes its words of outB, outA and no other lane touches them: outB may be e0 and outA
// may be e1.
struct KeygenPkArgs {
    uint64_t *outB, *outA;        // [nKeys][nParts][nLimbs][N]
    const uint64_t *p0, *p1;      // [pkPerKey ? nKeys : 1][nLimbs][N]
    const uint64_t* sOld;         // [nLimbs][N]; read only in rows that have a non-zero factor
    const uint64_t *u, *e0, *e1;  // [nKeys][nParts][nLimbs][N]
    const LimbConst* lc;          // [ctxLimbs]
    const TwPair* tab;            // Shoup pairs (device): f[nParts][nLimbs]; then, unless NS1, ns mod q_i [nLimbs]
    uint32_t logN, nLimbs, nParts, nKeys, pkPerKey;
    uint32_t pieces, chunk;       // the tower walk in `pieces` parts of `chunk` towers (the last one may be short)
    LimbSel sel;
};

template <bool NS1>
FHE_GLOBAL void FHE_LAUNCH_BOUNDS(kThreads) keygen_pk_combine_kernel(const KeygenPkArgs g) {
    const uint32_t t           = FHE_TID;
    const uint32_t tileLog     = g.logN < (uint32_t)kKeygenTileLog ? g.logN : (uint32_t)kKeygenTileLog;
    const uint32_t tilesPerRow = 1u << (g.logN - tileLog);
    const uint32_t tile        = FHE_BID & (tilesPerRow - 1u);
    const uint32_t pieceRow    = FHE_BID >> (g.logN - tileLog);
    const uint32_t row = pieceRow % g.nLimbs, keyPiece = pieceRow / g.nLimbs;
    const uint32_t piece = keyPiece % g.pieces, key = keyPiece / g.pieces;
    if (key >= g.nKeys)
        return;
    const uint32_t first = piece * g.chunk;
    const uint32_t last  = first + g.chunk < g.nParts ? first + g.chunk : g.nParts;
    const LimbConst lc   = g.lc[g.sel.idx[row]];
    const uint64_t q     = lc.q;
    const int msb        = (int)lc.msb;
    const TwPair* f      = g.tab + row;  // f[d * nLimbs]: the factor of tower d
    bool old             = false;
    for (uint32_t d = first; d < last; ++d)
        old |= f[(size_t)d * g.nLimbs].w != 0;
    const TwPair ns        = NS1 ? TwPair{1, 0} : g.tab[(size_t)g.nParts * g.nLimbs + row];
    const uint64_t rowBase = ((uint64_t)row << g.logN) + ((uint64_t)tile << tileLog);
    const uint64_t pkBase  = (((uint64_t)(g.pkPerKey ? key : 0u) * g.nLimbs) << g.logN) + rowBase;

    uint64_t kb[kKeygenPairs][2], ka[kKeygenPairs][2], so[kKeygenPairs][2];
#pragma unroll
    for (int m = 0; m < kKeygenPairs; ++m) {
        const uint32_t in = ((uint32_t)m * kThreads + t) << 1;
        kb[m][0] = kb[m][1] = ka[m][0] = ka[m][1] = so[m][0] = so[m][1] = 0;
        if (in >= (1u << tileLog))
            continue;
        kb[m][0] = g.p0[pkBase + in], kb[m][1] = g.p0[pkBase + in + 1];
        ka[m][0] = g.p1[pkBase + in], ka[m][1] = g.p1[pkBase + in + 1];
        if (old)
            so[m][0] = g.sOld[rowBase + in], so[m][1] = g.sOld[rowBase + in + 1];
    }
    for (uint32_t d = first; d < last; ++d) {
        const uint64_t base = ((((uint64_t)key * g.nParts + d) * g.nLimbs) << g.logN) + rowBase;
        const TwPair fd     = f[(size_t)d * g.nLimbs];
#pragma unroll
        for (int m = 0; m < kKeygenPairs; ++m) {
            const uint32_t in = ((uint32_t)m * kThreads + t) << 1;
            if (in >= (1u << tileLog))
                continue;
            const uint64_t off = base + in;
            const uint64_t u0 = g.u[off], u1 = g.u[off + 1];
            uint64_t x0 = g.e0[off], x1 = g.e0[off + 1];
            uint64_t y0 = g.e1[off], y1 = g.e1[off + 1];
            if (!NS1) {
                x0 = mul_shoup(x0, ns.w, ns.wp, q);
                x1 = mul_shoup(x1, ns.w, ns.wp, q);
                y0 = mul_shoup(y0, ns.w, ns.wp, q);
                y1 = mul_shoup(y1, ns.w, ns.wp, q);
            }
            uint64_t r0 = add_mod(mul_mod_barrett(u0, kb[m][0], q, lc.mu, msb), x0, q);
            uint64_t r1 = add_mod(mul_mod_barrett(u1, kb[m][1], q, lc.mu, msb), x1, q);
            if (fd.w != 0) {
                r0 = add_mod(r0, mul_shoup(so[m][0], fd.w, fd.wp, q), q);
                r1 = add_mod(r1, mul_shoup(so[m][1], fd.w, fd.wp, q), q);
            }
            const uint64_t s0 = add_mod(mul_mod_barrett(u0, ka[m][0], q, lc.mu, msb), y0, q);
            const uint64_t s1 = add_mod(mul_mod_barrett(u1, ka[m][1], q, lc.mu, msb), y1, q);
            g.outB[off]     = r0;
            g.outB[off + 1] = r1;
            g.outA[off]     = s0;
            g.outA[off + 1] = s1;
        }
    }
}

}  // namespace fhe
#endif
