// encrypt_kernels.h — the streaming pass of encryption (an HBM-bound stream like those of elemwise_kernels.h and keygen_kernels.h).
//
// Replaces the element arithmetic of PKERNS::EncryptZeroCore in both forms (src/pke/lib/schemerns/rns-pke.cpp:111-197) and the
// `(*ba)[0] += ptxt` of PKERNS::Encrypt (:40-70) for any number of ciphertexts in ONE launch.  For ciphertext t < batch, tower row
// i < nLimbs, word n:
//
//   public key (:148-197: `c0 = p0 * v + ns * e0`, `c1 = p1 * v + ns * e1`):
//     c0[t][i][n] = pkB[i][n] * v[t][i][n] + ns_i * e0[t][i][n] (+ m[t][i][n])
//     c1[t][i][n] = pkA[i][n] * v[t][i][n] + ns_i * e1[t][i][n]                       mod q_i
//   secret key (:111-146: `c0 = a * s + ns * e`, `c1 = -a`):
//     c0[t][i][n] = a[t][i][n] * s[i][n] + ns_i * e[t][i][n] (+ m[t][i][n])
//     c1[t][i][n] = -a[t][i][n]                                                       mod q_i
//
// All towers EVALUATION, all residues canonical on entry and on return.  The key rows are [nLimbs][N], aligned with the tower rows: the
// first rows of a full-level key serve a plaintext with fewer limbs (the reference's DropLastElements on the clones, :171-180).
//
// Work decomposition, as in keygen_kernels.h: a workgroup owns one (limb row, tile of 2048 coefficients, chunk of ciphertexts).  A lane
// holds 4 pairs of coefficients: it loads its words of pkB and pkA (or s) ONCE, keeps them in registers, and then streams v, e0, e1
// (and m) in and c0, c1 out for every ciphertext of the chunk with 16-byte accesses (a full wave instruction is 1 KiB, coalesced).  The
// key rows are the words read again and again: a chunk of c ciphertexts reads them once per c.  The host chooses the chunk
// (encrypt_chunk) so that a small batch still fills the part; the last chunk of a batch may be short.
// A lane reads its words of v, e0, e1 before it writes its words of c0, c1 and no other lane touches them: c0 may be e0 (or e) and c1
// may be e1 (or a).
#ifndef FHE_ENCRYPT_KERNELS_H
#define FHE_ENCRYPT_KERNELS_H
#include "keygen_kernels.h"

namespace fhe {

constexpr int kEncryptTileLog  = kKeygenTileLog;                            // coefficients of a limb row per workgroup (rings below that: the row)
constexpr int kEncryptPairs    = (1 << kEncryptTileLog) / (2 * kThreads);   // 16-byte pairs per lane
constexpr int kEncryptMaxChunk = 8;  // ciphertexts per workgroup at most: the key rows then add 2 / (8 * 5) = 5 % to the words moved

struct EncryptArgs {
    uint64_t *c0, *c1;          // [batch][nLimbs][N]
    const uint64_t *k0, *k1;    // [nLimbs][N]: pkB, pkA; secret-key form: s (k1 is not read)
    const uint64_t* v;          // [batch][nLimbs][N]: v; secret-key form: a
    const uint64_t *e0, *e1;    // [batch][nLimbs][N]; secret-key form: e (e1 is not read)
    const uint64_t* msg;        // [batch][nLimbs][N], HAS_MSG only
    const LimbConst* lc;        // [ctxLimbs]
    const TwPair* tab;          // Shoup pairs (device) of ns mod q_i [nLimbs], unless NS1
    uint32_t logN, nLimbs, batch, chunk;
    LimbSel sel;
};

// ciphertexts a workgroup walks: the largest power of two <= kEncryptMaxChunk that still leaves `minGroups` workgroups
FHE_HD uint32_t encrypt_chunk(uint64_t rowsTimesTiles, uint32_t batch, uint64_t minGroups) {
    uint32_t chunk = (uint32_t)kEncryptMaxChunk;
    while (chunk > 1 && rowsTimesTiles * ((batch + chunk - 1) / chunk) < minGroups)
        chunk >>= 1;
    return chunk;
}

template <bool NS1, bool HAS_MSG, bool SK>
FHE_GLOBAL void FHE_LAUNCH_BOUNDS(kThreads) encrypt_combine_kernel(const EncryptArgs g) {
    const uint32_t t           = FHE_TID;
    const uint32_t tileLog     = g.logN < (uint32_t)kEncryptTileLog ? g.logN : (uint32_t)kEncryptTileLog;
    const uint32_t tilesPerRow = 1u << (g.logN - tileLog);
    const uint32_t tile        = FHE_BID & (tilesPerRow - 1u);
    const uint32_t chunkRow    = FHE_BID >> (g.logN - tileLog);
    const uint32_t row = chunkRow % g.nLimbs, first = (chunkRow / g.nLimbs) * g.chunk;
    if (first >= g.batch)
        return;
    const uint32_t last = first + g.chunk < g.batch ? first + g.chunk : g.batch;
    const LimbConst lc  = g.lc[g.sel.idx[row]];
    const uint64_t q    = lc.q;
    const int msb       = (int)lc.msb;
    const TwPair ns     = NS1 ? TwPair{1, 0} : g.tab[row];
    const uint64_t rowBase = ((uint64_t)row << g.logN) + ((uint64_t)tile << tileLog);

    uint64_t kb[kEncryptPairs][2], ka[kEncryptPairs][2];
#pragma unroll
    for (int m = 0; m < kEncryptPairs; ++m) {
        const uint32_t in = ((uint32_t)m * kThreads + t) << 1;
        kb[m][0] = kb[m][1] = ka[m][0] = ka[m][1] = 0;
        if (in >= (1u << tileLog))
            continue;
        kb[m][0] = g.k0[rowBase + in], kb[m][1] = g.k0[rowBase + in + 1];
        if (!SK)
            ka[m][0] = g.k1[rowBase + in], ka[m][1] = g.k1[rowBase + in + 1];
    }
    for (uint32_t ct = first; ct < last; ++ct) {
        const uint64_t base = (((uint64_t)ct * g.nLimbs) << g.logN) + rowBase;
#pragma unroll
        for (int m = 0; m < kEncryptPairs; ++m) {
            const uint32_t in = ((uint32_t)m * kThreads + t) << 1;
            if (in >= (1u << tileLog))
                continue;
            const uint64_t off = base + in;
            const uint64_t v0 = g.v[off], v1 = g.v[off + 1];
            uint64_t x0 = g.e0[off], x1 = g.e0[off + 1];
            uint64_t y0 = 0, y1 = 0;
            if (!SK)
                y0 = g.e1[off], y1 = g.e1[off + 1];
            if (!NS1) {
                x0 = mul_shoup(x0, ns.w, ns.wp, q);
                x1 = mul_shoup(x1, ns.w, ns.wp, q);
                if (!SK) {
                    y0 = mul_shoup(y0, ns.w, ns.wp, q);
                    y1 = mul_shoup(y1, ns.w, ns.wp, q);
                }
            }
            uint64_t r0 = add_mod(mul_mod_barrett(v0, kb[m][0], q, lc.mu, msb), x0, q);
            uint64_t r1 = add_mod(mul_mod_barrett(v1, kb[m][1], q, lc.mu, msb), x1, q);
            if (HAS_MSG) {
                r0 = add_mod(r0, g.msg[off], q);
                r1 = add_mod(r1, g.msg[off + 1], q);
            }
            uint64_t s0, s1;
            if (SK) {
                s0 = v0 == 0 ? 0 : q - v0;
                s1 = v1 == 0 ? 0 : q - v1;
            } else {
                s0 = add_mod(mul_mod_barrett(v0, ka[m][0], q, lc.mu, msb), y0, q);
                s1 = add_mod(mul_mod_barrett(v1, ka[m][1], q, lc.mu, msb), y1, q);
            }
            g.c0[off]     = r0;
            g.c0[off + 1] = r1;
            g.c1[off]     = s0;
            g.c1[off + 1] = s1;
        }
    }
}

}  // namespace fhe
#endif
