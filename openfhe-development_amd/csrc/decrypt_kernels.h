// decrypt_kernels.h — the streaming pass of decryption (an HBM-bound stream like those of encrypt_kernels.h and keygen_kernels.h).
//
// Replaces PKERNS::DecryptCore (src/pke/lib/schemerns/rns-pke.cpp:199-225: `b = cv[0]`, then `b += sPower * cv[i]; sPower *= s` from
// sPower = s), CKKS's `b += noise` under NOISE_FLOODING_DECRYPT and the element arithmetic of MultipartyDecryptLead / MultipartyDecryptMain
// (src/pke/lib/schemerns/rns-multiparty.cpp:46-171: `b = cv[0] + s * cv[1] + ns * e`, `b = s * cv[1] + ns * e`) for any number of
// ciphertexts in ONE launch.  For ciphertext t < batch, tower row i < nLimbs, word n:
//
//   b[t][i][n] = [c0[t][i][n]] + s[i][n] * c1[t][i][n] + s[i][n]^2 * c2[t][i][n] + ... [+ ns_i * e[t][i][n]]   mod q_i
//
// evaluated by Horner, ((c_k * s + c_{k-1}) * s + ...) * s + c0: residues are exact, so the words are those of the reference's loop over
// powers of s, and no tower of s^2 exists anywhere.  All towers EVALUATION, all residues canonical on entry and on return.  s is
// [nLimbs][N], aligned with the tower rows: the first rows of a full-level key serve a ciphertext with fewer limbs (DropLastElements on
// the copy of the key, :203-206).
//
// Work decomposition, as in encrypt_kernels.h: a workgroup owns one (limb row, tile of 2048 coefficients, chunk of ciphertexts).  A lane
// holds 4 pairs of coefficients: it loads its words of s ONCE, keeps them in registers, and then streams the elements (and the noise) in
// and b out for every ciphertext of the chunk with 16-byte accesses.  The host chooses the chunk (decrypt_chunk == encrypt_chunk) so
// that a small batch still fills the part; the last chunk of a batch may be short.
// A lane reads its words of every input before it writes its words of b and no other lane touches them: out may be c[0] or the noise.
#ifndef FHE_DECRYPT_KERNELS_H
#define FHE_DECRYPT_KERNELS_H
#include "encrypt_kernels.h"

namespace fhe {

constexpr int kDecryptTileLog  = kEncryptTileLog;                           // coefficients of a limb row per workgroup (rings below that: the row)
constexpr int kDecryptPairs    = (1 << kDecryptTileLog) / (2 * kThreads);   // 16-byte pairs per lane
constexpr int kDecryptMaxChunk = kEncryptMaxChunk;  // ciphertexts per workgroup at most: s then adds 1 / (8 * 3) = 4 % to the words moved
constexpr int kDecryptMaxElems = 4;

// the noise term of an instantiation
constexpr int kDecryptNoNoise = 0, kDecryptNoiseNs1 = 1, kDecryptNoiseScaled = 2;

struct DecryptArgs {
    uint64_t* out;                       // [batch][nLimbs][N]
    const uint64_t* c[kDecryptMaxElems]; // [batch][nLimbs][N] each; c[0] is not read without C0
    const uint64_t* s;                   // [nLimbs][N]
    const uint64_t* noise;               // [batch][nLimbs][N], NOISE != kDecryptNoNoise only
    const LimbConst* lc;                 // [ctxLimbs]
    const TwPair* tab;                   // Shoup pairs (device) of ns mod q_i [nLimbs], kDecryptNoiseScaled only
    uint32_t logN, nLimbs, batch, chunk;
    LimbSel sel;
};

FHE_HD uint32_t decrypt_chunk(uint64_t rowsTimesTiles, uint32_t batch, uint64_t minGroups) {
    return encrypt_chunk(rowsTimesTiles, batch, minGroups);
}

template <int NELEM, bool C0, int NOISE>
FHE_GLOBAL void FHE_LAUNCH_BOUNDS(kThreads) decrypt_combine_kernel(const DecryptArgs g) {
    static_assert(NELEM >= 2 && NELEM <= kDecryptMaxElems, "2 to 4 elements");
    const uint32_t t           = FHE_TID;
    const uint32_t tileLog     = g.logN < (uint32_t)kDecryptTileLog ? g.logN : (uint32_t)kDecryptTileLog;
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
    const TwPair ns     = NOISE == kDecryptNoiseScaled ? g.tab[row] : TwPair{1, 0};
    const uint64_t rowBase = ((uint64_t)row << g.logN) + ((uint64_t)tile << tileLog);

    uint64_t sk[kDecryptPairs][2];
#pragma unroll
    for (int m = 0; m < kDecryptPairs; ++m) {
        const uint32_t in = ((uint32_t)m * kThreads + t) << 1;
        sk[m][0] = sk[m][1] = 0;
        if (in >= (1u << tileLog))
            continue;
        sk[m][0] = g.s[rowBase + in], sk[m][1] = g.s[rowBase + in + 1];
    }
    for (uint32_t ct = first; ct < last; ++ct) {
        const uint64_t base = (((uint64_t)ct * g.nLimbs) << g.logN) + rowBase;
#pragma unroll
        for (int m = 0; m < kDecryptPairs; ++m) {
            const uint32_t in = ((uint32_t)m * kThreads + t) << 1;
            if (in >= (1u << tileLog))
                continue;
            const uint64_t off = base + in;
            uint64_t x[NELEM][2];
#pragma unroll
            for (int e = C0 ? 0 : 1; e < NELEM; ++e)
                x[e][0] = g.c[e][off], x[e][1] = g.c[e][off + 1];
            uint64_t n0 = 0, n1 = 0;
            if (NOISE != kDecryptNoNoise)
                n0 = g.noise[off], n1 = g.noise[off + 1];
            uint64_t r0 = x[NELEM - 1][0], r1 = x[NELEM - 1][1];
#pragma unroll
            for (int e = NELEM - 2; e >= 0; --e) {
                r0 = mul_mod_barrett(r0, sk[m][0], q, lc.mu, msb);
                r1 = mul_mod_barrett(r1, sk[m][1], q, lc.mu, msb);
                if (e > 0 || C0) {
                    r0 = add_mod(r0, x[e][0], q);
                    r1 = add_mod(r1, x[e][1], q);
                }
            }
            if (NOISE == kDecryptNoiseScaled) {
                n0 = mul_shoup(n0, ns.w, ns.wp, q);
                n1 = mul_shoup(n1, ns.w, ns.wp, q);
            }
            if (NOISE != kDecryptNoNoise) {
                r0 = add_mod(r0, n0, q);
                r1 = add_mod(r1, n1, q);
            }
            g.out[off]     = r0;
            g.out[off + 1] = r1;
        }
    }
}

}  // namespace fhe
#endif
