// blake2_kernels.h — the reference's cryptographic PRNG construction, blake2xb in counter mode, on the device, with the samplers of
// sampler_kernels.h fused onto its output (FHE_HAL_DEVICE_SAMPLER=blake2).
//
// default_prng::Blake2Engine (utils/prng/blake2engine.cpp) draws 4 KiB per Generate(): blake2xb(out 4096 bytes, in = its 64-bit counter
// (8 bytes little-endian), key = its 512-bit seed), then increments the counter.  blake2xb (blake2xb-ref.c) is a BLAKE2b root hash
//   H0       = BLAKE2b-512(param: digest 64, key 64, fanout 1, depth 1, xof_length 4096;  key block, then the counter)
// and 64 independent leaves
//   leaf[i]  = BLAKE2b-512(param: digest 64, fanout 0, depth 0, leaf_length 64, node_offset i, xof_length 4096, inner_length 64;  H0)
// whose concatenation is the 4 KiB block.  Blocks of different counters are independent, and so are the leaves of a block.
//
// Work mapping: one wave walks `walk` (1 ... 64) consecutive counters.  Each of the first `walk` lanes computes H0 for one of them
// (2 compressions) and parks it in LDS; the wave then walks the counters with lane = leaf index (1 compression each): 66 compressions per
// 64 leaves at walk = 64.  The host picks the longest walk that still gives the device enough waves (a uniform key-generation call is 16 K
// blocks, a Gaussian one 256: at walk 64 they would occupy a quarter of the compute units, or one of them).  Every lane turns its
// 64-byte leaf into outputs in registers and stores them: no random buffer goes through HBM, and the result depends only on
// (key, counter0, shape), never on the launch geometry.
//
// The stream S(key, counter0) is the concatenation of the blocks for counters counter0, counter0 + 1, ... (64-bit, with carry): the 32-bit
// words Blake2Engine(key, counter0) returns.  R[i] = S[2i] | S[2i+1] << 32.  Samplers (element e counts from the first word of the call):
//   kind 0 uniform   e = (t * nLimbs + l) * N + j:  (R[2e+1] * 2^64 + R[2e]) mod q_l   (barrett128).  Statistical distance from uniform
//                    at most q / 2^128 < 2^-68 per coefficient; the reference instead rejects candidates of bitlen(q) bits (exact).
//   kind 1 Gaussian  e = t * N + j:  Peikert's inversion of s = (R[e] >> 11) * 2^-53 - 0.5 (peikert_invert, shared with the Philox path)
//   kind 2 ternary   e = t * N + j:  mulhi(R[e], 3) - 1: each outcome within 2^-64 of 1/3
//   kind 3           the raw stream (fhe_blake2xb_stream)
// Gaussian and ternary integers are stored modulo every selected limb, negative k as q - |k| (dcrtpoly-impl.h:126-150).
#ifndef FHE_BLAKE2_KERNELS_H
#define FHE_BLAKE2_KERNELS_H
#include "sampler_kernels.h"

namespace fhe {

constexpr uint64_t kB2IV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                               0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
// message schedule of RFC 7693 (rounds 10 and 11 repeat 0 and 1); only ever read in constant expressions (template arguments), so the
// message words stay in registers
constexpr uint8_t kB2Sigma[12][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};

// rotation right by S on the two 32-bit halves: 32 is a swap, 24, 16 and 63 are two funnel shifts each (v_alignbit_b32 / v_perm_b32;
// the 64-bit form compiles to two 64-bit shifts and an or per half)
template <int S>
FHE_HD uint64_t b2_rotr(uint64_t x) {
    const uint32_t a = (uint32_t)x, b = (uint32_t)(x >> 32);
    const uint32_t lo = S >= 32 ? b : a, hi = S >= 32 ? a : b;
    constexpr int s = S & 31;
    if (s == 0)
        return ((uint64_t)hi << 32) | lo;
    const uint32_t nlo = (lo >> s) | (hi << ((32 - s) & 31)), nhi = (hi >> s) | (lo << ((32 - s) & 31));
    return ((uint64_t)nhi << 32) | nlo;
}
template <int A, int B, int C, int D, int X, int Y>
FHE_HD void b2_g(uint64_t (&v)[16], const uint64_t (&m)[16]) {
    v[A] = v[A] + v[B] + m[X];
    v[D] = b2_rotr<32>(v[D] ^ v[A]);
    v[C] = v[C] + v[D];
    v[B] = b2_rotr<24>(v[B] ^ v[C]);
    v[A] = v[A] + v[B] + m[Y];
    v[D] = b2_rotr<16>(v[D] ^ v[A]);
    v[C] = v[C] + v[D];
    v[B] = b2_rotr<63>(v[B] ^ v[C]);
}
template <int R>
FHE_HD void b2_round(uint64_t (&v)[16], const uint64_t (&m)[16]) {
    constexpr const uint8_t* s = kB2Sigma[R];
    b2_g<0, 4, 8, 12, s[0], s[1]>(v, m);
    b2_g<1, 5, 9, 13, s[2], s[3]>(v, m);
    b2_g<2, 6, 10, 14, s[4], s[5]>(v, m);
    b2_g<3, 7, 11, 15, s[6], s[7]>(v, m);
    b2_g<0, 5, 10, 15, s[8], s[9]>(v, m);
    b2_g<1, 6, 11, 12, s[10], s[11]>(v, m);
    b2_g<2, 7, 8, 13, s[12], s[13]>(v, m);
    b2_g<3, 4, 9, 14, s[14], s[15]>(v, m);
}
// F of RFC 7693 section 3.2: byte counter t < 2^64 (t1 = 0), `last` = the final block of its node (f0 = ~0; f1, the last-node flag, is 0)
FHE_HD void b2_compress(uint64_t (&h)[8], const uint64_t (&m)[16], uint64_t t, bool last) {
    uint64_t v[16];
#pragma unroll
    for (int i = 0; i < 8; ++i)
        v[i] = h[i], v[i + 8] = kB2IV[i];
    v[12] ^= t;
    if (last)
        v[14] = ~v[14];
    b2_round<0>(v, m), b2_round<1>(v, m), b2_round<2>(v, m), b2_round<3>(v, m), b2_round<4>(v, m), b2_round<5>(v, m);
    b2_round<6>(v, m), b2_round<7>(v, m), b2_round<8>(v, m), b2_round<9>(v, m), b2_round<10>(v, m), b2_round<11>(v, m);
#pragma unroll
    for (int i = 0; i < 8; ++i)
        h[i] ^= v[i] ^ v[i + 8];
}
// parameter blocks (words 0..2 of the 64-byte block; the rest, salt and personalisation, is zero)
constexpr uint64_t kB2XofBytes = 4096;
// root: digest 64 | key 64 << 8 | fanout 1 << 16 | depth 1 << 24; node_offset 0 | xof_length << 32
constexpr uint64_t kB2RootP0 = 0x01014040ull, kB2RootP1 = kB2XofBytes << 32;
// leaf: digest 64, leaf_length 64 << 32; node_offset i | xof_length << 32; inner_length 64 << 8
constexpr uint64_t kB2LeafP0 = 0x40ull | (64ull << 32), kB2LeafP2 = 64ull << 8;

// H0 of blake2xb(4096 bytes, in = counter, key): the key block (128 bytes, not final), then the 8-byte counter (final, t = 136)
FHE_HD void b2x_root(uint64_t (&h)[8], const uint32_t (&key)[16], uint64_t counter) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
        h[i] = kB2IV[i];
    h[0] ^= kB2RootP0, h[1] ^= kB2RootP1;
    uint64_t m[16];
#pragma unroll
    for (int i = 0; i < 8; ++i)
        m[i] = (uint64_t)key[2 * i] | ((uint64_t)key[2 * i + 1] << 32), m[i + 8] = 0;
    b2_compress(h, m, 128, false);
#pragma unroll
    for (int i = 0; i < 16; ++i)
        m[i] = 0;
    m[0] = counter;
    b2_compress(h, m, 136, true);
}
// leaf i of the block whose root hash is H0 (bytes 64 i .. 64 i + 63 of the 4 KiB block)
FHE_HD void b2x_leaf(uint64_t (&out)[8], const uint64_t (&h0)[8], uint32_t i) {
#pragma unroll
    for (int w = 0; w < 8; ++w)
        out[w] = kB2IV[w];
    out[0] ^= kB2LeafP0, out[1] ^= (uint64_t)i | (kB2XofBytes << 32), out[2] ^= kB2LeafP2;
    uint64_t m[16];
#pragma unroll
    for (int w = 0; w < 8; ++w)
        m[w] = h0[w], m[w + 8] = 0;
    b2_compress(out, m, 64, true);
}

struct Blake2Args {
    uint32_t key[16];      // the 512-bit key, by value (never in a device buffer)
    uint64_t counter0;     // counter of the call's first block
    uint64_t nBlocks;      // blocks the call covers
    uint64_t total;        // samplers: elements of the call (uniform: batch * nLimbs * N, else batch * N)
    uint64_t* out;
    const uint64_t* q;     // [ctxLimbs]
    const uint64_t* mu128; // [ctxLimbs][2]
    const double* cdf;     // Gaussian: the reference's inversion table (sampler_kernels.h), length cdfLen; a = 1 / (2 * cusum + 1)
    double a;
    uint32_t cdfLen, logN, nLimbs;
    uint32_t walk;         // counters per wave (a power of two, 1 ... 64)
    LimbSel sel;
};
constexpr uint32_t kB2Threads = kThreads;  // 4 waves
constexpr uint32_t kB2MaxWalk = 64;

// one leaf (8 words R[8 * (64 b + lane) ...]) of block b of the call turned into outputs
template <int KIND>
FHE_HD void b2_emit(const Blake2Args& a, const uint64_t (&r)[8], uint64_t b, uint32_t lane) {
    const uint64_t leaf = b * 64 + lane;
    if (KIND == 3) {
#pragma unroll
        for (int w = 0; w < 8; ++w)
            a.out[leaf * 8 + w] = r[w];
    } else if (KIND == 0) {
        const uint64_t e0 = leaf * 4;  // 4 coefficients of one row (N >= 16): the whole group is in range or none of it
        if (e0 >= a.total)
            return;
        const uint32_t l = (uint32_t)((e0 >> a.logN) % a.nLimbs), cl = a.sel.idx[l];
        const uint64_t q = a.q[cl], mulo = a.mu128[2 * cl], muhi = a.mu128[2 * cl + 1];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            a.out[e0 + c] = barrett128(u128w{r[2 * c], r[2 * c + 1]}, q, mulo, muhi);
    } else {
        const uint64_t e0 = leaf * 8;  // 8 coefficients of one tower (N >= 16)
        if (e0 >= a.total)
            return;
        int64_t k[8];
#pragma unroll
        for (int c = 0; c < 8; ++c)
            k[c] = KIND == 1 ? peikert_invert(r[c], a.cdf, a.cdfLen, a.a) : (int64_t)mulhi64(r[c], 3) - 1;
        const uint64_t t = e0 >> a.logN, j = e0 & ((1ull << a.logN) - 1);
        for (uint32_t l = 0; l < a.nLimbs; ++l) {
            const uint64_t q = a.q[a.sel.idx[l]];
            uint64_t* o      = a.out + ((t * a.nLimbs + l) << a.logN) + j;
#pragma unroll
            for (int c = 0; c < 8; ++c)
                o[c] = k[c] < 0 ? q - (uint64_t)(-k[c]) : (uint64_t)k[c];
        }
    }
}

// grid: ceil(nBlocks / (4 walk)) workgroups of kB2Threads lanes; wave w of workgroup g walks blocks (4 g + w) walk ... + walk - 1
template <int KIND>
FHE_GLOBAL void FHE_LAUNCH_BOUNDS(kB2Threads) blake2xb_kernel(const Blake2Args a) {
    FHE_SHARED_U64(roots, (kB2Threads / 64) * kB2MaxWalk * 8);
    const uint32_t lane = FHE_TID & 63u, wave = FHE_TID >> 6;
    const uint64_t base = ((uint64_t)FHE_BID * (kB2Threads / 64) + wave) * a.walk;
    const uint32_t nb   = base >= a.nBlocks ? 0u : (uint32_t)(a.nBlocks - base < a.walk ? a.nBlocks - base : a.walk);
    uint64_t* mine      = roots + (size_t)wave * kB2MaxWalk * 8;
    if (lane < nb) {
        uint64_t h[8];
        b2x_root(h, a.key, a.counter0 + base + lane);
#pragma unroll
        for (int w = 0; w < 8; ++w)
            mine[lane * 8 + w] = h[w];
    }
    FHE_WAVE_SYNC();
    for (uint32_t k = 0; k < nb; ++k) {
        uint64_t h0[8], r[8];
#pragma unroll
        for (int w = 0; w < 8; ++w)
            h0[w] = mine[k * 8 + w];
        b2x_leaf(r, h0, lane);
        b2_emit<KIND>(a, r, base + k, lane);
    }
}

}  // namespace fhe
#endif
