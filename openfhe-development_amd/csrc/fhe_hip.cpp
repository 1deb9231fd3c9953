// fhe_hip.cpp — implementation of the C ABI in include/fhe_hip.h (compiled by hipcc for gfx950).
//
// Host logic only: contexts (device twiddle tables), the passes of the NTT and their kernels, conversion / key-switch
// plans (tables as CryptoParametersRNS::PrecomputeCRTTables builds them,
// src/pke/lib/schemerns/rns-cryptoparameters.cpp:80-350) and the launch sequences that replace
// KeySwitchHYBRID (src/pke/lib/keyswitch/keyswitch-hybrid.cpp:308-435), ApproxModDown
// (src/core/include/lattice/hal/default/dcrtpoly-impl.h:966-1005) and DropLastElementAndScale (:693-712).
// All arithmetic runs in the kernels of ntt_kernels.h / elemwise_kernels.h / basis_kernels.h.
#include "../../include/fhe_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "basis_kernels.h"
#include "bfv_kernels.h"
#include "elemwise_kernels.h"
#include "host_math.h"
#include "keygen_kernels.h"
#include "encrypt_kernels.h"
#include "decrypt_kernels.h"
#include "ntt_kernels.h"
#include "ntt_static.h"
#include "ntt_row8.h"
#include "rt.h"
#include "sampler_kernels.h"
#include "blake2_kernels.h"

using namespace fhe;

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_lastError;
static fhe_status fail(fhe_status code, const std::string& msg) {
    g_lastError = msg;
    return code;
}
#define RT_CHECK(expr)                                                                  \
    do {                                                                                \
        const char* _e = (expr);                                                        \
        if (_e)                                                                         \
            return fail(FHE_ERR_DEVICE, std::string(#expr) + ": " + _e);                \
    } while (0)
#define ARG_CHECK(cond, msg)                  \
    do {                                      \
        if (!(cond))                          \
            return fail(FHE_ERR_ARG, msg);    \
    } while (0)

extern "C" const char* fhe_last_error(void) { return g_lastError.c_str(); }
extern "C" const char* fhe_version(void) {
#ifdef FHE_EMU
    return "fhe_hip 0.1 (TEST lane emulator build — not a product build)";
#else
    return "fhe_hip 0.1 (gfx950)";
#endif
}
extern "C" int fhe_device_count(void) { return rt::device_count(); }

// ------------------------------------------------------------------------------------------------
// host math
// ------------------------------------------------------------------------------------------------
namespace fhe {
namespace host {
bool is_prime(uint64_t n) {
    static const uint64_t w[] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37};
    if (n < 2)
        return false;
    for (uint64_t p : w) {
        if (n == p)
            return true;
        if (n % p == 0)
            return false;
    }
    uint64_t d = n - 1;
    int s      = 0;
    while (!(d & 1)) {
        d >>= 1;
        ++s;
    }
    for (uint64_t a : w) {
        uint64_t x = powmod(a, d, n);
        if (x == 1 || x == n - 1)
            continue;
        bool comp = true;
        for (int r = 1; r < s && comp; ++r) {
            x = mulmod(x, x, n);
            if (x == n - 1)
                comp = false;
        }
        if (comp)
            return false;
    }
    return true;
}
bool is_primitive_root_2n(uint64_t psi, uint64_t twoN, uint64_t q) {
    return psi != 0 && psi < q && powmod(psi, twoN / 2, q) == q - 1;
}
uint64_t first_prime(uint32_t bits, uint64_t m) {  // nbtheory-impl.h:329-347
    uint64_t q = (uint64_t)1 << bits, r = q % m, c = q + 1 - r;
    if (r > 0)
        c += m;
    while (!is_prime(c))
        c += m;
    return c;
}
uint64_t last_prime(uint32_t bits, uint64_t m) {  // nbtheory-impl.h:349-373
    uint64_t q = (uint64_t)1 << bits, r = q % m, c = q + 1 - r;
    if (r < 2)
        c -= m;
    while (!is_prime(c))
        c -= m;
    return c;
}
uint64_t previous_prime(uint64_t q, uint64_t m) {
    uint64_t c = q - m;
    while (!is_prime(c))
        c -= m;
    return c;
}
uint64_t next_prime(uint64_t q, uint64_t m) {
    uint64_t c = q + m;
    while (!is_prime(c))
        c += m;
    return c;
}
uint64_t min_root_of_unity(uint64_t m, uint64_t q) {  // nbtheory-impl.h:183-231
    uint64_t e = (q - 1) / m, root = 0;
    for (uint64_t g = 2; g < q; ++g) {
        uint64_t r = powmod(g, e, q);
        if (powmod(r, m / 2, q) == q - 1) {
            root = r;
            break;
        }
    }
    uint64_t sq = mulmod(root, root, q), x = root, best = root;
    for (uint64_t i = 1; i < m / 2; ++i) {
        x = mulmod(x, sq, q);
        if (x < best)
            best = x;
    }
    return best;
}
uint64_t prod_mod(const std::vector<uint64_t>& mods, int skip, uint64_t mod) {
    uint64_t v = 1 % mod;
    for (int k = 0; k < (int)mods.size(); ++k)
        if (k != skip)
            v = mulmod(v, mods[k] % mod, mod);
    return v;
}
}  // namespace host
}  // namespace fhe

// ------------------------------------------------------------------------------------------------
// host-side parameter helpers
// ------------------------------------------------------------------------------------------------
extern "C" uint64_t fhe_param_first_prime(uint32_t bits, uint64_t m) { return host::first_prime(bits, m); }
extern "C" uint64_t fhe_param_last_prime(uint32_t bits, uint64_t m) { return host::last_prime(bits, m); }
extern "C" uint64_t fhe_param_next_prime(uint64_t q, uint64_t m) { return host::next_prime(q, m); }
extern "C" uint64_t fhe_param_previous_prime(uint64_t q, uint64_t m) { return host::previous_prime(q, m); }
extern "C" uint64_t fhe_param_root_of_unity(uint64_t m, uint64_t q) {
    if (m == 0 || (m & (m - 1)) || (q - 1) % m != 0)
        return 0;
    return host::min_root_of_unity(m, q);
}
extern "C" fhe_status fhe_param_dcrt_chain(uint32_t order, uint32_t nLimbs, uint32_t bits, uint64_t* q, uint64_t* psi) {
    ARG_CHECK(q && psi && nLimbs >= 1, "fhe_param_dcrt_chain: null argument");
    ARG_CHECK(bits >= 4 && bits <= 60, "Invalid bits for ILDCRTParams");  // ildcrtparams.h:103-104 (MAX_MODULUS_SIZE 60)
    ARG_CHECK(order >= 2 && (order & (order - 1)) == 0, "fhe_param_dcrt_chain: order must be a power of two");
    uint64_t cur = host::last_prime(bits, order);
    for (uint32_t i = 0; i < nLimbs; ++i) {
        if (i)
            cur = host::previous_prime(cur, order);
        q[i]   = cur;
        psi[i] = host::min_root_of_unity(order, cur);
    }
    return FHE_OK;
}
extern "C" uint32_t fhe_param_find_automorphism_index_2n_complex(int32_t index, uint32_t m) {
    if (m < 4 || (m & (m - 1)))
        return 0;  // "m should be a power of two."
    if (index == 0)
        return 1;
    if (index == (int32_t)m - 1)
        return (uint32_t)index;
    const uint64_t mask = m - 1;
    uint64_t g0         = 5;
    if (index < 0) {  // 5^-1 mod 2^k by Hensel lifting (every step doubles the number of correct bits)
        uint64_t inv = 1;
        for (int it = 0; it < 6; ++it)
            inv = (inv * (2 - 5 * inv)) & mask;
        g0 = inv;
    }
    uint64_t g = g0;
    for (uint32_t j = 1, n = (uint32_t)(index < 0 ? -(int64_t)index : index); j < n; ++j)
        g = (g * g0) & mask;
    return (uint32_t)g;
}
extern "C" uint32_t fhe_param_select_p(uint32_t logN, uint32_t sizeQ, const uint64_t* q, uint32_t numPartQ,
                                       uint32_t auxBits, uint64_t* p, uint64_t* psiP) {
    if (!q || !p || !psiP || numPartQ == 0 || sizeQ == 0 || auxBits < 4 || auxBits > 60)
        return 0;
    const uint32_t a = (sizeQ + numPartQ - 1) / numPartQ;
    uint32_t maxBits = 0;
    for (uint32_t j = 0; j < numPartQ; ++j) {  // bit length of each composite digit (exact, multi-word product)
        std::vector<uint64_t> big(1, 1);
        for (uint32_t i = a * j; i < (j + 1) * a && i < sizeQ; ++i) {
            uint64_t carry = 0;
            for (auto& w : big) {
                host::u128 t = (host::u128)w * q[i] + carry;
                w            = (uint64_t)t;
                carry        = (uint64_t)(t >> 64);
            }
            if (carry)
                big.push_back(carry);
        }
        maxBits = std::max(maxBits, (uint32_t)(64 * (big.size() - 1) + host::bitlen(big.back())));
    }
    const uint32_t sizeP = (maxBits + auxBits - 1) / auxBits;
    if (sizeP > 64)
        return 0;
    const uint64_t step = 2ull << logN;
    uint64_t prev       = host::first_prime(auxBits, step);
    for (uint32_t i = 0; i < sizeP; ++i) {
        bool inQ;
        do {
            p[i] = host::previous_prime(prev, step);
            inQ  = false;
            for (uint32_t j = 0; j < sizeQ; ++j)
                inQ |= (p[i] == q[j]);
            prev = p[i];
        } while (inQ);
        psiP[i] = host::min_root_of_unity(step, p[i]);
    }
    return sizeP;
}

static uint32_t env_u32(const char* name, uint32_t dflt);

// The device copy of a host table h[0..n): allocated, copied and waited for on the null stream, so that the table is complete before any
// launch that reads it is enqueued, on whatever stream.  owned: the list its owner frees from when it is destroyed (null: the caller keeps
// the pointer, as a cache that frees its own entries does).  Every table of the library is uploaded here; allocations that a call frees
// again before it returns are not tables and do not come here.
template <typename T, typename D>
static fhe_status dev_copy(std::vector<void*>* owned, const T* h, size_t n, D** d) {
    static_assert(std::is_same<T, typename std::remove_const<D>::type>::value, "dev_copy: host and device element types differ");
    void* p = nullptr;
    RT_CHECK(rt::dmalloc(&p, n * sizeof(T)));
    if (owned)
        owned->push_back(p);
    RT_CHECK(rt::h2d(p, h, n * sizeof(T), nullptr));
    RT_CHECK(rt::sync(nullptr));
    *d = (D*)p;
    return FHE_OK;
}

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
struct fhe_ctx {
    uint32_t logN = 0, N = 0, L = 0;
    int device    = 0;
    uint32_t cus  = 0;  // compute units of the device (grid of the persistent row pass, ntt_row8.h)
    std::vector<uint64_t> q, psi;
    // device tables
    TwPair* d_tw      = nullptr;  // [L][N] forward
    TwPair* d_twInv   = nullptr;  // [L][N] inverse
    TwPair* d_fin     = nullptr;  // [L][2] {N^-1, TableInv[1]*N^-1}
    std::vector<TwPair> h_fin;    // host copy (the key-switch plans derive tables with extra per-limb factors from it)
    TwPair* d_twRow   = nullptr;  // [L][N/4096][15][256] lane-major twiddles of the row pass's bit-0 step (N >= 4096), forward
    TwPair* d_twRowInv = nullptr; // ... inverse
    uint64_t* d_q     = nullptr;  // [L]
    LimbConst* d_lc   = nullptr;  // [L]
    uint64_t* d_red   = nullptr;  // [L] redM | redR << 32: quotient estimate of the static NTT kernels (ntt_static.h)
    uint64_t* d_mu128 = nullptr;  // [L][2]
    std::vector<void*> owned;     // every device allocation made for tables (freed in destroy)
    // discrete-Gaussian inversion tables by standard deviation (fhe_sample_gaussian): {device table, length, a}
    std::map<double, std::tuple<const double*, uint32_t, double>> dggTabs;
    // cached per-level rescale tables (ckksrns-cryptoparameters.cpp:60-81): sizeQl -> {A, B} device arrays
    std::map<uint32_t, std::pair<TwPair*, TwPair*>> rescaleTabs;
    std::map<std::vector<uint64_t>, TwPair*> constTabs;  // per-limb constants of callers' tables, by content (const_table); the map owns
                                                         // them and is emptied when it passes kMaxConstTabs entries (const_tables_trim)
    std::shared_mutex constTabsGate;  // shared: an entry point between asking for its tables and enqueuing the launches that read them
    // cached ModReduce tables per (sizeQl, t): [0..l) = A_i, [l..2l) = B_i, [2l] = negtInvModq, [2l+1] = t^-1 mod q_l, [2l+2..3l+2) = t mod q_i   (fhe_mod_reduce)
    std::map<std::pair<uint32_t, uint64_t>, TwPair*> modReduceTabs;
    // cached tables of mod_reduce_chain_kernel by {t, limbs dropped, with the residue modulo t, the tower's context limbs...}
    std::map<std::vector<uint64_t>, const uint64_t*> chainTabs;
    std::mutex cacheMutex;        // guards the lazily filled caches above (callers may be OpenMP threads)
};


extern "C" fhe_status fhe_ctx_create(uint32_t logN, uint32_t nLimbs, const uint64_t* q, const uint64_t* psi,
                                     int device, fhe_ctx** out) {
    ARG_CHECK(out != nullptr, "fhe_ctx_create: out is null");
    ARG_CHECK(logN >= 4 && logN <= 17, "fhe_ctx_create: logN must be in [4,17]");
    ARG_CHECK(nLimbs >= 1 && nLimbs <= (uint32_t)kMaxLimbs, "fhe_ctx_create: nLimbs must be in [1,256]");
    ARG_CHECK(q && psi, "fhe_ctx_create: null modulus/root array");
    if (rt::device_count() <= 0)
        return fail(FHE_ERR_DEVICE, "fhe_ctx_create: no HIP device available (there is no CPU fallback)");
    ARG_CHECK(device >= 0 && device < rt::device_count(), "fhe_ctx_create: bad device ordinal");
    const uint32_t N = 1u << logN;
    for (uint32_t i = 0; i < nLimbs; ++i) {
        ARG_CHECK(q[i] > 2 && q[i] < ((uint64_t)1 << 60), "fhe_ctx_create: modulus must be < 2^60");
        ARG_CHECK((q[i] - 1) % (2ull * N) == 0, "fhe_ctx_create: modulus must be 1 mod 2N");
        ARG_CHECK(host::is_primitive_root_2n(psi[i], 2ull * N, q[i]),
                  "fhe_ctx_create: psi is not a primitive 2N-th root of unity");
    }
    RT_CHECK(rt::set_device(device));
    fhe_ctx* c = new fhe_ctx;
    c->logN    = logN;
    c->N       = N;
    c->L       = nLimbs;
    c->device  = device;
    c->cus     = rt::cu_count(device);
    c->q.assign(q, q + nLimbs);
    c->psi.assign(psi, psi + nLimbs);

    // twiddle tables: Table[bitrev(i)] = psi^i, TableI[bitrev(i)] = psi^-i  (transformnat-impl.h:725-737)
    std::vector<TwPair> tw((size_t)nLimbs * N), twInv((size_t)nLimbs * N), fin((size_t)nLimbs * 2);
    const bool rowTables   = logN >= (uint32_t)kTileLog;
    const size_t rowPerLimb = rowTables ? (size_t)(N >> kTileLog) * kRowTwSlots * kThreads : 0;
    std::vector<TwPair> twRow(rowPerLimb * nLimbs), twRowInv(rowPerLimb * nLimbs);
    std::vector<LimbConst> lc(nLimbs);
    std::vector<uint64_t> mu(2 * (size_t)nLimbs), red(nLimbs);
    // one thread per limb at most: a team of every host core would keep spinning after the region (libgomp's default
    // wait policy) and slow down the caller's kernel launches for a while
#pragma omp parallel for schedule(dynamic) num_threads(std::max(1, std::min<int>((int)nLimbs, 32)))
    for (uint32_t l = 0; l < nLimbs; ++l) {
        const uint64_t ql = q[l], ps = psi[l], psInv = host::invmod(ps, ql);
        uint64_t x = 1, xi = 1;
        TwPair* t  = tw.data() + (size_t)l * N;
        TwPair* ti = twInv.data() + (size_t)l * N;
        for (uint32_t i = 0; i < N; ++i) {
            const uint32_t r = host::bitrev(i, logN);
            t[r]             = TwPair{x, host::shoup(x, ql)};
            ti[r]            = TwPair{xi, host::shoup(xi, ql)};
            x                = host::mulmod(x, ps, ql);
            xi               = host::mulmod(xi, psInv, ql);
        }
        // lane-major copy for the step whose register field is tile bit 0 (ntt_static.h, TwSrc): lane t of tile tr holds
        // coefficients j0 = tr*4096 + 16t .. +15; stage b, twiddle g: index 2^(logN-1-b) + ((j0 >> 4) << (3-b)) + g
        for (size_t tr = 0; rowTables && tr < (N >> kTileLog); ++tr)
            for (uint32_t b = 0; b < 4; ++b)
                for (uint32_t g = 0; g < (8u >> b); ++g) {
                    const size_t slot = (size_t)(1u << (3 - b)) - 1 + g;
                    TwPair* d  = twRow.data() + (size_t)l * rowPerLimb + (tr * kRowTwSlots + slot) * kThreads;
                    TwPair* di = twRowInv.data() + (size_t)l * rowPerLimb + (tr * kRowTwSlots + slot) * kThreads;
                    for (uint32_t lane = 0; lane < (uint32_t)kThreads; ++lane) {
                        const size_t idx = ((size_t)1 << (logN - 1 - b)) + (((tr << 8) + lane) << (3 - b)) + g;
                        d[lane]  = t[idx];
                        di[lane] = ti[idx];
                    }
                }
        const uint64_t nInv = host::invmod((uint64_t)N % ql, ql);
        const uint64_t w1n  = host::mulmod(ti[1].w, nInv, ql);  // transformnat-impl.h:533-534
        fin[2 * l]          = TwPair{nInv, host::shoup(nInv, ql)};
        fin[2 * l + 1]      = TwPair{w1n, host::shoup(w1n, ql)};
        lc[l]               = LimbConst{ql, host::barrett_mu(ql), host::bitlen(ql), 0};
        host::mu128(ql, &mu[2 * l]);
        // k = (x.hi * redM) >> (32 + redR) is floor(x / q) or one less for every 64-bit x once bitlen(q) >= 36:
        // redR = bitlen(q) - 33, redM = floor(2^(64 + redR) / q) < 2^32; smaller moduli take the ladder (redR = 255)
        const uint32_t bl = host::bitlen(ql);
        if (bl >= 36) {
            const uint32_t rr = bl - 33;
            red[l] = (uint64_t)((((unsigned __int128)1) << (64 + rr)) / ql) | ((uint64_t)rr << 32);
        }
        else
            red[l] = (uint64_t)255 << 32;
    }
    c->h_fin = fin;
    fhe_status s;
    if ((s = dev_copy(&c->owned, tw.data(), tw.size(), &c->d_tw)) || (s = dev_copy(&c->owned, twInv.data(), twInv.size(), &c->d_twInv)) ||
        (s = dev_copy(&c->owned, fin.data(), fin.size(), &c->d_fin)) ||
        (rowTables && (s = dev_copy(&c->owned, twRow.data(), twRow.size(), &c->d_twRow))) ||
        (rowTables && (s = dev_copy(&c->owned, twRowInv.data(), twRowInv.size(), &c->d_twRowInv))) ||
        (s = dev_copy(&c->owned, c->q.data(), nLimbs, &c->d_q)) || (s = dev_copy(&c->owned, lc.data(), nLimbs, &c->d_lc)) ||
        (s = dev_copy(&c->owned, red.data(), nLimbs, &c->d_red)) || (s = dev_copy(&c->owned, mu.data(), mu.size(), &c->d_mu128))) {
        fhe_ctx_destroy(c);
        return s;
    }
    *out = c;
    return FHE_OK;
}

extern "C" void fhe_ctx_destroy(fhe_ctx* c) {
    if (!c)
        return;
    rt::set_device(c->device);
    for (void* p : c->owned)
        rt::dfree(p);
    for (auto& kv : c->constTabs)
        rt::dfree(kv.second);
    delete c;
}
extern "C" uint32_t fhe_ctx_logn(const fhe_ctx* c) { return c ? c->logN : 0; }
extern "C" uint32_t fhe_ctx_limbs(const fhe_ctx* c) { return c ? c->L : 0; }
extern "C" int fhe_ctx_device(const fhe_ctx* c) { return c ? c->device : -1; }

// ------------------------------------------------------------------------------------------------
// memory / streams
// ------------------------------------------------------------------------------------------------
extern "C" fhe_status fhe_malloc(fhe_ctx* c, size_t bytes, void** p) {
    ARG_CHECK(c && p, "fhe_malloc: null argument");
    RT_CHECK(rt::set_device(c->device));
    if (const char* e = rt::dmalloc(p, bytes))
        return fail(FHE_ERR_ALLOC, std::string("fhe_malloc: ") + e);
    return FHE_OK;
}
extern "C" fhe_status fhe_mem_info(fhe_ctx* c, size_t* freeBytes, size_t* totalBytes) {
    ARG_CHECK(c && freeBytes && totalBytes, "fhe_mem_info: null argument");
    RT_CHECK(rt::set_device(c->device));
    RT_CHECK(rt::mem_info(freeBytes, totalBytes));
    return FHE_OK;
}
extern "C" fhe_status fhe_free(fhe_ctx* c, void* p) {
    ARG_CHECK(c, "fhe_free: null context");
    RT_CHECK(rt::dfree(p));
    return FHE_OK;
}
extern "C" fhe_status fhe_memcpy_h2d(fhe_ctx* c, void* d, const void* s, size_t n, void* st) {
    ARG_CHECK(c && d && s, "fhe_memcpy_h2d: null argument");
    RT_CHECK(rt::h2d(d, s, n, (rt::stream_t)st));
    return FHE_OK;
}
extern "C" fhe_status fhe_memcpy_d2h(fhe_ctx* c, void* d, const void* s, size_t n, void* st) {
    ARG_CHECK(c && d && s, "fhe_memcpy_d2h: null argument");
    RT_CHECK(rt::d2h(d, s, n, (rt::stream_t)st));
    return FHE_OK;
}
extern "C" fhe_status fhe_memcpy_d2d(fhe_ctx* c, void* d, const void* s, size_t n, void* st) {
    ARG_CHECK(c && d && s, "fhe_memcpy_d2d: null argument");
    RT_CHECK(rt::d2d(d, s, n, (rt::stream_t)st));
    return FHE_OK;
}
extern "C" fhe_status fhe_stream_sync(fhe_ctx* c, void* st) {
    ARG_CHECK(c, "fhe_stream_sync: null context");
    RT_CHECK(rt::sync((rt::stream_t)st));
    return FHE_OK;
}

// Streams and graphs.  Composite calls (EvalMult, key switch, BFV EvalMult ...) are sequences of 20-60 kernel launches of
// 50-1000 us each; on a busy host the launch path, not the GPU, sets their pace.  Every entry point only enqueues work on
// the caller's stream (tables are built on first use, so run the sequence once before capturing), hence a caller can
// record a sequence into a HIP graph once and replay it with a single launch.
extern "C" fhe_status fhe_stream_create(fhe_ctx* c, void** stream) {
    ARG_CHECK(c && stream, "fhe_stream_create: null argument");
    RT_CHECK(rt::set_device(c->device));
    rt::stream_t s;
    RT_CHECK(rt::stream_create(&s));
    *stream = (void*)s;
    return FHE_OK;
}
extern "C" fhe_status fhe_stream_destroy(fhe_ctx* c, void* stream) {
    ARG_CHECK(c, "fhe_stream_destroy: null context");
    RT_CHECK(rt::stream_destroy((rt::stream_t)stream));
    return FHE_OK;
}
// `stream` waits on the device (the host is not blocked) for everything enqueued so far on `other`: the one cross-stream
// primitive a multi-threaded host needs (one stream per host thread, hand-over of a tower between threads)
extern "C" fhe_status fhe_stream_wait(fhe_ctx* c, void* stream, void* other) {
    ARG_CHECK(c, "fhe_stream_wait: null context");
    if (stream == other)
        return FHE_OK;
    RT_CHECK(rt::set_device(c->device));
    RT_CHECK(rt::stream_wait((rt::stream_t)stream, (rt::stream_t)other));
    return FHE_OK;
}
extern "C" fhe_status fhe_event_create(fhe_ctx* c, void** event) {
    ARG_CHECK(c && event, "fhe_event_create: null argument");
    RT_CHECK(rt::set_device(c->device));
    rt::event_t e;
    RT_CHECK(rt::event_create(&e));
    *event = (void*)e;
    return FHE_OK;
}
extern "C" fhe_status fhe_event_record(fhe_ctx* c, void* event, void* stream) {
    ARG_CHECK(c && event, "fhe_event_record: null argument");
    RT_CHECK(rt::set_device(c->device));
    RT_CHECK(rt::event_record((rt::event_t)event, (rt::stream_t)stream));
    return FHE_OK;
}
extern "C" fhe_status fhe_stream_wait_event(fhe_ctx* c, void* stream, void* event) {
    ARG_CHECK(c && event, "fhe_stream_wait_event: null argument");
    RT_CHECK(rt::set_device(c->device));
    RT_CHECK(rt::stream_wait_event((rt::stream_t)stream, (rt::event_t)event));
    return FHE_OK;
}
extern "C" fhe_status fhe_event_destroy(fhe_ctx* c, void* event) {
    ARG_CHECK(c, "fhe_event_destroy: null context");
    if (event)
        RT_CHECK(rt::event_destroy((rt::event_t)event));
    return FHE_OK;
}
extern "C" fhe_status fhe_memset_zero(fhe_ctx* c, void* dst, size_t bytes, void* stream) {
    ARG_CHECK(c && dst, "fhe_memset_zero: null argument");
    RT_CHECK(rt::set_device(c->device));
    RT_CHECK(rt::dzero(dst, bytes, (rt::stream_t)stream));
    return FHE_OK;
}
extern "C" fhe_status fhe_graph_begin(fhe_ctx* c, void* stream) {
    ARG_CHECK(c && stream, "fhe_graph_begin: capture needs a stream created with fhe_stream_create");
    RT_CHECK(rt::set_device(c->device));
    RT_CHECK(rt::capture_begin((rt::stream_t)stream));
    return FHE_OK;
}
extern "C" fhe_status fhe_graph_end(fhe_ctx* c, void* stream, void** graph) {
    ARG_CHECK(c && stream && graph, "fhe_graph_end: null argument");
    rt::graph_t g;
    RT_CHECK(rt::capture_end((rt::stream_t)stream, &g));
    *graph = (void*)g;
    return FHE_OK;
}
extern "C" fhe_status fhe_graph_launch(fhe_ctx* c, void* graph, void* stream) {
    ARG_CHECK(c && graph, "fhe_graph_launch: null argument");
    RT_CHECK(rt::graph_launch((rt::graph_t)graph, (rt::stream_t)stream));
    return FHE_OK;
}
extern "C" void fhe_graph_destroy(void* graph) {
    if (graph)
        rt::graph_destroy((rt::graph_t)graph);
}

// ------------------------------------------------------------------------------------------------
// helpers
// ------------------------------------------------------------------------------------------------
static fhe_status make_sel(const fhe_ctx* c, const uint32_t* limbIdx, uint32_t nLimbs, LimbSel* sel, const char* who) {
    if (nLimbs < 1 || nLimbs > (uint32_t)kMaxLimbs)
        return fail(FHE_ERR_ARG, std::string(who) + ": nLimbs out of range");
    for (uint32_t i = 0; i < nLimbs; ++i) {
        uint32_t l = limbIdx ? limbIdx[i] : i;
        if (l >= c->L)
            return fail(FHE_ERR_ARG, std::string(who) + ": limb index exceeds context size");
        sel->idx[i] = (uint8_t)l;
    }
    for (uint32_t i = nLimbs; i < (uint32_t)kMaxLimbs; ++i)
        sel->idx[i] = 0;
    return FHE_OK;
}
static inline uint32_t tiles_for(const fhe_ctx* c, uint64_t rows) {
    const uint64_t words = rows << c->logN;
    return (uint32_t)((words + kTile - 1) >> kTileLog);
}
#define LAUNCH_CHECK() RT_CHECK(rt::last_launch_error())

// ------------------------------------------------------------------------------------------------
// NTT: passes, kernel instances, launches
// ------------------------------------------------------------------------------------------------
static uint32_t env_u32(const char* name, uint32_t dflt) {
    const char* v = std::getenv(name);
    return v ? (uint32_t)std::strtoul(v, nullptr, 10) : dflt;
}
// The measurement switches of the NTT host path, read once per process (measurements, tests).
//   FHE_NTT_ROW8 = 0 / 1        forces the 16- / the 8-residues-per-lane row kernel for every stage count (default: row8_for)
//   FHE_NTT_ROW8_BATCH = 1/2/4  forces the polynomials per workgroup of the 12-stage row pass (default: row8_batch_for)
//   FHE_NTT_ROW8_X1 = 0 / 1     forces the exchange between the waves of the batched kernel: 0 one set of LDS regions and a barrier
//                               between the polynomials, 1 a set per polynomial (default: row8_x1_regions)
//   FHE_NTT_HANDOVER = 0 / 1    forces the hand-over between the passes of an inverse transform off / on; any other value is
//                               reported and means off
//   FHE_NTT_T1 = 4 / 5          another split of a two-pass ring (ntt_t1)
//   FHE_NTT_SPLIT6 = 0 / 1 / fwd / inv   the 6 + 10 split of N = 2^16 (ntt_run) off / on / forward transforms only / inverse only.  Only the
//                               forward direction has the pair (profiles/ntt_split6.md), so 1 and fwd are the default and inv is 0; any
//                               other value is reported and means off
constexpr bool kHandoverDefault = true;
constexpr bool kSplit6Default = true;
struct NttSwitches {
    int row8 = -1, row8X1 = -1;  // -1: not forced
    uint32_t row8Batch = 0, t1 = 0;  // 0: not forced
    bool handover = kHandoverDefault;
    bool split6 = kSplit6Default;
};
static const NttSwitches& ntt_switches() {
    static const NttSwitches sw = [] {
        NttSwitches s;
        auto flag = [](const char* name) {
            const char* v = std::getenv(name);
            return v && (v[0] == '0' || v[0] == '1') ? v[0] - '0' : -1;
        };
        s.row8   = flag("FHE_NTT_ROW8");
        s.row8X1 = flag("FHE_NTT_ROW8_X1");
        if (const char* v = std::getenv("FHE_NTT_ROW8_BATCH"))
            s.row8Batch = (v[0] == '1' || v[0] == '2' || v[0] == '4') && !v[1] ? (uint32_t)(v[0] - '0') : 0u;
        if (const char* v = std::getenv("FHE_NTT_HANDOVER")) {
            s.handover = v[0] == '1' && !v[1];
            if (!s.handover && !(v[0] == '0' && !v[1]))
                fprintf(stderr, "fhe_hip: FHE_NTT_HANDOVER=%s is neither 0 nor 1: hand-over is off\n", v);
        }
        s.t1 = env_u32("FHE_NTT_T1", 0);
        if (const char* v = std::getenv("FHE_NTT_SPLIT6")) {
            const std::string w = v;
            s.split6 = w == "1" || w == "fwd";
            if (!s.split6 && w != "0" && w != "inv")
                fprintf(stderr, "fhe_hip: FHE_NTT_SPLIT6=%s is none of 0, 1, fwd, inv: the 6 + 10 split is off\n", v);
        }
        return s;
    }();
    return sw;
}
// Which row pass runs (both are bit-exact; profiles/r06_sweeps.md section 4): ntt_row8.h for 9..11 stages (rings 2^13..2^15: 2-10 % faster),
// ntt_static.h's 16-residues-per-lane kernel for 12 stages (1-3 % faster there) -- for what row8_batch_for leaves of a 12-stage batch: its
// P-aligned part runs ntt_row8.h's batched kernel.
static bool row8_for(uint32_t T) { return ntt_switches().row8 >= 0 ? ntt_switches().row8 == 1 : T <= 11u; }
// Polynomials per workgroup of the 12-stage row pass (ntt_row8.h, the batched kernel: one twiddle fetch serves P polynomials): the
// measured winner per stage count (profiles/r09_sweeps.md: P = 2 with one set of X1 regions, 27.33 against 27.92 ms per headline step;
// P = 4 27.37, a set of regions per polynomial 28.4 / 32.7); 1 = the kernel row8_for names
constexpr uint32_t kRow8BatchDefault = 2;
constexpr bool kRow8X1RegionsP2 = false, kRow8X1RegionsP4 = false;
static uint32_t row8_batch_for(uint32_t T) {
    if (T != 12u)
        return 1u;
    // (a forced unbatched kernel, FHE_NTT_ROW8, takes the whole batch unless P is forced as well)
    return ntt_switches().row8Batch ? ntt_switches().row8Batch : ntt_switches().row8 >= 0 ? 1u : kRow8BatchDefault;
}
static bool row8_x1_regions(uint32_t P) {
    return ntt_switches().row8X1 >= 0 ? ntt_switches().row8X1 == 1 : (P == 2 ? kRow8X1RegionsP2 : kRow8X1RegionsP4);
}
// stages of the strided column pass of a two-pass ring: as few as possible (>= 4), so that the column pass reads rows of
// 2^(12-T1) consecutive words and, at T1 = 4, is a pure register radix-16 step; the other splits were measured slower
// (profiles/r01_sweeps.md) and their kernel instances are gone.  FHE_NTT_T1 names another split where both passes have kernel
// instances (column 4..5, row 9..12)
static uint32_t ntt_t1(uint32_t logN) {
    const uint32_t forced = ntt_switches().t1;
    if (forced >= 4 && forced <= 5 && logN > (uint32_t)kTileLog && logN - forced >= 9 && logN - forced <= 12)
        return forced;
    return std::max(4u, logN - (uint32_t)kTileLog);
}

// One pass of a transform, as far as the choice of its kernel goes.  The single pass of a ring of at most one tile; of a larger ring the
// strided column pass of T1 stages (the coefficient index's top bits) and the contiguous row pass of the other T2 = logN - T1.
struct NttPass {
    enum Kind { Single, Column, Row };
    bool inverse = false;
    Kind kind    = Single;
    uint32_t T   = 0;  // stages
    // MODE of the static kernels (ntt_static.h).  Forward: the bound class of the pass's input, 1 = canonical, 9 = at most 9q: what a
    // row pass sees, since a column pass leaves its residues below 2q.  Inverse: 1 = the pass ends the transform, 0 = it does not.
    int mode = 1;
    NttPass() = default;
    NttPass(bool inv, Kind k, uint32_t stages) : inverse(inv), kind(k), T(stages), mode(k == Row ? (inv ? 0 : 9) : 1) {}
    bool layoutA() const { return kind == Column; }
};
// the passes of a transform of this context, in the order they run: forward column then row, inverse row then column
struct NttPasses {
    uint32_t n;
    NttPass p[2];
};
static NttPasses ntt_passes(const fhe_ctx* c, bool inverse) {
    if (c->logN <= (uint32_t)kTileLog)
        return {1, {NttPass(inverse, NttPass::Single, c->logN), NttPass()}};
    const uint32_t T1 = ntt_t1(c->logN);
    const NttPass col(inverse, NttPass::Column, T1), row(inverse, NttPass::Row, c->logN - T1);
    return inverse ? NttPasses{2, {row, col}} : NttPasses{2, {col, row}};
}

// fused epilogue of a forward transform's last pass (NttPassArgs::epi*)
struct NttEpilogue {
    uint32_t mode = 0, split = 0, aStride = 0, aFirst = 0;
    int64_t aDelta = 0;  // != 0: towers of A are this many words apart (NttPassArgs::epiADelta)
    const uint64_t* A = nullptr;
    const TwPair* C   = nullptr;
    uint64_t *out0 = nullptr, *out1 = nullptr;
};
// What a transform (ntt_run) or a pass (launch_pass) does besides the plain dense, canonical one.
struct NttView {
    uint32_t stride = 0;  // 0: dense [batch][nLimbs][N]; else a [batch][stride][N] view ...
    uint32_t first  = 0;  // ... whose rows first.. of every tower are the transform's
};
struct NttOpts {
    NttView src, dst;
    int64_t srcDelta = 0;            // != 0: towers of the source are this many words apart (allocated on their own); overrides src.stride
    const NttEpilogue* epi = nullptr;
    bool canonOut = true;            // false: the output may stay lazy (forward: below the bound of the last step)
    const uint32_t* proSrcLimb = nullptr;  // forward: every limb is loaded from row src.first, a limb modulo q[*proSrcLimb] (NttPassArgs::proMode)
    const TwPair* proC = nullptr;          // with proSrcLimb: ... and multiplied by proC[row of the tower] (proMode 2)
    uint32_t proRows = 0;                  // != 0 (proMode 3): every limb is the sum of rows 0..proRows-1 of the source tower, row k modulo
                                           // q[proSrcLimb[k]] and weighted by proC[k * nLimbs + row of the tower]
};

// ---- the small-ring kernel (N < 4096): ntt_pass_kernel reads its plan from the arguments (steps, nSteps, canonLevels, canonStep) ----
// stages of one pass act on the T bits of the in-tile point index p (bit T-1 first for the forward
// transform, bit 0 first for the inverse); they are grouped into register-resident steps of <= 4 stages.
static void plan_pass(bool inverse, bool layoutA, NttPassArgs& a) {
    const uint32_t logN = a.logN, T = a.T;
    const int logC  = kTileLog - (int)T;
    const int jsh   = layoutA ? (int)(logN - T) : 0;  // p bit b  <->  j bit b + jsh
    const int ish   = layoutA ? logC : 0;             // p bit b  <->  tile-index bit b + ish
    const int nst   = (int)(T + 3) / 4;
    int sizes[4];
    for (int i = 0; i < nst; ++i)
        sizes[i] = (int)T / nst + (i < (int)T % nst ? 1 : 0);
    NttStep real[4] = {};
    if (!inverse) {
        int top = (int)T - 1;
        for (int i = 0; i < nst; ++i) {
            const int r = sizes[i], fp = std::max(top - 3, 0);
            real[i] = NttStep{(int8_t)(fp + ish), (int8_t)(fp + jsh), (int8_t)(top - fp), (int8_t)(top - fp - r + 1), 0, 0, 0, 0};
            top -= r;
        }
    }
    else {
        int bot = 0;
        for (int i = 0; i < nst; ++i) {
            const int r = sizes[i], fp = std::min(bot, (int)T - 4);
            real[i] = NttStep{(int8_t)(fp + ish), (int8_t)(fp + jsh), (int8_t)(bot - fp + r - 1), (int8_t)(bot - fp), 0, 0, 0, 0};
            bot += r;
        }
    }
    // staging steps: a first/last step whose register field sits below tile-index bit 4 would touch HBM in
    // < 128-byte pieces; route it through LDS with the fully coalesced mapping (field at bits 8..11) instead
    uint32_t n = 0;
    const NttStep stage{8, 0, -1, 0, 0, 0, 0, 0};
    if (!layoutA && real[0].fI < 4)
        a.steps[n++] = stage;
    for (int i = 0; i < nst; ++i)
        a.steps[n++] = real[i];
    if (!layoutA && real[nst - 1].fI < 4)
        a.steps[n++] = stage;
    a.nSteps = n;
}
// lazy-reduction schedule of a forward pass (the static kernels derive the same at compile time, ntt_static.h SPlan): a
// butterfly with the truncated quotient adds at most 3q to the bound of its operands and 16q < 2^64, so a step of r
// stages needs a correction (the `a` inputs of its first stage below 2q) only when bound + 3r would exceed 16.
// `bound` (in units of q) is the bound of the pass input; returns that of its output.
static uint32_t schedule_fwd(NttPassArgs& a, uint32_t bound) {
    for (uint32_t i = 0; i < a.nSteps; ++i) {
        NttStep& st = a.steps[i];
        if (st.bHi < st.bLo)
            continue;
        const uint32_t r = (uint32_t)(st.bHi - st.bLo + 1);
        st.mode          = bound + 3 * r <= 16 ? 0 : 1;
        bound            = (st.mode ? 2 : bound) + 3 * r;
    }
    return bound;
}
// twiddle index = 2^s + (j >> (Fj+4))...: lane-independent iff no lane-dependent bit of j lies above the field
static void mark_uniform(NttPassArgs& a, bool layoutA) {
    for (uint32_t i = 0; i < a.nSteps; ++i) {
        NttStep& st = a.steps[i];
        if (st.bHi >= st.bLo)
            st.uniformTw = layoutA ? ((uint32_t)st.Fj + 4 == a.logN) : ((uint32_t)st.Fj + 4 >= (uint32_t)kTileLog);
    }
}
static uint32_t pass_tiles(const NttPassArgs& a) { return (uint32_t)((((uint64_t)a.rows << a.logN) + kTile - 1) >> kTileLog); }
// plans the pass into the arguments and launches it: several limbs per workgroup.  (Every pass of a ring this small is a single one; the
// column instances of the kernel stay named here.)
static void launch_small(const NttPass& p, bool canonOut, NttPassArgs a, void* stream) {
    plan_pass(p.inverse, p.layoutA(), a);
    mark_uniform(a, p.layoutA());
    const uint32_t outBound = p.inverse ? 16u : schedule_fwd(a, 1);  // (bound of the pass output under the lazy schedule, units of q)
    // canonicalise right after the last step that has butterfly stages (a trailing staging step only moves data)
    a.canonStep   = 0xffffffffu;
    a.canonLevels = 1;
    while ((1u << a.canonLevels) < outBound)
        ++a.canonLevels;
    for (uint32_t i = 0; canonOut && i < a.nSteps; ++i)
        if (a.steps[i].bHi >= a.steps[i].bLo)
            a.canonStep = i;
    if (p.layoutA()) {
        if (p.inverse)
            FHE_LAUNCH_BARRIER((ntt_pass_kernel<true, true>), pass_tiles(a), stream, a);
        else
            FHE_LAUNCH_BARRIER((ntt_pass_kernel<true, false>), pass_tiles(a), stream, a);
    }
    else {
        if (p.inverse)
            FHE_LAUNCH_BARRIER((ntt_pass_kernel<false, true>), pass_tiles(a), stream, a);
        else
            FHE_LAUNCH_BARRIER((ntt_pass_kernel<false, false>), pass_tiles(a), stream, a);
    }
}

// ---- kernel instances (N >= 4096): one function per family, THE list of its instances.  Each answers whether the family has an
// instance for the pass and, given arguments (a != nullptr), launches it on the rows of *a.  Whatever the host wants to know about the
// kernel a pass can land on -- the *_supported questions, the hand-over decision, the "no kernel" failures -- it asks here.
#define FHE_PASS_IS(LA, INV, TT, MODE) (p.layoutA() == LA && p.inverse == INV && p.T == TT && p.mode == MODE)
#define FHE_INSTANCE(COND, LAUNCH) \
    if (COND) {                    \
        if (a) {                   \
            LAUNCH;                \
        }                          \
        return true;               \
    }
// ntt_static.h, 16 residues per lane: column passes of logN = 13..16 (T1 = 4) and 17 (T1 = 5); row passes T2 = logN - T1; the single
// pass of logN = 12
static bool static_instance(const NttPass& p, const NttPassArgs* a, void* stream) {
#define FHE_CASE(LA, INV, TT, MODE) \
    FHE_INSTANCE(FHE_PASS_IS(LA, INV, TT, MODE), FHE_LAUNCH_BARRIER((ntt_static_kernel<LA, INV, TT, MODE>), pass_tiles(*a), stream, *a))
    FHE_CASE(true, false, 4, 1) FHE_CASE(true, true, 4, 1) FHE_CASE(true, false, 5, 1) FHE_CASE(true, true, 5, 1)
    FHE_CASE(false, false, 12, 9) FHE_CASE(false, true, 12, 0) FHE_CASE(false, false, 11, 9) FHE_CASE(false, true, 11, 0)
    FHE_CASE(false, false, 10, 9) FHE_CASE(false, true, 10, 0) FHE_CASE(false, false, 9, 9) FHE_CASE(false, true, 9, 0)
    FHE_CASE(false, false, 12, 1) FHE_CASE(false, true, 12, 1)
#undef FHE_CASE
    return false;
}
// ... with the fused epilogue (NttPassArgs::epi*): the forward row passes and the single pass
static bool static_epilogue_instance(const NttPass& p, const NttPassArgs* a, void* stream) {
#define FHE_CASE(TT, MODE) \
    FHE_INSTANCE(FHE_PASS_IS(false, false, TT, MODE),                                                                                \
                 FHE_LAUNCH_AS("EPI", (ntt_static_kernel<false, false, TT, MODE, true>), pass_tiles(*a), kThreads, true, stream, *a))
    FHE_CASE(12, 9) FHE_CASE(11, 9) FHE_CASE(10, 9) FHE_CASE(9, 9) FHE_CASE(12, 1)
#undef FHE_CASE
    return false;
}
// ... with the load prologue (NttPassArgs::proMode): the forward column passes.  The prologue modes have the same pass shapes, so the
// question "is there an instance" (a == nullptr) has one answer for all; a launch takes the instance of a->proMode.
static bool static_prologue_instance(const NttPass& p, const NttPassArgs* a, void* stream) {
#define FHE_CASE(TT)                                                                                                                  \
    FHE_INSTANCE(FHE_PASS_IS(true, false, TT, 1) && !(a && a->proMode >= 2u),                                                         \
                 FHE_LAUNCH_AS("PRO", (ntt_static_kernel<true, false, TT, 1, false, 1>), pass_tiles(*a), kThreads, true, stream, *a))  \
    FHE_INSTANCE(FHE_PASS_IS(true, false, TT, 1) && a && a->proMode == 2u,                                                            \
                 FHE_LAUNCH_AS("PRO2", (ntt_static_kernel<true, false, TT, 1, false, 2>), pass_tiles(*a), kThreads, true, stream, *a)) \
    FHE_INSTANCE(FHE_PASS_IS(true, false, TT, 1) && a && a->proMode == 3u,                                                            \
                 FHE_LAUNCH_AS("PRO3", (ntt_static_kernel<true, false, TT, 1, false, 3>), pass_tiles(*a), kThreads, true, stream, *a))
    FHE_CASE(4) FHE_CASE(5)
#undef FHE_CASE
    return false;
}
// ... the inverse 4-stage column pass that takes the hand-over (below)
static bool static_handover_instance(const NttPass& p, const NttPassArgs* a, void* stream) {
    FHE_INSTANCE(FHE_PASS_IS(true, true, 4, 1), FHE_LAUNCH_AS("HAND", (ntt_static_kernel<true, true, 4, 1, false, false, true>), pass_tiles(*a),
                                                              kThreads, true, stream, *a))
    return false;
}
// ... the forward 4-stage column pass of the 6 + 10 split (ntt_run): six stages for the towers below a->split6Batch, four for the rest
static bool static_split6_instance(const NttPass& p, const NttPassArgs* a, void* stream) {
    FHE_INSTANCE(FHE_PASS_IS(true, false, 4, 1), FHE_LAUNCH_AS("SPLIT6", (ntt_static_kernel<true, false, 4, 1, false, 0, false, true>),
                                                               pass_tiles(*a), kThreads, true, stream, *a))
    return false;
}
// ntt_row8.h: tiles of 2^T words on 2^(T-9) waves, groups of P polynomials.  Its instances take the arguments in this form: rows and XCD order
// for that tile size
static NttPassArgs row8_args(const NttPassArgs& a, uint32_t P) {
    NttPassArgs r = a;
    r.batch       = a.batch / P;  // groups of P polynomials: the batch-fastest XCD order, in units of P
    r.rows        = r.batch * a.nLimbs;
    r.xcdSwizzle  = ((a.nLimbs << (a.logN - a.T)) % 8u == 0) ? 1u : 0u;
    return r;
}
// row passes of two-pass rings at 8 residues per lane (8 waves per SIMD, one barrier per tile)
static bool row8_instance(const NttPass& p, const NttPassArgs* a, void* stream) {
#define FHE_CASE(INV, TT, MODE)                                                                                                       \
    FHE_INSTANCE(FHE_PASS_IS(false, INV, TT, MODE), FHE_LAUNCH_BARRIER_N((r8::ntt_row8_kernel<INV, TT - 9, MODE>), a->rows << (a->logN - TT), \
                                                                         64u << (TT - 9), stream, *a))
    FHE_CASE(false, 12, 9) FHE_CASE(true, 12, 0) FHE_CASE(false, 11, 9) FHE_CASE(true, 11, 0)
    FHE_CASE(false, 10, 9) FHE_CASE(true, 10, 0) FHE_CASE(false, 9, 9) FHE_CASE(true, 9, 0)
#undef FHE_CASE
    return false;
}
// 12-stage row passes, P polynomials per workgroup; hand: the inverse instances that hand the last stage's twiddle products over; split6: the
// forward instance behind the six-stage column pass (ten stages in the 12-stage tile)
static bool row8_batched_instance(const NttPass& p, uint32_t P, bool hand, bool split6, const NttPassArgs* a, void* stream) {
    const bool x1p = row8_x1_regions(P);
    if (split6) {
        FHE_INSTANCE(FHE_PASS_IS(false, false, 12, 9) && P == 2 && !x1p && !hand,
                     FHE_LAUNCH_AS("SPLIT6", (r8::ntt_row8_batched_kernel<false, 3, 9, 2, false, false, true>), a->rows << (a->logN - 12), 512u,
                                   true, stream, *a))
        return false;
    }
#define FHE_CASE(INV, MODE, PP, X1P)                                                                                                  \
    FHE_INSTANCE(FHE_PASS_IS(false, INV, 12, MODE) && P == PP && x1p == X1P && !hand,                                                 \
                 FHE_LAUNCH_BARRIER_N((r8::ntt_row8_batched_kernel<INV, 3, MODE, PP, X1P>), a->rows << (a->logN - 12), 512u, stream, *a))      \
    FHE_INSTANCE(INV && FHE_PASS_IS(false, INV, 12, MODE) && P == PP && x1p == X1P && hand,                                           \
                 FHE_LAUNCH_AS("HAND", (r8::ntt_row8_batched_kernel<INV, 3, MODE, PP, X1P, INV>), a->rows << (a->logN - 12), 512u, true, stream, \
                               *a))
    FHE_CASE(false, 9, 2, false) FHE_CASE(true, 0, 2, false) FHE_CASE(false, 9, 2, true) FHE_CASE(true, 0, 2, true)
    FHE_CASE(false, 9, 4, false) FHE_CASE(true, 0, 4, false) FHE_CASE(false, 9, 4, true) FHE_CASE(true, 0, 4, true)
#undef FHE_CASE
    return false;
}
// ntt_static.h, the fused rows of fhe_poly_mul: p is the forward row pass; second = false: poly_mul_row_a, true: poly_mul_row_b
static bool poly_mul_instance(const NttPass& p, bool second, const PolyMulArgs* a, void* stream) {
#define FHE_CASE(TT)                                                                                                                \
    FHE_INSTANCE(FHE_PASS_IS(false, false, TT, 9) && !second, FHE_LAUNCH_BARRIER((poly_mul_row_a_kernel<TT>), pass_tiles(a->fwd), stream, *a)) \
    FHE_INSTANCE(FHE_PASS_IS(false, false, TT, 9) && second, FHE_LAUNCH_BARRIER((poly_mul_row_b_kernel<TT>), pass_tiles(a->fwd), stream, *a))
    FHE_CASE(12) FHE_CASE(11) FHE_CASE(10) FHE_CASE(9)
#undef FHE_CASE
    return false;
}
#undef FHE_INSTANCE
#undef FHE_PASS_IS

// does a forward transform of this ring end in a kernel that can carry the fused epilogue?
static bool ntt_epilogue_supported(const fhe_ctx* c) {
    const NttPasses f = ntt_passes(c, false);
    return static_epilogue_instance(f.p[f.n - 1], nullptr, nullptr);
}
// a two-pass forward transform whose column pass can carry the load prologue (NttPassArgs::proMode)
static bool ntt_prologue_supported(const fhe_ctx* c) {
    const NttPasses f = ntt_passes(c, false);
    return f.n == 2 && static_prologue_instance(f.p[0], nullptr, nullptr);
}

static void fill_pass_args(const fhe_ctx* c, const NttPass& p, const uint64_t* xin, uint64_t* xout, const LimbSel& sel, uint32_t nLimbs,
                           uint32_t batch, const NttOpts& o, NttPassArgs& a) {
    a.outStride = o.dst.stride;
    a.outFirst  = o.dst.first;
    a.inStride  = o.src.stride;
    a.inFirst   = o.src.first;
    a.inDelta   = o.srcDelta;
    a.xin       = xin;
    a.x         = xout;
    a.tw        = p.inverse ? c->d_twInv : c->d_tw;
    a.twRow     = p.inverse ? c->d_twRowInv : c->d_twRow;
    a.q         = c->d_q;
    a.red       = c->d_red;
    a.fin       = c->d_fin;
    a.logN      = c->logN;
    a.T         = p.T;
    a.nLimbs    = nLimbs;
    a.rows      = batch * nLimbs;
    a.batch     = batch;
    // the plan of ntt_pass_kernel (launch_small fills it in): every other kernel has its own and only asks whether canonStep is set
    a.nSteps = a.canonLevels = 0;
    a.canonStep              = o.canonOut ? 0u : 0xffffffffu;
    for (NttStep& st : a.steps)
        st = NttStep{0, 0, -1, 0, 0, 0, 0, 0};
    a.sel = sel;
    const uint32_t tilesPerRow = c->N >= (uint32_t)kTile ? (c->N >> kTileLog) : 1u;
    a.xcdSwizzle = (c->N >= (uint32_t)kTile && ((nLimbs * tilesPerRow) % 8u == 0)) ? 1u : 0u;
    static const NttEpilogue noEpi;
    const NttEpilogue& e = o.epi && o.epi->mode ? *o.epi : noEpi;
    a.epiMode = e.mode, a.epiSplit = e.split, a.epiAStride = e.aStride, a.epiAFirst = e.aFirst;
    a.epiA = e.A, a.epiC = e.C, a.epiOut0 = e.out0, a.epiOut1 = e.out1, a.epiADelta = e.aDelta;
    a.proMode = o.proSrcLimb ? (o.proRows ? 3 : o.proC ? 2 : 1) : 0, a.proSrcLimb = o.proSrcLimb ? *o.proSrcLimb : 0;
    a.proC = o.proSrcLimb ? o.proC : nullptr;
    a.proRows = o.proSrcLimb ? o.proRows : 0;
    a.split6Batch = 0;
    for (uint32_t k = 0; k < 4; ++k)
        a.proSrcLimbs[k] = k < a.proRows ? o.proSrcLimb[k] : 0;
}
// the first n polynomials of the pass's batch as a pass of their own; `a` goes on with the rest, on the same stream, as the same pass over a
// view that starts at its first polynomial
static NttPassArgs split_head(NttPassArgs& a, uint32_t n) {
    NttPassArgs h = a;
    h.batch       = n;
    h.rows        = n * a.nLimbs;
    a.xin += a.inDelta ? (int64_t)n * a.inDelta : (int64_t)(((uint64_t)n * (a.inStride ? a.inStride : a.nLimbs)) << a.logN);
    a.x += ((uint64_t)n * (a.outStride ? a.outStride : a.nLimbs)) << a.logN;
    a.batch -= n;
    a.rows = a.batch * a.nLimbs;
    return h;
}
// Hand-over between the two passes of an INVERSE 4 + 12-stage transform (ntt_row8.h / ntt_static.h, HAND): the column pass does the
// twiddle products of the row pass's last stage.  The pair runs for exactly the part of a transform that the batched 12-stage row kernel takes:
// ntt_run decides it once (handP = that kernel's P) and only for a plain transform with canonical output, and both passes are then launched in the
// same two parts, the P-aligned one with hand-over and the remainder on the kernels every other consumer of the intermediate tower uses.
static fhe_status launch_pass(const fhe_ctx* c, const NttPass& p, const uint64_t* xin, uint64_t* xout, const LimbSel& sel, uint32_t nLimbs,
                              uint32_t batch, void* stream, const NttOpts& o = NttOpts(), uint32_t handP = 0, uint32_t splitP = 0) {
    NttPassArgs a;
    fill_pass_args(c, p, xin, xout, sel, nLimbs, batch, o, a);
    // the route of this pass for this batch: a head of whole groups of headP polynomials on a kernel of its own, the rest on another
    enum { Small, Static, Epilogue, Prologue, Row8 } rest = c->logN < (uint32_t)kTileLog ? Small : Static;
    uint32_t headP = 0;
    if (o.srcDelta && rest == Small)  // (the static and row8 kernels only)
        return fail(FHE_ERR_UNSUPPORTED, "ntt: separately allocated towers need a ring of at least 4096");
    if (o.proSrcLimb) {
        rest = Prologue;
        if (!static_prologue_instance(p, nullptr, nullptr))
            return fail(FHE_ERR_UNSUPPORTED, "ntt: no prologue kernel for this pass shape");
    }
    else if (a.epiMode) {
        rest = Epilogue;
        if (!static_epilogue_instance(p, nullptr, nullptr))
            return fail(FHE_ERR_UNSUPPORTED, "ntt: no epilogue kernel for this pass shape");
    }
    else if (rest != Small) {
        const uint32_t P = p.kind == NttPass::Row ? row8_batch_for(p.T) : 1u;
        // a transform with hand-over: both passes must land on the hand-over instances, or the intermediate tower is misread
        if (handP && !(batch >= handP && (p.layoutA() ? static_handover_instance(p, nullptr, nullptr)
                                                      : P == handP && row8_batched_instance(p, P, true, false, nullptr, nullptr))))
            return fail(FHE_ERR_UNSUPPORTED, "ntt: no hand-over kernel for this pass shape");
        // ... and so must the two passes of a forward transform on the 6 + 10 split
        if (splitP && !(batch >= splitP && (p.layoutA() ? static_split6_instance(p, nullptr, nullptr)
                                                        : P == splitP && row8_batched_instance(p, P, false, true, nullptr, nullptr))))
            return fail(FHE_ERR_UNSUPPORTED, "ntt: no kernel of the 6 + 10 split for this pass shape");
        if (splitP && p.layoutA()) {
            // ONE launch for the whole batch: six stages for the part that the batched row kernel takes, four for the remainder
            a.split6Batch = batch / splitP * splitP;
            static_split6_instance(p, &a, stream);
            LAUNCH_CHECK();
            return FHE_OK;
        }
        if (handP && p.layoutA())
            headP = handP;  // the column pass of the part of the batch that the batched row kernel takes
        else if (P > 1 && batch >= P && row8_batched_instance(p, P, handP != 0, splitP != 0, nullptr, nullptr))
            headP = P;
        if (p.kind == NttPass::Row && row8_for(p.T) && row8_instance(p, nullptr, nullptr))
            rest = Row8;
        else if (!static_instance(p, nullptr, nullptr))
            return fail(FHE_ERR_UNSUPPORTED, "ntt: no kernel instance for this pass shape");
    }
    if (headP) {
        NttPassArgs h = split_head(a, batch / headP * headP);
        if (p.layoutA())
            static_handover_instance(p, &h, stream);
        else
            h = row8_args(h, headP), row8_batched_instance(p, headP, handP != 0, splitP != 0, &h, stream);
    }
    if (a.batch)
        switch (rest) {
            case Static: static_instance(p, &a, stream); break;
            case Epilogue: static_epilogue_instance(p, &a, stream); break;
            case Prologue: static_prologue_instance(p, &a, stream); break;
            case Row8: a = row8_args(a, 1), row8_instance(p, &a, stream); break;
            case Small: launch_small(p, o.canonOut, a, stream); break;
        }
    LAUNCH_CHECK();
    return FHE_OK;
}

static fhe_status ntt_run(fhe_ctx* c, bool inverse, const uint64_t* xin, uint64_t* xout, const uint32_t* limbIdx, uint32_t nLimbs,
                          uint32_t batch, void* stream, const NttOpts& o = NttOpts()) {
    ARG_CHECK(c && xin && xout, "fhe_ntt: null argument");
    ARG_CHECK(batch >= 1, "fhe_ntt: batch must be >= 1");
    LimbSel sel;
    if (fhe_status s = make_sel(c, limbIdx, nLimbs, &sel, "fhe_ntt"))
        return s;
    RT_CHECK(rt::set_device(c->device));
    const NttPasses ps = ntt_passes(c, inverse);
    if (ps.n == 1)
        return launch_pass(c, ps.p[0], xin, xout, sel, nLimbs, batch, stream, o);
    // Two passes over HBM, both of the whole batch back to back on the caller's stream.  What else was built and measured, bit-exact and
    // slower or equal, and removed again (profiles/r02_sweeps.md session 3, profiles/r05_sweeps.md): both passes in one launch with the tower
    // kept in an XCD's L2 (no retention); launches per chunk sized to the Infinity Cache (its bandwidth is within 15 % of HBM's);
    // the column pass of one chunk and the row pass of another on two streams (the queues split a CU's four workgroup slots: the
    // pair takes the sum of its parts) or as one grid of alternating roles (6 % slower); persistent pass kernels (11 % slower: a
    // fresh workgroup's loads overlap the drain of its predecessor's stores); 5 + 11 stages instead of 4 + 12 (1 % slower).
    // THE hand-over decision (launch_pass): the plain inverse 4 + 12 transform with canonical output, for the part of the batch the batched row
    // kernel takes.  A transform whose output stays lazy keeps the parent's words (another representative of the boundary product would show in
    // them), and the epilogue and prologue instances keep the plain intermediate tower.
    const uint32_t rowP  = inverse ? row8_batch_for(ps.p[0].T) : 1u;
    const uint32_t handP = (o.canonOut && !(o.epi && o.epi->mode) && !o.proSrcLimb && ntt_switches().handover && rowP >= 2 &&
                            batch >= rowP && row8_batched_instance(ps.p[0], rowP, true, false, nullptr, nullptr) &&
                            static_handover_instance(ps.p[1], nullptr, nullptr))
                               ? rowP
                               : 0u;
    // THE decision on the 6 + 10 split of N = 2^16, forward transforms only: the column pass runs six stages (ntt_static.h, SPLIT),
    // the batched row pass ten in its 12-stage tile (ntt_row8.h, SPLIT).  Taken for exactly the part of a plain transform -- no load prologue, no
    // fused epilogue; canonical or lazy output -- that the batched row kernel takes at its default P = 2; a forced FHE_NTT_ROW8, FHE_NTT_T1 or
    // another P keep 4 + 12, and so does every other consumer of the intermediate tower.  (The inverse pair, 10 + 6 behind the hand-over, was
    // built and measured slower than the hand-over pair: profiles/ntt_split6.md.)
    const NttSwitches& sw = ntt_switches();
    const uint32_t fwdP   = inverse ? 1u : row8_batch_for(ps.p[1].T);
    const uint32_t splitP = (!inverse && sw.split6 && c->logN == 16u && !(o.epi && o.epi->mode) && !o.proSrcLimb && sw.row8 < 0 && !sw.t1 &&
                             fwdP == 2u && batch >= fwdP && static_split6_instance(ps.p[0], nullptr, nullptr) &&
                             row8_batched_instance(ps.p[1], fwdP, false, true, nullptr, nullptr))
                                ? fwdP
                                : 0u;
    // the first pass reads the source into the destination's rows and leaves them lazy; the second runs in place there and ends the transform
    NttOpts first = o, second;
    first.epi = nullptr, first.canonOut = false;
    second.src = second.dst = o.dst;
    second.epi = o.epi, second.canonOut = o.canonOut;
    if (fhe_status s = launch_pass(c, ps.p[0], xin, xout, sel, nLimbs, batch, stream, first, handP, splitP))
        return s;
    return launch_pass(c, ps.p[1], xout, xout, sel, nLimbs, batch, stream, second, handP, splitP);
}

extern "C" fhe_status fhe_ntt_fwd(fhe_ctx* c, uint64_t* x, const uint32_t* li, uint32_t nl, uint32_t b, void* st) {
    return ntt_run(c, false, x, x, li, nl, b, st);
}
extern "C" fhe_status fhe_ntt_inv(fhe_ctx* c, uint64_t* x, const uint32_t* li, uint32_t nl, uint32_t b, void* st) {
    return ntt_run(c, true, x, x, li, nl, b, st);
}
extern "C" fhe_status fhe_ntt_fwd_oop(fhe_ctx* c, const uint64_t* xi, uint64_t* xo, const uint32_t* li, uint32_t nl,
                                      uint32_t b, void* st) {
    return ntt_run(c, false, xi, xo, li, nl, b, st);
}
extern "C" fhe_status fhe_ntt_inv_oop(fhe_ctx* c, const uint64_t* xi, uint64_t* xo, const uint32_t* li, uint32_t nl,
                                      uint32_t b, void* st) {
    return ntt_run(c, true, xi, xo, li, nl, b, st);
}

// ---- negacyclic polynomial product of COEFFICIENT-format towers: c = INTT(NTT(a) o NTT(b)) per limb ----
// What a caller of the reference writes as a.SetFormat(EVALUATION); b.SetFormat(EVALUATION); c = a * b; c.SetFormat(COEFFICIENT)
// (dcrtpoly-impl.h:1932-1940, dcrtpoly.h:174-189): three transforms and a Hadamard product.  Two-pass rings whose row pass has a
// poly_mul_row_* instance (ntt_static.h) run those fused kernels; every other ring runs the plain sequence.
extern "C" size_t fhe_poly_mul_workspace_bytes(const fhe_ctx* c, uint32_t nLimbs, uint32_t batch) {
    return c ? (((size_t)2 * batch * nLimbs) << c->logN) * 8 : 0;
}
extern "C" fhe_status fhe_poly_mul(fhe_ctx* c, const uint64_t* a, const uint64_t* b, uint64_t* out, const uint32_t* limbIdx,
                                   uint32_t nLimbs, uint32_t batch, void* wsv, size_t wsBytes, void* stream) {
    ARG_CHECK(c && a && b && out && wsv, "fhe_poly_mul: null argument");
    ARG_CHECK(batch >= 1, "fhe_poly_mul: batch must be >= 1");
    ARG_CHECK(wsBytes >= fhe_poly_mul_workspace_bytes(c, nLimbs, batch), "fhe_poly_mul: workspace too small");
    LimbSel sel;
    if (fhe_status s = make_sel(c, limbIdx, nLimbs, &sel, "fhe_poly_mul"))
        return s;
    RT_CHECK(rt::set_device(c->device));
    uint64_t* wa = (uint64_t*)wsv;
    uint64_t* wb = wa + (((size_t)batch * nLimbs) << c->logN);
    const NttPasses f = ntt_passes(c, false), i = ntt_passes(c, true);  // forward column, row; inverse row, column
    if (f.n != 2 || !poly_mul_instance(f.p[1], false, nullptr, nullptr)) {
        if (fhe_status s = ntt_run(c, false, a, wa, limbIdx, nLimbs, batch, stream))
            return s;
        if (fhe_status s = ntt_run(c, false, b, wb, limbIdx, nLimbs, batch, stream))
            return s;
        if (fhe_status s = fhe_mul(c, out, wa, wb, limbIdx, nLimbs, batch, stream))
            return s;
        return ntt_run(c, true, out, out, limbIdx, nLimbs, batch, stream);
    }
    NttOpts lazy;
    lazy.canonOut = false;
    // column passes of a and b, out of place into the workspace
    if (fhe_status s = launch_pass(c, f.p[0], a, wa, sel, nLimbs, batch, stream, lazy))
        return s;
    if (fhe_status s = launch_pass(c, f.p[0], b, wb, sel, nLimbs, batch, stream, lazy))
        return s;
    PolyMulArgs g;
    fill_pass_args(c, f.p[1], wa, wa, sel, nLimbs, batch, NttOpts(), g.fwd);
    g.fwd.xcdSwizzle = 0;  // block id = tile: the workspace tile of a block is addressed by its id
    g.inv = g.fwd;
    g.aEval = wa;
    g.lc = c->d_lc;
    poly_mul_instance(f.p[1], false, &g, stream);
    LAUNCH_CHECK();
    fill_pass_args(c, f.p[1], wb, wb, sel, nLimbs, batch, NttOpts(), g.fwd);
    fill_pass_args(c, i.p[0], out, out, sel, nLimbs, batch, lazy, g.inv);
    g.fwd.xcdSwizzle = g.inv.xcdSwizzle = 0;
    poly_mul_instance(f.p[1], true, &g, stream);
    LAUNCH_CHECK();
    // inverse column pass: ends the transform (N^-1 folded in, canonical residues)
    return launch_pass(c, i.p[1], out, out, sel, nLimbs, batch, stream);
}

// dir: 0 fwd, 1 inv, 2 fwd then inv; 10/11 = only the column / row pass of the forward transform,
// 12/13 = only the row / column pass of the inverse (two-pass rings; timing only, data is not meaningful)
extern "C" fhe_status fhe_time_ntt(fhe_ctx* c, uint64_t* x, const uint32_t* li, uint32_t nl, uint32_t b, int dir,
                                   int iters, void* st, float* ms) {
    ARG_CHECK(c && x && ms && iters > 0, "fhe_time_ntt: bad argument");
    LimbSel sel;
    if (fhe_status s = make_sel(c, li, nl, &sel, "fhe_time_ntt"))
        return s;
    RT_CHECK(rt::set_device(c->device));
    NttPass pp;
    NttOpts lazy;
    lazy.canonOut = false;
    if (dir >= 10) {
        ARG_CHECK(c->logN > (uint32_t)kTileLog && dir <= 13, "fhe_time_ntt: single-pass timing needs a two-pass ring");
        pp = ntt_passes(c, dir >= 12).p[dir & 1];  // (the passes in the order they run)
    }
    rt::Timer tm;
    RT_CHECK(tm.start((rt::stream_t)st));
    for (int i = 0; i < iters; ++i) {
        if (dir >= 10) {
            if (fhe_status s = launch_pass(c, pp, x, x, sel, nl, b, st, lazy))
                return s;
            continue;
        }
        if (dir == 0 || dir == 2)
            if (fhe_status s = fhe_ntt_fwd(c, x, li, nl, b, st))
                return s;
        if (dir == 1 || dir == 2)
            if (fhe_status s = fhe_ntt_inv(c, x, li, nl, b, st))
                return s;
    }
    float total = 0;
    RT_CHECK(tm.stop((rt::stream_t)st, &total));
    *ms = total / iters;
    return FHE_OK;
}

// ------------------------------------------------------------------------------------------------
// element-wise
// ------------------------------------------------------------------------------------------------
template <int OP>
static fhe_status elem_run(fhe_ctx* c, uint64_t* out, const uint64_t* a, const uint64_t* b, const TwPair* d_consts,
                           const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, void* stream, const char* who,
                           uint32_t aStride = 0, uint32_t aFirst = 0, uint32_t bStride = 0, uint32_t bFirst = 0,
                           uint32_t oStride = 0, uint32_t oFirst = 0, const int64_t* deltas = nullptr) {
    ARG_CHECK(c && out && a, std::string(who) + ": null argument");
    ARG_CHECK(batch >= 1, std::string(who) + ": batch must be >= 1");
    ElemArgs g;
    if (fhe_status s = make_sel(c, limbIdx, nLimbs, &g.sel, who))
        return s;
    RT_CHECK(rt::set_device(c->device));
    g.out    = out;
    g.a      = a;
    g.b      = b;
    g.lc     = c->d_lc;
    g.consts = d_consts;
    g.logN   = c->logN;
    g.nLimbs = nLimbs;
    g.rows   = batch * nLimbs;
    g.aStride = aStride, g.aFirst = aFirst, g.bStride = bStride, g.bFirst = bFirst;
    g.oStride = oStride, g.oFirst = oFirst;
    if (deltas)  // towers allocated on their own: words between tower 0 and tower 1 of out / a / b
        g.oDelta = deltas[0], g.aDelta = deltas[1], g.bDelta = deltas[2];
    FHE_LAUNCH((elemwise_kernel<OP>), tiles_for(c, g.rows), stream, g);
    LAUNCH_CHECK();
    return FHE_OK;
}
extern "C" fhe_status fhe_add(fhe_ctx* c, uint64_t* o, const uint64_t* a, const uint64_t* b, const uint32_t* li,
                              uint32_t nl, uint32_t bt, void* st) {
    ARG_CHECK(b, "fhe_add: null argument");
    return elem_run<OP_ADD>(c, o, a, b, nullptr, li, nl, bt, st, "fhe_add");
}
extern "C" fhe_status fhe_sub(fhe_ctx* c, uint64_t* o, const uint64_t* a, const uint64_t* b, const uint32_t* li,
                              uint32_t nl, uint32_t bt, void* st) {
    ARG_CHECK(b, "fhe_sub: null argument");
    return elem_run<OP_SUB>(c, o, a, b, nullptr, li, nl, bt, st, "fhe_sub");
}
extern "C" fhe_status fhe_mul(fhe_ctx* c, uint64_t* o, const uint64_t* a, const uint64_t* b, const uint32_t* li,
                              uint32_t nl, uint32_t bt, void* st) {
    ARG_CHECK(b, "fhe_mul: null argument");
    return elem_run<OP_MUL>(c, o, a, b, nullptr, li, nl, bt, st, "fhe_mul");
}
// acc += a * b per limb (exact): the accumulation of KeySwitchHYBRID::EvalFastKeySwitchCoreExt, keyswitch-hybrid.cpp:419-430
// (`elements[k].SetElementAtIndex(i, elements[k].GetElementAtIndex(i) + cji * bji)`), on whole towers
extern "C" fhe_status fhe_mul_add(fhe_ctx* c, uint64_t* acc, const uint64_t* a, const uint64_t* b, const uint32_t* li,
                                  uint32_t nl, uint32_t bt, void* st) {
    ARG_CHECK(b, "fhe_mul_add: null argument");
    return elem_run<OP_MULT_ACC>(c, acc, a, b, nullptr, li, nl, bt, st, "fhe_mul_add");
}
extern "C" fhe_status fhe_neg(fhe_ctx* c, uint64_t* o, const uint64_t* a, const uint32_t* li, uint32_t nl, uint32_t bt,
                              void* st) {
    return elem_run<OP_NEG>(c, o, a, nullptr, nullptr, li, nl, bt, st, "fhe_neg");
}

// per-call constant vectors (Times(vector<NativeInteger>), MultAccEqNoCheck ...): the host constants become Shoup pairs
// and travel BY VALUE in the kernel arguments — no staging buffer, no synchronisation, capturable into a HIP graph
// (the whole vector on the host; a launch carries a window of kConstVecLimbs rows of it: launch_cv)
struct HostConstVec {
    TwPair c[kMaxLimbs];
};
template <int OP>
static void launch_cv(fhe_ctx* c, ElemArgs g, const HostConstVec& cv, void* stream) {
    for (uint32_t first = 0; first < g.nLimbs; first += (uint32_t)kConstVecLimbs) {
        ConstVec w;
        for (uint32_t i = 0; i < (uint32_t)kConstVecLimbs; ++i)
            w.c[i] = first + i < (uint32_t)kMaxLimbs ? cv.c[first + i] : TwPair{0, 0};
        g.cvFirst = first;
        FHE_LAUNCH((elemwise_cv_kernel<OP>), tiles_for(c, g.rows), stream, g, w);
    }
}
static fhe_status make_const_vec(const fhe_ctx* c, const uint64_t* consts, const uint32_t* limbIdx, uint32_t nLimbs,
                                 HostConstVec* cv, const char* who) {
    ARG_CHECK(c && consts, std::string(who) + ": null argument");
    ARG_CHECK(nLimbs >= 1 && nLimbs <= (uint32_t)kMaxLimbs, std::string(who) + ": nLimbs out of range");
    for (uint32_t i = 0; i < (uint32_t)kMaxLimbs; ++i)
        cv->c[i] = TwPair{0, 0};
    for (uint32_t i = 0; i < nLimbs; ++i) {
        const uint32_t l = limbIdx ? limbIdx[i] : i;
        ARG_CHECK(l < c->L, std::string(who) + ": limb index exceeds context size");
        const uint64_t ql = c->q[l], v = consts[i] % ql;
        cv->c[i]          = TwPair{v, host::shoup(v, ql)};
    }
    return FHE_OK;
}
template <int OP>
static fhe_status elem_cv_run(fhe_ctx* c, uint64_t* out, const uint64_t* a, const uint64_t* b, const HostConstVec& cv,
                              const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, void* stream, const char* who,
                              uint32_t oStride = 0, uint32_t oFirst = 0, const int64_t* deltas = nullptr) {
    ARG_CHECK(c && out && a, std::string(who) + ": null argument");
    ARG_CHECK(batch >= 1, std::string(who) + ": batch must be >= 1");
    ElemArgs g;
    if (fhe_status s = make_sel(c, limbIdx, nLimbs, &g.sel, who))
        return s;
    RT_CHECK(rt::set_device(c->device));
    g.out = out, g.a = a, g.b = b, g.lc = c->d_lc, g.consts = nullptr;
    g.logN = c->logN, g.nLimbs = nLimbs, g.rows = batch * nLimbs;
    g.aStride = g.aFirst = g.bStride = g.bFirst = 0;
    g.oStride = oStride, g.oFirst = oFirst;
    if (deltas)
        g.oDelta = deltas[0], g.aDelta = deltas[1], g.bDelta = deltas[2];
    launch_cv<OP>(c, g, cv, stream);
    LAUNCH_CHECK();
    return FHE_OK;
}
extern "C" fhe_status fhe_mul_const(fhe_ctx* c, uint64_t* o, const uint64_t* a, const uint64_t* consts,
                                    const uint32_t* li, uint32_t nl, uint32_t bt, void* st) {
    HostConstVec cv;
    if (fhe_status s = make_const_vec(c, consts, li, nl, &cv, "fhe_mul_const"))
        return s;
    return elem_cv_run<OP_MUL_CONST>(c, o, a, nullptr, cv, li, nl, bt, st, "fhe_mul_const");
}
static fhe_status const_table(fhe_ctx* c, const uint32_t* limbIdx, const uint64_t* v, uint32_t n, const TwPair** out);
static fhe_status const_tables_trim(fhe_ctx* c);
// out = sum_i consts[i][.] (.) x[i]  (+ out when accumulate): the weighted sums of pke (ckksrns-advancedshe.cpp:97-136) as ONE launch per
// 16 terms.  consts: HOST array [nTerms][nLimbs], reduced modulo their limbs; their device table is cached by content (the Chebyshev
// coefficients of a bootstrap repeat), so only the first use of a table blocks for its upload.
extern "C" fhe_status fhe_lincomb(fhe_ctx* c, uint64_t* out, const uint64_t* const* x, const uint64_t* consts, uint32_t nTerms,
                                  const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, int accumulate, void* stream) {
    ARG_CHECK(c && out && x && consts && nTerms >= 1 && batch >= 1, "fhe_lincomb: bad argument");
    LinCombArgs g;
    if (fhe_status s = make_sel(c, limbIdx, nLimbs, &g.sel, "fhe_lincomb"))
        return s;
    RT_CHECK(rt::set_device(c->device));
    // More than kMaxLinTerms terms take several launches and the first one overwrites `out`: terms that ARE `out` go into the first
    // launch (a launch reads every word before it writes it), so the sum is right wherever the caller put them.
    std::vector<uint32_t> order;
    order.reserve(nTerms);
    for (uint32_t i = 0; i < nTerms; ++i)
        if (x[i] == out)
            order.push_back(i);
    ARG_CHECK(order.size() <= (size_t)kMaxLinTerms || nTerms <= (uint32_t)kMaxLinTerms,
              "fhe_lincomb: more than 16 of more than 16 terms alias out");
    if (nTerms <= (uint32_t)kMaxLinTerms)
        order.clear();
    const size_t nAliased = order.size();
    for (uint32_t i = 0; i < nTerms; ++i)
        if (!(nAliased && x[i] == out))
            order.push_back(i);
    std::vector<uint32_t> li((size_t)nTerms * nLimbs);
    std::vector<uint64_t> cs((size_t)nTerms * nLimbs);
    for (uint32_t i = 0; i < nTerms; ++i)
        for (uint32_t r = 0; r < nLimbs; ++r) {
            li[(size_t)i * nLimbs + r] = limbIdx ? limbIdx[r] : r;
            cs[(size_t)i * nLimbs + r] = consts[(size_t)order[i] * nLimbs + r];
        }
    const TwPair* table = nullptr;
    if (fhe_status s = const_tables_trim(c))
        return s;
    std::shared_lock<std::shared_mutex> gate(c->constTabsGate);
    if (fhe_status s = const_table(c, li.data(), cs.data(), nTerms * nLimbs, &table))
        return s;
    g.out = out, g.q = c->d_q, g.logN = c->logN, g.nLimbs = nLimbs, g.rows = batch * nLimbs;
    for (uint32_t first = 0; first < nTerms; first += (uint32_t)kMaxLinTerms) {
        const uint32_t n = std::min<uint32_t>(kMaxLinTerms, nTerms - first);
        for (uint32_t i = 0; i < (uint32_t)kMaxLinTerms; ++i) {
            g.x[i] = i < n ? x[order[first + i]] : nullptr;
            ARG_CHECK(i >= n || g.x[i], "fhe_lincomb: null term");
        }
        g.consts = table + (size_t)first * nLimbs, g.nTerms = n, g.accumulate = (accumulate || first) ? 1u : 0u;
        FHE_LAUNCH(lincomb_kernel, tiles_for(c, g.rows), stream, g);
        LAUNCH_CHECK();
    }
    return FHE_OK;
}
// ---- the two elements of a ciphertext in ONE launch: towers 0 and 1 of every operand are separately allocated buffers ----
// (pke applies every operation element by element, base-leveledshe.cpp:562-606, ckksrns-leveledshe.cpp:748-759: at one ciphertext
// a launch per element leaves most of the chip idle — a tower of 14 limbs at N = 2^17 is 448 workgroups for 1024 resident slots)
static bool pair_deltas(const uint64_t* o0, const uint64_t* o1, const uint64_t* a0, const uint64_t* a1, const uint64_t* b0,
                        const uint64_t* b1, int64_t d[3]) {
    d[0] = o1 - o0, d[1] = a1 - a0, d[2] = b0 ? b1 - b0 : 1;
    return d[0] != 0 && d[1] != 0 && d[2] != 0;  // (0 means "dense" to the kernels: distinct towers are never 0 apart)
}
extern "C" fhe_status fhe_add_pair(fhe_ctx* c, uint64_t* o0, uint64_t* o1, const uint64_t* a0, const uint64_t* a1, const uint64_t* b0,
                                   const uint64_t* b1, const uint32_t* li, uint32_t nl, void* st) {
    int64_t d[3];
    ARG_CHECK(o0 && o1 && a0 && a1 && b0 && b1 && pair_deltas(o0, o1, a0, a1, b0, b1, d), "fhe_add_pair: bad argument");
    return elem_run<OP_ADD>(c, o0, a0, b0, nullptr, li, nl, 2, st, "fhe_add_pair", 0, 0, 0, 0, 0, 0, d);
}
extern "C" fhe_status fhe_sub_pair(fhe_ctx* c, uint64_t* o0, uint64_t* o1, const uint64_t* a0, const uint64_t* a1, const uint64_t* b0,
                                   const uint64_t* b1, const uint32_t* li, uint32_t nl, void* st) {
    int64_t d[3];
    ARG_CHECK(o0 && o1 && a0 && a1 && b0 && b1 && pair_deltas(o0, o1, a0, a1, b0, b1, d), "fhe_sub_pair: bad argument");
    return elem_run<OP_SUB>(c, o0, a0, b0, nullptr, li, nl, 2, st, "fhe_sub_pair", 0, 0, 0, 0, 0, 0, d);
}
extern "C" fhe_status fhe_mul_const_pair(fhe_ctx* c, uint64_t* o0, uint64_t* o1, const uint64_t* a0, const uint64_t* a1,
                                         const uint64_t* consts, const uint32_t* li, uint32_t nl, void* st) {
    int64_t d[3];
    ARG_CHECK(o0 && o1 && a0 && a1 && pair_deltas(o0, o1, a0, a1, nullptr, nullptr, d), "fhe_mul_const_pair: bad argument");
    HostConstVec cv;
    if (fhe_status s = make_const_vec(c, consts, li, nl, &cv, "fhe_mul_const_pair"))
        return s;
    return elem_cv_run<OP_MUL_CONST>(c, o0, a0, nullptr, cv, li, nl, 2, st, "fhe_mul_const_pair", 0, 0, d);
}
// DCRTPolyImpl::Plus(vector<Integer>) (dcrtpoly-impl.h:520-527 -> PolyImpl::Plus(Integer), poly-impl.h:211-218): limb i plus the
// constant polynomial consts[i] — every word in EVALUATION, coefficient 0 only in COEFFICIENT (coeff0Only)
extern "C" fhe_status fhe_add_const(fhe_ctx* c, uint64_t* o, const uint64_t* a, const uint64_t* consts, const uint32_t* li,
                                    uint32_t nl, uint32_t bt, int coeff0Only, void* st) {
    HostConstVec cv;
    if (fhe_status s = make_const_vec(c, consts, li, nl, &cv, "fhe_add_const"))
        return s;
    if (coeff0Only)
        return elem_cv_run<OP_ADD_CONST_AT0>(c, o, a, nullptr, cv, li, nl, bt, st, "fhe_add_const");
    return elem_cv_run<OP_ADD_CONST>(c, o, a, nullptr, cv, li, nl, bt, st, "fhe_add_const");
}
// DCRTPolyImpl::Minus(vector<Integer>) (dcrtpoly-impl.h:541-548 -> PolyImpl::Minus(Integer), poly-impl.h:221-225: ModSub on
// every word in both formats)
extern "C" fhe_status fhe_sub_const(fhe_ctx* c, uint64_t* o, const uint64_t* a, const uint64_t* consts, const uint32_t* li,
                                    uint32_t nl, uint32_t bt, void* st) {
    HostConstVec cv;
    if (fhe_status s = make_const_vec(c, consts, li, nl, &cv, "fhe_sub_const"))
        return s;
    for (uint32_t i = 0; i < nl; ++i) {  // a - k = a + (q - k)
        const uint64_t ql = c->q[li ? li[i] : i], k = cv.c[i].w;
        cv.c[i]           = TwPair{k ? ql - k : 0, 0};
    }
    return elem_cv_run<OP_ADD_CONST>(c, o, a, nullptr, cv, li, nl, bt, st, "fhe_sub_const");
}
// DCRTPolyImpl::TimesQovert (dcrtpoly-impl.h:868-885): every word x of limb i becomes ((x * NegQModt) mod t) * tInvModq[i] mod q_i
// (ModMulFastConst modulo t, then the generalized Barrett product modulo q_i); BFV encryption's scaling of the message by Q/t
extern "C" fhe_status fhe_times_q_over_t(fhe_ctx* c, uint64_t* o, const uint64_t* a, uint64_t t, uint64_t negQModt,
                                         const uint64_t* tInvModq, const uint32_t* li, uint32_t nl, uint32_t bt, void* st) {
    ARG_CHECK(c && o && a && tInvModq && t >= 2 && bt >= 1, "fhe_times_q_over_t: bad argument");
    HostConstVec cv;
    if (fhe_status s = make_const_vec(c, tInvModq, li, nl, &cv, "fhe_times_q_over_t"))
        return s;
    ElemArgs g;
    if (fhe_status s = make_sel(c, li, nl, &g.sel, "fhe_times_q_over_t"))
        return s;
    RT_CHECK(rt::set_device(c->device));
    g.out = o, g.a = a, g.b = nullptr, g.lc = c->d_lc, g.consts = nullptr;
    g.logN = c->logN, g.nLimbs = nl, g.rows = bt * nl;
    g.aStride = g.aFirst = g.bStride = g.bFirst = g.oStride = g.oFirst = 0;
    g.pre = TwPair{negQModt % t, host::shoup(negQModt % t, t)}, g.preMod = t;
    launch_cv<OP_TIMES_QOVERT>(c, g, cv, st);
    LAUNCH_CHECK();
    return FHE_OK;
}
// DCRTPolyImpl::SetValuesModSwitch (dcrtpoly-impl.h:630-647) on `words` COEFFICIENT words modulo qFrom -> residues modulo qTo
extern "C" fhe_status fhe_mod_switch_round(fhe_ctx* c, const uint64_t* x, uint64_t qFrom, uint64_t qTo, uint64_t* out, size_t words,
                                           void* st) {
    ARG_CHECK(c && x && out && qFrom >= 2 && qTo >= 2 && words >= 1, "fhe_mod_switch_round: bad argument");
    RT_CHECK(rt::set_device(c->device));
    ModSwitchRoundArgs g;
    g.x = x, g.out = out, g.qTo = qTo, g.words = words;
    g.ratio = static_cast<double>(qTo) / static_cast<double>(qFrom);  // :641
    FHE_LAUNCH(mod_switch_round_kernel, (words + kThreads - 1) / kThreads, st, g);
    LAUNCH_CHECK();
    return FHE_OK;
}
// NativeVectorT::MultAccEqNoCheck per limb (mubintvecnat.cpp:132-142): acc[r] += v[r] * I[r]  (I reduced first, Shoup
// product, ModAddFastEq)
extern "C" fhe_status fhe_mult_acc(fhe_ctx* c, uint64_t* acc, const uint64_t* v, const uint64_t* consts,
                                   const uint32_t* li, uint32_t nl, uint32_t bt, void* st) {
    HostConstVec cv;
    if (fhe_status s = make_const_vec(c, consts, li, nl, &cv, "fhe_mult_acc"))
        return s;
    return elem_cv_run<OP_MUL_CONST_ADD>(c, acc, v, acc, cv, li, nl, bt, st, "fhe_mult_acc");
}
// DCRTPolyImpl::ExpandCRTBasisQlHat (dcrtpoly-impl.h:1167-1187): limbs [0, sizeQl) times QlHatModq[i], limbs [sizeQl, sizeQ)
// zero; x [batch][sizeQl][N] -> out [batch][sizeQ][N] over context limbs limbIdx[0..sizeQ) (format unchanged)
// rows [first, first + nRows) of every tower of out[batch][stride][N] = 0, at copy speed (zero_rows_kernel, elemwise_kernels.h)
static fhe_status zero_rows(const fhe_ctx* c, uint64_t* out, uint32_t stride, uint32_t first, uint32_t nRows, uint32_t batch, void* st) {
    if (!nRows || !batch)
        return FHE_OK;
    ZeroRowsArgs g{out, c->logN, stride, first, nRows, batch};
    FHE_LAUNCH(zero_rows_kernel, tiles_for(c, (uint64_t)batch * nRows), st, g);
    LAUNCH_CHECK();
    return FHE_OK;
}
extern "C" fhe_status fhe_expand_crt_basis_ql_hat(fhe_ctx* c, const uint64_t* x, uint32_t sizeQl, const uint64_t* QlHatModq,
                                                  const uint32_t* li, uint32_t sizeQ, uint32_t bt, uint64_t* out, void* st) {
    ARG_CHECK(c && x && out && QlHatModq, "fhe_expand_crt_basis_ql_hat: null argument");
    ARG_CHECK(sizeQl >= 1 && sizeQl <= sizeQ && sizeQ <= (uint32_t)kMaxLimbs && bt >= 1, "fhe_expand_crt_basis_ql_hat: bad sizes");
    ARG_CHECK(out != x || sizeQl == sizeQ, "fhe_expand_crt_basis_ql_hat: in-place only when no limb is appended");
    HostConstVec cv;
    if (fhe_status s = make_const_vec(c, QlHatModq, li, sizeQl, &cv, "fhe_expand_crt_basis_ql_hat"))
        return s;
    for (uint32_t i = sizeQl; i < sizeQ; ++i)
        ARG_CHECK((li ? li[i] : i) < c->L, "fhe_expand_crt_basis_ql_hat: limb index exceeds context size");
    RT_CHECK(rt::set_device(c->device));
    if (fhe_status s = zero_rows(c, out, sizeQ, sizeQl, sizeQ - sizeQl, bt, st))
        return s;
    return elem_cv_run<OP_MUL_CONST>(c, out, x, nullptr, cv, li, sizeQl, bt, st, "fhe_expand_crt_basis_ql_hat", sizeQ, 0);
}

extern "C" fhe_status fhe_tensor(fhe_ctx* c, const uint64_t* a0, const uint64_t* a1, const uint64_t* b0,
                                 const uint64_t* b1, uint64_t* d0, uint64_t* d1, uint64_t* d2, const uint32_t* li,
                                 uint32_t nl, uint32_t bt, void* st) {
    ARG_CHECK(c && a0 && a1 && b0 && b1 && d0 && d1 && d2, "fhe_tensor: null argument");
    ARG_CHECK(bt >= 1, "fhe_tensor: batch must be >= 1");
    TensorArgs g;
    if (fhe_status s = make_sel(c, li, nl, &g.sel, "fhe_tensor"))
        return s;
    RT_CHECK(rt::set_device(c->device));
    g.a0 = a0, g.a1 = a1, g.b0 = b0, g.b1 = b1, g.d0 = d0, g.d1 = d1, g.d2 = d2;
    g.lc     = c->d_lc;
    g.logN   = c->logN;
    g.nLimbs = nl;
    g.rows   = bt * nl;
    FHE_LAUNCH(tensor_kernel, tiles_for(c, g.rows), st, g);
    LAUNCH_CHECK();
    return FHE_OK;
}

// LeveledSHEBase::EvalSquareCore for 2-element ciphertexts (base-leveledshe.cpp:646-664)
extern "C" fhe_status fhe_tensor_square(fhe_ctx* c, const uint64_t* a0, const uint64_t* a1, uint64_t* d0, uint64_t* d1,
                                        uint64_t* d2, const uint32_t* li, uint32_t nl, uint32_t bt, void* st) {
    ARG_CHECK(c && a0 && a1 && d0 && d1 && d2, "fhe_tensor_square: null argument");
    ARG_CHECK(bt >= 1, "fhe_tensor_square: batch must be >= 1");
    TensorSqArgs g;
    if (fhe_status s = make_sel(c, li, nl, &g.sel, "fhe_tensor_square"))
        return s;
    RT_CHECK(rt::set_device(c->device));
    g.a0 = a0, g.a1 = a1, g.d0 = d0, g.d1 = d1, g.d2 = d2;
    g.lc = c->d_lc, g.logN = c->logN, g.nLimbs = nl, g.rows = bt * nl;
    FHE_LAUNCH(tensor_square_kernel, tiles_for(c, g.rows), st, g);
    LAUNCH_CHECK();
    return FHE_OK;
}

extern "C" fhe_status fhe_automorph(fhe_ctx* c, uint64_t* out, const uint64_t* in, uint32_t k, int evalFormat,
                                    const uint32_t* li, uint32_t nl, uint32_t bt, void* st) {
    ARG_CHECK(c && out && in, "fhe_automorph: null argument");
    ARG_CHECK(out != in, "fhe_automorph: out must not alias in");
    ARG_CHECK(k % 2 == 1, "Automorphism index not odd");  // poly-impl.h:337-338
    ARG_CHECK(bt >= 1, "fhe_automorph: batch must be >= 1");
    AutoArgs g;
    if (fhe_status s = make_sel(c, li, nl, &g.sel, "fhe_automorph"))
        return s;
    RT_CHECK(rt::set_device(c->device));
    g.out = out, g.in = in, g.q = c->d_q;
    g.logN = c->logN, g.nLimbs = nl, g.rows = bt * nl, g.k = k, g.evalFormat = evalFormat ? 1u : 0u;
    FHE_LAUNCH(automorph_kernel, tiles_for(c, g.rows), st, g);
    LAUNCH_CHECK();
    return FHE_OK;
}
static fhe_status switch_modulus_run(fhe_ctx* c, uint64_t* out, const LimbSel& sel, uint32_t nl, const uint64_t* src,
                                     uint32_t srcLimbs, uint32_t srcPos, uint32_t srcCtxLimb, const TwPair* d_consts,
                                     uint32_t bt, void* st) {
    SwitchModArgs g;
    g.out = out, g.src = src, g.q = c->d_q, g.consts = d_consts;
    g.logN = c->logN, g.nLimbs = nl, g.rows = bt * nl;
    g.srcStrideLimbs = srcLimbs, g.srcLimbPos = srcPos, g.srcCtxLimb = srcCtxLimb;
    g.sel = sel;
    FHE_LAUNCH(switch_modulus_kernel, tiles_for(c, g.rows), st, g);
    LAUNCH_CHECK();
    return FHE_OK;
}
extern "C" fhe_status fhe_switch_modulus(fhe_ctx* c, uint64_t* out, const uint32_t* li, uint32_t nl, const uint64_t* src,
                                         uint32_t srcLimbs, uint32_t srcPos, uint32_t srcCtxLimb, uint32_t bt,
                                         void* st) {
    ARG_CHECK(c && out && src, "fhe_switch_modulus: null argument");
    ARG_CHECK(srcPos < srcLimbs && srcCtxLimb < c->L && bt >= 1, "fhe_switch_modulus: bad source limb");
    LimbSel sel;
    if (fhe_status s = make_sel(c, li, nl, &sel, "fhe_switch_modulus"))
        return s;
    RT_CHECK(rt::set_device(c->device));
    return switch_modulus_run(c, out, sel, nl, src, srcLimbs, srcPos, srcCtxLimb, nullptr, bt, st);
}

// DCRTPolyImpl::CRTDecompose(baseBits) (dcrtpoly-impl.h:230-285): x [nLimbs][N] COEFFICIENT -> out [towers][nLimbs][N] EVALUATION, towers in the
// reference's order (limb 0's digits, least significant first, then limb 1's ...).  ONE launch cuts every source limb (crt_digits_kernel), ONE
// transform covers all towers.
static uint32_t crt_windows(const fhe_ctx* c, uint32_t limb, uint32_t baseBits) {
    if (baseBits == 0)
        return 1;
    const uint32_t nBits = host::bitlen(c->q[limb]);
    return nBits / baseBits + (nBits % baseBits != 0);
}
extern "C" uint32_t fhe_crt_decompose_towers(const fhe_ctx* c, const uint32_t* li, uint32_t nl, uint32_t baseBits) {
    if (!c || nl < 1 || nl > (uint32_t)kMaxLimbs || baseBits > 31)  // (the reference's base is `1 << baseBits` in 32 bits)
        return 0;
    uint32_t towers = 0;
    for (uint32_t i = 0; i < nl; ++i) {
        const uint32_t l = li ? li[i] : i;
        if (l >= c->L)
            return 0;
        const uint32_t nW = crt_windows(c, l, baseBits);
        if ((uint64_t)nW * baseBits > 64)  // (the reference reads bits beyond the word there: undefined, left to the caller's host path)
            return 0;
        towers += nW;
    }
    return towers;
}
// every window of every limb of `batch` COEFFICIENT towers src [batch][nl][N] -> dst [towers][batch][nl][N], still COEFFICIENT (digit-major:
// crt_digits_kernel); the table of first towers travels in the kernel argument
static fhe_status crt_digits_run(fhe_ctx* c, const uint64_t* src, const uint32_t* li, uint32_t nl, uint32_t baseBits, uint32_t batch,
                                 uint64_t* dst, void* st, const char* who) {
    CrtDigitsArgs g;
    if (fhe_status s = make_sel(c, li, nl, &g.sel, who))
        return s;
    uint32_t t0 = 0, maxW = 0;
    for (uint32_t i = 0; i <= (uint32_t)kMaxLimbs; ++i) {
        g.first[i] = (uint16_t)t0;  // (at most 256 limbs x 60 windows)
        if (i < nl) {
            const uint32_t nW = crt_windows(c, li ? li[i] : i, baseBits);
            maxW = std::max(maxW, nW), t0 += nW;
        }
    }
    const uint32_t tilesPerRow = c->N >= (uint32_t)kTile ? (c->N >> kTileLog) : 1u;
    const uint64_t grid        = (uint64_t)tilesPerRow * batch * maxW * nl;
    ARG_CHECK(grid < ((uint64_t)1 << 31), std::string(who) + ": batch too large for one launch");
    g.out = dst, g.src = src, g.q = c->d_q, g.logN = c->logN, g.nLimbs = nl, g.batch = batch, g.baseBits = baseBits, g.maxW = maxW;
    FHE_LAUNCH(crt_digits_kernel, grid, st, g);
    LAUNCH_CHECK();
    return FHE_OK;
}
extern "C" fhe_status fhe_crt_decompose(fhe_ctx* c, const uint64_t* x, const uint32_t* li, uint32_t nl, uint32_t baseBits, uint64_t* out,
                                        void* st) {
    ARG_CHECK(c && x && out, "fhe_crt_decompose: null argument");
    const uint32_t towers = fhe_crt_decompose_towers(c, li, nl, baseBits);
    ARG_CHECK(towers >= 1, "fhe_crt_decompose: limb selection or digit size outside the device path (baseBits <= 31, every window inside the word)");
    RT_CHECK(rt::set_device(c->device));
    if (fhe_status s = crt_digits_run(c, x, li, nl, baseBits, 1, out, st, "fhe_crt_decompose"))
        return s;
    return fhe_ntt_fwd(c, out, li, nl, towers, st);
}

// ---- f3: sampled towers on the device (sampler_kernels.h) ----------------------------------------------------------------------
// the reference's table (DiscreteGaussianGeneratorImpl::Initialize, discretegaussiangenerator-impl.h:75-89), built once per sigma and
// shared by both generators
static fhe_status dgg_table(fhe_ctx* c, double sigma, const double** cdf, uint32_t* len, double* av, const char* who) {
    ARG_CHECK(sigma > 1.000000001 && sigma < 300.0, std::string(who) + ": the inversion sampler covers 1 < sigma < 300 (the reference's Peikert range)");
    std::lock_guard<std::mutex> lk(c->cacheMutex);
    auto it = c->dggTabs.find(sigma);
    if (it == c->dggTabs.end()) {
        const double M = 12.00610553538285;
        const int64_t fin = (int64_t)std::ceil(sigma * M);
        std::vector<double> vals((size_t)fin);
        const double variance = 2 * sigma * sigma;
        double cusum = 0.0;
        for (int64_t x = 1; x <= fin; ++x)
            vals[(size_t)(x - 1)] = (cusum += std::exp(-((double)(x * x) / variance)));
        const double a = 1.0 / (2 * cusum + 1.0);
        for (auto& v : vals)
            v *= a;
        const double* d = nullptr;
        if (fhe_status s = dev_copy(&c->owned, vals.data(), vals.size(), &d))
            return s;
        it = c->dggTabs.emplace(sigma, std::make_tuple(d, (uint32_t)fin, a)).first;
    }
    *cdf = std::get<0>(it->second), *len = std::get<1>(it->second), *av = std::get<2>(it->second);
    return FHE_OK;
}
static fhe_status sample_run(fhe_ctx* c, uint64_t* out, const uint32_t* li, uint32_t nl, uint32_t bt, uint32_t kind, double sigma,
                             uint64_t seed, uint32_t streamId, void* st, const char* who) {
    ARG_CHECK(c && out && bt >= 1, "fhe_sample: null argument or empty batch");
    SampleArgs a;
    if (fhe_status s = make_sel(c, li, nl, &a.sel, who))
        return s;
    RT_CHECK(rt::set_device(c->device));
    a.out = out, a.q = c->d_q, a.logN = c->logN, a.nLimbs = nl, a.batch = bt, a.seed = seed, a.stream = streamId, a.kind = kind;
    a.cdf = nullptr, a.cdfLen = 0, a.a = 0.0;
    if (kind == 1)
        if (fhe_status s = dgg_table(c, sigma, &a.cdf, &a.cdfLen, &a.a, who))
            return s;
    const uint64_t lanes = kind == 0 ? ((uint64_t)bt * nl) << c->logN : (uint64_t)bt << c->logN;
    FHE_LAUNCH(sample_kernel, (uint32_t)((lanes + kThreads - 1) / kThreads), st, a);
    LAUNCH_CHECK();
    return FHE_OK;
}
extern "C" fhe_status fhe_sample_uniform(fhe_ctx* c, uint64_t* out, const uint32_t* li, uint32_t nl, uint32_t bt, uint64_t seed,
                                         uint32_t streamId, void* st) {
    return sample_run(c, out, li, nl, bt, 0, 0.0, seed, streamId, st, "fhe_sample_uniform");
}
extern "C" fhe_status fhe_sample_gaussian(fhe_ctx* c, uint64_t* out, const uint32_t* li, uint32_t nl, uint32_t bt, double sigma,
                                          uint64_t seed, uint32_t streamId, void* st) {
    return sample_run(c, out, li, nl, bt, 1, sigma, seed, streamId, st, "fhe_sample_gaussian");
}
extern "C" fhe_status fhe_sample_ternary(fhe_ctx* c, uint64_t* out, const uint32_t* li, uint32_t nl, uint32_t bt, uint64_t seed,
                                         uint32_t streamId, void* st) {
    return sample_run(c, out, li, nl, bt, 2, 0.0, seed, streamId, st, "fhe_sample_ternary");
}

// ---- f3: the same samplers on blake2xb in counter mode (blake2_kernels.h) ------------------------------------------------------------
template <int KIND>
static fhe_status blake2_launch(const fhe_ctx* c, Blake2Args& a, const uint32_t* key, uint64_t counter0, void* st) {
    for (int i = 0; i < 16; ++i)
        a.key[i] = key[i];
    a.counter0 = counter0;
    // the longest walk that leaves at least two waves per SIMD (one H0 per counter is computed by one lane: a shorter walk costs
    // 2 / walk compressions more per leaf)
    const uint64_t minWaves = 8ull * (c->cus ? c->cus : 256);
    a.walk = kB2MaxWalk;
    while (a.walk > 1 && a.nBlocks / a.walk < minWaves)
        a.walk >>= 1;
    const uint64_t perWg = (uint64_t)(kB2Threads / 64) * a.walk;
    if (a.nBlocks)
        FHE_LAUNCH_BARRIER_N(blake2xb_kernel<KIND>, (a.nBlocks + perWg - 1) / perWg, kB2Threads, st, a);
    for (int i = 0; i < 16; ++i)  // (the argument copy on the host stack: the key leaves no trace here)
        ((volatile uint32_t*)a.key)[i] = 0;
    LAUNCH_CHECK();
    return FHE_OK;
}
extern "C" fhe_status fhe_blake2xb_stream(fhe_ctx* c, uint32_t* out, uint64_t nBlocks, const uint32_t key[16], uint64_t counter0, void* st) {
    ARG_CHECK(c && key && (out || nBlocks == 0), "fhe_blake2xb_stream: null argument");
    ARG_CHECK(((uintptr_t)out & 7u) == 0, "fhe_blake2xb_stream: out must be 8-byte aligned");
    ARG_CHECK(nBlocks <= ((uint64_t)UINT32_MAX - 1) * 4, "fhe_blake2xb_stream: nBlocks too large for one launch");
    RT_CHECK(rt::set_device(c->device));
    Blake2Args a{};
    a.out = (uint64_t*)out, a.nBlocks = nBlocks;
    return blake2_launch<3>(c, a, key, counter0, st);
}
static fhe_status blake2_sample(fhe_ctx* c, uint64_t* out, const uint32_t* li, uint32_t nl, uint32_t bt, int kind, double sigma,
                                const uint32_t* key, uint64_t counter0, void* st, const char* who) {
    ARG_CHECK(c && out && key && bt >= 1, std::string(who) + ": null argument or empty batch");
    Blake2Args a{};
    if (fhe_status s = make_sel(c, li, nl, &a.sel, who))
        return s;
    RT_CHECK(rt::set_device(c->device));
    a.out = out, a.q = c->d_q, a.mu128 = c->d_mu128, a.logN = c->logN, a.nLimbs = nl;
    if (kind == 1)
        if (fhe_status s = dgg_table(c, sigma, &a.cdf, &a.cdfLen, &a.a, who))
            return s;
    // uniform: 2 words of 64 bits per coefficient, 256 coefficients per 4 KiB block; Gaussian / ternary: 1 word, 512 per block
    a.total   = kind == 0 ? ((uint64_t)bt * nl) << c->logN : (uint64_t)bt << c->logN;
    a.nBlocks = kind == 0 ? (a.total + 255) / 256 : (a.total + 511) / 512;
    return kind == 0   ? blake2_launch<0>(c, a, key, counter0, st)
           : kind == 1 ? blake2_launch<1>(c, a, key, counter0, st)
                       : blake2_launch<2>(c, a, key, counter0, st);
}
extern "C" fhe_status fhe_sample_uniform_blake2(fhe_ctx* c, uint64_t* out, const uint32_t* li, uint32_t nl, uint32_t bt,
                                                const uint32_t key[16], uint64_t counter0, void* st) {
    return blake2_sample(c, out, li, nl, bt, 0, 0.0, key, counter0, st, "fhe_sample_uniform_blake2");
}
extern "C" fhe_status fhe_sample_gaussian_blake2(fhe_ctx* c, uint64_t* out, const uint32_t* li, uint32_t nl, uint32_t bt, double sigma,
                                                 const uint32_t key[16], uint64_t counter0, void* st) {
    return blake2_sample(c, out, li, nl, bt, 1, sigma, key, counter0, st, "fhe_sample_gaussian_blake2");
}
extern "C" fhe_status fhe_sample_ternary_blake2(fhe_ctx* c, uint64_t* out, const uint32_t* li, uint32_t nl, uint32_t bt,
                                                const uint32_t key[16], uint64_t counter0, void* st) {
    return blake2_sample(c, out, li, nl, bt, 2, 0.0, key, counter0, st, "fhe_sample_ternary_blake2");
}

// ------------------------------------------------------------------------------------------------
// basis conversion plans
// ------------------------------------------------------------------------------------------------
struct fhe_conv {
    fhe_ctx* ctx;
    uint32_t nSrc, nDst;
    std::vector<uint32_t> srcIdx, dstIdx;  // context limbs of the two bases (empty for internal plans)
    ConvTables tb;                   // = chunks[0]
    std::vector<ConvTables> chunks;  // source limbs [32k, 32k+32): one launch each (more than one only beyond 32 source limbs)
    const TwPair* allHatInv  = nullptr;  // chunked exact plans: every source limb's multiplier / modulus / 1.0/q_i
    const uint64_t* allSrcQ  = nullptr;
    const double* allQInv    = nullptr;
    std::vector<void*> owned;
};

static uint32_t conv_nsrc_pad(uint32_t nSrc) { return nSrc <= 8 ? 8u : nSrc <= 16 ? 16u : 32u; }
// device plan from explicit tables: hatInv[i] (multiplier of source residue i, mod src_i), hatMod[i*nDst + j] (weight of
// y_i in target j, mod dst_j), alphaMod[a*nDst + j] / qInv[i] for the exact variant (may be null: approximate only).
// Table rows are padded to the NSRC of the kernel instantiation conv_run picks, so that the kernel's table reads are
// unconditional (basis_kernels.h).
static fhe_status conv_from_tables(fhe_ctx* c, const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst,
                                   const uint64_t* hatInvIn, const uint64_t* hatModIn, const uint64_t* alphaIn,
                                   const double* qInvIn, fhe_conv** out) {
    const uint32_t nSrc = (uint32_t)src.size(), nDst = (uint32_t)dst.size();
    if (nSrc < 1 || nSrc > (uint32_t)kMaxLimbs || nDst < 1 || nDst > (uint32_t)kMaxLimbs)
        return fail(FHE_ERR_ARG, "basis conversion: 1..256 source and target limbs");
    fhe_conv* cv = new fhe_conv;
    cv->ctx      = c;
    cv->nSrc     = nSrc;
    cv->nDst     = nDst;
    // target-side tables, shared by all chunks
    std::vector<uint64_t> mu(2 * (size_t)nDst), alphaMod((size_t)(nSrc + 1) * nDst, 0), red(4 * (size_t)nDst);
    for (uint32_t j = 0; j < nDst; ++j) {
        host::mu128(dst[j], &mu[2 * j]);
        const uint64_t R = (uint64_t)((((unsigned __int128)1) << 64) % dst[j]);
        red[4 * j]       = dst[j];
        red[4 * j + 1]   = R;
        red[4 * j + 2]   = host::shoup(R, dst[j]);
        red[4 * j + 3]   = (uint64_t)((((unsigned __int128)1) << 64) / dst[j]);
    }
    if (alphaIn)
        for (size_t k = 0; k < alphaMod.size(); ++k)
            alphaMod[k] = alphaIn[k] % dst[k % nDst];
    ConvTables shared{};
    fhe_status s;
    if ((s = dev_copy(&cv->owned, dst.data(), dst.size(), &shared.dstQ)) ||
        (s = dev_copy(&cv->owned, mu.data(), mu.size(), &shared.dstMu)) ||
        (s = dev_copy(&cv->owned, red.data(), red.size(), &shared.dstRed)) ||
        (s = dev_copy(&cv->owned, alphaMod.data(), alphaMod.size(), &shared.alphaMod))) {
        fhe_conv_destroy(cv);
        return s;
    }
    // source-side tables per chunk of <= 32 source limbs (one chunk = one kernel launch; the usual case is one chunk)
    for (uint32_t c0 = 0; c0 < nSrc; c0 += 32u) {
        const uint32_t n   = std::min(32u, nSrc - c0);
        const uint32_t pad = conv_nsrc_pad(n);
        std::vector<TwPair> hatInv(32, TwPair{0, 0});
        std::vector<uint64_t> hatMod((size_t)pad * nDst, 0), srcPad(32, 1);
        std::vector<double> qInv(32, 0.0);
        for (uint32_t i = 0; i < n; ++i) {
            const uint64_t inv = hatInvIn[c0 + i] % src[c0 + i];
            hatInv[i]          = TwPair{inv, host::shoup(inv, src[c0 + i])};
            qInv[i]            = qInvIn ? qInvIn[c0 + i] : 1.0 / static_cast<double>(src[c0 + i]);
            srcPad[i]          = src[c0 + i];
            for (uint32_t j = 0; j < nDst; ++j)
                hatMod[(size_t)j * pad + i] = hatModIn[(size_t)(c0 + i) * nDst + j] % dst[j];
        }
        ConvTables tb = shared;
        if ((s = dev_copy(&cv->owned, hatInv.data(), hatInv.size(), &tb.hatInv)) ||
            (s = dev_copy(&cv->owned, hatMod.data(), hatMod.size(), &tb.hatMod)) ||
            (s = dev_copy(&cv->owned, srcPad.data(), srcPad.size(), &tb.srcQ)) ||
            (s = dev_copy(&cv->owned, qInv.data(), qInv.size(), &tb.srcQInv))) {
            fhe_conv_destroy(cv);
            return s;
        }
        cv->chunks.push_back(tb);
    }
    cv->tb = cv->chunks[0];
    if (nSrc > 32u) {  // the last chunk of the exact variant counts the overflow over all source limbs
        std::vector<TwPair> allInv(nSrc);
        std::vector<double> allQInv(nSrc);
        for (uint32_t i = 0; i < nSrc; ++i) {
            const uint64_t inv = hatInvIn[i] % src[i];
            allInv[i]          = TwPair{inv, host::shoup(inv, src[i])};
            allQInv[i]         = qInvIn ? qInvIn[i] : 1.0 / static_cast<double>(src[i]);
        }
        if ((s = dev_copy(&cv->owned, allInv.data(), allInv.size(), &cv->allHatInv)) ||
            (s = dev_copy(&cv->owned, src.data(), src.size(), &cv->allSrcQ)) ||
            (s = dev_copy(&cv->owned, allQInv.data(), allQInv.size(), &cv->allQInv))) {
            fhe_conv_destroy(cv);
            return s;
        }
    }
    *out = cv;
    return FHE_OK;
}
// tables for converting from moduli src[] to dst[]   (rns-cryptoparameters.cpp:214-246, 297-349); srcScale[i] (mod
// src_i) and dstScale[j] (mod dst_j), when given, are folded into the two constant sets: the plan then computes
// dstScale_j * SwitchBasis(srcScale_i * x_i) — exact as residues, used for the BGV t factors of ApproxModDown
static fhe_status conv_build(fhe_ctx* c, const std::vector<uint64_t>& src, const std::vector<uint64_t>& dst, fhe_conv** out,
                             const uint64_t* srcScale = nullptr, const uint64_t* dstScale = nullptr) {
    const uint32_t nSrc = (uint32_t)src.size(), nDst = (uint32_t)dst.size();
    std::vector<uint64_t> hatInv(nSrc), hatMod((size_t)nSrc * nDst), alphaMod((size_t)(nSrc + 1) * nDst);
    for (uint32_t i = 0; i < nSrc; ++i) {
        const uint64_t hat = host::prod_mod(src, (int)i, src[i]);
        hatInv[i]          = host::invmod(hat, src[i]);
        if (srcScale)
            hatInv[i] = host::mulmod(hatInv[i], srcScale[i] % src[i], src[i]);
        for (uint32_t j = 0; j < nDst; ++j) {
            uint64_t v = host::prod_mod(src, (int)i, dst[j]);
            if (dstScale)
                v = host::mulmod(v, dstScale[j] % dst[j], dst[j]);
            hatMod[(size_t)i * nDst + j] = v;
        }
    }
    for (uint32_t j = 0; j < nDst; ++j) {
        const uint64_t Qmod = host::prod_mod(src, -1, dst[j]);
        for (uint32_t a = 0; a <= nSrc; ++a)
            alphaMod[(size_t)a * nDst + j] = host::mulmod(a % dst[j], Qmod, dst[j]);
    }
    return conv_from_tables(c, src, dst, hatInv.data(), hatMod.data(), alphaMod.data(), nullptr, out);
}

extern "C" fhe_status fhe_conv_create(fhe_ctx* c, const uint32_t* srcIdx, uint32_t nSrc, const uint32_t* dstIdx,
                                      uint32_t nDst, fhe_conv** out) {
    ARG_CHECK(c && srcIdx && dstIdx && out, "fhe_conv_create: null argument");
    ARG_CHECK(nSrc >= 1 && nSrc <= (uint32_t)kMaxLimbs && nDst >= 1 && nDst <= (uint32_t)kMaxLimbs, "fhe_conv_create: bad basis size");
    std::vector<uint64_t> src(nSrc), dst(nDst);
    for (uint32_t i = 0; i < nSrc; ++i) {
        ARG_CHECK(srcIdx[i] < c->L, "fhe_conv_create: source limb exceeds context size");
        src[i] = c->q[srcIdx[i]];
    }
    for (uint32_t j = 0; j < nDst; ++j) {
        ARG_CHECK(dstIdx[j] < c->L, "fhe_conv_create: target limb exceeds context size");
        dst[j] = c->q[dstIdx[j]];
    }
    RT_CHECK(rt::set_device(c->device));
    if (fhe_status s = conv_build(c, src, dst, out))
        return s;
    (*out)->srcIdx.assign(srcIdx, srcIdx + nSrc);
    (*out)->dstIdx.assign(dstIdx, dstIdx + nDst);
    return FHE_OK;
}
// conversion plan with the CALLER's tables, laid out as the reference passes them to ApproxSwitchCRTBasis /
// SwitchCRTBasis (dcrtpoly-impl.h:888-932, 1008-1085): QHatInvModq[nSrc], QHatModp[nSrc][nDst]; for the exact variant
// alphaQModp[nSrc+1][nDst] and qInv[nSrc] (doubles), else null.  Needed where the tables are not the plain CRT ones,
// e.g. FastExpandCRTBasisPloverQ's mPlQHatInvModq / qInvModp (bfvrns-cryptoparameters.cpp).
extern "C" fhe_status fhe_conv_create_custom(fhe_ctx* c, const uint32_t* srcIdx, uint32_t nSrc, const uint32_t* dstIdx,
                                             uint32_t nDst, const uint64_t* hatInv, const uint64_t* hatMod,
                                             const uint64_t* alphaMod, const double* qInv, fhe_conv** out) {
    ARG_CHECK(c && srcIdx && dstIdx && hatInv && hatMod && out, "fhe_conv_create_custom: null argument");
    ARG_CHECK(nSrc >= 1 && nSrc <= (uint32_t)kMaxLimbs && nDst >= 1 && nDst <= (uint32_t)kMaxLimbs, "fhe_conv_create_custom: bad basis size");
    ARG_CHECK((alphaMod == nullptr) == (qInv == nullptr), "fhe_conv_create_custom: alphaMod and qInv go together");
    std::vector<uint64_t> src(nSrc), dst(nDst);
    for (uint32_t i = 0; i < nSrc; ++i) {
        ARG_CHECK(srcIdx[i] < c->L, "fhe_conv_create_custom: source limb exceeds context size");
        src[i] = c->q[srcIdx[i]];
    }
    for (uint32_t j = 0; j < nDst; ++j) {
        ARG_CHECK(dstIdx[j] < c->L, "fhe_conv_create_custom: target limb exceeds context size");
        dst[j] = c->q[dstIdx[j]];
    }
    RT_CHECK(rt::set_device(c->device));
    if (fhe_status s = conv_from_tables(c, src, dst, hatInv, hatMod, alphaMod, qInv, out))
        return s;
    (*out)->srcIdx.assign(srcIdx, srcIdx + nSrc);
    (*out)->dstIdx.assign(dstIdx, dstIdx + nDst);
    return FHE_OK;
}
extern "C" void fhe_conv_destroy(fhe_conv* cv) {
    if (!cv)
        return;
    for (void* p : cv->owned)
        rt::dfree(p);
    delete cv;
}

template <bool EXACT>
static fhe_status conv_run(fhe_conv* cv, const uint64_t* in, uint32_t inStride, uint32_t inFirst, uint64_t* out,
                           uint32_t outStride, uint32_t outFirst, uint32_t batch, void* st) {
    ARG_CHECK(cv && in && out, "fhe_switch_basis: null argument");
    ARG_CHECK(batch >= 1 && inFirst + cv->nSrc <= inStride && outFirst + cv->nDst <= outStride,
              "fhe_switch_basis: limb window exceeds tower stride");
    RT_CHECK(rt::set_device(cv->ctx->device));
    ConvArgs g{};
    g.in = in, g.out = out, g.tb = cv->tb;
    g.logN = cv->ctx->logN, g.batch = batch, g.nSrc = cv->nSrc, g.nDst = cv->nDst;
    g.inStride = inStride, g.inFirst = inFirst, g.outStride = outStride, g.outFirst = outFirst;
    const uint64_t coeffs = (uint64_t)batch << g.logN;
    const uint32_t grid   = (uint32_t)((coeffs + kThreads - 1) / kThreads);
    // column-sum form of the kernel: 2 = factors split at 30 bits (default), FHE_CONV_SUM8=1 = carry-counted 64-bit columns
    static const bool split30 = env_u32("FHE_CONV_SUM8", 2) != 1u;
    if (cv->chunks.size() > 1) {  // more than 32 source limbs: one launch per chunk, sums accumulated in `out`
        g.nSrcAll = cv->nSrc, g.inAll = in + ((size_t)inFirst << g.logN);
        g.allHatInv = cv->allHatInv, g.allSrcQ = cv->allSrcQ, g.allQInv = cv->allQInv;
        for (size_t k = 0; k < cv->chunks.size(); ++k) {
            g.tb      = cv->chunks[k];
            g.nSrc    = std::min(32u, cv->nSrc - 32u * (uint32_t)k);
            g.inFirst = inFirst + 32u * (uint32_t)k;
            g.acc     = k > 0;
            g.last    = k + 1 == cv->chunks.size();
            const uint32_t pad = conv_nsrc_pad(g.nSrc);
            if (pad == 8)
                FHE_LAUNCH((switch_basis_kernel<8, EXACT, 2, true>), grid, st, g);
            else if (pad == 16)
                FHE_LAUNCH((switch_basis_kernel<16, EXACT, 2, true>), grid, st, g);
            else
                FHE_LAUNCH((switch_basis_kernel<32, EXACT, 2, true>), grid, st, g);
            LAUNCH_CHECK();
        }
        return FHE_OK;
    }
    const uint32_t pad = conv_nsrc_pad(cv->nSrc);
    if (pad == 8 && split30)
        FHE_LAUNCH((switch_basis_kernel<8, EXACT, 2>), grid, st, g);
    else if (pad == 8)
        FHE_LAUNCH((switch_basis_kernel<8, EXACT, 1>), grid, st, g);
    else if (pad == 16 && split30)
        FHE_LAUNCH((switch_basis_kernel<16, EXACT, 2>), grid, st, g);
    else if (pad == 16)
        FHE_LAUNCH((switch_basis_kernel<16, EXACT, 1>), grid, st, g);
    else if (split30)
        FHE_LAUNCH((switch_basis_kernel<32, EXACT, 2>), grid, st, g);
    else
        FHE_LAUNCH((switch_basis_kernel<32, EXACT, 1>), grid, st, g);
    LAUNCH_CHECK();
    return FHE_OK;
}
extern "C" fhe_status fhe_approx_switch_basis(fhe_conv* cv, const uint64_t* in, uint32_t is, uint32_t ifst,
                                              uint64_t* out, uint32_t os, uint32_t ofst, uint32_t b, void* st) {
    return conv_run<false>(cv, in, is, ifst, out, os, ofst, b, st);
}
extern "C" fhe_status fhe_switch_basis_exact(fhe_conv* cv, const uint64_t* in, uint32_t is, uint32_t ifst,
                                             uint64_t* out, uint32_t os, uint32_t ofst, uint32_t b, void* st) {
    return conv_run<true>(cv, in, is, ifst, out, os, ofst, b, st);
}

// DCRTPolyImpl::ExpandCRTBasis / ExpandCRTBasisReverseOrder (dcrtpoly-impl.h:1088-1148): x over the plan's source basis Q
// (format inEval) -> out over Q u P in resultEval, P = SwitchCRTBasis of the coefficient form; reverse: P rows first.
extern "C" size_t fhe_expand_crt_basis_workspace_bytes(const fhe_conv* cv, uint32_t batch) {
    return cv ? (((size_t)batch * cv->nSrc) << cv->ctx->logN) * 8 : 0;
}
static fhe_status expand_run(fhe_conv* cv, const uint64_t* x, int inEval, uint64_t* out, int resultEval, int reverseOrder,
                             uint32_t batch, void* ws, size_t wsBytes, void* st, bool exact) {
    ARG_CHECK(cv && x && out && batch >= 1, "fhe_expand_crt_basis: bad argument");
    ARG_CHECK(!cv->srcIdx.empty(), "fhe_expand_crt_basis: the plan must come from fhe_conv_create[_custom]");
    fhe_ctx* c = cv->ctx;
    RT_CHECK(rt::set_device(c->device));
    const uint32_t nQ = cv->nSrc, nP = cv->nDst, tot = nQ + nP;
    const uint32_t qFirst = reverseOrder ? nP : 0, pFirst = reverseOrder ? 0 : nQ;
    const size_t rowB = (size_t)8 << c->logN;
    const uint64_t* coef = x;  // coefficient form of the Q part
    if (inEval) {              // :1096-1099
        ARG_CHECK(ws && wsBytes >= fhe_expand_crt_basis_workspace_bytes(cv, batch), "fhe_expand_crt_basis: workspace too small");
        if (fhe_status s = ntt_run(c, true, x, (uint64_t*)ws, cv->srcIdx.data(), nQ, batch, st))
            return s;
        coef = (const uint64_t*)ws;
    }
    if (fhe_status s = exact ? conv_run<true>(cv, coef, nQ, 0, out, tot, pFirst, batch, st)  // :1101-1102
                             : conv_run<false>(cv, coef, nQ, 0, out, tot, pFirst, batch, st))  // ApproxModUp :948
        return s;
    // Q rows of the result: the stored EVALUATION copy when it can be reused (:1104-1105), else the coefficient form
    const uint64_t* qsrc = (resultEval && inEval) ? x : coef;
    uint64_t* qdst       = out + ((size_t)qFirst << c->logN);
    RT_CHECK(rt::d2d_2d(qdst, tot * rowB, qsrc, nQ * rowB, nQ * rowB, batch, (rt::stream_t)st));
    if (resultEval) {  // :1112-1114: in place, the Q rows and the P rows of the tot-row towers
        NttOpts rows;
        rows.src.stride = rows.dst.stride = tot;
        rows.src.first = rows.dst.first = qFirst;
        if (!inEval)
            if (fhe_status s = ntt_run(c, false, out, out, cv->srcIdx.data(), nQ, batch, st, rows))
                return s;
        rows.src.first = rows.dst.first = pFirst;
        return ntt_run(c, false, out, out, cv->dstIdx.data(), nP, batch, st, rows);
    }
    return FHE_OK;
}
extern "C" fhe_status fhe_expand_crt_basis(fhe_conv* cv, const uint64_t* x, int inEval, uint64_t* out, int resultEval,
                                           int reverseOrder, uint32_t batch, void* ws, size_t wsBytes, void* st) {
    return expand_run(cv, x, inEval, out, resultEval, reverseOrder, batch, ws, wsBytes, st, true);
}
// DCRTPolyImpl::ApproxModUp (dcrtpoly-impl.h:935-963): x over the plan's source basis Q (format inEval) -> out over Q u P in
// EVALUATION: the EVALUATION copy of the Q limbs is kept when there is one (:943-946, 950-951), P = ApproxSwitchCRTBasis of the
// coefficient form (:948), every limb to EVALUATION (:958-960).  Workspace as fhe_expand_crt_basis (EVALUATION input only).
extern "C" fhe_status fhe_mod_up(fhe_conv* cv, const uint64_t* x, int inEval, uint64_t* out, uint32_t batch, void* ws,
                                 size_t wsBytes, void* st) {
    return expand_run(cv, x, inEval, out, 1, 0, batch, ws, wsBytes, st, false);
}
// DCRTPolyImpl::FastExpandCRTBasisPloverQ (dcrtpoly-impl.h:1151-1164), COEFFICIENT format: partPl =
// ApproxSwitchCRTBasis(x; toPl) with the caller's mPlQHatInvModq / qInvModp tables (fhe_conv_create_custom), partQl =
// SwitchCRTBasis(partPl; toQl); out = [Ql rows | Pl rows].
extern "C" fhe_status fhe_fast_expand_crt_basis_p_over_q(fhe_conv* toPl, fhe_conv* toQl, const uint64_t* x, uint64_t* out,
                                                         uint32_t batch, void* st) {
    ARG_CHECK(toPl && toQl && x && out && batch >= 1, "fhe_fast_expand_crt_basis_p_over_q: bad argument");
    ARG_CHECK(toQl->nSrc == toPl->nDst, "fhe_fast_expand_crt_basis_p_over_q: the second plan must start from the first plan's target basis");
    const uint32_t nQl = toQl->nDst, nPl = toPl->nDst, tot = nQl + nPl;
    if (fhe_status s = conv_run<false>(toPl, x, toPl->nSrc, 0, out, tot, nQl, batch, st))
        return s;
    return conv_run<true>(toQl, out, tot, nQl, out, tot, 0, batch, st);
}

// ------------------------------------------------------------------------------------------------
// HYBRID key switching
// ------------------------------------------------------------------------------------------------
struct fhe_ks_plan {
    fhe_ctx* ctx;
    uint32_t sizeQ, sizeP, numPartQ, alpha;
    // ModUp plans per (level sizeQl, digit): built lazily per level, cached
    struct Level {
        uint32_t sizeQl = 0, numParts = 0;
        std::vector<fhe_conv*> up;              // digit -> complement conversion
        std::vector<std::vector<uint32_t>> cidx;  // complement context-limb lists
        std::vector<uint32_t> partSize;
        fhe_conv* down = nullptr;               // P -> Q_l
        std::map<uint64_t, fhe_conv*> downT;    // BGV: P -> Q_l with t^-1 (mod p_j) and t (mod q_i) folded in, per t
        TwPair* d_PInv = nullptr;               // [sizeQl] Shoup pairs of [P^-1]_{q_i}
        TwPair* d_PModq = nullptr;              // [sizeQl] Shoup pairs of [P]_{q_i} (built on first use)
    };
    std::vector<Level*> levels;  // index sizeQl
    std::vector<void*> owned;
    std::map<std::vector<uint64_t>, void*> bsgsTables;  // device copies of the diagonal pointer tables, by content
    uint64_t* d_zeroRows = nullptr;                     // [sizeQ+sizeP][N] zeros: the "absent diagonal" of the BSGS transform
    std::mutex cacheMutex;                              // guards the lazily built levels / tables (callers may be OpenMP threads)
};
struct fhe_ks_key {
    fhe_ks_plan* plan;
    uint64_t *d_b = nullptr, *d_a = nullptr;
    size_t words = 0;
    bool owned = true;
};

extern "C" fhe_status fhe_ks_plan_create(fhe_ctx* c, uint32_t sizeQ, uint32_t sizeP, uint32_t numPartQ,
                                         fhe_ks_plan** out) {
    ARG_CHECK(c && out, "fhe_ks_plan_create: null argument");
    ARG_CHECK(sizeQ >= 1 && sizeP >= 1 && sizeQ + sizeP <= c->L, "fhe_ks_plan_create: context must hold Q then P limbs");
    ARG_CHECK(numPartQ >= 1, "numPartQ is zero");  // rns-cryptoparameters.cpp:82-83
    const uint32_t a = (sizeQ + numPartQ - 1) / numPartQ;
    // rns-cryptoparameters.cpp:87-91
    ARG_CHECK(sizeQ > a * (numPartQ - 1),
              "HYBRID key switching parameters: Can't appropriately distribute towers into digits");
    // (digits or P of more than 32 limbs — dnum = 1 or 2 on long chains — run as chunked conversions; more than 8 digits as
    // chunked inner products: the reference's loops have no such bounds, dcrtpoly-impl.h:895-915, keyswitch-hybrid.cpp:419-430)
    fhe_ks_plan* p = new fhe_ks_plan;
    p->ctx = c, p->sizeQ = sizeQ, p->sizeP = sizeP, p->numPartQ = numPartQ, p->alpha = a;
    p->levels.assign(sizeQ + 1, nullptr);
    *out = p;
    return FHE_OK;
}
static void ks_level_free(fhe_ks_plan::Level* lv) {
    if (!lv)
        return;
    for (auto* cv : lv->up)
        fhe_conv_destroy(cv);
    fhe_conv_destroy(lv->down);
    for (auto& kv : lv->downT)
        fhe_conv_destroy(kv.second);
    delete lv;
}
extern "C" void fhe_ks_plan_destroy(fhe_ks_plan* p) {
    if (!p)
        return;
    for (auto* lv : p->levels)
        ks_level_free(lv);
    for (void* q : p->owned)
        rt::dfree(q);
    for (auto& kv : p->bsgsTables)
        rt::dfree(kv.second);
    delete p;
}
extern "C" uint32_t fhe_ks_plan_alpha(const fhe_ks_plan* p) { return p ? p->alpha : 0; }
extern "C" uint32_t fhe_ks_plan_levels_built(fhe_ks_plan* p) {
    if (!p)
        return 0;
    std::lock_guard<std::mutex> lock(p->cacheMutex);
    uint32_t n = 0;
    for (auto* lv : p->levels)
        n += lv != nullptr;
    return n;
}

static fhe_status ks_level(fhe_ks_plan* p, uint32_t sizeQl, fhe_ks_plan::Level** out) {
    ARG_CHECK(sizeQl >= 1 && sizeQl <= p->sizeQ, "fhe_keyswitch: sizeQl out of range");
    std::lock_guard<std::mutex> lock(p->cacheMutex);
    if (p->levels[sizeQl]) {
        *out = p->levels[sizeQl];
        return FHE_OK;
    }
    fhe_ctx* c = p->ctx;
    auto* lv   = new fhe_ks_plan::Level;
    lv->sizeQl = sizeQl;
    // keyswitch-hybrid.cpp:329-333
    lv->numParts = std::min((sizeQl + p->alpha - 1) / p->alpha, p->numPartQ);
    for (uint32_t part = 0; part < lv->numParts; ++part) {
        const uint32_t start = p->alpha * part;
        const uint32_t sz    = (part == lv->numParts - 1) ? sizeQl - start : p->alpha;  // :341-352
        std::vector<uint64_t> src, dst;
        std::vector<uint32_t> cidx;
        for (uint32_t i = 0; i < sz; ++i)
            src.push_back(c->q[start + i]);
        // complementary basis (rns-cryptoparameters.cpp:253-283): Q_l limbs outside the digit, then P
        for (uint32_t i = 0; i < sizeQl; ++i)
            if (i < start || i >= start + sz)
                cidx.push_back(i);
        for (uint32_t j = 0; j < p->sizeP; ++j)
            cidx.push_back(p->sizeQ + j);
        for (uint32_t i : cidx)
            dst.push_back(c->q[i]);
        fhe_conv* cv = nullptr;
        if (fhe_status s = conv_build(c, src, dst, &cv)) {
            ks_level_free(lv);
            return s;
        }
        lv->up.push_back(cv);
        lv->cidx.push_back(cidx);
        lv->partSize.push_back(sz);
    }
    {
        std::vector<uint64_t> src, dst;
        for (uint32_t j = 0; j < p->sizeP; ++j)
            src.push_back(c->q[p->sizeQ + j]);
        for (uint32_t i = 0; i < sizeQl; ++i)
            dst.push_back(c->q[i]);
        if (fhe_status s = conv_build(c, src, dst, &lv->down)) {
            ks_level_free(lv);
            return s;
        }
        // [P^-1]_{q_i}  (rns-cryptoparameters.cpp:205-212)
        std::vector<TwPair> pinv(sizeQl);
        for (uint32_t i = 0; i < sizeQl; ++i) {
            const uint64_t v = host::invmod(host::prod_mod(src, -1, c->q[i]), c->q[i]);
            pinv[i]          = TwPair{v, host::shoup(v, c->q[i])};
        }
        if (dev_copy(&p->owned, pinv.data(), pinv.size(), &lv->d_PInv)) {
            ks_level_free(lv);
            return fail(FHE_ERR_DEVICE, "fhe_keyswitch: building the level tables: " + g_lastError);
        }
    }
    p->levels[sizeQl] = lv;
    *out              = lv;
    return FHE_OK;
}

extern "C" fhe_status fhe_ks_key_alloc(fhe_ks_plan* p, fhe_ks_key** out) {
    ARG_CHECK(p && out, "fhe_ks_key_alloc: null argument");
    RT_CHECK(rt::set_device(p->ctx->device));
    fhe_ks_key* k = new fhe_ks_key;
    k->plan       = p;
    k->words      = (size_t)p->numPartQ * (p->sizeQ + p->sizeP) << p->ctx->logN;
    if (rt::dmalloc((void**)&k->d_b, k->words * 8) || rt::dmalloc((void**)&k->d_a, k->words * 8)) {
        fhe_ks_key_destroy(k);
        return fail(FHE_ERR_ALLOC, "fhe_ks_key_alloc: device allocation failed");
    }
    *out = k;
    return FHE_OK;
}
extern "C" fhe_status fhe_ks_key_upload(fhe_ks_plan* p, const uint64_t* keyB, const uint64_t* keyA, fhe_ks_key** out) {
    ARG_CHECK(keyB && keyA, "fhe_ks_key_upload: null key");
    fhe_ks_key* k = nullptr;
    if (fhe_status s = fhe_ks_key_alloc(p, &k))
        return s;
    RT_CHECK(rt::h2d(k->d_b, keyB, k->words * 8, nullptr));
    RT_CHECK(rt::h2d(k->d_a, keyA, k->words * 8, nullptr));
    RT_CHECK(rt::sync(nullptr));
    *out = k;
    return FHE_OK;
}
extern "C" fhe_status fhe_ks_key_wrap(fhe_ks_plan* p, uint64_t* devB, uint64_t* devA, fhe_ks_key** out) {
    ARG_CHECK(p && devB && devA && out, "fhe_ks_key_wrap: null argument");
    fhe_ks_key* k = new fhe_ks_key;
    k->plan       = p;
    k->words      = (size_t)p->numPartQ * (p->sizeQ + p->sizeP) << p->ctx->logN;
    k->d_b        = devB;
    k->d_a        = devA;
    k->owned      = false;
    *out          = k;
    return FHE_OK;
}
extern "C" void fhe_ks_key_destroy(fhe_ks_key* k) {
    if (!k)
        return;
    if (k->owned && k->d_b)
        rt::dfree(k->d_b);
    if (k->owned && k->d_a)
        rt::dfree(k->d_a);
    delete k;
}
extern "C" uint64_t* fhe_ks_key_devptr(fhe_ks_key* k, int which) { return k ? (which ? k->d_a : k->d_b) : nullptr; }
extern "C" size_t fhe_ks_key_words(const fhe_ks_key* k) { return k ? k->words : 0; }

// workspace layout (words), all sized for `batch` towers:
//   coef   [batch][sizeQl][N]              INTT of the input
//   dig_j  [batch][nc_j][N]  j < numParts  ModUp complements
//   e0,e1  [batch][sizeQl+sizeP][N]        inner products
//   md     [2*batch][sizeQl][N]            ModDown conversion output  (also used as [2*batch][sizeP][N] scratch: pcoef)
//   pcoef  [2*batch][sizeP][N]
//   d2     [batch][sizeQl][N], k0,k1 [batch][sizeQl][N]   (eval_mult only)
struct KsLayout {
    size_t coef = 0, e0 = 0, e1 = 0, md = 0, pcoef = 0, d2 = 0, k0 = 0, k1 = 0, total = 0;
    std::vector<size_t> dig;
};
static KsLayout ks_layout(const fhe_ks_plan* p, uint32_t sizeQl, uint32_t batch) {
    KsLayout w;
    const size_t N = (size_t)1 << p->ctx->logN;
    const uint32_t numParts = std::min((sizeQl + p->alpha - 1) / p->alpha, p->numPartQ);
    w.dig.assign(numParts, 0);
    size_t off = 0;
    w.coef = off, off += (size_t)batch * sizeQl * N;
    for (uint32_t j = 0; j < numParts; ++j) {
        const uint32_t start = p->alpha * j;
        const uint32_t sz    = (j == numParts - 1) ? sizeQl - start : p->alpha;
        w.dig[j] = off, off += (size_t)batch * (sizeQl - sz + p->sizeP) * N;
    }
    w.e0 = off, off += (size_t)batch * (sizeQl + p->sizeP) * N;
    w.e1 = off, off += (size_t)batch * (sizeQl + p->sizeP) * N;
    w.md = off, off += (size_t)2 * batch * sizeQl * N;
    w.pcoef = off, off += (size_t)2 * batch * p->sizeP * N;
    w.d2 = off, off += (size_t)batch * sizeQl * N;
    w.k0 = off, off += (size_t)batch * sizeQl * N;
    w.k1 = off, off += (size_t)batch * sizeQl * N;
    w.total = off;
    return w;
}
extern "C" size_t fhe_ks_workspace_bytes(const fhe_ks_plan* p, uint32_t sizeQl, uint32_t batch) {
    if (!p || sizeQl < 1 || sizeQl > p->sizeQ || batch < 1)
        return 0;
    return ks_layout(p, sizeQl, batch).total * 8;
}

// ApproxModDown (dcrtpoly-impl.h:966-1005) in two parts so that the two accumulators of a key switch share the
// INTT / conversion / NTT launches:
//   mod_down_core: x[nTow][sizeQl+sizeP][N] -> md[nTow][sizeQl][N] = NTT(ApproxSwitchCRTBasis(INTT(P part)))
//   mod_down_tail: out_i = (x_i - md_i) * [P^-1]_{q_i}     (or out_i += ... when `accumulate`)
static fhe_status mod_down_core(fhe_ks_plan* p, fhe_ks_plan::Level* lv, const uint64_t* x, uint32_t nTow, uint64_t* pcoef,
                                uint64_t* md, void* st, fhe_conv* down = nullptr, const NttEpilogue* epi = nullptr) {
    fhe_ctx* c            = p->ctx;
    const uint32_t sizeQl = lv->sizeQl, sizeP = p->sizeP, sizeQlP = sizeQl + sizeP;
    std::vector<uint32_t> pIdx(sizeP);
    for (uint32_t j = 0; j < sizeP; ++j)
        pIdx[j] = p->sizeQ + j;
    // P part to COEFFICIENT (:978-985): INTT of rows [sizeQl, sizeQl+sizeP) of every tower, written densely
    NttOpts pRows;
    pRows.src.stride = sizeQlP, pRows.src.first = sizeQl;
    if (fhe_status s = ntt_run(c, true, x, pcoef, pIdx.data(), sizeP, nTow, st, pRows))
        return s;
    // P -> Q_l (:987-988)
    if (fhe_status s = fhe_approx_switch_basis(down ? down : lv->down, pcoef, sizeP, 0, md, sizeQl, 0, nTow, st))
        return s;
    // back to EVALUATION (:1001); with an epilogue the last pass also applies (:1002) and stores the final result
    NttOpts fused;
    fused.epi = epi;
    return ntt_run(c, false, md, md, nullptr, sizeQl, nTow, st, fused);
}
// C: the per-limb constant of (:1002) as device Shoup pairs [sizeQl]; null: the level's own [P^-1]_{q_i}
static fhe_status mod_down_tail(fhe_ks_plan* p, fhe_ks_plan::Level* lv, const uint64_t* x, const uint64_t* md, uint32_t nTow,
                                uint64_t* out, bool accumulate, void* st, const TwPair* C = nullptr) {
    const uint32_t sizeQl = lv->sizeQl, sizeQlP = sizeQl + p->sizeP;
    if (!C)
        C = lv->d_PInv;
    // (:1002); x towers are sizeQlP rows apart
    if (accumulate)
        return elem_run<OP_SUB_MUL_CONST_ACC>(p->ctx, out, x, md, C, nullptr, sizeQl, nTow, st, "fhe_approx_mod_down", sizeQlP, 0);
    return elem_run<OP_SUB_MUL_CONST>(p->ctx, out, x, md, C, nullptr, sizeQl, nTow, st, "fhe_approx_mod_down", sizeQlP, 0);
}
static fhe_status mod_down_run(fhe_ks_plan* p, fhe_ks_plan::Level* lv, const uint64_t* x, uint32_t nTow, uint64_t* out,
                               uint64_t* pcoef, uint64_t* md, void* st) {
    if (fhe_status s = mod_down_core(p, lv, x, nTow, pcoef, md, st))
        return s;
    return mod_down_tail(p, lv, x, md, nTow, out, false, st);
}

// EvalKeySwitchPrecomputeCore (keyswitch-hybrid.cpp:314-379): digit decomposition + ModUp of every digit into the
// workspace's digit buffers (the digit's own limbs are NOT copied: the inner product reads them from `cin`)
// ... in its two parts: the digits cut from a COEFFICIENT tower `coef` [batch][sizeQl][N] (the workspace's own copy, or a caller's tower:
// it is only read), and in front of it the inverse transform that fills the workspace's copy
static fhe_status ks_precompute_from_coef(fhe_ks_plan* p, fhe_ks_plan::Level* lv, const uint64_t* coef, uint32_t batch, uint64_t* ws,
                                          const KsLayout& w, void* st) {
    fhe_ctx* c            = p->ctx;
    const uint32_t sizeQl = lv->sizeQl;
    NttOpts lazy;
    lazy.canonOut = false;
    for (uint32_t j = 0; j < lv->numParts; ++j) {
        const uint32_t nc = (uint32_t)lv->cidx[j].size();
        uint64_t* dj      = ws + w.dig[j];
        if (fhe_status s = fhe_approx_switch_basis(lv->up[j], coef, sizeQl, p->alpha * j, dj, nc, 0, batch, st))
            return s;
        // the digits are only read by the inner product, whose 128-bit accumulation takes any 64-bit operand: the
        // transform's outputs stay in the lazy range (< 16q), the 4-level canonicalisation is skipped
        if (fhe_status s = ntt_run(c, false, dj, dj, lv->cidx[j].data(), nc, batch, st, lazy))
            return s;
    }
    return FHE_OK;
}
static fhe_status ks_precompute_run(fhe_ks_plan* p, fhe_ks_plan::Level* lv, const uint64_t* cin, uint32_t batch,
                                    uint64_t* ws, const KsLayout& w, void* st) {
    if (fhe_status s = fhe_ntt_inv_oop(p->ctx, cin, ws + w.coef, nullptr, lv->sizeQl, batch, st))
        return s;
    return ks_precompute_from_coef(p, lv, ws + w.coef, batch, ws, w, st);
}
// EvalFastKeySwitchCore (keyswitch-hybrid.cpp:381-435) on digits already in the workspace.
// accumulate: out0/out1 += result (EvalMult's `cv[0] += ab[0]; cv[1] += ab[1]`, base-leveledshe.cpp:210-211)
// EvalFastKeySwitchCoreExt (keyswitch-hybrid.cpp:402-435) of ONE digit decomposition with nKeys keys, at most 8 digits: one launch per 16
// keys, every digit residue read once per launch; first != null: e0_t's Q_l rows += first * dP[i] (EvalFastRotationExt's addFirst,
// ckksrns-leveledshe.cpp:561-570) in the same store
static fhe_status ks_inner_multi_launch(fhe_ks_plan* p, fhe_ks_plan::Level* lv, const fhe_ks_key* const* keys, uint32_t nKeys,
                                        const uint64_t* cin, uint32_t batch, uint64_t* const* e0, uint64_t* const* e1,
                                        const uint64_t* first, const TwPair* dP, uint64_t* ws, const KsLayout& w, void* st,
                                        uint32_t towOff = 0) {
    fhe_ctx* c            = p->ctx;
    const uint32_t sizeQl = lv->sizeQl, sizeP = p->sizeP, sizeQlP = sizeQl + sizeP;
    const uint32_t tilesPerRow = c->N >= (uint32_t)kTile ? (c->N >> kTileLog) : 1u;
    for (uint32_t t0 = 0; t0 < nKeys; t0 += (uint32_t)kMaxMultiKeys) {
        KsInnerMultiArgs g;
        const uint32_t nt = std::min<uint32_t>(kMaxMultiKeys, nKeys - t0);
        for (uint32_t j = 0; j < (uint32_t)kMaxDigits; ++j) {
            g.nc[j]     = j < lv->numParts ? (uint32_t)lv->cidx[j].size() : 0u;
            g.digits[j] = j < lv->numParts ? ws + w.dig[j] + (((size_t)towOff * g.nc[j]) << c->logN) : nullptr;
        }
        for (uint32_t t = 0; t < (uint32_t)kMaxMultiKeys; ++t) {
            const uint32_t tt = t < nt ? t0 + t : t0;
            g.keyB[t] = keys[tt]->d_b, g.keyA[t] = keys[tt]->d_a, g.out0[t] = e0[tt], g.out1[t] = e1[tt];
        }
        g.c = cin + (((size_t)towOff * sizeQl) << c->logN), g.first = first, g.firstC = dP;
        g.lc = c->d_lc, g.mu128 = c->d_mu128, g.red = c->d_red;
        g.logN = c->logN, g.batch = batch, g.sizeQl = sizeQl, g.sizeQ = p->sizeQ, g.sizeP = sizeP;
        g.numDigits = lv->numParts, g.alpha = p->alpha, g.nKeys = nt;
        const uint64_t grid = (((uint64_t)tilesPerRow * sizeQlP + 7) / 8) * 8 * batch;
        // three digits (the usual dnum): two adjacent coefficients per lane, 16-byte accesses — round 6: 1341 -> 1090 us per launch in the
        // lockstep bootstrap, EvalMult composite +2-3 % (profiles/r06_sweeps.md 9).  FHE_KSM selects the other forms for A/B runs:
        //   0 one coefficient per lane, next key prefetched (rounds 4-5) | 1 two per lane, prefetched (default) | 2 two per lane, no prefetch |
        //   3 one per lane, no prefetch
        static const uint32_t ksm = env_u32("FHE_KSM", 1);
        uintptr_t bits = (uintptr_t)g.c | (uintptr_t)g.first;  // (16-byte accesses need 16-byte aligned towers: any device allocation is)
        for (uint32_t j = 0; j < lv->numParts && j < (uint32_t)kMaxDigits; ++j)
            bits |= (uintptr_t)g.digits[j];
        for (uint32_t t = 0; t < nt; ++t)
            bits |= (uintptr_t)g.keyB[t] | (uintptr_t)g.keyA[t] | (uintptr_t)g.out0[t] | (uintptr_t)g.out1[t];
        const bool wide = (bits & 15u) == 0 && c->N >= 2;
        if (lv->numParts <= 3 && ksm == 1 && wide)
            FHE_LAUNCH((ks_inner_multi_kernel<3, 2, true>), grid, st, g);
        else if (lv->numParts <= 3 && ksm == 2 && wide)
            FHE_LAUNCH((ks_inner_multi_kernel<3, 2, false>), grid, st, g);
        else if (lv->numParts <= 3 && ksm == 3)
            FHE_LAUNCH((ks_inner_multi_kernel<3, 1, false>), grid, st, g);
        else if (lv->numParts <= 3)
            FHE_LAUNCH((ks_inner_multi_kernel<3>), grid, st, g);
        else if (lv->numParts <= 4)
            FHE_LAUNCH((ks_inner_multi_kernel<4>), grid, st, g);
        else
            FHE_LAUNCH((ks_inner_multi_kernel<8>), grid, st, g);
        LAUNCH_CHECK();
    }
    return FHE_OK;
}
// EvalFastKeySwitchCoreExt (keyswitch-hybrid.cpp:402-435): inner product of the digits in the workspace with the key, both
// halves, result [batch][sizeQl+sizeP][N] in the extended basis
// towOff: the `batch` towers start at tower towOff of `cin` and of every digit buffer (a slice of a larger precompute)
static fhe_status ks_inner_run(fhe_ks_plan* p, fhe_ks_plan::Level* lv, const fhe_ks_key* key, const uint64_t* cin,
                               uint32_t batch, uint64_t* e0, uint64_t* e1, uint64_t* ws, const KsLayout& w, void* st,
                               uint32_t towOff = 0) {
    fhe_ctx* c            = p->ctx;
    const uint32_t sizeQl = lv->sizeQl, sizeP = p->sizeP, sizeQlP = sizeQl + sizeP;
    const uint32_t tilesPerRow = c->N >= (uint32_t)kTile ? (c->N >> kTileLog) : 1u;
    // at most 8 digits: the kernel that keeps the digits' residues in registers and issues every load of a coefficient up front (EvalMult
    // composite 8440 -> 8611 op/s against the chunked kernel below, session i); more digits: chunks of 8 whose exact sums add up
    if (lv->numParts <= (uint32_t)kMaxDigits)
        return ks_inner_multi_launch(p, lv, &key, 1, cin, batch, &e0, &e1, nullptr, nullptr, ws, w, st, towOff);
    for (uint32_t j0 = 0; j0 < lv->numParts; j0 += (uint32_t)kMaxDigits) {  // (one launch up to 8 digits)
        KsInnerArgs g;
        const uint32_t nd = std::min<uint32_t>(kMaxDigits, lv->numParts - j0);
        for (uint32_t j = 0; j < (uint32_t)kMaxDigits; ++j) {
            g.nc[j]     = j < nd ? (uint32_t)lv->cidx[j0 + j].size() : 0u;
            g.digits[j] = j < nd ? ws + w.dig[j0 + j] + (((size_t)towOff * g.nc[j]) << c->logN) : nullptr;
        }
        g.c = cin + (((size_t)towOff * sizeQl) << c->logN), g.keyB = key->d_b, g.keyA = key->d_a;
        g.out0 = e0, g.out1 = e1;
        g.lc = c->d_lc, g.mu128 = c->d_mu128, g.red = c->d_red;
        g.logN = c->logN, g.batch = batch, g.sizeQl = sizeQl, g.sizeQ = p->sizeQ, g.sizeP = sizeP;
        g.numDigits = nd, g.alpha = p->alpha, g.j0 = j0, g.acc = j0 > 0;
        FHE_LAUNCH(ks_inner_product_kernel, (((uint64_t)tilesPerRow * sizeQlP + 7) / 8) * 8 * batch, st, g);
        LAUNCH_CHECK();
    }
    return FHE_OK;
}
// The same for SEVERAL keys on one digit decomposition (the baby-step rotations of a BSGS transform), optionally with addFirst.  More
// than 8 digits: key by key through ks_inner_run + the element-wise pass.
static fhe_status ks_inner_multi_run(fhe_ks_plan* p, fhe_ks_plan::Level* lv, const fhe_ks_key* const* keys, uint32_t nKeys,
                                     const uint64_t* cin, uint32_t batch, uint64_t* const* e0, uint64_t* const* e1,
                                     const uint64_t* first, const TwPair* dP, uint64_t* ws, const KsLayout& w, void* st) {
    if (lv->numParts <= (uint32_t)kMaxDigits)
        return ks_inner_multi_launch(p, lv, keys, nKeys, cin, batch, e0, e1, first, dP, ws, w, st);
    const uint32_t sizeQl = lv->sizeQl, sizeQlP = sizeQl + p->sizeP;
    for (uint32_t t = 0; t < nKeys; ++t) {
        if (fhe_status s = ks_inner_run(p, lv, keys[t], cin, batch, e0[t], e1[t], ws, w, st))
            return s;
        if (first)
            if (fhe_status s = elem_run<OP_MUL_CONST_ADD>(p->ctx, e0[t], first, e0[t], dP, nullptr, sizeQl, batch, st,
                                                          "fhe_eval_fast_rotation_ext", 0, 0, sizeQlP, 0, sizeQlP, 0))
                return s;
    }
    return FHE_OK;
}
// the HYBRID inner product (keyswitch-hybrid.cpp:419-430) over towers in separate allocations: see inner_rows_kernel
extern "C" fhe_status fhe_inner_product(fhe_ctx* c, uint32_t nTerms, const uint64_t* const* x, const uint64_t* const* k0,
                                        const uint64_t* const* k1, const uint32_t* keyRow, const uint32_t* limbIdx,
                                        uint32_t rows, uint32_t batch, uint64_t* out0, uint64_t* out1, void* st) {
    ARG_CHECK(c && x && k0 && out0, "fhe_inner_product: null argument");
    ARG_CHECK((k1 != nullptr) == (out1 != nullptr), "fhe_inner_product: the second key and the second output go together");
    ARG_CHECK(batch >= 1, "fhe_inner_product: batch must be >= 1");
    ARG_CHECK(nTerms >= 1, "fhe_inner_product: no terms");
    InnerRowsArgs g;
    if (fhe_status s = make_sel(c, limbIdx, rows, &g.sel, "fhe_inner_product"))
        return s;
    for (uint32_t i = 0; i < (uint32_t)kMaxLimbs; ++i) {
        const uint32_t kr = i < rows ? (keyRow ? keyRow[i] : i) : 0u;
        ARG_CHECK(kr < 256u, "fhe_inner_product: key row out of range");
        g.keyRow[i] = (uint8_t)kr;
    }
    for (uint32_t j = 0; j < nTerms; ++j)
        ARG_CHECK(x[j] && k0[j] && (!k1 || k1[j]), "fhe_inner_product: null term");
    RT_CHECK(rt::set_device(c->device));
    g.out0 = out0, g.out1 = out1, g.lc = c->d_lc, g.mu128 = c->d_mu128;
    g.logN = c->logN, g.batch = batch, g.rows = rows;
    const uint32_t tilesPerRow = c->N >= (uint32_t)kTile ? (c->N >> kTileLog) : 1u;
    for (uint32_t t0 = 0; t0 < nTerms; t0 += (uint32_t)kMaxDigits) {  // (one launch up to 8 terms; exact sums, so chunks add up)
        const uint32_t nt = std::min<uint32_t>(kMaxDigits, nTerms - t0);
        for (uint32_t j = 0; j < (uint32_t)kMaxDigits; ++j) {
            g.x[j]  = j < nt ? x[t0 + j] : nullptr;
            g.k0[j] = j < nt ? k0[t0 + j] : nullptr;
            g.k1[j] = (j < nt && k1) ? k1[t0 + j] : nullptr;
        }
        g.nTerms = nt, g.acc = t0 > 0;
        FHE_LAUNCH(inner_rows_kernel, (uint64_t)tilesPerRow * rows * batch, st, g);
        LAUNCH_CHECK();
    }
    return FHE_OK;
}
// The level's conversion P -> Q_l of ApproxModDown: t == 0 the plain one (CKKS, BFV), t >= 2 the BGV one with t^-1 mod p_j and t mod q_i
// folded into its two constant sets (fhe_approx_mod_down_bgv below), built on first use and kept per (level, t).  The reference passes
// t = GetPlaintextModulus() whenever GetNoiseScale() != 1 (keyswitch-hybrid.cpp:263, 299, 386).
static fhe_status ks_down_conv(fhe_ks_plan* p, fhe_ks_plan::Level* lv, uint64_t t, const char* who, fhe_conv** out) {
    if (t == 0) {
        *out = lv->down;
        return FHE_OK;
    }
    fhe_ctx* c = p->ctx;
    ARG_CHECK(t >= 2, std::string(who) + ": t must be at least 2");
    std::lock_guard<std::mutex> lock(p->cacheMutex);
    auto it = lv->downT.find(t);
    if (it == lv->downT.end()) {
        const uint32_t sizeQl = lv->sizeQl;
        std::vector<uint64_t> src(p->sizeP), dst(sizeQl), sScale(p->sizeP), dScale(sizeQl);
        for (uint32_t j = 0; j < p->sizeP; ++j) {
            src[j] = c->q[p->sizeQ + j];
            ARG_CHECK(t % src[j] != 0, std::string(who) + ": t must be invertible modulo every p_j");
            sScale[j] = host::invmod(t % src[j], src[j]);  // tInvModp (bgvrns-cryptoparameters.cpp:77-81)
        }
        for (uint32_t i = 0; i < sizeQl; ++i) {
            dst[i]    = c->q[i];
            dScale[i] = t % dst[i];
        }
        fhe_conv* cv = nullptr;
        if (fhe_status s = conv_build(c, src, dst, &cv, sScale.data(), dScale.data()))
            return s;
        it = lv->downT.emplace(t, cv).first;
    }
    *out = it->second;
    return FHE_OK;
}
// t: 0 = the CKKS / BFV form; >= 2 = the BGV form, the ModDown with the level's downT conversion (ks_down_conv) under the same fused epilogue
static fhe_status ks_fast_run(fhe_ks_plan* p, fhe_ks_plan::Level* lv, const fhe_ks_key* key, const uint64_t* cin,
                              uint32_t batch, uint64_t* out0, uint64_t* out1, uint64_t* ws, const KsLayout& w, void* st,
                              bool accumulate, uint64_t t = 0, const TwPair* C = nullptr) {
    fhe_ctx* c            = p->ctx;
    const uint32_t sizeQl = lv->sizeQl;
    fhe_conv* down        = nullptr;  // (null: the plan's own conversion, mod_down_core)
    if (!C)
        C = lv->d_PInv;  // (BFV below the top level: [P^-1]_{q_i} * QlHatModq(l)[i], fhe_bfv_hybrid_create)
    if (t)
        if (fhe_status s = ks_down_conv(p, lv, t, "key switch", &down))
            return s;
    if (fhe_status s = ks_inner_run(p, lv, key, cin, batch, ws + w.e0, ws + w.e1, ws, w, st))
        return s;
    // 2 x ApproxModDown (:381-400): e0 and e1 are adjacent in the workspace (w.e1 == w.e0 + batch*sizeQlP*N), so the
    // INTT / conversion / NTT run once over 2*batch towers; only the element-wise tails are per accumulator
    if (ntt_epilogue_supported(c)) {
        // (x_i - switched_i) * [P^-1]_{q_i} (+= into out for EvalMult) applied by the last NTT pass itself: the switched
        // tower is never written to HBM in EVALUATION form and the two tail kernels disappear
        NttEpilogue epi;
        epi.mode = accumulate ? 2u : 1u, epi.split = batch, epi.aStride = sizeQl + p->sizeP, epi.aFirst = 0;
        epi.A = ws + w.e0, epi.C = C, epi.out0 = out0, epi.out1 = out1;
        return mod_down_core(p, lv, ws + w.e0, 2 * batch, ws + w.pcoef, ws + w.md, st, down, &epi);
    }
    if (fhe_status s = mod_down_core(p, lv, ws + w.e0, 2 * batch, ws + w.pcoef, ws + w.md, st, down))
        return s;
    if (fhe_status s = mod_down_tail(p, lv, ws + w.e0, ws + w.md, batch, out0, accumulate, st, C))
        return s;
    return mod_down_tail(p, lv, ws + w.e1, ws + w.md + ((size_t)batch * sizeQl << c->logN), batch, out1, accumulate, st, C);
}
static fhe_status keyswitch_run(fhe_ks_plan* p, const fhe_ks_key* key, const uint64_t* cin, uint32_t sizeQl,
                                uint32_t batch, uint64_t* out0, uint64_t* out1, uint64_t* ws, const KsLayout& w,
                                void* st, bool accumulate = false, uint64_t t = 0) {
    fhe_ks_plan::Level* lv = nullptr;
    if (fhe_status s = ks_level(p, sizeQl, &lv))
        return s;
    if (fhe_status s = ks_precompute_run(p, lv, cin, batch, ws, w, st))
        return s;
    return ks_fast_run(p, lv, key, cin, batch, out0, out1, ws, w, st, accumulate, t);
}

extern "C" fhe_status fhe_keyswitch_hybrid(fhe_ks_plan* p, const fhe_ks_key* key, const uint64_t* cin, uint32_t sizeQl,
                                           uint32_t batch, uint64_t* out0, uint64_t* out1, void* ws, size_t wsBytes,
                                           void* st) {
    ARG_CHECK(p && key && cin && out0 && out1 && ws, "fhe_keyswitch_hybrid: null argument");
    ARG_CHECK(key->plan == p, "fhe_keyswitch_hybrid: key belongs to another plan");
    ARG_CHECK(sizeQl >= 1 && sizeQl <= p->sizeQ && batch >= 1, "fhe_keyswitch_hybrid: bad level or batch");
    const KsLayout w = ks_layout(p, sizeQl, batch);
    ARG_CHECK(wsBytes >= w.total * 8, "fhe_keyswitch_hybrid: workspace too small");
    RT_CHECK(rt::set_device(p->ctx->device));
    return keyswitch_run(p, key, cin, sizeQl, batch, out0, out1, (uint64_t*)ws, w, st);
}

// the same with `acc0 += ks0(c); acc1 += ks1(c)`: the tail of LeveledSHEBase::EvalMult(ct, ct, key) (base-leveledshe.cpp:207-211:
// KeySwitchCore on the third element, `cv[0] += ab[0]; cv[1] += ab[1]`), the additions fused into the ModDown epilogue
extern "C" fhe_status fhe_keyswitch_hybrid_acc(fhe_ks_plan* p, const fhe_ks_key* key, const uint64_t* cin, uint32_t sizeQl,
                                               uint32_t batch, uint64_t* acc0, uint64_t* acc1, void* ws, size_t wsBytes, void* st) {
    ARG_CHECK(p && key && cin && acc0 && acc1 && ws, "fhe_keyswitch_hybrid_acc: null argument");
    ARG_CHECK(key->plan == p, "fhe_keyswitch_hybrid_acc: key belongs to another plan");
    ARG_CHECK(sizeQl >= 1 && sizeQl <= p->sizeQ && batch >= 1, "fhe_keyswitch_hybrid_acc: bad level or batch");
    const KsLayout w = ks_layout(p, sizeQl, batch);
    ARG_CHECK(wsBytes >= w.total * 8, "fhe_keyswitch_hybrid_acc: workspace too small");
    RT_CHECK(rt::set_device(p->ctx->device));
    return keyswitch_run(p, key, cin, sizeQl, batch, acc0, acc1, (uint64_t*)ws, w, st, true);
}

extern "C" fhe_status fhe_ckks_eval_mult(fhe_ks_plan* p, const fhe_ks_key* key, const uint64_t* a0, const uint64_t* a1,
                                         const uint64_t* b0, const uint64_t* b1, uint32_t sizeQl, uint32_t batch,
                                         uint64_t* c0, uint64_t* c1, void* wsv, size_t wsBytes, void* st) {
    ARG_CHECK(p && key && a0 && a1 && b0 && b1 && c0 && c1 && wsv, "fhe_ckks_eval_mult: null argument");
    ARG_CHECK(key->plan == p, "fhe_ckks_eval_mult: key belongs to another plan");
    ARG_CHECK(sizeQl >= 1 && sizeQl <= p->sizeQ && batch >= 1, "fhe_ckks_eval_mult: bad level or batch");
    const KsLayout w = ks_layout(p, sizeQl, batch);
    ARG_CHECK(wsBytes >= w.total * 8, "fhe_ckks_eval_mult: workspace too small");
    fhe_ctx* c   = p->ctx;
    uint64_t* ws = (uint64_t*)wsv;
    RT_CHECK(rt::set_device(c->device));
    // EvalMultCore (base-leveledshe.cpp:607-644)
    if (fhe_status s = fhe_tensor(c, a0, a1, b0, b1, c0, c1, ws + w.d2, nullptr, sizeQl, batch, st))
        return s;
    // KeySwitchCore on d2 (:207) with `cv[0] += ab[0]; cv[1] += ab[1]` (:210-211) fused into the ModDown tails
    return keyswitch_run(p, key, ws + w.d2, sizeQl, batch, c0, c1, ws, w, st, true);
}

#define KS_COMMON_CHECKS(who)                                                                              \
    ARG_CHECK(p && ws, who ": null argument");                                                             \
    ARG_CHECK(sizeQl >= 1 && sizeQl <= p->sizeQ && batch >= 1, who ": bad level or batch");                \
    const KsLayout w = ks_layout(p, sizeQl, batch);                                                        \
    ARG_CHECK(wsBytes >= w.total * 8, who ": workspace too small");                                        \
    RT_CHECK(rt::set_device(p->ctx->device));                                                              \
    fhe_ks_plan::Level* lv = nullptr;                                                                      \
    if (fhe_status s_ = ks_level(p, sizeQl, &lv))                                                          \
        return s_;

extern "C" fhe_status fhe_ks_precompute(fhe_ks_plan* p, const uint64_t* c1, uint32_t sizeQl, uint32_t batch, void* ws,
                                        size_t wsBytes, void* st) {
    KS_COMMON_CHECKS("fhe_ks_precompute")
    ARG_CHECK(c1, "fhe_ks_precompute: null argument");
    return ks_precompute_run(p, lv, c1, batch, (uint64_t*)ws, w, st);
}
extern "C" fhe_status fhe_ks_fast_keyswitch(fhe_ks_plan* p, const fhe_ks_key* key, const uint64_t* c1, uint32_t sizeQl,
                                            uint32_t batch, uint64_t* out0, uint64_t* out1, void* ws, size_t wsBytes,
                                            void* st) {
    KS_COMMON_CHECKS("fhe_ks_fast_keyswitch")
    ARG_CHECK(key && c1 && out0 && out1 && key->plan == p, "fhe_ks_fast_keyswitch: bad key or null argument");
    return ks_fast_run(p, lv, key, c1, batch, out0, out1, (uint64_t*)ws, w, st, false);
}
// LeveledSHEBase::EvalFastRotation (base-leveledshe.cpp:432-463): ba = EvalFastKeySwitchCore(digits, key_k);
// ba[0] += cv[0]; both elements through AutomorphismTransform(k)
static fhe_status fast_rotation_run(fhe_ks_plan* p, fhe_ks_plan::Level* lv, const fhe_ks_key* key, const uint64_t* c0, const uint64_t* c1,
                                    uint32_t k, uint32_t batch, uint64_t* out0, uint64_t* out1, uint64_t* wsp, const KsLayout& w, void* st,
                                    uint64_t t) {
    fhe_ctx* c            = p->ctx;
    const uint32_t sizeQl = lv->sizeQl;
    if (fhe_status s = ks_fast_run(p, lv, key, c1, batch, wsp + w.k0, wsp + w.k1, wsp, w, st, false, t))
        return s;
    if (fhe_status s = fhe_add(c, wsp + w.k0, wsp + w.k0, c0, nullptr, sizeQl, batch, st))
        return s;
    if (fhe_status s = fhe_automorph(c, out0, wsp + w.k0, k, 1, nullptr, sizeQl, batch, st))
        return s;
    return fhe_automorph(c, out1, wsp + w.k1, k, 1, nullptr, sizeQl, batch, st);
}
extern "C" fhe_status fhe_eval_fast_rotation(fhe_ks_plan* p, const fhe_ks_key* key, const uint64_t* c0, const uint64_t* c1,
                                             uint32_t k, uint32_t sizeQl, uint32_t batch, uint64_t* out0, uint64_t* out1,
                                             void* ws, size_t wsBytes, void* st) {
    KS_COMMON_CHECKS("fhe_eval_fast_rotation")
    ARG_CHECK(key && c0 && c1 && out0 && out1 && key->plan == p, "fhe_eval_fast_rotation: bad key or null argument");
    ARG_CHECK(k % 2 == 1, "Automorphism index not odd");
    return fast_rotation_run(p, lv, key, c0, c1, k, batch, out0, out1, (uint64_t*)ws, w, st, 0);
}
// LeveledSHEBase::EvalAutomorphism (base-leveledshe.cpp:381-422) = KeySwitchInPlace + AutomorphismTransform on both
// elements; identical result to precompute + fast rotation
extern "C" fhe_status fhe_eval_automorphism(fhe_ks_plan* p, const fhe_ks_key* key, const uint64_t* c0, const uint64_t* c1,
                                            uint32_t k, uint32_t sizeQl, uint32_t batch, uint64_t* out0, uint64_t* out1,
                                            void* ws, size_t wsBytes, void* st) {
    if (fhe_status s = fhe_ks_precompute(p, c1, sizeQl, batch, ws, wsBytes, st))
        return s;
    return fhe_eval_fast_rotation(p, key, c0, c1, k, sizeQl, batch, out0, out1, ws, wsBytes, st);
}

// ---- BGV on HYBRID keys: the composites above with ApproxModDown's plaintext-modulus factors (t = GetPlaintextModulus(), passed by the
// reference whenever GetNoiseScale() != 1: keyswitch-hybrid.cpp:263, 299, 386).  Same plan, key, workspace and layout as the CKKS twins, the
// same launches: only the conversion constants of the ModDown differ (ks_down_conv).  Checks: those of the twin, t >= 2, t invertible modulo
// every p_j -- all before the first launch.
#define BGV_COMMON_CHECKS(who)                                      \
    KS_COMMON_CHECKS(who)                                           \
    ARG_CHECK(t >= 2, who ": t must be at least 2");                \
    {                                                               \
        fhe_conv* down_ = nullptr;                                  \
        if (fhe_status s_ = ks_down_conv(p, lv, t, who, &down_))    \
            return s_;                                              \
    }
// replaces KeySwitchHYBRID::KeySwitchCore (keyswitch-hybrid.cpp:308-400) under BGV
extern "C" fhe_status fhe_bgv_keyswitch_hybrid(fhe_ks_plan* p, const fhe_ks_key* key, const uint64_t* cin, uint32_t sizeQl, uint64_t t,
                                               uint32_t batch, uint64_t* out0, uint64_t* out1, void* ws, size_t wsBytes, void* st) {
    BGV_COMMON_CHECKS("fhe_bgv_keyswitch_hybrid")
    ARG_CHECK(key && cin && out0 && out1 && key->plan == p, "fhe_bgv_keyswitch_hybrid: bad key or null argument");
    return keyswitch_run(p, key, cin, sizeQl, batch, out0, out1, (uint64_t*)ws, w, st, false, t);
}
// ... with `acc0 += ks0(c); acc1 += ks1(c)` (base-leveledshe.cpp:207-211), the additions in the ModDown epilogue
extern "C" fhe_status fhe_bgv_keyswitch_hybrid_acc(fhe_ks_plan* p, const fhe_ks_key* key, const uint64_t* cin, uint32_t sizeQl, uint64_t t,
                                                   uint32_t batch, uint64_t* acc0, uint64_t* acc1, void* ws, size_t wsBytes, void* st) {
    BGV_COMMON_CHECKS("fhe_bgv_keyswitch_hybrid_acc")
    ARG_CHECK(key && cin && acc0 && acc1 && key->plan == p, "fhe_bgv_keyswitch_hybrid_acc: bad key or null argument");
    return keyswitch_run(p, key, cin, sizeQl, batch, acc0, acc1, (uint64_t*)ws, w, st, true, t);
}
// replaces LeveledSHEBase::EvalMult(ct, ct, key) (base-leveledshe.cpp:201-214, EvalMultCore :607-644) under BGV
extern "C" fhe_status fhe_bgv_eval_mult(fhe_ks_plan* p, const fhe_ks_key* key, const uint64_t* a0, const uint64_t* a1, const uint64_t* b0,
                                        const uint64_t* b1, uint32_t sizeQl, uint64_t t, uint32_t batch, uint64_t* c0, uint64_t* c1,
                                        void* ws, size_t wsBytes, void* st) {
    BGV_COMMON_CHECKS("fhe_bgv_eval_mult")
    ARG_CHECK(key && a0 && a1 && b0 && b1 && c0 && c1 && key->plan == p, "fhe_bgv_eval_mult: bad key or null argument");
    uint64_t* wsp = (uint64_t*)ws;
    if (fhe_status s = fhe_tensor(p->ctx, a0, a1, b0, b1, c0, c1, wsp + w.d2, nullptr, sizeQl, batch, st))
        return s;
    return keyswitch_run(p, key, wsp + w.d2, sizeQl, batch, c0, c1, wsp, w, st, true, t);
}
// replaces KeySwitchHYBRID::EvalFastKeySwitchCore (keyswitch-hybrid.cpp:381-400) under BGV, on the digits fhe_ks_precompute left (the digit
// decomposition does not depend on t: hoisting is shared with CKKS)
extern "C" fhe_status fhe_bgv_ks_fast_keyswitch(fhe_ks_plan* p, const fhe_ks_key* key, const uint64_t* c1, uint32_t sizeQl, uint64_t t,
                                                uint32_t batch, uint64_t* out0, uint64_t* out1, void* ws, size_t wsBytes, void* st) {
    BGV_COMMON_CHECKS("fhe_bgv_ks_fast_keyswitch")
    ARG_CHECK(key && c1 && out0 && out1 && key->plan == p, "fhe_bgv_ks_fast_keyswitch: bad key or null argument");
    return ks_fast_run(p, lv, key, c1, batch, out0, out1, (uint64_t*)ws, w, st, false, t);
}
// replaces LeveledSHEBase::EvalFastRotation (base-leveledshe.cpp:432-463) under BGV
extern "C" fhe_status fhe_bgv_eval_fast_rotation(fhe_ks_plan* p, const fhe_ks_key* key, const uint64_t* c0, const uint64_t* c1, uint32_t k,
                                                 uint32_t sizeQl, uint64_t t, uint32_t batch, uint64_t* out0, uint64_t* out1, void* ws,
                                                 size_t wsBytes, void* st) {
    BGV_COMMON_CHECKS("fhe_bgv_eval_fast_rotation")
    ARG_CHECK(key && c0 && c1 && out0 && out1 && key->plan == p, "fhe_bgv_eval_fast_rotation: bad key or null argument");
    ARG_CHECK(k % 2 == 1, "Automorphism index not odd");
    return fast_rotation_run(p, lv, key, c0, c1, k, batch, out0, out1, (uint64_t*)ws, w, st, t);
}
// replaces LeveledSHEBase::EvalAutomorphism (base-leveledshe.cpp:381-422) under BGV
extern "C" fhe_status fhe_bgv_eval_automorphism(fhe_ks_plan* p, const fhe_ks_key* key, const uint64_t* c0, const uint64_t* c1, uint32_t k,
                                                uint32_t sizeQl, uint64_t t, uint32_t batch, uint64_t* out0, uint64_t* out1, void* ws,
                                                size_t wsBytes, void* st) {
    BGV_COMMON_CHECKS("fhe_bgv_eval_automorphism")
    ARG_CHECK(key && c0 && c1 && out0 && out1 && key->plan == p, "fhe_bgv_eval_automorphism: bad key or null argument");
    ARG_CHECK(k % 2 == 1, "Automorphism index not odd");
    uint64_t* wsp = (uint64_t*)ws;
    if (fhe_status s = ks_precompute_run(p, lv, c1, batch, wsp, w, st))
        return s;
    return fast_rotation_run(p, lv, key, c0, c1, k, batch, out0, out1, wsp, w, st, t);
}
#undef BGV_COMMON_CHECKS

// ---- double hoisting: work in the extended basis Q_l u P, one ModDown at the end (ckksrns-fhe.cpp:1830-2000) ----
static fhe_status ext_limbs(const fhe_ks_plan* p, uint32_t sizeQl, std::vector<uint32_t>& idx) {
    idx.resize(sizeQl + p->sizeP);
    for (uint32_t i = 0; i < sizeQl; ++i)
        idx[i] = i;
    for (uint32_t j = 0; j < p->sizeP; ++j)
        idx[sizeQl + j] = p->sizeQ + j;
    return FHE_OK;
}
// [P]_{q_i} as Shoup pairs for limbs [0, sizeQl)  (PModq, rns-cryptoparameters.cpp:200-203), cached per level
static fhe_status ks_pmodq(fhe_ks_plan* p, fhe_ks_plan::Level* lv, TwPair** d) {
    std::lock_guard<std::mutex> lock(p->cacheMutex);
    if (!lv->d_PModq) {
        fhe_ctx* c = p->ctx;
        std::vector<uint64_t> pm(p->sizeP);
        for (uint32_t j = 0; j < p->sizeP; ++j)
            pm[j] = c->q[p->sizeQ + j];
        std::vector<TwPair> h(lv->sizeQl);
        for (uint32_t i = 0; i < lv->sizeQl; ++i) {
            const uint64_t v = host::prod_mod(pm, -1, c->q[i]);
            h[i]             = TwPair{v, host::shoup(v, c->q[i])};
        }
        if (fhe_status s = dev_copy(&p->owned, h.data(), h.size(), &lv->d_PModq))
            return s;
    }
    *d = lv->d_PModq;
    return FHE_OK;
}
// KeySwitchHYBRID::KeySwitchExt for one element (keyswitch-hybrid.cpp:217-243): out [batch][sizeQl+sizeP][N], Q_l rows =
// c * [P]_{q_i}, P rows = 0
extern "C" fhe_status fhe_ks_ext(fhe_ks_plan* p, const uint64_t* cin, uint32_t sizeQl, uint32_t batch, uint64_t* out, void* st) {
    ARG_CHECK(p && cin && out, "fhe_ks_ext: null argument");
    ARG_CHECK(sizeQl >= 1 && sizeQl <= p->sizeQ && batch >= 1, "fhe_ks_ext: bad level or batch");
    fhe_ctx* c = p->ctx;
    RT_CHECK(rt::set_device(c->device));
    fhe_ks_plan::Level* lv = nullptr;
    if (fhe_status s = ks_level(p, sizeQl, &lv))
        return s;
    TwPair* dP = nullptr;
    if (fhe_status s = ks_pmodq(p, lv, &dP))
        return s;
    const uint32_t sizeQlP = sizeQl + p->sizeP;
    if (fhe_status s = zero_rows(c, out, sizeQlP, sizeQl, p->sizeP, batch, st))
        return s;
    return elem_run<OP_MUL_CONST>(c, out, cin, nullptr, dP, nullptr, sizeQl, batch, st, "fhe_ks_ext", 0, 0, 0, 0, sizeQlP, 0);
}
// EvalFastKeySwitchCoreExt on digits already in the workspace (fhe_ks_precompute): out0/out1 [batch][sizeQl+sizeP][N]
extern "C" fhe_status fhe_ks_fast_keyswitch_ext(fhe_ks_plan* p, const fhe_ks_key* key, const uint64_t* c1, uint32_t sizeQl,
                                                uint32_t batch, uint64_t* out0, uint64_t* out1, void* ws, size_t wsBytes,
                                                void* st) {
    KS_COMMON_CHECKS("fhe_ks_fast_keyswitch_ext")
    ARG_CHECK(key && c1 && out0 && out1 && key->plan == p, "fhe_ks_fast_keyswitch_ext: bad key or null argument");
    return ks_inner_run(p, lv, key, c1, batch, out0, out1, (uint64_t*)ws, w, st);
}
// LeveledSHECKKSRNS::EvalFastRotationExt (ckksrns-leveledshe.cpp:534-582): EvalFastKeySwitchCoreExt, optionally
// + c0 * [P]_{q_i} on the first element's Q_l limbs, then the automorphism on both extended elements
extern "C" fhe_status fhe_eval_fast_rotation_ext(fhe_ks_plan* p, const fhe_ks_key* key, const uint64_t* c0, const uint64_t* c1,
                                                 uint32_t k, int addFirst, uint32_t sizeQl, uint32_t batch, uint64_t* out0,
                                                 uint64_t* out1, void* ws, size_t wsBytes, void* st) {
    KS_COMMON_CHECKS("fhe_eval_fast_rotation_ext")
    ARG_CHECK(key && c0 && c1 && out0 && out1 && key->plan == p, "fhe_eval_fast_rotation_ext: bad key or null argument");
    ARG_CHECK(k % 2 == 1, "Automorphism index not odd");
    fhe_ctx* c    = p->ctx;
    uint64_t* wsp = (uint64_t*)ws;
    const uint32_t sizeQlP = sizeQl + p->sizeP;
    if (addFirst) {  // cTilda[0] += psiC0  (:561-570): e0 rows [0, sizeQl) += c0 * PModq, in the inner product's own store
        TwPair* dP = nullptr;
        if (fhe_status s = ks_pmodq(p, lv, &dP))
            return s;
        uint64_t *e0 = wsp + w.e0, *e1 = wsp + w.e1;
        if (fhe_status s = ks_inner_multi_run(p, lv, &key, 1, c1, batch, &e0, &e1, c0, dP, wsp, w, st))
            return s;
    }
    else if (fhe_status s = ks_inner_run(p, lv, key, c1, batch, wsp + w.e0, wsp + w.e1, wsp, w, st))
        return s;
    std::vector<uint32_t> idx;
    ext_limbs(p, sizeQl, idx);
    if (fhe_status s = fhe_automorph(c, out0, wsp + w.e0, k, 1, idx.data(), sizeQlP, batch, st))
        return s;
    return fhe_automorph(c, out1, wsp + w.e1, k, 1, idx.data(), sizeQlP, batch, st);
}
// KeySwitchHYBRID::KeySwitchDown (keyswitch-hybrid.cpp:245-278): ApproxModDown of both extended elements
extern "C" fhe_status fhe_ks_down(fhe_ks_plan* p, const uint64_t* x0, const uint64_t* x1, uint32_t sizeQl, uint32_t batch,
                                  uint64_t* out0, uint64_t* out1, void* ws, size_t wsBytes, void* st) {
    KS_COMMON_CHECKS("fhe_ks_down")
    ARG_CHECK(x0 && x1 && out0 && out1, "fhe_ks_down: null argument");
    uint64_t* wsp = (uint64_t*)ws;
    if (fhe_status s = mod_down_run(p, lv, x0, batch, out0, wsp + w.pcoef, wsp + w.md, st))
        return s;
    return mod_down_run(p, lv, x1, batch, out1, wsp + w.pcoef, wsp + w.md, st);
}

// ---- evaluation-key generation (keygen_kernels.h) ----
// KeySwitchHYBRID::KeySwitchGenInternal (keyswitch-hybrid.cpp:51-130), LeveledSHEBase::EvalAutomorphismKeyGen (base-leveledshe.cpp:336-379)
// and PKEBase::KeyGenInternal (base-pke.cpp:47-98) for any number of keys: everything that is not sampling or transforming is ONE launch
// of keygen_combine_kernel per kKeygenKeys keys (the keys' automorphism indices travel by value in the kernel arguments, whose 4 KiB set
// that bound; the grid never does: 256 keys x 256 limbs x 64 tiles is far below 2^31 workgroups).  The factors f[j][i] and ns mod q_i go
// through the context's table cache (const_table): the first call with a new (factor, ns) uploads, later calls are pure launches.
static bool keygen_overlap(const void* x, size_t nx, const void* y, size_t ny) {
    const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y;
    return a < b + ny && b < a + nx;
}
// every check of the family, before anything is enqueued; oldRows: rows of sOld the kernel may read (0: no sOld term)
static fhe_status keygen_check(const std::string& who, const fhe_ctx* c, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t nKeys,
                               uint32_t nParts, const uint64_t* a, const uint64_t* e, const uint64_t* sNew, const uint32_t* kNew,
                               const uint64_t* sOld, const uint32_t* kOld, uint32_t oldRows, uint64_t ns, const uint64_t* out) {
    ARG_CHECK(c && a && e && sNew && out && (sOld || !oldRows), who + ": null argument");
    ARG_CHECK(nKeys >= 1, who + ": nKeys must be >= 1");
    ARG_CHECK(nParts >= 1, who + ": nParts must be >= 1");
    ARG_CHECK(nLimbs >= 1 && nLimbs <= (uint32_t)kMaxLimbs, who + ": nLimbs out of range");
    for (uint32_t i = 0; i < nLimbs; ++i)
        ARG_CHECK((limbIdx ? limbIdx[i] : i) < c->L, who + ": limb index exceeds context size");
    ARG_CHECK(ns != 0, who + ": the noise scale must not be zero");
    for (uint32_t k = 0; k < nKeys; ++k)
        for (const uint32_t* ks : {kNew, kOld})
            if (ks) {
                ARG_CHECK(ks[k] % 2 == 1, "Automorphism index not odd");  // poly-impl.h:337-338
                ARG_CHECK(ks[k] < 2u * c->N, who + ": automorphism index out of range (1 <= k < 2N)");
            }
    ARG_CHECK((uint64_t)nKeys * nParts * nLimbs < ((uint64_t)1 << 31), who + ": nKeys * nParts * nLimbs too large");
    const size_t row = (size_t)c->N * 8, slab = (size_t)nKeys * nParts * nLimbs * row;
    ARG_CHECK(out == e || !keygen_overlap(out, slab, e, slab), who + ": out may be e itself but not overlap it otherwise");
    ARG_CHECK(!keygen_overlap(out, slab, a, slab) && !keygen_overlap(out, slab, sNew, nLimbs * row) &&
                  !(oldRows && keygen_overlap(out, slab, sOld, oldRows * row)),
              who + ": out must not overlap a, sNew or sOld");
    return FHE_OK;
}
// rows of sOld that the factor table makes the kernel read: up to the last limb with a non-zero factor
static uint32_t keygen_old_rows(const fhe_ctx* c, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t nParts, const uint64_t* factor) {
    uint32_t rows = 0;
    if (factor && c && nLimbs <= (uint32_t)kMaxLimbs)
        for (uint32_t j = 0; j < nParts; ++j)
            for (uint32_t i = 0; i < nLimbs; ++i)
                if ((limbIdx ? limbIdx[i] : i) < c->L && factor[(size_t)j * nLimbs + i] % c->q[limbIdx ? limbIdx[i] : i])
                    rows = std::max(rows, i + 1);
    return rows;
}
static fhe_status keygen_combine_run(const std::string& who, fhe_ctx* c, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t nKeys,
                                     uint32_t nParts, const uint64_t* a, const uint64_t* e, const uint64_t* sNew, const uint32_t* kNew,
                                     const uint64_t* sOld, const uint32_t* kOld, const uint64_t* factor, uint64_t ns, uint64_t* out,
                                     void* st) {
    const uint32_t oldRows = keygen_old_rows(c, limbIdx, nLimbs, nParts, factor);
    if (fhe_status s = keygen_check(who, c, limbIdx, nLimbs, nKeys, nParts, a, e, sNew, kNew, sOld, kOld, oldRows, ns, out))
        return s;
    KeygenArgs g;
    if (fhe_status s = make_sel(c, limbIdx, nLimbs, &g.sel, who.c_str()))
        return s;
    RT_CHECK(rt::set_device(c->device));
    // the table: f[nParts][nLimbs] (when there is an sOld term), then ns mod q_i [nLimbs] (unless ns == 1)
    std::vector<uint32_t> li;
    std::vector<uint64_t> v;
    for (uint32_t j = 0; j < (factor ? nParts : 0u) + (ns != 1 ? 1u : 0u); ++j)
        for (uint32_t i = 0; i < nLimbs; ++i) {
            const uint32_t l = limbIdx ? limbIdx[i] : i;
            li.push_back(l);
            v.push_back((factor && j < nParts ? factor[(size_t)j * nLimbs + i] : ns) % c->q[l]);
        }
    const TwPair* table = nullptr;
    if (fhe_status s = const_tables_trim(c))
        return s;
    std::shared_lock<std::shared_mutex> gate(c->constTabsGate);
    if (!v.empty())
        if (fhe_status s = const_table(c, li.data(), v.data(), (uint32_t)v.size(), &table))
            return s;
    g.sNew = sNew, g.sOld = factor ? sOld : sNew, g.lc = c->d_lc, g.tab = table;
    g.logN = c->logN, g.nLimbs = nLimbs, g.nParts = nParts;
    const uint32_t tilesPerRow = c->logN > (uint32_t)kKeygenTileLog ? 1u << (c->logN - kKeygenTileLog) : 1u;
    const size_t keyWords      = ((size_t)nParts * nLimbs) << c->logN;
    for (uint32_t first = 0; first < nKeys; first += (uint32_t)kKeygenKeys) {
        g.nKeys = std::min<uint32_t>(kKeygenKeys, nKeys - first);
        for (uint32_t k = 0; k < (uint32_t)kKeygenKeys; ++k) {
            g.kNew[k] = k < g.nKeys && kNew ? kNew[first + k] : 1u;
            g.kOld[k] = k < g.nKeys && kOld ? kOld[first + k] : 1u;
        }
        g.out = out + first * keyWords, g.a = a + first * keyWords, g.e = e + first * keyWords;
        const uint32_t grid = g.nKeys * nLimbs * tilesPerRow;
        if (factor && ns == 1)
            FHE_LAUNCH((keygen_combine_kernel<true, true>), grid, st, g);
        else if (factor)
            FHE_LAUNCH((keygen_combine_kernel<false, true>), grid, st, g);
        else if (ns == 1)
            FHE_LAUNCH((keygen_combine_kernel<true, false>), grid, st, g);
        else
            FHE_LAUNCH((keygen_combine_kernel<false, false>), grid, st, g);
        LAUNCH_CHECK();
    }
    return FHE_OK;
}
extern "C" fhe_status fhe_keygen_combine(fhe_ctx* c, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t nKeys, uint32_t nParts,
                                         const uint64_t* a, const uint64_t* e, const uint64_t* sNew, const uint32_t* kNew,
                                         const uint64_t* sOld, const uint32_t* kOld, const uint64_t* factor, uint64_t ns, uint64_t* out,
                                         void* st) {
    return keygen_combine_run("fhe_keygen_combine", c, limbIdx, nLimbs, nKeys, nParts, a, e, sNew, kNew, sOld, kOld, factor, ns, out, st);
}
// the sNewExt block of KeySwitchGenInternal (keyswitch-hybrid.cpp:59-83): the Q rows as they are; the P rows from limb 0 in COEFFICIENT
// format, centre-switched to every p_j (PolyImpl::SwitchModulus) and transformed
extern "C" fhe_status fhe_ks_secret_extend(fhe_ks_plan* p, const uint64_t* sQ, uint64_t* outExt, void* ws, size_t wsBytes, void* st) {
    ARG_CHECK(p && sQ && outExt && ws, "fhe_ks_secret_extend: null argument");
    fhe_ctx* c       = p->ctx;
    const size_t row = (size_t)c->N * 8;
    ARG_CHECK(wsBytes >= row, "fhe_ks_secret_extend: workspace too small (one limb row)");
    ARG_CHECK(outExt == sQ || !keygen_overlap(outExt, (p->sizeQ + p->sizeP) * row, sQ, p->sizeQ * row),
              "fhe_ks_secret_extend: outExt may start at sQ but not overlap it otherwise");
    ARG_CHECK(!keygen_overlap(ws, row, outExt, (p->sizeQ + p->sizeP) * row) && !keygen_overlap(ws, row, sQ, p->sizeQ * row),
              "fhe_ks_secret_extend: the workspace overlaps an operand");
    RT_CHECK(rt::set_device(c->device));
    if (outExt != sQ)
        RT_CHECK(rt::d2d(outExt, sQ, p->sizeQ * row, (rt::stream_t)st));
    const uint32_t limb0 = 0;
    if (fhe_status s = fhe_ntt_inv_oop(c, sQ, (uint64_t*)ws, &limb0, 1, 1, st))
        return s;
    std::vector<uint32_t> pIdx(p->sizeP);
    for (uint32_t j = 0; j < p->sizeP; ++j)
        pIdx[j] = p->sizeQ + j;
    uint64_t* pRows = outExt + ((size_t)p->sizeQ << c->logN);
    if (fhe_status s = fhe_switch_modulus(c, pRows, pIdx.data(), p->sizeP, (const uint64_t*)ws, 1, 0, 0, 1, st))
        return s;
    return fhe_ntt_fwd(c, pRows, pIdx.data(), p->sizeP, 1, st);
}
// f[j][i] = [P]_{q_i} for the limbs of digit j (keyswitch-hybrid.cpp:105-119 with the partition of rns-cryptoparameters.cpp:85-91), else 0
static std::vector<uint64_t> ks_keygen_factors(const fhe_ks_plan* p) {
    const fhe_ctx* c     = p->ctx;
    const uint32_t sizeQP = p->sizeQ + p->sizeP;
    std::vector<uint64_t> pm(c->q.begin() + p->sizeQ, c->q.begin() + sizeQP), f((size_t)p->numPartQ * sizeQP, 0);
    for (uint32_t j = 0; j < p->numPartQ; ++j)
        for (uint32_t i = p->alpha * j; i < std::min(p->alpha * (j + 1), p->sizeQ); ++i)
            f[(size_t)j * sizeQP + i] = host::prod_mod(pm, -1, c->q[i]);
    return f;
}
extern "C" fhe_status fhe_ks_keygen_hybrid(fhe_ks_plan* p, uint32_t nKeys, const uint32_t* kNew, const uint32_t* kOld,
                                           const uint64_t* sNewExt, const uint64_t* sOld, uint64_t ns, const uint64_t* a, const uint64_t* e,
                                           uint64_t* devKeyB, void* st) {
    ARG_CHECK(p && sOld, "fhe_ks_keygen_hybrid: null argument");
    const std::vector<uint64_t> f = ks_keygen_factors(p);
    return keygen_combine_run("fhe_ks_keygen_hybrid", p->ctx, nullptr, p->sizeQ + p->sizeP, nKeys, p->numPartQ, a, e, sNewExt, kNew, sOld,
                              kOld, f.data(), ns, devKeyB, st);
}
extern "C" fhe_status fhe_ks_keygen_counters(const fhe_ks_plan* p, uint32_t nKeys, uint64_t* nA, uint64_t* nE) {
    ARG_CHECK(p && nA && nE, "fhe_ks_keygen_counters: null argument");
    ARG_CHECK(nKeys >= 1, "fhe_ks_keygen_counters: nKeys must be >= 1");
    const uint64_t towers = (uint64_t)nKeys * p->numPartQ;
    *nA = (((towers * (p->sizeQ + p->sizeP)) << p->ctx->logN) + 255) / 256;  // two 64-bit words per uniform residue, 512 per block
    *nE = ((towers << p->ctx->logN) + 511) / 512;                            // one word per Gaussian coefficient
    return FHE_OK;
}
// the seeded form, a composition: a = the uniform sampler's words as drawn (the reference draws a in EVALUATION format); e = the Gaussian
// sampler's words, transformed in the buffer that then becomes b.  Every argument is checked before the first launch.
extern "C" fhe_status fhe_ks_keygen_hybrid_blake2(fhe_ks_plan* p, uint32_t nKeys, const uint32_t* kNew, const uint32_t* kOld,
                                                  const uint64_t* sNewExt, const uint64_t* sOld, uint64_t ns, double sigma,
                                                  const uint32_t key[16], uint64_t counterA, uint64_t counterE, uint64_t* devKeyB,
                                                  uint64_t* devKeyA, void* st) {
    const std::string who = "fhe_ks_keygen_hybrid_blake2";
    ARG_CHECK(p && sOld && key && devKeyA && devKeyB, who + ": null argument");
    fhe_ctx* c            = p->ctx;
    const uint32_t sizeQP = p->sizeQ + p->sizeP;
    if (fhe_status s = keygen_check(who, c, nullptr, sizeQP, nKeys, p->numPartQ, devKeyA, devKeyB, sNewExt, kNew, sOld, kOld, p->sizeQ, ns,
                                    devKeyB))
        return s;
    ARG_CHECK(sigma > 1.000000001 && sigma < 300.0, who + ": the inversion sampler covers 1 < sigma < 300 (the reference's Peikert range)");
    const size_t slab = (((size_t)nKeys * p->numPartQ * sizeQP) << c->logN) * 8, row = (size_t)c->N * 8;
    ARG_CHECK(!keygen_overlap(devKeyA, slab, sNewExt, sizeQP * row) && !keygen_overlap(devKeyA, slab, sOld, p->sizeQ * row),
              who + ": devKeyA must not overlap sNewExt or sOld");
    const uint32_t towers = nKeys * p->numPartQ;
    if (fhe_status s = fhe_sample_uniform_blake2(c, devKeyA, nullptr, sizeQP, towers, key, counterA, st))
        return s;
    if (fhe_status s = fhe_sample_gaussian_blake2(c, devKeyB, nullptr, sizeQP, towers, sigma, key, counterE, st))
        return s;
    if (fhe_status s = fhe_ntt_fwd(c, devKeyB, nullptr, sizeQP, towers, st))
        return s;
    return fhe_ks_keygen_hybrid(p, nKeys, kNew, kOld, sNewExt, sOld, ns, devKeyA, devKeyB, devKeyB, st);
}

// ---- BV evaluation keys (KeySwitchBV::KeySwitchGenInternal, keyswitch-bv.cpp:49-225) ----
// The secret-key overloads (:49-160) are the formula of keygen_combine_kernel with the table of host::bv_keygen_factors over the context's
// leading sizeQ limbs: no new kernel.  The public-key overload (:162-225, PREBase::ReKeyGen) is keygen_pk_combine_kernel.
// sizeQ and the digit size, before anything else is looked at; D0 towers and their factor table [D0][sizeQ]
static fhe_status bv_keygen_shape(const std::string& who, const fhe_ctx* c, uint32_t sizeQ, uint32_t baseBits, uint32_t* D0,
                                  std::vector<uint64_t>* factor) {
    ARG_CHECK(c, who + ": null argument");
    ARG_CHECK(sizeQ >= 1 && sizeQ <= c->L, who + ": sizeQ must be in [1, limbs of the context]");
    std::vector<uint64_t> f;
    *D0 = fhe_crt_decompose_towers(c, nullptr, sizeQ, baseBits) ? host::bv_keygen_factors(c->q.data(), sizeQ, baseBits, f) : 0;
    if (*D0 == 0)
        return fail(FHE_ERR_UNSUPPORTED, who + ": digit size outside the device path (baseBits <= 31, every window inside the word)");
    if (factor)
        factor->swap(f);
    return FHE_OK;
}
extern "C" uint32_t fhe_bv_keygen_factors(const fhe_ctx* c, uint32_t sizeQ, uint32_t baseBits, uint64_t* factor) {
    if (!c || sizeQ < 1 || sizeQ > c->L || fhe_crt_decompose_towers(c, nullptr, sizeQ, baseBits) == 0)
        return 0;
    std::vector<uint64_t> f;
    const uint32_t D0 = host::bv_keygen_factors(c->q.data(), sizeQ, baseBits, f);
    if (factor)
        std::copy(f.begin(), f.end(), factor);
    return D0;
}
extern "C" fhe_status fhe_bv_keygen(fhe_ctx* c, uint32_t sizeQ, uint32_t baseBits, uint32_t nKeys, const uint32_t* kNew,
                                    const uint32_t* kOld, const uint64_t* sNew, const uint64_t* sOld, uint64_t ns, const uint64_t* a,
                                    const uint64_t* e, uint64_t* devKeyB, void* st) {
    const std::string who = "fhe_bv_keygen";
    ARG_CHECK(c && sOld, who + ": null argument");
    uint32_t D0 = 0;
    std::vector<uint64_t> f;
    if (fhe_status s = bv_keygen_shape(who, c, sizeQ, baseBits, &D0, &f))
        return s;
    return keygen_combine_run(who, c, nullptr, sizeQ, nKeys, D0, a, e, sNew, kNew, sOld, kOld, f.data(), ns, devKeyB, st);
}
extern "C" fhe_status fhe_bv_keygen_counters(const fhe_ctx* c, uint32_t sizeQ, uint32_t baseBits, uint32_t nKeys, int form,
                                             uint64_t* nAorU, uint64_t* nE) {
    const std::string who = "fhe_bv_keygen_counters";
    ARG_CHECK(c && nAorU && nE, who + ": null argument");
    ARG_CHECK(nKeys >= 1, who + ": nKeys must be >= 1");
    ARG_CHECK(form == 0 || form == 1, who + ": form is 0 (secret key) or 1 (public key)");
    uint32_t D0 = 0;
    if (fhe_status s = bv_keygen_shape(who, c, sizeQ, baseBits, &D0, nullptr))
        return s;
    const uint64_t coef = ((uint64_t)nKeys * D0) << c->logN;  // coefficients of one error tower set
    if (form == 0) {
        *nAorU = (coef * sizeQ + 255) / 256;  // two 64-bit words per uniform residue, 512 per block
        *nE    = (coef + 511) / 512;          // one word per Gaussian coefficient
    } else {
        *nAorU = (coef + 511) / 512;      // one word per coefficient of u
        *nE    = 2 * ((coef + 511) / 512);  // e0, then e1 from the next block (N >= 512: the next word)
    }
    return FHE_OK;
}
// the seeded secret-key form: the composition of fhe_ks_keygen_hybrid_blake2 over nKeys * D0 towers of sizeQ limbs
extern "C" fhe_status fhe_bv_keygen_blake2(fhe_ctx* c, uint32_t sizeQ, uint32_t baseBits, uint32_t nKeys, const uint32_t* kNew,
                                           const uint32_t* kOld, const uint64_t* sNew, const uint64_t* sOld, uint64_t ns, double sigma,
                                           const uint32_t key[16], uint64_t counterA, uint64_t counterE, uint64_t* devKeyB,
                                           uint64_t* devKeyA, void* st) {
    const std::string who = "fhe_bv_keygen_blake2";
    ARG_CHECK(c && sOld && key && devKeyA && devKeyB, who + ": null argument");
    uint32_t D0 = 0;
    std::vector<uint64_t> f;
    if (fhe_status s = bv_keygen_shape(who, c, sizeQ, baseBits, &D0, &f))
        return s;
    if (fhe_status s = keygen_check(who, c, nullptr, sizeQ, nKeys, D0, devKeyA, devKeyB, sNew, kNew, sOld, kOld, sizeQ, ns, devKeyB))
        return s;
    ARG_CHECK(sigma > 1.000000001 && sigma < 300.0, who + ": the inversion sampler covers 1 < sigma < 300 (the reference's Peikert range)");
    const size_t row = (size_t)c->N * 8, slab = (size_t)nKeys * D0 * sizeQ * row;
    ARG_CHECK(!keygen_overlap(devKeyA, slab, sNew, sizeQ * row) && !keygen_overlap(devKeyA, slab, sOld, sizeQ * row),
              who + ": devKeyA must not overlap sNew or sOld");
    const uint32_t towers = nKeys * D0;
    if (fhe_status s = fhe_sample_uniform_blake2(c, devKeyA, nullptr, sizeQ, towers, key, counterA, st))
        return s;
    if (fhe_status s = fhe_sample_gaussian_blake2(c, devKeyB, nullptr, sizeQ, towers, sigma, key, counterE, st))
        return s;
    if (fhe_status s = fhe_ntt_fwd(c, devKeyB, nullptr, sizeQ, towers, st))
        return s;
    return keygen_combine_run(who, c, nullptr, sizeQ, nKeys, D0, devKeyA, devKeyB, sNew, kNew, sOld, kOld, f.data(), ns, devKeyB, st);
}
static uint32_t bv_keygen_tiles(const fhe_ctx* c) { return c->logN > (uint32_t)kKeygenTileLog ? 1u << (c->logN - kKeygenTileLog) : 1u; }
struct BvKeygenPkOperands {
    const uint64_t *p0, *p1, *sOld, *u, *e0, *e1;
    uint64_t *outB, *outA;
};
// every check of the public-key form, before anything is enqueued
static fhe_status bv_keygen_pk_check(const std::string& who, const fhe_ctx* c, uint32_t sizeQ, uint32_t D0, uint32_t nKeys, int pkPerKey,
                                     const BvKeygenPkOperands& o, uint64_t ns) {
    ARG_CHECK(o.p0 && o.p1 && o.sOld && o.u && o.e0 && o.e1 && o.outB && o.outA, who + ": null argument");
    ARG_CHECK(nKeys >= 1, who + ": nKeys must be >= 1");
    ARG_CHECK(sizeQ <= (uint32_t)kMaxLimbs, who + ": sizeQ out of range");
    ARG_CHECK(ns != 0, who + ": the noise scale must not be zero");
    ARG_CHECK((uint64_t)nKeys * D0 * sizeQ * bv_keygen_tiles(c) < ((uint64_t)1 << 31), who + ": nKeys * D_0 * sizeQ too large");
    const size_t row = (size_t)c->N * 8, slab = (size_t)nKeys * D0 * sizeQ * row, pk = (size_t)(pkPerKey ? nKeys : 1u) * sizeQ * row;
    ARG_CHECK(!keygen_overlap(o.outB, slab, o.outA, slab), who + ": devKeyB and devKeyA overlap");
    ARG_CHECK(o.outB == o.e0 || !keygen_overlap(o.outB, slab, o.e0, slab), who + ": devKeyB may be e0 itself but not overlap it otherwise");
    ARG_CHECK(o.outA == o.e1 || !keygen_overlap(o.outA, slab, o.e1, slab), who + ": devKeyA may be e1 itself but not overlap it otherwise");
    ARG_CHECK(!keygen_overlap(o.outA, slab, o.e0, slab) && !keygen_overlap(o.outB, slab, o.e1, slab),
              who + ": devKeyB overlaps e1 or devKeyA overlaps e0");
    for (const uint64_t* out : {o.outB, o.outA}) {
        ARG_CHECK(!keygen_overlap(out, slab, o.u, slab), who + ": an output overlaps u");
        ARG_CHECK(!keygen_overlap(out, slab, o.p0, pk) && !keygen_overlap(out, slab, o.p1, pk), who + ": an output overlaps the public key");
        ARG_CHECK(!keygen_overlap(out, slab, o.sOld, sizeQ * row), who + ": an output overlaps sOld");
    }
    return FHE_OK;
}
// pieces the tower walk of keygen_pk_combine_kernel is cut into: one, unless keys x rows x tiles alone leave fewer than four workgroups
// (16 waves) per compute unit, the filling the encrypt and decrypt combines aim at; then as many as reach it (one key at
// N = 2^15 with 7 limbs is 112 workgroups, and the walk in 7 pieces takes half the time of the walk in one)
static uint32_t bv_keygen_pk_pieces(const fhe_ctx* c, uint32_t sizeQ, uint32_t D0, uint32_t nKeys) {
    const uint64_t groups = (uint64_t)nKeys * sizeQ * bv_keygen_tiles(c), want = 4ull * (c->cus ? c->cus : 256);
    if (groups >= want)
        return 1;
    return (uint32_t)std::min<uint64_t>(D0, (want + groups - 1) / groups);
}
// (the arguments have passed bv_keygen_pk_check)
static fhe_status bv_keygen_pk_run(const std::string& who, fhe_ctx* c, uint32_t sizeQ, uint32_t D0, const std::vector<uint64_t>& factor,
                                   uint32_t nKeys, int pkPerKey, const BvKeygenPkOperands& o, uint64_t ns, void* st) {
    KeygenPkArgs g;
    if (fhe_status s = make_sel(c, nullptr, sizeQ, &g.sel, who.c_str()))
        return s;
    RT_CHECK(rt::set_device(c->device));
    // the table: f[D0][sizeQ], then ns mod q_i [sizeQ] unless ns = 1 modulo every limb
    std::vector<uint32_t> li;
    std::vector<uint64_t> v(factor);
    bool ns1 = true;
    for (uint32_t i = 0; i < sizeQ; ++i)
        ns1 = ns1 && ns % c->q[i] == 1;
    for (uint32_t j = 0; j < D0 + (ns1 ? 0u : 1u); ++j)
        for (uint32_t i = 0; i < sizeQ; ++i) {
            li.push_back(i);
            if (j == D0)
                v.push_back(ns % c->q[i]);
        }
    const TwPair* table = nullptr;
    if (fhe_status s = const_tables_trim(c))
        return s;
    std::shared_lock<std::shared_mutex> gate(c->constTabsGate);
    if (fhe_status s = const_table(c, li.data(), v.data(), (uint32_t)v.size(), &table))
        return s;
    g.outB = o.outB, g.outA = o.outA, g.p0 = o.p0, g.p1 = o.p1, g.sOld = o.sOld, g.u = o.u, g.e0 = o.e0, g.e1 = o.e1;
    g.lc = c->d_lc, g.tab = table, g.logN = c->logN, g.nLimbs = sizeQ, g.nParts = D0, g.nKeys = nKeys, g.pkPerKey = pkPerKey ? 1u : 0u;
    const uint32_t pieces = bv_keygen_pk_pieces(c, sizeQ, D0, nKeys);
    g.chunk               = (D0 + pieces - 1) / pieces;
    g.pieces              = (D0 + g.chunk - 1) / g.chunk;
    const uint32_t grid   = nKeys * g.pieces * sizeQ * bv_keygen_tiles(c);
    if (ns1)
        FHE_LAUNCH((keygen_pk_combine_kernel<true>), grid, st, g);
    else
        FHE_LAUNCH((keygen_pk_combine_kernel<false>), grid, st, g);
    LAUNCH_CHECK();
    return FHE_OK;
}
extern "C" fhe_status fhe_bv_keygen_pk(fhe_ctx* c, uint32_t sizeQ, uint32_t baseBits, uint32_t nKeys, const uint64_t* p0, const uint64_t* p1,
                                       int pkPerKey, const uint64_t* sOld, uint64_t ns, const uint64_t* u, const uint64_t* e0,
                                       const uint64_t* e1, uint64_t* devKeyB, uint64_t* devKeyA, void* st) {
    const std::string who = "fhe_bv_keygen_pk";
    uint32_t D0           = 0;
    std::vector<uint64_t> f;
    if (fhe_status s = bv_keygen_shape(who, c, sizeQ, baseBits, &D0, &f))
        return s;
    const BvKeygenPkOperands o{p0, p1, sOld, u, e0, e1, devKeyB, devKeyA};
    if (fhe_status s = bv_keygen_pk_check(who, c, sizeQ, D0, nKeys, pkPerKey, o, ns))
        return s;
    return bv_keygen_pk_run(who, c, sizeQ, D0, f, nKeys, pkPerKey, o, ns, st);
}
extern "C" size_t fhe_bv_keygen_workspace_bytes(const fhe_ctx* c, uint32_t sizeQ, uint32_t baseBits, uint32_t nKeys) {
    if (!c || sizeQ < 1 || sizeQ > c->L)
        return 0;
    return (((size_t)nKeys * fhe_crt_decompose_towers(c, nullptr, sizeQ, baseBits) * sizeQ) << c->logN) * 8;
}
// the seeded public-key form, a composition: u into ws, e0 into devKeyB and e1 into devKeyA from the blake2 samplers, the forward
// transform over all of it, one combine in place.  e1's words start at the block after e0's last one, so that the three blocks may lie
// anywhere: contiguous (devKeyB | devKeyA | ws) they take one Gaussian call and one transform call, apart one call per block, and the
// words are the same.  Every argument is checked before the first launch.
extern "C" fhe_status fhe_bv_keygen_pk_blake2(fhe_ctx* c, uint32_t sizeQ, uint32_t baseBits, uint32_t nKeys, const uint64_t* p0,
                                              const uint64_t* p1, int pkPerKey, const uint64_t* sOld, int uDist, uint64_t ns, double sigma,
                                              const uint32_t key[16], uint64_t counterU, uint64_t counterE, uint64_t* devKeyB,
                                              uint64_t* devKeyA, void* ws, size_t wsBytes, void* st) {
    const std::string who = "fhe_bv_keygen_pk_blake2";
    uint32_t D0           = 0;
    std::vector<uint64_t> f;
    if (fhe_status s = bv_keygen_shape(who, c, sizeQ, baseBits, &D0, &f))
        return s;
    ARG_CHECK(key && ws, who + ": null argument");
    uint64_t* u = (uint64_t*)ws;
    const BvKeygenPkOperands o{p0, p1, sOld, u, devKeyB, devKeyA, devKeyB, devKeyA};
    ARG_CHECK(devKeyB && devKeyA && p0 && p1 && sOld, who + ": null argument");
    ARG_CHECK(nKeys >= 1, who + ": nKeys must be >= 1");
    ARG_CHECK(sigma > 1.000000001 && sigma < 300.0, who + ": the inversion sampler covers 1 < sigma < 300 (the reference's Peikert range)");
    ARG_CHECK(uDist == 0 || uDist == 1, who + ": uDist is 0 (ternary) or 1 (Gaussian)");
    ARG_CHECK(wsBytes >= fhe_bv_keygen_workspace_bytes(c, sizeQ, baseBits, nKeys), who + ": workspace too small");
    const size_t row = (size_t)c->N * 8, words = ((size_t)nKeys * D0 * sizeQ) << c->logN, slab = words * 8;
    ARG_CHECK(!keygen_overlap(u, slab, devKeyB, slab) && !keygen_overlap(u, slab, devKeyA, slab), who + ": the workspace overlaps a key block");
    ARG_CHECK(!keygen_overlap(u, slab, p0, (size_t)(pkPerKey ? nKeys : 1u) * sizeQ * row) &&
                  !keygen_overlap(u, slab, p1, (size_t)(pkPerKey ? nKeys : 1u) * sizeQ * row) && !keygen_overlap(u, slab, sOld, sizeQ * row),
              who + ": the workspace overlaps the public key or sOld");
    if (fhe_status s = bv_keygen_pk_check(who, c, sizeQ, D0, nKeys, pkPerKey, o, ns))
        return s;
    const uint32_t towers  = nKeys * D0;
    const uint64_t coef    = (uint64_t)towers << c->logN, eBlocks = (coef + 511) / 512;
    const bool contiguous  = devKeyA == devKeyB + words && u == devKeyA + words;
    if (fhe_status s = uDist == 0 ? fhe_sample_ternary_blake2(c, u, nullptr, sizeQ, towers, key, counterU, st)
                                  : fhe_sample_gaussian_blake2(c, u, nullptr, sizeQ, towers, sigma, key, counterU, st))
        return s;
    if (contiguous && coef % 512 == 0) {
        if (fhe_status s = fhe_sample_gaussian_blake2(c, devKeyB, nullptr, sizeQ, 2 * towers, sigma, key, counterE, st))
            return s;
    } else {
        if (fhe_status s = fhe_sample_gaussian_blake2(c, devKeyB, nullptr, sizeQ, towers, sigma, key, counterE, st))
            return s;
        if (fhe_status s = fhe_sample_gaussian_blake2(c, devKeyA, nullptr, sizeQ, towers, sigma, key, counterE + eBlocks, st))
            return s;
    }
    if (contiguous) {
        if (fhe_status s = fhe_ntt_fwd(c, devKeyB, nullptr, sizeQ, 3 * towers, st))
            return s;
    } else {
        for (uint64_t* block : {devKeyB, devKeyA, u})
            if (fhe_status s = fhe_ntt_fwd(c, block, nullptr, sizeQ, towers, st))
                return s;
    }
    return bv_keygen_pk_run(who, c, sizeQ, D0, f, nKeys, pkPerKey, o, ns, st);
}

// ---- encryption (encrypt_kernels.h) ----
// PKERNS::EncryptZeroCore in both forms (rns-pke.cpp:111-197) with the `(*ba)[0] += plaintext` of PKERNS::Encrypt (:40-70) for any number
// of ciphertexts: everything that is not sampling or transforming is ONE launch of encrypt_combine_kernel.  ns mod q_i goes through the
// context's table cache (const_table), as the keygen combine's table does.
struct EncryptOperands {
    const uint64_t *k0, *k1;  // pkB, pkA | s, (unused)
    const uint64_t *v, *e0, *e1;  // v, e0, e1 | a, e, (unused)
    const uint64_t* msg;      // EVALUATION message or null
    uint64_t *c0, *c1;
};
static uint32_t encrypt_tiles(const fhe_ctx* c) {
    return c->logN > (uint32_t)kEncryptTileLog ? 1u << (c->logN - kEncryptTileLog) : 1u;
}
// ciphertexts per workgroup: the longest walk that leaves four workgroups (16 waves, four per SIMD) per compute unit
static uint32_t encrypt_chunk_for(const fhe_ctx* c, uint32_t nLimbs, uint32_t batch) {
    return encrypt_chunk((uint64_t)nLimbs * encrypt_tiles(c), batch, 4ull * (c->cus ? c->cus : 256));
}
// the checks every entry of the family shares, before anything is enqueued
static fhe_status encrypt_check_shape(const std::string& who, const fhe_ctx* c, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch,
                                      uint64_t ns) {
    ARG_CHECK(c, who + ": null argument");
    ARG_CHECK(batch >= 1, who + ": batch must be >= 1");
    ARG_CHECK(nLimbs >= 1 && nLimbs <= (uint32_t)kMaxLimbs, who + ": nLimbs out of range");
    for (uint32_t i = 0; i < nLimbs; ++i)
        ARG_CHECK((limbIdx ? limbIdx[i] : i) < c->L, who + ": limb index exceeds context size");
    ARG_CHECK(ns != 0, who + ": the noise scale must not be zero");
    ARG_CHECK((uint64_t)batch * nLimbs * encrypt_tiles(c) < ((uint64_t)1 << 31), who + ": batch * nLimbs too large");
    return FHE_OK;
}
static fhe_status encrypt_check(const std::string& who, const fhe_ctx* c, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch,
                                bool sk, const EncryptOperands& o, uint64_t ns) {
    ARG_CHECK(c && o.k0 && (sk || o.k1) && o.v && o.e0 && (sk || o.e1) && o.c0 && o.c1, who + ": null argument");
    if (fhe_status s = encrypt_check_shape(who, c, limbIdx, nLimbs, batch, ns))
        return s;
    const size_t row = (size_t)c->N * 8, key = nLimbs * row, slab = (size_t)batch * key;
    const uint64_t* in1 = sk ? o.v : o.e1;  // what c1 may be: e1, or a
    ARG_CHECK(!keygen_overlap(o.c0, slab, o.c1, slab), who + ": c0 and c1 overlap");
    ARG_CHECK(o.c0 == o.e0 || !keygen_overlap(o.c0, slab, o.e0, slab),
              who + (sk ? ": c0 may be e itself but not overlap it otherwise" : ": c0 may be e0 itself but not overlap it otherwise"));
    ARG_CHECK(o.c1 == in1 || !keygen_overlap(o.c1, slab, in1, slab),
              who + (sk ? ": c1 may be a itself but not overlap it otherwise" : ": c1 may be e1 itself but not overlap it otherwise"));
    ARG_CHECK(!keygen_overlap(o.c1, slab, o.e0, slab) && !keygen_overlap(o.c0, slab, in1, slab),
              who + (sk ? ": c0 overlaps a or c1 overlaps e" : ": c0 overlaps e1 or c1 overlaps e0"));
    if (!sk)
        ARG_CHECK(!keygen_overlap(o.v, slab, o.e0, slab) && !keygen_overlap(o.v, slab, o.e1, slab) &&
                      !keygen_overlap(o.v, slab, o.c0, slab) && !keygen_overlap(o.v, slab, o.c1, slab),
                  who + ": v overlaps e0, e1 or an output");
    for (const uint64_t* out : {o.c0, o.c1}) {
        ARG_CHECK(!keygen_overlap(out, slab, o.k0, key) && !(!sk && keygen_overlap(out, slab, o.k1, key)),
                  who + (sk ? ": an output overlaps s" : ": an output overlaps the public key"));
        ARG_CHECK(!(o.msg && keygen_overlap(out, slab, o.msg, slab)), who + ": an output overlaps msg");
    }
    return FHE_OK;
}
// (the arguments have passed encrypt_check)
static fhe_status encrypt_combine_run(const std::string& who, fhe_ctx* c, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, bool sk,
                                      const EncryptOperands& o, uint64_t ns, void* st) {
    EncryptArgs g;
    if (fhe_status s = make_sel(c, limbIdx, nLimbs, &g.sel, who.c_str()))
        return s;
    RT_CHECK(rt::set_device(c->device));
    std::vector<uint32_t> li;
    std::vector<uint64_t> v;
    bool ns1 = true;  // ns = 1 modulo every limb in use (q_i > 1): no product at all
    for (uint32_t i = 0; i < nLimbs; ++i) {
        const uint32_t l = limbIdx ? limbIdx[i] : i;
        li.push_back(l);
        v.push_back(ns % c->q[l]);
        ns1 = ns1 && v.back() == 1;
    }
    const TwPair* table = nullptr;
    if (fhe_status s = const_tables_trim(c))
        return s;
    std::shared_lock<std::shared_mutex> gate(c->constTabsGate);
    if (!ns1)
        if (fhe_status s = const_table(c, li.data(), v.data(), (uint32_t)v.size(), &table))
            return s;
    g.c0 = o.c0, g.c1 = o.c1, g.k0 = o.k0, g.k1 = sk ? o.k0 : o.k1, g.v = o.v, g.e0 = o.e0, g.e1 = sk ? o.e0 : o.e1, g.msg = o.msg;
    g.lc = c->d_lc, g.tab = table, g.logN = c->logN, g.nLimbs = nLimbs, g.batch = batch;
    g.chunk             = encrypt_chunk_for(c, nLimbs, batch);
    const uint32_t grid = ((batch + g.chunk - 1) / g.chunk) * nLimbs * encrypt_tiles(c);
#define ENCRYPT_LAUNCH(NS1, MSG)                                                   \
    do {                                                                           \
        if (sk)                                                                    \
            FHE_LAUNCH((encrypt_combine_kernel<NS1, MSG, true>), grid, st, g);     \
        else                                                                       \
            FHE_LAUNCH((encrypt_combine_kernel<NS1, MSG, false>), grid, st, g);    \
    } while (0)
    if (ns1 && o.msg)
        ENCRYPT_LAUNCH(true, true);
    else if (ns1)
        ENCRYPT_LAUNCH(true, false);
    else if (o.msg)
        ENCRYPT_LAUNCH(false, true);
    else
        ENCRYPT_LAUNCH(false, false);
#undef ENCRYPT_LAUNCH
    LAUNCH_CHECK();
    return FHE_OK;
}
extern "C" uint32_t fhe_encrypt_chunk(const fhe_ctx* c, uint32_t nLimbs, uint32_t batch) {
    return c && nLimbs && batch ? encrypt_chunk_for(c, nLimbs, batch) : 0;
}
extern "C" fhe_status fhe_encrypt_pk_combine(fhe_ctx* c, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, const uint64_t* pkB,
                                             const uint64_t* pkA, const uint64_t* v, const uint64_t* e0, const uint64_t* e1,
                                             const uint64_t* msg, uint64_t ns, uint64_t* c0, uint64_t* c1, void* st) {
    const std::string who = "fhe_encrypt_pk_combine";
    const EncryptOperands o{pkB, pkA, v, e0, e1, msg, c0, c1};
    if (fhe_status s = encrypt_check(who, c, limbIdx, nLimbs, batch, false, o, ns))
        return s;
    return encrypt_combine_run(who, c, limbIdx, nLimbs, batch, false, o, ns, st);
}
extern "C" fhe_status fhe_encrypt_sk_combine(fhe_ctx* c, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, const uint64_t* s,
                                             const uint64_t* a, const uint64_t* e, const uint64_t* msg, uint64_t ns, uint64_t* c0,
                                             uint64_t* c1, void* st) {
    const std::string who = "fhe_encrypt_sk_combine";
    const EncryptOperands o{s, nullptr, a, e, nullptr, msg, c0, c1};
    if (fhe_status r = encrypt_check(who, c, limbIdx, nLimbs, batch, true, o, ns))
        return r;
    return encrypt_combine_run(who, c, limbIdx, nLimbs, batch, true, o, ns, st);
}
extern "C" size_t fhe_encrypt_workspace_bytes(const fhe_ctx* c, uint32_t nLimbs, uint32_t batch) {
    return c ? (((size_t)batch * nLimbs) << c->logN) * 8 : 0;
}
extern "C" fhe_status fhe_encrypt_counters(const fhe_ctx* c, uint32_t nLimbs, uint32_t batch, int form, uint64_t* nVorA, uint64_t* nE) {
    ARG_CHECK(c && nVorA && nE, "fhe_encrypt_counters: null argument");
    ARG_CHECK(batch >= 1 && nLimbs >= 1, "fhe_encrypt_counters: batch and nLimbs must be >= 1");
    ARG_CHECK(form == 0 || form == 1, "fhe_encrypt_counters: form is 0 (public key) or 1 (secret key)");
    const uint64_t coef = (uint64_t)batch << c->logN;
    if (form == 0) {
        *nVorA = (coef + 511) / 512;      // one word per coefficient of v
        *nE    = (2 * coef + 511) / 512;  // e0 || e1: ONE sampler call over 2 * batch towers
    } else {
        *nVorA = (coef * nLimbs + 255) / 256;  // two 64-bit words per uniform residue
        *nE    = (coef + 511) / 512;
    }
    return FHE_OK;
}
// what the two seeded forms check alike
static fhe_status encrypt_check_seeded(const std::string& who, const fhe_ctx* c, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch,
                                       uint64_t ns, double sigma, const uint32_t* key, const uint64_t* msg, int msgFormat) {
    ARG_CHECK(key, who + ": null argument");
    if (fhe_status s = encrypt_check_shape(who, c, limbIdx, nLimbs, batch, ns))
        return s;
    ARG_CHECK(sigma > 1.000000001 && sigma < 300.0, who + ": the inversion sampler covers 1 < sigma < 300 (the reference's Peikert range)");
    ARG_CHECK(msgFormat == 0 || msgFormat == 1, who + ": msgFormat is 0 (EVALUATION) or 1 (COEFFICIENT)");
    if (msg && msgFormat == 1)
        for (uint32_t i = 0; i < nLimbs; ++i)
            ARG_CHECK(ns % c->q[limbIdx ? limbIdx[i] : i] == 1,
                      who + ": a COEFFICIENT message joins e before the noise scale is applied: ns must be 1 modulo every limb");
    return FHE_OK;
}
// the seeded public-key form, a composition: v and e0 || e1 from the blake2 samplers, one forward transform when the workspace follows
// ct (two otherwise), one combine in place.  Every argument is checked before the first launch.
extern "C" fhe_status fhe_encrypt_pk_blake2(fhe_ctx* c, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, const uint64_t* pkB,
                                            const uint64_t* pkA, int vDist, uint64_t ns, double sigma, const uint32_t key[16],
                                            uint64_t counterV, uint64_t counterE, const uint64_t* msg, int msgFormat, uint64_t* ct,
                                            void* ws, size_t wsBytes, void* st) {
    const std::string who = "fhe_encrypt_pk_blake2";
    ARG_CHECK(c && pkB && pkA && ct && ws, who + ": null argument");
    if (fhe_status s = encrypt_check_seeded(who, c, limbIdx, nLimbs, batch, ns, sigma, key, msg, msgFormat))
        return s;
    ARG_CHECK(vDist == 0 || vDist == 1, who + ": vDist is 0 (ternary) or 1 (Gaussian)");
    const size_t words = ((size_t)batch * nLimbs) << c->logN, slab = words * 8, keyBytes = ((size_t)nLimbs << c->logN) * 8;
    ARG_CHECK(wsBytes >= fhe_encrypt_workspace_bytes(c, nLimbs, batch), who + ": workspace too small");
    uint64_t* v = (uint64_t*)ws;
    ARG_CHECK(!keygen_overlap(v, slab, ct, 2 * slab), who + ": the workspace overlaps ct");
    ARG_CHECK(!keygen_overlap(v, slab, pkB, keyBytes) && !keygen_overlap(v, slab, pkA, keyBytes) && !(msg && keygen_overlap(v, slab, msg, slab)),
              who + ": the workspace overlaps the public key or msg");
    const uint64_t* evalMsg = msg && msgFormat == 0 ? msg : nullptr;
    const EncryptOperands o{pkB, pkA, v, ct, ct + words, msg, ct, ct + words};  // (msg, whatever its format, must stay clear of ct)
    if (fhe_status s = encrypt_check(who, c, limbIdx, nLimbs, batch, false, o, ns))
        return s;
    if (fhe_status s = vDist == 0 ? fhe_sample_ternary_blake2(c, v, limbIdx, nLimbs, batch, key, counterV, st)
                                  : fhe_sample_gaussian_blake2(c, v, limbIdx, nLimbs, batch, sigma, key, counterV, st))
        return s;
    if (fhe_status s = fhe_sample_gaussian_blake2(c, ct, limbIdx, nLimbs, 2 * batch, sigma, key, counterE, st))
        return s;
    if (msg && msgFormat == 1)
        if (fhe_status s = fhe_add(c, ct, ct, msg, limbIdx, nLimbs, batch, st))
            return s;
    if (v == ct + 2 * words) {
        if (fhe_status s = fhe_ntt_fwd(c, ct, limbIdx, nLimbs, 3 * batch, st))
            return s;
    } else {
        if (fhe_status s = fhe_ntt_fwd(c, ct, limbIdx, nLimbs, 2 * batch, st))
            return s;
        if (fhe_status s = fhe_ntt_fwd(c, v, limbIdx, nLimbs, batch, st))
            return s;
    }
    EncryptOperands run = o;
    run.msg             = evalMsg;
    return encrypt_combine_run(who, c, limbIdx, nLimbs, batch, false, run, ns, st);
}
// the seeded secret-key form: a = the uniform sampler's words in the c1 block, used as drawn (the reference draws a in EVALUATION format);
// e = the Gaussian sampler's words in the c0 block, transformed there; one combine in place.  No workspace.
extern "C" fhe_status fhe_encrypt_sk_blake2(fhe_ctx* c, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, const uint64_t* sKey,
                                            uint64_t ns, double sigma, const uint32_t key[16], uint64_t counterA, uint64_t counterE,
                                            const uint64_t* msg, int msgFormat, uint64_t* ct, void* st) {
    const std::string who = "fhe_encrypt_sk_blake2";
    ARG_CHECK(c && sKey && ct, who + ": null argument");
    if (fhe_status s = encrypt_check_seeded(who, c, limbIdx, nLimbs, batch, ns, sigma, key, msg, msgFormat))
        return s;
    const size_t words = ((size_t)batch * nLimbs) << c->logN;
    const EncryptOperands o{sKey, nullptr, ct + words, ct, nullptr, msg, ct, ct + words};
    if (fhe_status s = encrypt_check(who, c, limbIdx, nLimbs, batch, true, o, ns))
        return s;
    if (fhe_status s = fhe_sample_uniform_blake2(c, ct + words, limbIdx, nLimbs, batch, key, counterA, st))
        return s;
    if (fhe_status s = fhe_sample_gaussian_blake2(c, ct, limbIdx, nLimbs, batch, sigma, key, counterE, st))
        return s;
    if (msg && msgFormat == 1)
        if (fhe_status s = fhe_add(c, ct, ct, msg, limbIdx, nLimbs, batch, st))
            return s;
    if (fhe_status s = fhe_ntt_fwd(c, ct, limbIdx, nLimbs, batch, st))
        return s;
    EncryptOperands run = o;
    run.msg             = msg && msgFormat == 0 ? msg : nullptr;
    return encrypt_combine_run(who, c, limbIdx, nLimbs, batch, true, run, ns, st);
}

// ---- BSGS plaintext-matrix product with double hoisting ----
// FHECKKSRNS::EvalLinearTransform (ckksrns-fhe.cpp:1832-1882) and one level of EvalCoeffsToSlots / EvalSlotsToCoeffs
// (:1884-2198).  The reference walks the outer (giant) steps one after the other; here every stage runs ONCE over all
// outer steps (the accumulations `first += ...` and `outer += ...` are exact modular sums, so their order is free):
//   1. rot_j      inner rotations on one digit decomposition of c1, kept in the extended basis: the inner products with all
//                 rotation keys (+ c0 * P) in one launch, the digits read once; stored BEFORE the automorphism
//   2. inner_i    all outer steps' multiply-accumulate sums in one pass over the rot_j, each read through its rotation's
//                 index map (the automorphism is this kernel's gather)                               (1 kernel)
//   3. d_i        KeySwitchDown of every inner_i as one batch of 2*nOut*batch towers                (INTT, conversion, NTT)
//   4. first      sum_i Automorphism_{k_i}(d_i[0])                                                   (1 kernel)
//   5. digits     ModUp of every rotated step's d_i[1] as one batch                                  (INTT, conversions, NTTs)
//   6. e_i        inner product with the outer step's own key                                        (1 kernel per rotated step)
//   7. outer      sum_i Automorphism_{k_i}(e_i)  (+ inner_i[1] of the unrotated steps)               (2 kernels)
//   8. result     KeySwitchDown(outer), result[0] += first
// workspace = [key-switch layout for batch*nOut towers][rot: nIn x 2 x batch ext][inner: 2 x nOut x batch ext]
//             [d: 2 x nOut x batch Q_l][outer: 2 x batch ext][first: batch Q_l]
struct BsgsLayout {
    size_t ksTotal, rot, inner, d, outer, first, total;
};
static BsgsLayout bsgs_layout(const fhe_ks_plan* p, uint32_t sizeQl, uint32_t batch, uint32_t nIn, uint32_t nOut) {
    BsgsLayout b{};
    b.ksTotal        = ks_layout(p, sizeQl, batch * nOut).total;
    const size_t N   = (size_t)1 << p->ctx->logN;
    const size_t ext = (size_t)batch * (sizeQl + p->sizeP) * N, low = (size_t)batch * sizeQl * N;
    size_t off       = b.ksTotal;
    b.rot = off, off += (size_t)nIn * 2 * ext;
    b.inner = off, off += (size_t)nOut * 2 * ext;
    b.d = off, off += (size_t)nOut * 2 * low;
    b.outer = off, off += 2 * ext;
    b.first = off, off += low;
    b.total = off;
    return b;
}
extern "C" size_t fhe_ckks_bsgs_workspace_bytes(const fhe_ks_plan* p, uint32_t sizeQl, uint32_t batch, uint32_t nIn,
                                                uint32_t nOut) {
    if (!p || sizeQl < 1 || sizeQl > p->sizeQ || batch < 1 || nIn < 1 || nOut < 1)
        return 0;
    return bsgs_layout(p, sizeQl, batch, nIn, nOut).total * 8;
}
// KeySwitchDown of two adjacent extended towers x[2*batch] -> out0, out1 (keyswitch-hybrid.cpp:245-278); out1 == nullptr:
// all nTow towers go to out0 (one batch of ApproxModDown calls)
static fhe_status mod_down_many(fhe_ks_plan* p, fhe_ks_plan::Level* lv, const uint64_t* x, uint32_t nTow, uint32_t split,
                                uint64_t* out0, uint64_t* out1, uint64_t* pcoef, uint64_t* md, void* st) {
    fhe_ctx* c = p->ctx;
    if (ntt_epilogue_supported(c)) {
        NttEpilogue epi;
        epi.mode = 1u, epi.split = split, epi.aStride = lv->sizeQl + p->sizeP, epi.aFirst = 0;
        epi.A = x, epi.C = lv->d_PInv, epi.out0 = out0, epi.out1 = out1 ? out1 : out0;
        return mod_down_core(p, lv, x, nTow, pcoef, md, st, nullptr, &epi);
    }
    if (fhe_status s = mod_down_core(p, lv, x, nTow, pcoef, md, st))
        return s;
    if (fhe_status s = mod_down_tail(p, lv, x, md, split, out0, false, st))
        return s;
    if (split == nTow)
        return FHE_OK;
    const size_t ext = ((size_t)split * (lv->sizeQl + p->sizeP)) << c->logN, low = ((size_t)split * lv->sizeQl) << c->logN;
    return mod_down_tail(p, lv, x + ext, md + low, nTow - split, out1, false, st);
}
// out (+)= sum_s Automorphism_{k_s}(in_s) over towers of `nl` limbs
static fhe_status automorph_sum_run(fhe_ctx* c, uint64_t* out, const std::vector<const uint64_t*>& in, const std::vector<uint32_t>& k,
                                    const uint32_t* li, uint32_t nl, uint32_t bt, void* st) {
    for (size_t s0 = 0; s0 < in.size(); s0 += kMaxAutoSum) {
        AutoSumArgs g;
        if (fhe_status s = make_sel(c, li, nl, &g.sel, "automorphism"))
            return s;
        g.nSrc = (uint32_t)std::min<size_t>(kMaxAutoSum, in.size() - s0);
        for (uint32_t s = 0; s < (uint32_t)kMaxAutoSum; ++s) {
            g.in[s] = s < g.nSrc ? in[s0 + s] : nullptr;
            g.k[s]  = s < g.nSrc ? k[s0 + s] : 1u;
        }
        g.out = out, g.q = c->d_q, g.logN = c->logN, g.nLimbs = nl, g.rows = bt * nl, g.accumulate = s0 ? 1u : 0u;
        FHE_LAUNCH(automorph_sum_kernel, tiles_for(c, g.rows), st, g);
        LAUNCH_CHECK();
    }
    return FHE_OK;
}
extern "C" fhe_status fhe_ckks_bsgs_transform(fhe_ks_plan* p, const uint64_t* c0, const uint64_t* c1, uint32_t sizeQl,
                                              uint32_t batch, uint32_t nIn, const uint32_t* inK,
                                              const fhe_ks_key* const* inKeys, uint32_t nOut, const uint32_t* outK,
                                              const fhe_ks_key* const* outKeys, const uint64_t* const* diag, uint64_t* out0,
                                              uint64_t* out1, void* wsv, size_t wsBytes, void* st) {
    ARG_CHECK(p && c0 && c1 && inK && outK && diag && out0 && out1 && wsv, "fhe_ckks_bsgs_transform: null argument");
    ARG_CHECK(sizeQl >= 1 && sizeQl <= p->sizeQ && batch >= 1, "fhe_ckks_bsgs_transform: bad level or batch");
    ARG_CHECK(nIn >= 1 && nOut >= 1, "fhe_ckks_bsgs_transform: needs at least one inner and one outer step");
    const BsgsLayout L = bsgs_layout(p, sizeQl, batch, nIn, nOut);
    ARG_CHECK(wsBytes >= L.total * 8, "fhe_ckks_bsgs_transform: workspace too small");
    for (uint32_t j = 0; j < nIn; ++j) {
        ARG_CHECK(inK[j] == 0 || inK[j] % 2 == 1, "Automorphism index not odd");
        ARG_CHECK(inK[j] == 0 || (inKeys && inKeys[j] && inKeys[j]->plan == p), "fhe_ckks_bsgs_transform: missing inner rotation key");
    }
    for (uint32_t i = 0; i < nOut; ++i) {
        ARG_CHECK(outK[i] == 0 || outK[i] % 2 == 1, "Automorphism index not odd");
        ARG_CHECK(outK[i] == 0 || (outKeys && outKeys[i] && outKeys[i]->plan == p), "fhe_ckks_bsgs_transform: missing outer rotation key");
    }
    fhe_ctx* c = p->ctx;
    RT_CHECK(rt::set_device(c->device));
    fhe_ks_plan::Level* lv = nullptr;
    if (fhe_status s = ks_level(p, sizeQl, &lv))
        return s;
    uint64_t* ws           = (uint64_t*)wsv;
    const uint32_t sizeQlP = sizeQl + p->sizeP;
    const size_t ext = ((size_t)batch * sizeQlP) << c->logN, low = ((size_t)batch * sizeQl) << c->logN;
    uint64_t *rot = ws + L.rot, *inner = ws + L.inner, *outer = ws + L.outer, *d = ws + L.d, *first = ws + L.first;
    std::vector<uint32_t> extIdx;
    ext_limbs(p, sizeQl, extIdx);
    TwPair* dP = nullptr;
    if (fhe_status s = ks_pmodq(p, lv, &dP))
        return s;
    // outer steps without a rotation first, the rotated ones behind them (slices of one batch from stage 3 on)
    std::vector<uint32_t> perm;
    for (uint32_t i = 0; i < nOut; ++i)
        if (outK[i] == 0)
            perm.push_back(i);
    const uint32_t nZ = (uint32_t)perm.size(), nR = nOut - nZ;
    for (uint32_t i = 0; i < nOut; ++i)
        if (outK[i] != 0)
            perm.push_back(i);
    // the diagonals' pointer table on the device: outer steps permuted, rows padded to the kernel's unroll width, absent
    // terms and padding pointing at rows of zeros (cached by content: the same transform is applied many times)
    const uint32_t ninK   = nIn <= 4 ? 4u : nIn <= 8 ? 8u : (uint32_t)kMaxBsgsIn;  // kernel instance (NIN)
    const uint32_t nInPad = (nIn + ninK - 1) / ninK * ninK;
    std::unique_lock<std::mutex> bsgsLock(p->cacheMutex);
    if (!p->d_zeroRows) {
        void* dz = nullptr;
        const size_t bytes = ((size_t)(p->sizeQ + p->sizeP) << c->logN) * 8;
        RT_CHECK(rt::dmalloc(&dz, bytes));
        p->owned.push_back(dz);
        RT_CHECK(rt::dzero_2d(dz, bytes, bytes, 1, nullptr));
        RT_CHECK(rt::sync(nullptr));
        p->d_zeroRows = (uint64_t*)dz;
    }
    std::vector<uint64_t> tab((size_t)nOut * nInPad, (uint64_t)(uintptr_t)p->d_zeroRows);
    for (uint32_t i = 0; i < nOut; ++i)
        for (uint32_t j = 0; j < nIn; ++j)
            if (diag[(size_t)perm[i] * nIn + j])
                tab[(size_t)i * nInPad + j] = (uint64_t)(uintptr_t)diag[(size_t)perm[i] * nIn + j];
    auto it = p->bsgsTables.find(tab);
    if (it == p->bsgsTables.end()) {
        if (p->bsgsTables.size() >= 64) {  // a caller that keeps re-allocating its diagonals: drop the stale tables
            RT_CHECK(rt::device_sync());   // (a launch on ANY stream may still read one of them)
            for (auto& kv : p->bsgsTables)
                rt::dfree(kv.second);
            p->bsgsTables.clear();
        }
        uint64_t* dp = nullptr;
        if (fhe_status s = dev_copy(nullptr, tab.data(), tab.size(), &dp))  // (no owner list: the map owns its entries)
            return s;
        it = p->bsgsTables.emplace(tab, dp).first;
    }
    const uint64_t* const* dTab = (const uint64_t* const*)it->second;
    bsgsLock.unlock();

    // 1. inner (baby-step) rotations: one digit decomposition of c1 serves all of them (EvalFastRotationPrecompute, :1842), and ONE
    //    launch computes EvalFastKeySwitchCoreExt + `cTilda[0] += c0 * P` (EvalFastRotationExt(ct, index, digits, addFirst = true)) for all
    //    of them.  rot_j keeps the result BEFORE the rotation's AutomorphismTransform: stage 2 reads it through the index map
    const KsLayout wB = ks_layout(p, sizeQl, batch);
    {
        std::vector<const fhe_ks_key*> keys;
        std::vector<uint64_t*> e0, e1;
        for (uint32_t j = 0; j < nIn; ++j) {
            uint64_t* rj = rot + (size_t)j * 2 * ext;
            if (inK[j] == 0) {  // KeySwitchExt(ct, true)
                if (fhe_status s = fhe_ks_ext(p, c0, sizeQl, batch, rj, st))
                    return s;
                if (fhe_status s = fhe_ks_ext(p, c1, sizeQl, batch, rj + ext, st))
                    return s;
                continue;
            }
            keys.push_back(inKeys[j]), e0.push_back(rj), e1.push_back(rj + ext);
        }
        if (!keys.empty()) {
            if (fhe_status s = ks_precompute_run(p, lv, c1, batch, ws, wB, st))
                return s;
            if (fhe_status s = ks_inner_multi_run(p, lv, keys.data(), (uint32_t)keys.size(), c1, batch, e0.data(), e1.data(), c0, dP, ws,
                                                  wB, st))
                return s;
        }
    }
    // 2. inner_i = sum_j rot_j * diag[i][j] for every outer step: inner is [2][nOut][batch] extended towers
    for (uint32_t j0 = 0; j0 < nIn; j0 += ninK) {
        BsgsInnerArgs g;
        g.nIn = std::min<uint32_t>(ninK, nIn - j0), g.nInPad = nInPad, g.j0 = j0, g.nOut = nOut;
        g.rot = rot + (size_t)j0 * 2 * ext, g.diag = dTab, g.out = inner, g.lc = c->d_lc, g.mu128 = c->d_mu128;
        g.logN = c->logN, g.batch = batch, g.sizeQl = sizeQl, g.sizeQ = p->sizeQ, g.sizeP = p->sizeP;
        g.accumulate = j0 ? 1u : 0u;
        for (uint32_t j = 0; j < (uint32_t)kMaxBsgsIn; ++j)
            g.k[j] = (j < g.nIn && inK[j0 + j]) ? inK[j0 + j] : 1u;
        const uint32_t tilesPerRow = c->N >= (uint32_t)kTile ? (c->N >> kTileLog) : 1u;
        const uint64_t nGroups = (uint64_t)sizeQlP * tilesPerRow, grid = ((nGroups + 7) / 8) * 8 * 2 * batch;
        static const uint32_t cpl = env_u32("FHE_BSGS_CPL", 2);  // coefficients per lane of the 4- and 8-term instances
        if (ninK == 4 && cpl == 2 && c->N >= 2)
            FHE_LAUNCH((bsgs_inner_kernel<4, 2>), grid, st, g);
        else if (ninK == 4)
            FHE_LAUNCH((bsgs_inner_kernel<4, 1>), grid, st, g);
        else if (ninK == 8 && cpl == 2 && c->N >= 2)
            FHE_LAUNCH((bsgs_inner_kernel<8, 2>), grid, st, g);
        else if (ninK == 8)
            FHE_LAUNCH((bsgs_inner_kernel<8, 1>), grid, st, g);
        else
            FHE_LAUNCH((bsgs_inner_kernel<16, 1>), grid, st, g);
        LAUNCH_CHECK();
    }
    // 3. KeySwitchDown of every inner_i (KeySwitchDownFirstElement for the unrotated steps: their second element is only
    //    needed in the extended basis): element-0 towers of all steps, and element-1 towers when any step is rotated
    const KsLayout wM   = ks_layout(p, sizeQl, batch * nOut);
    const uint32_t nTow = (nR ? 2u : 1u) * nOut * batch;
    if (fhe_status s = mod_down_many(p, lv, inner, nTow, nTow, d, nullptr, ws + wM.pcoef, ws + wM.md, st))
        return s;
    // 4. first = sum_i Automorphism_{k_i}(d_i[0])      (:1861, 1873, 1976)
    {
        std::vector<const uint64_t*> src(nOut);
        std::vector<uint32_t> ks(nOut);
        for (uint32_t i = 0; i < nOut; ++i)
            src[i] = d + (size_t)i * low, ks[i] = outK[perm[i]] ? outK[perm[i]] : 1u;
        if (fhe_status s = automorph_sum_run(c, first, src, ks, nullptr, sizeQl, batch, st))
            return s;
    }
    // 5.-7. outer = sum over the rotated steps of EvalFastRotationExt(d_i, k_i, digits(d_i[1]), addFirst = false)
    //       (+ inner_i[1] of the unrotated steps in the second element)           (:1875-1876, 1863-1866, 1977-1979)
    std::vector<const uint64_t*> src0, src1;
    std::vector<uint32_t> k0, k1;
    for (uint32_t i = 0; i < nZ; ++i)
        src1.push_back(inner + (size_t)(nOut + i) * ext), k1.push_back(1u);
    if (nR) {
        const KsLayout wR  = ks_layout(p, sizeQl, batch * nR);
        const uint64_t* dR = d + (size_t)(nOut + nZ) * low;  // second elements of the rotated steps: nR*batch towers
        if (fhe_status s = ks_precompute_run(p, lv, dR, batch * nR, ws, wR, st))
            return s;
        for (uint32_t i = 0; i < nR; ++i) {
            uint64_t *e0 = ws + wR.e0 + (size_t)i * ext, *e1 = ws + wR.e1 + (size_t)i * ext;
            if (fhe_status s = ks_inner_run(p, lv, outKeys[perm[nZ + i]], dR, batch, e0, e1, ws, wR, st, i * batch))
                return s;
            src0.push_back(e0), src1.push_back(e1);
            k0.push_back(outK[perm[nZ + i]]), k1.push_back(outK[perm[nZ + i]]);
        }
        if (fhe_status s = automorph_sum_run(c, outer, src0, k0, extIdx.data(), sizeQlP, batch, st))
            return s;
    }
    else if (fhe_status s = zero_rows(c, outer, sizeQlP, 0, sizeQlP, batch, st))
        return s;
    if (fhe_status s = automorph_sum_run(c, outer + ext, src1, k1, extIdx.data(), sizeQlP, batch, st))
        return s;
    // 8. result = KeySwitchDown(outer); result[0] += first  (:1879-1880)
    if (fhe_status s = mod_down_many(p, lv, outer, 2 * batch, batch, out0, out1, ws + wB.pcoef, ws + wB.md, st))
        return s;
    return elem_run<OP_ADD>(c, out0, out0, first, nullptr, nullptr, sizeQl, batch, st, "fhe_ckks_bsgs_transform");
}

extern "C" fhe_status fhe_approx_mod_down(fhe_ks_plan* p, const uint64_t* x, uint32_t sizeQl, uint32_t batch,
                                          uint64_t* out, void* wsv, size_t wsBytes, void* st) {
    ARG_CHECK(p && x && out && wsv, "fhe_approx_mod_down: null argument");
    ARG_CHECK(sizeQl >= 1 && sizeQl <= p->sizeQ && batch >= 1, "fhe_approx_mod_down: bad level or batch");
    const KsLayout w = ks_layout(p, sizeQl, batch);
    ARG_CHECK(wsBytes >= w.total * 8, "fhe_approx_mod_down: workspace too small");
    RT_CHECK(rt::set_device(p->ctx->device));
    fhe_ks_plan::Level* lv = nullptr;
    if (fhe_status s = ks_level(p, sizeQl, &lv))
        return s;
    uint64_t* ws = (uint64_t*)wsv;
    return mod_down_run(p, lv, x, batch, out, ws + w.pcoef, ws + w.md, st);
}

// ApproxModDown with the BGV plaintext-modulus factors (dcrtpoly-impl.h:966-1005 with t > 0): the P part is multiplied
// by t^-1 mod p_j before the conversion (:981-983) and the converted part by t mod q_i after it (:996-998).  Both
// are constant multiplications of canonical residues, so they are folded into the conversion's two constant sets
// (y_j = x_j * [t^-1 * Phat_j^-1]_{p_j};  out_i = sum_j y_j * [t * Phat_j]_{q_i}): same words, no extra pass.
extern "C" fhe_status fhe_approx_mod_down_bgv(fhe_ks_plan* p, const uint64_t* x, uint32_t sizeQl, uint64_t t, uint32_t batch,
                                              uint64_t* out, void* wsv, size_t wsBytes, void* st) {
    ARG_CHECK(p && x && out && wsv, "fhe_approx_mod_down_bgv: null argument");
    ARG_CHECK(sizeQl >= 1 && sizeQl <= p->sizeQ && batch >= 1, "fhe_approx_mod_down_bgv: bad level or batch");
    ARG_CHECK(t >= 2, "fhe_approx_mod_down_bgv: t must be at least 2");
    const KsLayout w = ks_layout(p, sizeQl, batch);
    ARG_CHECK(wsBytes >= w.total * 8, "fhe_approx_mod_down_bgv: workspace too small");
    fhe_ctx* c = p->ctx;
    RT_CHECK(rt::set_device(c->device));
    fhe_ks_plan::Level* lv = nullptr;
    if (fhe_status s = ks_level(p, sizeQl, &lv))
        return s;
    fhe_conv* downT = nullptr;
    if (fhe_status s = ks_down_conv(p, lv, t, "fhe_approx_mod_down_bgv", &downT))
        return s;
    uint64_t* ws = (uint64_t*)wsv;
    if (fhe_status s = mod_down_core(p, lv, x, batch, ws + w.pcoef, ws + w.md, st, downT))
        return s;
    return mod_down_tail(p, lv, x, ws + w.md, batch, out, false, st);
}

// ------------------------------------------------------------------------------------------------
// dropping the last limbs of a tower: CKKS rescale, BGV ModReduce, CKKS rescale by several limbs
// ------------------------------------------------------------------------------------------------
// One operation, three members: INTT the dropped limb(s), switch them into every kept limb on the way into the forward transform, store
// (x - r) * C on the way out.  Everything below shares one set of argument checks (drop_check), one derivation of each table set
// (host_math.h), one runner for a single dropped limb (drop_last_run) and one place that sets up the fused store (drop_fused_store).
//
// When the fused form may replace the member's own steps is a property of the tables, decided once per call by the entry:
//   * a single CKKS limb fuses for ANY pair with A == -B (host::negated_pair): x*B + r*A is then (x - r)*B whatever B is, so the fused
//     store computes exactly what the caller's tables say;
//   * several CKKS limbs in one pass need, at every step, the negated pair of the TRUE inverses (host::true_inverses as well): the chain
//     kernel, the load's weights and the store's constant are products of q_l^-1 that the library forms itself (host::rescale_multi_tables),
//     so the caller's values enter the fused form not at all;
//   * BGV needs the true inverses of distinct moduli and the true negtInvModq: the fused form multiplies by t^-1 mod q_l and t mod q_i where
//     the member multiplies by negtInvModq and t, which is the same residue only for the values the library would derive itself.
// Any other tables run the member's formula with the given values, launch by launch.  FHE_RESCALE_UNFUSED / FHE_MOD_REDUCE_UNFUSED (read
// once per process) force that form for the CKKS / BGV entries.
static bool rescale_unfused() {
    static const bool v = env_u32("FHE_RESCALE_UNFUSED", 0) != 0;
    return v;
}
static bool mod_reduce_unfused() {
    static const bool v = env_u32("FHE_MOD_REDUCE_UNFUSED", 0) != 0;
    return v;
}
extern "C" size_t fhe_rescale_workspace_bytes(const fhe_ctx* c, uint32_t sizeQl, uint32_t batch) {
    if (!c || sizeQl < 2)
        return 0;
    // last[batch][1][N] + tmp[batch][sizeQl-1][N]
    return ((size_t)batch * sizeQl << c->logN) * 8;
}
// A caller that keeps inventing constants (weighted sums with ever new weights) must not grow the cache without bound: an entry point
// calls this BEFORE it asks for its tables; past the bound every table goes (after a device-wide wait: a launch on any stream may
// still read one) and the cache refills with what is in use.
constexpr size_t kMaxConstTabs = 8192;
static fhe_status const_tables_trim(fhe_ctx* c) {
    {
        std::lock_guard<std::mutex> lock(c->cacheMutex);
        if (c->constTabs.size() < kMaxConstTabs)
            return FHE_OK;
    }
    std::unique_lock<std::shared_mutex> gate(c->constTabsGate);  // (no entry point holds a table it has not launched with yet)
    std::lock_guard<std::mutex> lock(c->cacheMutex);
    RT_CHECK(rt::device_sync());
    for (auto& kv : c->constTabs)
        rt::dfree(kv.second);
    c->constTabs.clear();
    return FHE_OK;
}
// device copy of per-limb constants {v[i], Shoup(v[i], q[limb_i])}, cached by content (the caller's tables of one level)
static fhe_status const_table(fhe_ctx* c, const uint32_t* limbIdx, const uint64_t* v, uint32_t n, const TwPair** out) {
    std::vector<uint64_t> key(2 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i)
        key[i] = limbIdx ? limbIdx[i] : i, key[n + i] = v[i];
    std::lock_guard<std::mutex> lock(c->cacheMutex);
    auto it = c->constTabs.find(key);
    if (it == c->constTabs.end()) {
        std::vector<TwPair> h(n);
        for (uint32_t i = 0; i < n; ++i) {
            const uint64_t qi = c->q[key[i]];
            if (v[i] >= qi)
                return fail(FHE_ERR_ARG, "const_table: constant is not reduced modulo its limb");
            h[i] = TwPair{v[i], host::shoup(v[i], qi)};
        }
        TwPair* d = nullptr;
        if (fhe_status s = dev_copy(nullptr, h.data(), n, &d))  // (no owner list: the map owns its entries)
            return s;
        it = c->constTabs.emplace(std::move(key), d).first;
    }
    *out = it->second;
    return FHE_OK;
}
// the moduli of a tower over context limbs limbIdx[0..n) (null: the leading ones)
static std::vector<uint64_t> tower_moduli(const fhe_ctx* c, const uint32_t* limbIdx, uint32_t n) {
    std::vector<uint64_t> qs(n);
    for (uint32_t i = 0; i < n; ++i)
        qs[i] = c->q[limbIdx ? limbIdx[i] : i];
    return qs;
}
// h += {v[i], Shoup(v[i], q[i])}, i < n
static void append_pairs(std::vector<TwPair>& h, const uint64_t* v, const uint64_t* q, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i)
        h.push_back(TwPair{v[i], host::shoup(v[i], q[i])});
}
// The argument checks of the family for the entry `who`: a tower of sizeQl limbs over context limbs limbIdx (null: the leading ones;
// leading: and then within the context's own), of which the last `levels` are dropped and the first nOut produced (the single-limb entries
// pass 1 and sizeQl - 1), and a workspace of wsNeed bytes for `batch` towers.  nonNull: the entry's own pointers.  The several-limb entries
// report a limb index outside the context before a short workspace, the single-limb ones after it: callers see which text comes first.
// "Removing last element ..." is the reference's text (dcrtpoly-impl.h:672-673).
static fhe_status drop_check(const char* who, const fhe_ctx* c, bool nonNull, const uint32_t* limbIdx, bool leading, uint32_t sizeQl,
                             uint32_t levels, uint32_t nOut, uint32_t batch, size_t wsBytes, size_t wsNeed, bool several) {
    const std::string w(who);
    ARG_CHECK(c && nonNull, w + ": null argument");
    ARG_CHECK(sizeQl >= 2 && sizeQl <= (leading ? c->L : (uint32_t)kMaxLimbs), "Removing last element of DCRTPoly renders it invalid.");
    ARG_CHECK(levels >= 1 && levels < sizeQl, w + ": levels must be in [1, sizeQl)");
    ARG_CHECK(nOut >= 1 && nOut <= sizeQl - levels, w + ": nOut must be in [1, sizeQl - levels]");
    bool limbsOk = true;
    for (uint32_t i = 0; i < sizeQl; ++i)
        limbsOk = limbsOk && (limbIdx ? limbIdx[i] : i) < c->L;
    ARG_CHECK(limbsOk || !several, w + ": limb index exceeds context size");
    ARG_CHECK(batch >= 1 && wsBytes >= wsNeed, w + ": workspace too small");
    RT_CHECK(rt::set_device(c->device));
    ARG_CHECK(limbsOk, w + ": limb index exceeds context size");
    return FHE_OK;
}

// The forward transform of r into nOut limbs whose store is (x - NTT(r_i)) * C_i, r_i being the dropped limb(s) switched into limb i on the
// way in: the one place that sets up the fused store of the family.
//   rows   the dropped limbs in COEFFICIENT format, [batch][max(proRows, 1)][N]; row k is a limb modulo q[rowIdx[k]]
//   proRows == 0: one row, r_i = SwitchModulus(row) (proC null: prologue mode 1) or SwitchModulus(row) * proC[i] (mode 2)
//   proRows == d: r_i = sum_k SwitchModulus(row k) * proC[k * nOut + i] (mode 3; the caller has asked ntt_prologue_supported)
//   x      the towers the store reads: xStride rows (or, xDelta != 0, xDelta words) apart, limb i in row i
//   out0, out1   out1 null: dense out0[batch][nOut][N], the transform works in place there; else tower 0 -> out0, tower 1 -> out1 (batch 2)
//                and the transform works in `work`, its fused store going to the two output towers
// Two launches on a ring of two passes: the column pass with the prologue, the row pass with the epilogue.  N = 4096 has one pass and no
// prologue: SwitchModulus (times proC) as a kernel of its own into the working tower, then the single pass with the fused store.
static fhe_status drop_fused_store(fhe_ctx* c, const uint64_t* rows, const uint32_t* rowIdx, uint32_t proRows, const TwPair* proC,
                                   const uint64_t* x, int64_t xDelta, uint32_t xStride, const TwPair* C, const uint32_t* limbIdx,
                                   uint32_t nOut, uint32_t batch, uint64_t* out0, uint64_t* out1, uint64_t* work, void* st, const char* who) {
    NttEpilogue epi;
    epi.mode = 1, epi.split = out1 ? 1 : batch, epi.aStride = xStride, epi.aFirst = 0, epi.aDelta = xDelta;
    epi.A = x, epi.C = C, epi.out0 = out0, epi.out1 = out1 ? out1 : out0;
    uint64_t* dst = out1 ? work : out0;
    NttOpts fusedStore;
    fusedStore.epi = &epi;
    if (ntt_prologue_supported(c)) {
        fusedStore.src.stride = proRows ? proRows : 1, fusedStore.src.first = 0;
        fusedStore.proSrcLimb = rowIdx, fusedStore.proRows = proRows, fusedStore.proC = proC;
        return ntt_run(c, false, rows, dst, limbIdx, nOut, batch, st, fusedStore);
    }
    LimbSel sel;
    if (fhe_status s = make_sel(c, limbIdx, nOut, &sel, who))
        return s;
    if (fhe_status s = switch_modulus_run(c, dst, sel, nOut, rows, 1, 0, rowIdx[0], proC, batch, st))
        return s;
    return ntt_run(c, false, dst, dst, limbIdx, nOut, batch, st, fusedStore);
}

// The device constants of dropping ONE limb (one Shoup pair per kept limb unless noted), for the two members:
//   DropLastElementAndScale (dcrtpoly-impl.h:693-712), CKKS:  out_i = x_i * B_i + NTT(SwitchModulus(last) * A_i)
//     A = QlQlInvModqlDivqlModq, B = qlInvModq, no T and no row multiplier; evalFormat 1.
//   ModReduce (dcrtpoly-impl.h:736-755), BGV with plaintext modulus t:
//     delta = [last limb]_COEFF * (-t^-1 mod q_l);  out_i = (x_i + t * SwitchModulus(delta -> q_i)) * q_l^-1
//     A = t * qlInvModq, B = qlInvModq, T = t mod q_i, rowUnfused = negtInvModq, rowFused = t^-1 mod q_l.
struct DropTabs {
    const TwPair* A;           // unfused: the switched row times A_i goes through the forward transform
    const TwPair* B;           // the store's constant: x_i * B_i + NTT(..) unfused, (x_i - r_i) * B_i fused
    const TwPair* T;           // fused: r_i = NTT(SwitchModulus(row) * T_i); null: no constant (prologue mode 1)
    const TwPair* rowUnfused;  // one pair modulo q_l that the INTT row is multiplied by first; null: no such launch
    const TwPair* rowFused;    // ... in the fused form
    bool fusable;              // the rule of the entry (above), its *_UNFUSED switch folded in
    const char* who;           // the member, for the texts of the launches' own errors
};
// x[batch][sizeQl][N] over context limbs limbIdx[0..sizeQl) (null: the leading ones) -> out[batch][sizeQl-1][N].  ws: last[batch][N] +
// tmp[batch][l][N] (fhe_rescale_workspace_bytes).
//   unfused (rings below 4096, COEFFICIENT towers, tables that are not fusable): x_i * B_i + NTT(SwitchModulus(row) * A_i), row = INTT of the
//   last limb (times rowUnfused).  The NTT is linear and every step yields canonical residues, so the words equal the reference's.  Five
//   launches for a CKKS tower on a ring of two passes, six for an EVALUATION BGV tower.
//   fused (EVALUATION towers on rings of static passes): the shape (A - r) * C of the transform's epilogue (NttPassArgs::epi*),
//     row   = INTT(x_l) (* rowFused)                     one row per tower
//     r_i   = NTT(SwitchModulus(row -> q_i) (* T_i))
//     out_i = (x_i - r_i) * B_i.
//   CKKS: x*B + NTT(SwitchModulus(last)*(-B)) == (x - NTT(SwitchModulus(last)))*B with canonical residues on both sides.  4 launches.
//   BGV: row is the canonical residue of -delta.  SwitchModulus is odd under negation for odd q_l: with h = floor(q_l / 2), v > h holds
//   exactly when q_l - v <= h (v != 0), so the centred representative of q_l - v is minus that of v and SwitchModulus(q_l - v -> q_i) =
//   -SwitchModulus(v -> q_i) mod q_i (0 maps to 0).  Hence r_i = -NTT(t * SwitchModulus(delta)) and out_i = (x_i + t * NTT(SwitchModulus(
//   delta))) * q_l^-1 as residues; every step (the one-row product, the switch, the product by t mod q_i, the transform, the epilogue) yields
//   the canonical residue, so the words are the reference's.  5 launches: the one-row product by t^-1 is kept a launch of its own (it is one
//   row per tower, against 16 more multiplications per lane and limb inside the prologue).
//   Neither the switched tower nor its transform goes to HBM outside `out` (drop_fused_store).
// x1 / out1 != null: the two elements of one ciphertext, allocated on their own (batch must be 2): the same launches over both towers, or,
// unfused, element by element.  xRows != 0: the towers of x are xRows >= sizeQl rows apart and the rows beyond sizeQl are not read (the
// LevelReduce in front of a step of fhe_mod_reduce_multi).
static fhe_status drop_last_run(fhe_ctx* c, const uint64_t* x, const uint32_t* limbIdx, uint32_t sizeQl, const DropTabs& tb, int evalFormat,
                                uint32_t batch, uint64_t* out, uint64_t* ws, void* st, const uint64_t* x1 = nullptr,
                                uint64_t* out1 = nullptr, uint32_t xRows = 0) {
    const uint32_t xs      = xRows ? xRows : sizeQl;  // rows between the towers of x
    const uint32_t l       = sizeQl - 1;
    const uint32_t lastIdx = limbIdx ? limbIdx[l] : l;
    uint64_t* last         = ws;                                 // [batch][N]
    uint64_t* tmp          = last + ((size_t)batch << c->logN);  // [batch][l][N]
    const bool fused       = evalFormat && tb.fusable && ntt_epilogue_supported(c);
    if (x1 && !fused) {
        if (fhe_status s = drop_last_run(c, x, limbIdx, sizeQl, tb, evalFormat, 1, out, ws, st))
            return s;
        return drop_last_run(c, x1, limbIdx, sizeQl, tb, evalFormat, 1, out1, ws, st);
    }
    const int64_t xDelta = x1 ? x1 - x : 0;
    if (evalFormat) {  // lastPoly.SetFormat(COEFFICIENT)  (:696-697, :741): INTT of the last limb of every tower, written densely
        NttOpts lastRow;
        lastRow.src.stride = xs, lastRow.src.first = l, lastRow.srcDelta = xDelta;
        if (fhe_status s = ntt_run(c, true, x, last, &lastIdx, 1, batch, st, lastRow))
            return s;
    }
    else
        RT_CHECK(rt::d2d_2d(last, (size_t)8 << c->logN, x + ((size_t)l << c->logN), ((size_t)xs * 8) << c->logN,
                            (size_t)8 << c->logN, batch, (rt::stream_t)st));
    if (const TwPair* row = fused ? tb.rowFused : tb.rowUnfused)  // :742
        if (fhe_status s = elem_run<OP_MUL_CONST>(c, last, last, nullptr, row, &lastIdx, 1, batch, st, tb.who))
            return s;
    if (fused)
        return drop_fused_store(c, last, &lastIdx, 0, tb.T, x, xDelta, xs, tb.B, limbIdx, l, batch, out, out1, tmp, st, tb.who);
    // tmp = SwitchModulus(row -> q_i) * A_i   (:703-705; :749, :752 with t folded into A_i)
    LimbSel sel;
    if (fhe_status s = make_sel(c, limbIdx, l, &sel, tb.who))
        return s;
    if (fhe_status s = switch_modulus_run(c, tmp, sel, l, last, 1, 0, lastIdx, tb.A, batch, st))
        return s;
    if (evalFormat)  // tmp.SwitchFormat()  (:706-707, :750-751)
        if (fhe_status s = fhe_ntt_fwd(c, tmp, limbIdx, l, batch, st))
            return s;
    // m_vectors[i] = m_vectors[i] * B_i + tmp  (:708-709, :752-753); x towers are sizeQl rows apart
    return elem_run<OP_MUL_CONST_ADD>(c, out, x, tmp, tb.B, limbIdx, l, batch, st, tb.who, xs, 0);
}

// ---- CKKS rescale ----
// towers over the leading limbs, tables derived per sizeQl (and kept: a steady-state call derives and uploads nothing)
extern "C" fhe_status fhe_rescale(fhe_ctx* c, const uint64_t* x, uint32_t sizeQl, uint32_t batch, uint64_t* out,
                                  void* wsv, size_t wsBytes, void* st) {
    if (fhe_status s = drop_check("fhe_rescale", c, x && out && wsv, nullptr, true, sizeQl, 1, sizeQl - 1, batch, wsBytes,
                                  fhe_rescale_workspace_bytes(c, sizeQl, batch), false))
        return s;
    const uint32_t l = sizeQl - 1;
    std::unique_lock<std::mutex> lock(c->cacheMutex);
    auto it = c->rescaleTabs.find(sizeQl);
    if (it == c->rescaleTabs.end()) {
        std::vector<uint64_t> A, B;
        host::rescale_step_tables(c->q.data(), sizeQl, 1, A, B);
        std::vector<TwPair> hA, hB;
        append_pairs(hA, A.data(), c->q.data(), l), append_pairs(hB, B.data(), c->q.data(), l);
        TwPair *dA = nullptr, *dB = nullptr;
        fhe_status s;
        if ((s = dev_copy(&c->owned, hA.data(), l, &dA)) || (s = dev_copy(&c->owned, hB.data(), l, &dB)))
            return s;
        it = c->rescaleTabs.emplace(sizeQl, std::make_pair(dA, dB)).first;
    }
    const DropTabs tb{it->second.first, it->second.second, nullptr, nullptr, nullptr, !rescale_unfused(), "fhe_rescale"};
    lock.unlock();
    return drop_last_run(c, x, nullptr, sizeQl, tb, 1, batch, out, (uint64_t*)wsv, st);
}
// the same with the caller's tables (host arrays of sizeQl-1 residues: CryptoParametersRNS::GetQlQlInvModqlDivqlModq(l) /
// GetqlInvModq(l)) over any limbs of the context: what the DCRTPoly backend's DropLastElementAndScale calls
static fhe_status rescale_limbs_run(fhe_ctx* c, const uint64_t* x, const uint64_t* x1, const uint32_t* limbIdx, uint32_t sizeQl,
                                    const uint64_t* QlQlInvModqlDivqlModq, const uint64_t* qlInvModq, uint32_t batch, uint64_t* out,
                                    uint64_t* out1, void* wsv, size_t wsBytes, void* st, const char* who) {
    if (fhe_status s = drop_check(who, c, x && out && wsv && QlQlInvModqlDivqlModq && qlInvModq, limbIdx, false, sizeQl, 1, sizeQl - 1,
                                  batch, wsBytes, fhe_rescale_workspace_bytes(c, sizeQl, batch), false))
        return s;
    const uint32_t l = sizeQl - 1;
    DropTabs tb{};
    tb.who     = "fhe_rescale";
    tb.fusable = host::negated_pair(tower_moduli(c, limbIdx, l).data(), QlQlInvModqlDivqlModq, qlInvModq, l) && !rescale_unfused();
    if (fhe_status s = const_tables_trim(c))
        return s;
    std::shared_lock<std::shared_mutex> gate(c->constTabsGate);
    if (fhe_status s = const_table(c, limbIdx, QlQlInvModqlDivqlModq, l, &tb.A))
        return s;
    if (fhe_status s = const_table(c, limbIdx, qlInvModq, l, &tb.B))
        return s;
    return drop_last_run(c, x, limbIdx, sizeQl, tb, 1, batch, out, (uint64_t*)wsv, st, x1, out1);
}
extern "C" fhe_status fhe_rescale_limbs(fhe_ctx* c, const uint64_t* x, const uint32_t* limbIdx, uint32_t sizeQl,
                                        const uint64_t* QlQlInvModqlDivqlModq, const uint64_t* qlInvModq, uint32_t batch,
                                        uint64_t* out, void* wsv, size_t wsBytes, void* st) {
    return rescale_limbs_run(c, x, nullptr, limbIdx, sizeQl, QlQlInvModqlDivqlModq, qlInvModq, batch, out, nullptr, wsv, wsBytes, st,
                             "fhe_rescale_limbs");
}
// the two elements of one ciphertext (towers x0, x1 -> out0, out1, each allocated on its own) in the same four launches;
// ws of fhe_rescale_workspace_bytes(ctx, sizeQl, 2)
extern "C" fhe_status fhe_rescale_limbs_pair(fhe_ctx* c, const uint64_t* x0, const uint64_t* x1, const uint32_t* limbIdx, uint32_t sizeQl,
                                             const uint64_t* QlQlInvModqlDivqlModq, const uint64_t* qlInvModq, uint64_t* out0,
                                             uint64_t* out1, void* wsv, size_t wsBytes, void* st) {
    ARG_CHECK(x1 && out1 && x1 != x0 && out1 != out0, "fhe_rescale_limbs_pair: needs two distinct towers");
    return rescale_limbs_run(c, x0, x1, limbIdx, sizeQl, QlQlInvModqlDivqlModq, qlInvModq, 2, out0, out1, wsv, wsBytes, st,
                             "fhe_rescale_limbs_pair");
}

// ---- CKKS rescale by several limbs (composite scaling) ----
// LeveledSHECKKSRNS::ModReduceInternalInPlace(ct, levels) (ckksrns-leveledshe.cpp:172-191) calls DropLastElementAndScale `levels` times on
// every element; under COMPOSITESCALINGAUTO / COMPOSITESCALINGMANUAL levels = compositeDegree on every rescale, and AdjustLevelsAndDepthInPlace
// (:600-730) puts a scalar product in front and a LevelReduceInternalInPlace behind.  One call here: x[batch][sizeQl][N] EVALUATION, optionally
// times the scalar's residues scale[sizeQl], rescaled by the last `levels` limbs, of which the first nOut limbs are produced.
// ws: three regions of batch * sizeQl * N words each —
//   R0  fused: INTT of the dropped limbs, rows[batch][d][N];  sequential: the workspace of drop_last_run
//   R1, R2  the towers between chunks / steps, alternating; the transform's working tower when the store goes to two output towers
extern "C" size_t fhe_rescale_multi_workspace_bytes(const fhe_ctx* c, uint32_t sizeQl, uint32_t levels, uint32_t batch) {
    if (!c || sizeQl < 2 || levels < 1 || levels >= sizeQl)
        return 0;
    return (((size_t)3 * batch * sizeQl) << c->logN) * 8;
}
// the caller's (or the derived) tables of step k: sizeQl-1-k residues at offset sum_{j<k} (sizeQl-1-j)
static size_t rescale_multi_tab_offset(uint32_t sizeQl, uint32_t k) { return (size_t)k * (sizeQl - 1) - (size_t)k * (k ? k - 1 : 0) / 2; }
// One chunk of d <= kMaxRescaleDrop limbs, fused: x is a tower of n limbs (towers n rows or xDelta words apart), limbs
// limbIdx[0..n) of the context with moduli qs[0..n); out0 (and out1 != null: tower 1 goes there, batch must be 2) dense [.][nOut][N].  Five
// launches on a ring of two passes: the two inverse passes over the d dropped limbs, the chain kernel, the column pass whose load sums the d
// switched rows, the row pass whose store is (x - r) * C.
static fhe_status rescale_multi_chunk(fhe_ctx* c, const uint64_t* x, int64_t xDelta, const uint32_t* limbIdx, const uint64_t* qs, uint32_t n,
                                      uint32_t d, uint32_t nOut, const uint64_t* scale, uint32_t batch, uint64_t* out0, uint64_t* out1,
                                      uint64_t* rows, uint64_t* work, void* st) {
    uint32_t rowIdx[kMaxRescaleDrop];  // step k drops limb n-1-k; row p of `rows` is limb n-d+p
    uint64_t qDrop[kMaxRescaleDrop], sDrop[kMaxRescaleDrop];
    for (uint32_t k = 0; k < d; ++k) {
        rowIdx[k] = limbIdx ? limbIdx[n - d + k] : n - d + k;
        qDrop[k]  = qs[n - 1 - k];
        sDrop[k]  = scale ? scale[n - 1 - k] : 1;
    }
    std::vector<uint64_t> W(2 * (size_t)d * nOut), C(2 * (size_t)nOut);
    uint64_t B[2 * kMaxRescaleDrop * kMaxRescaleDrop], S[2 * kMaxRescaleDrop];
    host::rescale_multi_tables(qDrop, d, qs, nOut, scale ? sDrop : nullptr, scale, B, W.data(), C.data(), S);
    // device copies: the weights in the order of the rows (row p = step d-1-p), cached by content like every per-call table
    std::vector<uint32_t> wLimb((size_t)d * nOut);
    std::vector<uint64_t> wVal((size_t)d * nOut), cVal(nOut);
    for (uint32_t p = 0; p < d; ++p)
        for (uint32_t i = 0; i < nOut; ++i) {
            wLimb[(size_t)p * nOut + i] = limbIdx ? limbIdx[i] : i;
            wVal[(size_t)p * nOut + i]  = W[2 * ((size_t)(d - 1 - p) * nOut + i)];
        }
    for (uint32_t i = 0; i < nOut; ++i)
        cVal[i] = C[2 * i];
    const TwPair *dW = nullptr, *dC = nullptr;
    if (fhe_status s = const_table(c, wLimb.data(), wVal.data(), d * nOut, &dW))
        return s;
    if (fhe_status s = const_table(c, wLimb.data(), cVal.data(), nOut, &dC))
        return s;
    // lastPoly.SetFormat(COEFFICIENT) of every step's last limb (dcrtpoly-impl.h:696-697), all d rows of every tower at once
    NttOpts dropped;
    dropped.src.stride = n, dropped.src.first = n - d, dropped.srcDelta = xDelta;
    if (fhe_status s = ntt_run(c, true, x, rows, rowIdx, d, batch, st, dropped))
        return s;
    RescaleChainArgs g;
    g.rows = rows, g.logN = c->logN, g.d = d, g.batch = batch, g.hasScale = scale ? 1u : 0u;
    for (uint32_t k = 0; k < (uint32_t)kMaxRescaleDrop; ++k) {
        g.q[k] = k < d ? qDrop[k] : 1;
        g.s[k] = k < d ? TwPair{S[2 * k], S[2 * k + 1]} : TwPair{0, 0};
        for (uint32_t j = 0; j < (uint32_t)kMaxRescaleDrop; ++j)
            g.B[k][j] = (k < d && j < d) ? TwPair{B[2 * (k * d + j)], B[2 * (k * d + j) + 1]} : TwPair{0, 0};
    }
    if (d > 1 || scale) {
        FHE_LAUNCH(rescale_chain_kernel, tiles_for(c, batch), st, g);
        LAUNCH_CHECK();
    }
    return drop_fused_store(c, rows, rowIdx, d, dW, x, xDelta, n, dC, limbIdx, nOut, batch, out0, out1, work, st, "fhe_rescale_multi");
}
// derived: the tables are the negated pair of the true inverses at every step, i.e. what the library would compute itself; only then do the
// steps collapse into the one-pass form.  tabA / tabB: host tables in the layout of fhe_rescale_multi_limbs; qs: the tower's moduli.
static fhe_status rescale_multi_run(fhe_ctx* c, const uint64_t* x, const uint64_t* x1, const uint32_t* limbIdx, const uint64_t* qs,
                                    uint32_t sizeQl, uint32_t levels, uint32_t nOut, const uint64_t* scale, const uint64_t* tabA,
                                    const uint64_t* tabB, bool derived, uint32_t batch, uint64_t* out, uint64_t* out1, uint64_t* ws, void* st) {
    const size_t region = ((size_t)batch * sizeQl) << c->logN;
    uint64_t *R0 = ws, *R[2] = {ws + region, ws + 2 * region};
    bool fused = derived && !rescale_unfused() && ntt_epilogue_supported(c) && ntt_prologue_supported(c);
    for (uint32_t i = 0; scale && i < sizeQl; ++i)
        fused = fused && scale[i] != 0;  // (a zero residue has no inverse to put into the load's weights)
    if (levels == 1 && !scale && nOut == sizeQl - 1)
        fused = false;  // the member itself: drop_last_run's four launches
    if (fused) {
        const uint64_t* cur = x;
        int64_t curDelta    = x1 ? x1 - x : 0;
        uint32_t n = sizeQl, left = levels, j = 0;
        while (left) {
            const uint32_t d    = std::min<uint32_t>(left, (uint32_t)kMaxRescaleDrop);
            const bool lastOne  = left == d;
            const uint32_t keep = lastOne ? nOut : n - d;
            uint64_t* dst       = lastOne ? out : R[j & 1];
            if (fhe_status s = rescale_multi_chunk(c, cur, curDelta, limbIdx, qs, n, d, keep, j == 0 ? scale : nullptr, batch, dst,
                                                   lastOne ? out1 : nullptr, R0, R[j & 1], st))
                return s;
            cur = dst, curDelta = 0, n -= d, left -= d, ++j;
        }
        return FHE_OK;
    }
    if (x1) {  // element by element
        if (fhe_status s = rescale_multi_run(c, x, nullptr, limbIdx, qs, sizeQl, levels, nOut, scale, tabA, tabB, derived, 1, out, nullptr, ws, st))
            return s;
        return rescale_multi_run(c, x1, nullptr, limbIdx, qs, sizeQl, levels, nOut, scale, tabA, tabB, derived, 1, out1, nullptr, ws, st);
    }
    // the reference's loop: EvalMultCoreInPlace's scalar product, DropLastElementAndScale `levels` times, the limbs beyond nOut dropped
    const uint64_t* cur = x;
    if (scale) {
        const TwPair* dS = nullptr;
        if (fhe_status s = const_table(c, limbIdx, scale, sizeQl, &dS))
            return s;
        if (fhe_status s = elem_run<OP_MUL_CONST>(c, R[1], x, nullptr, dS, limbIdx, sizeQl, batch, st, "fhe_rescale_multi"))
            return s;
        cur = R[1];
    }
    uint32_t n = sizeQl;
    for (uint32_t k = 0; k < levels; ++k, --n) {
        const size_t off = rescale_multi_tab_offset(sizeQl, k);
        DropTabs tb{};
        tb.who     = "fhe_rescale";
        tb.fusable = host::negated_pair(qs, tabA + off, tabB + off, n - 1) && !rescale_unfused();
        if (fhe_status s = const_table(c, limbIdx, tabA + off, n - 1, &tb.A))
            return s;
        if (fhe_status s = const_table(c, limbIdx, tabB + off, n - 1, &tb.B))
            return s;
        const bool direct = k + 1 == levels && nOut == n - 1;
        uint64_t* dst     = direct ? out : R[k & 1];
        if (fhe_status s = drop_last_run(c, cur, limbIdx, n, tb, 1, batch, dst, R0, st))
            return s;
        cur = dst;
    }
    if (cur != out)  // LevelReduceInternalInPlace: the first nOut limbs of every tower
        RT_CHECK(rt::d2d_2d(out, ((size_t)nOut * 8) << c->logN, cur, ((size_t)n * 8) << c->logN, ((size_t)nOut * 8) << c->logN, batch,
                            (rt::stream_t)st));
    return FHE_OK;
}
// argument checks and tables of the three entry points; tabA / tabB null: the library's own tables over the leading limbs
static fhe_status rescale_multi_entry(fhe_ctx* c, const uint64_t* x, const uint64_t* x1, const uint32_t* limbIdx, uint32_t sizeQl,
                                      uint32_t levels, uint32_t nOut, const uint64_t* scale, const uint64_t* tabA, const uint64_t* tabB,
                                      bool ownTables, uint32_t batch, uint64_t* out, uint64_t* out1, void* wsv, size_t wsBytes, void* st,
                                      const char* who) {
    const std::string w(who);
    if (fhe_status s = drop_check(who, c, x && out && wsv && (ownTables || (tabA && tabB)), limbIdx, !limbIdx, sizeQl, levels, nOut, batch,
                                  wsBytes, fhe_rescale_multi_workspace_bytes(c, sizeQl, levels, batch), true))
        return s;
    ARG_CHECK(out != x && out != x1 && (!out1 || (out1 != x && out1 != x1)), w + ": out must not alias x");
    const std::vector<uint64_t> qs = tower_moduli(c, limbIdx, sizeQl);
    for (uint32_t i = 0; scale && i < sizeQl; ++i)
        ARG_CHECK(scale[i] < qs[i], w + ": scale is not reduced modulo its limb");
    std::vector<uint64_t> ownA, ownB;  // ckksrns-cryptoparameters.cpp:60-81 at every step
    host::rescale_step_tables(qs.data(), sizeQl, levels, ownA, ownB);
    bool derived = true;
    for (uint32_t k = 0; k < levels; ++k) {
        const size_t off = rescale_multi_tab_offset(sizeQl, k);
        const uint32_t n = sizeQl - 1 - k;
        if (ownTables) {
            ARG_CHECK(host::true_inverses(&ownB[off], &ownB[off], n), w + ": the moduli of a tower must be distinct");
            continue;
        }
        for (uint32_t i = 0; i < n; ++i)
            ARG_CHECK(tabA[off + i] < qs[i] && tabB[off + i] < qs[i], w + ": table entry is not reduced modulo its limb");
        derived = derived && host::true_inverses(&ownB[off], tabB + off, n) && host::negated_pair(qs.data(), tabA + off, tabB + off, n);
    }
    if (ownTables)
        tabA = ownA.data(), tabB = ownB.data();
    if (fhe_status s = const_tables_trim(c))
        return s;
    std::shared_lock<std::shared_mutex> gate(c->constTabsGate);
    return rescale_multi_run(c, x, x1, limbIdx, qs.data(), sizeQl, levels, nOut, scale, tabA, tabB, derived, batch, out, out1, (uint64_t*)wsv,
                             st);
}
extern "C" fhe_status fhe_rescale_multi(fhe_ctx* c, const uint64_t* x, uint32_t sizeQl, uint32_t levels, uint32_t nOut,
                                        const uint64_t* scale, uint32_t batch, uint64_t* out, void* wsv, size_t wsBytes, void* st) {
    return rescale_multi_entry(c, x, nullptr, nullptr, sizeQl, levels, nOut, scale, nullptr, nullptr, true, batch, out, nullptr, wsv,
                               wsBytes, st, "fhe_rescale_multi");
}
extern "C" fhe_status fhe_rescale_multi_limbs(fhe_ctx* c, const uint64_t* x, const uint32_t* limbIdx, uint32_t sizeQl, uint32_t levels,
                                              uint32_t nOut, const uint64_t* scale, const uint64_t* QlQlInvModqlDivqlModq,
                                              const uint64_t* qlInvModq, uint32_t batch, uint64_t* out, void* wsv, size_t wsBytes,
                                              void* st) {
    return rescale_multi_entry(c, x, nullptr, limbIdx, sizeQl, levels, nOut, scale, QlQlInvModqlDivqlModq, qlInvModq, false, batch, out,
                               nullptr, wsv, wsBytes, st, "fhe_rescale_multi_limbs");
}
// the two elements of one ciphertext (towers x0, x1 -> out0, out1, each allocated on its own) in the same launches; ws for batch 2
extern "C" fhe_status fhe_rescale_multi_limbs_pair(fhe_ctx* c, const uint64_t* x0, const uint64_t* x1, const uint32_t* limbIdx,
                                                   uint32_t sizeQl, uint32_t levels, uint32_t nOut, const uint64_t* scale,
                                                   const uint64_t* QlQlInvModqlDivqlModq, const uint64_t* qlInvModq, uint64_t* out0,
                                                   uint64_t* out1, void* wsv, size_t wsBytes, void* st) {
    ARG_CHECK(x1 && out1, "fhe_rescale_multi_limbs_pair: null argument");
    ARG_CHECK(x1 != x0 && out1 != out0, "fhe_rescale_multi_limbs_pair: needs two distinct towers");
    return rescale_multi_entry(c, x0, x1, limbIdx, sizeQl, levels, nOut, scale, QlQlInvModqlDivqlModq, qlInvModq, false, 2, out0, out1,
                               wsv, wsBytes, st, "fhe_rescale_multi_limbs_pair");
}
// the host-side constants of one fused chunk (host::rescale_multi_tables) as the library derives them, for checks against exact integers
extern "C" fhe_status fhe_rescale_multi_host_tables(const uint64_t* qDrop, uint32_t d, const uint64_t* qKeep, uint32_t nKeep,
                                                    const uint64_t* sDrop, const uint64_t* sKeep, uint64_t* B, uint64_t* W, uint64_t* C,
                                                    uint64_t* S) {
    ARG_CHECK(qDrop && qKeep && B && W && C && S && (!sDrop == !sKeep), "fhe_rescale_multi_host_tables: null argument");
    ARG_CHECK(d >= 1 && d <= (uint32_t)kMaxRescaleDrop && nKeep >= 1, "fhe_rescale_multi_host_tables: bad sizes");
    for (uint32_t i = 0; sKeep && i < nKeep; ++i)
        ARG_CHECK(sKeep[i] % qKeep[i] != 0, "fhe_rescale_multi_host_tables: a zero scalar residue has no inverse");
    host::rescale_multi_tables(qDrop, d, qKeep, nKeep, sDrop, sKeep, B, W, C, S);
    return FHE_OK;
}

// ---- BGV ModReduce ----
// replaces DCRTPolyImpl::ModReduce (dcrtpoly-impl.h:736-755) on towers over the leading limbs, tables derived per (sizeQl, t) and kept
extern "C" fhe_status fhe_mod_reduce(fhe_ctx* c, const uint64_t* x, uint32_t sizeQl, uint64_t t, int evalFormat,
                                     uint32_t batch, uint64_t* out, void* wsv, size_t wsBytes, void* st) {
    if (fhe_status s = drop_check("fhe_mod_reduce", c, x && out && wsv, nullptr, true, sizeQl, 1, sizeQl - 1, batch, wsBytes,
                                  fhe_rescale_workspace_bytes(c, sizeQl, batch), false))
        return s;
    const uint32_t l  = sizeQl - 1;
    const uint64_t ql = c->q[l];
    ARG_CHECK(t >= 2 && t % ql != 0, "fhe_mod_reduce: t must be invertible modulo the dropped limb");
    std::unique_lock<std::mutex> lock(c->cacheMutex);
    auto it = c->modReduceTabs.find({sizeQl, t});
    if (it == c->modReduceTabs.end()) {
        const host::ModReduceTables own = host::mod_reduce_tables(c->q.data(), sizeQl, t, nullptr);
        std::vector<TwPair> h;  // (the layout of fhe_ctx::modReduceTabs)
        append_pairs(h, own.A.data(), c->q.data(), l), append_pairs(h, own.B.data(), c->q.data(), l);
        append_pairs(h, &own.negtInv, &ql, 1), append_pairs(h, &own.tInv, &ql, 1), append_pairs(h, own.T.data(), c->q.data(), l);
        TwPair* d = nullptr;
        if (fhe_status s = dev_copy(&c->owned, h.data(), h.size(), &d))
            return s;
        it = c->modReduceTabs.emplace(std::make_pair(sizeQl, t), d).first;
    }
    const TwPair* d = it->second;
    lock.unlock();
    const DropTabs tb{d, d + l, d + 2 * (size_t)l + 2, d + 2 * (size_t)l, d + 2 * (size_t)l + 1, !mod_reduce_unfused(), "fhe_mod_reduce"};
    return drop_last_run(c, x, nullptr, sizeQl, tb, evalFormat, batch, out, (uint64_t*)wsv, st);
}
// the same with the caller's tables over any limbs of the context, as DCRTPoly::ModReduce receives them (t, negtInvModq = -t^-1 mod q_l,
// qlInvModq[i] = q_l^-1 mod q_i for the sizeQl-1 kept limbs: CryptoParametersBGVRNS::GetNegtInvModq(l) / GetqlInvModq(l))
static fhe_status mod_reduce_limbs_run(fhe_ctx* c, const uint64_t* x, const uint64_t* x1, const uint32_t* limbIdx, uint32_t sizeQl, uint64_t t,
                                       uint64_t negtInvModq, const uint64_t* qlInvModq, int evalFormat, uint32_t batch, uint64_t* out,
                                       uint64_t* out1, void* wsv, size_t wsBytes, void* st, const char* who) {
    if (fhe_status s = drop_check(who, c, x && out && wsv && qlInvModq, limbIdx, false, sizeQl, 1, sizeQl - 1, batch, wsBytes,
                                  fhe_rescale_workspace_bytes(c, sizeQl, batch), false))
        return s;
    const uint32_t l               = sizeQl - 1;
    const uint32_t lastIdx         = limbIdx ? limbIdx[l] : l;
    const std::vector<uint64_t> qs = tower_moduli(c, limbIdx, sizeQl);
    const uint64_t ql              = qs[l];
    ARG_CHECK(t >= 2 && t % ql != 0, std::string(who) + ": t must be invertible modulo the dropped limb");
    ARG_CHECK(negtInvModq < ql, std::string(who) + ": negtInvModq is not reduced modulo the dropped limb");
    for (uint32_t i = 0; i < l; ++i)
        ARG_CHECK(qlInvModq[i] < qs[i], std::string(who) + ": qlInvModq is not reduced modulo its limb");
    const host::ModReduceTables own = host::mod_reduce_tables(qs.data(), sizeQl, t, qlInvModq);  // (A from the caller's inverses)
    DropTabs tb{};
    tb.who     = "fhe_mod_reduce";
    tb.fusable = negtInvModq == own.negtInv && host::true_inverses(own.B.data(), qlInvModq, l) && !mod_reduce_unfused();
    if (fhe_status s = const_tables_trim(c))
        return s;
    std::shared_lock<std::shared_mutex> gate(c->constTabsGate);
    if (fhe_status s = const_table(c, limbIdx, own.A.data(), l, &tb.A))
        return s;
    if (fhe_status s = const_table(c, limbIdx, qlInvModq, l, &tb.B))
        return s;
    if (fhe_status s = const_table(c, limbIdx, own.T.data(), l, &tb.T))
        return s;
    if (fhe_status s = const_table(c, &lastIdx, &negtInvModq, 1, &tb.rowUnfused))
        return s;
    if (fhe_status s = const_table(c, &lastIdx, &own.tInv, 1, &tb.rowFused))
        return s;
    return drop_last_run(c, x, limbIdx, sizeQl, tb, evalFormat, batch, out, (uint64_t*)wsv, st, x1, out1);
}
extern "C" fhe_status fhe_mod_reduce_limbs(fhe_ctx* c, const uint64_t* x, const uint32_t* limbIdx, uint32_t sizeQl, uint64_t t,
                                           uint64_t negtInvModq, const uint64_t* qlInvModq, int evalFormat, uint32_t batch, uint64_t* out,
                                           void* wsv, size_t wsBytes, void* st) {
    return mod_reduce_limbs_run(c, x, nullptr, limbIdx, sizeQl, t, negtInvModq, qlInvModq, evalFormat, batch, out, nullptr, wsv, wsBytes, st,
                                "fhe_mod_reduce_limbs");
}
// the two elements of one ciphertext (towers x0, x1 -> out0, out1, each allocated on its own) in the same launches: what
// LeveledSHEBGVRNS::ModReduceInternalInPlace (bgvrns-leveledshe.cpp:44-75) does element by element; ws of fhe_rescale_workspace_bytes(ctx, sizeQl, 2)
extern "C" fhe_status fhe_mod_reduce_limbs_pair(fhe_ctx* c, const uint64_t* x0, const uint64_t* x1, const uint32_t* limbIdx, uint32_t sizeQl,
                                                uint64_t t, uint64_t negtInvModq, const uint64_t* qlInvModq, int evalFormat, uint64_t* out0,
                                                uint64_t* out1, void* wsv, size_t wsBytes, void* st) {
    ARG_CHECK(x1 && out1 && x1 != x0 && out1 != out0, "fhe_mod_reduce_limbs_pair: needs two distinct towers");
    return mod_reduce_limbs_run(c, x0, x1, limbIdx, sizeQl, t, negtInvModq, qlInvModq, evalFormat, 2, out0, out1, wsv, wsBytes, st,
                                "fhe_mod_reduce_limbs_pair");
}

// ---- BGV level alignment of the automatic scaling modes: scalar, ModReduce, LevelReduce, ModReduce as one call ----
// LeveledSHEBGVRNS::AdjustLevelsAndDepth[ToOne]InPlace (bgvrns-leveledshe.cpp:83-233) does to one operand, under FLEXIBLEAUTO[EXT], some of:
// cv[i] *= scalar, ModReduceInternalInPlace (:44-75, DCRTPolyImpl::ModReduce on every element, dcrtpoly-impl.h:736-755), LevelReduce, and
// ModReduceInternalInPlace again.  One call here: every row times scalar mod q_i; then, for k = 0 .. levels-1, the rows above drop[k]
// discarded and ModReduce on row drop[k]; rows 0 .. nOut-1 kept.  x[batch][sizeQl][N] -> out[batch][nOut][N], same format.
// The steps collapse as those of the CKKS rescale do: the chain kernel leaves rho_k, the canonical residue of -delta_k, in
// the coefficient domain (its s[k] slot holds scalar * t^-1), prologue mode 3 sums the switched rows times (t mod q_i) * ..., and the row pass
// stores (x - r) * C; the constants are host::mod_reduce_multi_tables.  ws: the three regions of fhe_rescale_multi_workspace_bytes.
extern "C" size_t fhe_mod_reduce_multi_workspace_bytes(const fhe_ctx* c, uint32_t sizeQl, uint32_t levels, uint32_t batch) {
    return fhe_rescale_multi_workspace_bytes(c, sizeQl, levels, batch);
}
// One fused chunk of d <= kMaxRescaleDrop steps: x holds towers of which rows 0 .. drop[0] are read (xRows rows or xDelta words apart), limbs
// limbIdx[.] of the context with moduli qs[.]; drop[0] > drop[1] > ... are the rows of the steps; scale: the scalar's residues per row, or
// null.  out0 (and out1 != null: tower 1 goes there, batch must be 2) dense [.][nOut][N].  On a ring of two passes: two inverse passes per run
// of adjacent dropped rows (each run lands in its place in `rows`, ascending as the chain kernel reads them), the chain kernel, the column
// pass whose load sums the d switched rows, the row pass whose store is (x - r) * C: five launches for adjacent rows, seven for two runs.
static fhe_status mod_reduce_multi_chunk(fhe_ctx* c, const uint64_t* x, int64_t xDelta, uint32_t xRows, const uint32_t* limbIdx,
                                         const uint64_t* qs, const uint32_t* drop, uint32_t d, uint32_t nOut, uint64_t t,
                                         const uint64_t* scale, uint32_t batch, uint64_t* out0, uint64_t* out1, uint64_t* rows, uint64_t* work,
                                         void* st) {
    uint32_t rowIdx[kMaxRescaleDrop];  // row p of `rows` is the row of step d-1-p
    uint64_t qDrop[kMaxRescaleDrop], sDrop[kMaxRescaleDrop];
    for (uint32_t k = 0; k < d; ++k) {
        rowIdx[d - 1 - k] = limbIdx ? limbIdx[drop[k]] : drop[k];
        qDrop[k]          = qs[drop[k]];
        sDrop[k]          = scale ? scale[drop[k]] : 1;
    }
    std::vector<uint64_t> W(2 * (size_t)d * nOut), C(2 * (size_t)nOut);
    uint64_t B[2 * kMaxRescaleDrop * kMaxRescaleDrop], S[2 * kMaxRescaleDrop];
    host::mod_reduce_multi_tables(qDrop, d, qs, nOut, t, scale ? sDrop : nullptr, scale, B, W.data(), C.data(), S);
    std::vector<uint32_t> wLimb((size_t)d * nOut);
    std::vector<uint64_t> wVal((size_t)d * nOut), cVal(nOut);
    for (uint32_t p = 0; p < d; ++p)
        for (uint32_t i = 0; i < nOut; ++i) {
            wLimb[(size_t)p * nOut + i] = limbIdx ? limbIdx[i] : i;
            wVal[(size_t)p * nOut + i]  = W[2 * ((size_t)(d - 1 - p) * nOut + i)];
        }
    for (uint32_t i = 0; i < nOut; ++i)
        cVal[i] = C[2 * i];
    const TwPair *dW = nullptr, *dC = nullptr;
    if (fhe_status s = const_table(c, wLimb.data(), wVal.data(), d * nOut, &dW))
        return s;
    if (fhe_status s = const_table(c, wLimb.data(), cVal.data(), nOut, &dC))
        return s;
    // lastPoly.SetFormat(COEFFICIENT) of every step (dcrtpoly-impl.h:741): one inverse transform per run of adjacent dropped rows
    for (uint32_t k0 = 0; k0 < d;) {
        uint32_t k1 = k0;
        while (k1 + 1 < d && drop[k1 + 1] + 1 == drop[k1])
            ++k1;
        const uint32_t cnt = k1 - k0 + 1, p0 = d - 1 - k1;
        NttOpts run;
        run.src.stride = xRows, run.src.first = drop[k1], run.srcDelta = xDelta;
        if (cnt != d)
            run.dst.stride = d, run.dst.first = p0;
        if (fhe_status s = ntt_run(c, true, x, rows, rowIdx + p0, cnt, batch, st, run))
            return s;
        k0 = k1 + 1;
    }
    RescaleChainArgs g;
    g.rows = rows, g.logN = c->logN, g.d = d, g.batch = batch, g.hasScale = 1u;  // (s[k] = scalar * t^-1: never absent)
    for (uint32_t k = 0; k < (uint32_t)kMaxRescaleDrop; ++k) {
        g.q[k] = k < d ? qDrop[k] : 1;
        g.s[k] = k < d ? TwPair{S[2 * k], S[2 * k + 1]} : TwPair{0, 0};
        for (uint32_t j = 0; j < (uint32_t)kMaxRescaleDrop; ++j)
            g.B[k][j] = (k < d && j < d) ? TwPair{B[2 * (k * d + j)], B[2 * (k * d + j) + 1]} : TwPair{0, 0};
    }
    FHE_LAUNCH(rescale_chain_kernel, tiles_for(c, batch), st, g);
    LAUNCH_CHECK();
    return drop_fused_store(c, rows, rowIdx, d, dW, x, xDelta, xRows, dC, limbIdx, nOut, batch, out0, out1, work, st, "fhe_mod_reduce_multi");
}
// the tables of one step as DCRTPolyImpl::ModReduce receives them, and whether they are the ones the library derives
struct ModReduceStep {
    host::ModReduceTables own;  // A from the caller's inverses; B, T, tInv, negtInv derived
    uint64_t negtInv;           // the caller's (or the derived) negtInvModq
    const uint64_t* inv;        // the caller's (or the derived) qlInvModq, drop[k] residues
    bool derived;
};
static fhe_status mod_reduce_multi_run(fhe_ctx* c, const uint64_t* x, const uint64_t* x1, const uint32_t* limbIdx, const uint64_t* qs,
                                       uint32_t sizeQl, const uint32_t* drop, uint32_t levels, uint32_t nOut, uint64_t t,
                                       const uint64_t* scale, const std::vector<ModReduceStep>& steps, int evalFormat, uint32_t batch,
                                       uint64_t* out, uint64_t* out1, uint64_t* ws, void* st) {
    const size_t region = ((size_t)batch * sizeQl) << c->logN;
    uint64_t *R0 = ws, *R[2] = {ws + region, ws + 2 * region};
    bool fused = evalFormat && !mod_reduce_unfused() && ntt_epilogue_supported(c) && ntt_prologue_supported(c);
    for (uint32_t k = 0; k < levels; ++k)
        fused = fused && steps[k].derived;
    for (uint32_t i = 0; scale && i < sizeQl; ++i)
        fused = fused && scale[i] != 0;  // (a zero residue has no inverse to put into the load's weights)
    if (levels == 1 && !scale && nOut == drop[0])
        fused = false;  // the member itself on the rows below: drop_last_run's five launches
    if (fused) {
        const uint64_t* cur = x;
        int64_t curDelta    = x1 ? x1 - x : 0;
        uint32_t curRows    = sizeQl;
        for (uint32_t k = 0, j = 0; k < levels; ++j) {
            const uint32_t d    = std::min<uint32_t>(levels - k, (uint32_t)kMaxRescaleDrop);
            const bool lastOne  = k + d == levels;
            const uint32_t keep = lastOne ? nOut : drop[k + d - 1];
            uint64_t* dst       = lastOne ? out : R[j & 1];
            if (fhe_status s = mod_reduce_multi_chunk(c, cur, curDelta, curRows, limbIdx, qs, drop + k, d, keep, t, j == 0 ? scale : nullptr,
                                                      batch, dst, lastOne ? out1 : nullptr, R0, R[j & 1], st))
                return s;
            cur = dst, curDelta = 0, curRows = keep, k += d;
        }
        return FHE_OK;
    }
    if (x1) {  // element by element
        if (fhe_status s = mod_reduce_multi_run(c, x, nullptr, limbIdx, qs, sizeQl, drop, levels, nOut, t, scale, steps, evalFormat, 1, out,
                                                nullptr, ws, st))
            return s;
        return mod_reduce_multi_run(c, x1, nullptr, limbIdx, qs, sizeQl, drop, levels, nOut, t, scale, steps, evalFormat, 1, out1, nullptr, ws,
                                    st);
    }
    // the reference's steps: the scalar product on the rows that are read at all, then ModReduce on ever shorter towers
    const uint64_t* cur = x;
    uint32_t curRows    = sizeQl;
    if (scale) {
        const TwPair* dS = nullptr;
        if (fhe_status s = const_table(c, limbIdx, scale, drop[0] + 1, &dS))
            return s;
        if (fhe_status s = elem_run<OP_MUL_CONST>(c, R[1], x, nullptr, dS, limbIdx, drop[0] + 1, batch, st, "fhe_mod_reduce_multi", sizeQl, 0))
            return s;
        cur = R[1], curRows = drop[0] + 1;
    }
    for (uint32_t k = 0; k < levels; ++k) {
        const uint32_t n = drop[k] + 1, l = drop[k], lastIdx = limbIdx ? limbIdx[l] : l;
        const ModReduceStep& sp = steps[k];
        DropTabs tb{};
        tb.who     = "fhe_mod_reduce";
        tb.fusable = sp.derived && !mod_reduce_unfused();
        if (fhe_status s = const_table(c, limbIdx, sp.own.A.data(), l, &tb.A))
            return s;
        if (fhe_status s = const_table(c, limbIdx, sp.inv, l, &tb.B))
            return s;
        if (fhe_status s = const_table(c, limbIdx, sp.own.T.data(), l, &tb.T))
            return s;
        if (fhe_status s = const_table(c, &lastIdx, &sp.negtInv, 1, &tb.rowUnfused))
            return s;
        if (fhe_status s = const_table(c, &lastIdx, &sp.own.tInv, 1, &tb.rowFused))
            return s;
        const bool direct = k + 1 == levels && nOut == l;
        uint64_t* dst     = direct ? out : R[k & 1];
        if (fhe_status s = drop_last_run(c, cur, limbIdx, n, tb, evalFormat, batch, dst, R0, st, nullptr, nullptr, curRows))
            return s;
        cur = dst, curRows = l;
    }
    if (cur != out)  // LevelReduce: the first nOut rows of every tower
        RT_CHECK(rt::d2d_2d(out, ((size_t)nOut * 8) << c->logN, cur, ((size_t)curRows * 8) << c->logN, ((size_t)nOut * 8) << c->logN, batch,
                            (rt::stream_t)st));
    return FHE_OK;
}
// argument checks and tables of the entry points; negtInv / tabB null: the library's own tables over the leading limbs
static fhe_status mod_reduce_multi_entry(fhe_ctx* c, const uint64_t* x, const uint64_t* x1, const uint32_t* limbIdx, uint32_t sizeQl,
                                         uint64_t t, uint64_t scalar, const uint32_t* dropRows, uint32_t levels, uint32_t nOut,
                                         const uint64_t* negtInv, const uint64_t* tabB, bool ownTables, int evalFormat, uint32_t batch,
                                         uint64_t* out, uint64_t* out1, void* wsv, size_t wsBytes, void* st, const char* who) {
    const std::string w(who);
    if (fhe_status s = drop_check(who, c, x && out && wsv && (ownTables || (negtInv && tabB)), limbIdx, !limbIdx, sizeQl, levels, nOut, batch,
                                  wsBytes, fhe_mod_reduce_multi_workspace_bytes(c, sizeQl, levels, batch), true))
        return s;
    ARG_CHECK(!dropRows || levels <= (uint32_t)kMaxRescaleDrop, w + ": a row list takes at most 4 levels");
    std::vector<uint32_t> drop(levels);
    bool rowsOk = true;
    for (uint32_t k = 0; k < levels; ++k) {
        drop[k] = dropRows ? dropRows[k] : sizeQl - 1 - k;
        rowsOk  = rowsOk && drop[k] >= 1 && drop[k] < (k ? drop[k - 1] : sizeQl);
    }
    ARG_CHECK(rowsOk, w + ": dropRows must be strictly decreasing, below sizeQl and at least 1");
    ARG_CHECK(nOut <= drop[levels - 1], w + ": nOut must be in [1, dropRows[levels - 1]]");
    ARG_CHECK(out != x && out != x1 && (!out1 || (out1 != x && out1 != x1)), w + ": out must not alias x");
    const std::vector<uint64_t> qs = tower_moduli(c, limbIdx, sizeQl);
    ARG_CHECK(t >= 2, w + ": t must be invertible modulo the dropped limbs");
    std::vector<ModReduceStep> steps(levels);
    for (uint32_t k = 0; k < levels; ++k) {  // bgvrns-cryptoparameters.cpp at every step
        ARG_CHECK(t % qs[drop[k]] != 0, w + ": t must be invertible modulo the dropped limbs");
        steps[k].own = host::mod_reduce_tables(qs.data(), drop[k] + 1, t, nullptr);
        ARG_CHECK(host::true_inverses(steps[k].own.B.data(), steps[k].own.B.data(), drop[k]), w + ": the moduli of a tower must be distinct");
    }
    size_t off = 0;
    for (uint32_t k = 0; k < levels; off += drop[k], ++k) {
        const uint32_t l  = drop[k];
        ModReduceStep& sp = steps[k];
        if (ownTables) {
            sp.negtInv = sp.own.negtInv, sp.inv = sp.own.B.data(), sp.derived = true;
            continue;
        }
        const host::ModReduceTables own = sp.own;
        ARG_CHECK(negtInv[k] < qs[l], w + ": table entry is not reduced modulo its limb");
        for (uint32_t i = 0; i < l; ++i)
            ARG_CHECK(tabB[off + i] < qs[i], w + ": table entry is not reduced modulo its limb");
        sp.own     = host::mod_reduce_tables(qs.data(), l + 1, t, tabB + off);
        sp.negtInv = negtInv[k], sp.inv = tabB + off;
        sp.derived = negtInv[k] == own.negtInv && host::true_inverses(own.B.data(), tabB + off, l);
    }
    std::vector<uint64_t> scale;
    if (scalar != 1)
        for (uint32_t i = 0; i < sizeQl; ++i)
            scale.push_back(scalar % qs[i]);
    if (fhe_status s = const_tables_trim(c))
        return s;
    std::shared_lock<std::shared_mutex> gate(c->constTabsGate);
    return mod_reduce_multi_run(c, x, x1, limbIdx, qs.data(), sizeQl, drop.data(), levels, nOut, t, scalar != 1 ? scale.data() : nullptr, steps,
                                evalFormat, batch, out, out1, (uint64_t*)wsv, st);
}
extern "C" fhe_status fhe_mod_reduce_multi(fhe_ctx* c, const uint64_t* x, uint32_t sizeQl, uint64_t t, uint64_t scalar,
                                           const uint32_t* dropRows, uint32_t levels, uint32_t nOut, int evalFormat, uint32_t batch,
                                           uint64_t* out, void* wsv, size_t wsBytes, void* st) {
    return mod_reduce_multi_entry(c, x, nullptr, nullptr, sizeQl, t, scalar, dropRows, levels, nOut, nullptr, nullptr, true, evalFormat, batch,
                                  out, nullptr, wsv, wsBytes, st, "fhe_mod_reduce_multi");
}
extern "C" fhe_status fhe_mod_reduce_multi_limbs(fhe_ctx* c, const uint64_t* x, const uint32_t* limbIdx, uint32_t sizeQl, uint64_t t,
                                                 uint64_t scalar, const uint32_t* dropRows, uint32_t levels, uint32_t nOut,
                                                 const uint64_t* negtInvModq, const uint64_t* qlInvModq, int evalFormat, uint32_t batch,
                                                 uint64_t* out, void* wsv, size_t wsBytes, void* st) {
    return mod_reduce_multi_entry(c, x, nullptr, limbIdx, sizeQl, t, scalar, dropRows, levels, nOut, negtInvModq, qlInvModq, false, evalFormat,
                                  batch, out, nullptr, wsv, wsBytes, st, "fhe_mod_reduce_multi_limbs");
}
// the two elements of one ciphertext (towers x0, x1 -> out0, out1, each allocated on its own) in the same launches; ws for batch 2
extern "C" fhe_status fhe_mod_reduce_multi_limbs_pair(fhe_ctx* c, const uint64_t* x0, const uint64_t* x1, const uint32_t* limbIdx,
                                                      uint32_t sizeQl, uint64_t t, uint64_t scalar, const uint32_t* dropRows, uint32_t levels,
                                                      uint32_t nOut, const uint64_t* negtInvModq, const uint64_t* qlInvModq, int evalFormat,
                                                      uint64_t* out0, uint64_t* out1, void* wsv, size_t wsBytes, void* st) {
    ARG_CHECK(x1 && out1, "fhe_mod_reduce_multi_limbs_pair: null argument");
    ARG_CHECK(x1 != x0 && out1 != out0, "fhe_mod_reduce_multi_limbs_pair: needs two distinct towers");
    return mod_reduce_multi_entry(c, x0, x1, limbIdx, sizeQl, t, scalar, dropRows, levels, nOut, negtInvModq, qlInvModq, false, evalFormat, 2,
                                  out0, out1, wsv, wsBytes, st, "fhe_mod_reduce_multi_limbs_pair");
}
// the host-side constants of one fused chunk (host::mod_reduce_multi_tables) as the library derives them, for checks against exact integers
extern "C" fhe_status fhe_mod_reduce_multi_host_tables(const uint64_t* qDrop, uint32_t d, const uint64_t* qKeep, uint32_t nKeep, uint64_t t,
                                                       const uint64_t* sDrop, const uint64_t* sKeep, uint64_t* B, uint64_t* W, uint64_t* C,
                                                       uint64_t* S) {
    ARG_CHECK(qDrop && qKeep && B && W && C && S && (!sDrop == !sKeep), "fhe_mod_reduce_multi_host_tables: null argument");
    ARG_CHECK(d >= 1 && d <= (uint32_t)kMaxRescaleDrop && nKeep >= 1, "fhe_mod_reduce_multi_host_tables: bad sizes");
    for (uint32_t k = 0; k < d; ++k)
        ARG_CHECK(t >= 2 && t % qDrop[k] != 0, "fhe_mod_reduce_multi_host_tables: t must be invertible modulo the dropped limbs");
    for (uint32_t i = 0; sKeep && i < nKeep; ++i)
        ARG_CHECK(sKeep[i] % qKeep[i] != 0, "fhe_mod_reduce_multi_host_tables: a zero scalar residue has no inverse");
    host::mod_reduce_multi_tables(qDrop, d, qKeep, nKeep, t, sDrop, sKeep, B, W, C, S);
    return FHE_OK;
}

// ---- BGV ModReduce over several limbs of a COEFFICIENT tower, and decryption ----
// PKEBGVRNS::Decrypt (bgvrns-pke.cpp:44-99) and MultipartyBGVRNS::MultipartyDecryptFusion (bgvrns-multiparty.cpp:62-97) switch b to
// COEFFICIENT and call DCRTPolyImpl::ModReduce sizeQl - 1 times, then take the last limb's centred residues modulo t.  One launch of
// mod_reduce_chain_kernel per kMaxChainDrop dropped limbs does that; the tables are the library's own, derived from the
// tower's moduli and t (host::mod_reduce_chain_table) and kept per (limb list, t, limbs dropped, with or without the residue modulo t).
// ws: the towers between chunks, two regions that alternate; none when levels <= kMaxChainDrop.
extern "C" size_t fhe_mod_reduce_chain_workspace_bytes(const fhe_ctx* c, uint32_t sizeQl, uint32_t levels, uint32_t batch) {
    if (!c || levels >= sizeQl || levels <= (uint32_t)kMaxChainDrop)
        return 0;
    return (((size_t)2 * batch * (sizeQl - kMaxChainDrop)) << c->logN) * 8;
}
static fhe_status mod_reduce_chain_table(fhe_ctx* c, const uint32_t* limbIdx, const uint64_t* qs, uint32_t n, uint32_t d, uint64_t t, bool modT,
                                         const uint64_t** out) {
    std::vector<uint64_t> key{t, d, modT ? 1u : 0u};
    for (uint32_t i = 0; i < n; ++i)
        key.push_back(limbIdx ? limbIdx[i] : i);
    std::lock_guard<std::mutex> lock(c->cacheMutex);
    auto it = c->chainTabs.find(key);
    if (it == c->chainTabs.end()) {
        const std::vector<uint64_t> h = host::mod_reduce_chain_table(qs, n, d, t, modT);
        uint64_t* dev = nullptr;
        if (fhe_status s = dev_copy(&c->owned, h.data(), h.size(), &dev))
            return s;
        it = c->chainTabs.emplace(std::move(key), dev).first;
    }
    *out = it->second;
    return FHE_OK;
}
// x[batch][sizeQl][N] COEFFICIENT over limbIdx (null: the leading limbs), the last `levels` limbs dropped one by one; toT: levels is
// sizeQl - 1 (zero included) and out[batch][N] holds the residues modulo t of the limb that is left.  Checks first, then launches.
static fhe_status mod_reduce_chain_run(fhe_ctx* c, const uint64_t* x, const uint32_t* limbIdx, uint32_t sizeQl, uint32_t levels, uint64_t t,
                                       bool toT, uint32_t batch, uint64_t* out, void* wsv, size_t wsBytes, void* st, const char* who) {
    const std::string w(who);
    const size_t need = fhe_mod_reduce_chain_workspace_bytes(c, sizeQl, levels, batch);
    if (levels == 0) {  // (fhe_mod_reduce_to_t on one limb: no step, no limb to remove)
        ARG_CHECK(c && x && out, w + ": null argument");
        ARG_CHECK(batch >= 1, w + ": workspace too small");
        ARG_CHECK((limbIdx ? limbIdx[0] : 0u) < c->L, w + ": limb index exceeds context size");
        RT_CHECK(rt::set_device(c->device));
    }
    else if (fhe_status s = drop_check(who, c, x && out && (wsv || !need), limbIdx, !limbIdx, sizeQl, levels, sizeQl - levels, batch, wsBytes,
                                       need, true))
        return s;
    const std::vector<uint64_t> qs = tower_moduli(c, limbIdx, sizeQl);
    ARG_CHECK(t >= 2 && (!toT || t < ((uint64_t)1 << 63)), w + ": t must be in [2, 2^63)");
    for (uint32_t k = 0; k < levels; ++k) {
        ARG_CHECK(t % qs[sizeQl - 1 - k] != 0, w + ": t must be invertible modulo every dropped limb");
        for (uint32_t i = 0; i < sizeQl - 1 - k; ++i)
            ARG_CHECK(qs[i] != qs[sizeQl - 1 - k], w + ": the moduli of a tower must be distinct");
    }
    ARG_CHECK(out != x, w + ": out must not alias x");
    uint64_t* R[2] = {(uint64_t*)wsv, need ? (uint64_t*)wsv + need / 16 : nullptr};  // (two regions of need / 2 bytes)
    const uint64_t* cur = x;
    uint32_t n = sizeQl, left = levels, j = 0;
    do {
        const uint32_t d   = std::min<uint32_t>(left, (uint32_t)kMaxChainDrop);
        const bool lastOne = left == d;
        ModReduceChainArgs g;
        g.x = cur, g.out = lastOne ? out : R[j & 1], g.logN = c->logN, g.n = n, g.d = d, g.batch = batch;
        if (fhe_status s = mod_reduce_chain_table(c, limbIdx, qs.data(), n, d, t, lastOne && toT, &g.tab))
            return s;
        const uint32_t grid = (uint32_t)((((uint64_t)batch << c->logN) + kThreads - 1) / kThreads);
        if (lastOne && toT)
            FHE_LAUNCH((mod_reduce_chain_kernel<true>), grid, st, g);
        else
            FHE_LAUNCH((mod_reduce_chain_kernel<false>), grid, st, g);
        LAUNCH_CHECK();
        cur = g.out, n -= d, left -= d, ++j;
    } while (left);
    return FHE_OK;
}
// replaces `levels` consecutive DCRTPolyImpl::ModReduce calls (dcrtpoly-impl.h:736-755) on a COEFFICIENT tower: the second branch of
// PKEBGVRNS::Decrypt (bgvrns-pke.cpp:73-81) element by element
extern "C" fhe_status fhe_mod_reduce_chain(fhe_ctx* c, const uint64_t* x, const uint32_t* limbIdx, uint32_t sizeQl, uint32_t levels, uint64_t t,
                                           uint32_t batch, uint64_t* out, void* wsv, size_t wsBytes, void* st) {
    ARG_CHECK(levels >= 1, "fhe_mod_reduce_chain: levels must be in [1, sizeQl)");
    return mod_reduce_chain_run(c, x, limbIdx, sizeQl, levels, t, false, batch, out, wsv, wsBytes, st, "fhe_mod_reduce_chain");
}
// replaces the ModReduce loop and DecryptionCRTInterpolate of PKEBGVRNS::Decrypt (bgvrns-pke.cpp:56-60, 96) and of
// MultipartyBGVRNS::MultipartyDecryptFusion (bgvrns-multiparty.cpp:79-83, 94) on b in COEFFICIENT format
extern "C" fhe_status fhe_mod_reduce_to_t(fhe_ctx* c, const uint64_t* x, const uint32_t* limbIdx, uint32_t sizeQl, uint64_t t, uint32_t batch,
                                          uint64_t* out, void* wsv, size_t wsBytes, void* st) {
    ARG_CHECK(sizeQl >= 1, "fhe_mod_reduce_to_t: sizeQl must be at least 1");
    return mod_reduce_chain_run(c, x, limbIdx, sizeQl, sizeQl - 1, t, true, batch, out, wsv, wsBytes, st, "fhe_mod_reduce_to_t");
}
// replaces the first branch of PKEBGVRNS::Decrypt (bgvrns-pke.cpp:52-60, 96): PKERNS::DecryptCore (rns-pke.cpp:199-216), b = c0 + c1 * s
// (+ c2 * s^2), with the element-wise kernels, one inverse transform of all limbs of all towers, the chain down to one limb and its
// residues modulo t.  c[e]: element e of `batch` ciphertexts, [batch][sizeQl][N]; s: the secret key, ONE tower [sizeQl][N]; all in
// EVALUATION over limbIdx.  ws: b[batch][sizeQl][N], s^2 (nElem == 3), then the chain's workspace.
static size_t bgv_decrypt_b_words(const fhe_ctx* c, uint32_t nElem, uint32_t sizeQl, uint32_t batch) {
    return ((size_t)batch * sizeQl + (nElem == 3 ? sizeQl : 0)) << c->logN;
}
extern "C" size_t fhe_bgv_decrypt_workspace_bytes(const fhe_ctx* c, uint32_t nElem, uint32_t sizeQl, uint32_t batch) {
    if (!c || sizeQl < 1 || nElem < 2 || nElem > 3)
        return 0;
    return bgv_decrypt_b_words(c, nElem, sizeQl, batch) * 8 + fhe_mod_reduce_chain_workspace_bytes(c, sizeQl, sizeQl - 1, batch);
}
extern "C" fhe_status fhe_bgv_decrypt(fhe_ctx* c, const uint64_t* const* ct, uint32_t nElem, const uint64_t* s, const uint32_t* limbIdx,
                                      uint32_t sizeQl, uint64_t t, uint32_t batch, uint64_t* out, void* wsv, size_t wsBytes, void* st) {
    const char* who = "fhe_bgv_decrypt";
    ARG_CHECK(c && ct && s && out && wsv, "fhe_bgv_decrypt: null argument");
    ARG_CHECK(nElem == 2 || nElem == 3, "fhe_bgv_decrypt: a ciphertext of 2 or 3 elements expected");
    for (uint32_t e = 0; e < nElem; ++e)
        ARG_CHECK(ct[e] && ct[e] != out, "fhe_bgv_decrypt: null argument");
    ARG_CHECK(sizeQl >= 1 && sizeQl <= (limbIdx ? (uint32_t)kMaxLimbs : c->L), "fhe_bgv_decrypt: sizeQl exceeds context size");
    for (uint32_t i = 0; i < sizeQl; ++i)
        ARG_CHECK((limbIdx ? limbIdx[i] : i) < c->L, "fhe_bgv_decrypt: limb index exceeds context size");
    ARG_CHECK(batch >= 1 && wsBytes >= fhe_bgv_decrypt_workspace_bytes(c, nElem, sizeQl, batch), "fhe_bgv_decrypt: workspace too small");
    // (the chain's own checks, before anything is enqueued: the same texts under this entry's name)
    const std::vector<uint64_t> qs = tower_moduli(c, limbIdx, sizeQl);
    ARG_CHECK(t >= 2 && t < ((uint64_t)1 << 63), "fhe_bgv_decrypt: t must be in [2, 2^63)");
    for (uint32_t k = 1; k < sizeQl; ++k) {
        ARG_CHECK(t % qs[k] != 0, "fhe_bgv_decrypt: t must be invertible modulo every dropped limb");
        for (uint32_t i = 0; i < k; ++i)
            ARG_CHECK(qs[i] != qs[k], "fhe_bgv_decrypt: the moduli of a tower must be distinct");
    }
    uint64_t* b        = (uint64_t*)wsv;
    uint64_t* s2       = b + (((size_t)batch * sizeQl) << c->logN);
    uint64_t* chainWs  = b + bgv_decrypt_b_words(c, nElem, sizeQl, batch);
    const size_t chainBytes = wsBytes - bgv_decrypt_b_words(c, nElem, sizeQl, batch) * 8;
    if (fhe_status r = elem_run<OP_MUL_ROW>(c, b, ct[1], s, nullptr, limbIdx, sizeQl, batch, st, who))  // c1 * s
        return r;
    if (fhe_status r = elem_run<OP_ADD>(c, b, b, ct[0], nullptr, limbIdx, sizeQl, batch, st, who))  // c0 + c1 * s
        return r;
    if (nElem == 3) {  // sPower *= s; b += sPower * c2  (rns-pke.cpp:208-213)
        if (fhe_status r = elem_run<OP_MUL>(c, s2, s, s, nullptr, limbIdx, sizeQl, 1, st, who))
            return r;
        if (fhe_status r = elem_run<OP_MULT_ACC_ROW>(c, b, ct[2], s2, nullptr, limbIdx, sizeQl, batch, st, who))
            return r;
    }
    if (fhe_status r = fhe_ntt_inv(c, b, limbIdx, sizeQl, batch, st))  // b.SetFormat(COEFFICIENT), every limb of every tower at once
        return r;
    return mod_reduce_chain_run(c, b, limbIdx, sizeQl, sizeQl - 1, t, true, batch, out, chainWs, chainBytes, st, who);
}

// ------------------------------------------------------------------------------------------------
// BFV side: ScaleAndRound family and BEHZ
// ------------------------------------------------------------------------------------------------
struct fhe_sr_plan {
    fhe_ctx* ctx;
    uint32_t sizeI, sizeO;
    bool exact;
    uint64_t *d_tab = nullptr, *d_o = nullptr, *d_mu = nullptr;
    double* d_frac  = nullptr;
    std::vector<void*> owned;
};
extern "C" fhe_status fhe_sr_plan_create(fhe_ctx* c, uint32_t sizeI, const uint32_t* outLimbIdx, uint32_t sizeO,
                                         const uint64_t* tab, const double* frac, fhe_sr_plan** out) {
    ARG_CHECK(c && outLimbIdx && tab && out, "fhe_sr_plan_create: null argument");
    // (the 128-bit sums of the kernel hold sizeI + 1 products of residues below 2^60: 2^8 terms — as the reference's DoubleNativeInt sums)
    ARG_CHECK(sizeI >= 1 && sizeO >= 1 && sizeI < (uint32_t)kMaxLimbs && sizeO <= (uint32_t)kMaxLimbs, "fhe_sr_plan_create: bad basis size");
    RT_CHECK(rt::set_device(c->device));
    std::vector<uint64_t> o(sizeO), mu(2 * (size_t)sizeO);
    for (uint32_t j = 0; j < sizeO; ++j) {
        ARG_CHECK(outLimbIdx[j] < c->L, "fhe_sr_plan_create: limb index exceeds context size");
        o[j] = c->q[outLimbIdx[j]];
        host::mu128(o[j], &mu[2 * j]);
    }
    fhe_sr_plan* p = new fhe_sr_plan;
    p->ctx = c, p->sizeI = sizeI, p->sizeO = sizeO, p->exact = frac != nullptr;
    fhe_status s;
    if ((s = dev_copy(&p->owned, tab, (size_t)sizeO * (sizeI + 1), &p->d_tab)) || (s = dev_copy(&p->owned, o.data(), o.size(), &p->d_o)) ||
        (s = dev_copy(&p->owned, mu.data(), mu.size(), &p->d_mu)) || (frac && (s = dev_copy(&p->owned, frac, sizeI, &p->d_frac)))) {
        fhe_sr_plan_destroy(p);
        return s;
    }
    *out = p;
    return FHE_OK;
}
extern "C" void fhe_sr_plan_destroy(fhe_sr_plan* p) {
    if (!p)
        return;
    for (void* q : p->owned)
        rt::dfree(q);
    delete p;
}
extern "C" fhe_status fhe_scale_and_round(fhe_sr_plan* p, const uint64_t* x, int outputFirst, uint64_t* out, uint32_t batch,
                                          void* st) {
    ARG_CHECK(p && x && out && batch >= 1, "fhe_scale_and_round: bad argument");
    RT_CHECK(rt::set_device(p->ctx->device));
    ScaleRoundArgs g;
    const uint32_t tot = p->sizeI + p->sizeO;
    uint64_t* xm       = const_cast<uint64_t*>(x);
    g.in  = TowerView{xm, tot, outputFirst ? p->sizeO : 0u};   // inputIndex  (:1527-1534)
    g.own = TowerView{xm, tot, outputFirst ? 0u : p->sizeI};   // outputIndex
    g.out = TowerView{out, p->sizeO, 0};
    g.tab = p->d_tab, g.frac = p->d_frac, g.o = p->d_o, g.mu = p->d_mu;
    g.logN = p->ctx->logN, g.batch = batch, g.sizeI = p->sizeI, g.sizeO = p->sizeO;
    const uint32_t grid = (uint32_t)((((uint64_t)batch << g.logN) + kThreads - 1) / kThreads);
    if (p->exact)
        FHE_LAUNCH((scale_round_kernel<true>), grid, st, g);
    else
        FHE_LAUNCH((scale_round_kernel<false>), grid, st, g);
    LAUNCH_CHECK();
    return FHE_OK;
}
extern "C" fhe_status fhe_scale_and_round_p_over_q(fhe_ctx* c, const uint64_t* x, const uint32_t* limbIdx, uint32_t sizeQ,
                                                   uint64_t* out, uint32_t batch, void* st) {
    ARG_CHECK(c && x && limbIdx && out && batch >= 1 && sizeQ >= 1 && sizeQ < (uint32_t)kMaxLimbs,
              "fhe_scale_and_round_p_over_q: bad argument");
    for (uint32_t i = 0; i <= sizeQ; ++i)
        ARG_CHECK(limbIdx[i] < c->L, "fhe_scale_and_round_p_over_q: limb index exceeds context size");
    RT_CHECK(rt::set_device(c->device));
    ARG_CHECK(sizeQ <= (uint32_t)kMaxPOverQ, "fhe_scale_and_round_p_over_q: at most 64 limbs supported");
    const uint64_t pLast = c->q[limbIdx[sizeQ]];
    POverQArgs g;
    for (uint32_t i = 0; i < (uint32_t)kMaxPOverQ; ++i)
        g.q[i] = 1, g.pInv[i] = TwPair{0, 0};
    for (uint32_t i = 0; i < sizeQ; ++i) {
        const uint64_t qi = c->q[limbIdx[i]], inv = host::invmod(pLast % qi, qi);  // pInvModq
        g.q[i]    = qi;
        g.pInv[i] = TwPair{inv, host::shoup(inv, qi)};
    }
    g.x = TowerView{const_cast<uint64_t*>(x), sizeQ + 1, 0}, g.out = TowerView{out, sizeQ, 0};
    g.pLast = pLast, g.logN = c->logN, g.batch = batch, g.sizeQ = sizeQ;
    FHE_LAUNCH(p_over_q_kernel, (uint32_t)((((uint64_t)batch << g.logN) + kThreads - 1) / kThreads), st, g);
    LAUNCH_CHECK();
    return FHE_OK;
}

// DCRTPolyImpl::ScaleAndRound -> NativePoly mod t (dcrtpoly-impl.h:1190-1467, BFV HPS decryption) with the caller's
// tables tQHatInvModqDivqModt / tQHatInvModqBDivqModt / tQHatInvModqDivqFrac / tQHatInvModqDivqBFrac; the branch the
// reference takes depends only on (max q_i, t, sizeQ) and is selected here with its own conditions.
static uint32_t msb64(uint64_t v) {
    uint32_t n = 0;
    while (v)
        ++n, v >>= 1;
    return n;
}
static fhe_status native_tables(fhe_ctx* c, uint32_t sizeQ, const uint64_t* a, const uint64_t* b, const uint64_t* modA,
                                const uint64_t* modB, std::vector<TwPair>& h) {
    h.assign(2 * (size_t)sizeQ, TwPair{0, 0});
    for (uint32_t i = 0; i < sizeQ; ++i) {
        h[i] = TwPair{a[i], host::shoup(a[i], modA[i])};  // PrepModMulConst: table values are residues of their modulus
        if (b)
            h[sizeQ + i] = TwPair{b[i], host::shoup(b[i], modB[i])};
    }
    (void)c;
    return FHE_OK;
}
extern "C" fhe_status fhe_scale_and_round_native(fhe_ctx* c, const uint64_t* x, const uint32_t* limbIdx, uint32_t sizeQ,
                                                 uint64_t t, const uint64_t* tabModt, const uint64_t* tabBModt,
                                                 const double* frac, const double* bfrac, uint32_t batch, uint64_t* out,
                                                 void* st) {
    ARG_CHECK(c && x && tabModt && frac && out && batch >= 1, "fhe_scale_and_round_native: bad argument");
    ARG_CHECK(sizeQ >= 1 && sizeQ <= (uint32_t)kMaxLimbs && t >= 2, "fhe_scale_and_round_native: bad basis size or t");
    RT_CHECK(rt::set_device(c->device));
    uint64_t qmax = 0;
    for (uint32_t i = 0; i < sizeQ; ++i) {
        const uint32_t l = limbIdx ? limbIdx[i] : i;
        ARG_CHECK(l < c->L, "fhe_scale_and_round_native: limb index exceeds context size");
        qmax = std::max(qmax, c->q[l]);
    }
    ScaleRoundNativeArgs g;
    const uint32_t qMSB = msb64(qmax), tMSB = msb64(t), sizeQMSB = msb64(sizeQ);
    g.qMSBHf = qMSB >> 1;
    g.pow2   = (t & (t - 1)) == 0 ? 1u : 0u;
    g.split  = (qMSB + sizeQMSB < 52) ? 0u : 1u;
    if (!g.split)
        g.nomod = g.pow2 ? (qMSB + sizeQMSB + tMSB < 63) : (qMSB + tMSB + sizeQMSB < 52);
    else
        g.nomod = g.pow2 ? (g.qMSBHf + tMSB + sizeQMSB < 62) : (g.qMSBHf + tMSB + sizeQMSB < 52);
    ARG_CHECK(!g.split || (tabBModt && bfrac), "fhe_scale_and_round_native: this (q, t, sizeQ) needs the B tables");
    std::vector<uint64_t> tv(sizeQ, t);
    std::vector<TwPair> h;
    native_tables(c, sizeQ, tabModt, g.split ? tabBModt : nullptr, tv.data(), tv.data(), h);
    std::vector<double> fr(2 * (size_t)sizeQ, 0.0);
    for (uint32_t i = 0; i < sizeQ; ++i) {
        fr[i] = frac[i];
        if (g.split)
            fr[sizeQ + i] = bfrac[i];
    }
    void *dT = nullptr, *dF = nullptr;
    RT_CHECK(rt::dmalloc(&dT, h.size() * sizeof(TwPair)));
    RT_CHECK(rt::dmalloc(&dF, fr.size() * sizeof(double)));
    RT_CHECK(rt::h2d(dT, h.data(), h.size() * sizeof(TwPair), (rt::stream_t)st));
    RT_CHECK(rt::h2d(dF, fr.data(), fr.size() * sizeof(double), (rt::stream_t)st));
    g.in = TowerView{const_cast<uint64_t*>(x), sizeQ, 0};
    g.out = out, g.q = nullptr;
    g.tabModt = (TwPair*)dT, g.tabBModt = (TwPair*)dT + sizeQ;
    g.frac = (double*)dF, g.bfrac = (double*)dF + sizeQ;
    g.t = t, g.logN = c->logN, g.batch = batch, g.sizeQ = sizeQ;
    FHE_LAUNCH(scale_round_native_kernel, (uint32_t)((((uint64_t)batch << g.logN) + kThreads - 1) / kThreads), st, g);
    const char* le = rt::last_launch_error();
    RT_CHECK(rt::sync((rt::stream_t)st));  // decryption is a once-per-result call: tables live for this call only
    rt::dfree(dT), rt::dfree(dF);
    RT_CHECK(le);
    return FHE_OK;
}
// DCRTPolyImpl::ScaleAndRound, BEHZ decryption overload (dcrtpoly-impl.h:1631-1671): tables tgammaQHatModq (mod q_i) and
// negInvqModtgamma (mod t*gamma, gamma = 2^26)
extern "C" fhe_status fhe_scale_and_round_behz_decrypt(fhe_ctx* c, const uint64_t* x, const uint32_t* limbIdx, uint32_t sizeQ,
                                                       uint64_t tgamma, const uint64_t* tgammaQHatModq,
                                                       const uint64_t* negInvqModtgamma, uint32_t batch, uint64_t* out,
                                                       void* st) {
    ARG_CHECK(c && x && tgammaQHatModq && negInvqModtgamma && out && batch >= 1, "fhe_scale_and_round_behz_decrypt: bad argument");
    ARG_CHECK(sizeQ >= 1 && sizeQ <= (uint32_t)kMaxLimbs && tgamma >= 2, "fhe_scale_and_round_behz_decrypt: bad basis size or t*gamma");
    RT_CHECK(rt::set_device(c->device));
    std::vector<uint64_t> qv(sizeQ), tg(sizeQ, tgamma);
    for (uint32_t i = 0; i < sizeQ; ++i) {
        const uint32_t l = limbIdx ? limbIdx[i] : i;
        ARG_CHECK(l < c->L, "fhe_scale_and_round_behz_decrypt: limb index exceeds context size");
        qv[i] = c->q[l];
    }
    std::vector<TwPair> h;
    native_tables(c, sizeQ, tgammaQHatModq, negInvqModtgamma, qv.data(), tg.data(), h);
    void *dT = nullptr, *dQ = nullptr;
    RT_CHECK(rt::dmalloc(&dT, h.size() * sizeof(TwPair)));
    RT_CHECK(rt::dmalloc(&dQ, qv.size() * 8));
    RT_CHECK(rt::h2d(dT, h.data(), h.size() * sizeof(TwPair), (rt::stream_t)st));
    RT_CHECK(rt::h2d(dQ, qv.data(), qv.size() * 8, (rt::stream_t)st));
    ScaleRoundNativeArgs g{};
    g.in = TowerView{const_cast<uint64_t*>(x), sizeQ, 0};
    g.out = out, g.q = (uint64_t*)dQ;
    g.tabModt = (TwPair*)dT, g.tabBModt = (TwPair*)dT + sizeQ;
    g.t = tgamma, g.logN = c->logN, g.batch = batch, g.sizeQ = sizeQ;
    FHE_LAUNCH(scale_round_behz_decrypt_kernel, (uint32_t)((((uint64_t)batch << g.logN) + kThreads - 1) / kThreads), st, g);
    const char* le = rt::last_launch_error();
    RT_CHECK(rt::sync((rt::stream_t)st));
    rt::dfree(dT), rt::dfree(dQ);
    RT_CHECK(le);
    return FHE_OK;
}

// ---- decryption on the device (decrypt_kernels.h) ----
// PKERNS::DecryptCore (rns-pke.cpp:199-225), CKKS's `b += noise` and the element arithmetic of MultipartyDecryptLead / Main
// (rns-multiparty.cpp:46-171) for any number of ciphertexts: ONE launch of decrypt_combine_kernel.  ns mod q_i goes through the context's
// table cache (const_table), as the encrypt combine's table does.
struct DecryptOperands {
    const uint64_t* const* c;  // host array [nElem]
    uint32_t nElem;
    const uint64_t *s, *noise;
    uint64_t ns;
    bool withC0;
    uint64_t* out;
};
static uint32_t decrypt_chunk_for(const fhe_ctx* c, uint32_t nLimbs, uint32_t batch) {
    return decrypt_chunk((uint64_t)nLimbs * encrypt_tiles(c), batch, 4ull * (c->cus ? c->cus : 256));
}
// every check of the combine, before anything is enqueued
static fhe_status decrypt_check(const std::string& who, const fhe_ctx* c, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch,
                                const DecryptOperands& o) {
    ARG_CHECK(c && o.c && o.s && o.out, who + ": null argument");
    ARG_CHECK(o.nElem >= 2 && o.nElem <= (uint32_t)kDecryptMaxElems, who + ": a ciphertext of 2 to 4 elements expected");
    ARG_CHECK(o.withC0 || o.nElem == 2, who + ": without c0 (MultipartyDecryptMain) a ciphertext has 2 elements");
    for (uint32_t e = o.withC0 ? 0 : 1; e < o.nElem; ++e)
        ARG_CHECK(o.c[e], who + ": null argument");
    ARG_CHECK(batch >= 1, who + ": batch must be >= 1");
    ARG_CHECK(nLimbs >= 1 && nLimbs <= (uint32_t)kMaxLimbs, who + ": nLimbs out of range");
    for (uint32_t i = 0; i < nLimbs; ++i)
        ARG_CHECK((limbIdx ? limbIdx[i] : i) < c->L, who + ": limb index exceeds context size");
    ARG_CHECK(!(o.noise && o.ns == 0), who + ": the noise scale must not be zero");
    ARG_CHECK((uint64_t)batch * nLimbs * encrypt_tiles(c) < ((uint64_t)1 << 31), who + ": batch * nLimbs too large");
    const size_t row = (size_t)c->N * 8, key = nLimbs * row, slab = (size_t)batch * key;
    ARG_CHECK(!keygen_overlap(o.out, slab, o.s, key), who + ": out overlaps s");
    for (uint32_t e = o.withC0 ? 0 : 1; e < o.nElem; ++e)
        ARG_CHECK((e == 0 && o.out == o.c[0]) || !keygen_overlap(o.out, slab, o.c[e], slab),
                  who + ": out may be c[0] itself but not overlap an element otherwise");
    ARG_CHECK(!o.noise || o.out == o.noise || !keygen_overlap(o.out, slab, o.noise, slab),
              who + ": out may be the noise tower itself but not overlap it otherwise");
    return FHE_OK;
}
// (the arguments have passed decrypt_check)
static fhe_status decrypt_combine_run(const std::string& who, fhe_ctx* c, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch,
                                      const DecryptOperands& o, void* st) {
    DecryptArgs g;
    if (fhe_status s = make_sel(c, limbIdx, nLimbs, &g.sel, who.c_str()))
        return s;
    RT_CHECK(rt::set_device(c->device));
    std::vector<uint32_t> li;
    std::vector<uint64_t> v;
    bool ns1 = true;  // ns = 1 modulo every limb in use: no product at all
    for (uint32_t i = 0; i < nLimbs; ++i) {
        const uint32_t l = limbIdx ? limbIdx[i] : i;
        li.push_back(l);
        v.push_back(o.ns % c->q[l]);
        ns1 = ns1 && v.back() == 1;
    }
    const TwPair* table = nullptr;
    if (fhe_status s = const_tables_trim(c))
        return s;
    std::shared_lock<std::shared_mutex> gate(c->constTabsGate);
    if (o.noise && !ns1)
        if (fhe_status s = const_table(c, li.data(), v.data(), (uint32_t)v.size(), &table))
            return s;
    for (uint32_t e = 0; e < (uint32_t)kDecryptMaxElems; ++e)
        g.c[e] = e < o.nElem && o.c[e] ? o.c[e] : o.c[1];
    g.out = o.out, g.s = o.s, g.noise = o.noise, g.lc = c->d_lc, g.tab = table;
    g.logN = c->logN, g.nLimbs = nLimbs, g.batch = batch;
    g.chunk             = decrypt_chunk_for(c, nLimbs, batch);
    const uint32_t grid = ((batch + g.chunk - 1) / g.chunk) * nLimbs * encrypt_tiles(c);
    const int noise     = !o.noise ? kDecryptNoNoise : ns1 ? kDecryptNoiseNs1 : kDecryptNoiseScaled;
#define DECRYPT_LAUNCH(NELEM, C0)                                                                       \
    do {                                                                                                \
        if (noise == kDecryptNoNoise)                                                                   \
            FHE_LAUNCH((decrypt_combine_kernel<NELEM, C0, kDecryptNoNoise>), grid, st, g);              \
        else if (noise == kDecryptNoiseNs1)                                                             \
            FHE_LAUNCH((decrypt_combine_kernel<NELEM, C0, kDecryptNoiseNs1>), grid, st, g);             \
        else                                                                                            \
            FHE_LAUNCH((decrypt_combine_kernel<NELEM, C0, kDecryptNoiseScaled>), grid, st, g);          \
    } while (0)
    if (!o.withC0)
        DECRYPT_LAUNCH(2, false);
    else if (o.nElem == 2)
        DECRYPT_LAUNCH(2, true);
    else if (o.nElem == 3)
        DECRYPT_LAUNCH(3, true);
    else
        DECRYPT_LAUNCH(4, true);
#undef DECRYPT_LAUNCH
    LAUNCH_CHECK();
    return FHE_OK;
}
extern "C" uint32_t fhe_decrypt_chunk(const fhe_ctx* c, uint32_t nLimbs, uint32_t batch) {
    return c && nLimbs && batch ? decrypt_chunk_for(c, nLimbs, batch) : 0;
}
extern "C" fhe_status fhe_decrypt_core(fhe_ctx* c, const uint64_t* const* ct, uint32_t nElem, const uint64_t* s, const uint32_t* limbIdx,
                                       uint32_t nLimbs, uint32_t batch, const uint64_t* noise, uint64_t ns, int withC0, int outFormat,
                                       uint64_t* out, void* st) {
    const std::string who = "fhe_decrypt_core";
    const DecryptOperands o{ct, nElem, s, noise, ns, withC0 != 0, out};
    if (fhe_status r = decrypt_check(who, c, limbIdx, nLimbs, batch, o))
        return r;
    ARG_CHECK(outFormat == 0 || outFormat == 1, who + ": outFormat is 0 (EVALUATION) or 1 (COEFFICIENT)");
    if (fhe_status r = decrypt_combine_run(who, c, limbIdx, nLimbs, batch, o, st))
        return r;
    return outFormat == 1 ? fhe_ntt_inv(c, out, limbIdx, nLimbs, batch, st) : FHE_OK;
}

// PKEBFVRNS::Decrypt at sizeQl == sizeQ (bfvrns-pke.cpp:215-245) as a plan: the tables of CryptoParametersBFVRNS's "Decrypt : ScaleAndRound"
// block (bfvrns-cryptoparameters.cpp:434-484) or of its BEHZ "Decrns" block (:851-882), derived here from the moduli and t and kept on the
// device, so that a call is the combine, one inverse transform and one launch of the scaling kernel, with no allocation and no wait.
struct fhe_bfv_dec {
    fhe_ctx* ctx;
    uint32_t sizeQ;
    int technique;
    std::vector<uint32_t> idx;
    ScaleRoundNativeArgs g;  // everything but in, out and batch
    std::map<int, std::vector<uint64_t>> tables;
    std::vector<void*> owned;
};
namespace {
// a^-1 mod m for any m > 1 with gcd(a, m) = 1 (extended Euclid; 0 when there is none)
uint64_t inv_mod_any(uint64_t a, uint64_t m) {
    __int128 r0 = m, r1 = a % m, t0 = 0, t1 = 1;
    while (r1) {
        const __int128 qq = r0 / r1, r2 = r0 - qq * r1, t2 = t0 - qq * t1;
        r0 = r1, r1 = r2, t0 = t1, t1 = t2;
    }
    if (r0 != 1)
        return 0;
    return (uint64_t)(t0 < 0 ? t0 + m : t0);
}
uint64_t double_bits(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    return u;
}
}  // namespace
extern "C" void fhe_bfv_decrypt_destroy(fhe_bfv_dec* p) {
    if (!p)
        return;
    for (void* q : p->owned)
        rt::dfree(q);
    delete p;
}
extern "C" fhe_status fhe_bfv_decrypt_create(fhe_ctx* c, const uint32_t* limbIdx, uint32_t sizeQ, uint64_t t, int technique,
                                             fhe_bfv_dec** out) {
    const std::string who = "fhe_bfv_decrypt_create";
    ARG_CHECK(c && out, who + ": null argument");
    ARG_CHECK(technique >= 0 && technique <= 3, who + ": technique must be BEHZ (0), HPS (1), HPSPOVERQ (2) or HPSPOVERQLEVELED (3)");
    ARG_CHECK(sizeQ >= 1 && sizeQ <= (uint32_t)kMaxLimbs, who + ": sizeQ out of range");
    ARG_CHECK(t >= 2, who + ": bad plaintext modulus");
    std::vector<uint64_t> q(sizeQ);
    std::vector<uint32_t> idx(sizeQ);
    for (uint32_t i = 0; i < sizeQ; ++i) {
        idx[i] = limbIdx ? limbIdx[i] : i;
        ARG_CHECK(idx[i] < c->L, who + ": limb index exceeds context size");
        q[i] = c->q[idx[i]];
        for (uint32_t k = 0; k < i; ++k)
            ARG_CHECK(q[k] != q[i], who + ": the moduli of a tower must be distinct");
    }
    const uint64_t gamma = 1ull << 26;  // m_gamma (bfvrns-cryptoparameters.cpp:851-857: t * gamma < 2^58)
    if (technique == 0 && t >= (1ull << 32))
        return fail(FHE_ERR_UNSUPPORTED, who + ": BEHZ decryption needs t * 2^26 < 2^58");
    RT_CHECK(rt::set_device(c->device));
    fhe_bfv_dec* p = new fhe_bfv_dec;
    p->ctx = c, p->sizeQ = sizeQ, p->technique = technique, p->idx = idx;
    ScaleRoundNativeArgs& g = p->g;
    g = ScaleRoundNativeArgs{};
    g.logN = c->logN, g.sizeQ = sizeQ;
    std::vector<TwPair> h(2 * (size_t)sizeQ, TwPair{0, 0});
    fhe_status s = FHE_OK;
    if (technique != 0) {
        const uint64_t qmax = *std::max_element(q.begin(), q.end());
        const uint32_t qMSB = msb64(qmax), tMSB = msb64(t), sizeQMSB = msb64(sizeQ);
        g.t = t, g.qMSBHf = qMSB >> 1;
        g.pow2  = (t & (t - 1)) == 0 ? 1u : 0u;
        g.split = (qMSB + sizeQMSB < 52) ? 0u : 1u;
        if (!g.split)
            g.nomod = g.pow2 ? (qMSB + sizeQMSB + tMSB < 63) : (qMSB + tMSB + sizeQMSB < 52);
        else
            g.nomod = g.pow2 ? (g.qMSBHf + tMSB + sizeQMSB < 62) : (g.qMSBHf + tMSB + sizeQMSB < 52);
        std::vector<uint64_t> modt(sizeQ), frac(sizeQ), bmodt, bfrac;
        std::vector<double> fr(2 * (size_t)sizeQ, 0.0);
        if (g.split)
            bmodt.resize(sizeQ), bfrac.resize(sizeQ);
        for (uint32_t i = 0; i < sizeQ; ++i) {
            // v = t * [(Q/q_i)^-1]_{q_i} = a * q_i + r, below 2^124
            const uint64_t qi   = q[i];
            const host::u128 v  = (host::u128)host::invmod(host::prod_mod(q, (int)i, qi), qi) * t;
            const host::u128 a  = v / qi;
            const uint64_t r    = (uint64_t)(v % qi);
            modt[i]             = (uint64_t)(a % t);
            fr[i]               = static_cast<double>((int64_t)r) / static_cast<double>((int64_t)qi);  // :454-456
            frac[i]             = double_bits(fr[i]);
            h[i]                = TwPair{modt[i], host::shoup(modt[i], t)};
            if (g.split) {  // (v << qMSBHf) = (a << qMSBHf) * q_i + (r << qMSBHf), r << qMSBHf below 2^90
                const host::u128 rs = (host::u128)r << g.qMSBHf;
                const uint64_t hi   = host::mulmod((uint64_t)(a % t), host::powmod(2, g.qMSBHf, t), t);
                bmodt[i]            = (uint64_t)(((host::u128)hi + (uint64_t)((rs / qi) % t)) % t);
                fr[sizeQ + i]       = static_cast<double>((int64_t)(uint64_t)(rs % qi)) / static_cast<double>((int64_t)qi);  // :481-482
                bfrac[i]            = double_bits(fr[sizeQ + i]);
                h[sizeQ + i]        = TwPair{bmodt[i], host::shoup(bmodt[i], t)};
            }
        }
        p->tables[0] = modt, p->tables[2] = frac;
        if (g.split)
            p->tables[1] = bmodt, p->tables[3] = bfrac;
        double* dF = nullptr;
        s          = dev_copy(&p->owned, fr.data(), fr.size(), &dF);
        g.frac = dF, g.bfrac = dF ? dF + sizeQ : nullptr;
    } else {
        const uint64_t tgamma = t * gamma;
        g.t                   = tgamma;
        std::vector<uint64_t> a(sizeQ), b(sizeQ);
        for (uint32_t i = 0; i < sizeQ; ++i) {
            const uint64_t qi = q[i], inv = inv_mod_any(qi % tgamma, tgamma);
            if (!inv) {
                fhe_bfv_decrypt_destroy(p);
                return fail(FHE_ERR_ARG, who + ": every modulus must be invertible modulo t * 2^26");
            }
            b[i] = host::mulmod(tgamma - 1, inv, tgamma);  // [-1/q_i]_{t*gamma}, :857-867
            a[i] = host::mulmod(host::mulmod(host::invmod(host::prod_mod(q, (int)i, qi), qi), gamma % qi, qi), t % qi, qi);  // :869-882
            h[i] = TwPair{a[i], host::shoup(a[i], qi)}, h[sizeQ + i] = TwPair{b[i], host::shoup(b[i], tgamma)};
        }
        p->tables[4] = std::vector<uint64_t>(1, tgamma), p->tables[5] = a, p->tables[6] = b;
        uint64_t* dQ = nullptr;
        s            = dev_copy(&p->owned, q.data(), q.size(), &dQ);
        g.q          = dQ;
    }
    TwPair* dT = nullptr;
    if (!s)
        s = dev_copy(&p->owned, h.data(), h.size(), &dT);
    if (s) {
        fhe_bfv_decrypt_destroy(p);
        return s;
    }
    g.tabModt = dT, g.tabBModt = dT + sizeQ;
    *out = p;
    return FHE_OK;
}
// ids: 0 tQHatInvModqDivqModt, 1 tQHatInvModqBDivqModt, 2 tQHatInvModqDivqFrac, 3 tQHatInvModqBDivqFrac (doubles, as their 64 bits),
// 4 tgamma (one word), 5 tgammaQHatInvModq, 6 negInvqModtgamma; [sizeQ] each.  Returns the number of words of the table (0: no such table for
// this plan: the B tables on the unsplit branch, the other technique's); copies min(that, cap) words into out.
extern "C" size_t fhe_bfv_decrypt_table(const fhe_bfv_dec* p, int tableId, uint64_t* out, size_t cap) {
    if (!p)
        return 0;
    auto it = p->tables.find(tableId);
    if (it == p->tables.end())
        return 0;
    if (out && cap)
        std::memcpy(out, it->second.data(), std::min(cap, it->second.size()) * 8);
    return it->second.size();
}
extern "C" size_t fhe_bfv_decrypt_workspace_bytes(const fhe_bfv_dec* p, uint32_t batch) {
    return p ? (((size_t)batch * p->sizeQ) << p->ctx->logN) * 8 : 0;
}
// the scaling kernel on a COEFFICIENT b [batch][sizeQ][N]
static fhe_status bfv_decrypt_tail(const fhe_bfv_dec* p, const uint64_t* b, uint32_t batch, uint64_t* out, void* st) {
    ScaleRoundNativeArgs g = p->g;
    g.in = TowerView{const_cast<uint64_t*>(b), p->sizeQ, 0}, g.out = out, g.batch = batch;
    const uint32_t grid = (uint32_t)((((uint64_t)batch << g.logN) + kThreads - 1) / kThreads);
    if (p->technique != 0)
        FHE_LAUNCH(scale_round_native_kernel, grid, st, g);
    else
        FHE_LAUNCH(scale_round_behz_decrypt_kernel, grid, st, g);
    LAUNCH_CHECK();
    return FHE_OK;
}
extern "C" fhe_status fhe_bfv_decrypt(fhe_bfv_dec* p, const uint64_t* const* ct, uint32_t nElem, const uint64_t* s, uint32_t batch,
                                      uint64_t* out, void* wsv, size_t wsBytes, void* st) {
    const std::string who = "fhe_bfv_decrypt";
    ARG_CHECK(p && out && wsv, who + ": null argument");
    fhe_ctx* c = p->ctx;
    uint64_t* b = (uint64_t*)wsv;
    const DecryptOperands o{ct, nElem, s, nullptr, 1, true, b};
    if (fhe_status r = decrypt_check(who, c, p->idx.data(), p->sizeQ, batch, o))
        return r;
    const size_t slab = fhe_bfv_decrypt_workspace_bytes(p, batch), res = ((size_t)batch << c->logN) * 8;
    ARG_CHECK(wsBytes >= slab, who + ": workspace too small");
    ARG_CHECK(!keygen_overlap(out, res, b, slab) && !keygen_overlap(out, res, s, slab / batch), who + ": out overlaps the workspace or s");
    for (uint32_t e = 0; e < nElem; ++e)
        ARG_CHECK(!keygen_overlap(out, res, ct[e], slab) && ct[e] != b, who + ": out or the workspace overlaps an element");
    RT_CHECK(rt::set_device(c->device));
    if (fhe_status r = decrypt_combine_run(who, c, p->idx.data(), p->sizeQ, batch, o, st))
        return r;
    if (fhe_status r = fhe_ntt_inv(c, b, p->idx.data(), p->sizeQ, batch, st))  // b.SetFormat(COEFFICIENT), every limb of every tower at once
        return r;
    return bfv_decrypt_tail(p, b, batch, out, st);
}
extern "C" fhe_status fhe_bfv_decrypt_b(fhe_bfv_dec* p, const uint64_t* b, int evalFormat, uint32_t batch, uint64_t* out, void* wsv,
                                        size_t wsBytes, void* st) {
    const std::string who = "fhe_bfv_decrypt_b";
    ARG_CHECK(p && b && out && (wsv || !evalFormat), who + ": null argument");
    ARG_CHECK(batch >= 1, who + ": batch must be >= 1");
    fhe_ctx* c = p->ctx;
    const size_t slab = fhe_bfv_decrypt_workspace_bytes(p, batch), res = ((size_t)batch << c->logN) * 8;
    ARG_CHECK(!keygen_overlap(out, res, b, slab), who + ": out overlaps b");
    RT_CHECK(rt::set_device(c->device));
    if (evalFormat) {
        ARG_CHECK(wsBytes >= slab, who + ": workspace too small");
        ARG_CHECK(!keygen_overlap(wsv, slab, b, slab) && !keygen_overlap(wsv, slab, out, res), who + ": the workspace overlaps b or out");
        if (fhe_status r = fhe_ntt_inv_oop(c, b, (uint64_t*)wsv, p->idx.data(), p->sizeQ, batch, st))
            return r;
        b = (const uint64_t*)wsv;
    }
    return bfv_decrypt_tail(p, b, batch, out, st);
}

// ---- BEHZ ----
struct fhe_behz {
    fhe_ctx* ctx;
    uint32_t numQ, numBsk;
    std::vector<uint32_t> qIdx, bskIdx, allIdx;
    BehzTables tb;
    std::vector<void*> owned;
};
// Bsk = numQ primes below q.back() then m_sk  (bfvrns-cryptoparameters.cpp:682-711)
extern "C" uint32_t fhe_param_behz_bsk(uint32_t logN, uint32_t numQ, const uint64_t* q, uint64_t t, uint64_t* bsk,
                                       uint64_t* psiBsk) {
    if (!q || !bsk || !psiBsk || numQ < 1 || numQ > (uint32_t)kBehzWideLimbs - 1)
        return 0;
    const uint64_t M = 2ull << logN;
    uint64_t cur     = q[numQ - 1];
    for (uint32_t i = 0; i < numQ; ++i) {
        cur    = host::previous_prime(cur, M);
        bsk[i] = cur;
    }
    uint64_t msk = host::previous_prime(bsk[numQ - 1], M);
    uint32_t sb  = host::bitlen(msk);
    auto mulw = [](std::vector<uint64_t>& big, uint64_t m) {
        uint64_t carry = 0;
        for (auto& w : big) {
            host::u128 tt = (host::u128)w * m + carry;
            w             = (uint64_t)tt;
            carry         = (uint64_t)(tt >> 64);
        }
        if (carry)
            big.push_back(carry);
    };
    auto less = [](const std::vector<uint64_t>& a, const std::vector<uint64_t>& b) {
        if (a.size() != b.size())
            return a.size() < b.size();
        for (size_t k = a.size(); k-- > 0;)
            if (a[k] != b[k])
                return a[k] < b[k];
        return false;
    };
    std::vector<uint64_t> rhs(1, 1);
    mulw(rhs, M);
    mulw(rhs, t);
    for (uint32_t i = 0; i < numQ; ++i)
        mulw(rhs, q[i]);
    for (;;) {
        std::vector<uint64_t> lhs(1, 1);
        for (uint32_t i = 0; i < numQ; ++i)
            mulw(lhs, bsk[i]);
        mulw(lhs, msk);
        if (!less(lhs, rhs))
            break;
        if (++sb > 60)
            return 0;  // the reference throws: requested bit length exceeds MAX_MODULUS_SIZE
        msk = host::next_prime(host::first_prime(sb, M), M);
    }
    bsk[numQ] = msk;
    for (uint32_t i = 0; i <= numQ; ++i)
        psiBsk[i] = host::min_root_of_unity(M, bsk[i]);
    return numQ + 1;
}

extern "C" fhe_status fhe_behz_create(fhe_ctx* c, const uint32_t* qLimbIdx, uint32_t numQ, const uint32_t* bskLimbIdx,
                                      uint64_t t, fhe_behz** out) {
    ARG_CHECK(c && qLimbIdx && bskLimbIdx && out, "fhe_behz_create: null argument");
    ARG_CHECK(numQ >= 1 && numQ + 1 <= (uint32_t)kBehzWideLimbs, "fhe_behz_create: at most 127 Q limbs supported");
    const uint32_t numB = numQ, numBsk = numQ + 1;
    std::vector<uint64_t> q(numQ), bsk(numBsk);
    for (uint32_t i = 0; i < numQ; ++i) {
        ARG_CHECK(qLimbIdx[i] < c->L, "fhe_behz_create: limb index exceeds context size");
        q[i] = c->q[qLimbIdx[i]];
    }
    for (uint32_t j = 0; j < numBsk; ++j) {
        ARG_CHECK(bskLimbIdx[j] < c->L, "fhe_behz_create: limb index exceeds context size");
        bsk[j] = c->q[bskLimbIdx[j]];
    }
    RT_CHECK(rt::set_device(c->device));
    const uint64_t mtilde = 1ull << 16, msk = bsk[numB];
    std::vector<uint64_t> B(bsk.begin(), bsk.begin() + numB);
    // vectors padded to W, matrices stored [target][W]: 16 for the register-resident kernels, kBehzWideLimbs above 15 Q limbs (bfv_kernels.h)
    const size_t W = numBsk <= (uint32_t)kMaxBfvLimbs ? (size_t)kMaxBfvLimbs : (size_t)kBehzWideLimbs;
    std::vector<uint64_t> muQ(2 * W, 0), muBsk(2 * W, 0), QHatModbsk(W * numBsk, 0), QHatModmt(W, 0), qInvModbsk(W * numBsk, 0),
        BHatModmsk(W, 0), BHatModq(W * numQ, 0), qPad(W, 1), bskPad(W, 1);
    std::vector<TwPair> mtQHatInv(W, TwPair{0, 0}), tQHatInv(W, TwPair{0, 0}), BModq(W, TwPair{0, 0}), QModbsk(W, TwPair{0, 0}),
        mtInvModbsk(W, TwPair{0, 0}), tQInvModbsk(W, TwPair{0, 0}), BHatInv(W, TwPair{0, 0});
    std::copy(q.begin(), q.end(), qPad.begin());
    std::copy(bsk.begin(), bsk.end(), bskPad.begin());
    auto pair = [](uint64_t v, uint64_t m) { return TwPair{v, host::shoup(v, m)}; };
    for (uint32_t i = 0; i < numQ; ++i) {
        const uint64_t qi = q[i], hatInv = host::invmod(host::prod_mod(q, (int)i, qi), qi);
        tQHatInv[i]  = pair(host::mulmod(hatInv, t % qi, qi), qi);        // :722-733
        mtQHatInv[i] = pair(host::mulmod(hatInv, mtilde % qi, qi), qi);   // :755-768
        for (uint32_t j = 0; j < numBsk; ++j) {
            QHatModbsk[(size_t)j * W + i] = host::prod_mod(q, (int)i, bsk[j]);         // :735-747
            qInvModbsk[(size_t)j * W + i] = host::invmod(qi % bsk[j], bsk[j]);          // :749-755
        }
        uint64_t v = 1;
        for (uint32_t k = 0; k < numQ; ++k)
            if (k != i)
                v = (v * (q[k] & (mtilde - 1))) & (mtilde - 1);
        QHatModmt[i] = v;
        BModq[i]     = pair(host::prod_mod(B, -1, qi), qi);                // :838-845
        host::mu128(qi, &muQ[2 * i]);
    }
    uint64_t Qm = 1;
    for (uint32_t k = 0; k < numQ; ++k)
        Qm = (Qm * (q[k] & (mtilde - 1))) & (mtilde - 1);
    uint64_t inv = 1;
    for (int it = 0; it < 5; ++it)
        inv = (inv * (2 - Qm * inv)) & (mtilde - 1);
    for (uint32_t j = 0; j < numBsk; ++j) {
        const uint64_t bj = bsk[j], Qb = host::prod_mod(q, -1, bj);
        QModbsk[j]     = pair(Qb, bj);                                                        // :775-783
        mtInvModbsk[j] = pair(host::invmod(mtilde % bj, bj), bj);                              // :785-793
        tQInvModbsk[j] = pair(host::mulmod(host::invmod(Qb, bj), t % bj, bj), bj);             // :795-804
        host::mu128(bj, &muBsk[2 * j]);
    }
    for (uint32_t i = 0; i < numB; ++i) {
        BHatInv[i]    = pair(host::invmod(host::prod_mod(B, (int)i, B[i]), B[i]), B[i]);       // :806-817
        BHatModmsk[i] = host::prod_mod(B, (int)i, msk);                                      // :829-834
        for (uint32_t j = 0; j < numQ; ++j)
            BHatModq[(size_t)j * W + i] = host::prod_mod(B, (int)i, q[j]);                 // :819-827
    }
    fhe_behz* h = new fhe_behz;
    h->ctx = c, h->numQ = numQ, h->numBsk = numBsk;
    h->qIdx.assign(qLimbIdx, qLimbIdx + numQ);
    h->bskIdx.assign(bskLimbIdx, bskLimbIdx + numBsk);
    h->allIdx = h->qIdx;
    h->allIdx.insert(h->allIdx.end(), h->bskIdx.begin(), h->bskIdx.end());
    BehzTables& tb = h->tb;
    tb.numQ = numQ, tb.numBsk = numBsk, tb.W = (uint32_t)W;
    tb.negQInvModmt = ((mtilde - 1) * inv) & (mtilde - 1);                                    // :770-773
    tb.BInvModmsk   = pair(host::invmod(host::prod_mod(B, -1, msk), msk), msk);              // :836-837
    tb.mskMu        = host::barrett_mu(msk);
    tb.mskMsb       = host::bitlen(msk);
    fhe_status s;
    uint64_t *dq, *dbsk, *dmuQ, *dmuB, *d1, *d2, *d3, *d4, *d5;
    TwPair *p1, *p2, *p3, *p4, *p5, *p6, *p7;
    if ((s = dev_copy(&h->owned, qPad.data(), qPad.size(), &dq)) || (s = dev_copy(&h->owned, bskPad.data(), bskPad.size(), &dbsk)) ||
        (s = dev_copy(&h->owned, muQ.data(), muQ.size(), &dmuQ)) || (s = dev_copy(&h->owned, muBsk.data(), muBsk.size(), &dmuB)) ||
        (s = dev_copy(&h->owned, QHatModbsk.data(), QHatModbsk.size(), &d1)) || (s = dev_copy(&h->owned, QHatModmt.data(), QHatModmt.size(), &d2)) ||
        (s = dev_copy(&h->owned, qInvModbsk.data(), qInvModbsk.size(), &d3)) || (s = dev_copy(&h->owned, BHatModmsk.data(), BHatModmsk.size(), &d4)) ||
        (s = dev_copy(&h->owned, BHatModq.data(), BHatModq.size(), &d5)) || (s = dev_copy(&h->owned, mtQHatInv.data(), mtQHatInv.size(), &p1)) ||
        (s = dev_copy(&h->owned, tQHatInv.data(), tQHatInv.size(), &p2)) || (s = dev_copy(&h->owned, BModq.data(), BModq.size(), &p3)) ||
        (s = dev_copy(&h->owned, QModbsk.data(), QModbsk.size(), &p4)) || (s = dev_copy(&h->owned, mtInvModbsk.data(), mtInvModbsk.size(), &p5)) ||
        (s = dev_copy(&h->owned, tQInvModbsk.data(), tQInvModbsk.size(), &p6)) || (s = dev_copy(&h->owned, BHatInv.data(), BHatInv.size(), &p7))) {
        fhe_behz_destroy(h);
        return s;
    }
    tb.q = dq, tb.bsk = dbsk, tb.muQ = dmuQ, tb.muBsk = dmuB, tb.QHatModbsk = d1, tb.QHatModmt = d2, tb.qInvModbsk = d3;
    tb.BHatModmsk = d4, tb.BHatModq = d5, tb.mtQHatInv = p1, tb.tQHatInv = p2, tb.BModq = p3, tb.QModbsk = p4;
    tb.mtInvModbsk = p5, tb.tQInvModbsk = p6, tb.BHatInv = p7;
    *out = h;
    return FHE_OK;
}
extern "C" void fhe_behz_destroy(fhe_behz* h) {
    if (!h)
        return;
    for (void* p : h->owned)
        rt::dfree(p);
    delete h;
}
// The caller's tables in place of the derived ones, per member (the arguments the reference passes to that member, row-major as it
// indexes them).  A DCRTPoly backend receives exactly these vectors from pke (CryptoParametersBFVRNS getters): with an override the
// member computes with the CALLER's values, whatever they are, as the reference's member does.
static fhe_status behz_pairs(fhe_behz* h, const uint64_t* v, const uint64_t* mod, uint32_t n, const TwPair** slot) {
    std::vector<TwPair> t(h->tb.W, TwPair{0, 0});
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t w = v[i] % mod[i];
        t[i]             = TwPair{w, host::shoup(w, mod[i])};
    }
    TwPair* d = nullptr;
    if (fhe_status s = dev_copy(&h->owned, t.data(), t.size(), &d))
        return s;
    *slot = d;
    return FHE_OK;
}
// matrix given as [nRow][nCol] (reference order) -> device [nCol][kMaxBfvLimbs] (one target's weights contiguous)
static fhe_status behz_matrix(fhe_behz* h, const uint64_t* m, uint32_t nRow, uint32_t nCol, const uint64_t* colMod, const uint64_t** slot) {
    const size_t W = h->tb.W;
    std::vector<uint64_t> t(W * nCol, 0);
    for (uint32_t i = 0; i < nRow; ++i)
        for (uint32_t j = 0; j < nCol; ++j)
            t[(size_t)j * W + i] = m[(size_t)i * nCol + j] % colMod[j];
    uint64_t* d = nullptr;
    if (fhe_status s = dev_copy(&h->owned, t.data(), t.size(), &d))
        return s;
    *slot = d;
    return FHE_OK;
}
static void behz_moduli(const fhe_behz* h, std::vector<uint64_t>& q, std::vector<uint64_t>& bsk) {
    q.resize(h->numQ), bsk.resize(h->numBsk);
    for (uint32_t i = 0; i < h->numQ; ++i)
        q[i] = h->ctx->q[h->qIdx[i]];
    for (uint32_t j = 0; j < h->numBsk; ++j)
        bsk[j] = h->ctx->q[h->bskIdx[j]];
}
extern "C" fhe_status fhe_behz_override_q_to_bsk(fhe_behz* h, const uint64_t* mtildeQHatInvModq, const uint64_t* QHatModbsk,
                                                 const uint64_t* QHatModmtilde, const uint64_t* QModbsk, uint64_t negQInvModmtilde,
                                                 const uint64_t* mtildeInvModbsk) {
    ARG_CHECK(h && mtildeQHatInvModq && QHatModbsk && QHatModmtilde && QModbsk && mtildeInvModbsk, "fhe_behz_override_q_to_bsk: null argument");
    RT_CHECK(rt::set_device(h->ctx->device));
    std::vector<uint64_t> q, bsk;
    behz_moduli(h, q, bsk);
    fhe_status s;
    if ((s = behz_pairs(h, mtildeQHatInvModq, q.data(), h->numQ, &h->tb.mtQHatInv)) ||
        (s = behz_matrix(h, QHatModbsk, h->numQ, h->numBsk, bsk.data(), &h->tb.QHatModbsk)) ||
        (s = behz_pairs(h, QModbsk, bsk.data(), h->numBsk, &h->tb.QModbsk)) ||
        (s = behz_pairs(h, mtildeInvModbsk, bsk.data(), h->numBsk, &h->tb.mtInvModbsk)))
        return s;
    std::vector<uint64_t> mt(h->tb.W, 0);
    std::copy(QHatModmtilde, QHatModmtilde + h->numQ, mt.begin());
    uint64_t* d = nullptr;
    if ((s = dev_copy(&h->owned, mt.data(), mt.size(), &d)))
        return s;
    h->tb.QHatModmt    = d;
    h->tb.negQInvModmt = negQInvModmtilde;
    return FHE_OK;
}
extern "C" fhe_status fhe_behz_override_floorq(fhe_behz* h, const uint64_t* tQHatInvModq, const uint64_t* QHatModbsk,
                                               const uint64_t* qInvModbsk, const uint64_t* tQInvModbsk) {
    ARG_CHECK(h && tQHatInvModq && QHatModbsk && qInvModbsk && tQInvModbsk, "fhe_behz_override_floorq: null argument");
    RT_CHECK(rt::set_device(h->ctx->device));
    std::vector<uint64_t> q, bsk;
    behz_moduli(h, q, bsk);
    fhe_status s;
    if ((s = behz_pairs(h, tQHatInvModq, q.data(), h->numQ, &h->tb.tQHatInv)) ||
        (s = behz_matrix(h, QHatModbsk, h->numQ, h->numBsk, bsk.data(), &h->tb.QHatModbsk)) ||
        (s = behz_matrix(h, qInvModbsk, h->numQ, h->numBsk, bsk.data(), &h->tb.qInvModbsk)) ||
        (s = behz_pairs(h, tQInvModbsk, bsk.data(), h->numBsk, &h->tb.tQInvModbsk)))
        return s;
    return FHE_OK;
}
extern "C" fhe_status fhe_behz_override_conv_sk(fhe_behz* h, const uint64_t* BHatInvModb, const uint64_t* BHatModmsk, uint64_t BInvModmsk,
                                                const uint64_t* BHatModq, const uint64_t* BModq) {
    ARG_CHECK(h && BHatInvModb && BHatModmsk && BHatModq && BModq, "fhe_behz_override_conv_sk: null argument");
    RT_CHECK(rt::set_device(h->ctx->device));
    std::vector<uint64_t> q, bsk;
    behz_moduli(h, q, bsk);
    const uint32_t numB = h->numQ;
    const uint64_t msk  = bsk[numB];
    fhe_status s;
    if ((s = behz_pairs(h, BHatInvModb, bsk.data(), numB, &h->tb.BHatInv)) ||
        (s = behz_matrix(h, BHatModq, numB, h->numQ, q.data(), &h->tb.BHatModq)) || (s = behz_pairs(h, BModq, q.data(), h->numQ, &h->tb.BModq)))
        return s;
    std::vector<uint64_t> bm(h->tb.W, 0);
    for (uint32_t i = 0; i < numB; ++i)
        bm[i] = BHatModmsk[i] % msk;
    uint64_t* d = nullptr;
    if ((s = dev_copy(&h->owned, bm.data(), bm.size(), &d)))
        return s;
    h->tb.BHatModmsk = d;
    h->tb.BInvModmsk = TwPair{BInvModmsk % msk, host::shoup(BInvModmsk % msk, msk)};
    return FHE_OK;
}
static bool behz_split30() {  // the BEHZ dot products with 30-bit split factors (default; same knob as the conversion kernel)
    static const bool on = env_u32("FHE_CONV_SUM8", 2) != 1u;
    return on;
}
static uint32_t coeff_grid(const fhe_ctx* c, uint32_t batch) {
    return (uint32_t)((((uint64_t)batch << c->logN) + kThreads - 1) / kThreads);
}
extern "C" size_t fhe_behz_workspace_bytes(const fhe_behz* h, uint32_t batch) {
    return h ? ((size_t)batch * h->numQ << h->ctx->logN) * 8 : 0;
}
// DCRTPolyImpl::FastBaseConvqToBskMontgomery (dcrtpoly-impl.h:1694-1786): x is [batch][numQ+numBsk][N]; on entry its
// first numQ rows hold the input in `evalFormat`; on return ALL rows are in EVALUATION format
extern "C" fhe_status fhe_behz_q_to_bsk(fhe_behz* h, uint64_t* x, int evalFormat, uint32_t batch, void* ws, size_t wsBytes,
                                        void* st) {
    ARG_CHECK(h && x && batch >= 1, "fhe_behz_q_to_bsk: bad argument");
    fhe_ctx* c = h->ctx;
    RT_CHECK(rt::set_device(c->device));
    const uint32_t tot = h->numQ + h->numBsk;
    BehzArgs g;
    g.tb = h->tb, g.logN = c->logN, g.batch = batch;
    g.outBsk = TowerView{x, tot, h->numQ};
    g.inBsk = g.outBsk, g.outQ = TowerView{x, tot, 0};
    if (evalFormat) {
        ARG_CHECK(ws && wsBytes >= fhe_behz_workspace_bytes(h, batch), "fhe_behz_q_to_bsk: workspace too small");
        uint64_t* coef = (uint64_t*)ws;
        NttOpts rows;  // the Q rows of the tot-row towers ...
        rows.src.stride = tot, rows.src.first = 0;
        if (fhe_status s = ntt_run(c, true, x, coef, h->qIdx.data(), h->numQ, batch, st, rows))  // :1708-1712
            return s;
        g.inQ = TowerView{coef, h->numQ, 0};
        if (h->tb.W > (uint32_t)kMaxBfvLimbs)
            FHE_LAUNCH(behz_q_to_bsk_wide_kernel, coeff_grid(c, batch), st, g);
        else if (behz_split30())
            FHE_LAUNCH((behz_q_to_bsk_kernel<true>), coeff_grid(c, batch), st, g);
        else
            FHE_LAUNCH((behz_q_to_bsk_kernel<false>), coeff_grid(c, batch), st, g);
        LAUNCH_CHECK();
        // only the new Bsk limbs go to EVALUATION; the Q limbs keep their original NTT form (:1776-1780)
        rows.dst.stride = tot, rows.src.first = rows.dst.first = h->numQ;  // ... and, in place, their Bsk rows
        return ntt_run(c, false, x, x, h->bskIdx.data(), h->numBsk, batch, st, rows);
    }
    g.inQ = TowerView{x, tot, 0};
    if (h->tb.W > (uint32_t)kMaxBfvLimbs)
        FHE_LAUNCH(behz_q_to_bsk_wide_kernel, coeff_grid(c, batch), st, g);
    else if (behz_split30())
        FHE_LAUNCH((behz_q_to_bsk_kernel<true>), coeff_grid(c, batch), st, g);
    else
        FHE_LAUNCH((behz_q_to_bsk_kernel<false>), coeff_grid(c, batch), st, g);
    LAUNCH_CHECK();
    return fhe_ntt_fwd(c, x, h->allIdx.data(), tot, batch, st);  // every limb to EVALUATION (:1774, :1781-1785)
}
// DCRTPolyImpl::FastRNSFloorq (:1791-1840), in place on x[batch][numQ+numBsk][N] COEFFICIENT
extern "C" fhe_status fhe_behz_floorq(fhe_behz* h, uint64_t* x, uint32_t batch, void* st) {
    ARG_CHECK(h && x && batch >= 1, "fhe_behz_floorq: bad argument");
    RT_CHECK(rt::set_device(h->ctx->device));
    const uint32_t tot = h->numQ + h->numBsk;
    BehzArgs g;
    g.tb = h->tb, g.logN = h->ctx->logN, g.batch = batch;
    g.inQ = g.outQ = TowerView{x, tot, 0};
    g.inBsk = g.outBsk = TowerView{x, tot, h->numQ};
    if (h->tb.W > (uint32_t)kMaxBfvLimbs)
        FHE_LAUNCH(behz_floorq_wide_kernel, coeff_grid(h->ctx, batch), st, g);
    else if (behz_split30())
        FHE_LAUNCH((behz_floorq_kernel<true>), coeff_grid(h->ctx, batch), st, g);
    else
        FHE_LAUNCH((behz_floorq_kernel<false>), coeff_grid(h->ctx, batch), st, g);
    LAUNCH_CHECK();
    return FHE_OK;
}
// DCRTPolyImpl::FastBaseConvSK (:1845-1929): x[batch][numQ+numBsk][N] COEFFICIENT -> out[batch][numQ][N]
extern "C" fhe_status fhe_behz_conv_sk(fhe_behz* h, const uint64_t* x, uint64_t* out, uint32_t batch, void* st) {
    ARG_CHECK(h && x && out && batch >= 1, "fhe_behz_conv_sk: bad argument");
    RT_CHECK(rt::set_device(h->ctx->device));
    const uint32_t tot = h->numQ + h->numBsk;
    BehzArgs g;
    g.tb = h->tb, g.logN = h->ctx->logN, g.batch = batch;
    uint64_t* xm = const_cast<uint64_t*>(x);
    g.inQ = TowerView{xm, tot, 0}, g.inBsk = TowerView{xm, tot, h->numQ};
    g.outQ = TowerView{out, h->numQ, 0}, g.outBsk = g.inBsk;
    if (h->tb.W > (uint32_t)kMaxBfvLimbs)
        FHE_LAUNCH(behz_conv_sk_wide_kernel, coeff_grid(h->ctx, batch), st, g);
    else if (behz_split30())
        FHE_LAUNCH((behz_conv_sk_kernel<true>), coeff_grid(h->ctx, batch), st, g);
    else
        FHE_LAUNCH((behz_conv_sk_kernel<false>), coeff_grid(h->ctx, batch), st, g);
    LAUNCH_CHECK();
    return FHE_OK;
}

// LeveledSHEBFVRNS::EvalMult, BEHZ branch, without relinearisation (bfvrns-leveledshe.cpp:198-445):
//   :302-325 FastBaseConvqToBskMontgomery + SetFormat(EVALUATION) on the four input elements,
//   :327-372 tensor product over Q u Bsk,  :414-437 SetFormat(COEFFICIENT); FastRNSFloorq; FastBaseConvSK per product.
// Inputs [batch][numQ][N] EVALUATION; outputs [batch][numQ][N], COEFFICIENT as the reference leaves them, or
// EVALUATION when outEval != 0 (what LeveledSHEBase::EvalMult(ct,ct,key) does next, base-leveledshe.cpp:204-205).
extern "C" size_t fhe_bfv_eval_mult_behz_workspace_bytes(const fhe_behz* h, uint32_t batch) {
    if (!h)
        return 0;
    const size_t ext = ((size_t)batch * (h->numQ + h->numBsk)) << h->ctx->logN;
    return (7 * ext) * 8 + fhe_behz_workspace_bytes(h, batch);
}
extern "C" fhe_status fhe_bfv_eval_mult_behz(fhe_behz* h, const uint64_t* a0, const uint64_t* a1, const uint64_t* b0,
                                             const uint64_t* b1, uint64_t* d0, uint64_t* d1, uint64_t* d2, int outEval,
                                             uint32_t batch, void* ws, size_t wsBytes, void* st) {
    ARG_CHECK(h && a0 && a1 && b0 && b1 && d0 && d1 && d2 && ws && batch >= 1, "fhe_bfv_eval_mult_behz: bad argument");
    ARG_CHECK(wsBytes >= fhe_bfv_eval_mult_behz_workspace_bytes(h, batch), "fhe_bfv_eval_mult_behz: workspace too small");
    fhe_ctx* c = h->ctx;
    RT_CHECK(rt::set_device(c->device));
    const uint32_t tot = h->numQ + h->numBsk;
    const size_t ext = ((size_t)batch * tot) << c->logN, rowB = (size_t)8 << c->logN;
    uint64_t* w        = (uint64_t*)ws;
    uint64_t* e[4]     = {w, w + ext, w + 2 * ext, w + 3 * ext};
    uint64_t* p[3]     = {w + 4 * ext, w + 5 * ext, w + 6 * ext};
    void* sub          = w + 7 * ext;
    const size_t subB  = fhe_behz_workspace_bytes(h, batch);
    const uint64_t* in[4] = {a0, a1, b0, b1};
    for (int k = 0; k < 4; ++k) {
        RT_CHECK(rt::d2d_2d(e[k], tot * rowB, in[k], h->numQ * rowB, h->numQ * rowB, batch, (rt::stream_t)st));
        if (fhe_status s = fhe_behz_q_to_bsk(h, e[k], 1, batch, sub, subB, st))
            return s;
    }
    if (fhe_status s = fhe_tensor(c, e[0], e[1], e[2], e[3], p[0], p[1], p[2], h->allIdx.data(), tot, batch, st))
        return s;
    uint64_t* out[3] = {d0, d1, d2};
    for (int k = 0; k < 3; ++k) {
        if (fhe_status s = fhe_ntt_inv(c, p[k], h->allIdx.data(), tot, batch, st))
            return s;
        if (fhe_status s = fhe_behz_floorq(h, p[k], batch, st))
            return s;
        if (fhe_status s = fhe_behz_conv_sk(h, p[k], out[k], batch, st))
            return s;
        if (outEval)
            if (fhe_status s = fhe_ntt_fwd(c, out[k], h->qIdx.data(), h->numQ, batch, st))
                return s;
    }
    return FHE_OK;
}

// LeveledSHEBase::EvalMult(ct, ct, key) for BFV/BEHZ (base-leveledshe.cpp:201-214 over bfvrns-leveledshe.cpp:198-445):
// EvalMultNoRelin (three elements, COEFFICIENT) -> SetFormat(EVALUATION) -> KeySwitchCore on the third element ->
// c0 += ks0, c1 += ks1.  The context holds Q (limbs 0..sizeQ-1, the key-switch plan's Q), P and the Bsk limbs.
extern "C" size_t fhe_bfv_eval_mult_relin_workspace_bytes(const fhe_behz* bz, const fhe_ks_plan* p, uint32_t batch) {
    if (!bz || !p)
        return 0;
    return fhe_bfv_eval_mult_behz_workspace_bytes(bz, batch) + fhe_ks_workspace_bytes(p, p->sizeQ, batch) +
           (((size_t)batch * p->sizeQ) << p->ctx->logN) * 8;
}
extern "C" fhe_status fhe_bfv_eval_mult_relin_behz(fhe_behz* bz, fhe_ks_plan* p, const fhe_ks_key* key, const uint64_t* a0,
                                                   const uint64_t* a1, const uint64_t* b0, const uint64_t* b1, uint64_t* c0,
                                                   uint64_t* c1, uint32_t batch, void* wsv, size_t wsBytes, void* st) {
    ARG_CHECK(bz && p && key && a0 && a1 && b0 && b1 && c0 && c1 && wsv && batch >= 1, "fhe_bfv_eval_mult_relin_behz: bad argument");
    ARG_CHECK(key->plan == p && bz->ctx == p->ctx, "fhe_bfv_eval_mult_relin_behz: plans / key do not belong together");
    ARG_CHECK(bz->numQ == p->sizeQ, "fhe_bfv_eval_mult_relin_behz: the BEHZ basis Q must be the key-switch plan's Q");
    for (uint32_t i = 0; i < bz->numQ; ++i)
        ARG_CHECK(bz->qIdx[i] == i, "fhe_bfv_eval_mult_relin_behz: Q must be the context's leading limbs");
    ARG_CHECK(wsBytes >= fhe_bfv_eval_mult_relin_workspace_bytes(bz, p, batch), "fhe_bfv_eval_mult_relin_behz: workspace too small");
    const size_t nrB = fhe_bfv_eval_mult_behz_workspace_bytes(bz, batch), ksB = fhe_ks_workspace_bytes(p, p->sizeQ, batch);
    char* w      = (char*)wsv;
    uint64_t* d2 = (uint64_t*)(w + nrB + ksB);
    if (fhe_status s = fhe_bfv_eval_mult_behz(bz, a0, a1, b0, b1, c0, c1, d2, 1, batch, w, nrB, st))
        return s;
    const KsLayout lay = ks_layout(p, p->sizeQ, batch);
    return keyswitch_run(p, key, d2, p->sizeQ, batch, c0, c1, (uint64_t*)(w + nrB), lay, st, true);
}

// ------------------------------------------------------------------------------------------------
// BFV EvalMult, HPS family (HPS, HPSPOVERQ, HPSPOVERQLEVELED)
// ------------------------------------------------------------------------------------------------
// The plan derives every table of CryptoParametersBFVRNS::PrecomputeCRTTables' HPS block (bfvrns-cryptoparameters.cpp:143-665)
// from the moduli with 64-bit modular arithmetic.  The reference forms X = t*M*[(B/s)^-1]_s as a big integer and stores
// floor(X/s) mod o and (X mod s)/s; with o | M, floor(X/s) = -(X mod s) * s^-1 (mod o), and X/o_j = t*(M/o_j)*[(B/o_j)^-1]_{o_j}
// is a product of residues — the same numbers.
struct fhe_hps {
    fhe_ctx* ctx;
    uint32_t numQ, numR;
    int technique;
    uint64_t t;
    std::vector<uint32_t> qIdx, rIdx;
    std::vector<uint64_t> q, r;
    struct Level {
        uint32_t L = 0, Lr = 0, nApprox = 0;  // limbs of Q_l, of R_l, and source limbs of the approximate Q -> R_l conversion
        std::vector<uint32_t> idx;            // context limbs of [Q_l | R_l]
        fhe_conv* qToR    = nullptr;          // ExpandCRTBasis Q_l -> R_l
        fhe_conv* rToQ    = nullptr;          // SwitchCRTBasis R_l -> Q_l
        fhe_conv* pOverQ  = nullptr;          // FastExpandCRTBasisPloverQ's approximate half (null for HPS)
        fhe_sr_plan* tail = nullptr;          // HPS: QR -> R;  else Q_lR_l -> Q_l
        fhe_sr_plan* drop = nullptr;          // Q -> Q_l (levels below the top)
        std::vector<uint64_t> QlHatModq;
        // the register-resident kernels (bfv_kernels.h); usable when every basis they hold has at most kMaxBfvLimbs limbs
        bool fuseExpand = false, fuseTail = false, fuseHead = false;
        HpsSwitchTables swRQ{}, swQR{};
        HpsScaleTables scTail{}, scDrop{};
        const TwPair* exHatInv  = nullptr;
        const uint64_t *exSrcQ = nullptr, *exHatMod = nullptr, *exR = nullptr, *exMuR = nullptr;
    };
    std::vector<Level> lv;
    std::map<std::pair<int, uint32_t>, std::vector<uint64_t>> tables;  // (table id, level) -> values, for fhe_hps_table
    std::vector<void*> owned;
};
enum {
    HPS_T_QlHatInvModq = 0, HPS_T_QlHatModr, HPS_T_alphaQlModr, HPS_T_qInv, HPS_T_RlHatInvModr, HPS_T_RlHatModq, HPS_T_alphaRlModq,
    HPS_T_rInv, HPS_T_tRSHatInvModsDivsModr, HPS_T_tRSHatInvModsDivsFrac, HPS_T_tQlSlHatInvModsDivsModq, HPS_T_tQlSlHatInvModsDivsFrac,
    HPS_T_negRlQHatInvModq, HPS_T_negRlQlHatInvModq, HPS_T_qInvModr, HPS_T_QlQHatInvModqDivqModq, HPS_T_QlQHatInvModqDivqFrac,
    HPS_T_QlHatModq, HPS_T_COUNT
};

extern "C" uint32_t fhe_param_hps_r(uint32_t logN, uint32_t numQ, const uint64_t* q, int technique, uint64_t* r, uint64_t* psiR) {
    if (!q || !r || !psiR || numQ < 1 || technique < 1 || technique > 3)
        return 0;
    const uint32_t numR = technique == 1 ? numQ + 1 : numQ;  // bfvrns-cryptoparameters.cpp:126
    if (numQ + numR > (uint32_t)kMaxLimbs)
        return 0;
    const uint64_t M = 2ull << logN;
    uint64_t cur     = q[numQ - 1];
    for (uint32_t j = 0; j < numR; ++j) {  // :75, :135-137
        cur     = host::previous_prime(cur, M);
        r[j]    = cur;
        psiR[j] = host::min_root_of_unity(M, cur);
    }
    return numR;
}

namespace {
std::vector<uint64_t> head_of(const std::vector<uint64_t>& v, uint32_t n) { return std::vector<uint64_t>(v.begin(), v.begin() + n); }
uint64_t dbits(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    return u;
}
// plain CRT conversion tables S -> D in the layout of fhe_conv_create_custom: hatInv[nS], hatMod[nS][nD], alpha[nS+1][nD], inv[nS]
struct CrtTabs {
    std::vector<uint64_t> hatInv, hatMod, alpha, inv;
};
CrtTabs crt_tabs(const std::vector<uint64_t>& S, const std::vector<uint64_t>& D) {
    const size_t nS = S.size(), nD = D.size();
    CrtTabs c;
    c.hatInv.resize(nS), c.hatMod.resize(nS * nD), c.alpha.resize((nS + 1) * nD), c.inv.resize(nS);
    for (size_t i = 0; i < nS; ++i) {
        c.hatInv[i] = host::invmod(host::prod_mod(S, (int)i, S[i]), S[i]);
        c.inv[i]    = dbits(1. / static_cast<double>(S[i]));
        for (size_t j = 0; j < nD; ++j)
            c.hatMod[i * nD + j] = host::prod_mod(S, (int)i, D[j]);
    }
    for (size_t j = 0; j < nD; ++j) {
        const uint64_t Sm = host::prod_mod(S, -1, D[j]);
        for (size_t a = 0; a <= nS; ++a)
            c.alpha[a * nD + j] = host::mulmod(a % D[j], Sm, D[j]);
    }
    return c;
}
// ScaleAndRound tables for input basis I, output basis O, B = I u O, factor t * prod(O):
//   tab[j][i] = floor(X_i / s_i) mod o_j, tab[j][nI] = (X'_j / o_j) mod o_j, frac[i] = (X_i mod s_i) / s_i,
//   X_i = t * prod(O) * [(B/s_i)^-1]_{s_i},  X'_j = t * prod(O) * [(B/o_j)^-1]_{o_j}
void sr_tabs(const std::vector<uint64_t>& I, const std::vector<uint64_t>& O, uint64_t t, std::vector<uint64_t>& tab,
             std::vector<uint64_t>& frac) {
    const size_t nI = I.size(), nO = O.size();
    tab.assign(nO * (nI + 1), 0);
    frac.assign(nI, 0);
    for (size_t i = 0; i < nI; ++i) {
        const uint64_t s  = I[i];
        const uint64_t h  = host::invmod(host::mulmod(host::prod_mod(I, (int)i, s), host::prod_mod(O, -1, s), s), s);
        const uint64_t Xm = host::mulmod(host::mulmod(t % s, host::prod_mod(O, -1, s), s), h, s);
        frac[i]           = dbits(static_cast<double>(Xm) / static_cast<double>(s));
        for (size_t j = 0; j < nO; ++j) {
            const uint64_t o         = O[j];
            tab[j * (nI + 1) + i] = host::mulmod((o - Xm % o) % o, host::invmod(s % o, o), o);
        }
    }
    for (size_t j = 0; j < nO; ++j) {
        const uint64_t o = O[j], hat = host::prod_mod(O, (int)j, o);
        const uint64_t g = host::invmod(host::mulmod(host::prod_mod(I, -1, o), hat, o), o);
        tab[j * (nI + 1) + nI] = host::mulmod(host::mulmod(t % o, hat, o), g, o);
    }
}
}  // namespace

static void hps_free_level(fhe_hps::Level& v) {
    fhe_conv_destroy(v.qToR);
    fhe_conv_destroy(v.rToQ);
    fhe_conv_destroy(v.pOverQ);
    fhe_sr_plan_destroy(v.tail);
    fhe_sr_plan_destroy(v.drop);
}
extern "C" void fhe_hps_destroy(fhe_hps* h) {
    if (!h)
        return;
    for (auto& v : h->lv)
        hps_free_level(v);
    for (void* p : h->owned)
        rt::dfree(p);
    delete h;
}
// device tables of the register-resident kernels: vectors padded to kMaxBfvLimbs, matrices [target][kMaxBfvLimbs]
static fhe_status hps_switch_tables(fhe_hps* h, const std::vector<uint64_t>& S, const std::vector<uint64_t>& D, const CrtTabs& c,
                                    HpsSwitchTables* out) {
    const size_t W = kMaxBfvLimbs, nS = S.size(), nD = D.size();
    std::vector<TwPair> hatInv(W, TwPair{0, 0});
    std::vector<uint64_t> srcQ(W, 1), hatMod(nD * W, 0), mu(2 * nD);
    std::vector<double> inv(W, 0.0);
    for (size_t i = 0; i < nS; ++i) {
        hatInv[i] = TwPair{c.hatInv[i], host::shoup(c.hatInv[i], S[i])};
        srcQ[i]   = S[i];
        inv[i]    = 1. / static_cast<double>(S[i]);
        for (size_t j = 0; j < nD; ++j)
            hatMod[j * W + i] = c.hatMod[i * nD + j];
    }
    for (size_t j = 0; j < nD; ++j)
        host::mu128(D[j], &mu[2 * j]);
    TwPair* p1;
    uint64_t *d1, *d2, *d3, *d4, *d5;
    double* f1;
    fhe_status s;
    if ((s = dev_copy(&h->owned, hatInv.data(), W, &p1)) || (s = dev_copy(&h->owned, srcQ.data(), W, &d1)) ||
        (s = dev_copy(&h->owned, inv.data(), W, &f1)) || (s = dev_copy(&h->owned, hatMod.data(), hatMod.size(), &d2)) ||
        (s = dev_copy(&h->owned, D.data(), nD, &d3)) || (s = dev_copy(&h->owned, mu.data(), mu.size(), &d4)) ||
        (s = dev_copy(&h->owned, c.alpha.data(), c.alpha.size(), &d5)))
        return s;
    *out = HpsSwitchTables{p1, d1, f1, d2, d3, d4, d5, (uint32_t)nS, (uint32_t)nD};
    return FHE_OK;
}
static fhe_status hps_scale_tables(fhe_hps* h, const std::vector<uint64_t>& I, const std::vector<uint64_t>& O,
                                   const std::vector<uint64_t>& tab, const std::vector<uint64_t>& frac, HpsScaleTables* out) {
    const size_t W = kMaxBfvLimbs, nI = I.size(), nO = O.size();
    std::vector<uint64_t> t16(nO * W, 0), o(W, 1), mu(2 * W, 0);
    std::vector<TwPair> last(W, TwPair{0, 0});
    std::vector<double> f(W, 0.0);
    for (size_t j = 0; j < nO; ++j) {
        for (size_t i = 0; i < nI; ++i)
            t16[j * W + i] = tab[j * (nI + 1) + i];
        last[j] = TwPair{tab[j * (nI + 1) + nI], host::shoup(tab[j * (nI + 1) + nI], O[j])};
        o[j]    = O[j];
        host::mu128(O[j], &mu[2 * j]);
    }
    for (size_t i = 0; i < nI; ++i)
        std::memcpy(&f[i], &frac[i], 8);
    uint64_t *d1, *d2, *d3;
    TwPair* p1;
    double* f1;
    fhe_status s;
    if ((s = dev_copy(&h->owned, t16.data(), t16.size(), &d1)) || (s = dev_copy(&h->owned, last.data(), W, &p1)) ||
        (s = dev_copy(&h->owned, f.data(), W, &f1)) || (s = dev_copy(&h->owned, o.data(), W, &d2)) ||
        (s = dev_copy(&h->owned, mu.data(), mu.size(), &d3)))
        return s;
    *out = HpsScaleTables{d1, p1, f1, d2, d3, (uint32_t)nI, (uint32_t)nO};
    return FHE_OK;
}
static fhe_status hps_conv(fhe_hps* h, const std::vector<uint32_t>& sIdx, const std::vector<uint32_t>& dIdx, const uint64_t* hatInv,
                           const uint64_t* hatMod, const uint64_t* alpha, const uint64_t* inv, fhe_conv** out) {
    std::vector<double> invd;
    if (inv) {
        invd.resize(sIdx.size());
        std::memcpy(invd.data(), inv, sIdx.size() * 8);
    }
    return fhe_conv_create_custom(h->ctx, sIdx.data(), (uint32_t)sIdx.size(), dIdx.data(), (uint32_t)dIdx.size(), hatInv, hatMod, alpha,
                                  inv ? invd.data() : nullptr, out);
}
static fhe_status hps_sr(fhe_hps* h, uint32_t sizeI, const std::vector<uint32_t>& oIdx, const std::vector<uint64_t>& tab,
                         const std::vector<uint64_t>& frac, fhe_sr_plan** out) {
    std::vector<double> f(frac.size());
    std::memcpy(f.data(), frac.data(), frac.size() * 8);
    return fhe_sr_plan_create(h->ctx, sizeI, oIdx.data(), (uint32_t)oIdx.size(), tab.data(), f.data(), out);
}

extern "C" fhe_status fhe_hps_create(fhe_ctx* c, const uint32_t* qLimbIdx, uint32_t numQ, const uint32_t* rLimbIdx, uint32_t numR,
                                     uint64_t t, int technique, fhe_hps** out) {
    ARG_CHECK(c && qLimbIdx && rLimbIdx && out, "fhe_hps_create: null argument");
    ARG_CHECK(technique >= 1 && technique <= 3, "fhe_hps_create: technique must be HPS (1), HPSPOVERQ (2) or HPSPOVERQLEVELED (3)");
    ARG_CHECK(numQ >= 1 && numR == (technique == 1 ? numQ + 1 : numQ), "fhe_hps_create: R has numQ + 1 limbs for HPS, numQ otherwise");
    ARG_CHECK(numQ + numR <= (uint32_t)kMaxLimbs, "fhe_hps_create: numQ + numR exceeds the row bound of a tower (256)");
    ARG_CHECK(t >= 2, "fhe_hps_create: bad plaintext modulus");
    std::vector<uint64_t> q(numQ), r(numR);
    for (uint32_t i = 0; i < numQ; ++i) {
        ARG_CHECK(qLimbIdx[i] < c->L, "fhe_hps_create: limb index exceeds context size");
        q[i] = c->q[qLimbIdx[i]];
    }
    for (uint32_t j = 0; j < numR; ++j) {
        ARG_CHECK(rLimbIdx[j] < c->L, "fhe_hps_create: limb index exceeds context size");
        r[j] = c->q[rLimbIdx[j]];
    }
    RT_CHECK(rt::set_device(c->device));
    fhe_hps* h = new fhe_hps;
    h->ctx = c, h->numQ = numQ, h->numR = numR, h->technique = technique, h->t = t, h->q = q, h->r = r;
    h->qIdx.assign(qLimbIdx, qLimbIdx + numQ);
    h->rIdx.assign(rLimbIdx, rLimbIdx + numR);
    const bool hps = technique == 1;
    auto& T        = h->tables;
    // level-independent tables
    {
        std::vector<uint64_t> qInv(numQ), rInv(numR), qInvModr((size_t)numQ * numR);
        for (uint32_t i = 0; i < numQ; ++i) {
            qInv[i] = dbits(1. / static_cast<double>(q[i]));  // :262-265
            for (uint32_t j = 0; j < numR; ++j)
                qInvModr[(size_t)i * numR + j] = host::invmod(q[i] % r[j], r[j]);  // :524-530
        }
        for (uint32_t j = 0; j < numR; ++j)
            rInv[j] = dbits(1. / static_cast<double>(r[j]));  // :429-432
        T[{HPS_T_qInv, 0}] = qInv, T[{HPS_T_rInv, 0}] = rInv, T[{HPS_T_qInvModr, 0}] = qInvModr;
        sr_tabs(q, r, t, T[{HPS_T_tRSHatInvModsDivsModr, 0}], T[{HPS_T_tRSHatInvModsDivsFrac, 0}]);  // :281-304
    }
    const uint32_t nLevels = hps ? 1u : numQ;
    h->lv.resize(nLevels);
    fhe_status s = FHE_OK;
    for (uint32_t l = 0; l < numQ && !s; ++l) {
        const uint32_t L = l + 1;
        const std::vector<uint64_t> Ql = head_of(q, L), Qrest(q.begin() + L, q.end());
        // ScaleAndRound Q -> Q_l (:599-623) and ExpandCRTBasisQlHat (:629-639): functions of Q alone, kept for every technique
        std::vector<uint64_t> &dropTab = T[{HPS_T_QlQHatInvModqDivqModq, l}], &dropFrac = T[{HPS_T_QlQHatInvModqDivqFrac, l}];
        sr_tabs(Qrest, Ql, 1, dropTab, dropFrac);
        std::vector<uint64_t> hatq(L);
        for (uint32_t i = 0; i < L; ++i)
            hatq[i] = host::prod_mod(Qrest, -1, q[i]);
        T[{HPS_T_QlHatModq, l}] = hatq;
        if (hps && l != numQ - 1)
            continue;
        fhe_hps::Level& v = h->lv[hps ? 0 : l];
        const uint32_t lev = hps ? 0 : l;  // the reference keeps HPS's single table set at index 0
        v.L = L, v.Lr = hps ? numR : L, v.QlHatModq = hatq;
        const std::vector<uint64_t> Rl = head_of(r, v.Lr);
        std::vector<uint32_t> qlIdx(h->qIdx.begin(), h->qIdx.begin() + L), rlIdx(h->rIdx.begin(), h->rIdx.begin() + v.Lr);
        v.idx = qlIdx;
        v.idx.insert(v.idx.end(), rlIdx.begin(), rlIdx.end());
        const CrtTabs qr = crt_tabs(Ql, Rl), rq = crt_tabs(Rl, Ql);  // :143-203, :334-427
        T[{HPS_T_QlHatInvModq, lev}] = qr.hatInv, T[{HPS_T_QlHatModr, lev}] = qr.hatMod, T[{HPS_T_alphaQlModr, lev}] = qr.alpha;
        T[{HPS_T_RlHatInvModr, lev}] = rq.hatInv, T[{HPS_T_RlHatModq, lev}] = rq.hatMod, T[{HPS_T_alphaRlModq, lev}] = rq.alpha;
        if ((s = hps_conv(h, qlIdx, rlIdx, qr.hatInv.data(), qr.hatMod.data(), qr.alpha.data(), qr.inv.data(), &v.qToR)) ||
            (s = hps_conv(h, rlIdx, qlIdx, rq.hatInv.data(), rq.hatMod.data(), rq.alpha.data(), rq.inv.data(), &v.rToQ)))
            break;
        const bool regs = L <= (uint32_t)kMaxBfvLimbs && v.Lr <= (uint32_t)kMaxBfvLimbs;
        if (regs && (s = hps_switch_tables(h, Rl, Ql, rq, &v.swRQ)))
            break;
        if (hps) {
            const std::vector<uint64_t>&tab = T[{HPS_T_tRSHatInvModsDivsModr, 0}], &frac = T[{HPS_T_tRSHatInvModsDivsFrac, 0}];
            if ((s = hps_sr(h, numQ, rlIdx, tab, frac, &v.tail)))
                break;
            v.fuseTail = regs;
            if (regs && (s = hps_scale_tables(h, q, Rl, tab, frac, &v.scTail)))
                break;
            continue;
        }
        // Q_lR_l -> Q_l with t*Q_l/(Q_lR_l) (:565-593)
        std::vector<uint64_t> &tab = T[{HPS_T_tQlSlHatInvModsDivsModq, l}], &frac = T[{HPS_T_tQlSlHatInvModsDivsFrac, l}];
        sr_tabs(Rl, Ql, t, tab, frac);
        if ((s = hps_sr(h, L, qlIdx, tab, frac, &v.tail)))
            break;
        // FastExpandCRTBasisPloverQ (:490-522): [-R_l (Q/q_i)^-1]_{q_i} from all of Q, [-R_l (Q_l/q_i)^-1]_{q_i} from Q_l
        std::vector<uint64_t> negQ(numQ), negQl(L);
        for (uint32_t i = 0; i < numQ; ++i) {
            const uint64_t Rm = host::prod_mod(Rl, -1, q[i]);
            negQ[i]           = q[i] - host::mulmod(Rm, host::invmod(host::prod_mod(q, (int)i, q[i]), q[i]), q[i]);
            if (i < L)
                negQl[i] = q[i] - host::mulmod(Rm, qr.hatInv[i], q[i]);
        }
        T[{HPS_T_negRlQHatInvModq, l}] = negQ, T[{HPS_T_negRlQlHatInvModq, l}] = negQl;
        // (at the top level Q_l = Q and the two tables coincide; below it the composite converts from all of Q)
        v.nApprox = numQ;
        std::vector<uint64_t> invMod((size_t)numQ * L);
        for (uint32_t i = 0; i < numQ; ++i)
            for (uint32_t j = 0; j < L; ++j)
                invMod[(size_t)i * L + j] = T[{HPS_T_qInvModr, 0}][(size_t)i * numR + j];
        if ((s = hps_conv(h, h->qIdx, rlIdx, negQ.data(), invMod.data(), nullptr, nullptr, &v.pOverQ)))
            break;
        v.fuseExpand = regs && numQ <= (uint32_t)kMaxBfvLimbs;
        if (v.fuseExpand) {
            const size_t W = kMaxBfvLimbs;
            std::vector<TwPair> hi(W, TwPair{0, 0});
            std::vector<uint64_t> sq(W, 1), hm((size_t)L * W, 0), rr(W, 1), mu(2 * W, 0);
            for (uint32_t i = 0; i < numQ; ++i) {
                hi[i] = TwPair{negQ[i], host::shoup(negQ[i], q[i])};
                sq[i] = q[i];
                for (uint32_t j = 0; j < L; ++j)
                    hm[(size_t)j * W + i] = invMod[(size_t)i * L + j];
            }
            for (uint32_t j = 0; j < L; ++j) {
                rr[j] = r[j];
                host::mu128(r[j], &mu[2 * j]);
            }
            TwPair* p1;
            uint64_t *d1, *d2, *d3, *d4;
            if ((s = dev_copy(&h->owned, hi.data(), W, &p1)) || (s = dev_copy(&h->owned, sq.data(), W, &d1)) ||
                (s = dev_copy(&h->owned, hm.data(), hm.size(), &d2)) || (s = dev_copy(&h->owned, rr.data(), W, &d3)) ||
                (s = dev_copy(&h->owned, mu.data(), mu.size(), &d4)))
                break;
            v.exHatInv = p1, v.exSrcQ = d1, v.exHatMod = d2, v.exR = d3, v.exMuR = d4;
        }
        if (technique == 3 && L < numQ) {
            std::vector<uint32_t> restIdx(h->qIdx.begin() + L, h->qIdx.end());
            if ((s = hps_sr(h, numQ - L, qlIdx, dropTab, dropFrac, &v.drop)))
                break;
            v.fuseHead = regs && numQ - L <= (uint32_t)kMaxBfvLimbs;
            if (v.fuseHead && ((s = hps_scale_tables(h, Qrest, Ql, dropTab, dropFrac, &v.scDrop)) || (s = hps_switch_tables(h, Ql, Rl, qr, &v.swQR))))
                break;
        }
    }
    if (s) {
        fhe_hps_destroy(h);
        return s;
    }
    *out = h;
    return FHE_OK;
}

// Read-only view of a derived table (tests compare every one with the reference's, bit for bit).  Layouts, row-major, L = level + 1
// limbs of Q_l and Lr limbs of R_l (HPS keeps one set at level 0 with L = numQ, Lr = numR); doubles are returned as their bit patterns:
//    0 QlHatInvModq [L]           1 QlHatModr [L][Lr]           2 alphaQlModr [L+1][Lr]        3 qInv [numQ] (double)
//    4 RlHatInvModr [Lr]          5 RlHatModq [Lr][L]           6 alphaRlModq [Lr+1][L]        7 rInv [numR] (double)
//    8 tRSHatInvModsDivsModr [numR][numQ+1]                     9 tRSHatInvModsDivsFrac [numQ] (double)
//   10 tQlSlHatInvModsDivsModq [L][L+1]                        11 tQlSlHatInvModsDivsFrac [L] (double)
//   12 mNegRlQHatInvModq [numQ]  13 mNegRlQlHatInvModq [L]      14 qInvModr [numQ][numR]
//   15 QlQHatInvModqDivqModq [L][numQ-L+1]                     16 QlQHatInvModqDivqFrac [numQ-L] (double)     17 QlHatModq [L]
// Returns the number of 64-bit words of the table (0: no such table for this plan); copies min(that, cap) words into out.
extern "C" size_t fhe_hps_table(const fhe_hps* h, int tableId, uint32_t level, uint64_t* out, size_t cap) {
    if (!h)
        return 0;
    auto it = h->tables.find({tableId, level});
    if (it == h->tables.end())
        return 0;
    if (out && cap)
        std::memcpy(out, it->second.data(), std::min(cap, it->second.size()) * 8);
    return it->second.size();
}

static const fhe_hps::Level* hps_level(const fhe_hps* h, uint32_t sizeQl) {
    if (!h || sizeQl < 1 || sizeQl > h->numQ)
        return nullptr;
    if (h->technique != 3 && sizeQl != h->numQ)
        return nullptr;
    return &h->lv[h->technique == 1 ? 0 : sizeQl - 1];
}
extern "C" size_t fhe_bfv_eval_mult_hps_workspace_bytes(const fhe_hps* h, uint32_t sizeQl, uint32_t batch) {
    const fhe_hps::Level* v = hps_level(h, sizeQl);
    if (!v)
        return 0;
    const size_t rows = 7 * (size_t)(v->L + v->Lr) + h->numQ + std::max(h->numQ, h->numR);
    return ((rows * batch) << h->ctx->logN) * 8;
}
// LeveledSHEBFVRNS::EvalMult, the three HPS branches, without relinearisation (bfvrns-leveledshe.cpp:198-439).
extern "C" fhe_status fhe_bfv_eval_mult_hps(fhe_hps* h, const uint64_t* a0, const uint64_t* a1, const uint64_t* b0, const uint64_t* b1,
                                            uint64_t* d0, uint64_t* d1, uint64_t* d2, uint32_t sizeQl, int outEval, uint32_t batch,
                                            void* ws, size_t wsBytes, void* st) {
    ARG_CHECK(h && a0 && a1 && b0 && b1 && d0 && d1 && d2 && ws && batch >= 1, "fhe_bfv_eval_mult_hps: bad argument");
    const fhe_hps::Level* vp = hps_level(h, sizeQl);
    ARG_CHECK(vp, "fhe_bfv_eval_mult_hps: sizeQl must be numQ (1 ... numQ for HPSPOVERQLEVELED)");
    ARG_CHECK(wsBytes >= fhe_bfv_eval_mult_hps_workspace_bytes(h, sizeQl, batch), "fhe_bfv_eval_mult_hps: workspace too small");
    const fhe_hps::Level& v = *vp;
    fhe_ctx* c = h->ctx;
    RT_CHECK(rt::set_device(c->device));
    const uint32_t nQ = h->numQ, L = v.L, tot = v.L + v.Lr, logN = c->logN;
    const bool hps = h->technique == 1, dropped = L < nQ;
    const size_t ext = ((size_t)batch * tot) << logN, qB = (((size_t)batch * nQ) << logN) * 8;
    uint64_t* w      = (uint64_t*)ws;
    uint64_t* e[4]   = {w, w + ext, w + 2 * ext, w + 3 * ext};
    uint64_t* p[3]   = {w + 4 * ext, w + 5 * ext, w + 6 * ext};
    uint64_t* coef   = w + 7 * ext;                        // [batch][numQ][N]: coefficient form of one input element
    uint64_t* tmp    = coef + (((size_t)batch * nQ) << logN);  // [batch][max(numQ, numR)][N]
    const uint32_t grid = coeff_grid(c, batch);
    const uint64_t* in[4] = {a0, a1, b0, b1};
    for (int k = 0; k < 4; ++k) {
        fhe_status s = FHE_OK;
        if (hps || (k < 2 && !dropped)) {  // ExpandCRTBasis Q -> QR, the EVALUATION copy of the Q limbs kept (:223-246)
            if ((s = expand_run(v.qToR, in[k], 1, e[k], 1, 0, batch, coef, qB, st, true)))
                return s;
            continue;
        }
        if ((s = ntt_run(c, true, in[k], coef, h->qIdx.data(), nQ, batch, st)))  // SetFormat(COEFFICIENT) (:257, :275, :297)
            return s;
        if (k < 2) {  // ScaleAndRound Q -> Q_l, ExpandCRTBasis Q_l -> Q_lR_l (:276-286)
            if (v.fuseHead) {
                ScaleSwitchArgs g;
                g.in = TowerView{coef, nQ, L}, g.own = TowerView{coef, nQ, 0};
                g.outMid = TowerView{e[k], tot, 0}, g.outDst = TowerView{e[k], tot, L};
                g.sr = v.scDrop, g.sw = v.swQR, g.logN = logN, g.batch = batch;
                FHE_LAUNCH((scale_round_switch_kernel<true>), grid, st, g);
                LAUNCH_CHECK();
                s = fhe_ntt_fwd(c, e[k], v.idx.data(), tot, batch, st);
            }
            else if (!(s = fhe_scale_and_round(v.drop, coef, 1, tmp, batch, st)))
                s = expand_run(v.qToR, tmp, 0, e[k], 1, 0, batch, nullptr, 0, st, true);
        }
        else {  // FastExpandCRTBasisPloverQ, SetFormat(EVALUATION) (:256-261, :296-301)
            if (v.fuseExpand) {
                POverQExpandArgs g;
                g.in = TowerView{coef, nQ, 0}, g.out = TowerView{e[k], tot, 0};
                g.hatInv = v.exHatInv, g.srcQ = v.exSrcQ, g.hatMod = v.exHatMod, g.r = v.exR, g.muR = v.exMuR;
                g.sw = v.swRQ, g.nSrc = v.nApprox, g.logN = logN, g.batch = batch;
                FHE_LAUNCH(p_over_q_expand_kernel, grid, st, g);
                LAUNCH_CHECK();
            }
            else if ((s = conv_run<false>(v.pOverQ, coef, nQ, 0, e[k], tot, L, batch, st)) ||
                     (s = conv_run<true>(v.rToQ, e[k], tot, L, e[k], tot, 0, batch, st)))
                return s;
            s = fhe_ntt_fwd(c, e[k], v.idx.data(), tot, batch, st);
        }
        if (s)
            return s;
    }
    if (fhe_status s = fhe_tensor(c, e[0], e[1], e[2], e[3], p[0], p[1], p[2], v.idx.data(), tot, batch, st))  // :354-365
        return s;
    uint64_t* out[3] = {d0, d1, d2};
    for (int k = 0; k < 3; ++k) {
        fhe_status s;
        if ((s = fhe_ntt_inv(c, p[k], v.idx.data(), tot, batch, st)))
            return s;
        if (hps) {  // ScaleAndRound QR -> R, SwitchCRTBasis R -> Q (:368-383)
            if (v.fuseTail) {
                ScaleSwitchArgs g;
                g.in = TowerView{p[k], tot, 0}, g.own = TowerView{p[k], tot, L};
                g.outMid = g.own, g.outDst = TowerView{out[k], nQ, 0};
                g.sr = v.scTail, g.sw = v.swRQ, g.logN = logN, g.batch = batch;
                FHE_LAUNCH((scale_round_switch_kernel<false>), grid, st, g);
                LAUNCH_CHECK();
            }
            else if ((s = fhe_scale_and_round(v.tail, p[k], 0, tmp, batch, st)) ||
                     (s = conv_run<true>(v.rToQ, tmp, v.Lr, 0, out[k], nQ, 0, batch, st)))
                return s;
        }
        else if (!dropped) {  // ScaleAndRound QR -> Q (:385-395, :397-404)
            if ((s = fhe_scale_and_round(v.tail, p[k], 1, out[k], batch, st)))
                return s;
        }
        else {  // ScaleAndRound Q_lR_l -> Q_l, ExpandCRTBasisQlHat (:402-410)
            if ((s = fhe_scale_and_round(v.tail, p[k], 1, tmp, batch, st)) ||
                (s = fhe_expand_crt_basis_ql_hat(c, tmp, L, v.QlHatModq.data(), h->qIdx.data(), nQ, batch, out[k], st)))
                return s;
        }
        if (outEval)
            if ((s = fhe_ntt_fwd(c, out[k], h->qIdx.data(), nQ, batch, st)))
                return s;
    }
    return FHE_OK;
}

// ---- BV key switching (keyswitch-bv.cpp) --------------------------------------------------------------------------------------------
// KeySwitchBV::KeySwitchCore (:245-259) = EvalFastKeySwitchCore(EvalKeySwitchPrecomputeCore(a), ek): digits = a.CRTDecompose(r) (:254), then
// for both key vectors the sum over the digits of digit * key tower, the key towers cut to the level's limbs (:261-278).  No auxiliary
// basis, no ModDown: the same calls serve BFV, BGV and CKKS.  The windows of a limb depend on its modulus only, so the digits of level sizeQl
// meet the FIRST D_l towers of a key generated over sizeQ limbs (KeySwitchGenInternal, :49-103), row i of a key tower is limb i.
struct fhe_bv_key {
    fhe_ctx* ctx;
    uint32_t sizeQ, baseBits, D0;
    uint64_t *d_b = nullptr, *d_a = nullptr;  // [D0][sizeQ][N] EVALUATION
    bool owned = true;
};
static fhe_status bv_key_new(fhe_ctx* c, uint32_t sizeQ, uint32_t baseBits, const char* who, fhe_bv_key** out) {
    ARG_CHECK(sizeQ >= 1 && sizeQ <= c->L, std::string(who) + ": sizeQ must be in [1, limbs of the context]");
    const uint32_t D0 = fhe_crt_decompose_towers(c, nullptr, sizeQ, baseBits);
    if (D0 == 0)
        return fail(FHE_ERR_UNSUPPORTED, std::string(who) + ": digit size outside the device path (baseBits <= 31, every window inside the word)");
    fhe_bv_key* k = new fhe_bv_key;
    k->ctx = c, k->sizeQ = sizeQ, k->baseBits = baseBits, k->D0 = D0;
    *out = k;
    return FHE_OK;
}
extern "C" fhe_status fhe_bv_key_upload(fhe_ctx* c, uint32_t sizeQ, uint32_t baseBits, const uint64_t* keyB, const uint64_t* keyA,
                                        fhe_bv_key** out) {
    ARG_CHECK(c && keyB && keyA && out, "fhe_bv_key_upload: null argument");
    fhe_bv_key* k = nullptr;
    if (fhe_status s = bv_key_new(c, sizeQ, baseBits, "fhe_bv_key_upload", &k))
        return s;
    const size_t bytes = (((size_t)k->D0 * sizeQ) << c->logN) * 8;
    if (rt::set_device(c->device) || rt::dmalloc((void**)&k->d_b, bytes) || rt::dmalloc((void**)&k->d_a, bytes)) {
        fhe_bv_key_destroy(k);
        return fail(FHE_ERR_ALLOC, "fhe_bv_key_upload: device allocation failed");
    }
    const char* e = rt::h2d(k->d_b, keyB, bytes, nullptr);
    if (!e)
        e = rt::h2d(k->d_a, keyA, bytes, nullptr);
    if (!e)
        e = rt::sync(nullptr);
    if (e) {
        fhe_bv_key_destroy(k);
        return fail(FHE_ERR_DEVICE, std::string("fhe_bv_key_upload: ") + e);
    }
    *out = k;
    return FHE_OK;
}
extern "C" fhe_status fhe_bv_key_wrap(fhe_ctx* c, uint32_t sizeQ, uint32_t baseBits, uint64_t* devB, uint64_t* devA, fhe_bv_key** out) {
    ARG_CHECK(c && devB && devA && out, "fhe_bv_key_wrap: null argument");
    fhe_bv_key* k = nullptr;
    if (fhe_status s = bv_key_new(c, sizeQ, baseBits, "fhe_bv_key_wrap", &k))
        return s;
    k->d_b = devB, k->d_a = devA, k->owned = false;
    *out = k;
    return FHE_OK;
}
extern "C" void fhe_bv_key_destroy(fhe_bv_key* k) {
    if (!k)
        return;
    if (k->owned && k->d_b)
        rt::dfree(k->d_b);
    if (k->owned && k->d_a)
        rt::dfree(k->d_a);
    delete k;
}
// workspace (words): digits [D_l][batch][sizeQl][N] | coef [batch][sizeQl][N] (the coefficient copy of an EVALUATION input, dcrtpoly-impl.h:231-233)
extern "C" size_t fhe_bv_workspace_bytes(const fhe_ctx* c, uint32_t sizeQl, uint32_t baseBits, uint32_t batch) {
    const uint32_t D = fhe_crt_decompose_towers(c, nullptr, sizeQl, baseBits);
    if (D == 0 || sizeQl > c->L || batch < 1)
        return 0;
    return ((((size_t)D + 1) * batch * sizeQl) << c->logN) * 8;
}
extern "C" fhe_status fhe_bv_precompute(fhe_ctx* c, const uint64_t* cin, int evalFormat, uint32_t sizeQl, uint32_t baseBits, uint32_t batch,
                                        void* ws, size_t wsBytes, void* st) {
    ARG_CHECK(c && cin && ws, "fhe_bv_precompute: null argument");
    ARG_CHECK(sizeQl >= 1 && sizeQl <= c->L && batch >= 1, "fhe_bv_precompute: sizeQl must be in [1, sizeQ], batch >= 1");
    const uint32_t D = fhe_crt_decompose_towers(c, nullptr, sizeQl, baseBits);
    if (D == 0)
        return fail(FHE_ERR_UNSUPPORTED, "fhe_bv_precompute: digit size outside the device path (baseBits <= 31, every window inside the word)");
    ARG_CHECK((uint64_t)D * batch < ((uint64_t)1 << 31), "fhe_bv_precompute: batch too large");
    ARG_CHECK(wsBytes >= fhe_bv_workspace_bytes(c, sizeQl, baseBits, batch), "fhe_bv_precompute: workspace too small");
    RT_CHECK(rt::set_device(c->device));
    uint64_t* dig = (uint64_t*)ws;
    const uint64_t* coef = cin;
    if (evalFormat) {
        uint64_t* cf = dig + (((size_t)D * batch * sizeQl) << c->logN);
        if (fhe_status s = fhe_ntt_inv_oop(c, cin, cf, nullptr, sizeQl, batch, st))
            return s;
        coef = cf;
    }
    if (fhe_status s = crt_digits_run(c, coef, nullptr, sizeQl, baseBits, batch, dig, st, "fhe_bv_precompute"))
        return s;
    // canonical output: the digits a hoisting caller finds in ws are the words of DCRTPolyImpl::CRTDecompose
    return fhe_ntt_fwd(c, dig, nullptr, sizeQl, D * batch, st);
}
static fhe_status bv_fast_check(const fhe_bv_key* k, uint32_t sizeQl, uint32_t batch, const void* out0, const void* out1, const void* ws,
                                size_t wsBytes, const char* who) {
    ARG_CHECK(k && out0 && out1 && ws, std::string(who) + ": null argument");
    ARG_CHECK(sizeQl >= 1 && sizeQl <= k->sizeQ && batch >= 1, std::string(who) + ": sizeQl must be in [1, sizeQ], batch >= 1");
    ARG_CHECK(wsBytes >= fhe_bv_workspace_bytes(k->ctx, sizeQl, k->baseBits, batch), std::string(who) + ": workspace too small for the digits of this key (sizeQl, batch, or digits cut for another baseBits)");
    return FHE_OK;
}
static fhe_status bv_fast_run(const fhe_bv_key* k, uint32_t sizeQl, uint32_t batch, uint64_t* out0, uint64_t* out1, int accumulate,
                              const uint64_t* dig, void* st) {
    fhe_ctx* c = k->ctx;
    RT_CHECK(rt::set_device(c->device));
    BvInnerArgs g;
    g.digits = dig, g.keyB = k->d_b, g.keyA = k->d_a, g.out0 = out0, g.out1 = out1, g.lc = c->d_lc, g.mu128 = c->d_mu128;
    g.logN = c->logN, g.batch = batch, g.sizeQl = sizeQl, g.sizeQ = k->sizeQ, g.acc = accumulate != 0;
    g.D = fhe_crt_decompose_towers(c, nullptr, sizeQl, k->baseBits);  // the key's first D_l towers
    const uint32_t tilesPerRow = c->N >= (uint32_t)kTile ? (c->N >> kTileLog) : 1u;
    const uint64_t grid        = (((uint64_t)tilesPerRow * sizeQl + 7) / 8) * 8 * batch;
    ARG_CHECK(grid < ((uint64_t)1 << 31), "fhe_bv_fast_keyswitch: batch too large for one launch");
    // two adjacent coefficients per lane need 16-byte aligned towers (any device allocation is) and N >= 2
    const uintptr_t bits = (uintptr_t)dig | (uintptr_t)k->d_b | (uintptr_t)k->d_a | (uintptr_t)out0 | (uintptr_t)out1;
    if ((bits & 15u) == 0 && c->N >= 2)
        FHE_LAUNCH((bv_inner_product_kernel<2, false>), grid, st, g, BvNoStage{});
    else
        FHE_LAUNCH((bv_inner_product_kernel<1, false>), grid, st, g, BvNoStage{});
    LAUNCH_CHECK();
    return FHE_OK;
}
extern "C" fhe_status fhe_bv_fast_keyswitch(const fhe_bv_key* k, uint32_t sizeQl, uint32_t batch, uint64_t* out0, uint64_t* out1,
                                            int accumulate, const void* ws, size_t wsBytes, void* st) {
    if (fhe_status s = bv_fast_check(k, sizeQl, batch, out0, out1, ws, wsBytes, "fhe_bv_fast_keyswitch"))
        return s;
    return bv_fast_run(k, sizeQl, batch, out0, out1, accumulate, (const uint64_t*)ws, st);
}
extern "C" fhe_status fhe_keyswitch_bv(const fhe_bv_key* k, const uint64_t* cin, uint32_t sizeQl, uint32_t batch, uint64_t* out0,
                                       uint64_t* out1, int accumulate, void* ws, size_t wsBytes, void* st) {
    ARG_CHECK(cin, "fhe_keyswitch_bv: null argument");
    if (fhe_status s = bv_fast_check(k, sizeQl, batch, out0, out1, ws, wsBytes, "fhe_keyswitch_bv"))
        return s;
    if (fhe_status s = fhe_bv_precompute(k->ctx, cin, 1, sizeQl, k->baseBits, batch, ws, wsBytes, st))
        return s;
    return bv_fast_run(k, sizeQl, batch, out0, out1, accumulate, (const uint64_t*)ws, st);
}
// LeveledSHEBase::EvalMult(ct, ct, key) (base-leveledshe.cpp:201-214) on BFV ciphertexts of the HPS family with a BV key: EvalMultNoRelin with
// d0, d1 written to c0, c1, SetFormat(EVALUATION) (fhe_bfv_eval_mult_hps, outEval), KeySwitchCore on d2 at numQ limbs, c0 += ks0, c1 += ks1.
// workspace (bytes): d2 [batch][numQ][N] | max(the product's, the key switch's)
extern "C" size_t fhe_bfv_eval_mult_relin_hps_bv_workspace_bytes(const fhe_hps* h, uint32_t sizeQl, uint32_t baseBits, uint32_t batch) {
    const size_t mul = fhe_bfv_eval_mult_hps_workspace_bytes(h, sizeQl, batch);
    if (!mul)
        return 0;
    const size_t ks = fhe_bv_workspace_bytes(h->ctx, h->numQ, baseBits, batch);
    if (!ks)
        return 0;
    return ((((size_t)batch * h->numQ) << h->ctx->logN) * 8) + std::max(mul, ks);
}
extern "C" fhe_status fhe_bfv_eval_mult_relin_hps_bv(fhe_hps* h, const fhe_bv_key* k, const uint64_t* a0, const uint64_t* a1,
                                                     const uint64_t* b0, const uint64_t* b1, uint64_t* c0, uint64_t* c1, uint32_t sizeQl,
                                                     uint32_t batch, void* ws, size_t wsBytes, void* st) {
    ARG_CHECK(h && k && a0 && a1 && b0 && b1 && c0 && c1 && ws && batch >= 1, "fhe_bfv_eval_mult_relin_hps_bv: bad argument");
    ARG_CHECK(k->ctx == h->ctx && k->sizeQ == h->numQ, "fhe_bfv_eval_mult_relin_hps_bv: the key was built for another context or another Q");
    for (uint32_t i = 0; i < h->numQ; ++i)
        ARG_CHECK(h->qIdx[i] == i, "fhe_bfv_eval_mult_relin_hps_bv: Q must be the context's leading limbs");
    ARG_CHECK(hps_level(h, sizeQl), "fhe_bfv_eval_mult_relin_hps_bv: sizeQl must be numQ (1 ... numQ for HPSPOVERQLEVELED)");
    const size_t need = fhe_bfv_eval_mult_relin_hps_bv_workspace_bytes(h, sizeQl, k->baseBits, batch);
    ARG_CHECK(need && wsBytes >= need, "fhe_bfv_eval_mult_relin_hps_bv: workspace too small");
    const size_t d2Bytes = (((size_t)batch * h->numQ) << h->ctx->logN) * 8;
    uint64_t* d2 = (uint64_t*)ws;
    void* rest   = (char*)ws + d2Bytes;
    if (fhe_status s = fhe_bfv_eval_mult_hps(h, a0, a1, b0, b1, c0, c1, d2, sizeQl, 1, batch, rest, wsBytes - d2Bytes, st))
        return s;
    return fhe_keyswitch_bv(k, d2, h->numQ, batch, c0, c1, 1, rest, wsBytes - d2Bytes, st);
}

// ---- rotations and leveled relinearisation on a BV key ---------------------------------------------------------------------------------
// One launch of bv_inner_product_kernel's output-stage instance takes the digits in `dig` through the key's first D_l towers and the tail
// of the reference's member: ExpandCRTBasisQlHat with hat (HOST, QlHatModq(l), [sizeQl]; null: none, outRows == sizeQl), += add0 / add1
// (null: none), the EVALUATION automorphism k of both.
static fhe_status bv_out_run(const fhe_bv_key* k, uint32_t sizeQl, uint32_t outRows, uint32_t batch, const uint64_t* dig, const uint64_t* hat,
                             const uint64_t* add0, const uint64_t* add1, uint32_t kAuto, uint64_t* out0, uint64_t* out1, void* st,
                             const char* who) {
    fhe_ctx* c = k->ctx;
    ARG_CHECK(outRows >= sizeQl && outRows <= c->L && (hat || outRows == sizeQl), std::string(who) + ": bad output rows");
    ARG_CHECK(!hat || sizeQl <= (uint32_t)kConstVecLimbs, std::string(who) + ": more limbs than the constant vector of one launch holds");
    ARG_CHECK(kAuto % 2 == 1, "Automorphism index not odd");
    const uint32_t twoNmask = (2u << c->logN) - 1u;
    uint32_t kInv = kAuto;  // Newton: the inverse of an odd k modulo 2^32, then modulo 2N
    for (int it = 0; it < 5; ++it)
        kInv *= 2u - kAuto * kInv;
    kInv &= twoNmask;
    ARG_CHECK(((kAuto & twoNmask) == 1u) || (out0 != add0 && out1 != add1 && out0 != add1 && out1 != add0),
              std::string(who) + ": an output may be its own addend only when k = 1");
    RT_CHECK(rt::set_device(c->device));
    BvInnerArgs g;
    g.digits = dig, g.keyB = k->d_b, g.keyA = k->d_a, g.out0 = out0, g.out1 = out1, g.lc = c->d_lc, g.mu128 = c->d_mu128;
    g.logN = c->logN, g.batch = batch, g.sizeQl = sizeQl, g.sizeQ = k->sizeQ, g.acc = 0;
    g.D = fhe_crt_decompose_towers(c, nullptr, sizeQl, k->baseBits);  // the key's first D_l towers
    BvOutStage e;
    e.add0 = add0, e.add1 = add1, e.outRows = outRows, e.kInv = kInv, e.useHat = hat != nullptr;
    for (uint32_t i = 0; i < (uint32_t)kConstVecLimbs; ++i) {
        const uint64_t v = hat && i < sizeQl ? hat[i] % c->q[i] : 0;
        e.hat.c[i]       = TwPair{v, hat && i < sizeQl ? host::shoup(v, c->q[i]) : 0};
    }
    const uint32_t tilesPerRow = c->N >= (uint32_t)kTile ? (c->N >> kTileLog) : 1u;
    const uint64_t grid        = (((uint64_t)tilesPerRow * outRows + 7) / 8) * 8 * batch;
    ARG_CHECK(grid < ((uint64_t)1 << 31), std::string(who) + ": batch too large for one launch");
    // two adjacent coefficients per lane need 16-byte aligned towers (any device allocation is) and N >= 2
    const uintptr_t bits = (uintptr_t)dig | (uintptr_t)k->d_b | (uintptr_t)k->d_a | (uintptr_t)out0 | (uintptr_t)out1 | (uintptr_t)add0 | (uintptr_t)add1;
    if ((bits & 15u) == 0 && c->N >= 2)
        FHE_LAUNCH((bv_inner_product_kernel<2, true>), grid, st, g, e);
    else
        FHE_LAUNCH((bv_inner_product_kernel<1, true>), grid, st, g, e);
    LAUNCH_CHECK();
    return FHE_OK;
}
// LeveledSHEBase::EvalFastRotation (base-leveledshe.cpp:432-463) with a BV key, on the digits fhe_bv_precompute(c1) left in ws
extern "C" fhe_status fhe_bv_eval_fast_rotation(const fhe_bv_key* k, const uint64_t* c0, uint32_t kAuto, uint32_t sizeQl, uint32_t batch,
                                                uint64_t* out0, uint64_t* out1, const void* ws, size_t wsBytes, void* st) {
    if (fhe_status s = bv_fast_check(k, sizeQl, batch, out0, out1, ws, wsBytes, "fhe_bv_eval_fast_rotation"))
        return s;
    ARG_CHECK(c0, "fhe_bv_eval_fast_rotation: null argument");
    ARG_CHECK(out0 != c0 && out1 != c0, "fhe_bv_eval_fast_rotation: the outputs must not alias c0");
    ARG_CHECK(kAuto % 2 == 1, "Automorphism index not odd");
    return bv_out_run(k, sizeQl, sizeQl, batch, (const uint64_t*)ws, nullptr, c0, nullptr, kAuto, out0, out1, st, "fhe_bv_eval_fast_rotation");
}
// LeveledSHEBase::EvalAutomorphism (base-leveledshe.cpp:381-422) with a BV key = precompute + fast rotation
extern "C" fhe_status fhe_bv_eval_automorphism(const fhe_bv_key* k, const uint64_t* c0, const uint64_t* c1, uint32_t kAuto, uint32_t sizeQl,
                                               uint32_t batch, uint64_t* out0, uint64_t* out1, void* ws, size_t wsBytes, void* st) {
    if (fhe_status s = bv_fast_check(k, sizeQl, batch, out0, out1, ws, wsBytes, "fhe_bv_eval_automorphism"))
        return s;
    ARG_CHECK(c0 && c1, "fhe_bv_eval_automorphism: null argument");
    ARG_CHECK(out0 != c0 && out1 != c0, "fhe_bv_eval_automorphism: the outputs must not alias c0");
    ARG_CHECK(kAuto % 2 == 1, "Automorphism index not odd");
    if (fhe_status s = fhe_bv_precompute(k->ctx, c1, 1, sizeQl, k->baseBits, batch, ws, wsBytes, st))
        return s;
    return bv_out_run(k, sizeQl, sizeQl, batch, (const uint64_t*)ws, nullptr, c0, nullptr, kAuto, out0, out1, st, "fhe_bv_eval_automorphism");
}

// BFV, HPS family (bfvrns-leveledshe.cpp:767-938).  In HPSPOVERQLEVELED the element to be switched goes from Q down to Q_l first
// (ScaleAndRound, :806-808, :910-912), the key switch runs at sizeQl = l + 1 limbs and both results come back to Q (ExpandCRTBasisQlHat,
// :864-867, :920-923) before they are added.  At sizeQl == numQ both steps are the identity (Q_l = Q: the scaling tables are the CRT
// reconstruction with zero fractions, QlHatModq is all ones) and are skipped; HPS and HPSPOVERQ never take them (:795, :859, :903).
// workspace (words): digits [D_l][batch][sizeQl][N] | scaled / coefficient copy [batch][sizeQl][N] (the layout of fhe_bv_workspace_bytes) |
// coefficient copy over Q [batch][numQ][N]
static size_t bfv_bv_ws_words(const fhe_hps* h, uint32_t sizeQl, uint32_t baseBits, uint32_t batch) {
    if (!hps_level(h, sizeQl) || batch < 1 || sizeQl > h->ctx->L)
        return 0;
    const uint32_t D = fhe_crt_decompose_towers(h->ctx, nullptr, sizeQl, baseBits);
    if (D == 0)
        return 0;
    return (((size_t)D + 1) * batch * sizeQl + (size_t)batch * h->numQ) << h->ctx->logN;
}
extern "C" size_t fhe_bfv_bv_workspace_bytes(const fhe_hps* h, uint32_t sizeQl, uint32_t baseBits, uint32_t batch) {
    return bfv_bv_ws_words(h, sizeQl, baseBits, batch) * 8;
}
// everything a call below checks before it enqueues; key may be null (the precompute takes baseBits instead)
static fhe_status bfv_bv_check(const fhe_hps* h, const fhe_bv_key* k, uint32_t sizeQl, uint32_t baseBits, uint32_t batch, const void* ws,
                               size_t wsBytes, const char* who) {
    ARG_CHECK(h && ws && batch >= 1, std::string(who) + ": null argument");
    if (k)
        ARG_CHECK(k->ctx == h->ctx && k->sizeQ == h->numQ, std::string(who) + ": the key was built for another context or another Q");
    for (uint32_t i = 0; i < h->numQ; ++i)
        ARG_CHECK(h->qIdx[i] == i, std::string(who) + ": Q must be the context's leading limbs");
    ARG_CHECK(hps_level(h, sizeQl), std::string(who) + ": sizeQl must be numQ (1 ... numQ for HPSPOVERQLEVELED)");
    if (fhe_crt_decompose_towers(h->ctx, nullptr, sizeQl, baseBits) == 0)
        return fail(FHE_ERR_UNSUPPORTED, std::string(who) + ": digit size outside the device path (baseBits <= 31, every window inside the word)");
    const size_t need = fhe_bfv_bv_workspace_bytes(h, sizeQl, baseBits, batch);
    ARG_CHECK(need && wsBytes >= need, std::string(who) + ": workspace too small");
    return FHE_OK;
}
// x [batch][numQ][N] in evalFormat -> digits at sizeQl limbs at the start of ws (checked by the caller)
static fhe_status bfv_bv_digits(fhe_hps* h, const uint64_t* x, int evalFormat, uint32_t sizeQl, uint32_t baseBits, uint32_t batch, void* ws,
                                size_t wsBytes, void* st) {
    fhe_ctx* c = h->ctx;
    if (sizeQl == h->numQ)
        return fhe_bv_precompute(c, x, evalFormat, sizeQl, baseBits, batch, ws, wsBytes, st);
    const uint32_t D = fhe_crt_decompose_towers(c, nullptr, sizeQl, baseBits);
    uint64_t* scaled = (uint64_t*)ws + (((size_t)D * batch * sizeQl) << c->logN);
    uint64_t* coef   = scaled + (((size_t)batch * sizeQl) << c->logN);
    if (evalFormat) {
        if (fhe_status s = fhe_ntt_inv_oop(c, x, coef, nullptr, h->numQ, batch, st))
            return s;
        x = coef;
    }
    if (fhe_status s = fhe_scale_and_round(hps_level(h, sizeQl)->drop, x, 1, scaled, batch, st))
        return s;
    return fhe_bv_precompute(c, scaled, 0, sizeQl, baseBits, batch, ws, wsBytes, st);
}
static const uint64_t* bfv_bv_hat(const fhe_hps* h, uint32_t sizeQl) {
    return sizeQl == h->numQ ? nullptr : hps_level(h, sizeQl)->QlHatModq.data();
}
// LeveledSHEBFVRNS::EvalFastRotationPrecompute (bfvrns-leveledshe.cpp:782-813)
extern "C" fhe_status fhe_bfv_fast_rotation_precompute_bv(fhe_hps* h, const uint64_t* c1, uint32_t sizeQl, uint32_t baseBits, uint32_t batch,
                                                          void* ws, size_t wsBytes, void* st) {
    ARG_CHECK(c1, "fhe_bfv_fast_rotation_precompute_bv: null argument");
    if (fhe_status s = bfv_bv_check(h, nullptr, sizeQl, baseBits, batch, ws, wsBytes, "fhe_bfv_fast_rotation_precompute_bv"))
        return s;
    return bfv_bv_digits(h, c1, 1, sizeQl, baseBits, batch, ws, wsBytes, st);
}
// LeveledSHEBFVRNS::EvalFastRotation (bfvrns-leveledshe.cpp:815-882) on the digits the precompute left in ws
extern "C" fhe_status fhe_bfv_eval_fast_rotation_bv(fhe_hps* h, const fhe_bv_key* k, const uint64_t* c0, uint32_t kAuto, uint32_t sizeQl,
                                                    uint32_t batch, uint64_t* out0, uint64_t* out1, const void* ws, size_t wsBytes, void* st) {
    ARG_CHECK(k && c0 && out0 && out1, "fhe_bfv_eval_fast_rotation_bv: null argument");
    ARG_CHECK(out0 != c0 && out1 != c0, "fhe_bfv_eval_fast_rotation_bv: the outputs must not alias c0");
    ARG_CHECK(kAuto % 2 == 1, "Automorphism index not odd");
    if (fhe_status s = bfv_bv_check(h, k, sizeQl, k->baseBits, batch, ws, wsBytes, "fhe_bfv_eval_fast_rotation_bv"))
        return s;
    return bv_out_run(k, sizeQl, h->numQ, batch, (const uint64_t*)ws, bfv_bv_hat(h, sizeQl), c0, nullptr, kAuto, out0, out1, st,
                      "fhe_bfv_eval_fast_rotation_bv");
}
// LeveledSHEBFVRNS::EvalAutomorphism (bfvrns-leveledshe.cpp:767-780): RelinearizeCore on two elements, then both through the automorphism
extern "C" fhe_status fhe_bfv_eval_automorphism_bv(fhe_hps* h, const fhe_bv_key* k, const uint64_t* c0, const uint64_t* c1, uint32_t kAuto,
                                                   uint32_t sizeQl, uint32_t batch, uint64_t* out0, uint64_t* out1, void* ws, size_t wsBytes,
                                                   void* st) {
    ARG_CHECK(k && c0 && c1 && out0 && out1, "fhe_bfv_eval_automorphism_bv: null argument");
    ARG_CHECK(out0 != c0 && out1 != c0, "fhe_bfv_eval_automorphism_bv: the outputs must not alias c0");
    ARG_CHECK(kAuto % 2 == 1, "Automorphism index not odd");
    if (fhe_status s = bfv_bv_check(h, k, sizeQl, k->baseBits, batch, ws, wsBytes, "fhe_bfv_eval_automorphism_bv"))
        return s;
    if (fhe_status s = bfv_bv_digits(h, c1, 1, sizeQl, k->baseBits, batch, ws, wsBytes, st))
        return s;
    return bv_out_run(k, sizeQl, h->numQ, batch, (const uint64_t*)ws, bfv_bv_hat(h, sizeQl), c0, nullptr, kAuto, out0, out1, st,
                      "fhe_bfv_eval_automorphism_bv");
}
// LeveledSHEBFVRNS::RelinearizeCore on three elements (bfvrns-leveledshe.cpp:888-938).  inEval == 0: d2 goes straight into ScaleAndRound (the
// reference's SetFormat(COEFFICIENT), :910, finds it there already), d0 / d1 are transformed once, into c0 / c1, and the kernel adds in place.
extern "C" fhe_status fhe_bfv_relinearize_bv(fhe_hps* h, const fhe_bv_key* k, const uint64_t* d0, const uint64_t* d1, const uint64_t* d2,
                                             int inEval, uint32_t sizeQl, uint32_t batch, uint64_t* c0, uint64_t* c1, void* ws, size_t wsBytes,
                                             void* st) {
    ARG_CHECK(k && d0 && d1 && d2 && c0 && c1, "fhe_bfv_relinearize_bv: null argument");
    if (fhe_status s = bfv_bv_check(h, k, sizeQl, k->baseBits, batch, ws, wsBytes, "fhe_bfv_relinearize_bv"))
        return s;
    fhe_ctx* c = h->ctx;
    if (fhe_status s = bfv_bv_digits(h, d2, inEval, sizeQl, k->baseBits, batch, ws, wsBytes, st))
        return s;
    if (!inEval) {
        if (fhe_status s = fhe_ntt_fwd_oop(c, d0, c0, nullptr, h->numQ, batch, st))
            return s;
        if (fhe_status s = fhe_ntt_fwd_oop(c, d1, c1, nullptr, h->numQ, batch, st))
            return s;
        d0 = c0, d1 = c1;
    }
    return bv_out_run(k, sizeQl, h->numQ, batch, (const uint64_t*)ws, bfv_bv_hat(h, sizeQl), d0, d1, 1, c0, c1, st, "fhe_bfv_relinearize_bv");
}
// LeveledSHEBFVRNS::EvalMult(ct, ct, key) (bfvrns-leveledshe.cpp:735-741): the product at sizeQlMult with d0, d1 left in c0, c1 and d2 in ws,
// COEFFICIENT as the reference leaves them, then the relinearisation at sizeQlRelin.
// workspace (bytes): d2 [batch][numQ][N] | max(the product's, the relinearisation's)
extern "C" size_t fhe_bfv_eval_mult_relin_hps_bv_leveled_workspace_bytes(const fhe_hps* h, uint32_t sizeQlMult, uint32_t sizeQlRelin,
                                                                         uint32_t baseBits, uint32_t batch) {
    const size_t mul = fhe_bfv_eval_mult_hps_workspace_bytes(h, sizeQlMult, batch);
    const size_t ks  = fhe_bfv_bv_workspace_bytes(h, sizeQlRelin, baseBits, batch);
    if (!mul || !ks)
        return 0;
    return ((((size_t)batch * h->numQ) << h->ctx->logN) * 8) + std::max(mul, ks);
}
extern "C" fhe_status fhe_bfv_eval_mult_relin_hps_bv_leveled(fhe_hps* h, const fhe_bv_key* k, const uint64_t* a0, const uint64_t* a1,
                                                             const uint64_t* b0, const uint64_t* b1, uint64_t* c0, uint64_t* c1,
                                                             uint32_t sizeQlMult, uint32_t sizeQlRelin, uint32_t batch, void* ws,
                                                             size_t wsBytes, void* st) {
    ARG_CHECK(h && k && a0 && a1 && b0 && b1 && c0 && c1 && ws && batch >= 1, "fhe_bfv_eval_mult_relin_hps_bv_leveled: null argument");
    ARG_CHECK(hps_level(h, sizeQlMult), "fhe_bfv_eval_mult_relin_hps_bv_leveled: sizeQlMult must be numQ (1 ... numQ for HPSPOVERQLEVELED)");
    const size_t d2Bytes = (((size_t)batch * h->numQ) << h->ctx->logN) * 8;
    if (fhe_status s = bfv_bv_check(h, k, sizeQlRelin, k->baseBits, batch, ws, ~(size_t)0, "fhe_bfv_eval_mult_relin_hps_bv_leveled"))
        return s;  // (everything but the size, which is this call's own)
    const size_t need = fhe_bfv_eval_mult_relin_hps_bv_leveled_workspace_bytes(h, sizeQlMult, sizeQlRelin, k->baseBits, batch);
    ARG_CHECK(need && wsBytes >= need, "fhe_bfv_eval_mult_relin_hps_bv_leveled: workspace too small");
    uint64_t* d2 = (uint64_t*)ws;
    void* rest   = (char*)ws + d2Bytes;
    if (fhe_status s = fhe_bfv_eval_mult_hps(h, a0, a1, b0, b1, c0, c1, d2, sizeQlMult, 0, batch, rest, wsBytes - d2Bytes, st))
        return s;
    return fhe_bfv_relinearize_bv(h, k, c0, c1, d2, 0, sizeQlRelin, batch, c0, c1, rest, wsBytes - d2Bytes, st);
}

// ---- BFV, HPS family, on HYBRID keys ------------------------------------------------------------------------------------------------------
// The members of "rotations and leveled relinearisation on a BV key" above with KeySwitchHYBRID in the middle (bfvrns-leveledshe.cpp:767-938,
// keyswitch-hybrid.cpp:308-400).  Below the top level the element goes Q -> Q_l (ScaleAndRound) straight into the key switch's coefficient
// buffer, the key switch runs at sizeQl limbs with the ModDown constant C'_i = [P^-1]_{q_i} * QlHatModq(l)[i] mod q_i -- ((A - sw) * P^-1 mod q)
// * QlHat mod q and (A - sw) * C' mod q are the same canonical residue, so ExpandCRTBasisQlHat's product costs nothing -- and
// bfv_hybrid_tail_kernel zero-extends to numQ rows, adds the ciphertext's own elements and applies the automorphism, one launch.
// workspace (words): the key switch's layout at sizeQl (ks_layout: coef = the scaled COEFFICIENT tower, d2 = its EVALUATION copy, whose own
// limbs the inner product reads, k0 / k1 = the two ModDown results) | below numQ: coefficient copy over Q [batch][numQ][N]
struct fhe_bfv_hybrid {
    fhe_hps* h;
    fhe_ks_plan* ks;
    std::vector<fhe_ks_plan::Level*> lv;  // index sizeQl; null: a level the technique cannot use
    std::vector<TwPair*> d_C;             // index sizeQl: C' as device Shoup pairs [sizeQl]; null at numQ (QlHatModq is all ones: the level's own P^-1)
    std::vector<void*> owned;
};
extern "C" void fhe_bfv_hybrid_destroy(fhe_bfv_hybrid* bh) {
    if (!bh)
        return;
    for (void* p : bh->owned)
        rt::dfree(p);
    delete bh;
}
extern "C" fhe_status fhe_bfv_hybrid_create(fhe_hps* h, fhe_ks_plan* ks, fhe_bfv_hybrid** out) {
    ARG_CHECK(h && ks && out, "fhe_bfv_hybrid_create: null argument");
    ARG_CHECK(h->ctx == ks->ctx, "fhe_bfv_hybrid_create: the two plans were built for different contexts");
    for (uint32_t i = 0; i < h->numQ; ++i)
        ARG_CHECK(h->qIdx[i] == i, "fhe_bfv_hybrid_create: Q must be the context's leading limbs");
    ARG_CHECK(ks->sizeQ == h->numQ, "fhe_bfv_hybrid_create: the key-switch plan's Q must be the HPS plan's Q");
    fhe_ctx* c = h->ctx;
    RT_CHECK(rt::set_device(c->device));
    fhe_bfv_hybrid* bh = new fhe_bfv_hybrid;
    bh->h = h, bh->ks = ks;
    bh->lv.assign(h->numQ + 1, nullptr), bh->d_C.assign(h->numQ + 1, nullptr);
    std::vector<uint64_t> pm(ks->sizeP);
    for (uint32_t j = 0; j < ks->sizeP; ++j)
        pm[j] = c->q[ks->sizeQ + j];
    for (uint32_t sizeQl = h->technique == 3 ? 1u : h->numQ; sizeQl <= h->numQ; ++sizeQl) {
        fhe_status s = ks_level(ks, sizeQl, &bh->lv[sizeQl]);  // (every level now: no call below builds one)
        if (!s && sizeQl < h->numQ) {
            const std::vector<uint64_t>& hat = hps_level(h, sizeQl)->QlHatModq;
            std::vector<TwPair> cp(sizeQl);
            for (uint32_t i = 0; i < sizeQl; ++i) {
                const uint64_t qi = c->q[i];
                const uint64_t v  = host::mulmod(host::invmod(host::prod_mod(pm, -1, qi), qi), hat[i] % qi, qi);
                cp[i]             = TwPair{v, host::shoup(v, qi)};
            }
            s = dev_copy(&bh->owned, cp.data(), cp.size(), &bh->d_C[sizeQl]);
        }
        if (s) {
            fhe_bfv_hybrid_destroy(bh);
            return s;
        }
    }
    *out = bh;
    return FHE_OK;
}
static bool bfv_hybrid_level_ok(const fhe_bfv_hybrid* bh, uint32_t sizeQl) {
    return bh && sizeQl >= 1 && sizeQl <= bh->h->numQ && bh->lv[sizeQl];
}
static size_t bfv_hybrid_ws_words(const fhe_bfv_hybrid* bh, uint32_t sizeQl, uint32_t batch) {
    if (!bfv_hybrid_level_ok(bh, sizeQl) || batch < 1)
        return 0;
    const size_t ks = ks_layout(bh->ks, sizeQl, batch).total;
    return ks + (sizeQl < bh->h->numQ ? ((size_t)batch * bh->h->numQ) << bh->h->ctx->logN : 0);
}
extern "C" size_t fhe_bfv_hybrid_workspace_bytes(const fhe_bfv_hybrid* bh, uint32_t sizeQl, uint32_t batch) {
    return bfv_hybrid_ws_words(bh, sizeQl, batch) * 8;
}
// everything a call below checks before it enqueues; key may be null (the precompute has none)
static fhe_status bfv_hybrid_check(const fhe_bfv_hybrid* bh, const fhe_ks_key* key, bool needKey, uint32_t sizeQl, uint32_t batch,
                                   const void* ws, size_t wsBytes, const char* who) {
    ARG_CHECK(bh && ws && batch >= 1 && (key || !needKey), std::string(who) + ": null argument");
    ARG_CHECK(bfv_hybrid_level_ok(bh, sizeQl), std::string(who) + ": sizeQl must be numQ (1 ... numQ for HPSPOVERQLEVELED)");
    ARG_CHECK(!key || key->plan == bh->ks, std::string(who) + ": the key belongs to another key-switch plan");
    ARG_CHECK(wsBytes >= fhe_bfv_hybrid_workspace_bytes(bh, sizeQl, batch), std::string(who) + ": workspace too small");
    const fhe_ctx* c           = bh->h->ctx;
    const uint32_t tilesPerRow = c->N >= (uint32_t)kTile ? (c->N >> kTileLog) : 1u;
    ARG_CHECK((uint64_t)tilesPerRow * bh->h->numQ * batch < ((uint64_t)1 << 31), std::string(who) + ": batch too large for one launch");
    return FHE_OK;
}
// [lo, lo + n) and [p, p + m) share a byte
static bool bfv_hybrid_overlap(const void* lo, size_t n, const void* p, size_t m) {
    const uintptr_t a = (uintptr_t)lo, b = (uintptr_t)p;
    return a < b + m && b < a + n;
}
// x [batch][numQ][N] in evalFormat -> the digits at sizeQl limbs, the scaled COEFFICIENT tower and its EVALUATION copy in ws.  (The
// EVALUATION tower whose own limbs the inner product reads is then ws's d2 -- or x itself at the top level when x is EVALUATION.)
static fhe_status bfv_hybrid_digits(fhe_bfv_hybrid* bh, const uint64_t* x, int evalFormat, uint32_t sizeQl, uint32_t batch, uint64_t* ws,
                                    const KsLayout& w, void* st) {
    fhe_hps* h             = bh->h;
    fhe_ctx* c             = h->ctx;
    fhe_ks_plan::Level* lv = bh->lv[sizeQl];
    if (sizeQl == h->numQ) {
        if (evalFormat)  // the launches of fhe_ks_precompute
            return ks_precompute_run(bh->ks, lv, x, batch, ws, w, st);
        if (fhe_status s = fhe_ntt_fwd_oop(c, x, ws + w.d2, nullptr, sizeQl, batch, st))
            return s;
        return ks_precompute_from_coef(bh->ks, lv, x, batch, ws, w, st);
    }
    if (evalFormat) {
        uint64_t* coefQ = ws + w.total;
        if (fhe_status s = fhe_ntt_inv_oop(c, x, coefQ, nullptr, h->numQ, batch, st))
            return s;
        x = coefQ;
    }
    if (fhe_status s = fhe_scale_and_round(hps_level(h, sizeQl)->drop, x, 1, ws + w.coef, batch, st))
        return s;
    if (fhe_status s = fhe_ntt_fwd_oop(c, ws + w.coef, ws + w.d2, nullptr, sizeQl, batch, st))
        return s;
    return ks_precompute_from_coef(bh->ks, lv, ws + w.coef, batch, ws, w, st);
}
// EvalFastKeySwitchCore at sizeQl on the digits in ws (results in ws: k0, k1), then the tail kernel
static fhe_status bfv_hybrid_fast(fhe_bfv_hybrid* bh, const fhe_ks_key* key, const uint64_t* cin, const uint64_t* add0, const uint64_t* add1,
                                  uint32_t kAuto, uint32_t sizeQl, uint32_t batch, uint64_t* out0, uint64_t* out1, uint64_t* ws,
                                  const KsLayout& w, void* st, const char* who) {
    fhe_hps* h = bh->h;
    fhe_ctx* c = h->ctx;
    const uint32_t twoNmask = (2u << c->logN) - 1u;
    uint32_t kInv = kAuto;  // Newton: the inverse of an odd k modulo 2^32, then modulo 2N
    for (int it = 0; it < 5; ++it)
        kInv *= 2u - kAuto * kInv;
    kInv &= twoNmask;
    const uint32_t tilesPerRow = c->N >= (uint32_t)kTile ? (c->N >> kTileLog) : 1u;
    const uint64_t grid        = (uint64_t)tilesPerRow * h->numQ * batch;  // (< 2^31: bfv_hybrid_check)
    RT_CHECK(rt::set_device(c->device));
    if (fhe_status s = ks_fast_run(bh->ks, bh->lv[sizeQl], key, cin, batch, ws + w.k0, ws + w.k1, ws, w, st, false, 0, bh->d_C[sizeQl]))
        return s;
    BfvHybridTailArgs g;
    g.t0 = ws + w.k0, g.t1 = ws + w.k1, g.add0 = add0, g.add1 = add1, g.out0 = out0, g.out1 = out1, g.lc = c->d_lc;
    g.logN = c->logN, g.batch = batch, g.sizeQl = sizeQl, g.outRows = h->numQ, g.kInv = kInv;
    // two adjacent coefficients per lane need 16-byte aligned towers (any device allocation is) and N >= 2
    const uintptr_t bits = (uintptr_t)g.t0 | (uintptr_t)g.t1 | (uintptr_t)add0 | (uintptr_t)add1 | (uintptr_t)out0 | (uintptr_t)out1;
    if ((bits & 15u) == 0 && c->N >= 2)
        FHE_LAUNCH((bfv_hybrid_tail_kernel<2>), grid, st, g);
    else
        FHE_LAUNCH((bfv_hybrid_tail_kernel<1>), grid, st, g);
    LAUNCH_CHECK();
    return FHE_OK;
}
// the checks the two rotation entries share: k odd, outputs apart from c0, c1 and ws
static fhe_status bfv_hybrid_rot_check(const fhe_bfv_hybrid* bh, const uint64_t* c0, const uint64_t* c1, uint32_t kAuto, uint32_t sizeQl,
                                       uint32_t batch, const uint64_t* out0, const uint64_t* out1, const void* ws, const char* who) {
    ARG_CHECK(kAuto % 2 == 1, "Automorphism index not odd");
    const size_t tower = (((size_t)batch * bh->h->numQ) << bh->h->ctx->logN) * 8, wsB = fhe_bfv_hybrid_workspace_bytes(bh, sizeQl, batch);
    for (const uint64_t* o : {out0, out1})
        ARG_CHECK(!bfv_hybrid_overlap(o, tower, c0, tower) && !bfv_hybrid_overlap(o, tower, c1, tower) && !bfv_hybrid_overlap(o, tower, ws, wsB),
                  std::string(who) + ": the outputs must not alias c0, c1 or ws");
    ARG_CHECK(!bfv_hybrid_overlap(out0, tower, out1, tower), std::string(who) + ": the outputs must not alias each other");
    return FHE_OK;
}
// LeveledSHEBFVRNS::EvalFastRotationPrecompute (bfvrns-leveledshe.cpp:782-813) with KeySwitchHYBRID::EvalKeySwitchPrecomputeCore
extern "C" fhe_status fhe_bfv_fast_rotation_precompute_hybrid(fhe_bfv_hybrid* bh, const uint64_t* c1, uint32_t sizeQl, uint32_t batch, void* ws,
                                                              size_t wsBytes, void* st) {
    ARG_CHECK(c1, "fhe_bfv_fast_rotation_precompute_hybrid: null argument");
    if (fhe_status s = bfv_hybrid_check(bh, nullptr, false, sizeQl, batch, ws, wsBytes, "fhe_bfv_fast_rotation_precompute_hybrid"))
        return s;
    RT_CHECK(rt::set_device(bh->h->ctx->device));
    return bfv_hybrid_digits(bh, c1, 1, sizeQl, batch, (uint64_t*)ws, ks_layout(bh->ks, sizeQl, batch), st);
}
// LeveledSHEBFVRNS::EvalFastRotation (bfvrns-leveledshe.cpp:815-882) on the digits the precompute left in ws
extern "C" fhe_status fhe_bfv_eval_fast_rotation_hybrid(fhe_bfv_hybrid* bh, const fhe_ks_key* key, const uint64_t* c0, const uint64_t* c1,
                                                        uint32_t kAuto, uint32_t sizeQl, uint32_t batch, uint64_t* out0, uint64_t* out1,
                                                        void* ws, size_t wsBytes, void* st) {
    ARG_CHECK(c0 && c1 && out0 && out1, "fhe_bfv_eval_fast_rotation_hybrid: null argument");
    if (fhe_status s = bfv_hybrid_check(bh, key, true, sizeQl, batch, ws, wsBytes, "fhe_bfv_eval_fast_rotation_hybrid"))
        return s;
    if (fhe_status s = bfv_hybrid_rot_check(bh, c0, c1, kAuto, sizeQl, batch, out0, out1, ws, "fhe_bfv_eval_fast_rotation_hybrid"))
        return s;
    const KsLayout w = ks_layout(bh->ks, sizeQl, batch);
    uint64_t* wsp    = (uint64_t*)ws;
    return bfv_hybrid_fast(bh, key, sizeQl == bh->h->numQ ? c1 : wsp + w.d2, c0, nullptr, kAuto, sizeQl, batch, out0, out1, wsp, w, st,
                           "fhe_bfv_eval_fast_rotation_hybrid");
}
// LeveledSHEBFVRNS::EvalAutomorphism (bfvrns-leveledshe.cpp:767-780): RelinearizeCore on two elements, then both through the automorphism
extern "C" fhe_status fhe_bfv_eval_automorphism_hybrid(fhe_bfv_hybrid* bh, const fhe_ks_key* key, const uint64_t* c0, const uint64_t* c1,
                                                       uint32_t kAuto, uint32_t sizeQl, uint32_t batch, uint64_t* out0, uint64_t* out1,
                                                       void* ws, size_t wsBytes, void* st) {
    ARG_CHECK(c0 && c1 && out0 && out1, "fhe_bfv_eval_automorphism_hybrid: null argument");
    if (fhe_status s = bfv_hybrid_check(bh, key, true, sizeQl, batch, ws, wsBytes, "fhe_bfv_eval_automorphism_hybrid"))
        return s;
    if (fhe_status s = bfv_hybrid_rot_check(bh, c0, c1, kAuto, sizeQl, batch, out0, out1, ws, "fhe_bfv_eval_automorphism_hybrid"))
        return s;
    const KsLayout w = ks_layout(bh->ks, sizeQl, batch);
    uint64_t* wsp    = (uint64_t*)ws;
    RT_CHECK(rt::set_device(bh->h->ctx->device));
    if (fhe_status s = bfv_hybrid_digits(bh, c1, 1, sizeQl, batch, wsp, w, st))
        return s;
    return bfv_hybrid_fast(bh, key, sizeQl == bh->h->numQ ? c1 : wsp + w.d2, c0, nullptr, kAuto, sizeQl, batch, out0, out1, wsp, w, st,
                           "fhe_bfv_eval_automorphism_hybrid");
}
// LeveledSHEBFVRNS::RelinearizeCore on three elements (bfvrns-leveledshe.cpp:888-938).  inEval == 0: d2 goes straight into ScaleAndRound (at the
// top level: straight into the digit decomposition), d0 / d1 are transformed once, into c0 / c1, and the tail adds in place.
extern "C" fhe_status fhe_bfv_relinearize_hybrid(fhe_bfv_hybrid* bh, const fhe_ks_key* key, const uint64_t* d0, const uint64_t* d1,
                                                 const uint64_t* d2, int inEval, uint32_t sizeQl, uint32_t batch, uint64_t* c0, uint64_t* c1,
                                                 void* ws, size_t wsBytes, void* st) {
    ARG_CHECK(d0 && d1 && d2 && c0 && c1, "fhe_bfv_relinearize_hybrid: null argument");
    if (fhe_status s = bfv_hybrid_check(bh, key, true, sizeQl, batch, ws, wsBytes, "fhe_bfv_relinearize_hybrid"))
        return s;
    fhe_ctx* c       = bh->h->ctx;
    const KsLayout w = ks_layout(bh->ks, sizeQl, batch);
    uint64_t* wsp    = (uint64_t*)ws;
    RT_CHECK(rt::set_device(c->device));
    if (fhe_status s = bfv_hybrid_digits(bh, d2, inEval, sizeQl, batch, wsp, w, st))
        return s;
    if (!inEval) {
        if (fhe_status s = fhe_ntt_fwd_oop(c, d0, c0, nullptr, bh->h->numQ, batch, st))
            return s;
        if (fhe_status s = fhe_ntt_fwd_oop(c, d1, c1, nullptr, bh->h->numQ, batch, st))
            return s;
        d0 = c0, d1 = c1;
    }
    return bfv_hybrid_fast(bh, key, sizeQl == bh->h->numQ && inEval ? d2 : wsp + w.d2, d0, d1, 1, sizeQl, batch, c0, c1, wsp, w, st,
                           "fhe_bfv_relinearize_hybrid");
}
// LeveledSHEBFVRNS::EvalMult(ct, ct, key) (bfvrns-leveledshe.cpp:735-741): the product at sizeQlMult with d0, d1 left in c0, c1 and d2 in ws,
// COEFFICIENT as the reference leaves them, then the relinearisation at sizeQlRelin.
// workspace (bytes): d2 [batch][numQ][N] | max(the product's, the relinearisation's)
extern "C" size_t fhe_bfv_eval_mult_relin_hps_hybrid_workspace_bytes(const fhe_bfv_hybrid* bh, uint32_t sizeQlMult, uint32_t sizeQlRelin,
                                                                     uint32_t batch) {
    if (!bh)
        return 0;
    const size_t mul = fhe_bfv_eval_mult_hps_workspace_bytes(bh->h, sizeQlMult, batch);
    const size_t ks  = fhe_bfv_hybrid_workspace_bytes(bh, sizeQlRelin, batch);
    if (!mul || !ks)
        return 0;
    return ((((size_t)batch * bh->h->numQ) << bh->h->ctx->logN) * 8) + std::max(mul, ks);
}
extern "C" fhe_status fhe_bfv_eval_mult_relin_hps_hybrid(fhe_bfv_hybrid* bh, const fhe_ks_key* key, const uint64_t* a0, const uint64_t* a1,
                                                         const uint64_t* b0, const uint64_t* b1, uint64_t* c0, uint64_t* c1,
                                                         uint32_t sizeQlMult, uint32_t sizeQlRelin, uint32_t batch, void* ws, size_t wsBytes,
                                                         void* st) {
    ARG_CHECK(bh && key && a0 && a1 && b0 && b1 && c0 && c1 && ws && batch >= 1, "fhe_bfv_eval_mult_relin_hps_hybrid: null argument");
    ARG_CHECK(hps_level(bh->h, sizeQlMult), "fhe_bfv_eval_mult_relin_hps_hybrid: sizeQlMult must be numQ (1 ... numQ for HPSPOVERQLEVELED)");
    if (fhe_status s = bfv_hybrid_check(bh, key, true, sizeQlRelin, batch, ws, ~(size_t)0, "fhe_bfv_eval_mult_relin_hps_hybrid"))
        return s;  // (everything but the size, which is this call's own)
    const size_t need = fhe_bfv_eval_mult_relin_hps_hybrid_workspace_bytes(bh, sizeQlMult, sizeQlRelin, batch);
    ARG_CHECK(need && wsBytes >= need, "fhe_bfv_eval_mult_relin_hps_hybrid: workspace too small");
    const size_t d2Bytes = (((size_t)batch * bh->h->numQ) << bh->h->ctx->logN) * 8;
    uint64_t* d2 = (uint64_t*)ws;
    void* rest   = (char*)ws + d2Bytes;
    if (fhe_status s = fhe_bfv_eval_mult_hps(bh->h, a0, a1, b0, b1, c0, c1, d2, sizeQlMult, 0, batch, rest, wsBytes - d2Bytes, st))
        return s;
    return fhe_bfv_relinearize_hybrid(bh, key, c0, c1, d2, 0, sizeQlRelin, batch, c0, c1, rest, wsBytes - d2Bytes, st);
}

// whole-tower checksums (checksum_kernel): out[row] = {sum_i w_i, sum_i (2i + 1) w_i} mod 2^64 of every limb-row of x[rows][N]; out is DEVICE memory
extern "C" fhe_status fhe_checksum(fhe_ctx* c, const uint64_t* x, uint32_t rows, uint64_t* out, void* st) {
    ARG_CHECK(c && x && out && rows >= 1, "fhe_checksum: bad argument");
    RT_CHECK(rt::set_device(c->device));
    RT_CHECK(rt::dzero(out, (size_t)rows * 16, (rt::stream_t)st));
    ChecksumArgs g;
    g.x = x, g.out = out, g.logN = c->logN, g.rows = rows;
    const uint32_t tileLog = std::min<uint32_t>(c->logN, kTileLog);
    FHE_LAUNCH_BARRIER(checksum_kernel, ((uint64_t)rows << c->logN) >> tileLog, st, g);
    LAUNCH_CHECK();
    return FHE_OK;
}

extern "C" size_t fhe_launch_stats(char* buf, size_t cap, uint64_t* total) {
    std::map<std::string, uint64_t> byKernel;
    uint64_t sum = 0;
    for (auto* s = fhe::rt::LaunchSite::head().load(); s; s = s->next) {
        std::string k = s->kernel;
        k = k.substr(0, k.find('<'));
        k.erase(std::remove(k.begin(), k.end(), '('), k.end());
        byKernel[k] += s->n.load();
        if (s->label[0])  // a labelled site (the NTT passes' hand-over instances: <HAND>; those of the 6 + 10 split: <SPLIT6>) once more, on a line of its own (not in the total twice)
            byKernel[k + "<" + s->label + ">"] += s->n.load();
        sum += s->n.load();
    }
    std::vector<std::pair<uint64_t, std::string>> v;
    for (auto& kv : byKernel)
        if (kv.second)
            v.emplace_back(kv.second, kv.first);
    std::sort(v.rbegin(), v.rend());
    std::string text;
    for (auto& e : v)
        text += e.second + " " + std::to_string(e.first) + "\n";
    if (total)
        *total = sum;
    if (buf && cap) {
        const size_t n = std::min(cap - 1, text.size());
        std::memcpy(buf, text.data(), n);
        buf[n] = 0;
    }
    return text.size() + 1;
}
