/*
 * fhe_hip.h — C ABI of the MI355X (gfx950) RNS polynomial-arithmetic backend for OpenFHE's DCRTPoly
 * hot path.  This is the drop-in boundary: a thin `lattice/hal/hip/` HAL shim implementing
 * lbcrypto::DCRTPolyInterface and the standalone parity/benchmark harness both
 * bind exactly these entry points.  The reference has no FFI of its own — its "operator API" is the C++
 * class surface selected at compile time by src/core/include/lattice/hal/lat-backend.h:39-61 — so each
 * entry point cites the reference member function(s) it replaces (paths relative to
 * openfhe-development/).
 *
 * Conventions
 *  - plain C types only; every call returns fhe_status (0 = OK), no exceptions cross the ABI;
 *    fhe_last_error() returns the message of the last failure on the calling thread
 *    (the C++ shim re-throws it with OPENFHE_THROW so callers see the reference's behaviour);
 *  - a tower lives in DEVICE memory as uint64_t[batch][nLimbs][N], limb-major, N contiguous, every word
 *    a canonical residue in [0, q_limb) (reference: std::vector<PolyImpl<NativeVector>>,
 *    src/core/include/lattice/hal/default/dcrtpoly.h:395-397); `limbIdx[r]` maps tower row r to a limb
 *    of the context (NULL = identity), which is how towers at lower levels, digits and the Q∪P
 *    extension share one context;
 *  - the caller owns all tower memory (fhe_malloc/fhe_free or any other device allocation, e.g. a
 *    torch tensor's data_ptr); the library owns its context/plan tables behind opaque handles;
 *  - all work is asynchronous on `stream` (a hipStream_t passed as void*, NULL = default stream);
 *    fhe_stream_sync() or the caller's own hip sync makes results visible;
 *  - there is NO CPU fallback: if no gfx950 device is usable every entry point fails with
 *    FHE_ERR_DEVICE.
 */
#ifndef FHE_HIP_H
#define FHE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int fhe_status;
enum {
    FHE_OK          = 0,
    FHE_ERR_ARG     = 1, /* bad argument (the reference would OPENFHE_THROW) */
    FHE_ERR_DEVICE  = 2, /* HIP runtime failure / no device */
    FHE_ERR_ALLOC   = 3,
    FHE_ERR_UNSUPPORTED = 4
};

typedef struct fhe_ctx fhe_ctx;          /* ring + modulus tower + device twiddle tables */
typedef struct fhe_conv fhe_conv;        /* one CRT basis-conversion plan (tables on device) */
typedef struct fhe_ks_plan fhe_ks_plan;  /* HYBRID key-switching plan for a (Q, P, dnum) */
typedef struct fhe_ks_key fhe_ks_key;    /* an evaluation key resident on the device */

const char* fhe_last_error(void);
const char* fhe_version(void);
/* number of usable devices (hipGetDeviceCount); 0 if none */
int fhe_device_count(void);

/* ---- context -------------------------------------------------------------------------------------
 * Replaces ILDCRTParams + the lazily built static twiddle cache
 * (src/core/include/lattice/hal/default/ildcrtparams.h:70-372,
 *  ChineseRemainderTransformFTTNat::PreCompute, src/core/include/math/hal/intnat/transformnat-impl.h:714-756).
 * q[i] prime < 2^60 with q[i] = 1 mod 2N, psi[i] a primitive 2N-th root of unity mod q[i] (the reference
 * uses RootOfUnity(), the minimum one). Tables are built eagerly and are immutable afterwards.
 * logN in [4, 17]; nLimbs <= 256 (rows of one tower and limbs of one context; round 6, until then 128). */
fhe_status fhe_ctx_create(uint32_t logN, uint32_t nLimbs, const uint64_t* q, const uint64_t* psi, int device,
                          fhe_ctx** out);
void       fhe_ctx_destroy(fhe_ctx* ctx);
uint32_t   fhe_ctx_logn(const fhe_ctx* ctx);
uint32_t   fhe_ctx_limbs(const fhe_ctx* ctx);
int        fhe_ctx_device(const fhe_ctx* ctx);

/* ---- memory / streams ---------------------------------------------------------------------------- */
fhe_status fhe_malloc(fhe_ctx* ctx, size_t bytes, void** devPtr);
fhe_status fhe_free(fhe_ctx* ctx, void* devPtr);
/* free / total bytes of the context's device (hipMemGetInfo): a host runtime that caches released buffers (the HAL backend of
 * DCRTPoly) keeps a reserve for kernel launches with it */
fhe_status fhe_mem_info(fhe_ctx* ctx, size_t* freeBytes, size_t* totalBytes);
fhe_status fhe_memcpy_h2d(fhe_ctx* ctx, void* dst, const void* src, size_t bytes, void* stream);
fhe_status fhe_memcpy_d2h(fhe_ctx* ctx, void* dst, const void* src, size_t bytes, void* stream);
fhe_status fhe_memcpy_d2d(fhe_ctx* ctx, void* dst, const void* src, size_t bytes, void* stream);
fhe_status fhe_stream_sync(fhe_ctx* ctx, void* stream);
/* Streams and graphs.  Every entry point only enqueues work on the caller's stream, so a sequence of calls (an EvalMult, a
 * BFV EvalMult, a rotation ... 20-60 kernel launches) can be recorded ONCE into a HIP graph and replayed with a single
 * launch: fhe_graph_begin(stream) ... calls on that stream ... fhe_graph_end(stream, &graph); fhe_graph_launch(graph,
 * stream).  Run the sequence once before capturing (tables are built on first use; building is not capturable). */
fhe_status fhe_stream_create(fhe_ctx* ctx, void** stream);
fhe_status fhe_stream_destroy(fhe_ctx* ctx, void* stream);
/* `stream` waits ON THE DEVICE (the host is not blocked) for everything enqueued so far on `other`: the hand-over of a tower
 * from one host thread's stream to another's (the HAL backend gives every host thread a stream of its own). */
fhe_status fhe_stream_wait(fhe_ctx* ctx, void* stream, void* other);
/* Completion marks: an event recorded on `stream` NOW; another stream waits for it on the device later.  Exact where fhe_stream_wait is
 * not (that one makes the waiter follow everything the other stream has enqueued by the time of the call): the HAL backend marks every
 * released buffer it caches, so that a host thread reusing another thread's buffer waits for that buffer's last use only. */
fhe_status fhe_event_create(fhe_ctx* ctx, void** event);
fhe_status fhe_event_record(fhe_ctx* ctx, void* event, void* stream);
fhe_status fhe_stream_wait_event(fhe_ctx* ctx, void* stream, void* event);
fhe_status fhe_event_destroy(fhe_ctx* ctx, void* event);
fhe_status fhe_memset_zero(fhe_ctx* ctx, void* dst, size_t bytes, void* stream);
fhe_status fhe_graph_begin(fhe_ctx* ctx, void* stream);
fhe_status fhe_graph_end(fhe_ctx* ctx, void* stream, void** graph);
fhe_status fhe_graph_launch(fhe_ctx* ctx, void* graph, void* stream);
void       fhe_graph_destroy(void* graph);

/* ---- a4/a5/a6: NTT -------------------------------------------------------------------------------
 * Replaces DCRTPolyImpl::SwitchFormat (dcrtpoly-impl.h:1932-1940) -> PolyImpl::SwitchFormat
 * (poly-impl.h:420-440) -> ChineseRemainderTransformFTTNat::ForwardTransformToBitReverseInPlace /
 * InverseTransformFromBitReverseInPlace (transformnat-impl.h:648-657, 678-690; loops :303-374, :512-625).
 * In place on x[batch][nLimbs][N] (or out of place with xin != xout); forward = COEFFICIENT -> EVALUATION
 * (natural -> bit-reversed order), inverse = EVALUATION -> COEFFICIENT (1/N folded in). */
fhe_status fhe_ntt_fwd(fhe_ctx* ctx, uint64_t* x, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, void* stream);
fhe_status fhe_ntt_inv(fhe_ctx* ctx, uint64_t* x, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, void* stream);
fhe_status fhe_ntt_fwd_oop(fhe_ctx* ctx, const uint64_t* xin, uint64_t* xout, const uint32_t* limbIdx, uint32_t nLimbs,
                           uint32_t batch, void* stream);
fhe_status fhe_ntt_inv_oop(fhe_ctx* ctx, const uint64_t* xin, uint64_t* xout, const uint32_t* limbIdx, uint32_t nLimbs,
                           uint32_t batch, void* stream);

/* Negacyclic polynomial product of COEFFICIENT-format towers, c = a * b in Z_q[x]/(x^N + 1) per limb: what the reference
 * spells a.SetFormat(EVALUATION); b.SetFormat(EVALUATION); c = a * b; c.SetFormat(COEFFICIENT)
 * (dcrtpoly-impl.h:1932-1940 with transformnat-impl.h:303-374, 512-625; dcrtpoly.h:174-189).  a and b are not modified; out may
 * not alias them.  Two-pass rings run fused kernels (the forward row pass of b, the Hadamard product and the inverse row
 * pass are one kernel: SURVEY.md 8(d) "fused fwd o mul o inv").  ws: 2 towers of device workspace. */
size_t     fhe_poly_mul_workspace_bytes(const fhe_ctx* ctx, uint32_t nLimbs, uint32_t batch);
fhe_status fhe_poly_mul(fhe_ctx* ctx, const uint64_t* a, const uint64_t* b, uint64_t* out, const uint32_t* limbIdx,
                        uint32_t nLimbs, uint32_t batch, void* ws, size_t wsBytes, void* stream);

/* DCRTPolyImpl::Plus(const std::vector<Integer>&) (dcrtpoly-impl.h:520-527): limb i plus the constant consts[i] (reduced mod
 * q_i first) — PolyImpl::Plus(Integer) (poly-impl.h:211-218) adds it to every word in EVALUATION and to coefficient 0 only in
 * COEFFICIENT (coeff0Only != 0).  This is what LeveledSHECKKSRNS::EvalAddInPlace(ciphertext, double)
 * (ckksrns-leveledshe.cpp:60-68) does to element 0.  out may alias a; constants travel by value (asynchronous). */
fhe_status fhe_add_const(fhe_ctx* ctx, uint64_t* out, const uint64_t* a, const uint64_t* consts, const uint32_t* limbIdx,
                         uint32_t nLimbs, uint32_t batch, int coeff0Only, void* stream);
/* DCRTPolyImpl::Minus(const std::vector<Integer>&) (dcrtpoly-impl.h:541-548 -> poly-impl.h:221-225: ModSub on every word, in
 * both formats); EvalSubInPlace(ciphertext, double) (ckksrns-leveledshe.cpp:112-120) */
fhe_status fhe_sub_const(fhe_ctx* ctx, uint64_t* out, const uint64_t* a, const uint64_t* consts, const uint32_t* limbIdx,
                         uint32_t nLimbs, uint32_t batch, void* stream);

/* ---- a7: element-wise tower arithmetic -----------------------------------------------------------
 * Replaces DCRTPolyImpl::operator+= / -= / *= , Plus/Minus/Times, Negate
 * (dcrtpoly-impl.h:347-408, dcrtpoly.h:131-189) and NativeVectorT::ModAddEq/ModSubEq/ModMulEq
 * (src/core/lib/math/hal/intnat/mubintvecnat.cpp:229-339). out may alias a or b. */
fhe_status fhe_add(fhe_ctx* ctx, uint64_t* out, const uint64_t* a, const uint64_t* b, const uint32_t* limbIdx,
                   uint32_t nLimbs, uint32_t batch, void* stream);
fhe_status fhe_sub(fhe_ctx* ctx, uint64_t* out, const uint64_t* a, const uint64_t* b, const uint32_t* limbIdx,
                   uint32_t nLimbs, uint32_t batch, void* stream);
fhe_status fhe_mul(fhe_ctx* ctx, uint64_t* out, const uint64_t* a, const uint64_t* b, const uint32_t* limbIdx,
                   uint32_t nLimbs, uint32_t batch, void* stream);
fhe_status fhe_neg(fhe_ctx* ctx, uint64_t* out, const uint64_t* a, const uint32_t* limbIdx, uint32_t nLimbs,
                   uint32_t batch, void* stream);
/* acc += a * b per limb: the accumulation step of KeySwitchHYBRID::EvalFastKeySwitchCoreExt
 * (src/pke/lib/keyswitch/keyswitch-hybrid.cpp:419-430) on whole towers; exact, so the order of accumulation is free */
fhe_status fhe_mul_add(fhe_ctx* ctx, uint64_t* acc, const uint64_t* a, const uint64_t* b, const uint32_t* limbIdx,
                       uint32_t nLimbs, uint32_t batch, void* stream);
/* Times(const std::vector<NativeInteger>&) / operator*=(NativeInteger) (dcrtpoly-impl.h:582-620):
 * consts[r] (HOST array, one per tower row) multiplies limb r of every tower in the batch.  The constants travel by value
 * in the kernel arguments: the call is asynchronous like every other one and can be captured into a graph; the host
 * array may be released as soon as the call returns. */
fhe_status fhe_mul_const(fhe_ctx* ctx, uint64_t* out, const uint64_t* a, const uint64_t* consts,
                         const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, void* stream);
/* out = sum_i consts[i] (.) x[i] per limb (+ out when accumulate != 0): pke's weighted sums — internalEvalLinearWSumMutable,
 * src/pke/lib/scheme/ckksrns/ckksrns-advancedshe.cpp:97-136: `EvalMultInPlace(ct_i, c_i); EvalAddInPlaceNoCheck(ct_0, ct_i)` for every
 * term, the inner loops of the Chebyshev evaluation of bootstrapping (ckksrns-fhe.cpp:691-692, :786) — as one launch per 16 terms:
 * every term is read once, the sum written once.  x: HOST array of nTerms DEVICE towers [batch][nLimbs][N] (each dense, allocated
 * on its own); consts: HOST array [nTerms][nLimbs], reduced modulo their limbs (their device table is cached by content).  Exact
 * modular arithmetic: the residues are the reference's whatever the order of the sum.  out may be one of the x[i] (with more than 16 terms the
 * terms that alias out are summed by the first launch, before out is overwritten; at most 16 terms may alias out then). */
fhe_status fhe_lincomb(fhe_ctx* ctx, uint64_t* out, const uint64_t* const* x, const uint64_t* consts, uint32_t nTerms,
                       const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, int accumulate, void* stream);
/* The two elements of a ciphertext in ONE launch: element e of every operand is a tower allocated on its own (o_e = a_e op b_e,
 * o_e = a_e * consts per limb).  pke applies its operations element by element (base-leveledshe.cpp:562-606,
 * ckksrns-leveledshe.cpp:748-759); one ciphertext's tower alone leaves most of the chip idle.  In-place use (o_e == a_e) is fine. */
fhe_status fhe_add_pair(fhe_ctx* ctx, uint64_t* o0, uint64_t* o1, const uint64_t* a0, const uint64_t* a1, const uint64_t* b0,
                        const uint64_t* b1, const uint32_t* limbIdx, uint32_t nLimbs, void* stream);
fhe_status fhe_sub_pair(fhe_ctx* ctx, uint64_t* o0, uint64_t* o1, const uint64_t* a0, const uint64_t* a1, const uint64_t* b0,
                        const uint64_t* b1, const uint32_t* limbIdx, uint32_t nLimbs, void* stream);
fhe_status fhe_mul_const_pair(fhe_ctx* ctx, uint64_t* o0, uint64_t* o1, const uint64_t* a0, const uint64_t* a1, const uint64_t* consts,
                              const uint32_t* limbIdx, uint32_t nLimbs, void* stream);
/* DCRTPolyImpl::TimesQovert (dcrtpoly-impl.h:868-885): every word x of limb r becomes ((x * NegQModt) mod t) * tInvModq[r] mod q_r —
 * ModMulFastConst modulo the plaintext modulus, then the generalized Barrett product modulo q_r (BFV encryption scales the message
 * by Q/t with it).  out may alias a; tInvModq is a HOST array (by value in the kernel arguments). */
fhe_status fhe_times_q_over_t(fhe_ctx* ctx, uint64_t* out, const uint64_t* a, uint64_t t, uint64_t negQModt,
                              const uint64_t* tInvModq, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, void* stream);
/* DCRTPolyImpl::SetValuesModSwitch (dcrtpoly-impl.h:630-647): `words` COEFFICIENT words modulo qFrom scaled to the modulus qTo,
 * out[j] = uint64(floor(0.5 + double(x[j]) * (double(qTo) / double(qFrom)))) mod qTo, in the reference's double arithmetic. */
fhe_status fhe_mod_switch_round(fhe_ctx* ctx, const uint64_t* x, uint64_t qFrom, uint64_t qTo, uint64_t* out, size_t words,
                                void* stream);
/* NativeVectorT::MultAccEqNoCheck per limb (src/core/lib/math/hal/intnat/mubintvecnat.cpp:132-142; PolyImpl wrapper
 * poly.h:323): acc[r] += v[r] * consts[r]  (constant reduced mod q first, Shoup product, ModAddFast) */
fhe_status fhe_mult_acc(fhe_ctx* ctx, uint64_t* acc, const uint64_t* v, const uint64_t* consts,
                        const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, void* stream);
/* LeveledSHEBase::EvalMultCore (src/pke/lib/schemebase/base-leveledshe.cpp:607-644):
 * d0 = a0*b0, d1 = a0*b1 + a1*b0, d2 = a1*b1 */
fhe_status fhe_tensor(fhe_ctx* ctx, const uint64_t* a0, const uint64_t* a1, const uint64_t* b0, const uint64_t* b1,
                      uint64_t* d0, uint64_t* d1, uint64_t* d2, const uint32_t* limbIdx, uint32_t nLimbs,
                      uint32_t batch, void* stream);

/* LeveledSHEBase::EvalSquareCore for 2-element ciphertexts (base-leveledshe.cpp:646-664):
 * d0 = a0*a0, d1 = a0*a1 + a0*a1, d2 = a1*a1 */
fhe_status fhe_tensor_square(fhe_ctx* ctx, const uint64_t* a0, const uint64_t* a1, uint64_t* d0, uint64_t* d1, uint64_t* d2,
                             const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, void* stream);

/* ---- a8: automorphism ----------------------------------------------------------------------------
 * Replaces DCRTPolyImpl::AutomorphismTransform(k[, precomp]) (dcrtpoly-impl.h:314-333) ->
 * PolyImpl::AutomorphismTransform (poly-impl.h:310-376; table PrecomputeAutoMap, nbtheory2.cpp:264-275).
 * k odd. evalFormat != 0: EVALUATION gather; 0: COEFFICIENT signed permutation. out must not alias in. */
fhe_status fhe_automorph(fhe_ctx* ctx, uint64_t* out, const uint64_t* in, uint32_t k, int evalFormat,
                         const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, void* stream);

/* ---- a9: centred modulus switch -------------------------------------------------------------------
 * Replaces PolyImpl::SwitchModulus / NativeVectorT::SwitchModulus (poly-impl.h:400-407,
 * mubintvecnat.cpp:109-122): limb `srcPos` (context limb srcCtxLimb) of every tower src[batch][srcLimbs][N]
 * is lifted, centred, into each of the nLimbs rows of out. */
fhe_status fhe_switch_modulus(fhe_ctx* ctx, uint64_t* out, const uint32_t* limbIdx, uint32_t nLimbs,
                              const uint64_t* src, uint32_t srcLimbs, uint32_t srcPos, uint32_t srcCtxLimb,
                              uint32_t batch, void* stream);
/* With srcLimbs = 1 this is also the "ModRaise" constructor DCRTPolyImpl(const PolyType&, params) (dcrtpoly-impl.h:87-93,
 * used by FHECKKSRNS::EvalBootstrap, ckksrns-fhe.cpp:592-601): one COEFFICIENT polynomial modulo q_0 lifted, centred, into
 * every limb of a tower. */

/* DCRTPolyImpl::CRTDecompose(baseBits) (dcrtpoly-impl.h:230-285; KeySwitchBV's digit decomposition, keyswitch-bv.cpp:254): x [nLimbs][N] in
 * COEFFICIENT format -> out [towers][nLimbs][N] in EVALUATION format, towers in the reference's order (limb 0's digits, least significant
 * first, then limb 1's ...; baseBits == 0: one tower per limb).  fhe_crt_decompose_towers returns the number of towers, 0 when the
 * selection is outside the device path (baseBits > 31, or a window that would leave the 64-bit word — where the reference itself is
 * undefined). */
uint32_t fhe_crt_decompose_towers(const fhe_ctx* ctx, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t baseBits);
fhe_status fhe_crt_decompose(fhe_ctx* ctx, const uint64_t* x, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t baseBits, uint64_t* out,
                             void* stream);

/* ---- a10/a16: CRT basis conversion ------------------------------------------------------------------
 * fhe_conv_create builds the device tables for converting from the basis {srcLimbIdx} to {dstLimbIdx}
 * (context limbs). The table VALUES are computed by the library the way CryptoParametersRNS /
 * CryptoParametersBFVRNS do (src/pke/lib/schemerns/rns-cryptoparameters.cpp:199-349):
 *   QHatInvModq[i] = [(Q/q_i)^-1]_{q_i},  QHatModp[i][j] = [Q/q_i]_{p_j},  mu_j = floor(2^128/p_j),
 *   and for the exact form alphaQModp[a][j] = [a*Q]_{p_j}, qInv[i] = 1.0/q_i.
 * fhe_approx_switch_basis replaces DCRTPolyImpl::ApproxSwitchCRTBasis (dcrtpoly-impl.h:888-932, fast path);
 * fhe_switch_basis_exact replaces DCRTPolyImpl::SwitchCRTBasis (:1008-1085; the overflow count is
 * accumulated in double in the reference's order).
 * in  = [batch][inStride][N]  COEFFICIENT format, source limb i at row inFirst+i;
 * out = [batch][outStride][N] COEFFICIENT format, target limb j at row outFirst+j. */
fhe_status fhe_conv_create(fhe_ctx* ctx, const uint32_t* srcLimbIdx, uint32_t nSrc, const uint32_t* dstLimbIdx,
                           uint32_t nDst, fhe_conv** out);
void       fhe_conv_destroy(fhe_conv* conv);
fhe_status fhe_approx_switch_basis(fhe_conv* conv, const uint64_t* in, uint32_t inStride, uint32_t inFirst,
                                   uint64_t* out, uint32_t outStride, uint32_t outFirst, uint32_t batch, void* stream);
fhe_status fhe_switch_basis_exact(fhe_conv* conv, const uint64_t* in, uint32_t inStride, uint32_t inFirst,
                                  uint64_t* out, uint32_t outStride, uint32_t outFirst, uint32_t batch, void* stream);
/* Plan with the CALLER's tables, laid out as the reference passes them to ApproxSwitchCRTBasis / SwitchCRTBasis
 * (dcrtpoly-impl.h:888-932, 1008-1085): QHatInvModq[nSrc], QHatModp[nSrc][nDst]; for the exact variant additionally
 * alphaQModp[nSrc+1][nDst] and qInv[nSrc] (doubles), else both NULL.  Needed where the tables are not the plain CRT
 * ones, e.g. FastExpandCRTBasisPloverQ's mPlQHatInvModq / qInvModp. */
fhe_status fhe_conv_create_custom(fhe_ctx* ctx, const uint32_t* srcLimbIdx, uint32_t nSrc, const uint32_t* dstLimbIdx,
                                  uint32_t nDst, const uint64_t* hatInv, const uint64_t* hatMod, const uint64_t* alphaMod,
                                  const double* qInv, fhe_conv** out);
/* DCRTPolyImpl::ExpandCRTBasis / ExpandCRTBasisReverseOrder (dcrtpoly-impl.h:1088-1148): x [batch][nSrc][N] over the plan's
 * source basis Q in format inEval -> out [batch][nSrc+nDst][N] over Q u P in resultEval (reverseOrder: P rows first).
 * ws (fhe_expand_crt_basis_workspace_bytes) is only needed for EVALUATION input. */
size_t     fhe_expand_crt_basis_workspace_bytes(const fhe_conv* plan, uint32_t batch);
fhe_status fhe_expand_crt_basis(fhe_conv* plan, const uint64_t* x, int inEval, uint64_t* out, int resultEval,
                                int reverseOrder, uint32_t batch, void* ws, size_t wsBytes, void* stream);
/* DCRTPolyImpl::ApproxModUp (dcrtpoly-impl.h:935-963): x [batch][nSrc][N] over the plan's source basis Q in format inEval ->
 * out [batch][nSrc+nDst][N] over Q u P in EVALUATION (the P part is ApproxSwitchCRTBasis of the coefficient form; the
 * EVALUATION copy of the Q limbs is reused when the input has one).  ws as for fhe_expand_crt_basis. */
fhe_status fhe_mod_up(fhe_conv* plan, const uint64_t* x, int inEval, uint64_t* out, uint32_t batch, void* ws, size_t wsBytes,
                      void* stream);
/* DCRTPolyImpl::ExpandCRTBasisQlHat (dcrtpoly-impl.h:1167-1187): limbs [0, sizeQl) of x [batch][sizeQl][N] times
 * QlHatModq[i] (HOST constants), limbs [sizeQl, sizeQ) zero -> out [batch][sizeQ][N] over context limbs limbIdx[0..sizeQ)
 * (NULL = identity); the format is unchanged. */
fhe_status fhe_expand_crt_basis_ql_hat(fhe_ctx* ctx, const uint64_t* x, uint32_t sizeQl, const uint64_t* QlHatModq,
                                       const uint32_t* limbIdx, uint32_t sizeQ, uint32_t batch, uint64_t* out, void* stream);
/* DCRTPolyImpl::FastExpandCRTBasisPloverQ (dcrtpoly-impl.h:1151-1164), COEFFICIENT format: toPl = custom-table plan
 * Q -> Pl (mPlQHatInvModq, qInvModp), toQl = plan Pl -> Ql; x [batch][nQ][N] -> out [batch][nQl+nPl][N] = [Ql | Pl]. */
fhe_status fhe_fast_expand_crt_basis_p_over_q(fhe_conv* toPl, fhe_conv* toQl, const uint64_t* x, uint64_t* out,
                                              uint32_t batch, void* stream);

/* ---- a11..a14: HYBRID key switching -----------------------------------------------------------------
 * The context must hold the Q limbs [0,sizeQ) followed by the P limbs [sizeQ, sizeQ+sizeP).
 * fhe_ks_plan_create replaces the HYBRID part of CryptoParametersRNS::PrecomputeCRTTables
 * (rns-cryptoparameters.cpp:80-350): digit partition (alpha = ceil(sizeQ/numPartQ)), complementary bases,
 * PartQlHatInvModq / PartQlHatModp per level, PInvModq, PHatInvModp, PHatModq, Barrett constants.
 * fhe_ks_key_upload copies an evaluation key (b and a vectors of EvalKeyRelin,
 * src/pke/include/key/evalkeyrelin.h:141,171), each given as HOST uint64_t[numPartQ][sizeQ+sizeP][N] in
 * EVALUATION format, to the device. With RCCL the caller broadcasts the device copy instead
 * (fhe_ks_key_alloc + fhe_ks_key_devptr). */
fhe_status fhe_ks_plan_create(fhe_ctx* ctx, uint32_t sizeQ, uint32_t sizeP, uint32_t numPartQ, fhe_ks_plan** out);
void       fhe_ks_plan_destroy(fhe_ks_plan* plan);
uint32_t   fhe_ks_plan_alpha(const fhe_ks_plan* plan);
/* how many levels sizeQl the plan has built its tables for so far (a level is built on first use, or all at once by fhe_bfv_hybrid_create) */
uint32_t   fhe_ks_plan_levels_built(fhe_ks_plan* plan);
fhe_status fhe_ks_key_alloc(fhe_ks_plan* plan, fhe_ks_key** out);
fhe_status fhe_ks_key_upload(fhe_ks_plan* plan, const uint64_t* keyB, const uint64_t* keyA, fhe_ks_key** out);
/* adopt key vectors that already live in device memory (not owned: destroy leaves them alone). This is the
 * multi-GPU path: rank 0 uploads, every rank receives the words with an RCCL broadcast into its own buffer
 * (e.g. a torch tensor) and wraps it — the only collective of the whole design. */
fhe_status fhe_ks_key_wrap(fhe_ks_plan* plan, uint64_t* devKeyB, uint64_t* devKeyA, fhe_ks_key** out);
void       fhe_ks_key_destroy(fhe_ks_key* key);
/* device pointers of the b (which=0) / a (which=1) vectors: uint64_t[numPartQ][sizeQ+sizeP][N] */
uint64_t*  fhe_ks_key_devptr(fhe_ks_key* key, int which);
size_t     fhe_ks_key_words(const fhe_ks_key* key);

/* ---- evaluation-key generation on the device ---------------------------------------------------------
 * fhe_keygen_combine: everything of key generation that is not sampling or transforming, for nKeys keys of nParts digits in ONE launch
 * (csrc/keygen_kernels.h).  For key < nKeys, digit j < nParts, tower row i < nLimbs (context limb limbIdx[i], NULL = identity), word n:
 *   out[key][j][i][n] = ns * e[key][j][i][n] - a[key][j][i][n] * sNew[i][pi_kNew[key](n)] + factor[j][i] * sOld[i][pi_kOld[key](n)]  mod q_i
 * which is the loop body of KeySwitchHYBRID::KeySwitchGenInternal (src/pke/lib/keyswitch/keyswitch-hybrid.cpp:98-123:
 * b_i = -a_i * sNewExt_i + ns * e_i [+ PModq_i * sOld_i]) with the permuted secret of LeveledSHEBase::EvalAutomorphismKeyGen
 * (src/pke/lib/schemebase/base-leveledshe.cpp:336-379) read through the index map instead of being materialised, and with factor == NULL
 * (no sOld term: sOld and kOld are ignored) b = ns * e - a * s of PKEBase::KeyGenInternal (src/pke/lib/schemebase/base-pke.cpp:47-98).
 *   a, e, out  DEVICE [nKeys][nParts][nLimbs][N]; sNew, sOld DEVICE [nLimbs][N]; all EVALUATION format, canonical residues in and out;
 *   pi_k       the index map of fhe_automorph(evalFormat = 1) for the odd index k in [1, 2N); kNew, kOld: HOST arrays [nKeys], NULL = all 1
 *              (k = 1 reads the row in place, without a gather);
 *   factor     HOST array [nParts][nLimbs], reduced modulo q_i inside.  A zero entry means "term absent": sOld is read only in rows where
 *              some digit has a non-zero factor, so it needs rows only up to the last such limb (HYBRID keys: sizeQ rows).  The
 *              secret-key forms of a BV key are this formula with the table of fhe_bv_keygen_factors (fhe_bv_keygen below); the
 *              public-key form of a BV key is NOT: it has a kernel of its own (fhe_bv_keygen_pk);
 *   ns         GetNoiseScale(): 1 for CKKS and BFV, t for BGV; reduced modulo every limb (ns >= q_i is legal), 0 is refused.
 * out may be e itself (every word of e is read before the same word of out is written); it must not overlap e otherwise, nor a, sNew or
 * sOld.  Errors (FHE_ERR_ARG, nothing is enqueued, out untouched): a null operand, nKeys == 0, nParts == 0, an even automorphism index
 * ("Automorphism index not odd") or one >= 2N, ns == 0, a forbidden overlap.  The factors and ns go through a table cached by content:
 * the first call with new ones uploads it (not capturable), later calls are pure launches.  One launch per 256 keys: the keys' indices
 * travel by value in the kernel arguments (4 KiB); no grid limit is reached before that. */
fhe_status fhe_keygen_combine(fhe_ctx* ctx, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t nKeys, uint32_t nParts, const uint64_t* a,
                              const uint64_t* e, const uint64_t* sNew, const uint32_t* kNew, const uint64_t* sOld, const uint32_t* kOld,
                              const uint64_t* factor, uint64_t ns, uint64_t* out, void* stream);
/* The sNewExt block of KeySwitchHYBRID::KeySwitchGenInternal (keyswitch-hybrid.cpp:59-83): sQ [sizeQ][N] EVALUATION -> outExt
 * [sizeQ+sizeP][N] EVALUATION.  The Q rows are copied; the P rows are limb 0 in COEFFICIENT format (inverse transform), centre-switched to
 * every p_j (PolyImpl::SwitchModulus, the kernel of fhe_switch_modulus) and transformed.  ws: N words (8 N bytes) of device workspace.
 * outExt may start at sQ (the Q rows then stay where they are) and must not overlap it otherwise. */
fhe_status fhe_ks_secret_extend(fhe_ks_plan* plan, const uint64_t* sQ, uint64_t* outExt, void* ws, size_t wsBytes, void* stream);
/* KeySwitchHYBRID::KeySwitchGenInternal(oldKey, newKey) (keyswitch-hybrid.cpp:51-130) for nKeys keys with the caller's randomness: ONE
 * launch of fhe_keygen_combine over the plan's Q u P limbs with factor[j][i] = [P]_{q_i} for the limbs i of digit j (alpha * j <= i <
 * min(alpha * (j + 1), sizeQ)) and 0 elsewhere.  sNewExt [sizeQ+sizeP][N] (fhe_ks_secret_extend), sOld [sizeQ][N]; a, e, devKeyB
 * [nKeys][numPartQ][sizeQ+sizeP][N], devKeyB == e allowed.  Window `key` of devKeyB / a is what fhe_ks_key_wrap adopts.
 * EvalAutomorphismKeyGen (base-leveledshe.cpp:336-379) for the automorphism index k: kNew = k^-1 mod 2N, kOld = 1 (the NEW secret is the
 * permuted one); EvalMultKeyGen: kNew = kOld = 1 with sOld = s * s. */
fhe_status fhe_ks_keygen_hybrid(fhe_ks_plan* plan, uint32_t nKeys, const uint32_t* kNew, const uint32_t* kOld, const uint64_t* sNewExt,
                                const uint64_t* sOld, uint64_t ns, const uint64_t* a, const uint64_t* e, uint64_t* devKeyB, void* stream);
/* The seeded form, defined as a composition (batch = nKeys * numPartQ towers over Q u P):
 *   devKeyA = the words of fhe_sample_uniform_blake2(batch, key, counterA), used as drawn: the reference draws a in EVALUATION format;
 *   devKeyB = fhe_sample_gaussian_blake2(batch, sigma, key, counterE), then fhe_ntt_fwd in place, then fhe_ks_keygen_hybrid in place.
 * No workspace: the error tower never exists outside the buffer that ends up holding b.  Launches: the two samplers, the passes of one
 * forward transform over the whole batch and one combine (per 256 keys), whatever nKeys is: five on a two-pass ring (N >= 8192), six when
 * the batched row pass of N = 2^16 / 2^17 takes towers in pairs and an odd batch leaves it a last one.  The a half of every key is a function of
 * (key, counterA) alone: another device can regenerate it with fhe_sample_uniform_blake2 instead of receiving it.  The blake2 key travels
 * by value.  The first Gaussian call with a new sigma uploads its inversion table (not capturable), as in fhe_sample_gaussian.  Every
 * argument is checked before the first launch: the errors of fhe_keygen_combine, and sigma outside 1 < sigma < 300. */
fhe_status fhe_ks_keygen_hybrid_blake2(fhe_ks_plan* plan, uint32_t nKeys, const uint32_t* kNew, const uint32_t* kOld,
                                       const uint64_t* sNewExt, const uint64_t* sOld, uint64_t ns, double sigma, const uint32_t key[16],
                                       uint64_t counterA, uint64_t counterE, uint64_t* devKeyB, uint64_t* devKeyA, void* stream);
/* blake2 counters fhe_ks_keygen_hybrid_blake2 consumes from counterA (*nA) and from counterE (*nE): lay out disjoint ranges with them */
fhe_status fhe_ks_keygen_counters(const fhe_ks_plan* plan, uint32_t nKeys, uint64_t* nA, uint64_t* nE);

/* ---- encryption on the device -------------------------------------------------------------------------
 * fhe_encrypt_pk_combine / fhe_encrypt_sk_combine: everything of encryption that is not sampling or transforming, both elements of
 * `batch` ciphertexts in ONE launch (csrc/encrypt_kernels.h).  For ciphertext t < batch, tower row i < nLimbs (context limb limbIdx[i],
 * NULL = identity), word n, modulo q_i:
 *   public key   c0[t][i][n] = pkB[i][n] * v[t][i][n] + ns * e0[t][i][n] (+ msg[t][i][n])
 *                c1[t][i][n] = pkA[i][n] * v[t][i][n] + ns * e1[t][i][n]
 *                PKERNS::EncryptZeroCore(publicKey) (src/pke/lib/schemerns/rns-pke.cpp:148-197) and `(*ba)[0] += plaintext` of
 *                PKERNS::Encrypt (:56-70);
 *   secret key   c0[t][i][n] = a[t][i][n] * s[i][n] + ns * e[t][i][n] (+ msg[t][i][n])
 *                c1[t][i][n] = -a[t][i][n]
 *                PKERNS::EncryptZeroCore(privateKey) (:111-146) and PKERNS::Encrypt (:40-54).
 *   v, e0, e1, a, e, msg, c0, c1  DEVICE [batch][nLimbs][N]; pkB, pkA, s DEVICE [nLimbs][N] with row stride N: the first nLimbs rows of a
 *              full-level key serve a plaintext with fewer limbs (DropLastElements on the clones, :129-135, :175-182); all EVALUATION
 *              format, canonical residues in and out; msg may be NULL (EncryptZeroCore alone);
 *   ns         GetNoiseScale(): 1 for CKKS and BFV, t for BGV; reduced modulo every limb (ns >= q_i is legal), 0 is refused.
 * In place: c0 may be e0 (or e) itself and c1 may be e1 (or a) itself: every word is read by the lane that overwrites it.  Errors
 * (FHE_ERR_ARG, nothing is enqueued, outputs untouched): a null operand, batch == 0, nLimbs == 0, a limb outside the context, ns == 0, a
 * forbidden overlap (the key rows, msg or v against an output; v against e0 / e1; an output against an input other than its own; c0
 * against c1).  ns goes through a table cached by content: the first call with a new ns != 1 uploads it (not capturable), later calls are
 * pure launches.  A workgroup walks fhe_encrypt_chunk(ctx, nLimbs, batch) ciphertexts (1, 2, 4 or 8: as many as still leave four
 * workgroups per compute unit) with its words of the key rows in registers; batch need not be a multiple of it. */
fhe_status fhe_encrypt_pk_combine(fhe_ctx* ctx, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, const uint64_t* pkB,
                                  const uint64_t* pkA, const uint64_t* v, const uint64_t* e0, const uint64_t* e1, const uint64_t* msg,
                                  uint64_t ns, uint64_t* c0, uint64_t* c1, void* stream);
fhe_status fhe_encrypt_sk_combine(fhe_ctx* ctx, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, const uint64_t* s,
                                  const uint64_t* a, const uint64_t* e, const uint64_t* msg, uint64_t ns, uint64_t* c0, uint64_t* c1,
                                  void* stream);
uint32_t   fhe_encrypt_chunk(const fhe_ctx* ctx, uint32_t nLimbs, uint32_t batch);
/* The seeded public-key form, defined as a composition.  ct DEVICE [2][batch][nLimbs][N]: the c0 block, then the c1 block; ws holds v,
 * fhe_encrypt_workspace_bytes(ctx, nLimbs, batch) bytes:
 *   v       = fhe_sample_ternary_blake2 (vDist = 0) or fhe_sample_gaussian_blake2 (vDist = 1: the reference's choice under
 *             SecretKeyDist == GAUSSIAN, rns-pke.cpp:164-165) over batch towers from counterV, into ws;
 *   e0 ‖ e1 = ONE fhe_sample_gaussian_blake2 over 2 * batch towers from counterE, into ct;
 *   msg     with msgFormat 1 (COEFFICIENT) is added to the e0 block here with the kernel of fhe_add: one more launch, the path of
 *             PKEBFVRNS::Encrypt with the STANDARD technique (src/pke/lib/scheme/bfvrns/bfvrns-pke.cpp:157-213: TimesQovert on the
 *             COEFFICIENT plaintext, which is fhe_times_q_over_t, then `(*ba)[0] += ptxt`).  Legal only when ns = 1 modulo every limb
 *             in use, since e0 is scaled by ns afterwards;
 *   fhe_ntt_fwd, ONE call over 3 * batch towers when ws == ct + 2 * batch * nLimbs * N words, else one over ct and one over ws;
 *   fhe_encrypt_pk_combine in place in ct, with msg when msgFormat is 0 (EVALUATION).
 * With the contiguous workspace that is five launches on a two-pass ring (N >= 8192) whatever the batch is, six when the batched row pass
 * of N = 2^16 / 2^17 takes towers in pairs and 3 * batch is odd.  e0, e1 and v never exist outside ct / ws.  The blake2 key travels by
 * value; the first Gaussian call with a new sigma uploads its inversion table (not capturable).  Every argument is checked before the
 * first launch: the errors of fhe_encrypt_pk_combine, sigma outside 1 < sigma < 300, an unknown vDist or msgFormat, a COEFFICIENT message
 * with ns != 1 modulo some limb, a short workspace, ws overlapping ct, the public key or msg. */
size_t     fhe_encrypt_workspace_bytes(const fhe_ctx* ctx, uint32_t nLimbs, uint32_t batch);
fhe_status fhe_encrypt_pk_blake2(fhe_ctx* ctx, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, const uint64_t* pkB,
                                 const uint64_t* pkA, int vDist, uint64_t ns, double sigma, const uint32_t key[16], uint64_t counterV,
                                 uint64_t counterE, const uint64_t* msg, int msgFormat, uint64_t* ct, void* ws, size_t wsBytes,
                                 void* stream);
/* The seeded secret-key form: a = the words of fhe_sample_uniform_blake2(batch, key, counterA) in the c1 block, used as drawn (the
 * reference draws a in EVALUATION format, rns-pke.cpp:122); e = fhe_sample_gaussian_blake2(batch, sigma, key, counterE) in the c0 block
 * (+ a COEFFICIENT msg, as above), then fhe_ntt_fwd there, then fhe_encrypt_sk_combine in place.  No workspace.  The c1 half is a function
 * of (key, counterA) alone, as the a half of the evaluation keys is.  PKEBFVRNS::Encrypt(privateKey) is bfvrns-pke.cpp:99-155. */
fhe_status fhe_encrypt_sk_blake2(fhe_ctx* ctx, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, const uint64_t* s, uint64_t ns,
                                 double sigma, const uint32_t key[16], uint64_t counterA, uint64_t counterE, const uint64_t* msg,
                                 int msgFormat, uint64_t* ct, void* stream);
/* blake2 counters a seeded call consumes: form 0 (public key): *nVorA from counterV, *nE from counterE (e0 ‖ e1 together); form 1 (secret
 * key): *nVorA from counterA, *nE from counterE.  The arithmetic of fhe_ks_keygen_counters. */
fhe_status fhe_encrypt_counters(const fhe_ctx* ctx, uint32_t nLimbs, uint32_t batch, int form, uint64_t* nVorA, uint64_t* nE);

/* ---- decryption on the device -------------------------------------------------------------------------
 * fhe_decrypt_core: PKERNS::DecryptCore (src/pke/lib/schemerns/rns-pke.cpp:199-225) for `batch` ciphertexts in ONE launch
 * (csrc/decrypt_kernels.h).  For ciphertext t < batch, tower row i < nLimbs (context limb limbIdx[i], NULL = identity), word n, modulo q_i:
 *   b[t][i][n] = [c[0][t][i][n]] + s[i][n] * c[1][t][i][n] + s[i][n]^2 * c[2][t][i][n] + s[i][n]^3 * c[3][t][i][n] [+ ns * noise[t][i][n]]
 * evaluated by Horner: the words of the reference's loop `b += sPower * cv[i]; sPower *= s`, without a tower of s^2.
 *   c        HOST array of nElem (2, 3 or 4) DEVICE pointers, element e of all ciphertexts [batch][nLimbs][N];
 *   s        DEVICE, ONE tower [nLimbs][N] with row stride N: the first nLimbs rows of a full-level key serve a lower-level ciphertext
 *            (DropLastElements on the copy of the key, :203-206);
 *   noise    DEVICE [batch][nLimbs][N] or NULL.  With ns = 1 it is CKKS's `b += noise` under NOISE_FLOODING_DECRYPT
 *            (src/pke/lib/scheme/ckksrns/ckksrns-pke.cpp:49-54, 75-80); with nElem = 2 it is the flooding term of
 *            MultipartyDecryptLead (withC0 = 1: `cv[0] + s * cv[1] + ns * e`) and MultipartyDecryptMain (withC0 = 0: `s * cv[1] + ns * e`;
 *            c[0] is not read and may be NULL) (src/pke/lib/schemerns/rns-multiparty.cpp:46-171);
 *   ns       reduced modulo every limb through a table cached by content, as in fhe_encrypt_*_combine: the first call with a new
 *            ns != 1 uploads it (not capturable), later calls are pure launches; ns == 0 with a noise tower is refused;
 *   outFormat 0 (EVALUATION): exactly one launch.  1 (COEFFICIENT): that launch, then fhe_ntt_inv on out.  With nLimbs > 1 the
 *            COEFFICIENT tower is what PKECKKSRNS::Decrypt(.., Poly*) hands to CRTInterpolate (ckksrns-pke.cpp:70-96); with one limb
 *            it is the NativePoly of :44-68.  Interpolation and decoding stay on the host.
 * All towers EVALUATION on entry, canonical residues in and out.  In place: out may be c[0] itself or the noise tower itself (every word
 * is read by the lane that overwrites it); any other overlap is refused.  Errors (FHE_ERR_ARG, nothing is enqueued, out untouched): a
 * null operand, nElem outside [2, 4], withC0 == 0 with nElem != 2, batch == 0, nLimbs == 0, a limb outside the context, ns == 0 with
 * noise, an unknown outFormat, a forbidden overlap.  A workgroup walks fhe_decrypt_chunk(ctx, nLimbs, batch) ciphertexts (1, 2, 4 or 8, the
 * choice of fhe_encrypt_chunk) with its words of s in registers; batch need not be a multiple of it. */
fhe_status fhe_decrypt_core(fhe_ctx* ctx, const uint64_t* const* c, uint32_t nElem, const uint64_t* s, const uint32_t* limbIdx,
                            uint32_t nLimbs, uint32_t batch, const uint64_t* noise, uint64_t ns, int withC0, int outFormat,
                            uint64_t* out, void* stream);
uint32_t   fhe_decrypt_chunk(const fhe_ctx* ctx, uint32_t nLimbs, uint32_t batch);
/* PKEBFVRNS::Decrypt at sizeQl == sizeQ (src/pke/lib/scheme/bfvrns/bfvrns-pke.cpp:215-245) as a plan over the context limbs
 * limbIdx[sizeQ] (NULL = the leading limbs), the plaintext modulus t and a technique: 0 BEHZ, 1 HPS, 2 HPSPOVERQ, 3 HPSPOVERQLEVELED (the
 * three HPS techniques decrypt alike).  Every table is derived on the host from the moduli and t and kept on the device:
 *   HPS   tQHatInvModqDivqModt, tQHatInvModqDivqFrac and, when qMSB + sizeQMSB >= 52, tQHatInvModqBDivqModt, tQHatInvModqBDivqFrac
 *         (src/pke/lib/scheme/bfvrns/bfvrns-cryptoparameters.cpp:434-484; the Frac tables as double(numerator) / double(denominator), as there);
 *   BEHZ  tgamma, tgammaQHatInvModq, negInvqModtgamma with gamma = 2^26 (:851-882); t >= 2^32 is FHE_ERR_UNSUPPORTED.
 * fhe_bfv_decrypt_table reads one back: ids 0 tQHatInvModqDivqModt, 1 tQHatInvModqBDivqModt, 2 tQHatInvModqDivqFrac, 3
 * tQHatInvModqBDivqFrac (doubles as their 64 bits), 4 tgamma (one word), 5 tgammaQHatInvModq, 6 negInvqModtgamma; returns the number of
 * words (0: the plan has no such table) and copies min(that, cap) of them.
 * fhe_bfv_decrypt: c[nElem] and s as for fhe_decrypt_core over the plan's limbs -> out DEVICE [batch][N], the NativePoly words modulo t.
 * The combine into ws, ONE inverse transform of all limbs of all towers, then the kernel of fhe_scale_and_round_native or
 * fhe_scale_and_round_behz_decrypt with the plan's tables: four launches on a two-pass ring (N >= 8192) for any batch and any nElem.
 * ws: fhe_bfv_decrypt_workspace_bytes(plan, batch) = batch * sizeQ * N words.
 * fhe_bfv_decrypt_b: the tail alone on a b [batch][sizeQ][N] the caller holds, what MultipartyBFVRNS::MultipartyDecryptFusion runs after
 * its sum (src/pke/lib/scheme/bfvrns/bfvrns-multiparty.cpp:139-175).  evalFormat != 0: b is EVALUATION and is transformed out of place
 * into ws; b is only read.  evalFormat == 0: b is COEFFICIENT, ws is not used and may be NULL.
 * After creation the calls allocate nothing and do not wait for the device.  Errors, each before anything is enqueued (FHE_ERR_ARG, outputs
 * untouched): those of fhe_decrypt_core; equal moduli in the plan; t < 2; an unknown technique; a short workspace; out overlapping an
 * input or ws; ws overlapping an input.  The compressed-ciphertext branch of the member (sizeQl != sizeQ, :246-268) has no entry here: a
 * plan decrypts at its own sizeQ only. */
typedef struct fhe_bfv_dec fhe_bfv_dec;
fhe_status fhe_bfv_decrypt_create(fhe_ctx* ctx, const uint32_t* limbIdx, uint32_t sizeQ, uint64_t t, int technique, fhe_bfv_dec** out);
void       fhe_bfv_decrypt_destroy(fhe_bfv_dec* plan);
size_t     fhe_bfv_decrypt_workspace_bytes(const fhe_bfv_dec* plan, uint32_t batch);
size_t     fhe_bfv_decrypt_table(const fhe_bfv_dec* plan, int tableId, uint64_t* out, size_t cap);
fhe_status fhe_bfv_decrypt(fhe_bfv_dec* plan, const uint64_t* const* c, uint32_t nElem, const uint64_t* s, uint32_t batch, uint64_t* out,
                           void* ws, size_t wsBytes, void* stream);
fhe_status fhe_bfv_decrypt_b(fhe_bfv_dec* plan, const uint64_t* b, int evalFormat, uint32_t batch, uint64_t* out, void* ws,
                             size_t wsBytes, void* stream);

/* workspace (device bytes) needed by the composite calls below for `batch` towers at level sizeQl */
size_t     fhe_ks_workspace_bytes(const fhe_ks_plan* plan, uint32_t sizeQl, uint32_t batch);

/* KeySwitchHYBRID::EvalKeySwitchPrecomputeCore + EvalFastKeySwitchCore
 * (src/pke/lib/keyswitch/keyswitch-hybrid.cpp:314-400), i.e. KeySwitchCore (:308-312):
 * c[batch][sizeQl][N] EVALUATION -> out0,out1[batch][sizeQl][N] EVALUATION. `ws` = device workspace. */
fhe_status fhe_keyswitch_hybrid(fhe_ks_plan* plan, const fhe_ks_key* key, const uint64_t* c, uint32_t sizeQl,
                                uint32_t batch, uint64_t* out0, uint64_t* out1, void* ws, size_t wsBytes,
                                void* stream);
/* acc0 += ks0(c), acc1 += ks1(c): the tail of LeveledSHEBase::EvalMult(ct, ct, key) (base-leveledshe.cpp:207-211), the two
 * additions fused into the last kernel of the key switch.  Same layout and workspace as fhe_keyswitch_hybrid. */
fhe_status fhe_keyswitch_hybrid_acc(fhe_ks_plan* plan, const fhe_ks_key* key, const uint64_t* c, uint32_t sizeQl,
                                    uint32_t batch, uint64_t* acc0, uint64_t* acc1, void* ws, size_t wsBytes, void* stream);
/* cc->EvalMult(ct1, ct2) for 2-element ciphertexts: EvalMultCore + KeySwitchCore + add
 * (src/pke/lib/schemebase/base-leveledshe.cpp:201-214, 607-644).  All towers [batch][sizeQl][N] EVALUATION.
 * c0/c1 may alias a0/a1. */
fhe_status fhe_ckks_eval_mult(fhe_ks_plan* plan, const fhe_ks_key* key, const uint64_t* a0, const uint64_t* a1,
                              const uint64_t* b0, const uint64_t* b1, uint32_t sizeQl, uint32_t batch, uint64_t* c0,
                              uint64_t* c1, void* ws, size_t wsBytes, void* stream);
/* Hoisting (Halevi-Shoup): LeveledSHEBase::EvalFastRotationPrecompute = EvalKeySwitchPrecomputeCore(c1)
 * (src/pke/lib/schemebase/base-leveledshe.cpp:425-430) once, then per rotation key EvalFastKeySwitchCore + add +
 * automorphism (:432-463).  The digits stay in the workspace `ws` between the calls (same sizeQl / batch / ws).
 * fhe_eval_automorphism = EvalAutomorphism (:381-422): out0 = Auto_k(c0 + ks0(c1)), out1 = Auto_k(ks1(c1)).
 * `key` must be the evaluation key of automorphism index k (FindAutomorphismIndex2nComplex for CKKS rotations). */
fhe_status fhe_ks_precompute(fhe_ks_plan* plan, const uint64_t* c1, uint32_t sizeQl, uint32_t batch, void* ws,
                             size_t wsBytes, void* stream);
fhe_status fhe_ks_fast_keyswitch(fhe_ks_plan* plan, const fhe_ks_key* key, const uint64_t* c1, uint32_t sizeQl,
                                 uint32_t batch, uint64_t* out0, uint64_t* out1, void* ws, size_t wsBytes, void* stream);
fhe_status fhe_eval_fast_rotation(fhe_ks_plan* plan, const fhe_ks_key* key, const uint64_t* c0, const uint64_t* c1,
                                  uint32_t k, uint32_t sizeQl, uint32_t batch, uint64_t* out0, uint64_t* out1, void* ws,
                                  size_t wsBytes, void* stream);
fhe_status fhe_eval_automorphism(fhe_ks_plan* plan, const fhe_ks_key* key, const uint64_t* c0, const uint64_t* c1,
                                 uint32_t k, uint32_t sizeQl, uint32_t batch, uint64_t* out0, uint64_t* out1, void* ws,
                                 size_t wsBytes, void* stream);
/* The inner product of HYBRID key switching (KeySwitchHYBRID::EvalFastKeySwitchCoreExt, keyswitch-hybrid.cpp:419-430) over
 * towers that live in separate allocations — what a DCRTPoly backend holds: every digit and every element of the evaluation
 * key is its own tower.  out_e[b][i] = sum_{t < nTerms} x[t][b][i] * k_e[t][keyRow[i]] mod q_{limbIdx[i]}, e = 0 (k0 -> out0)
 * and, when k1/out1 are given, e = 1.  x[t] is [batch][rows][N], k_e[t] is a tower of at least max(keyRow)+1 rows, keyRow NULL
 * = identity (the reference's idx(i) = i < sizeQl ? i : i + sizeQ - sizeQl, :425).  x, k0, k1 are HOST arrays of device
 * pointers; all operands are canonical residues; nTerms >= 1: one launch per 8 terms, each launch after the first adds its (exact) sums
 * to what the earlier ones left in out0 / out1. */
fhe_status fhe_inner_product(fhe_ctx* ctx, uint32_t nTerms, const uint64_t* const* x, const uint64_t* const* k0,
                             const uint64_t* const* k1, const uint32_t* keyRow, const uint32_t* limbIdx, uint32_t rows,
                             uint32_t batch, uint64_t* out0, uint64_t* out1, void* stream);

/* Double hoisting (ckksrns-fhe.cpp:1830-2000) works in the extended basis Q_l u P and mods down once:
 *   fhe_ks_ext                 = KeySwitchHYBRID::KeySwitchExt for one element (keyswitch-hybrid.cpp:217-243):
 *                                out [batch][sizeQl+sizeP][N], Q_l rows = c * [P]_{q_i}, P rows = 0;
 *   fhe_ks_fast_keyswitch_ext  = EvalFastKeySwitchCoreExt (:402-435) on the digits fhe_ks_precompute left in ws;
 *   fhe_eval_fast_rotation_ext = LeveledSHECKKSRNS::EvalFastRotationExt (ckksrns-leveledshe.cpp:534-582);
 *   fhe_ks_down                = KeySwitchHYBRID::KeySwitchDown (:245-278), ApproxModDown of both elements.
 * Extended towers are [batch][sizeQl+sizeP][N] over context limbs {0..sizeQl-1, sizeQ..sizeQ+sizeP-1}; the generic
 * element-wise entry points (fhe_add / fhe_mul / fhe_automorph with that limb list) cover EvalAddExt / EvalMultExt. */
fhe_status fhe_ks_ext(fhe_ks_plan* plan, const uint64_t* c, uint32_t sizeQl, uint32_t batch, uint64_t* outExt, void* stream);
fhe_status fhe_ks_fast_keyswitch_ext(fhe_ks_plan* plan, const fhe_ks_key* key, const uint64_t* c1, uint32_t sizeQl,
                                     uint32_t batch, uint64_t* out0Ext, uint64_t* out1Ext, void* ws, size_t wsBytes,
                                     void* stream);
fhe_status fhe_eval_fast_rotation_ext(fhe_ks_plan* plan, const fhe_ks_key* key, const uint64_t* c0, const uint64_t* c1,
                                      uint32_t k, int addFirst, uint32_t sizeQl, uint32_t batch, uint64_t* out0Ext,
                                      uint64_t* out1Ext, void* ws, size_t wsBytes, void* stream);
fhe_status fhe_ks_down(fhe_ks_plan* plan, const uint64_t* x0Ext, const uint64_t* x1Ext, uint32_t sizeQl, uint32_t batch,
                       uint64_t* out0, uint64_t* out1, void* ws, size_t wsBytes, void* stream);
/* Baby-step/giant-step plaintext-matrix x ciphertext product with double hoisting: FHECKKSRNS::EvalLinearTransform
 * (src/pke/lib/scheme/ckksrns/ckksrns-fhe.cpp:1832-1882) and one level of EvalCoeffsToSlots / EvalSlotsToCoeffs
 * (:1884-2198), the linear-transform loops of CKKS bootstrapping.
 *   rot_j   = inK[j] ? EvalFastRotationExt(ct, inK[j], digits(ct), true) : KeySwitchExt(ct, true)        j < nIn
 *   inner_i = sum_j rot_j * diag[i*nIn + j]            (EvalMultExt / EvalAddExtInPlace; NULL = term absent)
 *   outK[i] == 0: first += KeySwitchDownFirstElement(inner_i); outer[1] += inner_i[1]
 *   else        : d = KeySwitchDown(inner_i); first += Automorphism(d[0]); outer += EvalFastRotationExt(d, outK[i], digits(d), false)
 *   (out0, out1) = KeySwitchDown(outer), out0 += first
 * inK / outK are automorphism indices (FindAutomorphismIndex2nComplex of the rotation), 0 = no rotation; inKeys[j] /
 * outKeys[i] the matching evaluation keys (ignored where the index is 0).  diag: HOST array of nOut*nIn DEVICE pointers to
 * plaintext rows [sizeQl+sizeP][N] in EVALUATION format over limbs {0..sizeQl-1, sizeQ..sizeQ+sizeP-1}
 * (EvalLinearTransformPrecompute's aux plaintexts), shared by the whole batch.  c0,c1,out0,out1: [batch][sizeQl][N].
 * Every stage runs once over all outer steps (their accumulations are exact modular sums, so the order is free); the
 * first call with a new set of diagonals uploads their pointer table (not capturable), later calls are pure launches. */
size_t fhe_ckks_bsgs_workspace_bytes(const fhe_ks_plan* plan, uint32_t sizeQl, uint32_t batch, uint32_t nIn, uint32_t nOut);
fhe_status fhe_ckks_bsgs_transform(fhe_ks_plan* plan, const uint64_t* c0, const uint64_t* c1, uint32_t sizeQl, uint32_t batch,
                                   uint32_t nIn, const uint32_t* inK, const fhe_ks_key* const* inKeys, uint32_t nOut,
                                   const uint32_t* outK, const fhe_ks_key* const* outKeys, const uint64_t* const* diag,
                                   uint64_t* out0, uint64_t* out1, void* ws, size_t wsBytes, void* stream);
/* DCRTPolyImpl::ApproxModDown with t = 0 (dcrtpoly-impl.h:966-1005):
 * x[batch][sizeQl+sizeP][N] EVALUATION -> out[batch][sizeQl][N] EVALUATION */
fhe_status fhe_approx_mod_down(fhe_ks_plan* plan, const uint64_t* x, uint32_t sizeQl, uint32_t batch, uint64_t* out,
                               void* ws, size_t wsBytes, void* stream);
/* ApproxModDown with the BGV factors t^-1 (mod p_j) before and t (mod q_i) after the conversion (dcrtpoly-impl.h:966-1005
 * with t > 0; tables tInvModp / tModqPrecon of CryptoParametersBGVRNS are derived inside).  Same layout and workspace. */
fhe_status fhe_approx_mod_down_bgv(fhe_ks_plan* plan, const uint64_t* x, uint32_t sizeQl, uint64_t t, uint32_t batch,
                                   uint64_t* out, void* ws, size_t wsBytes, void* stream);
/* BGV on HYBRID keys.  The reference passes t = GetPlaintextModulus() to ApproxModDown whenever GetNoiseScale() != 1
 * (keyswitch-hybrid.cpp:263, 299, 386); these are the composites above in that form.  Same plan, key, workspace and tower layout as
 * their twins and the same launches: the ModDown runs with the conversion of fhe_approx_mod_down_bgv under the same fused store (the
 * accumulating one included).  t >= 2 and invertible modulo every p_j, checked before the first launch; otherwise the twin's checks.
 *   fhe_bgv_keyswitch_hybrid[_acc]  KeySwitchHYBRID::KeySwitchCore (keyswitch-hybrid.cpp:308-400) [+ base-leveledshe.cpp:210-211]
 *   fhe_bgv_eval_mult               LeveledSHEBase::EvalMult(ct, ct, key) (base-leveledshe.cpp:201-214, 607-644)
 *   fhe_bgv_ks_fast_keyswitch       EvalFastKeySwitchCore (keyswitch-hybrid.cpp:381-400) on the digits fhe_ks_precompute left: the digit
 *                                   decomposition does not depend on t, so hoisting is shared with CKKS
 *   fhe_bgv_eval_fast_rotation      LeveledSHEBase::EvalFastRotation (base-leveledshe.cpp:432-463)
 *   fhe_bgv_eval_automorphism       LeveledSHEBase::EvalAutomorphism (base-leveledshe.cpp:381-422) */
fhe_status fhe_bgv_keyswitch_hybrid(fhe_ks_plan* plan, const fhe_ks_key* key, const uint64_t* c, uint32_t sizeQl, uint64_t t,
                                    uint32_t batch, uint64_t* out0, uint64_t* out1, void* ws, size_t wsBytes, void* stream);
fhe_status fhe_bgv_keyswitch_hybrid_acc(fhe_ks_plan* plan, const fhe_ks_key* key, const uint64_t* c, uint32_t sizeQl, uint64_t t,
                                        uint32_t batch, uint64_t* acc0, uint64_t* acc1, void* ws, size_t wsBytes, void* stream);
fhe_status fhe_bgv_eval_mult(fhe_ks_plan* plan, const fhe_ks_key* key, const uint64_t* a0, const uint64_t* a1, const uint64_t* b0,
                             const uint64_t* b1, uint32_t sizeQl, uint64_t t, uint32_t batch, uint64_t* c0, uint64_t* c1, void* ws,
                             size_t wsBytes, void* stream);
fhe_status fhe_bgv_ks_fast_keyswitch(fhe_ks_plan* plan, const fhe_ks_key* key, const uint64_t* c1, uint32_t sizeQl, uint64_t t,
                                     uint32_t batch, uint64_t* out0, uint64_t* out1, void* ws, size_t wsBytes, void* stream);
fhe_status fhe_bgv_eval_fast_rotation(fhe_ks_plan* plan, const fhe_ks_key* key, const uint64_t* c0, const uint64_t* c1, uint32_t k,
                                      uint32_t sizeQl, uint64_t t, uint32_t batch, uint64_t* out0, uint64_t* out1, void* ws,
                                      size_t wsBytes, void* stream);
fhe_status fhe_bgv_eval_automorphism(fhe_ks_plan* plan, const fhe_ks_key* key, const uint64_t* c0, const uint64_t* c1, uint32_t k,
                                     uint32_t sizeQl, uint64_t t, uint32_t batch, uint64_t* out0, uint64_t* out1, void* ws,
                                     size_t wsBytes, void* stream);

/* ---- a15: CKKS rescale ---------------------------------------------------------------------------
 * Replaces DCRTPolyImpl::DropLastElementAndScale (dcrtpoly-impl.h:693-712) with the tables of
 * CryptoParametersCKKSRNS (src/pke/lib/scheme/ckksrns/ckksrns-cryptoparameters.cpp:60-81) computed inside.
 * The tower uses context limbs [0,sizeQl). x[batch][sizeQl][N] EVALUATION -> out[batch][sizeQl-1][N].
 * ws: device workspace of fhe_rescale_workspace_bytes(). */
size_t     fhe_rescale_workspace_bytes(const fhe_ctx* ctx, uint32_t sizeQl, uint32_t batch);
fhe_status fhe_rescale(fhe_ctx* ctx, const uint64_t* x, uint32_t sizeQl, uint32_t batch, uint64_t* out, void* ws,
                       size_t wsBytes, void* stream);
/* The same over any limbs of the context (limbIdx[sizeQl], NULL = the leading ones; the last entry is the dropped limb) with the
 * CALLER's tables, host arrays of sizeQl-1 residues as DropLastElementAndScale receives them (dcrtpoly-impl.h:693-694).  When
 * QlQlInvModqlDivqlModq[i] == -qlInvModq[i] mod q_i (the reference's own tables) on a ring of two static passes, the call is 4
 * launches: the switched tower and its transform never go to HBM (fhe_hip.cpp drop_last_run).  out must not alias x. */
fhe_status fhe_rescale_limbs(fhe_ctx* ctx, const uint64_t* x, const uint32_t* limbIdx, uint32_t sizeQl,
                             const uint64_t* QlQlInvModqlDivqlModq, const uint64_t* qlInvModq, uint32_t batch, uint64_t* out,
                             void* ws, size_t wsBytes, void* stream);
/* The two elements of one ciphertext — towers x0, x1 -> out0, out1, each allocated on its own, any distance apart — in the same
 * four launches (LeveledSHECKKSRNS::ModReduceInternalInPlace, ckksrns-leveledshe.cpp:172-191, applies the member to both elements
 * with the same tables); ws of fhe_rescale_workspace_bytes(ctx, sizeQl, 2). */
fhe_status fhe_rescale_limbs_pair(fhe_ctx* ctx, const uint64_t* x0, const uint64_t* x1, const uint32_t* limbIdx, uint32_t sizeQl,
                                  const uint64_t* QlQlInvModqlDivqlModq, const uint64_t* qlInvModq, uint64_t* out0, uint64_t* out1,
                                  void* ws, size_t wsBytes, void* stream);
/* ---- CKKS rescale by several limbs in one pass (composite scaling) ---------------------------------------------------
 * Replaces the loop of LeveledSHECKKSRNS::ModReduceInternalInPlace(ct, levels) (ckksrns-leveledshe.cpp:172-191: DropLastElementAndScale
 * `levels` times on every element; levels = compositeDegree under COMPOSITESCALINGAUTO / COMPOSITESCALINGMANUAL), optionally with the scalar
 * product in front and the level drop behind it that AdjustLevelsAndDepthInPlace (ckksrns-leveledshe.cpp:600-730) adds:
 *   x[batch][sizeQl][N] EVALUATION -> out[batch][nOut][N], 1 <= nOut <= sizeQl - levels;
 *   scale: NULL, or host residues scale[sizeQl] of the integer of EvalMultCoreInPlace(ct, double) as the caller computed it: every limb is
 *          multiplied by its residue first;
 *   nOut < sizeQl - levels: the LevelReduceInternalInPlace that follows -- those limbs are not produced.
 * The words are those of the loop.  On a ring of two static passes (N >= 8192) with the reference's own tables a call of levels <= 4 is five
 * launches whatever levels is; more levels run in chunks of at most 4; smaller rings, other tables, a zero scale residue and
 * FHE_RESCALE_UNFUSED=1 run the member step by step.  levels == 1 without scale and with nOut == sizeQl - 1 is fhe_rescale itself.
 * Errors (nothing is enqueued): a null argument, levels == 0 or levels >= sizeQl, nOut out of range, a limb index outside the context, a
 * table or scale entry that is not reduced modulo its limb, a workspace below fhe_rescale_multi_workspace_bytes, out aliasing x. */
size_t     fhe_rescale_multi_workspace_bytes(const fhe_ctx* ctx, uint32_t sizeQl, uint32_t levels, uint32_t batch);
/* tables of CryptoParametersCKKSRNS (ckksrns-cryptoparameters.cpp:60-81) computed inside; context limbs [0, sizeQl) */
fhe_status fhe_rescale_multi(fhe_ctx* ctx, const uint64_t* x, uint32_t sizeQl, uint32_t levels, uint32_t nOut, const uint64_t* scale,
                             uint32_t batch, uint64_t* out, void* ws, size_t wsBytes, void* stream);
/* any limbs of the context (limbIdx[sizeQl], NULL = the leading ones; the LAST entries are dropped, the last one first) with the CALLER's
 * tables as the loop's steps receive them (dcrtpoly-impl.h:693-694): step k = 0 .. levels-1 drops limb sizeQl-1-k and reads the
 * sizeQl-1-k residues GetQlQlInvModqlDivqlModq(.) / GetqlInvModq(.) of that level at offset sum_{j<k} (sizeQl-1-j) of each array. */
fhe_status fhe_rescale_multi_limbs(fhe_ctx* ctx, const uint64_t* x, const uint32_t* limbIdx, uint32_t sizeQl, uint32_t levels,
                                   uint32_t nOut, const uint64_t* scale, const uint64_t* QlQlInvModqlDivqlModq,
                                   const uint64_t* qlInvModq, uint32_t batch, uint64_t* out, void* ws, size_t wsBytes, void* stream);
/* both elements of a ciphertext (towers x0, x1 -> out0, out1, each allocated on its own) in the same launches, as
 * ModReduceInternalInPlace treats them (ckksrns-leveledshe.cpp:176-181); ws of fhe_rescale_multi_workspace_bytes(ctx, sizeQl, levels, 2) */
fhe_status fhe_rescale_multi_limbs_pair(fhe_ctx* ctx, const uint64_t* x0, const uint64_t* x1, const uint32_t* limbIdx, uint32_t sizeQl,
                                        uint32_t levels, uint32_t nOut, const uint64_t* scale, const uint64_t* QlQlInvModqlDivqlModq,
                                        const uint64_t* qlInvModq, uint64_t* out0, uint64_t* out1, void* ws, size_t wsBytes,
                                        void* stream);
/* The host-side constants of one fused pass of d <= 4 limbs, as the library derives them (host_math.h rescale_multi_tables; nothing touches a
 * device): qDrop[d] in dropping order, qKeep[nKeep] the produced limbs, sDrop / sKeep the scalar's residues (both NULL: none).  Pairs
 * {value, Shoup companion}: B[d][d][2] (q_k^-1 mod q_j for k < j, else 0), W[d][nKeep][2], C[nKeep][2], S[d][2]. */
fhe_status fhe_rescale_multi_host_tables(const uint64_t* qDrop, uint32_t d, const uint64_t* qKeep, uint32_t nKeep, const uint64_t* sDrop,
                                         const uint64_t* sKeep, uint64_t* B, uint64_t* W, uint64_t* C, uint64_t* S);
/* DCRTPolyImpl::ModReduce (dcrtpoly-impl.h:736-755) — BGV modulus switching by the last limb with plaintext modulus t
 * (tables negtInvModq / qlInvModq / tModqPrecon of CryptoParametersBGVRNS are derived inside): x [batch][sizeQl][N] in
 * `evalFormat`, out [batch][sizeQl-1][N] in the same format; ws as for fhe_rescale. */
fhe_status fhe_mod_reduce(fhe_ctx* ctx, const uint64_t* x, uint32_t sizeQl, uint64_t t, int evalFormat, uint32_t batch,
                          uint64_t* out, void* ws, size_t wsBytes, void* stream);
/* An EVALUATION tower on a ring of static passes (N >= 4096) takes the fused form (fhe_hip.cpp drop_last_run): with
 * d = INTT(x_l) * (t^-1 mod q_l), out_i = (x_i - NTT((t mod q_i) * SwitchModulus(d -> q_i))) * q_l^-1 -- the reference's words, because
 * SwitchModulus is odd under negation for odd q_l and every step yields canonical residues.  On rings of two passes that is five launches
 * (two INTT passes of the dropped limb, the one-row product, the column pass that switches and multiplies on its way in, the row pass
 * whose store is the last line); the switched tower and its transform never go to HBM.  Smaller rings and COEFFICIENT towers run the
 * member launch by launch.  t may exceed a limb (its residue is used); t must be invertible modulo the dropped limb.
 *
 * fhe_mod_reduce_limbs: the same over any limbs of the context (limbIdx[sizeQl], NULL = the leading ones; the last entry is the dropped
 * limb) with the CALLER's tables as DCRTPolyImpl::ModReduce receives them (dcrtpoly-impl.h:736-738): t, negtInvModq = -t^-1 mod q_l and
 * qlInvModq[sizeQl-1] (CryptoParametersBGVRNS::GetNegtInvModq(l) / GetqlInvModq(l)).  Fused exactly when those are the values the library
 * derives itself; any other reduced values run the member's formula with them, launch by launch.  Errors: null argument, sizeQl < 2, a
 * limb index outside the context, a workspace below fhe_rescale_workspace_bytes, t < 2 or a multiple of the dropped limb, a table entry
 * that is not reduced modulo its limb.  out must not alias x. */
fhe_status fhe_mod_reduce_limbs(fhe_ctx* ctx, const uint64_t* x, const uint32_t* limbIdx, uint32_t sizeQl, uint64_t t,
                                uint64_t negtInvModq, const uint64_t* qlInvModq, int evalFormat, uint32_t batch, uint64_t* out,
                                void* ws, size_t wsBytes, void* stream);
/* The two elements of one ciphertext -- towers x0, x1 -> out0, out1, each allocated on its own -- in the same launches
 * (LeveledSHEBGVRNS::ModReduceInternalInPlace, bgvrns-leveledshe.cpp:44-75, applies the member to both elements with the same tables);
 * ws of fhe_rescale_workspace_bytes(ctx, sizeQl, 2). */
fhe_status fhe_mod_reduce_limbs_pair(fhe_ctx* ctx, const uint64_t* x0, const uint64_t* x1, const uint32_t* limbIdx, uint32_t sizeQl,
                                     uint64_t t, uint64_t negtInvModq, const uint64_t* qlInvModq, int evalFormat, uint64_t* out0,
                                     uint64_t* out1, void* ws, size_t wsBytes, void* stream);
/* ---- BGV level alignment of the automatic scaling modes in one pass ---------------------------------------------------
 * Under FLEXIBLEAUTO / FLEXIBLEAUTOEXT every EvalMult, EvalAdd and EvalSub first calls LeveledSHEBGVRNS::AdjustLevelsAndDepth[ToOne]InPlace
 * (bgvrns-leveledshe.cpp:83-233), which on one operand is some of: cv[i] *= scalar, ModReduceInternalInPlace (:44-75, DCRTPolyImpl::ModReduce
 * on every element, dcrtpoly-impl.h:736-755), a LevelReduce, ModReduceInternalInPlace again.  One call here.  The result is the words of
 *   multiply every row by scalar mod q_i; then, for k = 0 .. levels-1, discard the rows above dropRows[k] and call ModReduce on row
 *   dropRows[k]; keep rows 0 .. nOut-1:
 *   x[batch][sizeQl][N] in `evalFormat` -> out[batch][nOut][N] in the same format.
 *   dropRows: NULL = the last `levels` rows, the last one first.  Otherwise strictly decreasing, each < sizeQl, the lowest >= 1, and
 *             levels <= 4.  1 <= nOut <= dropRows[levels-1].  More than 4 levels (trailing rows only) run in chunks of 4, the scalar in
 *             the first chunk.
 *   scalar:   the integer of the scalar product (1: none); its residues are taken inside.  t may exceed a limb (its residue is used).
 * An EVALUATION tower on a ring of two static passes (N >= 8192) takes the fused form: the dropped rows to COEFFICIENT, a
 * chain kernel that leaves rho_k, the canonical residue of -delta_k of every step, the forward column pass whose load sums the switched
 * rho_k times (t mod q_i) * scalar^-1 * prod_{j<k} q_{r_j}, the row pass whose store is (x_i - r_i) * scalar * prod_k q_{r_k}^-1.
 * Launches: 5 when the dropped rows are adjacent, 5 + 2 * (runs - 1) when they form `runs` groups of adjacent rows (each group is an inverse
 * transform of two passes): 7 for ModReduce, LevelReduce, ModReduce, which is all the reference's case table asks for.
 * Everything else runs the member's formula step by step with the launches of fhe_mul_const and fhe_mod_reduce: rings below 8192,
 * COEFFICIENT towers, a scalar whose residue is zero modulo some row, tables that are not the derived ones, FHE_MOD_REDUCE_UNFUSED=1, and
 * the plain case levels == 1, scalar == 1, nOut == dropRows[0], which is fhe_mod_reduce itself on rows 0 .. dropRows[0].
 * fhe_mod_reduce_multi_limbs: any limbs of the context (limbIdx[sizeQl], NULL = the leading ones) with the CALLER's tables as the steps
 * receive them: negtInvModq[k] = -t^-1 mod q_{dropRows[k]} and, for step k, the dropRows[k] residues of qlInvModq at offset
 * sum_{j<k} dropRows[j].  Fused only when they equal what the library derives (the rule of fhe_mod_reduce_limbs).
 * Errors, each before anything is enqueued: a null argument; levels outside [1, sizeQl); a malformed dropRows; nOut out of range; a limb
 * index outside the context; t < 2 or a multiple of a dropped modulus; equal moduli in the tower; a table entry that is not reduced; a
 * workspace below fhe_mod_reduce_multi_workspace_bytes; out aliasing x. */
size_t     fhe_mod_reduce_multi_workspace_bytes(const fhe_ctx* ctx, uint32_t sizeQl, uint32_t levels, uint32_t batch);
fhe_status fhe_mod_reduce_multi(fhe_ctx* ctx, const uint64_t* x, uint32_t sizeQl, uint64_t t, uint64_t scalar, const uint32_t* dropRows,
                                uint32_t levels, uint32_t nOut, int evalFormat, uint32_t batch, uint64_t* out, void* ws, size_t wsBytes,
                                void* stream);
fhe_status fhe_mod_reduce_multi_limbs(fhe_ctx* ctx, const uint64_t* x, const uint32_t* limbIdx, uint32_t sizeQl, uint64_t t,
                                      uint64_t scalar, const uint32_t* dropRows, uint32_t levels, uint32_t nOut,
                                      const uint64_t* negtInvModq, const uint64_t* qlInvModq, int evalFormat, uint32_t batch, uint64_t* out,
                                      void* ws, size_t wsBytes, void* stream);
/* both elements of a ciphertext (towers x0, x1 -> out0, out1, each allocated on its own) in the same launches;
 * ws of fhe_mod_reduce_multi_workspace_bytes(ctx, sizeQl, levels, 2) */
fhe_status fhe_mod_reduce_multi_limbs_pair(fhe_ctx* ctx, const uint64_t* x0, const uint64_t* x1, const uint32_t* limbIdx, uint32_t sizeQl,
                                           uint64_t t, uint64_t scalar, const uint32_t* dropRows, uint32_t levels, uint32_t nOut,
                                           const uint64_t* negtInvModq, const uint64_t* qlInvModq, int evalFormat, uint64_t* out0,
                                           uint64_t* out1, void* ws, size_t wsBytes, void* stream);
/* The host-side constants of one fused pass of d <= 4 steps (host_math.h mod_reduce_multi_tables; nothing touches a device): the layout of
 * fhe_rescale_multi_host_tables, with S[k] = sDrop[k] * t^-1 mod qDrop[k] and W[k][i] times t mod qKeep[i]. */
fhe_status fhe_mod_reduce_multi_host_tables(const uint64_t* qDrop, uint32_t d, const uint64_t* qKeep, uint32_t nKeep, uint64_t t,
                                            const uint64_t* sDrop, const uint64_t* sKeep, uint64_t* B, uint64_t* W, uint64_t* C,
                                            uint64_t* S);
/* BGV decryption: the ModReduce chain down to one limb, and its residues modulo t, without a tower between the steps.
 * PKEBGVRNS::Decrypt (bgvrns-pke.cpp:44-99) and MultipartyBGVRNS::MultipartyDecryptFusion (bgvrns-multiparty.cpp:62-97) switch
 * b = c0 + c1*s (+ c2*s^2) to COEFFICIENT, call DCRTPolyImpl::ModReduce sizeQl - 1 times and take DecryptionCRTInterpolate(t) of the
 * limb that is left.  Here one launch of mod_reduce_chain_kernel runs up to 16 of those steps: the deltas of the dropped limbs stay in
 * registers, every kept limb is read once and written once.  The tables (negtInvModq, qlInvModq, t mod q_i of every step, multiplied
 * out) are the library's own, derived from the moduli and t and kept per (limb list, t, steps).  All towers are COEFFICIENT, all words in
 * and out canonical; every comparison with the member's loop is word for word.
 *
 * fhe_mod_reduce_chain: `levels` consecutive DCRTPolyImpl::ModReduce calls (dcrtpoly-impl.h:736-755), the words of `levels` calls of
 * fhe_mod_reduce with evalFormat 0: x [batch][sizeQl][N] over limbIdx[sizeQl] (NULL = the leading limbs), the last limb dropped first;
 * out [batch][sizeQl-levels][N].  What the COEFFICIENT branch of Decrypt (bgvrns-pke.cpp:73-81) runs on every element.  More than 16
 * levels run in chunks of 16 through ws (fhe_mod_reduce_chain_workspace_bytes; 0 bytes, and ws may be NULL, up to 16 levels).
 * fhe_mod_reduce_to_t: the whole chain (sizeQl - 1 steps; sizeQl == 1: none) and then (x_0 > floor(q_0/2) ? x_0 - q_0 : x_0) mod t in
 * [0, t), NativeVector::Mod(t) of DecryptionCRTInterpolate (mubintvecnat.cpp:145-161, 351-356): out [batch][N].  ws as for
 * fhe_mod_reduce_chain with levels = sizeQl - 1.  Serves MultipartyDecryptFusion after the caller's sum and inverse transform.
 * fhe_bgv_decrypt: the EVALUATION branch of Decrypt (bgvrns-pke.cpp:52-60, 96).  c[nElem] (host array, nElem 2 or 3): element e of
 * `batch` ciphertexts, each [batch][sizeQl][N]; s: the secret key, ONE tower [sizeQl][N]; all EVALUATION over limbIdx.  PKERNS::DecryptCore
 * (rns-pke.cpp:199-216) with element-wise launches (2, or 4 with s^2 formed for nElem == 3), ONE inverse transform of all limbs of all
 * towers, then the chain to t.  out [batch][N]; ws of fhe_bgv_decrypt_workspace_bytes.
 * Errors, each before anything is enqueued: a null argument; levels outside [1, sizeQl); a limb index outside the context; t < 2 (to_t and
 * decrypt: or t >= 2^63), t a multiple of a dropped limb, equal moduli in the tower; a short workspace; out aliasing x. */
size_t fhe_mod_reduce_chain_workspace_bytes(const fhe_ctx* ctx, uint32_t sizeQl, uint32_t levels, uint32_t batch);
fhe_status fhe_mod_reduce_chain(fhe_ctx* ctx, const uint64_t* x, const uint32_t* limbIdx, uint32_t sizeQl, uint32_t levels, uint64_t t,
                                uint32_t batch, uint64_t* out, void* ws, size_t wsBytes, void* stream);
fhe_status fhe_mod_reduce_to_t(fhe_ctx* ctx, const uint64_t* x, const uint32_t* limbIdx, uint32_t sizeQl, uint64_t t, uint32_t batch,
                               uint64_t* out, void* ws, size_t wsBytes, void* stream);
size_t fhe_bgv_decrypt_workspace_bytes(const fhe_ctx* ctx, uint32_t nElem, uint32_t sizeQl, uint32_t batch);
fhe_status fhe_bgv_decrypt(fhe_ctx* ctx, const uint64_t* const* c, uint32_t nElem, const uint64_t* s, const uint32_t* limbIdx,
                           uint32_t sizeQl, uint64_t t, uint32_t batch, uint64_t* out, void* ws, size_t wsBytes, void* stream);

/* ---- a17: ScaleAndRound family (BFV HPS) ----------------------------------------------------------------
 * fhe_sr_plan_create keeps the caller's tables on the device. They are the reference's own
 * (CryptoParametersBFVRNS getters, e.g. GettRSHatInvModsDivsModr / GettRSHatInvModsDivsFrac,
 * src/pke/include/schemerns/rns-cryptoparameters.h:829-848): tab is [sizeO][sizeI+1] exactly as the reference
 * indexes it, frac is [sizeI] (NULL selects ApproxScaleAndRound, which has no fractional part).
 * fhe_scale_and_round replaces DCRTPolyImpl::ScaleAndRound (dcrtpoly-impl.h:1513-1628) / ApproxScaleAndRound
 * (:1470-1510): x is [batch][sizeI+sizeO][N] COEFFICIENT; outputFirst != 0 means the output basis is the FIRST
 * sizeO limbs of x (the reference decides this by comparing the first moduli, :1527-1534), else the LAST sizeO.
 * out is [batch][sizeO][N].
 * fhe_scale_and_round_p_over_q replaces ScaleAndRoundPOverQ (:1674-1689): x [batch][sizeQ+1][N] over the context
 * limbs limbIdx[0..sizeQ] -> out [batch][sizeQ][N]. */
typedef struct fhe_sr_plan fhe_sr_plan;
fhe_status fhe_sr_plan_create(fhe_ctx* ctx, uint32_t sizeI, const uint32_t* outLimbIdx, uint32_t sizeO,
                              const uint64_t* tab, const double* frac, fhe_sr_plan** out);
void       fhe_sr_plan_destroy(fhe_sr_plan* plan);
fhe_status fhe_scale_and_round(fhe_sr_plan* plan, const uint64_t* x, int outputFirst, uint64_t* out, uint32_t batch,
                               void* stream);
fhe_status fhe_scale_and_round_p_over_q(fhe_ctx* ctx, const uint64_t* x, const uint32_t* limbIdx, uint32_t sizeQ,
                                        uint64_t* out, uint32_t batch, void* stream);

/* ScaleAndRound -> NativePoly modulo t, the BFV decryption step (dcrtpoly-impl.h:1190-1467): x [batch][sizeQ][N]
 * COEFFICIENT over the context limbs limbIdx (NULL: 0..sizeQ-1) -> out [batch][N] residues mod t.  Tables are the
 * reference's tQHatInvModqDivqModt, tQHatInvModqBDivqModt, tQHatInvModqDivqFrac, tQHatInvModqDivqBFrac (the two "B"
 * tables may be NULL when max(q_i) and sizeQ keep the reference on its unsplit branches); which of the reference's eight
 * branches runs is decided from (max q_i, t, sizeQ) exactly as there.  fhe_scale_and_round_behz_decrypt is the BEHZ
 * overload (:1631-1671) with tgammaQHatModq / negInvqModtgamma, gamma = 2^26. */
fhe_status fhe_scale_and_round_native(fhe_ctx* ctx, const uint64_t* x, const uint32_t* limbIdx, uint32_t sizeQ, uint64_t t,
                                      const uint64_t* tabModt, const uint64_t* tabBModt, const double* frac,
                                      const double* bfrac, uint32_t batch, uint64_t* out, void* stream);
fhe_status fhe_scale_and_round_behz_decrypt(fhe_ctx* ctx, const uint64_t* x, const uint32_t* limbIdx, uint32_t sizeQ,
                                            uint64_t tgamma, const uint64_t* tgammaQHatModq,
                                            const uint64_t* negInvqModtgamma, uint32_t batch, uint64_t* out, void* stream);

/* ---- a18: BEHZ base conversions (BFV) ---------------------------------------------------------------------
 * fhe_behz_create builds the tables of CryptoParametersBFVRNS's BEHZ block
 * (src/pke/lib/scheme/bfvrns/bfvrns-cryptoparameters.cpp:673-850) for the basis Q (context limbs qLimbIdx) and
 * Bsk = B ∪ {m_sk} (context limbs bskLimbIdx, numQ+1 of them, m_sk last), plaintext modulus t, m̃ = 2^16.
 * fhe_param_behz_bsk returns the Bsk moduli/roots the reference would pick (:682-711) so that a caller can put them
 * into the context; it returns numQ+1, or 0 if m_sk would need more than 60 bits.
 * Towers are x[batch][numQ+numBsk][N].  numQ <= 63 (a tower of Q and Bsk limbs has at most 127 rows): up to 15 Q limbs run on kernels that
 * keep one coefficient's residues in registers, 16 ... 63 on kernels that keep them in a per-lane array (same exact sums, same residues).
 *   fhe_behz_q_to_bsk  = FastBaseConvqToBskMontgomery (dcrtpoly-impl.h:1694-1786): Q rows in `evalFormat` on entry,
 *                        all rows EVALUATION on return (ws: fhe_behz_workspace_bytes, only needed for EVALUATION input);
 *   fhe_behz_floorq    = FastRNSFloorq (:1791-1840), COEFFICIENT, in place;
 *   fhe_behz_conv_sk   = FastBaseConvSK (:1845-1929), COEFFICIENT, result out[batch][numQ][N]. */
typedef struct fhe_behz fhe_behz;
uint32_t   fhe_param_behz_bsk(uint32_t logN, uint32_t numQ, const uint64_t* q, uint64_t t, uint64_t* bsk, uint64_t* psiBsk);
fhe_status fhe_behz_create(fhe_ctx* ctx, const uint32_t* qLimbIdx, uint32_t numQ, const uint32_t* bskLimbIdx, uint64_t t,
                           fhe_behz** out);
void       fhe_behz_destroy(fhe_behz* plan);
/* The CALLER's tables in place of the derived ones, one member at a time — the vectors the reference passes to that member
 * (dcrtpoly-interface.h: FastBaseConvqToBskMontgomery, FastRNSFloorq, FastBaseConvSK), flattened row-major in the reference's index
 * order: QHatModbsk / qInvModbsk [numQ][numBsk], BHatModq [numB][numQ], vectors over Q, Bsk or B.  With an override the member
 * computes with the caller's VALUES (whatever they are), as DCRTPolyImpl does; a DCRTPoly backend keeps one plan per member and
 * table content.  The Barrett constants are functions of the moduli and stay derived. */
fhe_status fhe_behz_override_q_to_bsk(fhe_behz* plan, const uint64_t* mtildeQHatInvModq, const uint64_t* QHatModbsk,
                                      const uint64_t* QHatModmtilde, const uint64_t* QModbsk, uint64_t negQInvModmtilde,
                                      const uint64_t* mtildeInvModbsk);
fhe_status fhe_behz_override_floorq(fhe_behz* plan, const uint64_t* tQHatInvModq, const uint64_t* QHatModbsk,
                                    const uint64_t* qInvModbsk, const uint64_t* tQInvModbsk);
fhe_status fhe_behz_override_conv_sk(fhe_behz* plan, const uint64_t* BHatInvModb, const uint64_t* BHatModmsk, uint64_t BInvModmsk,
                                     const uint64_t* BHatModq, const uint64_t* BModq);

size_t     fhe_behz_workspace_bytes(const fhe_behz* plan, uint32_t batch);
fhe_status fhe_behz_q_to_bsk(fhe_behz* plan, uint64_t* x, int evalFormat, uint32_t batch, void* ws, size_t wsBytes,
                             void* stream);
fhe_status fhe_behz_floorq(fhe_behz* plan, uint64_t* x, uint32_t batch, void* stream);
fhe_status fhe_behz_conv_sk(fhe_behz* plan, const uint64_t* x, uint64_t* out, uint32_t batch, void* stream);
/* LeveledSHEBFVRNS::EvalMult, BEHZ branch, no relinearisation (src/pke/lib/scheme/bfvrns/bfvrns-leveledshe.cpp:198-445;
 * config 5 of BASELINE.json): the four input elements [batch][numQ][N] EVALUATION -> three product elements
 * [batch][numQ][N], COEFFICIENT as the reference returns them, or EVALUATION when outEval != 0 (the SetFormat that
 * LeveledSHEBase::EvalMult(ct,ct,key) applies before KeySwitchCore, base-leveledshe.cpp:204-205). */
size_t     fhe_bfv_eval_mult_behz_workspace_bytes(const fhe_behz* plan, uint32_t batch);
fhe_status fhe_bfv_eval_mult_behz(fhe_behz* plan, const uint64_t* a0, const uint64_t* a1, const uint64_t* b0,
                                  const uint64_t* b1, uint64_t* d0, uint64_t* d1, uint64_t* d2, int outEval,
                                  uint32_t batch, void* ws, size_t wsBytes, void* stream);
/* The same with relinearisation — LeveledSHEBase::EvalMult(ct, ct, key) on BFV/BEHZ ciphertexts (base-leveledshe.cpp:201-214):
 * EvalMultNoRelin, SetFormat(EVALUATION), KeySwitchCore on the third element, c0 += ks0, c1 += ks1.  The context holds Q
 * as its leading limbs (the key-switch plan's Q), P, and the Bsk limbs; outputs [batch][numQ][N] EVALUATION. */
size_t     fhe_bfv_eval_mult_relin_workspace_bytes(const fhe_behz* plan, const fhe_ks_plan* ks, uint32_t batch);
fhe_status fhe_bfv_eval_mult_relin_behz(fhe_behz* plan, fhe_ks_plan* ks, const fhe_ks_key* key, const uint64_t* a0,
                                        const uint64_t* a1, const uint64_t* b0, const uint64_t* b1, uint64_t* c0, uint64_t* c1,
                                        uint32_t batch, void* ws, size_t wsBytes, void* stream);

/* ---- a18: BFV EvalMult, HPS family ----------------------------------------------------------------------------
 * LeveledSHEBFVRNS::EvalMult for the multiplication techniques HPS (1), HPSPOVERQ (2) and HPSPOVERQLEVELED (3, the
 * reference's default; enum MultiplicationTechnique, constants-defs.h:97), without relinearisation
 * (src/pke/lib/scheme/bfvrns/bfvrns-leveledshe.cpp:198-302, 354-412, 435-438).
 * fhe_param_hps_r returns the auxiliary basis R the reference picks (bfvrns-cryptoparameters.cpp:75, 126-139):
 * r_0 = PreviousPrime(q_{numQ-1}, 2N), r_j = PreviousPrime(r_{j-1}, 2N) with their minimum primitive 2N-th roots; numQ + 1
 * moduli for HPS, numQ otherwise.  Returns the count, 0 on a bad argument.
 * fhe_hps_create builds, in the call, every table of CryptoParametersBFVRNS::PrecomputeCRTTables' HPS block (:143-265, 267-665)
 * for Q (context limbs qLimbIdx) and R (rLimbIdx), for every level l = 0 .. numQ-1 with HPSPOVERQ[LEVELED], from the moduli with
 * 64-bit modular arithmetic.  numQ + numR <= 256.  fhe_hps_table reads a derived table back (ids and layouts: see the definition
 * in fhe_hip.cpp; doubles as bit patterns); it returns the table's length in 64-bit words, 0 if the plan has no such table.
 * fhe_bfv_eval_mult_hps: inputs [batch][numQ][N] EVALUATION -> outputs [batch][numQ][N], COEFFICIENT as the reference leaves
 * them, or EVALUATION when outEval != 0 (then fhe_keyswitch_hybrid_acc relinearises with a HYBRID key at numQ limbs, fhe_keyswitch_bv with
 * accumulate != 0 with a BV key; fhe_bfv_eval_mult_relin_hps_bv is the whole BV sequence, fhe_bfv_eval_mult_relin_hps_hybrid the whole HYBRID
 * one at any level the reference drops to).  sizeQl = l + 1 is the number of Q limbs the
 * product is computed over: numQ for HPS and HPSPOVERQ; for HPSPOVERQLEVELED the caller's numQ - levelsDropped (FindLevelsToDrop is
 * host-side noise estimation and stays in pke).  A wrong sizeQl or too small a workspace is an error and enqueues nothing.  The call
 * builds nothing lazily, allocates nothing and does not synchronise: it can be captured into a graph.
 * Sequences (the replaced reference lines):
 *   HPS        a, b: ExpandCRTBasis Q -> QR (:223-235); product: ScaleAndRound QR -> R, SwitchCRTBasis R -> Q (:368-383)
 *   HPSPOVERQ  a: ExpandCRTBasis (:239-246); b: FastExpandCRTBasisPloverQ (:256-261); product: ScaleAndRound QR -> Q (:385-395)
 *   LEVELED    sizeQl == numQ as HPSPOVERQ; below: a: ScaleAndRound Q -> Q_l, ExpandCRTBasis Q_l -> Q_lR_l (:274-287);
 *              b: FastExpandCRTBasisPloverQ from Q (:289-301); product: ScaleAndRound Q_lR_l -> Q_l, ExpandCRTBasisQlHat (:397-411)
 * FastExpandCRTBasisPloverQ, the HPS tail and the LEVELED head run as ONE kernel each that keeps the middle basis in registers
 * (p_over_q_expand_kernel, scale_round_switch_kernel; bfv_kernels.h) while every basis involved has at most 16 limbs (HPS: numQ <= 15,
 * since R has numQ + 1); beyond that the same residues come from the separate launches.
 * Not covered: ciphertexts with more than two elements, and the compressed-ciphertext branch (sizeQ < sizeQM, :237-262). */
typedef struct fhe_hps fhe_hps;
uint32_t   fhe_param_hps_r(uint32_t logN, uint32_t numQ, const uint64_t* q, int technique, uint64_t* r, uint64_t* psiR);
fhe_status fhe_hps_create(fhe_ctx* ctx, const uint32_t* qLimbIdx, uint32_t numQ, const uint32_t* rLimbIdx, uint32_t numR,
                          uint64_t t, int technique, fhe_hps** out);
void       fhe_hps_destroy(fhe_hps* plan);
size_t     fhe_hps_table(const fhe_hps* plan, int tableId, uint32_t level, uint64_t* out, size_t cap);
size_t     fhe_bfv_eval_mult_hps_workspace_bytes(const fhe_hps* plan, uint32_t sizeQl, uint32_t batch);
fhe_status fhe_bfv_eval_mult_hps(fhe_hps* plan, const uint64_t* a0, const uint64_t* a1, const uint64_t* b0, const uint64_t* b1,
                                 uint64_t* d0, uint64_t* d1, uint64_t* d2, uint32_t sizeQl, int outEval, uint32_t batch,
                                 void* ws, size_t wsBytes, void* stream);

/* ---- BV key switching ---------------------------------------------------------------------------------------
 * KeySwitchBV (src/pke/lib/keyswitch/keyswitch-bv.cpp), the reference's default technique for BFV (gen-cryptocontext-params-defaults.h) and
 * the one PRE and multiparty use.  No auxiliary basis and no ModDown: the same calls serve BFV, BGV and CKKS.  The tower uses the context's
 * leading limbs [0, sizeQ); baseBits is the digit size r (0: one digit per limb).
 * A key is the b and a vectors of the evaluation key (KeySwitchGenInternal, keyswitch-bv.cpp:49-103): D_0 =
 * fhe_crt_decompose_towers(ctx, NULL, sizeQ, baseBits) towers over all sizeQ limbs each, in the order of DCRTPolyImpl::CRTDecompose (limb 0's
 * windows, least significant first, then limb 1's ...).  The windows of a limb depend on its modulus only, so a level sizeQl <= sizeQ uses the
 * FIRST D_l = fhe_crt_decompose_towers(ctx, NULL, sizeQl, baseBits) key towers, and of each its first sizeQl rows (DropLastElements, :264-271):
 * output limb i meets key row i.  The key carries (ctx, sizeQ, baseBits, D_0); there is no plan object.
 * Apart from key upload every call builds nothing lazily, allocates nothing and does not synchronise: it can be captured into a graph.  An
 * error enqueues nothing: a null argument, sizeQl outside [1, sizeQ], too small a workspace, a key of another context, and
 * FHE_ERR_UNSUPPORTED at key upload and at precompute for a digit size outside the device path (fhe_crt_decompose_towers == 0).
 * Digits and key must have the same baseBits, and the CALLER pairs them: fhe_bv_fast_keyswitch receives no baseBits for the digits in ws
 * (fhe_keyswitch_bv and fhe_bfv_eval_mult_relin_hps_bv cut them with the key's own, so they cannot mismatch).  What the call can see is
 * the workspace size: a key of a SMALLER digit size than the precompute's needs more towers than a workspace sized for the precompute
 * holds and is refused; a key of a LARGER digit size needs fewer, passes the check and sums towers that do not belong to it — NOT
 * detected, the result is then meaningless (all reads stay inside ws and the key).
 * out0 / out1 must not alias c or ws; c is only read.  Any number of host threads and streams may share one key.
 *   fhe_bv_precompute      = EvalKeySwitchPrecomputeCore (:251-259), a.CRTDecompose(r) (dcrtpoly-impl.h:230-285): c [batch][sizeQl][N] in
 *                            evalFormat (0: COEFFICIENT) -> digits [D_l][batch][sizeQl][N] EVALUATION, canonical residues, at the start of ws.
 *                            Digit-major: the `batch` towers of one digit are one contiguous wide tower.  (baseBits == 0: the reference copies an
 *                            EVALUATION input's limb i into digit i instead of transforming it, :237-251; the words are the same.)
 *   fhe_bv_fast_keyswitch  = EvalFastKeySwitchCore (:261-278) on the digits fhe_bv_precompute left in ws (hoisting: one precompute, many keys):
 *                            out_e[b][i] = sum_{d < D_l} digits[d][b][i] * key_e[d][i] mod q_i; accumulate != 0: out0 += ks0, out1 += ks1, the
 *                            tail of LeveledSHEBase::EvalMult(ct, ct, key) (base-leveledshe.cpp:207-211)
 *   fhe_keyswitch_bv       = KeySwitchCore (:245-249): the two above on c [batch][sizeQl][N] EVALUATION
 *   fhe_bfv_eval_mult_relin_hps_bv = LeveledSHEBase::EvalMult(ct, ct, key) (base-leveledshe.cpp:201-214) on BFV ciphertexts of the HPS family
 *                            with a BV key (HPSPOVERQLEVELED + BV is the reference's default BFV configuration): fhe_bfv_eval_mult_hps(outEval = 1)
 *                            with d0, d1 written to c0, c1 and d2 into ws, then fhe_keyswitch_bv(accumulate = 1) at numQ limbs.  sizeQl as for
 *                            fhe_bfv_eval_mult_hps; the plan's Q must be the context's leading limbs and the key built over them.  It is the
 *                            sizeQlRelin == numQ case of fhe_bfv_eval_mult_relin_hps_bv_leveled below. */
typedef struct fhe_bv_key fhe_bv_key;
/* keyB, keyA: HOST uint64_t[D_0][sizeQ][N] each, EVALUATION */
fhe_status fhe_bv_key_upload(fhe_ctx* ctx, uint32_t sizeQ, uint32_t baseBits, const uint64_t* keyB, const uint64_t* keyA, fhe_bv_key** out);
/* adopt key vectors that already live in device memory (not owned: destroy leaves them alone) */
fhe_status fhe_bv_key_wrap(fhe_ctx* ctx, uint32_t sizeQ, uint32_t baseBits, uint64_t* devKeyB, uint64_t* devKeyA, fhe_bv_key** out);
void       fhe_bv_key_destroy(fhe_bv_key* key);
/* device bytes the calls below need for `batch` towers at level sizeQl: the digits and one coefficient copy; 0 outside the device path */
size_t     fhe_bv_workspace_bytes(const fhe_ctx* ctx, uint32_t sizeQl, uint32_t baseBits, uint32_t batch);
fhe_status fhe_bv_precompute(fhe_ctx* ctx, const uint64_t* c, int evalFormat, uint32_t sizeQl, uint32_t baseBits, uint32_t batch,
                             void* ws, size_t wsBytes, void* stream);
fhe_status fhe_bv_fast_keyswitch(const fhe_bv_key* key, uint32_t sizeQl, uint32_t batch, uint64_t* out0, uint64_t* out1, int accumulate,
                                 const void* ws, size_t wsBytes, void* stream);
fhe_status fhe_keyswitch_bv(const fhe_bv_key* key, const uint64_t* c, uint32_t sizeQl, uint32_t batch, uint64_t* out0, uint64_t* out1,
                            int accumulate, void* ws, size_t wsBytes, void* stream);
size_t     fhe_bfv_eval_mult_relin_hps_bv_workspace_bytes(const fhe_hps* plan, uint32_t sizeQl, uint32_t baseBits, uint32_t batch);
fhe_status fhe_bfv_eval_mult_relin_hps_bv(fhe_hps* plan, const fhe_bv_key* key, const uint64_t* a0, const uint64_t* a1, const uint64_t* b0,
                                          const uint64_t* b1, uint64_t* c0, uint64_t* c1, uint32_t sizeQl, uint32_t batch,
                                          void* ws, size_t wsBytes, void* stream);

/* ---- rotations and leveled relinearisation on a BV key ------------------------------------------------------------
 * The rules of "BV key switching" carry over: after key upload a call builds nothing lazily, allocates nothing and does not synchronise (it can
 * be captured); an error enqueues nothing: a null argument, an even k ("Automorphism index not odd", as fhe_eval_fast_rotation), sizeQl out of
 * range for the technique, too small a workspace, a key of another context or another Q, FHE_ERR_UNSUPPORTED for a digit size outside the
 * device path.  Outputs must not alias inputs or ws unless stated otherwise.  k is the automorphism index (FindAutomorphismIndex is host
 * arithmetic: fhe_param_find_automorphism_index_2n_complex or the caller's own).
 * The inner product, the basis expansion, the additions and the automorphism of both elements are ONE kernel (the output-stage instance of bv_inner_product_kernel):
 * the two key-switch results never travel through device memory on their own.
 *
 * Any scheme (LeveledSHEBase; the tower has sizeQl limbs, the context's leading ones):
 *   fhe_bv_eval_fast_rotation  = LeveledSHEBase::EvalFastRotation (base-leveledshe.cpp:432-463) on the digits fhe_bv_precompute(c1) left in ws
 *                                (hoisting: one precompute, many keys): out0 = Auto_k(c0 + ks0), out1 = Auto_k(ks1).  ws is only read.
 *                                Digits and key must have the same baseBits and the CALLER pairs them, exactly as for fhe_bv_fast_keyswitch:
 *                                a key of a smaller digit size is refused by the workspace check, one of a larger digit size is NOT detected.
 *   fhe_bv_eval_automorphism   = LeveledSHEBase::EvalAutomorphism (base-leveledshe.cpp:381-422): fhe_bv_precompute(c1, EVALUATION) + the above.
 *
 * BFV, HPS family, with the fhe_hps plan.  The plan's Q must be the context's leading limbs and the key's sizeQ == numQ (checked as
 * fhe_bfv_eval_mult_relin_hps_bv checks them).  All towers are [batch][numQ][N].  sizeQl = l + 1 is the caller's numQ - levelsDropped for
 * the KEY SWITCH (FindLevelsToDrop(..., keySwitch) is host-side noise estimation and stays in pke): 1 ... numQ for HPSPOVERQLEVELED, numQ
 * only for HPS and HPSPOVERQ (the reference's condition, bfvrns-leveledshe.cpp:795, :859, :903, is false there: no scaling, no expansion).
 * Below numQ the element to be switched is scaled from Q down to Q_l (ScaleAndRound with QlQHatInvModqDivqModq(l) / ...Frac(l)), the key
 * switch runs at sizeQl limbs and both results return to Q (ExpandCRTBasisQlHat with QlHatModq(l)) before anything is added.
 * At sizeQl == numQ under HPSPOVERQLEVELED the reference still calls both members with the level-(numQ-1) tables; they are the identity
 * there (Q_l = Q: the integer table is the CRT reconstruction, every fraction is 0, QlHatModq is all ones) and are SKIPPED.  The words are
 * the reference's: tests/test_bv_rot_golden.py compares with cc->EvalRotate / EvalFastRotation / EvalMult on fresh ciphertexts.
 *   fhe_bfv_bv_workspace_bytes           covers every call below but the last (0: sizeQl or baseBits outside the device path)
 *   fhe_bfv_fast_rotation_precompute_bv  = LeveledSHEBFVRNS::EvalFastRotationPrecompute (bfvrns-leveledshe.cpp:782-813): c1 EVALUATION ->
 *                                COEFFICIENT -> ScaleAndRound Q -> Q_l -> digits at sizeQl limbs, EVALUATION, digit-major at the start of ws
 *                                (the layout of fhe_bv_precompute)
 *   fhe_bfv_eval_fast_rotation_bv        = LeveledSHEBFVRNS::EvalFastRotation (:815-882): inner product at sizeQl, ExpandCRTBasisQlHat to numQ,
 *                                += c0, the automorphism of both.  ws is only read; the caveat about pairing digits and key by baseBits
 *                                applies as above.
 *   fhe_bfv_eval_automorphism_bv         = LeveledSHEBFVRNS::EvalAutomorphism (:767-780): RelinearizeCore on two elements, both through the
 *                                automorphism = the two calls above
 *   fhe_bfv_relinearize_bv               = LeveledSHEBFVRNS::RelinearizeCore on three elements (:888-938): c_e = d_e + Expand(ks_e(d2)), EVALUATION.
 *                                inEval == 0: d0, d1, d2 are COEFFICIENT as EvalMultNoRelin leaves them (d2 goes straight into ScaleAndRound,
 *                                d0 / d1 are transformed once); otherwise EVALUATION.  c_e may be d_e (in place).
 *   fhe_bfv_eval_mult_relin_hps_bv_leveled = LeveledSHEBFVRNS::EvalMult(ct, ct, key) (:735-741): fhe_bfv_eval_mult_hps(outEval = 0) at sizeQlMult,
 *                                then fhe_bfv_relinearize_bv(inEval = 0) at sizeQlRelin.  Its own _workspace_bytes. */
fhe_status fhe_bv_eval_fast_rotation(const fhe_bv_key* key, const uint64_t* c0, uint32_t k, uint32_t sizeQl, uint32_t batch, uint64_t* out0,
                                     uint64_t* out1, const void* ws, size_t wsBytes, void* stream);
fhe_status fhe_bv_eval_automorphism(const fhe_bv_key* key, const uint64_t* c0, const uint64_t* c1, uint32_t k, uint32_t sizeQl, uint32_t batch,
                                    uint64_t* out0, uint64_t* out1, void* ws, size_t wsBytes, void* stream);
size_t     fhe_bfv_bv_workspace_bytes(const fhe_hps* plan, uint32_t sizeQl, uint32_t baseBits, uint32_t batch);
fhe_status fhe_bfv_fast_rotation_precompute_bv(fhe_hps* plan, const uint64_t* c1, uint32_t sizeQl, uint32_t baseBits, uint32_t batch, void* ws,
                                               size_t wsBytes, void* stream);
fhe_status fhe_bfv_eval_fast_rotation_bv(fhe_hps* plan, const fhe_bv_key* key, const uint64_t* c0, uint32_t k, uint32_t sizeQl, uint32_t batch,
                                         uint64_t* out0, uint64_t* out1, const void* ws, size_t wsBytes, void* stream);
fhe_status fhe_bfv_eval_automorphism_bv(fhe_hps* plan, const fhe_bv_key* key, const uint64_t* c0, const uint64_t* c1, uint32_t k,
                                        uint32_t sizeQl, uint32_t batch, uint64_t* out0, uint64_t* out1, void* ws, size_t wsBytes, void* stream);
fhe_status fhe_bfv_relinearize_bv(fhe_hps* plan, const fhe_bv_key* key, const uint64_t* d0, const uint64_t* d1, const uint64_t* d2, int inEval,
                                  uint32_t sizeQl, uint32_t batch, uint64_t* c0, uint64_t* c1, void* ws, size_t wsBytes, void* stream);
size_t     fhe_bfv_eval_mult_relin_hps_bv_leveled_workspace_bytes(const fhe_hps* plan, uint32_t sizeQlMult, uint32_t sizeQlRelin,
                                                                  uint32_t baseBits, uint32_t batch);
fhe_status fhe_bfv_eval_mult_relin_hps_bv_leveled(fhe_hps* plan, const fhe_bv_key* key, const uint64_t* a0, const uint64_t* a1,
                                                  const uint64_t* b0, const uint64_t* b1, uint64_t* c0, uint64_t* c1, uint32_t sizeQlMult,
                                                  uint32_t sizeQlRelin, uint32_t batch, void* ws, size_t wsBytes, void* stream);

/* ---- BV evaluation keys on the device ----------------------------------------------------------------------------------
 * KeySwitchBV::KeySwitchGenInternal in its three overloads (src/pke/lib/keyswitch/keyswitch-bv.cpp:49-225) for nKeys keys over the context's
 * leading sizeQ limbs with digit size baseBits.  A key has D_0 = fhe_crt_decompose_towers(ctx, NULL, sizeQ, baseBits) towers of sizeQ rows
 * per half, in the order of DCRTPolyImpl::CRTDecompose.  Tower d, window k of limb i, carries the old secret times 2^(baseBits * k) at row
 * i and nothing of it elsewhere (PolyImpl::PowersOfBase, src/core/include/lattice/poly-impl.h:559-571):
 *   factor[d][i] = 2^(baseBits * k) mod q_i for that one (d, i), 0 elsewhere; baseBits == 0: one tower per limb with factor 1.
 * fhe_bv_keygen_factors writes that table (HOST uint64_t[D_0][sizeQ], NULL = count only) and returns D_0; 0 where fhe_crt_decompose_towers
 * returns 0.  All towers EVALUATION, canonical residues in and out.  Window `key` of devKeyB / devKeyA (D_0 * sizeQ * N words each) is what
 * fhe_bv_key_wrap adopts.
 *
 * Secret-key form (:49-160; EvalMultKeyGen, EvalAutomorphismKeyGen of base-leveledshe.cpp:336-379, KeySwitchGen): ONE launch of the kernel of
 * fhe_keygen_combine with nParts = D_0 and the table above,
 *   devKeyB[key][d][i] = ns * e[key][d][i] - a[key][d][i] * pi_kNew[key](sNew[i]) + factor[d][i] * pi_kOld[key](sOld[i])   mod q_i.
 *   sNew, sOld DEVICE [sizeQ][N] (no extension, no plan object); a, e, devKeyB DEVICE [nKeys][D_0][sizeQ][N]; devKeyB == e is allowed;
 *   kNew / kOld as for fhe_ks_keygen_hybrid: EvalAutomorphismKeyGen for the index k: kNew = k^-1 mod 2N, kOld = 1; EvalMultKeyGen: (1, 1)
 *   with sOld = s * s.  The caller supplies a, so the third overload (:105-160, MultiKeySwitchGen's reuse of another key's a vector) is this
 *   same call with that key's a.
 * fhe_bv_keygen_blake2 is the seeded form, the composition of fhe_ks_keygen_hybrid_blake2 over nKeys * D_0 towers of sizeQ limbs: devKeyA =
 * the words of fhe_sample_uniform_blake2 from counterA as drawn, devKeyB = fhe_sample_gaussian_blake2 from counterE, fhe_ntt_fwd in place,
 * the combine in place.  No workspace; five launches on a two-pass ring.
 *
 * Public-key form (:162-225, what PREBase::ReKeyGen, src/pke/lib/schemebase/base-pre.cpp:42-45, calls to make a proxy re-encryption key):
 * ONE launch of keygen_pk_combine_kernel (csrc/keygen_kernels.h),
 *   devKeyB[key][d][i] = p0[key][i] * u[key][d][i] + ns * e0[key][d][i] + factor[d][i] * sOld[i]
 *   devKeyA[key][d][i] = p1[key][i] * u[key][d][i] + ns * e1[key][d][i]                                mod q_i.
 *   p0, p1     the NEW public key, DEVICE [sizeQ][N] each, or with pkPerKey != 0 [nKeys][sizeQ][N] (one delegator, many delegatees);
 *   u, e0, e1, devKeyB, devKeyA DEVICE [nKeys][D_0][sizeQ][N]; devKeyB == e0 and devKeyA == e1 are allowed (every word is read by the lane
 *   that overwrites it); every other overlap is refused.
 * fhe_bv_keygen_pk_blake2 is its seeded form, a composition; ws holds u, fhe_bv_keygen_workspace_bytes(ctx, sizeQ, baseBits, nKeys) bytes
 * (nKeys * D_0 * sizeQ * N words):
 *   u   = fhe_sample_ternary_blake2 (uDist = 0) or fhe_sample_gaussian_blake2 (uDist = 1: the reference's choice under SecretKeyDist ==
 *         GAUSSIAN, keyswitch-bv.cpp:196-197) over nKeys * D_0 towers from counterU, into ws;
 *   e0  = fhe_sample_gaussian_blake2 over nKeys * D_0 towers from counterE, into devKeyB;
 *   e1  = the same from the block after e0's last one, counterE + ceil(nKeys * D_0 * N / 512), into devKeyA (N >= 512: the Gaussian
 *         stream's very next word, so e0 ‖ e1 is one sampler call over twice the towers);
 *   fhe_ntt_fwd over all three blocks; fhe_bv_keygen_pk in place.
 * When devKeyA == devKeyB + nKeys * D_0 * sizeQ * N words and ws follows devKeyA likewise, that is one Gaussian call (N >= 512) and one
 * transform call: five launches on a two-pass ring.  Otherwise one call per block.  The words are the same function of (blake2 key,
 * counters) either way.
 * fhe_bv_keygen_counters: blake2 counters a seeded call consumes.  form 0 (secret key): *nAorU from counterA, *nE from counterE; form 1
 * (public key): *nAorU from counterU, *nE from counterE (e0 and e1 together).  The arithmetic of fhe_ks_keygen_counters.
 *
 * Errors, all detected before anything is enqueued, outputs untouched: those of fhe_keygen_combine (a null operand, nKeys == 0, an even
 * automorphism index or one >= 2N, ns == 0, a forbidden overlap), sizeQ outside [1, limbs of the context], FHE_ERR_UNSUPPORTED for a digit
 * size outside the device path (fhe_crt_decompose_towers == 0), sigma outside 1 < sigma < 300, an unknown uDist or form, a short workspace,
 * ws overlapping a key block, the public key or sOld.  The factor table and ns go through the context's table cache: the first call with
 * new ones uploads (not capturable), later calls are pure launches. */
uint32_t   fhe_bv_keygen_factors(const fhe_ctx* ctx, uint32_t sizeQ, uint32_t baseBits, uint64_t* factor);
fhe_status fhe_bv_keygen(fhe_ctx* ctx, uint32_t sizeQ, uint32_t baseBits, uint32_t nKeys, const uint32_t* kNew, const uint32_t* kOld,
                         const uint64_t* sNew, const uint64_t* sOld, uint64_t ns, const uint64_t* a, const uint64_t* e, uint64_t* devKeyB,
                         void* stream);
fhe_status fhe_bv_keygen_blake2(fhe_ctx* ctx, uint32_t sizeQ, uint32_t baseBits, uint32_t nKeys, const uint32_t* kNew, const uint32_t* kOld,
                                const uint64_t* sNew, const uint64_t* sOld, uint64_t ns, double sigma, const uint32_t key[16],
                                uint64_t counterA, uint64_t counterE, uint64_t* devKeyB, uint64_t* devKeyA, void* stream);
fhe_status fhe_bv_keygen_counters(const fhe_ctx* ctx, uint32_t sizeQ, uint32_t baseBits, uint32_t nKeys, int form, uint64_t* nAorU,
                                  uint64_t* nE);
fhe_status fhe_bv_keygen_pk(fhe_ctx* ctx, uint32_t sizeQ, uint32_t baseBits, uint32_t nKeys, const uint64_t* p0, const uint64_t* p1,
                            int pkPerKey, const uint64_t* sOld, uint64_t ns, const uint64_t* u, const uint64_t* e0, const uint64_t* e1,
                            uint64_t* devKeyB, uint64_t* devKeyA, void* stream);
size_t     fhe_bv_keygen_workspace_bytes(const fhe_ctx* ctx, uint32_t sizeQ, uint32_t baseBits, uint32_t nKeys);
fhe_status fhe_bv_keygen_pk_blake2(fhe_ctx* ctx, uint32_t sizeQ, uint32_t baseBits, uint32_t nKeys, const uint64_t* p0, const uint64_t* p1,
                                   int pkPerKey, const uint64_t* sOld, int uDist, uint64_t ns, double sigma, const uint32_t key[16],
                                   uint64_t counterU, uint64_t counterE, uint64_t* devKeyB, uint64_t* devKeyA, void* ws, size_t wsBytes,
                                   void* stream);

/* ---- BFV, HPS family, on HYBRID keys: rotations and relinearisation at dropped levels -----------------------------
 * The BFV block above with KeySwitchHYBRID (src/pke/lib/keyswitch/keyswitch-hybrid.cpp) in the middle.  Under HPSPOVERQLEVELED the reference
 * runs every relinearisation and rotation at sizeQl = l + 1 <= numQ limbs whatever the key-switch technique (bfvrns-leveledshe.cpp:767-938):
 * ScaleAndRound Q -> Q_l, the key switch at sizeQl limbs, ExpandCRTBasisQlHat back to Q; fhe_keyswitch_hybrid_acc on the output of
 * fhe_bfv_eval_mult_hps(outEval = 1) is that sequence at sizeQl == numQ only.
 * The plan pairs an fhe_hps plan with an fhe_ks_plan of the same context: the HPS plan's Q must be the context's leading limbs (as for the BV
 * block) and the key-switch plan's sizeQ == numQ, so the context holds Q, then P, then whatever R needs beyond them.  P and R need not be
 * disjoint (the reference draws both downwards from the last q_i, bfvrns-cryptoparameters.cpp:75, 135-139, rns-cryptoparameters.cpp:128-176):
 * a modulus common to both is ONE context limb that the P range and the R index list both name.  Both parents must outlive the plan.
 * fhe_bfv_hybrid_create builds every level of the key-switch plan the technique can use (1 ... numQ for HPSPOVERQLEVELED, numQ otherwise) and,
 * per level below numQ, the device table C'_i = [P^-1]_{q_i} * QlHatModq(l)[i] mod q_i: ApproxModDown's last product run with C' returns the
 * ModDown result already multiplied by QlHatModq(l), i.e. ExpandCRTBasisQlHat's low rows, at no cost.  After creation every call builds
 * nothing, allocates nothing and does not synchronise: it can be captured into a graph.
 * All towers are [batch][numQ][N].  sizeQl: 1 ... numQ for HPSPOVERQLEVELED, numQ only for HPS and HPSPOVERQ (the reference's condition,
 * :795, :859, :903, is false there).  At sizeQl == numQ scaling and expansion are the identity and are skipped, as in the BV block: the results
 * equal fhe_eval_fast_rotation / fhe_eval_automorphism / fhe_keyswitch_hybrid_acc word for word.  FindLevelsToDrop stays with the caller.
 * An error enqueues nothing and leaves the outputs untouched: a null argument, an even k ("Automorphism index not odd"), sizeQl outside the
 * technique's range, too small a workspace, a key of another fhe_ks_plan, rotation outputs that alias c0, c1 or ws.
 * The tail -- zero-extension from sizeQl to numQ rows, the addition(s) and the automorphism of both elements -- is ONE kernel
 * (bfv_hybrid_tail_kernel): a call below the top level is the launches of the key switch at sizeQl plus that one.
 *   fhe_bfv_hybrid_workspace_bytes            covers every call below but the last two (0: sizeQl outside the technique's range)
 *   fhe_bfv_fast_rotation_precompute_hybrid   = LeveledSHEBFVRNS::EvalFastRotationPrecompute (:782-813): c1 EVALUATION -> COEFFICIENT over numQ rows
 *                                -> ScaleAndRound Q -> Q_l into the key switch's coefficient buffer -> its EVALUATION copy (one transform of
 *                                sizeQl rows) and EvalKeySwitchPrecomputeCore (keyswitch-hybrid.cpp:314-379) from the coefficient buffer.  The
 *                                digits stay in ws for any number of fast rotations (hoisting); the complementary rows are kept lazy (< 16 q).
 *   fhe_bfv_eval_fast_rotation_hybrid         = LeveledSHEBFVRNS::EvalFastRotation (:815-882): EvalFastKeySwitchCore (keyswitch-hybrid.cpp:381-435) on
 *                                those digits, both results expanded, += c0, both through AutomorphismTransform(k).  c1 is the tower the
 *                                precompute saw; it is read only at sizeQl == numQ (the digits' own limbs are c1 itself there; below, the
 *                                scaled EVALUATION copy in ws is read).  The ModDown scratch in ws is overwritten by every call.
 *   fhe_bfv_eval_automorphism_hybrid          = LeveledSHEBFVRNS::EvalAutomorphism (:767-780) = the two calls above
 *   fhe_bfv_relinearize_hybrid                = LeveledSHEBFVRNS::RelinearizeCore on three elements (:888-938): c_e = d_e + Expand(ks_e(d2)),
 *                                EVALUATION.  inEval == 0: d0, d1, d2 are COEFFICIENT as EvalMultNoRelin leaves them (d2 goes straight into
 *                                ScaleAndRound, d0 / d1 are transformed once into c0 / c1); otherwise EVALUATION.  c_e may be d_e (in place).
 *   fhe_bfv_eval_mult_relin_hps_hybrid        = LeveledSHEBFVRNS::EvalMult(ct, ct, key) (:735-741): fhe_bfv_eval_mult_hps(outEval = 0) at sizeQlMult,
 *                                then fhe_bfv_relinearize_hybrid(inEval = 0) at sizeQlRelin.  Its own _workspace_bytes. */
typedef struct fhe_bfv_hybrid fhe_bfv_hybrid;
fhe_status fhe_bfv_hybrid_create(fhe_hps* hps, fhe_ks_plan* ks, fhe_bfv_hybrid** out);
void       fhe_bfv_hybrid_destroy(fhe_bfv_hybrid* plan);
size_t     fhe_bfv_hybrid_workspace_bytes(const fhe_bfv_hybrid* plan, uint32_t sizeQl, uint32_t batch);
fhe_status fhe_bfv_fast_rotation_precompute_hybrid(fhe_bfv_hybrid* plan, const uint64_t* c1, uint32_t sizeQl, uint32_t batch, void* ws,
                                                   size_t wsBytes, void* stream);
fhe_status fhe_bfv_eval_fast_rotation_hybrid(fhe_bfv_hybrid* plan, const fhe_ks_key* key, const uint64_t* c0, const uint64_t* c1, uint32_t k,
                                             uint32_t sizeQl, uint32_t batch, uint64_t* out0, uint64_t* out1, void* ws, size_t wsBytes,
                                             void* stream);
fhe_status fhe_bfv_eval_automorphism_hybrid(fhe_bfv_hybrid* plan, const fhe_ks_key* key, const uint64_t* c0, const uint64_t* c1, uint32_t k,
                                            uint32_t sizeQl, uint32_t batch, uint64_t* out0, uint64_t* out1, void* ws, size_t wsBytes,
                                            void* stream);
fhe_status fhe_bfv_relinearize_hybrid(fhe_bfv_hybrid* plan, const fhe_ks_key* key, const uint64_t* d0, const uint64_t* d1, const uint64_t* d2,
                                      int inEval, uint32_t sizeQl, uint32_t batch, uint64_t* c0, uint64_t* c1, void* ws, size_t wsBytes,
                                      void* stream);
size_t     fhe_bfv_eval_mult_relin_hps_hybrid_workspace_bytes(const fhe_bfv_hybrid* plan, uint32_t sizeQlMult, uint32_t sizeQlRelin,
                                                              uint32_t batch);
fhe_status fhe_bfv_eval_mult_relin_hps_hybrid(fhe_bfv_hybrid* plan, const fhe_ks_key* key, const uint64_t* a0, const uint64_t* a1,
                                              const uint64_t* b0, const uint64_t* b1, uint64_t* c0, uint64_t* c1, uint32_t sizeQlMult,
                                              uint32_t sizeQlRelin, uint32_t batch, void* ws, size_t wsBytes, void* stream);

/* ---- parity helper: whole-tower checksums ----------------------------------------------------------------
 * out[row] = { sum_i w_i, sum_i (2i + 1) * w_i } mod 2^64 over the row's N words, for every limb-row of x[rows][N] (rows = batch *
 * nLimbs; the second word depends on the ORDER of the words); out is DEVICE memory, uint64_t[rows][2].  One read of the batch: bench.py and the full-shape tests compare EVERY
 * tower of a resident batch with the oracle's words summed on the host, instead of sampling a few towers. */
fhe_status fhe_checksum(fhe_ctx* ctx, const uint64_t* x, uint32_t rows, uint64_t* out, void* stream);

/* Kernel launches issued by this library since it was loaded, by kernel: writes lines "<kernel> <launches>\n" (most frequent first)
 * into buf (at most cap bytes, NUL-terminated when cap > 0) and returns the length the full text needs; *total, when given, receives
 * the sum.  (Tuning aid: the launch count of one pke operation is the difference of two calls.)  The hand-over instances of the inverse
 * NTT passes are counted under their kernels' names and once more on lines "<kernel><HAND> <launches>", the two passes of
 * the forward 6 + 10 split at N = 2^16 likewise on lines "<kernel><SPLIT6> <launches>". */
size_t fhe_launch_stats(char* buf, size_t cap, uint64_t* total);

/* ---- host-side parameter helpers (no device work) -------------------------------------------------
 * Number theory the reference uses to pick moduli and roots, restated with 64-bit arithmetic so that a
 * caller can reproduce the reference's (N, q_i, psi_i) without linking OpenFHE:
 * FirstPrime/LastPrime/NextPrime/PreviousPrime (src/core/include/math/nbtheory-impl.h:329-393),
 * RootOfUnity = the minimum primitive m-th root (:183-231), the ILDCRTParams(order, depth, bits) chain
 * (src/core/include/lattice/hal/default/ildcrtparams.h:100-117) and the HYBRID auxiliary basis P of
 * CryptoParametersRNS::PrecomputeCRTTables (src/pke/lib/schemerns/rns-cryptoparameters.cpp:128-176, with the
 * CKKS prime step 2N, src/pke/lib/scheme/ckksrns/ckksrns-cryptoparameters.cpp:185-188). */
uint64_t   fhe_param_first_prime(uint32_t bits, uint64_t m);
uint64_t   fhe_param_last_prime(uint32_t bits, uint64_t m);
uint64_t   fhe_param_next_prime(uint64_t q, uint64_t m);
uint64_t   fhe_param_previous_prime(uint64_t q, uint64_t m);
uint64_t   fhe_param_root_of_unity(uint64_t m, uint64_t q);
fhe_status fhe_param_dcrt_chain(uint32_t order, uint32_t nLimbs, uint32_t bits, uint64_t* q, uint64_t* psi);
/* returns sizeP (0 on error); p/psiP need capacity >= 64 */
uint32_t   fhe_param_select_p(uint32_t logN, uint32_t sizeQ, const uint64_t* q, uint32_t numPartQ, uint32_t auxBits,
                              uint64_t* p, uint64_t* psiP);
/* FindAutomorphismIndex2nComplex (src/core/lib/math/nbtheory2.cpp:243-262): automorphism index 5^index mod m of a CKKS
 * rotation by `index` slots (m = 2N, a power of two); 0 on error */
uint32_t   fhe_param_find_automorphism_index_2n_complex(int32_t index, uint32_t m);

/* ---- f3: sampled towers on the device (optional) ------------------------------------
 * The sampling constructors of DCRTPolyImpl (dcrtpoly-impl.h:126-205) as device kernels: out[batch][nLimbs][N], COEFFICIENT format,
 *   fhe_sample_uniform   every word uniform in [0, q_limb)          DiscreteUniformGeneratorImpl::GenerateVector (discreteuniformgenerator.h:55-77)
 *   fhe_sample_gaussian  ONE integer per coefficient, stored modulo every limb (negative k as q - |k|): Peikert's inversion over the
 *                        reference's table (discretegaussiangenerator-impl.h:75-115), 1 < sigma < 300
 *   fhe_sample_ternary   ONE value of {-1, 0, 1} per coefficient, uniform (TernaryUniformGeneratorImpl::GenerateVector, h = 0)
 * Generator: Philox4x32-10 keyed by `seed`, counter = (element, draw, streamId) — NOT the reference's sequential Blake2 stream: the
 * distributions are the reference's, the words are not (the survey marks this row "gives up bit-parity with Blake2; keep optional");
 * the oracle restates the same construction word for word.  Give every sampled tower set its own streamId. */
fhe_status fhe_sample_uniform(fhe_ctx* ctx, uint64_t* out, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, uint64_t seed,
                              uint32_t streamId, void* stream);
fhe_status fhe_sample_gaussian(fhe_ctx* ctx, uint64_t* out, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, double sigma,
                               uint64_t seed, uint32_t streamId, void* stream);
fhe_status fhe_sample_ternary(fhe_ctx* ctx, uint64_t* out, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, uint64_t seed,
                              uint32_t streamId, void* stream);

/* ---- f3: the same samplers on the reference's cryptographic PRNG construction (csrc/blake2_kernels.h) --------------------------
 * default_prng::Blake2Engine (src/core/lib/utils/prng/blake2engine.cpp) draws 4 KiB per Generate(): blake2xb (blake2xb-ref.c) with
 * out = 4096 bytes, in = the engine's 64-bit counter (8 bytes little-endian), key = its 512-bit seed; then the counter is incremented.
 * These entries compute that stream on the device, every block and every BLAKE2b leaf of a block in parallel:
 *   fhe_blake2xb_stream   out[k * 1024 + i] = word i of the block of counter counter0 + k (k < nBlocks): the words
 *                         Blake2Engine(key, counter0) returns from successive calls.  out must be 8-byte aligned.
 * With R[i] = S[2i] | S[2i+1] << 32 the 64-bit words of that stream, the samplers (same output layout and format as fhe_sample_*):
 *   fhe_sample_uniform_blake2    element e = (t * nLimbs + l) * N + j:  (R[2e+1] * 2^64 + R[2e]) mod q_l.  Statistical distance from
 *                                uniform at most q / 2^128 < 2^-68 per coefficient (the reference rejects instead: exact)
 *   fhe_sample_gaussian_blake2   element e = t * N + j:  Peikert's inversion of s = (R[e] >> 11) * 2^-53 - 0.5 over the same table
 *                                (and the same per-sigma cache and 1 < sigma < 300 range) as fhe_sample_gaussian
 *   fhe_sample_ternary_blake2    element e = t * N + j:  mulhi(R[e], 3) - 1 (each outcome within 2^-64 of 1/3)
 * A call uses counters counter0 ... counter0 + ceil(words64 / 512) - 1, words64 = 2 * batch * nLimbs * N (uniform) or batch * N; give
 * every call its own counter range.  The key travels by value in the kernel arguments: it is never stored in a device buffer.
 * Against the Philox entries above: a cryptographic generator keyed by 512 bits (Philox4x32-10 is a statistical generator keyed by 64
 * bits: its words are not fit for keys that will ever be published), and the words are pinned on the reference's own blake2xb. */
fhe_status fhe_blake2xb_stream(fhe_ctx* ctx, uint32_t* out, uint64_t nBlocks, const uint32_t key[16], uint64_t counter0, void* stream);
fhe_status fhe_sample_uniform_blake2(fhe_ctx* ctx, uint64_t* out, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch,
                                     const uint32_t key[16], uint64_t counter0, void* stream);
fhe_status fhe_sample_gaussian_blake2(fhe_ctx* ctx, uint64_t* out, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, double sigma,
                                      const uint32_t key[16], uint64_t counter0, void* stream);
fhe_status fhe_sample_ternary_blake2(fhe_ctx* ctx, uint64_t* out, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch,
                                     const uint32_t key[16], uint64_t counter0, void* stream);

/* ---- measurement helper ----------------------------------------------------------------------------
 * Runs `iters` back-to-back launches of fwd (dir=0), inv (dir=1) or fwd+inv (dir=2) NTT on x — or of a single
 * pass kernel of a two-pass ring: 10/11 = column/row pass of the forward, 12/13 = row/column pass of the
 * inverse (timing only; the data is then not a transform) — and returns
 * the average wall time per launch-set in milliseconds measured with hipEvents on `stream`
 * (bench.py's roofline leg: torch.cuda.Event only sees torch's stream). */
fhe_status fhe_time_ntt(fhe_ctx* ctx, uint64_t* x, const uint32_t* limbIdx, uint32_t nLimbs, uint32_t batch, int dir,
                        int iters, void* stream, float* msPerIter);

#ifdef __cplusplus
}
#endif
#endif
