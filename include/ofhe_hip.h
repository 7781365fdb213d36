/*
 * ofhe_hip.h -- C ABI of the MI355X (gfx950) RNS polynomial backend.
 *
 * This is the drop-in boundary that replaces the UPMEM interception layer of
 * MpokiAbel/UPMEM--OpenFHE (src/core/include/pim/PimManager.h,
 * src/core/include/pim/PimData.h, src/core/pim/host/PimManager.cpp) and the
 * CPU hot loops it was meant to offload:
 *   - ChineseRemainderTransformFTTNat forward / inverse NTT
 *       (src/core/include/math/hal/intnat/transformnat-impl.h:575-705),
 *   - NativeVectorT element-wise ModMul/ModAdd/ModSub
 *       (src/core/include/math/hal/intnat/mubintvecnat.h:426-432,501-513;
 *        src/core/lib/math/hal/intnat/mubintvecnat.cpp:245-367),
 *   - DCRTPolyImpl::ApproxSwitchCRTBasis / ApproxModUp / ApproxModDown
 *       (src/core/include/lattice/hal/default/dcrtpoly-impl.h:1034-1175),
 *   - the HYBRID key-switching core built on them
 *       (src/pke/lib/keyswitch/keyswitch-hybrid.cpp:325-482),
 *   - NativeVectorT::SwitchModulus and PolyImpl::AutomorphismTransform
 *       (mubintvecnat.cpp:111-136, poly-impl.h:312-365),
 *   - the BFV (HPS) multiplication's SwitchCRTBasis / ExpandCRTBasis /
 *     FastExpandCRTBasisPloverQ / ScaleAndRound
 *       (dcrtpoly-impl.h:1178-1230, 1311-1358, 1413-1466, 1876-1955),
 *   - the BFV (BEHZ) multiplication's FastBaseConvqToBskMontgomery /
 *     FastRNSFloorq / FastBaseConvSK
 *       (dcrtpoly-impl.h:2050-2208, 2212-2271, 2309-2411).
 *
 * Conventions
 *   - Plain C, no exceptions cross the ABI. Every entry point returns an int
 *     status (OFHE_OK = 0); ofhe_hip_last_error() gives a thread-local message.
 *     The C++ adapter (upmem--openfhe_amd/host/ofhe_dcrt.hpp) turns non-zero
 *     into lbcrypto-style math_error exceptions, as OPENFHE_THROW does.
 *   - Polynomial data is uint64_t residues laid out [batch][tower][N],
 *     contiguous, in DEVICE memory, unless a function says otherwise.
 *     Inputs must be canonical residues in [0, q_t); outputs are canonical.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *     Calls are asynchronous on that stream; nothing here synchronises.
 *   - The caller owns all data buffers; the library owns contexts, plans,
 *     twiddle tables and scratch.
 */
#ifndef OFHE_HIP_H
#define OFHE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    OFHE_OK = 0,
    OFHE_ERR_ARG = 1,     /* invalid argument (size, modulus, root ...)     */
    OFHE_ERR_HIP = 2,     /* a HIP runtime call failed                       */
    OFHE_ERR_NOMEM = 3,   /* device or host allocation failed                */
    OFHE_ERR_STATE = 4    /* use of a destroyed / uninitialised object       */
};

typedef struct ofhe_ctx_s* ofhe_ctx_t;   /* one per device (PimManager::getPim) */
typedef struct ofhe_plan_s* ofhe_plan_t; /* NTT plan: (N, towers, q[], psi[])  */

/* Thread-local description of the last failure in this thread: the message
 * OPENFHE_THROW(math_error, msg) carries (src/core/include/utils/exception.h:162);
 * the fork's PIM layer instead aborts in DPU_ASSERT (PimManager.cpp:5-37). */
const char* ofhe_hip_last_error(void);

/* Library version string ("ofhe-hip <ver> gfx950"); no reference counterpart
 * (the fork's kernel binaries are located by path, pim/kernel.h:4-8). */
const char* ofhe_hip_version(void);

/* ---- device context: replaces PimManager::getPim(nr_dpus, profile),
 *      PimManager.h:23-29 (lazily created singleton), and its allocator /
 *      transfers (PimManager.cpp:5-93). --------------------------------- */
int ofhe_hip_device_count(int* count);
int ofhe_hip_init(int device, ofhe_ctx_t* ctx);
int ofhe_hip_finalize(ofhe_ctx_t ctx);
/* PimManager::allocate / deallocate (PimManager.h:83-85) */
int ofhe_hip_alloc(ofhe_ctx_t ctx, size_t bytes, void** dptr);
int ofhe_hip_free(ofhe_ctx_t ctx, void* dptr);
/* Stream-ordered variants (hipMallocAsync / hipFreeAsync): the block is
 * released only after the work already queued on `stream` has finished, so a
 * buffer can be dropped right after the asynchronous calls that use it.
 * The blocks come from the context's own pool: ofhe_hip_finalize returns
 * OFHE_ERR_STATE (and leaves the context usable) while any block obtained
 * here has not been passed to ofhe_hip_free_async. */
int ofhe_hip_alloc_async(ofhe_ctx_t ctx, size_t bytes, void** dptr, void* stream);
int ofhe_hip_free_async(ofhe_ctx_t ctx, void* dptr, void* stream);
/* Pinned (page-locked) host memory for the staging buffers of a host-buffer
 * integration: towers gathered from the reference's per-tower vectors
 * (dcrtpoly.h:421, poly.h:368) into one buffer that DMA can read directly,
 * so host <-> device copies run at the PCIe rate and overlap compute. */
int ofhe_hip_host_alloc(ofhe_ctx_t ctx, size_t bytes, void** hptr);
int ofhe_hip_host_free(ofhe_ctx_t ctx, void* hptr);
/* dst[0..bytes) = 0 on the stream (a zero DCRTPoly, dcrtpoly.h initializing ctor). */
int ofhe_hip_zero(ofhe_ctx_t ctx, void* dst, size_t bytes, void* stream);
/* PimManager::copy_to_pim (scatter, type 0) / copy_from_pim (PimManager.h:44-54) */
int ofhe_hip_copy_to_device(ofhe_ctx_t ctx, void* dst, const void* src, size_t bytes, void* stream);
int ofhe_hip_copy_to_host(ofhe_ctx_t ctx, void* dst, const void* src, size_t bytes, void* stream);
/* device-to-device copy (poly copy constructor, poly.h:368 owns its vector) */
int ofhe_hip_copy_device(ofhe_ctx_t ctx, void* dst, const void* src, size_t bytes, void* stream);
/* PimManager::start_kernel is synchronous (PimManager.h:68); here explicit. */
int ofhe_hip_sync(ofhe_ctx_t ctx, void* stream);
/* A completion marker on one stream.  The reference's copies block until the
 * transfer is done (PimManager::copy_to_pim / copy_from_pim, PimManager.cpp:5-54);
 * with an event the host waits for one staged DMA only, not for every launch
 * queued on the stream (the C++ adapter's pinned staging, ofhe_dcrt.hpp). */
typedef struct ofhe_event_s* ofhe_event_t;
int ofhe_hip_event_create(ofhe_ctx_t ctx, ofhe_event_t* event);
int ofhe_hip_event_record(ofhe_event_t event, void* stream); /* marks the stream's work so far */
int ofhe_hip_event_sync(ofhe_event_t event);                 /* waits for the marked work     */
int ofhe_hip_event_destroy(ofhe_event_t event);
/* Return all but keep_bytes of the context's stream-ordered pool (scratch and
 * ofhe_hip_alloc_async blocks kept across synchronisations) to the device; the
 * reference frees DPU memory per call (PimManager::deallocate, PimManager.h:83-85). */
int ofhe_hip_trim(ofhe_ctx_t ctx, size_t keep_bytes);

/* ---- NTT plan: replaces ChineseRemainderTransformFTTNat::PreCompute and
 *      its static twiddle maps (transformnat-impl.h:708-763,
 *      transformnat.h:352-368).  N = 2^log_n, 1 <= log_n <= 17; q[t] prime,
 *      q[t] = 1 mod 2N, q[t] < 2^60; psi[t] a primitive 2N-th root of unity
 *      mod q[t] (OpenFHE uses the smallest one, nbtheory-impl.h:183-231).
 *      Tables are built on the host once and kept resident on the device. */
int ofhe_hip_plan_create(ofhe_ctx_t ctx, uint32_t log_n, uint32_t towers, const uint64_t* q,
                         const uint64_t* psi, ofhe_plan_t* plan);
/* Kernel choices of a plan, fixed at creation (ofhe_hip_plan_create_ex).  A
 * zero-initialised struct (or NULL) is exactly ofhe_hip_plan_create's choice.
 * Every setting gives the same canonical results; they let tests reach every
 * kernel and A/B timings compare them in one process.  No reference
 * counterpart (the reference has one CPU loop, transformnat-impl.h:300-354). */
enum {
    OFHE_SPLIT_AUTO = 0, /* log_n = 16: OFHE_SPLIT_8_8; other log_n > 12: OFHE_SPLIT_COLS  */
    OFHE_SPLIT_COLS = 1, /* log_n - 12 column stages (k_cols) + a 12-stage block pass     */
    OFHE_SPLIT_8_8 = 2,  /* log_n = 16 only: 8 column stages (k_tcols) + 8-stage block    */
    OFHE_SPLIT_9_8 = 3,  /* log_n = 17 only: 9 column stages (k_tcols9) + 8-stage block   */
    OFHE_SPLIT_8_9 = 4   /* log_n = 17 only: 8 column stages (k_tcols) + 9-stage block    */
};
typedef struct ofhe_plan_options {
    uint32_t split;          /* OFHE_SPLIT_*; log_n <= 12 plans accept only AUTO          */
    uint32_t generic_moduli; /* 1: the generic-modulus kernels even when every q is a
                                special prime 2^L - d (the default picks the faster ones) */
} ofhe_plan_options;
int ofhe_hip_plan_create_ex(ofhe_ctx_t ctx, uint32_t log_n, uint32_t towers, const uint64_t* q,
                            const uint64_t* psi, const ofhe_plan_options* options, ofhe_plan_t* plan);
int ofhe_hip_plan_destroy(ofhe_plan_t plan);
/* Performance knob for ofhe_hip_ntt_mul_intt at log_n > 12: process the batch
 * in chunks of `chunk_batch` entries (0 = whole batch in one pass) and, with
 * streams = 2, alternate the chunks over two internal streams forked from and
 * joined back into the caller's stream.  Results are identical for any
 * setting; only speed changes.  Set it while no other thread launches with
 * the same plan: the launches read the setting without taking the plan's lock. */
int ofhe_hip_plan_tune(ofhe_plan_t plan, uint32_t chunk_batch, uint32_t streams);
/* Copy the plan's host-side tables out (debug / parity tests): any pointer
 * may be NULL.  tab*: [towers][N] in OpenFHE order (Table[rev(i)] = psi^i). */
int ofhe_hip_plan_tables(ofhe_plan_t plan, uint64_t* tab, uint64_t* tab_pre, uint64_t* itab,
                         uint64_t* itab_pre, uint64_t* ninv);

/* Forward negacyclic NTT in place, natural order -> bit-reversed evaluation
 * order: ChineseRemainderTransformFTT<NativeVector>::ForwardTransformToBitReverseInPlace
 * (transformnat-impl.h:575-602 -> 300-354), for every (batch, tower). */
int ofhe_hip_ntt_fwd(ofhe_plan_t plan, uint64_t* data, uint32_t batch, void* stream);
/* Inverse NTT in place, bit-reversed -> natural, n^-1 applied:
 * InverseTransformFromBitReverseInPlace (transformnat-impl.h:637-666 -> 492-552). */
int ofhe_hip_ntt_inv(ofhe_plan_t plan, uint64_t* data, uint32_t batch, void* stream);

/* The same transforms on plan towers [t0, t0 + count) of strided data, in or
 * out of place: src / dst point at tower t0 of batch entry 0 and advance by
 * src_stride / dst_stride words (>= count * N) per batch entry.  This is the
 * per-tower SwitchFormat the DCRTPoly loops issue on sub-bases (e.g. the P
 * towers of a Q|P polynomial in ApproxModUp, dcrtpoly-impl.h:1112-1116). */
int ofhe_hip_ntt_fwd_range(ofhe_plan_t plan, uint32_t t0, uint32_t count, const uint64_t* src,
                           uint64_t* dst, uint64_t src_stride, uint64_t dst_stride, uint32_t batch,
                           void* stream);
int ofhe_hip_ntt_inv_range(ofhe_plan_t plan, uint32_t t0, uint32_t count, const uint64_t* src,
                           uint64_t* dst, uint64_t src_stride, uint64_t dst_stride, uint32_t batch,
                           void* stream);

/* LeveledSHEBase::EvalMultCore for two 2-element ciphertexts
 * (base-leveledshe.cpp:667-672), evaluation form, per (batch, tower) of plan:
 *   out2 = c1 * d1,  out1 = c1 * d0 + c0 * d1,  out0 = d0 * c0
 * (DCRTPoly operator* / += : Barrett ModMul, ModAdd), one pass over HBM.
 * Outputs must not alias inputs. */
int ofhe_hip_eval_mult_core(ofhe_plan_t plan, const uint64_t* c0, const uint64_t* c1, const uint64_t* d0,
                            const uint64_t* d1, uint64_t* out0, uint64_t* out1, uint64_t* out2, uint32_t batch,
                            void* stream);
/* c = a (op) b element-wise per tower: NativeVectorT::ModMul (Barrett,
 * mubintvecnat.cpp:353-367 / .h:501-513), ModAdd (.cpp:245-264 / .h:426-432),
 * ModSub (.cpp:301-307).  c may alias a or b (the *Eq forms). */
int ofhe_hip_modmul_vv(ofhe_plan_t plan, const uint64_t* a, const uint64_t* b, uint64_t* c,
                       uint32_t batch, void* stream);
int ofhe_hip_modadd_vv(ofhe_plan_t plan, const uint64_t* a, const uint64_t* b, uint64_t* c,
                       uint32_t batch, void* stream);
int ofhe_hip_modsub_vv(ofhe_plan_t plan, const uint64_t* a, const uint64_t* b, uint64_t* c,
                       uint32_t batch, void* stream);
/* Vector (.) scalar with one scalar per tower (host array s[towers], any
 * uint64_t; each is reduced mod q[t] first, as the reference does).  The
 * scalars travel in the kernel arguments: nothing is staged, nothing
 * synchronises, and c may alias a.  They replace the DPU SCALAR / SCALAR_EQ
 * kernels (src/core/pim/dpu/element-wise/add-mod.c:23-100, sub-mod.c,
 * mult-mod.c) and the CPU loops of
 *   c = a * s mod q: NativeVectorT::ModMul(Eq)(const IntegerType&)
 *                    (mubintvecnat.cpp:310-332, Shoup), DCRTPoly::Times(Integer);
 *   c = a + s mod q: NativeVectorT::ModAdd(Eq)(const IntegerType&)
 *                    (mubintvecnat.cpp:198-219), DCRTPoly::Plus(Integer) in
 *                    evaluation form (dcrtpoly.h:162-163, poly-impl.h:213-220);
 *   c = a - s mod q: NativeVectorT::ModSub(Eq)(const IntegerType&)
 *                    (mubintvecnat.cpp:267-288), DCRTPoly::Minus(Integer)
 *                    (dcrtpoly.h:182-183, poly-impl.h:223-227). */
int ofhe_hip_modmul_scalar(ofhe_plan_t plan, const uint64_t* a, const uint64_t* s, uint64_t* c,
                           uint32_t batch, void* stream);
int ofhe_hip_modadd_scalar(ofhe_plan_t plan, const uint64_t* a, const uint64_t* s, uint64_t* c,
                           uint32_t batch, void* stream);
int ofhe_hip_modsub_scalar(ofhe_plan_t plan, const uint64_t* a, const uint64_t* s, uint64_t* c,
                           uint32_t batch, void* stream);
/* c[index] = a[index] + s[t] mod q[t] in every (batch, tower); no other word is
 * written (use in place, or copy a to c first): NativeVectorT::ModAddAtIndex(Eq)
 * (mubintvecnat.cpp:221-231), i.e. PolyImpl / DCRTPoly::Plus(Integer) in
 * coefficient form (poly-impl.h:213-220: a constant added to coefficient 0). */
int ofhe_hip_modadd_scalar_at(ofhe_plan_t plan, const uint64_t* a, uint64_t index, const uint64_t* s,
                              uint64_t* c, uint32_t batch, void* stream);

/* Synthetic inputs for benchmarks and tests; no reference
 * counterpart (the benchmark draws uniform vectors on the host,
 * poly-benchmark-16k.cpp:45-70): dst[b][t][i] = splitmix64 draw i + 1 of the stream seeded
 * 0x5EED ^ ((batch_offset + b) << 20) ^ (t << 8) ^ seed, mod q[t] -- what the
 * CPU oracle's generator (oracle_fill_uniform) produces for the same seed. */
int ofhe_hip_fill_uniform(ofhe_plan_t plan, uint64_t* dst, uint32_t batch, uint32_t batch_offset, uint64_t seed,
                          void* stream);

/* The metric pipeline, per (batch, tower): c = INTT(NTT(a) (.) b), a in
 * coefficient form, b in evaluation form, c in coefficient form.  Equals
 * SwitchFormat -> Times -> SwitchFormat on DCRTPoly (dcrtpoly-impl.h:2518-2524,
 * dcrtpoly.h:185-200).  c may alias a. */
int ofhe_hip_ntt_mul_intt(ofhe_plan_t plan, const uint64_t* a, const uint64_t* b, uint64_t* c,
                          uint32_t batch, void* stream);

/* One launch of the pipeline above, for per-kernel timing (bench.py); no
 * reference counterpart (the reference's loop is per tower, dcrtpoly-impl.h:2518-2524):
 * stage 0 = forward column pass (a -> c), 1 = block pass (forward tail,
 * Hadamard with b, inverse head; reads c, or a when log_n <= 12),
 * 2 = inverse column pass (c -> c).  Stages 0 and 2 are no-ops for
 * log_n <= 12.  Running 0, 1, 2 in order equals ofhe_hip_ntt_mul_intt. */
int ofhe_hip_ntt_mul_intt_stage(ofhe_plan_t plan, int stage, const uint64_t* a, const uint64_t* b,
                                uint64_t* c, uint32_t batch, void* stream);

/* ---- RNS base conversion: DCRTPolyImpl::ApproxSwitchCRTBasis
 *      (dcrtpoly-impl.h:1034-1063, Mul128/BarrettUint128ModUint64 in
 *      utils/utilities-int.h:47-103).  x: [batch][size_q][N] coefficient form
 *      mod q[i]; out: [batch][size_p][N] mod p[j].  Precomputations as the pke
 *      layer builds them (pke/lib/schemerns/rns-cryptoparameters.cpp:273-337):
 *      qhat_inv_modq[i] = (Q/q_i)^-1 mod q_i, qhat_modp[i*size_p+j] = (Q/q_i) mod p_j,
 *      all host arrays.  Barrett constants are derived internally. */
typedef struct ofhe_bconv_s* ofhe_bconv_t;
int ofhe_hip_bconv_create(ofhe_ctx_t ctx, uint32_t log_n, uint32_t size_q, uint32_t size_p,
                          const uint64_t* q, const uint64_t* p, const uint64_t* qhat_inv_modq,
                          const uint64_t* qhat_modp, ofhe_bconv_t* bconv);
/* Kernel choices of a converter (ofhe_hip_bconv_create_ex; zero = the default
 * of ofhe_hip_bconv_create).  Same results for every setting. */
enum {
    OFHE_BCONV_KERNEL_AUTO = 0, /* matrix cores (<= 64 sources, N >= 32), else LIMB / WIDE */
    OFHE_BCONV_KERNEL_LIMB = 1, /* 30-bit limb sums on the VALU (<= 16 sources)            */
    OFHE_BCONV_KERNEL_WIDE = 2  /* 128-bit sums on the VALU, any number of sources         */
};
typedef struct ofhe_bconv_options {
    uint32_t kernel;        /* OFHE_BCONV_KERNEL_*; LIMB / WIDE hold on every path that
                               uses the converter (ApproxModUp / ApproxModDown at 2^17
                               then run conversion and column pass as two kernels)     */
    uint32_t separate_cols; /* 1: in ofhe_hip_approx_mod_up / _down at N = 2^17, the
                               conversion and the targets' forward column pass as two
                               kernels instead of the fused k_bconv_cols                  */
} ofhe_bconv_options;
int ofhe_hip_bconv_create_ex(ofhe_ctx_t ctx, uint32_t log_n, uint32_t size_q, uint32_t size_p,
                             const uint64_t* q, const uint64_t* p, const uint64_t* qhat_inv_modq,
                             const uint64_t* qhat_modp, const ofhe_bconv_options* options, ofhe_bconv_t* bconv);
int ofhe_hip_bconv_destroy(ofhe_bconv_t bconv);
int ofhe_hip_approx_switch_crt_basis(ofhe_bconv_t bconv, const uint64_t* x, uint64_t* out,
                                     uint32_t batch, void* stream);

/* DCRTPolyImpl::ApproxModUp (dcrtpoly-impl.h:1085-1131).  x: [batch][Q][N]
 * under plan_q, in evaluation form when eval_form != 0 (else coefficient
 * form); out: [batch][Q+P][N] in evaluation form, towers Q of plan_q then P
 * of plan_p.  q_to_p converts plan_q's basis to plan_p's.  out must not
 * overlap x. */
int ofhe_hip_approx_mod_up(ofhe_plan_t plan_q, ofhe_plan_t plan_p, ofhe_bconv_t q_to_p, int eval_form,
                           const uint64_t* x, uint64_t* out, uint32_t batch, void* stream);
/* DCRTPolyImpl::ApproxModDown (dcrtpoly-impl.h:1134-1175).  x: [batch][Q+P][N]
 * evaluation form; out: [batch][Q][N] evaluation form.  p_to_q converts
 * plan_p's basis to plan_q's (PHatInvModp, PHatModq); p_inv_modq: host
 * [Q] = P^-1 mod q_i.  t = 0 for CKKS / BFV; t > 0 (BGV) multiplies the P part
 * by t^-1 mod p_j and the switched part by t (t_inv_modp derived here).
 * The small constant tables are built and uploaded on the first call with a
 * given (t, p_inv_modq) and cached in p_to_q; no call synchronises. */
int ofhe_hip_approx_mod_down(ofhe_plan_t plan_q, ofhe_plan_t plan_p, ofhe_bconv_t p_to_q,
                             const uint64_t* p_inv_modq, uint64_t t, const uint64_t* x, uint64_t* out,
                             uint32_t batch, void* stream);

/* ---- HYBRID key switching: KeySwitchHYBRID (pke/lib/keyswitch/
 *      keyswitch-hybrid.cpp:325-482) with the CRT tables of
 *      CryptoParametersRNS::PrecomputeCRTTables (pke/lib/schemerns/
 *      rns-cryptoparameters.cpp:72-345) built internally from the moduli.
 *      Q = q[0..size_q) (element params), P = p[0..size_p) (GetParamsP()),
 *      num_part_q = dnum digits of alpha = ceil(size_q / num_part_q) towers.
 *      Every call works at level size_ql (1 <= size_ql <= size_q): the
 *      ciphertext has towers q[0..size_ql).  Evaluation keys are laid out
 *      [num_part_q][size_q + size_p][N] (EvalKey b / a vectors over QP),
 *      shared by the batch. ---- */
typedef struct ofhe_ks_s* ofhe_ks_t;
int ofhe_hip_ks_create(ofhe_ctx_t ctx, uint32_t log_n, uint32_t size_q, const uint64_t* q,
                       const uint64_t* psi_q, uint32_t size_p, const uint64_t* p, const uint64_t* psi_p,
                       uint32_t num_part_q, ofhe_ks_t* ks);
/* Engine choices (ofhe_hip_ks_create_ex; zero / NULL = ofhe_hip_ks_create's
 * defaults).  Same results for every setting. */
typedef struct ofhe_ks_options {
    ofhe_plan_options plan;   /* the engine's Q|P plan                                       */
    uint32_t separate_cols;   /* 1: base conversion and forward column pass as two kernels   */
    uint32_t separate_icol;   /* 1: the digits' inverse column pass as its own kernel        */
    uint32_t chunk;           /* ciphertexts per ModUp chunk (0 = the whole batch)           */
    uint32_t single_stream;   /* 1: every digit on the caller's stream (no side streams)     */
} ofhe_ks_options;
int ofhe_hip_ks_create_ex(ofhe_ctx_t ctx, uint32_t log_n, uint32_t size_q, const uint64_t* q,
                          const uint64_t* psi_q, uint32_t size_p, const uint64_t* p, const uint64_t* psi_p,
                          uint32_t num_part_q, const ofhe_ks_options* options, ofhe_ks_t* ks);
int ofhe_hip_ks_destroy(ofhe_ks_t ks);
/* alpha (towers per digit) and beta (digits at level size_ql, capped at
 * num_part_q), keyswitch-hybrid.cpp:341-345. */
int ofhe_hip_ks_digits(ofhe_ks_t ks, uint32_t size_ql, uint32_t* alpha, uint32_t* beta);
/* EvalKeySwitchPrecomputeCore (keyswitch-hybrid.cpp:330-412): c [batch][size_ql][N]
 * evaluation form -> digits [batch][beta][size_ql + size_p][N] evaluation form. */
int ofhe_hip_ks_precompute(ofhe_ks_t ks, uint32_t size_ql, const uint64_t* c, uint64_t* digits,
                           uint32_t batch, void* stream);
/* EvalFastKeySwitchCoreExt (keyswitch-hybrid.cpp:438-482): ct0 = sum_j digits_j * b_j,
 * ct1 = sum_j digits_j * a_j over Ql|P; ct0, ct1: [batch][size_ql + size_p][N]. */
int ofhe_hip_ks_fast_core_ext(ofhe_ks_t ks, uint32_t size_ql, const uint64_t* digits,
                              const uint64_t* key_b, const uint64_t* key_a, uint64_t* ct0, uint64_t* ct1,
                              uint32_t batch, void* stream);
/* ApproxModDown with the key-switching tables (keyswitch-hybrid.cpp:423-435):
 * x [batch][size_ql + size_p][N] -> out [batch][size_ql][N], evaluation form. */
int ofhe_hip_ks_mod_down(ofhe_ks_t ks, uint32_t size_ql, const uint64_t* x, uint64_t* out, uint64_t t,
                         uint32_t batch, void* stream);
/* KeySwitchCore = EvalFastKeySwitchCore(EvalKeySwitchPrecomputeCore(c))
 * (keyswitch-hybrid.cpp:325-328, 414-436): out0, out1 [batch][size_ql][N]. */
int ofhe_hip_ks_core(ofhe_ks_t ks, uint32_t size_ql, const uint64_t* c, const uint64_t* key_b,
                     const uint64_t* key_a, uint64_t* out0, uint64_t* out1, uint64_t t, uint32_t batch,
                     void* stream);
/* Hoisted rotations: nrot rotations of one digit set, the digits of
 * ofhe_hip_ks_precompute ([batch][beta][size_ql + size_p][N]) decomposed once.
 * auto_index[r] (host array) is rotation r's automorphism index, any odd value,
 * taken mod 2N; key_b[r] / key_a[r] (host arrays of device pointers) are its
 * evaluation key, laid out as for ofhe_hip_ks_fast_core_ext.  The pointers and
 * indices travel in kernel arguments: nothing is staged and nothing
 * synchronises.  Canonical outputs; out0 must differ from out1.
 *
 * LeveledSHECKKSRNS::EvalFastRotationExt (ckksrns-leveledshe.cpp:402-457), over Ql|P:
 *   out0[r][b] = sigma_k(sum_j digits_j * b_j^(r) + c0[b] * (P mod q_i) on the Q towers)
 *   out1[r][b] = sigma_k(sum_j digits_j * a_j^(r))
 * c0: [batch][size_ql][N] evaluation form, or NULL for addFirst = false;
 * out0, out1: [nrot][batch][size_ql + size_p][N]. */
int ofhe_hip_ks_fast_rotation_ext(ofhe_ks_t ks, uint32_t size_ql, const uint64_t* digits, const uint64_t* c0,
                                  uint32_t nrot, const uint32_t* auto_index, const uint64_t* const* key_b,
                                  const uint64_t* const* key_a, uint64_t* out0, uint64_t* out1, uint32_t batch,
                                  void* stream);
/* LeveledSHEBase::EvalFastRotation (base-leveledshe.cpp:471-513), in the
 * reference's order (ModDown, += c0, automorphism):
 *   out0[r][b] = sigma_k(ModDown(sum_j digits_j * b_j^(r)) + c0[b])
 *   out1[r][b] = sigma_k(ModDown(sum_j digits_j * a_j^(r)))
 * with t as in ofhe_hip_ks_mod_down; c0 is required;
 * out0, out1: [nrot][batch][size_ql][N]. */
int ofhe_hip_ks_fast_rotation(ofhe_ks_t ks, uint32_t size_ql, const uint64_t* digits, const uint64_t* c0,
                              uint32_t nrot, const uint32_t* auto_index, const uint64_t* const* key_b,
                              const uint64_t* const* key_a, uint64_t* out0, uint64_t* out1, uint64_t t,
                              uint32_t batch, void* stream);

/* ---- BSGS linear transform ("double hoisting") ----
 * FHECKKSRNS::EvalLinearTransform (ckksrns-fhe.cpp:1484-1555), every level of
 * EvalCoeffsToSlots / EvalSlotsToCoeffs (1636-1698 and the remainder blocks)
 * and the same loops of ckksrns-schemeswitching.cpp:889-918, 994-1024: baby
 * steps rotated into Ql|P, multiplied by plaintext diagonals and summed there,
 * each giant step's sum switched down, rotated under the giant key and summed
 * in Ql|P again, one final KeySwitchDown.  The three stage calls are the
 * pieces the fused call runs; all outputs are canonical, nothing synchronises,
 * and outputs must not alias inputs or each other. */
/* KeySwitchHYBRID::KeySwitchExt (keyswitch-hybrid.cpp:231-256) on one element:
 * c [batch][size_ql][N] -> out [batch][size_ql + size_p][N], c * (P mod q_i) on
 * the Q towers and zero on the P towers. */
int ofhe_hip_ks_ext(ofhe_ks_t ks, uint32_t size_ql, const uint64_t* c, uint64_t* out, uint32_t batch,
                    void* stream);
/* EvalMultExt / EvalAddExtInPlace (ckksrns-fhe.cpp:2373-2396) over the inner
 * loop of 1520-1526:  out_e[j] = sum_i x_e[i] * diag[j * nterm + i],  e = 0, 1,
 * j < nsum, over Ql|P.  x0, x1: [nterm][batch][size_ql + size_p][N] with
 * x_stride words between terms; diagonal d is (size_ql + size_p) towers of N in
 * evaluation form at diag + d * diag_stride, shared by the batch entries;
 * present (host bytes, [nsum * nterm], or NULL: all present) marks the
 * diagonals that exist -- an absent one is skipped and never read;
 * out0, out1: [nsum][batch][size_ql + size_p][N]. */
int ofhe_hip_ks_mult_ext_sum(ofhe_ks_t ks, uint32_t size_ql, uint32_t nterm, const uint64_t* x0,
                             const uint64_t* x1, uint64_t x_stride, const uint64_t* diag, uint64_t diag_stride,
                             const uint8_t* present, uint32_t nsum, uint64_t* out0, uint64_t* out1,
                             uint32_t batch, void* stream);
/* Sum of EvalFastRotationExt(., index_j, digits_j, false)
 * (ckksrns-leveledshe.cpp:402-457) over nset digit sets, each under its own key
 * (EvalAddExtInPlace, ckksrns-fhe.cpp:1544-1545):
 *   out_e[b] = sum_j sigma_kj(sum_d digits_j[b][d] * key_e_j[d])  (+ sum of addend1 on e = 1)
 * digits: [nset][batch][beta][size_ql + size_p][N]; auto_index, key_b, key_a as
 * for ofhe_hip_ks_fast_rotation_ext; addend1: [nadd][batch][size_ql + size_p][N]
 * added to element 1 unrotated (the identity giant steps, 1528-1533), or NULL
 * with nadd = 0; out0, out1: [batch][size_ql + size_p][N]. */
int ofhe_hip_ks_fast_rotation_ext_sum(ofhe_ks_t ks, uint32_t size_ql, uint32_t nset, const uint64_t* digits,
                                      const uint32_t* auto_index, const uint64_t* const* key_b,
                                      const uint64_t* const* key_a, const uint64_t* addend1, uint32_t nadd,
                                      uint64_t* out0, uint64_t* out1, uint32_t batch, void* stream);
/* One BSGS level.  Index arrays hold any odd values, taken mod 2N; an index
 * = 1 mod 2N is the reference's no-rotation branch (KeySwitchExt for a baby
 * step, 1521; KeySwitchDownFirstElement for a giant step, 1528-1533) and its key
 * pointers are ignored.  Keys are host arrays of device pointers, laid out as
 * for ofhe_hip_ks_fast_core_ext.  diag[j * nbaby + i] (device, diag_stride words
 * apart, (size_ql + size_p) towers of N each) is giant step j's diagonal for
 * baby step i; present: host bytes [ngiant * nbaby] or NULL (all present). */
typedef struct ofhe_bsgs {
    uint32_t nbaby, ngiant;
    const uint32_t* baby_index;          /* [nbaby]  */
    const uint32_t* giant_index;         /* [ngiant] */
    const uint64_t* const* baby_key_b;   /* [nbaby]  */
    const uint64_t* const* baby_key_a;
    const uint64_t* const* giant_key_b;  /* [ngiant] */
    const uint64_t* const* giant_key_a;
    const uint64_t* diag;
    uint64_t diag_stride;
    const uint8_t* present;
} ofhe_bsgs;
/* With R_i = KeySwitchExt(ct) or EvalFastRotationExt(ct, baby_index[i], digits(c1), true),
 * I_j = sum_{i present} R_i * diag[j * nbaby + i] (both elements, Ql|P):
 *   identity giant j:  first += ModDown(I_j[0]);  outer[1] += I_j[1]
 *   other giant j:     (m0, m1) = ModDown(I_j);   first += sigma_kj(m0);
 *                      outer += EvalFastRotationExt((., m1), giant_index[j], digits(m1), false)
 *   out0 = ModDown(outer[0]) + first,   out1 = ModDown(outer[1])
 * ModDown as ofhe_hip_ks_mod_down with the same t, applied where the reference
 * applies it (before the automorphism).  c0, c1, out0, out1: [batch][size_ql][N]. */
int ofhe_hip_ks_bsgs_transform(ofhe_ks_t ks, uint32_t size_ql, const ofhe_bsgs* tr, const uint64_t* c0,
                               const uint64_t* c1, uint64_t* out0, uint64_t* out1, uint64_t t, uint32_t batch,
                               void* stream);

/* ---- CKKS / BGV multiplication with relinearisation and rescaling ----
 * LeveledSHEBase::EvalMult(ct1, ct2, evalKey) and its InPlace / Mutable forms (base-leveledshe.cpp:199-259,
 * 322-338), EvalSquare(ct, evalKey) and its forms (262-319), EvalMultCore (657-696), EvalSquareCore (699-750),
 * Relinearize / RelinearizeInPlace / EvalMultAndRelinearize (341-372),
 * LeveledSHECKKSRNS::ModReduceInternalInPlace (ckksrns-leveledshe.cpp:107-132) and
 * LeveledSHEBGVRNS::ModReduceInternalInPlace (bgvrns-leveledshe.cpp:45-77), on the HYBRID engine.  All
 * polynomials are in evaluation form, [batch][towers][N] dense, over the engine's q[0..size_ql), 16-byte aligned.
 * The rescaling tables (qlInvModq, QlQlInvModqlDivqlModq, negtInvModq: ckksrns-cryptoparameters.cpp:66-87,
 * bgvrns-cryptoparameters.cpp:91-107) are built by the engine from its moduli.
 * scheme: OFHE_SHE_CKKS rescales by DropLastElementAndScale, t must be 0; OFHE_SHE_BGV rescales by ModReduce,
 * t >= 2 and invertible modulo every tower it meets (the same t goes to the key switch's ModDown).
 * The rescale the AUTO scaling techniques apply to an operand before the product (rns-leveledshe.cpp:172-216)
 * is the caller's ofhe_hip_ks_rescale on that operand; scaling factors and noise degrees stay with the caller. */
#define OFHE_SHE_CKKS 0
#define OFHE_SHE_BGV 1

/* ModReduceInternalInPlace (ckksrns-leveledshe.cpp:107-132, bgvrns-leveledshe.cpp:45-77): `levels` >= 1 rescalings of a ciphertext of nelem >= 1 elements,
 * x[k] over size_ql towers -> out[k] over size_ql - levels >= 1 towers. x / out: host arrays of device pointers.
 * No output may overlap an input or another output. */
int ofhe_hip_ks_rescale(ofhe_ks_t ks, uint32_t size_ql, int scheme, uint64_t t, uint32_t levels, uint32_t nelem,
                        const uint64_t* const* x, uint64_t* const* out, uint32_t batch, void* stream);

/* RelinearizeInPlace (base-leveledshe.cpp:357-372) of nelem >= 3 elements: for j >= 2, ab = KeySwitchCore(c[j], key[j-2]); out0 = c[0] + sum ab[0],
 * out1 = c[1] + sum ab[1]. key_b / key_a: host arrays of nelem - 2 device pointers, keys laid out as for ofhe_hip_ks_core.
 * out0 may be c[0] and out1 may be c[1]; no other overlap. t as for ofhe_hip_ks_core. */
int ofhe_hip_ks_relinearize(ofhe_ks_t ks, uint32_t size_ql, uint32_t nelem, const uint64_t* const* c,
                            const uint64_t* const* key_b, const uint64_t* const* key_a, uint64_t* out0, uint64_t* out1,
                            uint64_t t, uint32_t batch, void* stream);

/* EvalMult(ct1, ct2, evalKey) (base-leveledshe.cpp:199-218) then ModReduceInternalInPlace(levels), levels >= 0.
 * d0 == d1 == NULL: EvalSquare(ct, evalKey) (262-280).
 * out0, out1 over size_ql - levels towers. An output may start exactly at an operand's address (the InPlace
 * forms: the tensor product consumes the operands first); any other overlap is refused. */
int ofhe_hip_ks_eval_mult(ofhe_ks_t ks, uint32_t size_ql, const uint64_t* c0, const uint64_t* c1, const uint64_t* d0,
                          const uint64_t* d1, const uint64_t* key_b, const uint64_t* key_a, int scheme, uint64_t t,
                          uint32_t levels, uint64_t* out0, uint64_t* out1, uint32_t batch, void* stream);

/* ---- element maps ---- */
/* NativeVectorT::SwitchModulus (mubintvecnat.cpp:111-136) on n words:
 * values of modulus old_q re-centred to new_q, exactly as the reference. */
int ofhe_hip_switch_modulus(ofhe_ctx_t ctx, const uint64_t* src, uint64_t* dst, uint64_t n,
                            uint64_t old_q, uint64_t new_q, void* stream);
/* PolyImpl::AutomorphismTransform(k) (poly-impl.h:312-365), X -> X^k for odd
 * k, per (batch, tower) of plan; eval_form != 0 permutes bit-reversed
 * evaluation slots, else signed permutation of coefficients (a negated zero
 * stays q, as in the reference).  dst must not overlap src. */
int ofhe_hip_automorphism(ofhe_plan_t plan, uint32_t k, int eval_form, const uint64_t* src, uint64_t* dst,
                          uint32_t batch, void* stream);

/* ---- rescaling (callers of the path one tower down) ----
 * x: [batch][towers][N] (x_stride words per batch entry) over plan towers
 * 0..towers-1, canonical, all in evaluation form (eval_form != 0) or all in
 * coefficient form; out: [batch][towers-1][N] (out_stride).  out may be x
 * itself only with out_stride == x_stride (in place); any other overlap of
 * the two ranges is rejected with OFHE_ERR_ARG.
 * DCRTPolyImpl::DropLastElementAndScale (dcrtpoly-impl.h:746-768), CKKS / BFV
 * rescaling with ql_ql_inv_modql_divql_modq[i] and ql_inv_modq[i], i <
 * towers-1 (ckksrns-cryptoparameters.cpp:72-86):
 *   out_i = x_i ql_inv_modq_i + [SwitchModulus(x_last) c_i]   (evaluation:
 *   the last tower through the INTT, the switched term through the NTT);
 *   coefficient form: out_i = NTT(x_i ql_inv_modq_i + SwitchModulus(x_last) c_i)
 *   -- the reference switches these towers to evaluation form (lines 765-766).
 * ql_inv_modq_i must be invertible mod q_i in evaluation form (it is
 * q_last^-1 mod q_i). */
int ofhe_hip_drop_last_and_scale(ofhe_plan_t plan, uint32_t towers, const uint64_t* x, uint64_t x_stride,
                                 uint64_t* out, uint64_t out_stride, int eval_form,
                                 const uint64_t* ql_ql_inv_modql_divql_modq, const uint64_t* ql_inv_modq,
                                 uint32_t batch, void* stream);
/* DCRTPolyImpl::ModReduce (dcrtpoly-impl.h:792-812), BGV modulus switching:
 * delta = [x_last]_coefficient * neg_t_inv_modq mod q_last;
 *   out_i = (x_i + [SwitchModulus(delta)] t) ql_inv_modq_i, the switched term
 * through the NTT in evaluation form; the output keeps the input's form. */
int ofhe_hip_mod_reduce(ofhe_plan_t plan, uint32_t towers, const uint64_t* x, uint64_t x_stride, uint64_t* out,
                        uint64_t out_stride, int eval_form, uint64_t t, uint64_t neg_t_inv_modq,
                        const uint64_t* ql_inv_modq, uint32_t batch, void* stream);

/* ---- BV key switching, digitSize = 0 (KeySwitchBV, keyswitch-bv.cpp:302-340) ----
 * KeySwitchBV::EvalKeySwitchPrecomputeCore -> DCRTPolyImpl::CRTDecompose(0)
 * (keyswitch-bv.cpp:308-312, dcrtpoly-impl.h:266-288): c [batch][towers][N]
 * in evaluation form over plan towers 0..towers-1 -> digits
 * [batch][towers][towers][N], digit i = tower i of c in coefficient form,
 * SwitchModulus'd into every tower, in evaluation form. */
int ofhe_hip_bv_precompute(ofhe_plan_t plan, uint32_t towers, const uint64_t* c, uint64_t* digits, uint32_t batch,
                           void* stream);
/* KeySwitchBV::EvalFastKeySwitchCore (keyswitch-bv.cpp:314-340): ct0 =
 * sum_i bv[i] * d_i, ct1 = sum_i av[i] * d_i over the first `towers` towers of
 * the keys key_b / key_a [towers][key_towers][N] (DropLastElements at lower
 * levels); out0, out1 [batch][towers][N], evaluation form. */
int ofhe_hip_bv_core(ofhe_plan_t plan, uint32_t towers, const uint64_t* digits, const uint64_t* key_b,
                     const uint64_t* key_a, uint32_t key_towers, uint64_t* out0, uint64_t* out1, uint32_t batch,
                     void* stream);

/* ---- BV key switching with a digit size (digitSize = r, base-2^r digits;
 *      DCRTPolyImpl::CRTDecompose(r), dcrtpoly-impl.h:266-320) ----
 * Tower i of c in coefficient form is cut into w_i = ceil(bitlen(q_i) / r)
 * windows win_{i,j}[x] = (coef_i[x] >> (j r)) & (2^r - 1)
 * (PolyImpl::BaseDecompose, poly-impl.h:516-542).  Digit arrWindows[i] + j,
 * arrWindows[i] = w_0 + ... + w_{i-1}, holds win_{i,j} in tower i and
 * SwitchModulus(win_{i,j}, q_i -> q_k) in every tower k != i, in evaluation
 * form.  digit_size = 0 is the setting of the two calls above (one digit per
 * tower) and gives their words; digit_size > 30 has no defined reference
 * behaviour (1 << digitSize in an int) and is refused with OFHE_ERR_ARG.
 * Every data buffer is 16-byte aligned.  The argument rules that need no plan
 * (NULL pointers, batch == 0, alignment, digit_size > 30, count == NULL,
 * n_digits == 0, key_towers < towers, digits given as an output) are checked
 * before the plan and return OFHE_ERR_ARG; a NULL plan after those returns
 * OFHE_ERR_STATE.
 *
 * The reference's nWindows over the plan's first `towers` moduli. */
int ofhe_hip_bv_digit_count(ofhe_plan_t plan, uint32_t towers, uint32_t digit_size, uint32_t* count);
/* KeySwitchBV::EvalKeySwitchPrecomputeCore: c [batch][towers][N] in evaluation
 * form -> digits [batch][n_digits][towers][N] in evaluation form, in the
 * reference's digit order, n_digits = ofhe_hip_bv_digit_count. */
int ofhe_hip_bv_precompute_digits(ofhe_plan_t plan, uint32_t towers, uint32_t digit_size, const uint64_t* c,
                                  uint64_t* digits, uint32_t batch, void* stream);
/* KeySwitchBV::EvalFastKeySwitchCore (keyswitch-bv.cpp:314-338) over n_digits
 * digits: out0 = sum_d key_b[d] * digit_d, out1 = sum_d key_a[d] * digit_d.
 * The keys are [key_digits][key_towers][N]; the first `towers` towers of the
 * first n_digits polynomials are used (a lower level's digits are a prefix of
 * the key's numbering).  Any n_digits up to the digit count of these towers at
 * digit_size = 1: the sum is exact in 128 bits and folded every 256 terms. */
int ofhe_hip_bv_core_digits(ofhe_plan_t plan, uint32_t towers, uint32_t n_digits, const uint64_t* digits,
                            const uint64_t* key_b, const uint64_t* key_a, uint32_t key_towers,
                            uint64_t* out0, uint64_t* out1, uint32_t batch, void* stream);
/* KeySwitchBV::KeySwitchInPlace (keyswitch-bv.cpp:283-300) in one call:
 * out0 = add0 + ct0, out1 = add1 + ct1 with (ct0, ct1) the two sums above over
 * the digits of c.  add0 / add1: [batch][towers][N], canonical, NULL for zero,
 * and each may be its own output (a two-element ciphertext passes add1 = NULL,
 * a three-element one its first two elements); an output may also be c itself.
 * The whole digit array is never held: the decomposition and the inner product
 * run over chunk_digits digits at a time, each chunk adding into the outputs,
 * and the result does not depend on chunk_digits.  chunk_digits = 0 takes the
 * most digits whose [batch][chunk][towers][N] words fit in 1 GiB of scratch
 * (at least one). */
int ofhe_hip_bv_key_switch(ofhe_plan_t plan, uint32_t towers, uint32_t digit_size, const uint64_t* c,
                           const uint64_t* key_b, const uint64_t* key_a, uint32_t key_towers,
                           const uint64_t* add0, const uint64_t* add1, uint64_t* out0, uint64_t* out1,
                           uint32_t chunk_digits, uint32_t batch, void* stream);
/* Tuning knob of the inner product above, process-wide: the batch entries whose
 * accumulators one thread holds while it loads each key word pair once
 * (key-stationary).  0: the library's choice per batch size; 1: the plain loop;
 * 2 or 4.  The results are the same words under every setting. */
int ofhe_hip_bv_tune(uint32_t key_stationary);

/* ---- BFV multiplication, HPS family: what LeveledSHEBFVRNS::EvalMult
 *      (pke/lib/scheme/bfvrns/bfvrns-leveledshe.cpp:168-408) runs between the
 *      tensor product and key switching.  All results are bit-exact with the
 *      reference's HAVE_INT128 && NATIVEINT == 64 branches, the value of the
 *      floating-point correction term included.
 *
 *      Floating-point contract.  nu starts at 0.5.  For source towers
 *      i = 0, 1, ... in that order: nu = nu + (double(y_i) * qInv[i]) in
 *      SwitchCRTBasis and nu = nu + (frac[i] * double(x_i)) in ScaleAndRound.
 *      Every multiply and every add is rounded separately to IEEE double,
 *      round-to-nearest-even (the reference's baseline x86-64 build): no fused
 *      multiply-add, no tree or cross-lane reordering of the sum, no float.
 *      double(uint64) is the correctly rounded conversion (values reach 2^60).
 *      alpha = floor(nu), and nu >= 0.5 always.  Where a kernel spreads the
 *      source towers over lanes, only the products are computed apart; the
 *      additions happen in tower order. ---- */

/* DCRTPolyImpl::SwitchCRTBasis (dcrtpoly-impl.h:1178-1230), the exact switch:
 * y_i = [x_i QHat_i^-1]_{q_i} canonical, alpha = floor(0.5 + sum_i double(y_i) qInv[i]),
 * out_j = (sum_i y_i QHatModp_ij mod p_j).ModSubFast(alphaQModp[alpha][j]).
 * bconv must hold the true CRT tables (QHat^-1 mod q, QHat mod p); layout as
 * ofhe_hip_approx_switch_crt_basis (x: [batch][size_q][N] -> out:
 * [batch][size_p][N], coefficient form).  alphaQModp[a][j] = a Q mod p_j,
 * a = 0 .. size_q (bfvrns-cryptoparameters.cpp:343-350, 418-424) and
 * qInv[i] = 1.0 / double(q_i) (:270-273, 441-444) are derived from the
 * handle's moduli on its first exact call (that one call uploads them and waits
 * on the null stream, as a cache miss of ofhe_hip_approx_mod_down does, so it
 * cannot run inside a stream capture) and cached; no later call synchronises.
 * One fused kernel launch; OFHE_BCONV_KERNEL_LIMB / _WIDE on
 * the handle select the VALU variants here too. */
int ofhe_hip_switch_crt_basis(ofhe_bconv_t bconv, const uint64_t* x, uint64_t* out, uint32_t batch, void* stream);

/* DCRTPolyImpl::ExpandCRTBasis with resultFormat = EVALUATION
 * (dcrtpoly-impl.h:1311-1358); signature and layout of ofhe_hip_approx_mod_up:
 * x [batch][Q][N] (evaluation form when eval_form != 0, else coefficient
 * form) -> out [batch][Q+P][N], evaluation form.  In the reference's order:
 * INTT of an evaluation-form input, exact switch Q -> P, NTT of the P towers;
 * the Q towers of out are the caller's evaluation-form words copied, or the
 * NTT of a coefficient-form input.  out must not overlap x (OFHE_ERR_ARG), and
 * the three objects must belong to one context. */
int ofhe_hip_expand_crt_basis(ofhe_plan_t plan_q, ofhe_plan_t plan_p, ofhe_bconv_t q_to_p, int eval_form,
                              const uint64_t* x, uint64_t* out, uint32_t batch, void* stream);

/* DCRTPolyImpl::ScaleAndRound, DCRTPoly -> DCRTPoly (dcrtpoly-impl.h:1876-1955).
 * x: [batch][size_q + size_p][N], Q towers first, coefficient form.
 * out_is_q = 0 (HPS): the Q towers are summed, out is [batch][size_p][N] over
 * P and the "own tower" term uses x[size_q + j]; out_is_q = 1 (HPSPOVERQ): the
 * P towers are summed, out is [batch][size_q][N] over Q, own tower x[j].
 * With size_i summed towers and size_o outputs, int_table is host
 * [size_o][size_i + 1] (tOSHatInvModsDivsModo) and frac host [size_i] doubles
 * in [0, 1) (tOSHatInvModsDivsFrac), as the pke layer builds them
 * (bfvrns-cryptoparameters.cpp:289-311, 532-556); Barrett constants are derived
 * here.  size_i <= 255 (size_i + 1 products must fit the 128-bit sum, the limit
 * of the reference's DoubleNativeInt) and the output moduli must be odd.  One fused kernel: nu, alpha, the 128-bit sums of size_i + 1 products,
 * BarrettUint128ModUint64 and + (alpha mod o_j).  Both reference branches
 * compute floor(nu) mod o_j; floor(nu) is taken exactly as a 128-bit integer
 * from the double, so nu >= 2^64 is right, and nu == 2^64 (where the
 * reference's cast is undefined) is defined as floor(nu) mod o_j. */
typedef struct ofhe_scale_round_s* ofhe_scale_round_t;
int ofhe_hip_scale_round_create(ofhe_ctx_t ctx, uint32_t log_n, uint32_t size_q, uint32_t size_p, const uint64_t* q,
                                const uint64_t* p, int out_is_q, const uint64_t* int_table, const double* frac,
                                ofhe_scale_round_t* handle);
int ofhe_hip_scale_round_destroy(ofhe_scale_round_t handle);
int ofhe_hip_scale_and_round(ofhe_scale_round_t handle, const uint64_t* x, uint64_t* out, uint32_t batch,
                             void* stream);

/* LeveledSHEBFVRNS::EvalMult for two 2-element ciphertexts
 * (bfvrns-leveledshe.cpp:168-408), composed from handles the caller created and
 * keeps alive: plan_q / plan_r / plan_qr (Q towers then R towers), q_to_r and
 * r_to_q with the true CRT tables, scale_round, and for HPSPOVERQ q_to_r_neg, a
 * converter created with mNegRlQHatInvModq / qInvModr
 * (bfvrns-cryptoparameters.cpp:501-523); q_to_r_neg is NULL for HPS.  Every
 * handle must belong to ctx.
 * c0, c1, d0, d1: [batch][Q][N] evaluation form; out0..out2: [batch][Q][N] in
 * coefficient form, as the reference leaves cvMult.
 *   OFHE_BFV_HPS: ExpandCRTBasis of the four inputs, the tensor product over
 *     Q|R, INTT, ScaleAndRound to R (out_is_q = 0), exact switch R -> Q.
 *   OFHE_BFV_HPSPOVERQ (size_r == size_q): ExpandCRTBasis of c0, c1;
 *     FastExpandCRTBasisPloverQ of d0, d1 (dcrtpoly-impl.h:1413-1466: INTT,
 *     approximate switch through q_to_r_neg, exact switch R -> Q replacing the
 *     Q towers, NTT); the tensor product, INTT, ScaleAndRound to Q (out_is_q = 1).
 * Scratch comes from the context's stream-ordered pool; no call synchronises. */
enum {
    OFHE_BFV_HPS = 0,
    OFHE_BFV_HPSPOVERQ = 1,
    OFHE_BFV_BEHZ = 2 /* ofhe_hip_bfv_decrypt_create only; the multiplication is ofhe_hip_bfv_eval_mult_behz */
};
typedef struct ofhe_bfv_mult_s* ofhe_bfv_mult_t;
int ofhe_hip_bfv_mult_create(ofhe_ctx_t ctx, int technique, ofhe_plan_t plan_q, ofhe_plan_t plan_r,
                             ofhe_plan_t plan_qr, ofhe_bconv_t q_to_r, ofhe_bconv_t r_to_q, ofhe_bconv_t q_to_r_neg,
                             ofhe_scale_round_t scale_round, ofhe_bfv_mult_t* handle);
int ofhe_hip_bfv_mult_destroy(ofhe_bfv_mult_t handle);
int ofhe_hip_bfv_eval_mult(ofhe_bfv_mult_t handle, const uint64_t* c0, const uint64_t* c1, const uint64_t* d0,
                           const uint64_t* d1, uint64_t* out0, uint64_t* out1, uint64_t* out2, uint32_t batch,
                           void* stream);

/* ---- BFV multiplication, HPSPOVERQLEVELED with dropped levels.  l is the index
 *      of the last kept tower: Q_l = q_0 .. q_l and R_l = r_0 .. r_l have l + 1
 *      towers each, Q is the full chain of size_q towers.  The caller chooses l
 *      (FindLevelsToDrop, bfvrns-leveledshe.cpp:77-166); no call here does.
 *      The floating-point contract above holds for every call unchanged.
 *
 * One level's handle, composed from handles the caller created and keeps alive
 * (tables as bfvrns-cryptoparameters.cpp builds them for level l):
 *   plan_q                 the full chain Q
 *   plan_ql, plan_rl       Q_l and R_l; plan_qlrl their concatenation (:233-258)
 *   ql_to_rl, rl_to_ql     converters with the true CRT tables of Q_l -> R_l and
 *                          R_l -> Q_l (:156-188, :352-364, :390-439)
 *   q_to_rl_neg            size_q sources -> l + 1 targets, created with
 *                          mNegRlQHatInvModq(l) [size_q] (= q_i - R_l (Q/q_i)^-1 mod
 *                          q_i, the full Q) and qInvModr [size_q][l + 1] (:501-523)
 *   drop                   ScaleAndRound Q -> Q_l (QlQHatInvModqDivqModq(l) / Frac(l),
 *                          :592-615): a handle with size_q = l + 1, size_p =
 *                          size_q - l - 1, out_is_q = 1; NULL exactly when
 *                          l == size_q - 1
 *   scale_round            ScaleAndRound Q_l R_l -> Q_l (tQlSlHatInvModsDivsModq(l) /
 *                          Frac(l), :558-586): size_q = size_p = l + 1, out_is_q = 1
 *   ql_hat_modq            host [l + 1], QlHatModq(l)[i] = (Q / Q_l) mod q_i (:621-631)
 * Every argument is checked before the device is touched: the contexts and the
 * ring size, plan_ql / plan_rl against plan_qlrl, plan_ql as a prefix of plan_q,
 * every handle's tower counts, ql_hat_modq[i] < q_i. */
typedef struct ofhe_bfv_level_s* ofhe_bfv_level_t;
int ofhe_hip_bfv_level_create(ofhe_ctx_t ctx, uint32_t l, ofhe_plan_t plan_q, ofhe_plan_t plan_ql, ofhe_plan_t plan_rl,
                              ofhe_plan_t plan_qlrl, ofhe_bconv_t ql_to_rl, ofhe_bconv_t rl_to_ql,
                              ofhe_bconv_t q_to_rl_neg, ofhe_scale_round_t drop, ofhe_scale_round_t scale_round,
                              const uint64_t* ql_hat_modq, ofhe_bfv_level_t* handle);
int ofhe_hip_bfv_level_destroy(ofhe_bfv_level_t handle);
/* DCRTPolyImpl::ExpandCRTBasisQlHat (dcrtpoly-impl.h:1514-1534), with the
 * addition that follows it in RelinearizeCore (bfvrns-leveledshe.cpp:889-896)
 * when addend is not NULL:
 *   out_i = x_i QlHatModq_i mod q_i (ModMulFastConstEq) [+ addend_i]   i <= l
 *   out_i = addend_i, or 0 without an addend                           l < i < size_q
 * x: [batch][l + 1][N]; addend, out: [batch][size_q][N]; any form, canonical
 * words.  out may be addend itself; it must not overlap x (OFHE_ERR_ARG). */
int ofhe_hip_expand_ql_hat(ofhe_bfv_level_t handle, const uint64_t* x, const uint64_t* addend, uint64_t* out,
                           uint32_t batch, void* stream);
/* ScaleAndRound to Q_l with the handle's scale_round tables
 * (bfvrns-leveledshe.cpp:367-374; dcrtpoly-impl.h:1876-1955) and
 * ExpandCRTBasisQlHat (:376-380; dcrtpoly-impl.h:1514-1534) in one launch:
 * x [batch][2 (l + 1)][N] over Q_l R_l, coefficient form -> out
 * [batch][size_q][N].  Word for word ofhe_hip_scale_and_round followed by
 * ofhe_hip_expand_ql_hat. */
int ofhe_hip_scale_round_expand_ql_hat(ofhe_bfv_level_t handle, const uint64_t* x, uint64_t* out, uint32_t batch,
                                       void* stream);
/* LeveledSHEBFVRNS::EvalMult, HPSPOVERQLEVELED at level l
 * (bfvrns-leveledshe.cpp:235-274, 316-330, 367-382), and EvalSquare (:459-499)
 * when d0 == c0 and d1 == c1.  c0, c1, d0, d1: [batch][size_q][N] evaluation
 * form; out0..out2: [batch][size_q][N] coefficient form, as the reference leaves
 * cvMult.  (c0, c1): INTT, ScaleAndRound Q -> Q_l when l < size_q - 1,
 * ExpandCRTBasis Q_l -> Q_l R_l.  (d0, d1): INTT, FastExpandCRTBasisPloverQ
 * (dcrtpoly-impl.h:1413-1466) from all size_q towers through q_to_rl_neg, the
 * exact switch R_l -> Q_l, NTT.  Then the tensor product over Q_l R_l, INTT,
 * ScaleAndRound to Q_l and ExpandCRTBasisQlHat.  At l == size_q - 1 the words
 * are those of ofhe_hip_bfv_eval_mult with OFHE_BFV_HPSPOVERQ.  Scratch comes
 * from the context's stream-ordered pool; no call synchronises. */
int ofhe_hip_bfv_eval_mult_leveled(ofhe_bfv_level_t handle, const uint64_t* c0, const uint64_t* c1, const uint64_t* d0,
                                   const uint64_t* d1, uint64_t* out0, uint64_t* out1, uint64_t* out2, uint32_t batch,
                                   void* stream);
/* LeveledSHEBFVRNS::RelinearizeCore, HPSPOVERQLEVELED at level l
 * (bfvrns-leveledshe.cpp:845-899).  elements = 3: (c0, c1, c2); elements = 2:
 * (c0, c1) and c2 must be NULL.  Inputs [batch][size_q][N], all in evaluation
 * form (eval_form != 0) or all in coefficient form.  The last element is scaled
 * to Q_l (:863-872), KeySwitchCore runs at l + 1 towers with the HYBRID engine
 * ks (:878-879; keys laid out as for ofhe_hip_ks_core), ExpandCRTBasisQlHat
 * lifts both results (:881-887), and out0 = c0 + ab0; out1 = c1 + ab1 with three
 * elements, ab1 with two (:889-896).  out0, out1: [batch][size_q][N] evaluation
 * form; they must not overlap the inputs.  ks must have been created for the
 * chain Q of plan_q. */
int ofhe_hip_bfv_relinearize_leveled(ofhe_bfv_level_t handle, ofhe_ks_t ks, uint32_t elements, int eval_form,
                                     const uint64_t* c0, const uint64_t* c1, const uint64_t* c2, const uint64_t* key_b,
                                     const uint64_t* key_a, uint64_t* out0, uint64_t* out1, uint32_t batch,
                                     void* stream);

/* BFV multiplication by the BEHZ technique: LeveledSHEBFVRNS::EvalMult's
 * `else` branches (bfvrns-leveledshe.cpp:275-297, 383-403) and the three
 * DCRTPolyImpl functions under them, HAVE_INT128 && NATIVEINT == 64 branches,
 * integers only:
 *   FastBaseConvqToBskMontgomery  dcrtpoly-impl.h:2050-2208
 *   FastRNSFloorq                 dcrtpoly-impl.h:2212-2271
 *   FastBaseConvSK                dcrtpoly-impl.h:2309-2411
 * All data is [batch][towers][N] 64-bit words.  "Bsk" is the size_b towers of
 * B followed by msk: size_b + 1 towers (the reference always has size_b ==
 * size_q; nothing here assumes it).  mtilde = 2^16.
 * ofhe_behz_tables holds one host pointer per table of
 * CryptoParametersBFVRNS::PrecomputeCRTTables' BEHZ part
 * (bfvrns-cryptoparameters.cpp:665-851), row-major where two-dimensional,
 * one word where scalar; Shoup and 128-bit Barrett constants are derived in
 * create.  create uploads and waits (it cannot run under stream capture) and
 * returns OFHE_ERR_ARG -- before it looks at ctx -- for a modulus that is
 * even or not below 2^60, a Bsk modulus <= 2^16, a modulus repeated in
 * q u Bsk, size_q or size_b of 0 or above 255 (the sums of that many products
 * must fit 128 bits, the reference's DoubleNativeInt limit) or a NULL table.
 * Every other call is stream-ordered, one fused kernel launch per reference
 * function, and never synchronises:
 *   ofhe_hip_behz_q_to_bsk  x [batch][size_q][N] -> out [batch][size_b+1][N],
 *     both in coefficient form (dcrtpoly-impl.h:2098-2187 alone).
 *   ofhe_hip_behz_expand  the whole FastBaseConvqToBskMontgomery with its
 *     format handling (dcrtpoly-impl.h:2050-2208), as ofhe_hip_expand_crt_basis:
 *     x [batch][size_q][N] (evaluation form when eval_form != 0, else
 *     coefficient form) -> out [batch][size_q+size_b+1][N], evaluation form.
 *     An evaluation-form input keeps its Q towers (its INTT passes through
 *     out's Q slots); a coefficient-form input has them transformed; the Bsk
 *     towers are always transformed.  out must not overlap x.
 *   ofhe_hip_behz_floor  x [batch][size_q+size_b+1][N] -> out
 *     [batch][size_b+1][N], coefficient form; x is only read (the reference
 *     twists its Q towers in place and then discards them).
 *   ofhe_hip_behz_conv_sk  x [batch][size_b+1][N] -> out [batch][size_q][N].
 *     One deliberate definition: the correction is the CENTRED alpha,
 *     out_j = (S_j - alpha_c B) mod q_j with alpha_c = alpha - msk for
 *     alpha > floor(msk / 2).  The reference forms alpha.ModSubFast(msk, q_j)
 *     = alpha + q_j - msk in unsigned words (dcrtpoly-impl.h:2384-2385), which
 *     is that residue only while msk - alpha <= q_j and wraps for a ciphertext
 *     tower below msk / 2; the two agree wherever the reference does not
 *     wrap, in particular whenever msk < 2 min q_j.
 *   ofhe_hip_behz_floor_sk  floor then conv_sk (bfvrns-leveledshe.cpp:390-401):
 *     x [batch][size_q+size_b+1][N] -> out [batch][size_q][N].  fused = 1: one
 *     launch that keeps the size_b + 1 intermediate residues of a coefficient
 *     on chip (OFHE_ERR_ARG when size_b > OFHE_BEHZ_FUSED_MAX_B); 0: the two
 *     launches through pool scratch; 2: fused when it fits, which is what the
 *     multiplication does.  Same words either way; 0 and 1 exist, like the
 *     kernel choices of ofhe_bconv_options, so that tests and A/B timings
 *     reach both paths in one process.
 *   ofhe_hip_bfv_eval_mult_behz  c0, c1, d0, d1 [batch][Q][N] evaluation form
 *     -> out0..out2 [batch][Q][N] coefficient form, as ofhe_hip_bfv_eval_mult:
 *     behz_expand of the four inputs, ofhe_hip_eval_mult_core over plan_qbsk
 *     (Q towers then Bsk), INTT, floor and conv_sk (fused when it fits).
 *     Scratch comes from the context's stream-ordered pool.
 * The plans must transform exactly the handle's towers at its N in its
 * context (OFHE_ERR_ARG otherwise). */
#define OFHE_BEHZ_FUSED_MAX_B 16
typedef struct ofhe_behz_s* ofhe_behz_t;
typedef struct ofhe_behz_tables {
    const uint64_t* tQHatInvModq;      /* [size_q]              :724-735 */
    const uint64_t* QHatModbsk;        /* [size_q][size_b + 1]  :737-749 */
    const uint64_t* QHatModmtilde;     /* [size_q]              :748 */
    const uint64_t* qInvModbsk;        /* [size_q][size_b + 1]  :751-757 */
    const uint64_t* mtildeQHatInvModq; /* [size_q]              :759-772 */
    const uint64_t* negQInvModmtilde;  /* [1]                   :774-777 */
    const uint64_t* QModbsk;           /* [size_b + 1]          :779-787 */
    const uint64_t* mtildeInvModbsk;   /* [size_b + 1]          :789-797 */
    const uint64_t* tQInvModbsk;       /* [size_b + 1]          :799-808 */
    const uint64_t* BHatInvModb;       /* [size_b]              :810-821 */
    const uint64_t* BHatModq;          /* [size_b][size_q]      :823-832 */
    const uint64_t* BHatModmsk;        /* [size_b]              :834-839 */
    const uint64_t* BInvModmsk;        /* [1]                   :841-843 */
    const uint64_t* BModq;             /* [size_q]              :845-851 */
} ofhe_behz_tables;
int ofhe_hip_behz_create(ofhe_ctx_t ctx, uint32_t log_n, uint32_t size_q, const uint64_t* q, uint32_t size_b,
                         const uint64_t* bsk /* size_b + 1, msk last */, uint64_t t, const ofhe_behz_tables* tables,
                         ofhe_behz_t* handle);
int ofhe_hip_behz_destroy(ofhe_behz_t handle);
int ofhe_hip_behz_q_to_bsk(ofhe_behz_t handle, const uint64_t* x, uint64_t* out, uint32_t batch, void* stream);
int ofhe_hip_behz_expand(ofhe_behz_t handle, ofhe_plan_t plan_q, ofhe_plan_t plan_bsk, int eval_form,
                         const uint64_t* x, uint64_t* out, uint32_t batch, void* stream);
int ofhe_hip_behz_floor(ofhe_behz_t handle, const uint64_t* x, uint64_t* out, uint32_t batch, void* stream);
int ofhe_hip_behz_conv_sk(ofhe_behz_t handle, const uint64_t* x, uint64_t* out, uint32_t batch, void* stream);
int ofhe_hip_behz_floor_sk(ofhe_behz_t handle, int fused, const uint64_t* x, uint64_t* out, uint32_t batch,
                           void* stream);
int ofhe_hip_bfv_eval_mult_behz(ofhe_behz_t handle, ofhe_plan_t plan_q, ofhe_plan_t plan_bsk, ofhe_plan_t plan_qbsk,
                                const uint64_t* c0, const uint64_t* c1, const uint64_t* d0, const uint64_t* d1,
                                uint64_t* out0, uint64_t* out1, uint64_t* out2, uint32_t batch, void* stream);

/* ---- BFV decryption and encryption scaling: PKEBFVRNS::Decrypt
 *      (pke/lib/scheme/bfvrns/bfvrns-pke.cpp:205-248) and the one BFV-specific
 *      step of encryption, DCRTPolyImpl::TimesQovert
 *      (dcrtpoly-impl.h:1015-1031), so that only the N-word plaintext crosses
 *      the bus.  Bit-exact with the reference's NATIVEINT == 64 build.
 *
 *      Floating-point contract (the reference's decryption ScaleAndRound uses
 *      double throughout, dcrtpoly-impl.h:1537-1814; the contract of the HPS
 *      block above applies unchanged).  The reference chooses one of eight
 *      loops (dcrtpoly-impl.h:1547-1803), labelled A-H in
 *      UnitTestBFVrnsDecrypt.cpp:126-148, from qMSB = msb(q[0]), tMSB,
 *      sizeQMSB = GetMSB64(size_q), qMSBHf = qMSB >> 1 and whether t is a power
 *      of two; the library chooses the same one:
 *        t = 2^k:  qMSB + sizeQMSB < 52:  qMSB + tMSB + sizeQMSB < 63 ? A : B
 *                  else:                  qMSBHf + tMSB + sizeQMSB < 62 ? C : D
 *        else:     qMSB + sizeQMSB < 52:  qMSB + tMSB + sizeQMSB < 52 ? E : F
 *                  else:                  qMSBHf + tMSB + sizeQMSB < 52 ? G : H
 *      A-D: floatSum starts at 0.5; per tower, in order,
 *        floatSum = floatSum + (double(x_i) * frac[i]);
 *      in the split loops C and D this is done for lo = x_i - (hi << qMSBHf)
 *      with frac[i], then for hi = x_i >> qMSBHf with fracB[i].
 *        out = (intSum + uint64(floatSum)) & (t - 1)
 *      with intSum modulo 2^64 (A and B give the same word, and so do C and D).
 *      E-H: floatSum starts at 0.0, the same chain; intSum is the exact sum of
 *      the products x_i * table[i] in E and G and the sum of the products
 *      reduced mod t (ModMulFastConst) in F and H -- the two give different
 *      doubles, so the loop matters; then
 *        floatSum = floatSum + double(intSum)
 *        quot     = uint64(floatSum * tInv)          tInv = 1.0 / td, td = double(t)
 *        floatSum = floatSum - (td * double(quot))
 *        out      = uint64(floatSum + 0.5)
 *      written as computed: it may equal t, as the reference's may, and is not
 *      canonicalised.  Every multiply, add and subtract is rounded separately
 *      to IEEE double, round-to-nearest-even; nothing is fused or reordered;
 *      double(uint64) is the correctly rounded conversion.  The casts to
 *      uint64 are the reference's: of a negative double they are undefined
 *      there (and give 0 here).
 *      One tower (size_q == 1, either technique; bfvrns-pke.cpp:233-245,
 *      mubintvecnat.cpp:420-435, ubintnat.h:536-540): with
 *        MR(y) = uint64(double(t) * (double(y) / double(q)) + 0.5)
 *      -- one correctly rounded IEEE division, then a separate multiply and
 *      add -- r = x > (q >> 1) ? q - MR(q - x) : MR(x) mod q, and out =
 *      SwitchModulus(r, q -> t) as ofhe_hip_switch_modulus.
 *      BEHZ (dcrtpoly-impl.h:2005-2049) is integers only, gamma = 2^26
 *      (rns-cryptoparameters.h:1701): per tower y = x_i tgammaQHatInvModq[i] mod
 *      q_i, s = (s + y negInvqModtgamma[i] mod tgamma) mod tgamma; out =
 *      (s + (s & (2^26 - 1))) >> 26.
 *
 * ofhe_bfv_decrypt_tables holds one host pointer per table of
 * CryptoParametersBFVRNS::PrecomputeCRTTables (bfvrns-cryptoparameters.cpp):
 * the HPS family reads the first four (:446-495; the two B tables only when
 * qMSB + sizeQMSB >= 52), BEHZ the next two (:853-884); tInvModq and negQModt
 * (:87-94) serve ofhe_hip_times_q_over_t and may both be NULL.  Tables a
 * technique does not read may be NULL, and none is read when size_q == 1.
 * Shoup preconditioners, td and tInv are derived in create, which uploads once
 * and waits (it cannot run under stream capture) and returns OFHE_ERR_ARG --
 * before it looks at ctx -- for t < 2, size_q of 0 or above 255,
 * 2 size_q t >= 2^64 (the sums of reduced products could wrap), a modulus that
 * is even or not below 2^60, BEHZ with t 2^26 >= 2^58, or a missing table (a
 * missing B table when the split applies included).  Every other call is
 * stream-ordered and never synchronises. */
enum {
    OFHE_BFV_DECRYPT_BEHZ = 8,     /* ofhe_hip_bfv_decrypt_branch: after the loops A..H = 0..7 */
    OFHE_BFV_DECRYPT_ONE_TOWER = 9
};
typedef struct ofhe_bfv_decrypt_s* ofhe_bfv_decrypt_t;
typedef struct ofhe_bfv_decrypt_tables {
    const uint64_t* tQHatInvModqDivqModt;  /* [size_q]  :453-462, 480 */
    const uint64_t* tQHatInvModqBDivqModt; /* [size_q]  :487-489 */
    const double* tQHatInvModqDivqFrac;    /* [size_q]  :465-467, 483-485 */
    const double* tQHatInvModqBDivqFrac;   /* [size_q]  :492-493 */
    const uint64_t* tgammaQHatInvModq;     /* [size_q]  :871-884 */
    const uint64_t* negInvqModtgamma;      /* [size_q]  :859-869 */
    const uint64_t* tInvModq;              /* [size_q]  :87-90 */
    const uint64_t* negQModt;              /* [1]       :92-94 */
} ofhe_bfv_decrypt_tables;
int ofhe_hip_bfv_decrypt_create(ofhe_ctx_t ctx, uint32_t log_n, uint32_t size_q, const uint64_t* q, uint64_t t,
                                int technique, const ofhe_bfv_decrypt_tables* tables, ofhe_bfv_decrypt_t* handle);
int ofhe_hip_bfv_decrypt_destroy(ofhe_bfv_decrypt_t handle);
/* The loop the handle runs: 0..7 for A..H (dcrtpoly-impl.h:1547-1803),
 * OFHE_BFV_DECRYPT_BEHZ, or OFHE_BFV_DECRYPT_ONE_TOWER when size_q == 1. */
int ofhe_hip_bfv_decrypt_branch(ofhe_bfv_decrypt_t handle, int* branch);
/* DCRTPolyImpl::ScaleAndRound to a NativePoly mod t (dcrtpoly-impl.h:1537-1814
 * for the HPS family, 2005-2049 for BEHZ; bfvrns-pke.cpp:233-245 when size_q ==
 * 1): x [batch][size_q][N] in coefficient form -> out [batch][N].  One kernel,
 * one thread per (batch entry, coefficient): (size_q + 1) * 8 bytes move per
 * coefficient. */
int ofhe_hip_bfv_decrypt_scale_round(ofhe_bfv_decrypt_t handle, const uint64_t* x, uint64_t* out, uint32_t batch,
                                     void* stream);
/* PKEBFVRNS::Decrypt (bfvrns-pke.cpp:205-248) with PKERNS::DecryptCore
 * (rns-pke.cpp:199-224): `elements` (2 or 3) ciphertext elements c0, c1 (, c2),
 * each [batch][size_q][N], all in evaluation form (eval_form != 0) or all in
 * coefficient form (as ofhe_hip_bfv_eval_mult leaves them), and the secret key
 * s [size_q][N] in evaluation form, shared by the batch -> out [batch][N].
 * Coefficient-form elements are transformed first; one launch forms
 * b = c0 + c1 s (+ c2 s^2) towerwise with canonical results (s^2 in the
 * kernel); INTT through plan_q; the scale-round kernel.  The ciphertext must
 * have as many towers as the key (what ofhe_hip_bfv_eval_mult_leveled and
 * ofhe_hip_bfv_relinearize_leveled return has: they lift to Q).  plan_q must
 * transform exactly the handle's towers at its N in its context.  Scratch
 * comes from the context's stream-ordered pool. */
int ofhe_hip_bfv_decrypt(ofhe_bfv_decrypt_t handle, ofhe_plan_t plan_q, uint32_t elements, int eval_form,
                         const uint64_t* c0, const uint64_t* c1, const uint64_t* c2, const uint64_t* s, uint64_t* out,
                         uint32_t batch, void* stream);
/* DCRTPolyImpl::TimesQovert (dcrtpoly-impl.h:1015-1031): out_i =
 * ((x_i negQModt) mod t) tInvModq[i] mod q_i over [batch][size_q][N], canonical
 * for any 64-bit x_i; out may be x.  OFHE_ERR_STATE when the handle was created
 * without tInvModq / negQModt. */
int ofhe_hip_times_q_over_t(ofhe_bfv_decrypt_t handle, const uint64_t* x, uint64_t* out, uint32_t batch, void* stream);

/* ---- BGV decryption and the CKKS / generic decryption core: PKEBGVRNS::Decrypt
 *      (pke/lib/scheme/bgvrns/bgvrns-pke.cpp:44-99), PKECKKSRNS::Decrypt
 *      (ckksrns-pke.cpp:44-97) and PKERNS::Decrypt (rns-pke.cpp:70-109), so that
 *      only the plaintext crosses the bus.  Integers only, bit-exact with the
 *      reference's NATIVEINT == 64 build.
 *
 * The handle builds negtInvModq[j] = q_j - t^-1 mod q_j and qlInvModq[j][i] =
 * q_j^-1 mod q_i, i < j (bgvrns-cryptoparameters.cpp:91-107), with their
 * preconditioners, from the moduli, as ofhe_hip_ks_rescale does; create uploads
 * once and waits (it cannot run under stream capture) and returns OFHE_ERR_ARG
 * -- before it looks at ctx -- for t < 2, size_q of 0 or above
 * OFHE_BGV_DECRYPT_MAX_TOWERS, a modulus that is even or not below 2^60, a
 * repeated modulus (or one not invertible modulo an earlier one), or t not
 * invertible modulo some q_j, j >= 1 (q_0 is never divided out, so t may share
 * a factor with it).  Every other call is stream-ordered and never
 * synchronises. */
#define OFHE_BGV_DECRYPT_MAX_TOWERS 64
typedef struct ofhe_bgv_decrypt_s* ofhe_bgv_decrypt_t;
int ofhe_hip_bgv_decrypt_create(ofhe_ctx_t ctx, uint32_t log_n, uint32_t size_q, const uint64_t* q, uint64_t t,
                                ofhe_bgv_decrypt_t* handle);
int ofhe_hip_bgv_decrypt_destroy(ofhe_bgv_decrypt_t handle);
/* The ModReduce chain Q_l -> q_0 of bgvrns-pke.cpp:55-60 / 74-81 on a
 * polynomial in coefficient form, x [batch][size_ql][N] over q[0..size_ql) ->
 * out [batch][N], 1 <= size_ql <= size_q.  Per coefficient, for j = size_ql - 1
 * down to 1 (DCRTPolyImpl::ModReduce, dcrtpoly-impl.h:792-812):
 *   delta = x_j negtInvModq[j] mod q_j
 *   x_i   = (x_i + SwitchModulus(delta, q_j -> q_i) (t mod q_i) mod q_i) qlInvModq[j][i] mod q_i,  i < j
 * with SwitchModulus as ofhe_hip_switch_modulus (mubintvecnat.cpp:111-136).
 * to_plaintext == 0: out is x_0, canonical mod q_0.  Otherwise out is
 * NativeVectorT::Mod(t) of it (mubintvecnat.cpp:139-166), which is
 * PolyImpl::DecryptionCRTInterpolate (poly-impl.h:566-575) on one tower:
 * 1 & (x ^ (x > q_0 >> 1)) for t == 2 (ModByTwoEq, :379-384); x + (t - q_0) above
 * q_0 >> 1 for t > q_0; else x + (t - q_0 mod t) above q_0 >> 1, then % t when
 * >= t.  size_ql == 1 is the ending alone.  One kernel launch per 8 towers
 * retired, one thread per (batch entry, coefficient): (size_ql + 1) * 8 bytes
 * move per coefficient up to 9 towers.  out may not overlap x; buffers are
 * 16-byte aligned; scratch (past 9 towers) comes from the context's
 * stream-ordered pool. */
int ofhe_hip_bgv_mod_reduce_chain(ofhe_bgv_decrypt_t handle, uint32_t size_ql, int to_plaintext, const uint64_t* x,
                                  uint64_t* out, uint32_t batch, void* stream);
/* PKEBGVRNS::Decrypt (bgvrns-pke.cpp:44-99) of `elements` (2 or 3) ciphertext
 * elements c0, c1 (, c2), each [batch][size_ql][N] over q[0..size_ql), and the
 * secret key s [size_q][N] in evaluation form over the full chain, shared by
 * the batch; its first size_ql towers are what DecryptCore's DropLastElements
 * leaves (rns-pke.cpp:199-224).  out [batch][N], words mod t.  The reference's
 * two branches produce different intermediate words and both are kept:
 *   eval_form != 0 (:52-60): one launch forms b = c0 + c1 s (+ c2 s^2) on
 *     size_ql towers, INTT of those towers, the chain with to_plaintext;
 *   eval_form == 0 (:72-93): the chain without the ending on each element,
 *     then DecryptCore on tower 0 alone (forward NTT of the reduced elements,
 *     the product with s_0, INTT), then Mod t.
 * plan_q must transform exactly the handle's towers at its N in its context.
 * The scaling factor the reference returns is host arithmetic on the caller's
 * factors (bgvrns-pke.cpp:62-69, 82-89) and stays with the caller. */
int ofhe_hip_bgv_decrypt(ofhe_bgv_decrypt_t handle, ofhe_plan_t plan_q, uint32_t size_ql, uint32_t elements,
                         int eval_form, const uint64_t* c0, const uint64_t* c1, const uint64_t* c2, const uint64_t* s,
                         uint64_t* out, uint32_t batch, void* stream);
/* PKERNS::DecryptCore (rns-pke.cpp:199-224) over the first size_ql towers of
 * plan: b = c0 + c1 s (+ c2 s^2), elements [batch][size_ql][N] all in
 * evaluation form (eval_form != 0) or all in coefficient form (transformed
 * first, as the reference does), s [>= size_ql][N] in evaluation form.
 * coeff_out != 0 adds b.SetFormat(COEFFICIENT) on all size_ql towers, which is
 * PKECKKSRNS::Decrypt (ckksrns-pke.cpp:44-97) and PKERNS::Decrypt (rns-pke.cpp:
 * 70-109) up to their last line: for size_ql == 1 out is the NativePoly; for
 * more towers the caller's CRTInterpolate of out stays on the host (big
 * integers are out of scope).  CKKS noise flooding (ckksrns-pke.cpp:49-54) is
 * sampling and stays with the caller: coeff_out == 0 returns b in evaluation
 * form for it to add to.  out [batch][size_ql][N] may be c0 itself; any other
 * overlap is refused.  The first call on a plan uploads q and floor(2^128 / q)
 * and waits; later calls never synchronise. */
int ofhe_hip_decrypt_core(ofhe_plan_t plan, uint32_t size_ql, uint32_t elements, int eval_form, int coeff_out,
                          const uint64_t* c0, const uint64_t* c1, const uint64_t* c2, const uint64_t* s, uint64_t* out,
                          uint32_t batch, void* stream);

/* ---- multi-GPU: evaluation-key broadcast over RCCL (xGMI) ----
 * the path shards by ciphertext batch with no exchange;
 * the one collective is the broadcast of the key-switching keys from a root
 * GPU (the keys the HYBRID core reads, keyswitch-hybrid.cpp:452-478).  The
 * reference is single-device (PimManager.h:21-127 drives one DPU set), so
 * this has no reference counterpart beyond "the key is in device memory".
 * One communicator per (process, device); the 128-byte id from rank 0's
 * ofhe_hip_comm_unique_id travels to the other ranks out of band. */
#define OFHE_COMM_ID_BYTES 128
typedef struct ofhe_comm_s* ofhe_comm_t;
int ofhe_hip_comm_unique_id(void* id /* OFHE_COMM_ID_BYTES */);
/* Collective over all nranks processes (blocks until they have all joined). */
int ofhe_hip_comm_init(ofhe_ctx_t ctx, int nranks, int rank, const void* id, ofhe_comm_t* out);
int ofhe_hip_comm_destroy(ofhe_comm_t comm);
/* In-place broadcast of `words` u64 of device memory from rank `root`:
 * the root's key is read, every other rank's buffer is overwritten.  Enqueued
 * on `stream` (ncclBroadcast); all ranks must call it with the same words. */
int ofhe_hip_bcast_evalkey(ofhe_comm_t comm, uint64_t* key, size_t words, int root, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OFHE_HIP_H */
