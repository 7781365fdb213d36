// compose.hpp -- the host skeleton shared by the translation units that
// compose kernels into BFV-family operations (keyswitch.hip, bfv.hip,
// bfv_leveled.hip, behz.hip, bfv_decrypt.hip, bgv_decrypt.hip): argument checks, handle
// boilerplate, launch grids and the launch sequences they have in common.
// Host code only, with internal linkage: nothing here is part of the C ABI or
// adds to the library's exported symbols.
#pragma once
#include <algorithm>
#include <initializer_list>
#include <new>

#include "internal.hpp"

namespace ofhe {
namespace {

// [a, a + an) and [b, b + bn) (words) overlap; compared as integers, so no
// pointer past the end of a buffer is formed
inline bool words_overlap(const u64* a, u64 an, const u64* b, u64 bn) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + 8 * bn && b0 < a0 + 8 * an;
}

// The 128-bit Barrett constant floor(2^128 / m) as (low, high) words, taken as
// floor((2^128 - 1) / m): equal unless m is a power of two (the callers' moduli are odd)
inline void barrett128(u64 m, u64 out[2]) {
    const u128 mu = (~(u128)0) / m;
    out[0] = (u64)mu;
    out[1] = (u64)(mu >> 64);
}

// every modulus odd, at least 3 (barrett128) and below 2^60 (the limb kernels)
inline int check_moduli(const u64* m, size_t n) {
    for (size_t i = 0; i < n; i++) {
        if (!(m[i] & 1) || m[i] < 3) return fail(OFHE_ERR_ARG, "every modulus must be odd");
        if (m[i] >= (1ull << 60)) return fail(OFHE_ERR_ARG, "every modulus must be below 2^60");
    }
    return OFHE_OK;
}

// p's towers are the concatenation of the given moduli lists
using TowerLists = std::initializer_list<const std::vector<u64>*>;
inline bool plan_towers_are(ofhe_plan_t p, TowerLists spans) {
    size_t at = 0;
    for (const std::vector<u64>* v : spans) {
        if (at + v->size() > p->q.size() || !std::equal(v->begin(), v->end(), p->q.begin() + at)) return false;
        at += v->size();
    }
    return at == p->q.size();
}
// ... and p (named `what` in the messages) is live, of this context and of this ring dimension
inline int plan_is(ofhe_plan_t p, ofhe_ctx_t ctx, u32 log_n, TowerLists spans, const char* what) {
    if (!p || !p->ctx) return fail(OFHE_ERR_STATE, std::string(what) + " is NULL or destroyed");
    if (p->ctx != ctx) return fail(OFHE_ERR_ARG, std::string(what) + " belongs to another context");
    if (p->log_n != log_n) return fail(OFHE_ERR_ARG, std::string(what) + ": ring dimension differs from the handle's");
    if (!plan_towers_are(p, spans)) return fail(OFHE_ERR_ARG, std::string(what) + ": towers differ from the handle's");
    return OFHE_OK;
}

// Grid of the kernels that run one thread per item, 256 a block (a launch over
// rows of whole blocks passes blocks * 256)
inline int coeff_grid(u64 items, dim3* g, const char* msg = "batch too large") {
    const u64 blocks = (items + 255) / 256;
    if (blocks >= (1ull << 31)) return fail(OFHE_ERR_ARG, msg);
    *g = dim3((u32)blocks);
    return OFHE_OK;
}

// Handle boilerplate: the liveness test of every entry point, and the create
// and destroy sequences of a handle that owns one device table (create leaves
// every other field, ctx included, to the caller)
template <class H>
inline int live(H* h, const char* msg) {
    return h && h->ctx ? OFHE_OK : fail(OFHE_ERR_STATE, msg);
}
template <class H>
inline int create_with_table(H** out, u64* H::*d_mem, const std::vector<u64>& words, int device, const char* nomem,
                             const char* upload) {
    H* h = new (std::nothrow) H();
    if (!h) return fail(OFHE_ERR_NOMEM, nomem);
    const int rc = alloc_upload(&(h->*d_mem), words.data(), words.size() * sizeof(u64), upload, device);
    if (rc == OFHE_OK) *out = h;
    else delete h;
    return rc;
}
template <class H>
inline int destroy_with_table(H* h, u64* H::*d_mem, const char* msg) {
    if (!h) return fail(OFHE_ERR_ARG, msg);
    if (h->ctx) (void)hipSetDevice(h->ctx->device);
    (void)hipFree(h->*d_mem);
    delete h;
    return OFHE_OK;
}

// The expansion x [batch][Q][N] -> out [batch][Q + K][N] in evaluation form
// common to ApproxModUp, ExpandCRTBasis and FastBaseConvqToBskMontgomery: the
// INTT of an evaluation-form input goes through out's Q slots,
// convert(src, src_stride, dst, dst_stride) fills the K new towers and
// transforms them, and the Q towers are the caller's evaluation-form words
// copied, or the NTT of its coefficient-form ones.
template <class Convert>
inline int expand_skeleton(ofhe_plan_t pq, u32 Q, u32 K, int eval_form, const u64* x, u64* out, u32 batch,
                           hipStream_t s, Convert&& convert) {
    const u64 N = 1ull << pq->log_n, qn = Q * N, all = (Q + K) * N;
    if (eval_form) RCCHK(plan_ntt_range(pq, true, 0, Q, x, out, qn, all, batch, s));
    RCCHK(convert(eval_form ? out : x, eval_form ? all : qn, out + qn, all));
    if (eval_form) return copy_rows(out, all, x, qn, qn, batch, s);
    return plan_ntt_range(pq, false, 0, Q, x, out, qn, all, batch, s);
}

// FastExpandCRTBasisPloverQ (dcrtpoly-impl.h:1413-1466) of coefficient-form x
// (batch stride xs) into E [batch][pqr's towers][N]: the approximate switch
// with the negated table (mNegRlQHatInvModq / qInvModr) fills the slots past
// `back`'s targets (1419-1441), the exact switch `back` fills the leading ones
// from them (1445-1460), then SetFormat(EVALUATION) over both bases.
inline int fast_expand_p_over_q(ofhe_bconv_t neg, ofhe_bconv_t back, ofhe_plan_t pqr, const u64* x, u64 xs, u64* E,
                                u32 batch, hipStream_t s) {
    const u64 N = 1ull << pqr->log_n, lead = back->args.size_p * N, qr = pqr->towers * N;
    BconvArgs B = neg->args;
    B.in_stride = xs;
    B.out_stride = qr;
    B.lazy_out = 0;
    RCCHK(bconv_run(B, x, E + lead, batch, s));
    BconvArgs X = back->args;
    X.in_stride = X.out_stride = qr;
    RCCHK(switch_exact_run(back, X, E + lead, E, batch, s));
    return plan_ntt_range(pqr, false, 0, pqr->towers, E, E, qr, qr, batch, s);
}

// The tail shared by the three multiplications, on the scratch prefix E | T
// (four expanded inputs, three products, `one` words each): the tensor product
// over the joined plan, then the products' SetFormat(COEFFICIENT) as one batch.
inline int tensor_and_intt(ofhe_plan_t pqr, const u64* E, u64* T, u64 one, u32 batch, void* stream) {
    RCCHK(ofhe_hip_eval_mult_core(pqr, E, E + one, E + 2 * one, E + 3 * one, T, T + one, T + 2 * one, batch, stream));
    const u64 w = (u64)pqr->towers << pqr->log_n;
    return plan_ntt_range(pqr, true, 0, pqr->towers, T, T, w, w, 3 * batch, pick(stream));
}

}  // namespace
}  // namespace ofhe
