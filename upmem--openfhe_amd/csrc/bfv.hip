// bfv.hip -- BFV (HPS family) multiplication on gfx950, composed from the
// transforms, the tensor product, the base conversions and the kernels of
// bfv_kernels.hpp.
//
// Reference call stacks restated here (one launch per step covers the batch):
//   DCRTPolyImpl::ExpandCRTBasis             dcrtpoly-impl.h:1311-1358
//   DCRTPolyImpl::FastExpandCRTBasisPloverQ  dcrtpoly-impl.h:1413-1466
//   DCRTPolyImpl::ScaleAndRound              dcrtpoly-impl.h:1876-1955
//   LeveledSHEBFVRNS::EvalMult               bfvrns-leveledshe.cpp:168-408 (HPS, HPSPOVERQ)
#include <cstring>
#include <new>

#include "compose.hpp"

using namespace ofhe;

struct ofhe_bfv_mult_s {
    ofhe_ctx_t ctx = nullptr;
    u32 technique = 0;
    ofhe_plan_t plan_q = nullptr, plan_r = nullptr, plan_qr = nullptr;
    ofhe_bconv_t q_to_r = nullptr, r_to_q = nullptr, q_to_r_neg = nullptr;
    ofhe_scale_round_t sr = nullptr;
};

namespace {

int expand_check(ofhe_plan_t pq, ofhe_plan_t pp, ofhe_bconv_t bc) {
    if (!pq || !pp || !bc || !pq->ctx || !pp->ctx || !bc->ctx) return fail(OFHE_ERR_STATE, "NULL or destroyed object");
    if (pq->log_n != pp->log_n || bc->args.log_n != pq->log_n) return fail(OFHE_ERR_ARG, "ring dimensions differ");
    if (bc->args.size_q != pq->towers || bc->args.size_p != pp->towers || bc->hq != pq->q || bc->hp != pp->q)
        return fail(OFHE_ERR_ARG, "base converter does not map plan_q's towers to plan_p's");
    return OFHE_OK;
}

}  // namespace

namespace ofhe {

// ExpandCRTBasis with resultFormat = EVALUATION, in the reference's order:
// INTT of an evaluation-form input (1320-1323), exact switch Q -> P
// (1325-1326), NTT of the P towers (1338-1341), and the Q towers either the
// caller's evaluation-form words copied (1346-1349) or their NTT (1351-1355).
// The switch and the transforms stay separate launches: the fused conversion +
// column pass (k_bconv_cols) hands lazy values to the NTT, the exact switch's
// ModSubFast needs the canonical ones.
int expand_run(ofhe_plan_t pq, ofhe_plan_t pp, ofhe_bconv_t bc, int eval_form, const u64* x, u64* out, u32 batch,
               hipStream_t s) {
    auto convert = [&](const u64* src, u64 sstride, u64* dst, u64 dstride) {
        BconvArgs B = bc->args;
        B.in_stride = sstride;
        B.out_stride = dstride;
        RCCHK(switch_exact_run(bc, B, src, dst, batch, s));
        return plan_ntt_range(pp, false, 0, pp->towers, dst, dst, dstride, dstride, batch, s);
    };
    return expand_skeleton(pq, pq->towers, pp->towers, eval_form, x, out, batch, s, convert);
}

int sr_run(ofhe_scale_round_t h, const u64* x, u64* out, u32 batch, hipStream_t s) {
    dim3 g;
    RCCHK(coeff_grid((u64)batch << h->args.log_n, &g));
    hipLaunchKernelGGL((k_scale_round<4>), g, dim3(256), 0, s, h->args, x, out, batch);
    return post_launch();
}

}  // namespace ofhe

int ofhe_hip_expand_crt_basis(ofhe_plan_t pq, ofhe_plan_t pp, ofhe_bconv_t bc, int eval_form, const uint64_t* x,
                              uint64_t* out, uint32_t batch, void* stream) {
    RCCHK(expand_check(pq, pp, bc));
    if (!x || !out || batch == 0) return fail(OFHE_ERR_ARG, "bad data argument");
    if (pp->ctx != pq->ctx || bc->ctx != pq->ctx) return fail(OFHE_ERR_ARG, "objects of different contexts");
    // the INTT of an evaluation-form input goes through out's Q slots and x is read again at the end
    const u64 bn = (u64)batch << pq->log_n;
    if (words_overlap(x, bn * pq->towers, out, bn * (pq->towers + pp->towers)))
        return fail(OFHE_ERR_ARG, "out overlaps x");
    HIPCHK(hipSetDevice(pq->ctx->device));
    return expand_run(pq, pp, bc, eval_form, x, out, batch, pick(stream));
}

int ofhe_hip_scale_round_create(ofhe_ctx_t ctx, uint32_t log_n, uint32_t size_q, uint32_t size_p, const uint64_t* q,
                                const uint64_t* p, int out_is_q, const uint64_t* int_table, const double* frac,
                                ofhe_scale_round_t* out) {
    if (!ctx || !q || !p || !int_table || !frac || !out) return fail(OFHE_ERR_ARG, "NULL argument");
    if (log_n < 1 || log_n > 17) return fail(OFHE_ERR_ARG, "log_n must be in [1, 17]");
    if (size_q < 1 || size_p < 1 || size_q > 256 || size_p > 256)
        return fail(OFHE_ERR_ARG, "size_q and size_p must be in [1, 256]");
    if (out_is_q != 0 && out_is_q != 1) return fail(OFHE_ERR_ARG, "out_is_q must be 0 or 1");
    for (u32 i = 0; i < size_q; i++)
        if (q[i] < 2 || q[i] >= (1ull << 60)) return fail(OFHE_ERR_ARG, "q out of range");
    for (u32 j = 0; j < size_p; j++)
        if (p[j] < 2 || p[j] >= (1ull << 60)) return fail(OFHE_ERR_ARG, "p out of range");
    const u32 si = out_is_q ? size_p : size_q, so = out_is_q ? size_q : size_p;
    const u64* o = out_is_q ? q : p;
    // size_i + 1 products below 2^120 must fit the 128-bit accumulator (the
    // reference's DoubleNativeInt has the same limit)
    if (si > 255) return fail(OFHE_ERR_ARG, "at most 255 summed towers");
    for (u32 j = 0; j < so; j++)  // barrett128
        if (!(o[j] & 1)) return fail(OFHE_ERR_ARG, "output moduli must be odd");
    // the fractional parts are quotients (X mod s_i) / s_i: in [0, 1), which
    // keeps nu below 2^69 for 256 towers (floor_u128 takes nu < 2^127)
    for (u32 i = 0; i < si; i++)
        if (!(frac[i] >= 0.0 && frac[i] < 1.0)) return fail(OFHE_ERR_ARG, "frac must be in [0, 1)");
    // layout: tab[so][si + 1] | frac[si] | ov[so] | omu[so][2]
    const size_t row = (size_t)si + 1;
    std::vector<u64> h(so * row + si + 3 * (size_t)so);
    for (u32 j = 0; j < so; j++)
        for (u32 i = 0; i <= si; i++) h[j * row + i] = int_table[j * row + i] % o[j];
    std::memcpy(h.data() + so * row, frac, si * sizeof(double));
    u64* ov = h.data() + so * row + si;
    u64* omu = ov + so;
    for (u32 j = 0; j < so; j++) {
        ov[j] = o[j];
        barrett128(o[j], omu + 2 * j);
    }
    ofhe_scale_round_s* r = nullptr;
    RCCHK(create_with_table(&r, &ofhe_scale_round_s::d_mem, h, ctx->device, "scale-and-round allocation failed",
                            "scale-and-round upload"));
    r->ctx = ctx;
    r->size_q = size_q;
    r->size_p = size_p;
    r->out_is_q = (u32)out_is_q;
    SrArgs& A = r->args;
    A.tab = r->d_mem;
    A.frac = reinterpret_cast<const double*>(r->d_mem + so * row);
    A.ov = r->d_mem + so * row + si;
    A.omu = A.ov + so;
    A.log_n = log_n;
    A.size_i = si;
    A.size_o = so;
    // Q towers first: HPS sums the Q towers and takes the own tower from the
    // P part; HPSPOVERQ sums the P towers and takes the own tower from Q
    A.in0 = out_is_q ? size_q : 0;
    A.own0 = out_is_q ? 0 : size_q;
    *out = r;
    return OFHE_OK;
}

int ofhe_hip_scale_round_destroy(ofhe_scale_round_t h) {
    return destroy_with_table(h, &ofhe_scale_round_s::d_mem, "scale-and-round handle is NULL");
}

int ofhe_hip_scale_and_round(ofhe_scale_round_t h, const uint64_t* x, uint64_t* out, uint32_t batch, void* stream) {
    RCCHK(live(h, "scale-and-round handle is NULL or destroyed"));
    if (!x || !out || batch == 0) return fail(OFHE_ERR_ARG, "bad data argument");
    HIPCHK(hipSetDevice(h->ctx->device));
    return sr_run(h, x, out, batch, pick(stream));
}

int ofhe_hip_bfv_mult_create(ofhe_ctx_t ctx, int technique, ofhe_plan_t plan_q, ofhe_plan_t plan_r,
                             ofhe_plan_t plan_qr, ofhe_bconv_t q_to_r, ofhe_bconv_t r_to_q, ofhe_bconv_t q_to_r_neg,
                             ofhe_scale_round_t scale_round, ofhe_bfv_mult_t* out) {
    if (!ctx || !out) return fail(OFHE_ERR_ARG, "NULL argument");
    if (technique != OFHE_BFV_HPS && technique != OFHE_BFV_HPSPOVERQ)
        return fail(OFHE_ERR_ARG, "technique is not an OFHE_BFV_* value");
    if (!plan_qr || !plan_qr->ctx || !r_to_q || !r_to_q->ctx || !scale_round || !scale_round->ctx)
        return fail(OFHE_ERR_STATE, "NULL or destroyed object");
    RCCHK(expand_check(plan_q, plan_r, q_to_r));
    RCCHK(expand_check(plan_r, plan_q, r_to_q));
    for (ofhe_ctx_t c : {plan_q->ctx, plan_r->ctx, plan_qr->ctx, q_to_r->ctx, r_to_q->ctx, scale_round->ctx,
                         q_to_r_neg ? q_to_r_neg->ctx : ctx})
        if (c != ctx) return fail(OFHE_ERR_ARG, "every composed handle must belong to ctx");
    const u32 Q = plan_q->towers, R = plan_r->towers;
    if (plan_qr->log_n != plan_q->log_n || !plan_towers_are(plan_qr, {&plan_q->q, &plan_r->q}))
        return fail(OFHE_ERR_ARG, "plan_qr is not plan_q's towers followed by plan_r's");
    if (scale_round->args.log_n != plan_q->log_n || scale_round->size_q != Q || scale_round->size_p != R)
        return fail(OFHE_ERR_ARG, "scale-and-round handle does not match the bases");
    if (technique == OFHE_BFV_HPS) {
        if (q_to_r_neg) return fail(OFHE_ERR_ARG, "q_to_r_neg must be NULL for HPS");
        if (scale_round->out_is_q) return fail(OFHE_ERR_ARG, "HPS needs a scale-and-round handle with out_is_q = 0");
    } else {
        if (R != Q) return fail(OFHE_ERR_ARG, "HPSPOVERQ needs size_r == size_q");
        RCCHK(expand_check(plan_q, plan_r, q_to_r_neg));
        if (!scale_round->out_is_q) return fail(OFHE_ERR_ARG, "HPSPOVERQ needs a scale-and-round handle with out_is_q = 1");
    }
    ofhe_bfv_mult_s* m = new (std::nothrow) ofhe_bfv_mult_s();
    if (!m) return fail(OFHE_ERR_NOMEM, "bfv mult allocation failed");
    m->ctx = ctx;
    m->technique = (u32)technique;
    m->plan_q = plan_q;
    m->plan_r = plan_r;
    m->plan_qr = plan_qr;
    m->q_to_r = q_to_r;
    m->r_to_q = r_to_q;
    m->q_to_r_neg = q_to_r_neg;
    m->sr = scale_round;
    *out = m;
    return OFHE_OK;
}

int ofhe_hip_bfv_mult_destroy(ofhe_bfv_mult_t h) {
    if (!h) return fail(OFHE_ERR_ARG, "bfv mult handle is NULL");
    delete h;
    return OFHE_OK;
}

int ofhe_hip_bfv_eval_mult(ofhe_bfv_mult_t h, const uint64_t* c0, const uint64_t* c1, const uint64_t* d0,
                           const uint64_t* d1, uint64_t* out0, uint64_t* out1, uint64_t* out2, uint32_t batch,
                           void* stream) {
    RCCHK(live(h, "bfv mult handle is NULL or destroyed"));
    if (!c0 || !c1 || !d0 || !d1 || !out0 || !out1 || !out2 || batch == 0)
        return fail(OFHE_ERR_ARG, "bad data argument");
    if ((u64)batch * 4 >= (1ull << 32)) return fail(OFHE_ERR_ARG, "batch too large");
    HIPCHK(hipSetDevice(h->ctx->device));
    hipStream_t s = pick(stream);
    ofhe_plan_t pq = h->plan_q, pr = h->plan_r, pqr = h->plan_qr;
    const u64 N = 1ull << pq->log_n, Q = pq->towers, R = pr->towers, qr = (Q + R) * N;
    const u64 one = (u64)batch * qr;  // words of one expanded polynomial over the batch
    // scratch: E | T (compose.hpp: the four expanded inputs, the three products), (HPS) the products' R parts
    const bool hps = h->technique == OFHE_BFV_HPS;
    Scratch sc;
    RCCHK(sc.alloc((7 * one + (hps ? 3 * (u64)batch * R * N : 0)) * sizeof(u64), s, h->ctx));
    u64* E = sc.w();
    u64* T = E + 4 * one;
    u64* S = T + 3 * one;
    // cv1[i].ExpandCRTBasis (bfvrns-leveledshe.cpp:192-198, 208-215)
    RCCHK(expand_run(pq, pr, h->q_to_r, 1, c0, E, batch, s));
    RCCHK(expand_run(pq, pr, h->q_to_r, 1, c1, E + one, batch, s));
    const u64* dd[2] = {d0, d1};
    for (int k = 0; k < 2; k++) {
        u64* Ek = E + (2 + k) * one;
        if (hps) {
            RCCHK(expand_run(pq, pr, h->q_to_r, 1, dd[k], Ek, batch, s));  // 200-206
            continue;
        }
        // SetFormat(COEFFICIENT), FastExpandCRTBasisPloverQ, SetFormat(EVALUATION) (228-232):
        // the coefficient form goes to the Q slots, which the exact switch R -> Q then replaces
        RCCHK(plan_ntt_range(pq, true, 0, (u32)Q, dd[k], Ek, Q * N, qr, batch, s));
        RCCHK(fast_expand_p_over_q(h->q_to_r_neg, h->r_to_q, pqr, Ek, qr, Ek, batch, s));
    }
    // the tensor product over Q|R (316-330; EvalMultCore's three outputs), cvMult[i].SetFormat(COEFFICIENT) (342, 356)
    RCCHK(tensor_and_intt(pqr, E, T, one, batch, stream));
    u64* outs[3] = {out0, out1, out2};
    if (hps) {
        // ScaleAndRound to R (343-345), SwitchCRTBasis R -> Q (347-350)
        RCCHK(sr_run(h->sr, T, S, 3 * batch, s));
        for (int k = 0; k < 3; k++)
            RCCHK(switch_exact_run(h->r_to_q, h->r_to_q->args, S + (u64)k * batch * R * N, outs[k], batch, s));
    } else {
        // ScaleAndRound to Q (357-359)
        for (int k = 0; k < 3; k++) RCCHK(sr_run(h->sr, T + k * one, outs[k], batch, s));
    }
    return OFHE_OK;
}
