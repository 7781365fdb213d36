// bfv_leveled.hip -- BFV multiplication and relinearisation by HPSPOVERQLEVELED
// with dropped levels on gfx950, composed from the transforms, the tensor
// product, the base conversions, ScaleAndRound, the HYBRID key switch and the
// kernels of bfv_leveled_kernels.hpp.
//
// Reference call stacks restated here (one launch per step covers the batch):
//   LeveledSHEBFVRNS::EvalMult, HPSPOVERQLEVELED  bfvrns-leveledshe.cpp:235-274, 316-330, 367-382
//   LeveledSHEBFVRNS::EvalSquare                  bfvrns-leveledshe.cpp:459-499
//   LeveledSHEBFVRNS::RelinearizeCore             bfvrns-leveledshe.cpp:845-899
//   DCRTPolyImpl::FastExpandCRTBasisPloverQ       dcrtpoly-impl.h:1413-1466
//   DCRTPolyImpl::ExpandCRTBasisQlHat             dcrtpoly-impl.h:1514-1534
//   DCRTPolyImpl::ScaleAndRound                   dcrtpoly-impl.h:1876-1955
#include <algorithm>

#include "compose.hpp"
#include "bfv_leveled_kernels.hpp"

using namespace ofhe;

struct ofhe_bfv_level_s {
    ofhe_ctx_t ctx = nullptr;
    u32 l = 0, size_q = 0, log_n = 0;
    ofhe_plan_t plan_q = nullptr, plan_ql = nullptr, plan_rl = nullptr, plan_qlrl = nullptr;
    ofhe_bconv_t ql_to_rl = nullptr, rl_to_ql = nullptr, q_to_rl_neg = nullptr;
    ofhe_scale_round_t drop = nullptr, sr = nullptr;
    u64* d_tab = nullptr;  // [l + 1][3]: q_i, QlHatModq_i, its Shoup precon
    QlHatArgs args{};
};

namespace {

int level_ok(ofhe_bfv_level_t h, u32 batch) {
    RCCHK(live(h, "bfv level handle is NULL or destroyed"));
    if (batch == 0 || (u64)batch * 4 >= (1ull << 32)) return fail(OFHE_ERR_ARG, "batch must be in [1, 2^30)");
    return OFHE_OK;
}

int ql_hat_run(ofhe_bfv_level_t h, const u64* x, const u64* addend, u64* out, u32 batch, hipStream_t s) {
    const u64 half = (1ull << h->log_n) / 2;
    const u32 bpr = (u32)((half + 255) / 256);
    // out == addend: the towers past l are in place already
    const u32 rt = addend == out ? h->l + 1 : h->size_q;
    dim3 g;
    RCCHK(coeff_grid((u64)batch * rt * bpr * 256, &g));
    hipLaunchKernelGGL(k_expand_ql_hat, g, dim3(256), 0, s, h->args, x, addend, out, bpr, rt);
    return post_launch();
}

int sr_lift_run(ofhe_bfv_level_t h, const u64* x, u64* out, u32 batch, hipStream_t s) {
    dim3 g;
    RCCHK(coeff_grid((u64)batch << h->log_n, &g));
    hipLaunchKernelGGL((k_scale_round_lift<4>), g, dim3(256), 0, s, h->sr->args, h->args, x, out, batch);
    return post_launch();
}

}  // namespace

int ofhe_hip_bfv_level_create(ofhe_ctx_t ctx, uint32_t l, ofhe_plan_t plan_q, ofhe_plan_t plan_ql, ofhe_plan_t plan_rl,
                              ofhe_plan_t plan_qlrl, ofhe_bconv_t ql_to_rl, ofhe_bconv_t rl_to_ql,
                              ofhe_bconv_t q_to_rl_neg, ofhe_scale_round_t drop, ofhe_scale_round_t scale_round,
                              const uint64_t* ql_hat_modq, ofhe_bfv_level_t* out) {
    if (!ctx || !out || !ql_hat_modq) return fail(OFHE_ERR_ARG, "NULL argument");
    if (!plan_q || !plan_ql || !plan_rl || !plan_qlrl || !ql_to_rl || !rl_to_ql || !q_to_rl_neg || !scale_round)
        return fail(OFHE_ERR_STATE, "NULL object");
    if (!plan_q->ctx || !plan_ql->ctx || !plan_rl->ctx || !plan_qlrl->ctx || !ql_to_rl->ctx || !rl_to_ql->ctx ||
        !q_to_rl_neg->ctx || !scale_round->ctx || (drop && !drop->ctx))
        return fail(OFHE_ERR_STATE, "destroyed object");
    for (ofhe_ctx_t c : {plan_q->ctx, plan_ql->ctx, plan_rl->ctx, plan_qlrl->ctx, ql_to_rl->ctx, rl_to_ql->ctx,
                         q_to_rl_neg->ctx, scale_round->ctx, drop ? drop->ctx : ctx})
        if (c != ctx) return fail(OFHE_ERR_ARG, "every composed handle must belong to ctx");
    const u32 Q = plan_q->towers, L = l + 1, log_n = plan_q->log_n;
    if (l >= Q) return fail(OFHE_ERR_ARG, "l must be in [0, size_q - 1]");
    if (plan_ql->log_n != log_n || plan_rl->log_n != log_n || plan_qlrl->log_n != log_n ||
        ql_to_rl->args.log_n != log_n || rl_to_ql->args.log_n != log_n || q_to_rl_neg->args.log_n != log_n ||
        scale_round->args.log_n != log_n || (drop && drop->args.log_n != log_n))
        return fail(OFHE_ERR_ARG, "ring dimensions differ");
    if (plan_ql->towers != L || plan_rl->towers != L) return fail(OFHE_ERR_ARG, "plan_ql and plan_rl must have l + 1 towers");
    if (!std::equal(plan_ql->q.begin(), plan_ql->q.end(), plan_q->q.begin()))
        return fail(OFHE_ERR_ARG, "plan_ql is not a prefix of plan_q");
    if (!plan_towers_are(plan_qlrl, {&plan_ql->q, &plan_rl->q}))
        return fail(OFHE_ERR_ARG, "plan_qlrl is not plan_ql's towers followed by plan_rl's");
    if (ql_to_rl->hq != plan_ql->q || ql_to_rl->hp != plan_rl->q)
        return fail(OFHE_ERR_ARG, "ql_to_rl does not map plan_ql's towers to plan_rl's");
    if (rl_to_ql->hq != plan_rl->q || rl_to_ql->hp != plan_ql->q)
        return fail(OFHE_ERR_ARG, "rl_to_ql does not map plan_rl's towers to plan_ql's");
    if (q_to_rl_neg->hq != plan_q->q || q_to_rl_neg->hp != plan_rl->q)
        return fail(OFHE_ERR_ARG, "q_to_rl_neg does not map plan_q's towers to plan_rl's");
    if (scale_round->size_q != L || scale_round->size_p != L || !scale_round->out_is_q)
        return fail(OFHE_ERR_ARG, "scale_round must have size_q = size_p = l + 1 and out_is_q = 1");
    if (L == Q) {
        if (drop) return fail(OFHE_ERR_ARG, "drop must be NULL at l = size_q - 1");
    } else {
        if (!drop) return fail(OFHE_ERR_ARG, "drop is NULL below the full level");
        if (drop->size_q != L || drop->size_p != Q - L || !drop->out_is_q)
            return fail(OFHE_ERR_ARG, "drop must have size_q = l + 1, size_p = size_q - l - 1 and out_is_q = 1");
    }
    std::vector<u64> tab(3 * (size_t)L);
    for (u32 i = 0; i < L; i++) {
        const u64 q = plan_q->q[i];
        if (ql_hat_modq[i] >= q) return fail(OFHE_ERR_ARG, "ql_hat_modq is not below its modulus");
        tab[3 * i] = q;
        tab[3 * i + 1] = ql_hat_modq[i];
        tab[3 * i + 2] = shoup_pre(ql_hat_modq[i], q);
    }
    ofhe_bfv_level_s* h = nullptr;
    RCCHK(create_with_table(&h, &ofhe_bfv_level_s::d_tab, tab, ctx->device, "bfv level allocation failed",
                            "bfv level upload"));
    h->ctx = ctx;
    h->l = l;
    h->size_q = Q;
    h->log_n = log_n;
    h->plan_q = plan_q;
    h->plan_ql = plan_ql;
    h->plan_rl = plan_rl;
    h->plan_qlrl = plan_qlrl;
    h->ql_to_rl = ql_to_rl;
    h->rl_to_ql = rl_to_ql;
    h->q_to_rl_neg = q_to_rl_neg;
    h->drop = drop;
    h->sr = scale_round;
    h->args = QlHatArgs{h->d_tab, log_n, L, Q};
    *out = h;
    return OFHE_OK;
}

int ofhe_hip_bfv_level_destroy(ofhe_bfv_level_t h) {
    return destroy_with_table(h, &ofhe_bfv_level_s::d_tab, "bfv level handle is NULL");
}

int ofhe_hip_expand_ql_hat(ofhe_bfv_level_t h, const uint64_t* x, const uint64_t* addend, uint64_t* out, uint32_t batch,
                           void* stream) {
    RCCHK(level_ok(h, batch));
    if (!x || !out) return fail(OFHE_ERR_ARG, "bad data argument");
    const u64 N = 1ull << h->log_n;
    if (words_overlap(x, (u64)batch * (h->l + 1) * N, out, (u64)batch * h->size_q * N))
        return fail(OFHE_ERR_ARG, "out overlaps x");
    if (addend && addend != out && words_overlap(addend, (u64)batch * h->size_q * N, out, (u64)batch * h->size_q * N))
        return fail(OFHE_ERR_ARG, "out overlaps addend without being addend");
    HIPCHK(hipSetDevice(h->ctx->device));
    return ql_hat_run(h, x, addend, out, batch, pick(stream));
}

int ofhe_hip_scale_round_expand_ql_hat(ofhe_bfv_level_t h, const uint64_t* x, uint64_t* out, uint32_t batch,
                                       void* stream) {
    RCCHK(level_ok(h, batch));
    if (!x || !out) return fail(OFHE_ERR_ARG, "bad data argument");
    const u64 N = 1ull << h->log_n;
    if (words_overlap(x, (u64)batch * 2 * (h->l + 1) * N, out, (u64)batch * h->size_q * N))
        return fail(OFHE_ERR_ARG, "out overlaps x");
    HIPCHK(hipSetDevice(h->ctx->device));
    return sr_lift_run(h, x, out, batch, pick(stream));
}

int ofhe_hip_bfv_eval_mult_leveled(ofhe_bfv_level_t h, const uint64_t* c0, const uint64_t* c1, const uint64_t* d0,
                                   const uint64_t* d1, uint64_t* out0, uint64_t* out1, uint64_t* out2, uint32_t batch,
                                   void* stream) {
    RCCHK(level_ok(h, batch));
    if (!c0 || !c1 || !d0 || !d1 || !out0 || !out1 || !out2) return fail(OFHE_ERR_ARG, "bad data argument");
    HIPCHK(hipSetDevice(h->ctx->device));
    hipStream_t s = pick(stream);
    ofhe_plan_t pq = h->plan_q, pql = h->plan_ql, prl = h->plan_rl, pqr = h->plan_qlrl;
    const u64 N = 1ull << h->log_n, Q = h->size_q, L = h->l + 1, qr = 2 * L * N;
    const bool dropped = L < Q;
    const u64 one = (u64)batch * qr;   // words of one expanded polynomial over the batch
    const u64 full = (u64)batch * Q * N;  // ... of one polynomial over Q
    // scratch: E | T (compose.hpp), the coefficient forms of d0, d1 over Q, and
    // below the full level those of c0, c1 and their images over Q_l
    Scratch sc;
    RCCHK(sc.alloc((7 * one + 2 * full + (dropped ? 2 * full + 2 * (u64)batch * L * N : 0)) * sizeof(u64), s, h->ctx));
    u64* E = sc.w();
    u64* T = E + 4 * one;
    u64* D = T + 3 * one;   // d0 | d1, coefficient form over Q
    u64* C = D + 2 * full;  // c0 | c1, coefficient form over Q
    u64* Cl = C + 2 * full; // c0 | c1 over Q_l
    if (!dropped) {
        // cv1[i].ExpandCRTBasis (255-258): nothing to drop
        RCCHK(expand_run(pql, prl, h->ql_to_rl, 1, c0, E, batch, s));
        RCCHK(expand_run(pql, prl, h->ql_to_rl, 1, c1, E + one, batch, s));
    } else {
        // SetFormat(COEFFICIENT) (247), ScaleAndRound Q -> Q_l (250-252), ExpandCRTBasis (255-258);
        // both elements as one batch from the drop on
        RCCHK(plan_ntt_range(pq, true, 0, (u32)Q, c0, C, Q * N, Q * N, batch, s));
        RCCHK(plan_ntt_range(pq, true, 0, (u32)Q, c1, C + full, Q * N, Q * N, batch, s));
        RCCHK(sr_run(h->drop, C, Cl, 2 * batch, s));
        RCCHK(expand_run(pql, prl, h->ql_to_rl, 0, Cl, E, 2 * batch, s));
    }
    // cv2[i]: SetFormat(COEFFICIENT), FastExpandCRTBasisPloverQ, SetFormat(EVALUATION) (268-273).
    // The approximate switch reads all size_q towers (mNegRlQHatInvModq(l)); both elements as one
    // batch after the transforms.
    RCCHK(plan_ntt_range(pq, true, 0, (u32)Q, d0, D, Q * N, Q * N, batch, s));
    RCCHK(plan_ntt_range(pq, true, 0, (u32)Q, d1, D + full, Q * N, Q * N, batch, s));
    RCCHK(fast_expand_p_over_q(h->q_to_rl_neg, h->rl_to_ql, pqr, D, Q * N, E + 2 * one, 2 * batch, s));
    // the tensor product over Q_l R_l (316-330), cvMult[i].SetFormat(COEFFICIENT) (369)
    RCCHK(tensor_and_intt(pqr, E, T, one, batch, stream));
    u64* outs[3] = {out0, out1, out2};
    for (int k = 0; k < 3; k++) {
        // ScaleAndRound to Q_l (372-374), and below the full level ExpandCRTBasisQlHat (376-380)
        // in the same launch (k_scale_round_lift)
        if (!dropped)
            RCCHK(sr_run(h->sr, T + k * one, outs[k], batch, s));
        else
            RCCHK(sr_lift_run(h, T + k * one, outs[k], batch, s));
    }
    return OFHE_OK;
}

int ofhe_hip_bfv_relinearize_leveled(ofhe_bfv_level_t h, ofhe_ks_t ks, uint32_t elements, int eval_form,
                                     const uint64_t* c0, const uint64_t* c1, const uint64_t* c2, const uint64_t* key_b,
                                     const uint64_t* key_a, uint64_t* out0, uint64_t* out1, uint32_t batch,
                                     void* stream) {
    RCCHK(level_ok(h, batch));
    if (!ks) return fail(OFHE_ERR_STATE, "key-switch handle is NULL");
    if (elements != 2 && elements != 3) return fail(OFHE_ERR_ARG, "elements must be 2 or 3");
    if (!c0 || !c1 || !key_b || !key_a || !out0 || !out1) return fail(OFHE_ERR_ARG, "bad data argument");
    if ((elements == 3) != (c2 != nullptr)) return fail(OFHE_ERR_ARG, "c2 must be given exactly when elements is 3");
    const u64 N = 1ull << h->log_n, Q = h->size_q, L = h->l + 1;
    const u64 full = (u64)batch * Q * N, low = (u64)batch * L * N;
    if (words_overlap(out0, full, out1, full)) return fail(OFHE_ERR_ARG, "out0 overlaps out1");
    for (const u64* in : {c0, c1, c2})
        for (const u64* o : {(const u64*)out0, (const u64*)out1})
            if (in && words_overlap(in, full, o, full)) return fail(OFHE_ERR_ARG, "an output overlaps an input");
    {
        // the engine must reach level l + 1 (its own check of size_ql)
        u32 beta = 0;
        RCCHK(ofhe_hip_ks_digits(ks, (u32)L, nullptr, &beta));
    }
    HIPCHK(hipSetDevice(h->ctx->device));
    hipStream_t s = pick(stream);
    const bool dropped = L < Q;
    const u64* last = elements == 3 ? c2 : c1;
    Scratch sc;
    RCCHK(sc.alloc((3 * low + (dropped && eval_form ? full : 0)) * sizeof(u64), s, h->ctx));
    u64* Dl = sc.w();       // the last element over Q_l, evaluation form
    u64* A0 = Dl + low;     // KeySwitchCore's results over Q_l
    u64* A1 = A0 + low;
    u64* C = A1 + low;      // the last element's coefficient form over Q
    const u64* kin = Dl;
    if (dropped) {
        // SetFormat(COEFFICIENT), ScaleAndRound Q -> Q_l (863-872), SetFormat(EVALUATION) (875-876)
        const u64* coef = last;
        if (eval_form) {
            RCCHK(plan_ntt_range(h->plan_q, true, 0, (u32)Q, last, C, Q * N, Q * N, batch, s));
            coef = C;
        }
        RCCHK(sr_run(h->drop, coef, Dl, batch, s));
        RCCHK(plan_ntt_range(h->plan_ql, false, 0, (u32)L, Dl, Dl, L * N, L * N, batch, s));
    } else if (eval_form) {
        kin = last;  // the drop tables of the full level scale by one
    } else {
        RCCHK(plan_ntt_range(h->plan_q, false, 0, (u32)Q, last, Dl, Q * N, Q * N, batch, s));
    }
    // KeySwitchCore at l + 1 towers (878-879)
    RCCHK(ofhe_hip_ks_core(ks, (u32)L, kin, key_b, key_a, A0, A1, 0, batch, stream));
    // ExpandCRTBasisQlHat of both results (881-887), cv[0] += ab[0], cv[1] += ab[1] or = ab[1] (889-896).
    // Coefficient-form c0 / c1 go through the NTT into the outputs, which then are their own addends.
    const u64* add0 = c0;
    const u64* add1 = elements == 3 ? c1 : nullptr;
    if (!eval_form) {
        RCCHK(plan_ntt_range(h->plan_q, false, 0, (u32)Q, c0, out0, Q * N, Q * N, batch, s));
        add0 = out0;
        if (add1) {
            RCCHK(plan_ntt_range(h->plan_q, false, 0, (u32)Q, c1, out1, Q * N, Q * N, batch, s));
            add1 = out1;
        }
    }
    RCCHK(ql_hat_run(h, A0, add0, out0, batch, s));
    return ql_hat_run(h, A1, add1, out1, batch, s);
}
