// bfv_decrypt.hip -- BFV decryption and encryption scaling on gfx950: the
// kernels of bfv_decrypt_kernels.hpp composed with the transforms.
//
// Reference call stacks restated here (one launch per step covers the batch):
//   PKEBFVRNS::Decrypt                          bfvrns-pke.cpp:205-248
//   PKERNS::DecryptCore                         rns-pke.cpp:199-224
//   DCRTPolyImpl::ScaleAndRound -> NativePoly   dcrtpoly-impl.h:1537-1814 (HPS family), 2005-2049 (BEHZ)
//   NativeVectorT::MultiplyAndRound             mubintvecnat.cpp:420-435 (one tower)
//   DCRTPolyImpl::TimesQovert                   dcrtpoly-impl.h:1015-1031
#include <cstring>

#include "bfv_decrypt_kernels.hpp"
#include "compose.hpp"

using namespace ofhe;

struct ofhe_bfv_decrypt_s {
    ofhe_ctx_t ctx = nullptr;
    DecArgs args{};
    u64* d_mem = nullptr;
    int branch = 0;
    bool has_tqt = false;
    std::vector<u64> q;
};

namespace {

// the choice among the eight loops of dcrtpoly-impl.h:1547-1803
int dec_branch(u32 size_q, u64 q0, u64 t) {
    const unsigned qmsb = msb64(q0), tmsb = msb64(t), smsb = msb64(size_q), hf = qmsb >> 1;
    const bool pow2 = !(t & (t - 1));
    const bool split = qmsb + smsb >= 52;
    const unsigned bits = (split ? hf : qmsb) + tmsb + smsb;
    const bool reduced = bits >= (pow2 ? (split ? 62u : 63u) : 52u);
    return (pow2 ? 0 : 4) + (split ? 2 : 0) + (reduced ? 1 : 0);
}

int dec_live(ofhe_bfv_decrypt_t h) { return live(h, "decrypt handle is NULL or destroyed"); }

int dec_scale_round_run(ofhe_bfv_decrypt_t h, const u64* x, u64* out, u32 batch, hipStream_t s) {
    const dim3 g(grid_for((u64)batch << h->args.log_n)), t(256);
    const DecArgs& A = h->args;
    if (h->branch == OFHE_BFV_DECRYPT_ONE_TOWER)
        hipLaunchKernelGGL(k_dec_one_tower, g, t, 0, s, A, x, out, (u64)batch << A.log_n);
    else if (h->branch == OFHE_BFV_DECRYPT_BEHZ)
        hipLaunchKernelGGL(k_dec_scale_round_behz, g, t, 0, s, A, x, out, batch);
    else
        with_int<0, 1, 2, 3, 4, 5, 6, 7>(h->branch, [&](auto br) {
            hipLaunchKernelGGL((k_dec_scale_round<decltype(br)::value>), g, t, 0, s, A, x, out, batch);
        });
    return post_launch();
}

}  // namespace

int ofhe_hip_bfv_decrypt_create(ofhe_ctx_t ctx, uint32_t log_n, uint32_t size_q, const uint64_t* q, uint64_t t,
                                int technique, const ofhe_bfv_decrypt_tables* tb, ofhe_bfv_decrypt_t* out) {
    // every argument check comes before the context is looked at, so a bad
    // argument is reported without a device
    if (!q || !tb || !out) return fail(OFHE_ERR_ARG, "NULL argument");
    if (log_n < 1 || log_n > 17) return fail(OFHE_ERR_ARG, "log_n must be in [1, 17]");
    if (size_q < 1 || size_q > 255) return fail(OFHE_ERR_ARG, "size_q must be in [1, 255]");
    if (t < 2) return fail(OFHE_ERR_ARG, "t must be at least 2");
    // F and H add size_q (split: 2 size_q) products reduced mod t in one word
    if ((u128)2 * size_q * t >= ((u128)1 << 64)) return fail(OFHE_ERR_ARG, "2 size_q t must be below 2^64");
    if (technique != OFHE_BFV_HPS && technique != OFHE_BFV_HPSPOVERQ && technique != OFHE_BFV_BEHZ)
        return fail(OFHE_ERR_ARG, "technique must be HPS, HPSPOVERQ or BEHZ");
    RCCHK(check_moduli(q, size_q));
    const bool behz = technique == OFHE_BFV_BEHZ;
    int branch = OFHE_BFV_DECRYPT_ONE_TOWER;
    if (size_q > 1) {
        if (behz) {
            // t gamma < 2^58 (bfvrns-cryptoparameters.cpp:859)
            if (t >= (1ull << 32)) return fail(OFHE_ERR_ARG, "BEHZ needs t 2^26 below 2^58");
            if (!tb->tgammaQHatInvModq || !tb->negInvqModtgamma) return fail(OFHE_ERR_ARG, "NULL BEHZ table");
            branch = OFHE_BFV_DECRYPT_BEHZ;
        } else {
            if (!tb->tQHatInvModqDivqModt || !tb->tQHatInvModqDivqFrac) return fail(OFHE_ERR_ARG, "NULL table");
            branch = dec_branch(size_q, q[0], t);
            if ((branch & 2) && (!tb->tQHatInvModqBDivqModt || !tb->tQHatInvModqBDivqFrac))
                return fail(OFHE_ERR_ARG, "NULL B table: the split loops need tQHatInvModqBDivqModt / Frac");
        }
    }
    if ((tb->tInvModq == nullptr) != (tb->negQModt == nullptr))
        return fail(OFHE_ERR_ARG, "tInvModq and negQModt come together");
    if (!ctx) return fail(OFHE_ERR_ARG, "context is NULL");

    // one device block of 64-bit words (doubles by their bits): q | w | wb | frac | fracb | qmu | tiq
    const size_t Q = size_q;
    std::vector<u64> hm(11 * Q, 0);
    u64 *hq = hm.data(), *hw = hq + Q, *hwb = hw + 2 * Q, *hf = hwb + 2 * Q, *hfb = hf + Q, *hmu = hfb + Q,
        *hti = hmu + 2 * Q;
    const u64 tgamma = t << 26;
    auto pair = [](u64* at, u64 w, u64 m) {
        at[0] = w % m;
        at[1] = shoup_pre(w % m, m);
    };
    for (u32 i = 0; i < size_q; i++) {
        hq[i] = q[i];
        barrett128(q[i], hmu + 2 * i);
        if (branch == OFHE_BFV_DECRYPT_BEHZ) {
            pair(hw + 2 * i, tb->tgammaQHatInvModq[i], q[i]);
            pair(hwb + 2 * i, tb->negInvqModtgamma[i], tgamma);
        } else if (branch != OFHE_BFV_DECRYPT_ONE_TOWER) {
            pair(hw + 2 * i, tb->tQHatInvModqDivqModt[i], t);
            std::memcpy(hf + i, tb->tQHatInvModqDivqFrac + i, 8);
            if (branch & 2) {
                pair(hwb + 2 * i, tb->tQHatInvModqBDivqModt[i], t);
                std::memcpy(hfb + i, tb->tQHatInvModqBDivqFrac + i, 8);
            }
        }
        if (tb->tInvModq) pair(hti + 2 * i, tb->tInvModq[i], q[i]);
    }

    ofhe_bfv_decrypt_s* r = nullptr;
    RCCHK(create_with_table(&r, &ofhe_bfv_decrypt_s::d_mem, hm, ctx->device, "decrypt allocation failed",
                            "decrypt upload"));
    r->ctx = ctx;
    r->branch = branch;
    r->has_tqt = tb->tInvModq != nullptr;
    r->q.assign(q, q + size_q);
    DecArgs& A = r->args;
    const u64* d = r->d_mem;
    A.qv = d;
    A.w = d + Q;
    A.wb = d + 3 * Q;
    A.frac = reinterpret_cast<const double*>(d + 5 * Q);
    A.fracb = reinterpret_cast<const double*>(d + 6 * Q);
    A.qmu = d + 7 * Q;
    A.tiq = d + 9 * Q;
    A.t = t;
    A.tgamma = tgamma;
    if (r->has_tqt) {
        A.nqt = tb->negQModt[0] % t;
        A.nqt_pre = shoup_pre(A.nqt, t);
    }
    A.td = (double)t;   // double td = t.ConvertToInt() (dcrtpoly-impl.h:1674)
    A.tinv = 1. / A.td;  // :1675
    A.log_n = log_n;
    A.size_q = size_q;
    A.half = msb64(q[0]) >> 1;
    {
        // NativeVectorT::SwitchModulus q[0] -> t (mubintvecnat.cpp:111-136), the constants of sw_mod
        const bool down = t <= q[0];
        A.sw_q = q[0];
        A.sw = SwMod{q[0] >> 1, t, down ? t - (q[0] % t) : t - q[0], down, q[0] <= 2 * t};
    }
    *out = r;
    return OFHE_OK;
}

int ofhe_hip_bfv_decrypt_destroy(ofhe_bfv_decrypt_t h) {
    return destroy_with_table(h, &ofhe_bfv_decrypt_s::d_mem, "decrypt handle is NULL");
}

int ofhe_hip_bfv_decrypt_branch(ofhe_bfv_decrypt_t h, int* branch) {
    RCCHK(dec_live(h));
    if (!branch) return fail(OFHE_ERR_ARG, "branch is NULL");
    *branch = h->branch;
    return OFHE_OK;
}

int ofhe_hip_bfv_decrypt_scale_round(ofhe_bfv_decrypt_t h, const uint64_t* x, uint64_t* out, uint32_t batch,
                                     void* stream) {
    RCCHK(dec_live(h));
    if (!x || !out || batch == 0) return fail(OFHE_ERR_ARG, "bad data argument");
    HIPCHK(hipSetDevice(h->ctx->device));
    return dec_scale_round_run(h, x, out, batch, pick(stream));
}

int ofhe_hip_bfv_decrypt(ofhe_bfv_decrypt_t h, ofhe_plan_t plan_q, uint32_t elements, int eval_form,
                         const uint64_t* c0, const uint64_t* c1, const uint64_t* c2, const uint64_t* s, uint64_t* out,
                         uint32_t batch, void* stream) {
    RCCHK(dec_live(h));
    RCCHK(plan_is(plan_q, h->ctx, h->args.log_n, {&h->q}, "plan_q"));
    if (elements != 2 && elements != 3) return fail(OFHE_ERR_ARG, "2 or 3 ciphertext elements");
    if (!c0 || !c1 || (elements == 3 && !c2) || !s || !out || batch == 0) return fail(OFHE_ERR_ARG, "bad data argument");
    HIPCHK(hipSetDevice(h->ctx->device));
    hipStream_t st = pick(stream);
    const u64 N = 1ull << h->args.log_n, Q = h->args.size_q, one = (u64)batch * Q * N;
    const dim3 g(grid_for(one));
    // scratch: b, and the transforms of coefficient-form elements
    Scratch sc;
    RCCHK(sc.alloc((1 + (eval_form ? 0 : elements)) * one * sizeof(u64), st, h->ctx));
    u64* b = sc.w();
    const u64* cv[3] = {c0, c1, elements == 3 ? c2 : nullptr};
    if (!eval_form)
        for (u32 k = 0; k < elements; k++) {
            // b.SetFormat(EVALUATION), ci.SetFormat(EVALUATION) (rns-pke.cpp:213, 218)
            u64* e = b + (k + 1) * one;
            RCCHK(plan_ntt_range(plan_q, false, 0, (u32)Q, cv[k], e, Q * N, Q * N, batch, st));
            cv[k] = e;
        }
    with_bool(elements == 3, [&](auto three) {
        hipLaunchKernelGGL((k_decrypt_core<decltype(three)::value>), g, dim3(256), 0, st,
                           CoreArgs{h->args.qv, h->args.qmu, h->args.log_n, h->args.size_q}, cv[0], cv[1], cv[2], s, b,
                           one);
    });
    RCCHK(post_launch());
    // b.SetFormat(COEFFICIENT) (bfvrns-pke.cpp:211)
    RCCHK(plan_ntt_range(plan_q, true, 0, (u32)Q, b, b, Q * N, Q * N, batch, st));
    return dec_scale_round_run(h, b, out, batch, st);
}

int ofhe_hip_times_q_over_t(ofhe_bfv_decrypt_t h, const uint64_t* x, uint64_t* out, uint32_t batch, void* stream) {
    RCCHK(dec_live(h));
    if (!h->has_tqt) return fail(OFHE_ERR_STATE, "the handle was created without tInvModq / negQModt");
    if (!x || !out || batch == 0) return fail(OFHE_ERR_ARG, "bad data argument");
    HIPCHK(hipSetDevice(h->ctx->device));
    const u64 total = ((u64)batch * h->args.size_q) << h->args.log_n;
    const dim3 g(grid_for(total));
    hipLaunchKernelGGL(k_times_q_over_t, g, dim3(256), 0, pick(stream), h->args, x, out, total);
    return post_launch();
}
