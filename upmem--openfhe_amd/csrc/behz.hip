// behz.hip -- BFV (BEHZ) multiplication on gfx950: the Montgomery base
// extension, the RNS floor and the Shenoy-Kumaresan conversion of
// behz_kernels.hpp, composed with the transforms and the tensor product.
//
// Reference call stacks restated here (one launch per step covers the batch):
//   DCRTPolyImpl::FastBaseConvqToBskMontgomery  dcrtpoly-impl.h:2050-2208
//   DCRTPolyImpl::FastRNSFloorq                 dcrtpoly-impl.h:2212-2271
//   DCRTPolyImpl::FastBaseConvSK                dcrtpoly-impl.h:2309-2411
//   LeveledSHEBFVRNS::EvalMult                  bfvrns-leveledshe.cpp:275-297, 326-337, 383-403 (BEHZ)
#include <algorithm>

#include "behz_kernels.hpp"
#include "compose.hpp"

using namespace ofhe;

struct ofhe_behz_s {
    ofhe_ctx_t ctx = nullptr;
    BehzArgs args{};
    u64* d_mem = nullptr;
    u32 log_n = 0, size_q = 0, size_b = 0;
    std::vector<u64> q, bsk;
};

namespace {

enum { BEHZ_Q_TO_BSK, BEHZ_FLOOR, BEHZ_SK, BEHZ_FLOOR_SK };

static_assert(BEHZ_FUSED_BMAX == OFHE_BEHZ_FUSED_MAX_B, "the header documents the fused kernel's cap");
bool behz_fused_ok(ofhe_behz_t h) { return h->size_b <= BEHZ_FUSED_BMAX; }

int behz_launch(ofhe_behz_t h, int which, const u64* x, u64 in_stride, u64* out, u64 out_stride, u32 batch,
                hipStream_t s) {
    dim3 g;
    RCCHK(coeff_grid((u64)batch << h->log_n, &g));
    const dim3 t(256);
    const BehzArgs& A = h->args;
    switch (which) {
        case BEHZ_Q_TO_BSK:
            // the limb sums hold at most BCONV_LIMB_QMAX products below 2^60 in a word
            if (h->size_q <= BCONV_LIMB_QMAX)
                hipLaunchKernelGGL((k_behz_q_to_bsk_limb<BCONV_PT>), g, t, 0, s, A, x, in_stride, out, out_stride, batch);
            else
                hipLaunchKernelGGL((k_behz_q_to_bsk<BEHZ_PT>), g, t, 0, s, A, x, in_stride, out, out_stride, batch);
            break;
        case BEHZ_FLOOR:
            hipLaunchKernelGGL((k_behz_floor<BEHZ_PT>), g, t, 0, s, A, x, in_stride, out, out_stride, batch);
            break;
        case BEHZ_SK:
            hipLaunchKernelGGL((k_behz_sk<BEHZ_PT>), g, t, 0, s, A, x, in_stride, out, out_stride, batch);
            break;
        default:
            if (!behz_fused_ok(h)) return fail(OFHE_ERR_ARG, "too many B towers for the fused floor and conversion");
            hipLaunchKernelGGL((k_behz_floor_sk<BEHZ_PT>), g, t, (size_t)(h->size_b + 1) * 256 * sizeof(u64), s, A, x,
                               in_stride, out, out_stride, batch);
    }
    return post_launch();
}

int behz_live(ofhe_behz_t h) { return live(h, "behz handle is NULL or destroyed"); }

int plans_match(ofhe_behz_t h, ofhe_plan_t pq, ofhe_plan_t pb) {
    RCCHK(plan_is(pq, h->ctx, h->log_n, {&h->q}, "plan_q"));
    return plan_is(pb, h->ctx, h->log_n, {&h->bsk}, "plan_bsk");
}

// FastBaseConvqToBskMontgomery with its format handling, result in evaluation
// form: an evaluation-form input is kept for the Q towers (polyInNTT,
// 2077-2080, 2189-2192) and its INTT goes through out's Q slots; a
// coefficient-form input has its Q towers transformed (2194-2197); the Bsk
// towers are always transformed (2200-2201).
int behz_expand_run(ofhe_behz_t h, ofhe_plan_t pq, ofhe_plan_t pb, int eval_form, const u64* x, u64* out, u32 batch,
                    hipStream_t s) {
    const u32 K = h->size_b + 1;
    auto convert = [&](const u64* src, u64 sstride, u64* dst, u64 dstride) {
        RCCHK(behz_launch(h, BEHZ_Q_TO_BSK, src, sstride, dst, dstride, batch, s));
        return plan_ntt_range(pb, false, 0, K, dst, dst, dstride, dstride, batch, s);
    };
    return expand_skeleton(pq, h->size_q, K, eval_form, x, out, batch, s, convert);
}

}  // namespace

int ofhe_hip_behz_create(ofhe_ctx_t ctx, uint32_t log_n, uint32_t size_q, const uint64_t* q, uint32_t size_b,
                         const uint64_t* bsk, uint64_t t, const ofhe_behz_tables* tb, ofhe_behz_t* out) {
    // every argument check comes before the context is looked at, so a bad
    // argument is reported without a device
    if (!q || !bsk || !tb || !out) return fail(OFHE_ERR_ARG, "NULL argument");
    if (log_n < 1 || log_n > 17) return fail(OFHE_ERR_ARG, "log_n must be in [1, 17]");
    // size + 1 products below 2^120 must fit the 128-bit sums (the reference's DoubleNativeInt has the same limit)
    if (size_q < 1 || size_q > 255) return fail(OFHE_ERR_ARG, "size_q must be in [1, 255]");
    if (size_b < 1 || size_b > 255) return fail(OFHE_ERR_ARG, "size_b must be in [1, 255]");
    if (t < 2) return fail(OFHE_ERR_ARG, "t must be at least 2");
    const u32 K = size_b + 1;
    std::vector<u64> all(q, q + size_q);
    all.insert(all.end(), bsk, bsk + K);
    RCCHK(check_moduli(all.data(), all.size()));
    // the centred remainder mod mtilde = 2^16 is lifted as r + b_j - 2^16 (dcrtpoly-impl.h:2172-2174)
    for (u32 j = 0; j < K; j++)
        if (bsk[j] <= (1ull << 16)) return fail(OFHE_ERR_ARG, "every Bsk modulus must exceed 2^16");
    {
        std::vector<u64> sorted(all);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
            return fail(OFHE_ERR_ARG, "repeated modulus in q and Bsk");
    }
    const uint64_t* const ptrs[] = {tb->tQHatInvModq, tb->QHatModbsk, tb->QHatModmtilde, tb->qInvModbsk,
                                    tb->mtildeQHatInvModq, tb->negQInvModmtilde, tb->QModbsk, tb->mtildeInvModbsk,
                                    tb->tQInvModbsk, tb->BHatInvModb, tb->BHatModq, tb->BHatModmsk, tb->BInvModmsk,
                                    tb->BModq};
    for (const uint64_t* p : ptrs)
        if (!p) return fail(OFHE_ERR_ARG, "NULL table");
    if (!ctx) return fail(OFHE_ERR_ARG, "context is NULL");

    // one device block: every table reduced to its modulus, Shoup precons and
    // 128-bit Barrett constants derived here
    std::vector<u64> hm;
    auto put = [&](size_t words) {
        const size_t at = hm.size();
        hm.resize(at + words);
        return at;
    };
    auto mods = [&](const u64* m, u32 n) {  // moduli, then (mu_lo, mu_hi) each
        const size_t at = put(3 * (size_t)n);
        for (u32 i = 0; i < n; i++) {
            hm[at + i] = m[i];
            barrett128(m[i], &hm[at + n + 2 * i]);
        }
        return at;
    };
    auto shoup = [&](const u64* w, const u64* m, u32 n) {  // (w mod m, precon) pairs
        const size_t at = put(2 * (size_t)n);
        for (u32 i = 0; i < n; i++) {
            hm[at + 2 * i] = w[i] % m[i];
            hm[at + 2 * i + 1] = shoup_pre(w[i] % m[i], m[i]);
        }
        return at;
    };
    auto matrix = [&](const u64* w, u32 rows, u32 cols, const u64* colmod) {  // [rows][cols], column j mod colmod[j]
        const size_t at = put((size_t)rows * cols);
        for (u32 i = 0; i < rows; i++)
            for (u32 j = 0; j < cols; j++) hm[at + (size_t)i * cols + j] = w[(size_t)i * cols + j] % colmod[j];
        return at;
    };
    const u64 msk = bsk[size_b];
    const size_t o_q = mods(q, size_q), o_b = mods(bsk, K);
    const size_t o_mtq = shoup(tb->mtildeQHatInvModq, q, size_q), o_qhb = matrix(tb->QHatModbsk, size_q, K, bsk);
    // QHatModbsk once more as 30-bit limbs, [size_q][K rounded up to BCONV_PT] zero padded (k_bconv_limb's table)
    const u32 kpad = (K + BCONV_PT - 1) / BCONV_PT * BCONV_PT;
    const size_t o_qhl = put((size_t)size_q * kpad);
    for (u32 i = 0; i < size_q; i++)
        for (u32 j = 0; j < K; j++) {
            const u64 c = hm[o_qhb + (size_t)i * K + j];
            hm[o_qhl + (size_t)i * kpad + j] = (c & LIMB_MASK) | ((c >> LIMB) << 32);
        }
    const size_t o_bred = put(3 * (size_t)K);
    for (u32 j = 0; j < K; j++) limb_red_consts(bsk[j], &hm[o_bred + 3 * (size_t)j]);
    const size_t o_qhm = put(size_q);
    for (u32 i = 0; i < size_q; i++) hm[o_qhm + i] = tb->QHatModmtilde[i] & 0xffff;
    const size_t o_qmb = shoup(tb->QModbsk, bsk, K), o_mib = shoup(tb->mtildeInvModbsk, bsk, K);
    const size_t o_tqh = shoup(tb->tQHatInvModq, q, size_q), o_qib = matrix(tb->qInvModbsk, size_q, K, bsk);
    const size_t o_tqb = shoup(tb->tQInvModbsk, bsk, K), o_bhi = shoup(tb->BHatInvModb, bsk, size_b);
    const size_t o_bhq = matrix(tb->BHatModq, size_b, size_q, q);
    const size_t o_bhm = put(size_b);
    for (u32 i = 0; i < size_b; i++) hm[o_bhm + i] = tb->BHatModmsk[i] % msk;
    const size_t o_bmq = shoup(tb->BModq, q, size_q);

    ofhe_behz_s* r = nullptr;
    RCCHK(create_with_table(&r, &ofhe_behz_s::d_mem, hm, ctx->device, "behz allocation failed", "behz upload"));
    r->ctx = ctx;
    r->log_n = log_n;
    r->size_q = size_q;
    r->size_b = size_b;
    r->q.assign(q, q + size_q);
    r->bsk.assign(bsk, bsk + K);
    BehzArgs& A = r->args;
    const u64* d = r->d_mem;
    A.qv = d + o_q;
    A.qmu = d + o_q + size_q;
    A.bv = d + o_b;
    A.bmu = d + o_b + K;
    A.mtq = d + o_mtq;
    A.qhb = d + o_qhb;
    A.qhm = d + o_qhm;
    A.qhl = d + o_qhl;
    A.bred = d + o_bred;
    A.qmb = d + o_qmb;
    A.mib = d + o_mib;
    A.tqh = d + o_tqh;
    A.qib = d + o_qib;
    A.tqb = d + o_tqb;
    A.bhi = d + o_bhi;
    A.bhq = d + o_bhq;
    A.bhm = d + o_bhm;
    A.bmq = d + o_bmq;
    A.binv = tb->BInvModmsk[0] % msk;
    A.binv_pre = shoup_pre(A.binv, msk);
    A.neg_qinv_mt = (u32)(tb->negQInvModmtilde[0] & 0xffff);
    A.log_n = log_n;
    A.size_q = size_q;
    A.size_b = size_b;
    *out = r;
    return OFHE_OK;
}

int ofhe_hip_behz_destroy(ofhe_behz_t h) {
    return destroy_with_table(h, &ofhe_behz_s::d_mem, "behz handle is NULL");
}

int ofhe_hip_behz_q_to_bsk(ofhe_behz_t h, const uint64_t* x, uint64_t* out, uint32_t batch, void* stream) {
    RCCHK(behz_live(h));
    if (!x || !out || batch == 0) return fail(OFHE_ERR_ARG, "bad data argument");
    HIPCHK(hipSetDevice(h->ctx->device));
    const u64 N = 1ull << h->log_n;
    return behz_launch(h, BEHZ_Q_TO_BSK, x, h->size_q * N, out, (h->size_b + 1) * N, batch, pick(stream));
}

int ofhe_hip_behz_expand(ofhe_behz_t h, ofhe_plan_t plan_q, ofhe_plan_t plan_bsk, int eval_form, const uint64_t* x,
                         uint64_t* out, uint32_t batch, void* stream) {
    RCCHK(behz_live(h));
    RCCHK(plans_match(h, plan_q, plan_bsk));
    if (!x || !out || batch == 0) return fail(OFHE_ERR_ARG, "bad data argument");
    // the INTT of an evaluation-form input goes through out's Q slots and x is read again at the end
    const u64 bn = (u64)batch << h->log_n;
    if (words_overlap(x, bn * h->size_q, out, bn * (h->size_q + h->size_b + 1)))
        return fail(OFHE_ERR_ARG, "out overlaps x");
    HIPCHK(hipSetDevice(h->ctx->device));
    return behz_expand_run(h, plan_q, plan_bsk, eval_form, x, out, batch, pick(stream));
}

int ofhe_hip_behz_floor(ofhe_behz_t h, const uint64_t* x, uint64_t* out, uint32_t batch, void* stream) {
    RCCHK(behz_live(h));
    if (!x || !out || batch == 0) return fail(OFHE_ERR_ARG, "bad data argument");
    HIPCHK(hipSetDevice(h->ctx->device));
    const u64 N = 1ull << h->log_n, K = h->size_b + 1;
    return behz_launch(h, BEHZ_FLOOR, x, (h->size_q + K) * N, out, K * N, batch, pick(stream));
}

int ofhe_hip_behz_conv_sk(ofhe_behz_t h, const uint64_t* x, uint64_t* out, uint32_t batch, void* stream) {
    RCCHK(behz_live(h));
    if (!x || !out || batch == 0) return fail(OFHE_ERR_ARG, "bad data argument");
    HIPCHK(hipSetDevice(h->ctx->device));
    const u64 N = 1ull << h->log_n;
    return behz_launch(h, BEHZ_SK, x, (h->size_b + 1) * N, out, h->size_q * N, batch, pick(stream));
}

int ofhe_hip_behz_floor_sk(ofhe_behz_t h, int fused, const uint64_t* x, uint64_t* out, uint32_t batch, void* stream) {
    RCCHK(behz_live(h));
    if (!x || !out || batch == 0) return fail(OFHE_ERR_ARG, "bad data argument");
    if (fused < 0 || fused > 2) return fail(OFHE_ERR_ARG, "fused must be 0, 1 or 2");
    if (fused == 1 && !behz_fused_ok(h)) return fail(OFHE_ERR_ARG, "too many B towers for the fused floor and conversion");
    HIPCHK(hipSetDevice(h->ctx->device));
    hipStream_t s = pick(stream);
    const u64 N = 1ull << h->log_n, K = h->size_b + 1, Q = h->size_q;
    if (fused == 1 || (fused == 2 && behz_fused_ok(h)))
        return behz_launch(h, BEHZ_FLOOR_SK, x, (Q + K) * N, out, Q * N, batch, s);
    Scratch sc;
    RCCHK(sc.alloc((u64)batch * K * N * sizeof(u64), s, h->ctx));
    RCCHK(behz_launch(h, BEHZ_FLOOR, x, (Q + K) * N, sc.w(), K * N, batch, s));
    return behz_launch(h, BEHZ_SK, sc.w(), K * N, out, Q * N, batch, s);
}

int ofhe_hip_bfv_eval_mult_behz(ofhe_behz_t h, ofhe_plan_t plan_q, ofhe_plan_t plan_bsk, ofhe_plan_t plan_qbsk,
                                const uint64_t* c0, const uint64_t* c1, const uint64_t* d0, const uint64_t* d1,
                                uint64_t* out0, uint64_t* out1, uint64_t* out2, uint32_t batch, void* stream) {
    RCCHK(behz_live(h));
    RCCHK(plans_match(h, plan_q, plan_bsk));
    RCCHK(plan_is(plan_qbsk, h->ctx, h->log_n, {&h->q, &h->bsk}, "plan_qbsk"));
    if (!c0 || !c1 || !d0 || !d1 || !out0 || !out1 || !out2 || batch == 0)
        return fail(OFHE_ERR_ARG, "bad data argument");
    if ((u64)batch * 4 >= (1ull << 32)) return fail(OFHE_ERR_ARG, "batch too large");
    HIPCHK(hipSetDevice(h->ctx->device));
    hipStream_t s = pick(stream);
    const u64 N = 1ull << h->log_n, Q = h->size_q, K = h->size_b + 1, qk = (Q + K) * N;
    const u64 one = (u64)batch * qk;  // words of one expanded polynomial over the batch
    const bool fused = behz_fused_ok(h);
    // scratch: E | T (compose.hpp), (two launches) the products' floors
    Scratch sc;
    RCCHK(sc.alloc((7 * one + (fused ? 0 : 3 * (u64)batch * K * N)) * sizeof(u64), s, h->ctx));
    u64* E = sc.w();
    u64* T = E + 4 * one;
    u64* F = T + 3 * one;
    // FastBaseConvqToBskMontgomery, SetFormat(EVALUATION) of cv1, cv2 (bfvrns-leveledshe.cpp:276-296)
    const u64* in[4] = {c0, c1, d0, d1};
    for (int k = 0; k < 4; k++) RCCHK(behz_expand_run(h, plan_q, plan_bsk, 1, in[k], E + k * one, batch, s));
    // the tensor product over Q|Bsk (326-337), cvMult[i].SetFormat(COEFFICIENT) (387)
    RCCHK(tensor_and_intt(plan_qbsk, E, T, one, batch, stream));
    // FastRNSFloorq (390-393), FastBaseConvSK (396-401)
    u64* outs[3] = {out0, out1, out2};
    if (!fused) RCCHK(behz_launch(h, BEHZ_FLOOR, T, qk, F, K * N, 3 * batch, s));
    for (int k = 0; k < 3; k++) {
        if (fused)
            RCCHK(behz_launch(h, BEHZ_FLOOR_SK, T + k * one, qk, outs[k], Q * N, batch, s));
        else
            RCCHK(behz_launch(h, BEHZ_SK, F + (u64)k * batch * K * N, K * N, outs[k], Q * N, batch, s));
    }
    return OFHE_OK;
}
