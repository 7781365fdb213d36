// bgv_decrypt.hip -- BGV decryption and the CKKS decryption core on gfx950: the
// kernels of bgv_decrypt_kernels.hpp composed with the transforms.
//
// Reference call stacks restated here (one launch per step covers the batch):
//   PKEBGVRNS::Decrypt                          bgvrns-pke.cpp:44-99
//   PKECKKSRNS::Decrypt / PKERNS::Decrypt       ckksrns-pke.cpp:44-97, rns-pke.cpp:70-109 (up to their last line)
//   PKERNS::DecryptCore                         rns-pke.cpp:199-224
//   DCRTPolyImpl::ModReduce                     dcrtpoly-impl.h:792-812
//   CryptoParametersBGVRNS::PrecomputeCRTTables bgvrns-cryptoparameters.cpp:91-107 (negtInvModq, qlInvModq)
//   PolyImpl::DecryptionCRTInterpolate          poly-impl.h:566-575
#include "bgv_decrypt_kernels.hpp"
#include "compose.hpp"

using namespace ofhe;

struct ofhe_bgv_decrypt_s {
    ofhe_ctx_t ctx = nullptr;
    ChainArgs args{};
    CoreArgs core{};
    u64* d_mem = nullptr;
    std::vector<u64> q;
};

namespace {

// a^-1 mod m for odd m > 1 by the extended Euclidean algorithm; 0 when a is not invertible
u64 inv_or_zero(u64 a, u64 m) {
    __int128 r0 = m, r1 = a % m, t0 = 0, t1 = 1;
    while (r1) {
        const __int128 qt = r0 / r1, r2 = r0 - qt * r1, t2 = t0 - qt * t1;
        r0 = r1, r1 = r2, t0 = t1, t1 = t2;
    }
    if (r0 != 1) return 0;
    return (u64)(t0 < 0 ? t0 + m : t0);
}

int bgv_live(ofhe_bgv_decrypt_t h) { return live(h, "BGV decrypt handle is NULL or destroyed"); }

// x [batch][size_ql][N] -> out [batch][N] through passes of k_bgv_chain, each
// retiring up to BGV_CHAIN_K towers; the passes between the first and the last
// go through two scratch blocks.  plain: NativeVectorT::Mod(t) on the word left.
int chain_run(ofhe_bgv_decrypt_t h, u32 size_ql, bool plain, const u64* x, u64* out, u32 batch, hipStream_t s) {
    const ChainArgs& A = h->args;
    const u64 N = 1ull << A.log_n;
    const dim3 g(grid_for((u64)batch << A.log_n));
    u32 live = size_ql;
    Scratch sc;
    u64* pp[2] = {nullptr, nullptr};
    if (size_ql > BGV_CHAIN_K + 1) {
        // the first pass leaves size_ql - K towers, the second size_ql - 2 K
        const u64 w0 = (u64)batch * (size_ql - BGV_CHAIN_K) * N;
        const u64 w1 = size_ql > 2 * BGV_CHAIN_K + 1 ? (u64)batch * (size_ql - 2 * BGV_CHAIN_K) * N : 0;
        RCCHK(sc.alloc((w0 + w1) * sizeof(u64), s, h->ctx));
        pp[0] = sc.w();
        pp[1] = sc.w() + w0;
    }
    const u64* src = x;
    for (u32 pass = 0;; pass++) {
        const u32 k = std::min<u32>(live - 1, BGV_CHAIN_K), left = live - k;
        const bool last = left == 1;
        u64* dst = last ? out : pp[pass & 1];
        hipLaunchKernelGGL(k_bgv_chain<BGV_CHAIN_K>, g, dim3(256), 0, s, A, src, dst, live, k, (u32)(last && plain),
                           batch);
        RCCHK(post_launch());
        if (last) return OFHE_OK;
        src = dst;
        live = left;
    }
}

int core_launch(const CoreArgs& C, u32 elements, const u64* c0, const u64* c1, const u64* c2, const u64* s, u64* out,
                u64 total, hipStream_t st) {
    const dim3 g(grid_for(total));
    with_bool(elements == 3, [&](auto three) {
        hipLaunchKernelGGL((k_decrypt_core<decltype(three)::value>), g, dim3(256), 0, st, C, c0, c1, c2, s, out, total);
    });
    return post_launch();
}

int elements_ok(u32 elements, const u64* c0, const u64* c1, const u64* c2, const u64* s, const u64* out, u32 batch) {
    if (elements != 2 && elements != 3) return fail(OFHE_ERR_ARG, "2 or 3 ciphertext elements");
    if (!c0 || !c1 || (elements == 3 && !c2) || !s || !out || batch == 0) return fail(OFHE_ERR_ARG, "bad data argument");
    if (((uintptr_t)c0 | (uintptr_t)c1 | (uintptr_t)c2 | (uintptr_t)s | (uintptr_t)out) & 15)
        return fail(OFHE_ERR_ARG, "buffers must be 16-byte aligned");
    return OFHE_OK;
}

}  // namespace

int ofhe_hip_bgv_decrypt_create(ofhe_ctx_t ctx, uint32_t log_n, uint32_t size_q, const uint64_t* q, uint64_t t,
                                ofhe_bgv_decrypt_t* out) {
    // every argument check comes before the context is looked at, so a bad
    // argument is reported without a device
    if (!q || !out) return fail(OFHE_ERR_ARG, "NULL argument");
    if (log_n < 1 || log_n > 17) return fail(OFHE_ERR_ARG, "log_n must be in [1, 17]");
    if (size_q < 1 || size_q > OFHE_BGV_DECRYPT_MAX_TOWERS)
        return fail(OFHE_ERR_ARG, "size_q must be in [1, " + std::to_string(OFHE_BGV_DECRYPT_MAX_TOWERS) + "]");
    if (t < 2) return fail(OFHE_ERR_ARG, "t must be at least 2");
    RCCHK(check_moduli(q, size_q));
    const size_t Q = size_q, pairs = Q * (Q - 1) / 2;
    // one device block: tw | pw | q | qmu
    std::vector<u64> hm(BGV_TW * Q + BGV_PW * pairs + 3 * Q, 0);
    u64 *tw = hm.data(), *pw = tw + BGV_TW * Q, *hq = pw + BGV_PW * pairs, *hmu = hq + Q;
    auto pair = [](u64* at, u64 w, u64 m) {
        at[0] = w;
        at[1] = shoup_pre(w, m);
    };
    for (u32 j = 0; j < size_q; j++) {
        const u64 qj = q[j];
        for (u32 i = 0; i < j; i++)
            if (q[i] == qj) return fail(OFHE_ERR_ARG, "modulus " + std::to_string(j) + " repeats modulus " + std::to_string(i));
        hq[j] = tw[BGV_TW * j] = qj;
        tw[BGV_TW * j + 1] = 0 - qj;
        barrett128(qj, hmu + 2 * j);
        if (j == 0) continue;  // tower 0 is never retired: t need not be invertible there
        // negtInvModq[j] = q_j - t^-1 mod q_j (bgvrns-cryptoparameters.cpp:97)
        const u64 ti = inv_or_zero(t % qj, qj);
        if (!ti) return fail(OFHE_ERR_ARG, "t is not invertible modulo modulus " + std::to_string(j));
        pair(tw + BGV_TW * j + 2, qj - ti, qj);
        for (u32 i = 0; i < j; i++) {
            // qlInvModq[j][i] = q_j^-1 mod q_i (:104); t mod q_i (:99) folded into ta
            const u64 qi = q[i], a = inv_or_zero(qj % qi, qi);
            if (!a)
                return fail(OFHE_ERR_ARG, "modulus " + std::to_string(j) + " is not invertible modulo modulus " + std::to_string(i));
            u64* P = pw + BGV_PW * ((size_t)j * (j - 1) / 2 + i);
            pair(P, a, qi);
            pair(P + 2, mulmod(t % qi, a, qi), qi);
            P[4] = qi > qj ? qi - qj : qi - qj % qi;  // SwitchModulus's diff, mubintvecnat.cpp:119, 127
        }
    }
    if (!ctx) return fail(OFHE_ERR_ARG, "context is NULL");

    ofhe_bgv_decrypt_s* r = nullptr;
    RCCHK(create_with_table(&r, &ofhe_bgv_decrypt_s::d_mem, hm, ctx->device, "BGV decrypt allocation failed",
                            "BGV decrypt upload"));
    r->ctx = ctx;
    r->q.assign(q, q + size_q);
    const u64* d = r->d_mem;
    ChainArgs& A = r->args;
    A.tw = d;
    A.pw = d + BGV_TW * Q;
    A.t = t;
    A.mt_mode = t == 2 ? BGV_MT_TWO : t > q[0] ? BGV_MT_UP : BGV_MT_DOWN;
    A.mt_diff = t > q[0] ? t - q[0] : t - q[0] % t;  // mubintvecnat.cpp:148, 156
    A.log_n = log_n;
    r->core = CoreArgs{d + BGV_TW * Q + BGV_PW * pairs, d + BGV_TW * Q + BGV_PW * pairs + Q, log_n, size_q};
    *out = r;
    return OFHE_OK;
}

int ofhe_hip_bgv_decrypt_destroy(ofhe_bgv_decrypt_t h) {
    return destroy_with_table(h, &ofhe_bgv_decrypt_s::d_mem, "BGV decrypt handle is NULL");
}

int ofhe_hip_bgv_mod_reduce_chain(ofhe_bgv_decrypt_t h, uint32_t size_ql, int to_plaintext, const uint64_t* x,
                                  uint64_t* out, uint32_t batch, void* stream) {
    RCCHK(bgv_live(h));
    if (size_ql < 1 || size_ql > h->q.size()) return fail(OFHE_ERR_ARG, "size_ql must be in [1, size_q]");
    if (!x || !out || batch == 0) return fail(OFHE_ERR_ARG, "bad data argument");
    if (((uintptr_t)x | (uintptr_t)out) & 15) return fail(OFHE_ERR_ARG, "buffers must be 16-byte aligned");
    const u64 n = (u64)batch << h->args.log_n;
    if (words_overlap(x, n * size_ql, out, n)) return fail(OFHE_ERR_ARG, "out overlaps x");
    HIPCHK(hipSetDevice(h->ctx->device));
    return chain_run(h, size_ql, to_plaintext != 0, x, out, batch, pick(stream));
}

int ofhe_hip_bgv_decrypt(ofhe_bgv_decrypt_t h, ofhe_plan_t plan_q, uint32_t size_ql, uint32_t elements, int eval_form,
                         const uint64_t* c0, const uint64_t* c1, const uint64_t* c2, const uint64_t* s, uint64_t* out,
                         uint32_t batch, void* stream) {
    RCCHK(bgv_live(h));
    RCCHK(plan_is(plan_q, h->ctx, h->args.log_n, {&h->q}, "plan_q"));
    if (size_ql < 1 || size_ql > h->q.size()) return fail(OFHE_ERR_ARG, "size_ql must be in [1, size_q]");
    RCCHK(elements_ok(elements, c0, c1, c2, s, out, batch));
    HIPCHK(hipSetDevice(h->ctx->device));
    hipStream_t st = pick(stream);
    const u64 N = 1ull << h->args.log_n, L = size_ql, bn = (u64)batch * N;
    const u64* cv[3] = {c0, c1, c2};
    Scratch sc;
    if (eval_form) {
        // b = DecryptCore(cv), b.SetFormat(COEFFICIENT), the ModReduce chain, DecryptionCRTInterpolate (:53-60, 96)
        RCCHK(sc.alloc(bn * L * sizeof(u64), st, h->ctx));
        u64* b = sc.w();
        CoreArgs C = h->core;
        C.size_q = size_ql;
        RCCHK(core_launch(C, elements, c0, c1, c2, s, b, bn * L, st));
        RCCHK(plan_ntt_range(plan_q, true, 0, size_ql, b, b, L * N, L * N, batch, st));
        return chain_run(h, size_ql, true, b, out, batch, st);
    }
    // every element through the chain first (:73-81), then DecryptCore on the one tower left (:92-93)
    RCCHK(sc.alloc(bn * elements * sizeof(u64), st, h->ctx));
    u64* r = sc.w();
    for (u32 e = 0; e < elements; e++) {
        if (size_ql > 1)
            RCCHK(chain_run(h, size_ql, false, cv[e], r + e * bn, batch, st));
        // ci.SetFormat(EVALUATION) (rns-pke.cpp:213, 218)
        RCCHK(plan_ntt_range(plan_q, false, 0, 1, size_ql > 1 ? r + e * bn : cv[e], r + e * bn, N, N, batch, st));
    }
    CoreArgs C = h->core;
    C.size_q = 1;
    RCCHK(core_launch(C, elements, r, r + bn, r + 2 * bn, s, r, bn, st));
    RCCHK(plan_ntt_range(plan_q, true, 0, 1, r, r, N, N, batch, st));
    // Mod t alone: the chain kernel on one tower
    return chain_run(h, 1, true, r, out, batch, st);
}

int ofhe_hip_decrypt_core(ofhe_plan_t p, uint32_t size_ql, uint32_t elements, int eval_form, int coeff_out,
                          const uint64_t* c0, const uint64_t* c1, const uint64_t* c2, const uint64_t* s, uint64_t* out,
                          uint32_t batch, void* stream) {
    if (!p || !p->ctx) return fail(OFHE_ERR_STATE, "plan is NULL or destroyed");
    if (size_ql < 1 || size_ql > p->towers) return fail(OFHE_ERR_ARG, "size_ql must be in [1, plan towers]");
    RCCHK(elements_ok(elements, c0, c1, c2, s, out, batch));
    HIPCHK(hipSetDevice(p->ctx->device));
    hipStream_t st = pick(stream);
    const u64 N = 1ull << p->log_n, L = size_ql, one = (u64)batch * L * N;
    const u64* cv[3] = {c0, c1, elements == 3 ? c2 : nullptr};
    for (u32 k = 0; k < elements; k++)
        if (cv[k] != out ? words_overlap(cv[k], one, out, one) : k != 0)
            return fail(OFHE_ERR_ARG, "out may be c0 itself; any other overlap with an element is refused");
    // q | floor(2^128 / q) of the plan's towers, uploaded on the first call
    std::vector<u64> key(3 * (size_t)p->towers + 1);
    for (u32 i = 0; i < p->towers; i++) {
        key[i] = p->q[i];
        barrett128(p->q[i], &key[p->towers + 2 * (size_t)i]);
    }
    key.back() = 0x636f7265;  // the tag of this layout among the plan's tables
    const u64* d = nullptr;
    RCCHK(cached_table(p->tab_mu, p->tabs, key, "decrypt-core tables", &d,
                       [&]() -> const std::vector<u64>& { return key; }));
    const CoreArgs C{d, d + p->towers, p->log_n, size_ql};
    Scratch sc;
    if (!eval_form) {
        // b.SetFormat(EVALUATION), ci.SetFormat(EVALUATION) (rns-pke.cpp:213, 218)
        RCCHK(sc.alloc(elements * one * sizeof(u64), st, p->ctx));
        for (u32 k = 0; k < elements; k++) {
            u64* e = sc.w() + k * one;
            RCCHK(plan_ntt_range(p, false, 0, size_ql, cv[k], e, L * N, L * N, batch, st));
            cv[k] = e;
        }
    }
    RCCHK(core_launch(C, elements, cv[0], cv[1], cv[2], s, out, one, st));
    if (coeff_out) return plan_ntt_range(p, true, 0, size_ql, out, out, L * N, L * N, batch, st);
    return OFHE_OK;
}
