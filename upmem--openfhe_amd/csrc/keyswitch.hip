// keyswitch.hip -- ApproxModUp / ApproxModDown and HYBRID key switching on
// gfx950, composed from the NTT, base-conversion and element kernels.
//
// Reference call stacks restated here (one launch per step covers the whole
// batch; the reference loops over towers with OpenMP):
//   DCRTPolyImpl::ApproxModUp    dcrtpoly-impl.h:1085-1131
//   DCRTPolyImpl::ApproxModDown  dcrtpoly-impl.h:1134-1175
//   KeySwitchHYBRID::EvalKeySwitchPrecomputeCore  keyswitch-hybrid.cpp:330-412
//   KeySwitchHYBRID::EvalFastKeySwitchCoreExt     keyswitch-hybrid.cpp:438-482
//   KeySwitchHYBRID::EvalFastKeySwitchCore        keyswitch-hybrid.cpp:414-436
//   LeveledSHEBase::EvalMult / EvalSquare / Relinearize (with evaluation keys)
//                                                 base-leveledshe.cpp:199-372
//   ModReduceInternalInPlace   ckksrns-leveledshe.cpp:107-132, bgvrns-leveledshe.cpp:45-77
//   KeySwitchBV (digitSize 0 .. 30)  keyswitch-bv.cpp:283-338, DCRTPolyImpl::CRTDecompose dcrtpoly-impl.h:266-320
// CRT tables follow CryptoParametersRNS::PrecomputeCRTTables
// (rns-cryptoparameters.cpp:72-345).  The reference builds them with
// BigInteger quotients (Q/q_i) and reductions; every table entry is a residue
// of a product of the moduli, so it is computed here as that product reduced
// modulo the target prime -- the same integer.
#include <algorithm>
#include <initializer_list>
#include <map>
#include <new>

#include "compose.hpp"
#include "ks_kernels.hpp"
#include "lt_kernels.hpp"

using namespace ofhe;

// Tuning knob (tools/exp_ks.py):
// side streams the ModUp digits are spread over (digit j on stream j mod n)
#ifndef OFHE_KS_NSIDE
#define OFHE_KS_NSIDE 2
#endif
constexpr int KS_NSIDE = OFHE_KS_NSIDE;
static_assert(KS_NSIDE >= 1, "ModUp spreads its digits over the side streams");

namespace {

// prod_{k != skip} ms[k] mod m
u64 prod_mod(const u64* ms, u32 n, u32 skip, u64 m) {
    u64 r = 1 % m;
    for (u32 k = 0; k < n; k++)
        if (k != skip) r = mulmod(r, ms[k] % m, m);
    return r;
}

TowerScalar scalar_of(u64 q, u64 s) {
    s %= q;
    return TowerScalar{q, s, shoup_pre(s, q)};
}

// ApproxModDown's plaintext-modulus tables: [P] t^-1 mod p_j (tInvModp), then [Q] t mod q_i
std::vector<TowerScalar> t_tables(const u64* p, u32 P, const u64* q, u32 Q, u64 t) {
    std::vector<TowerScalar> tab(P + Q);
    for (u32 j = 0; j < P; j++) tab[j] = scalar_of(p[j], invmod(t % p[j], p[j]));
    for (u32 i = 0; i < Q; i++) tab[P + i] = scalar_of(q[i], t);
    return tab;
}

int scale_towers(const TowerScalar* d, const u64* x, u64* out, u64 xs, u64 os, u32 batch, u32 towers, u32 log_n,
                 hipStream_t s) {
    const u64 npairs = ((u64)batch * towers << log_n) / 2;
    hipLaunchKernelGGL(k_scale_towers, dim3(grid_for(npairs)), dim3(256), 0, s, d, x, out, xs, os, npairs, log_n,
                       towers);
    return post_launch();
}

int sub_scale(const TowerScalar* d, const u64* x, const u64* y, u64* out, u64 xs, u64 ys, u64 os, u32 batch,
              u32 towers, u32 log_n, hipStream_t s, const u64* add = nullptr) {
    const u64 npairs = ((u64)batch * towers << log_n) / 2;
    if (add)
        hipLaunchKernelGGL(k_sub_scale_add, dim3(grid_for(npairs)), dim3(256), 0, s, d, x, y, add, out, xs, ys, os,
                           npairs, log_n, towers);
    else
        hipLaunchKernelGGL(k_sub_scale, dim3(grid_for(npairs)), dim3(256), 0, s, d, x, y, out, xs, ys, os, npairs,
                           log_n, towers);
    return post_launch();
}

// ApproxModDown core shared by the generic entry point and the key-switch
// engine.  x: [batch][Q+P] (xstride), the P part at x + Q*N; plan towers
// pq0.. for Q and pp0.. for P (both in `plan_q` / `plan_p`).
struct ModDownArgs {
    ofhe_plan_t plan_q, plan_p;
    u32 q0, p0, size_q, size_p;
    BconvArgs bconv;               // P -> Q
    const TowerScalar* pinv;       // [size_q]
    const TowerScalar* tinv_p;     // [size_p] or NULL (t = 0)
    const TowerScalar* t_q;        // [size_q] or NULL
    bool bcols = false;            // k_bconv_cols for the conversion + column pass when it applies
    bool icol = false;             // ... also fed by the P part's inverse block pass (plan_p == plan_q)
};
// k_bconv_cols also runs the sources' inverse column pass (the INTT's second
// pass) when they come from the same plan and nothing scales them in between
static bool md_icol(const ModDownArgs& A) {
    return A.bcols && A.icol && !A.t_q && !A.tinv_p && A.plan_p == A.plan_q && A.plan_q->log_n == 17;
}

// ApproxModDown of nout >= 1 inputs of `batch` entries each into out[k];
// input k starts at x + k * batch * xstride (KeySwitchCore's ct1 follows its
// ct0), so the P-part INTT, the base conversion and the column pass run once
// over nout * batch polynomials; only the last pass, which writes the caller's
// out[k], runs per output.  add != NULL: out[k] = add[k] + that (add[k] laid
// out as out[k], and possibly out[k] itself): the sums of a relinearisation
// (base-leveledshe.cpp:212-213, 368-369) taken in the last pass.
int mod_down_run(const ModDownArgs& A, const u64* x, u64 xstride, u64* const* out, u32 nout, u64 ostride, u32 batch,
                 hipStream_t s, const u64* const* add = nullptr) {
    const u32 log_n = A.plan_q->log_n;
    const u64 N = 1ull << log_n;
    const u32 bn = nout * batch;
    Scratch sp, sq;
    RCCHK(sp.alloc((size_t)bn * A.size_p * N * 8, s, A.plan_q->ctx));
    RCCHK(sq.alloc((size_t)bn * A.size_q * N * 8, s, A.plan_q->ctx));
    const u64 ps = A.size_p * N, qs = A.size_q * N;
    BconvArgs B = A.bconv;
    B.in_stride = ps;
    B.out_stride = qs;
    B.gap_at = A.size_q;
    B.gap = 0;
    B.lazy_out = 1;  // a forward NTT (after an optional tower scale) follows
    // partP: P towers to coefficient form (dcrtpoly-impl.h:1147-1153)
    const bool icol = md_icol(A) && bconv_cols_ok(A.plan_q, B);
    if (icol)  // only the INTT's block pass here, its column pass inside the conversion
        RCCHK(plan_ntt_inv_block(A.plan_p, A.p0, A.size_p, x + qs, xstride, sp.w(), ps, bn, s));
    else
        RCCHK(plan_ntt_range(A.plan_p, true, A.p0, A.size_p, x + qs, sp.w(), xstride, ps, bn, s));
    if (A.tinv_p) RCCHK(scale_towers(A.tinv_p, sp.w(), sp.w(), ps, ps, bn, A.size_p, log_n, s));
    // partPSwitchedToQ (1156-1157), then SetFormat(EVALUATION) and
    // ans_i = (x_i - switched_i) * PInvModq_i (1165-1173): for log_n >= 12 one
    // transform whose block pass applies the subtraction and the scalar while
    // the values are in registers
    const u64* pinv = reinterpret_cast<const u64*>(A.pinv);
    const bool block_tail = log_n >= 12;
    if (A.bcols && !A.t_q && bconv_cols_ok(A.plan_q, B)) {
        // the conversion writes the Q towers' column-pass output (k_bconv_cols)
        RCCHK(bconv_cols_run(A.plan_q, A.q0, B, sp.w(), sq.w(), bn, s, icol ? (int)A.p0 : -1));
    } else {
        RCCHK(bconv_run(B, sp.w(), sq.w(), bn, s));
        if (A.t_q) RCCHK(scale_towers(A.t_q, sq.w(), sq.w(), qs, qs, bn, A.size_q, log_n, s));
        if (block_tail)
            RCCHK(plan_ntt_fwd_sub(A.plan_q, A.q0, A.size_q, sq.w(), qs, x, xstride, out[0], ostride, pinv, bn, s, 1));
        else
            RCCHK(plan_ntt_range(A.plan_q, false, A.q0, A.size_q, sq.w(), sq.w(), qs, qs, bn, s));
    }
    for (u32 k = 0; k < nout; k++) {
        const u64* xk = x + (u64)k * batch * xstride;
        u64* sqk = sq.w() + (u64)k * batch * qs;
        if (block_tail)
            RCCHK(plan_ntt_fwd_sub(A.plan_q, A.q0, A.size_q, sqk, qs, xk, xstride, out[k], ostride, pinv, batch, s, 2,
                                   add ? add[k] : nullptr));
        else
            RCCHK(sub_scale(A.pinv, xk, sqk, out[k], xstride, qs, ostride, batch, A.size_q, log_n, s,
                            add ? add[k] : nullptr));
    }
    return OFHE_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// Generic ApproxModUp / ApproxModDown
// ---------------------------------------------------------------------------
int ofhe_hip_approx_mod_up(ofhe_plan_t pq, ofhe_plan_t pp, ofhe_bconv_t bc, int eval_form, const uint64_t* x,
                           uint64_t* out, uint32_t batch, void* stream) {
    if (!pq || !pp || !bc || !pq->ctx || !pp->ctx || !bc->ctx) return fail(OFHE_ERR_STATE, "NULL or destroyed object");
    if (!x || !out || batch == 0) return fail(OFHE_ERR_ARG, "bad data argument");
    if (pq->log_n != pp->log_n || bc->args.log_n != pq->log_n) return fail(OFHE_ERR_ARG, "ring dimensions differ");
    if (bc->args.size_q != pq->towers || bc->args.size_p != pp->towers)
        return fail(OFHE_ERR_ARG, "base converter does not map plan_q's towers to plan_p's");
    HIPCHK(hipSetDevice(pq->ctx->device));
    hipStream_t s = pick(stream);
    const u32 P = pp->towers;
    auto convert = [&](const u64* src, u64 sstride, u64* dst, u64 dstride) {
        BconvArgs B = bc->args;
        B.in_stride = sstride;
        B.out_stride = dstride;
        B.lazy_out = 1;  // the P towers go through a forward NTT below
        if (bc->bcols && bconv_cols_ok(pp, B)) {
            // the conversion writes the P towers' column-pass output (k_bconv_cols),
            // the block pass finishes their forward transform (1112-1116)
            RCCHK(bconv_cols_run(pp, 0, B, src, dst, batch, s));
            return plan_ntt_fwd_block(pp, 0, P, dst, dstride, batch, s);
        }
        RCCHK(bconv_run(B, src, dst, batch, s));
        return plan_ntt_range(pp, false, 0, P, dst, dst, dstride, dstride, batch, s);  // (1112-1116)
    };
    // the coefficient copy of an evaluation-form x (SetFormat(COEFFICIENT), 1097-1100) goes into the Q
    // slots; the Q towers are the stored evaluation input, or its NTT (1119-1127)
    return expand_skeleton(pq, pq->towers, P, eval_form, x, out, batch, s, convert);
}

int ofhe_hip_approx_mod_down(ofhe_plan_t pq, ofhe_plan_t pp, ofhe_bconv_t bc, const uint64_t* p_inv_modq,
                             uint64_t t, const uint64_t* x, uint64_t* out, uint32_t batch, void* stream) {
    if (!pq || !pp || !bc || !pq->ctx || !pp->ctx || !bc->ctx) return fail(OFHE_ERR_STATE, "NULL or destroyed object");
    if (!x || !out || !p_inv_modq || batch == 0) return fail(OFHE_ERR_ARG, "bad data argument");
    if (pq->log_n != pp->log_n || bc->args.log_n != pq->log_n) return fail(OFHE_ERR_ARG, "ring dimensions differ");
    if (bc->args.size_q != pp->towers || bc->args.size_p != pq->towers)
        return fail(OFHE_ERR_ARG, "base converter does not map plan_p's towers to plan_q's");
    HIPCHK(hipSetDevice(pq->ctx->device));
    hipStream_t s = pick(stream);
    const u32 Q = pq->towers, P = pp->towers;
    // tables cached per (P^-1 mod q, t) in the converter
    std::vector<u64> key(p_inv_modq, p_inv_modq + Q);
    key.push_back(t);
    const u64* dtab = nullptr;
    RCCHK(cached_table(bc->tab_mu, bc->tabs, key, "mod-down tables", &dtab, [&] {
        std::vector<TowerScalar> tab(Q);
        for (u32 i = 0; i < Q; i++) tab[i] = scalar_of(pq->q[i], p_inv_modq[i]);
        if (t) {
            const auto tt = t_tables(pp->q.data(), P, pq->q.data(), Q, t);
            tab.insert(tab.end(), tt.begin(), tt.end());
        }
        return tab;
    }));
    const TowerScalar* d = (const TowerScalar*)dtab;
    ModDownArgs A{pq, pp, 0, 0, Q, P, bc->args, d, t ? d + Q : nullptr, t ? d + Q + P : nullptr, bc->bcols};
    const u64 N = 1ull << pq->log_n;
    return mod_down_run(A, x, (u64)(Q + P) * N, &out, 1, (u64)Q * N, batch, s);
}

// ---------------------------------------------------------------------------
// HYBRID key switching
// ---------------------------------------------------------------------------
struct KsLevel {
    u32 size_ql = 0, beta = 0;
    std::vector<u32> start, cnt;        // digit j = towers [start, start + cnt)
    std::vector<ofhe_bconv_t> up;       // digit j -> its complement basis (Ql \ digit) | P
    ofhe_bconv_t down = nullptr;        // P -> Ql
    KsTower* d_tow = nullptr;           // [size_ql + size_p]
    TowerScalar* d_pinv = nullptr;      // [size_ql] P^-1 mod q_i
    TowerScalar* d_pmodq = nullptr;     // [size_ql] P mod q_i (m_PModq, rns-cryptoparameters.h:340)
    std::map<u64, TowerScalar*> tscale; // t -> [size_p] t^-1 mod p_j, then [size_ql] t mod q_i
};

// One rescaling step's host tables (rs_build): the k_switch_scale mode, its sw rows, the sc rows of
// the forward-subtract pass (evaluation form) and the scalar applied to the last tower before the lift
struct RsTab {
    int mode = 0;
    std::vector<u64> sw, sc;
    u64 pre = 1;
};

struct ofhe_ks_s {
    ofhe_ctx_t ctx = nullptr;
    u32 log_n = 0, size_q = 0, size_p = 0, num_part_q = 0, alpha = 0;
    std::vector<u64> q, p;
    ofhe_plan_t plan = nullptr;  // towers q[0..size_q) then p[0..size_p)
    hipStream_t side[KS_NSIDE] = {};  // fork streams (options.single_stream: none)
    u32 chunk = 0;                    // ciphertexts per ModUp chunk (options.chunk; 0: the whole batch)
    bool bcols = true;                // k_bconv_cols in ModUp / ModDown (options.separate_cols: off)
    bool icol = true;                 // ... with the INTT's column pass inside it (options.separate_icol: off)
    std::mutex mu;
    std::map<u32, KsLevel*> levels;
    // rescaling tables for dropping tower `towers - 1`, keyed by (towers, t) with t = 0 for CKKS:
    // rescale_run's sw / sc words and ModReduce's negtInvModq (rs_tables)
    std::map<std::pair<u32, u64>, RsTab> rescale;
    // words of a polynomial over Ql (l towers), of one over Ql|P, and of one digit of an evaluation key
    u64 words_q(u32 l) const { return (u64)l << log_n; }
    u64 words_qp(u32 l) const { return (u64)(l + size_p) << log_n; }
    u64 key_stride() const { return words_qp(size_q); }
};

static void level_free(KsLevel* L) {
    if (!L) return;
    for (auto b : L->up) ofhe_hip_bconv_destroy(b);
    if (L->down) ofhe_hip_bconv_destroy(L->down);
    (void)hipFree(L->d_tow);
    (void)hipFree(L->d_pinv);
    (void)hipFree(L->d_pmodq);
    for (auto& kv : L->tscale) (void)hipFree(kv.second);
    delete L;
}

int ofhe_hip_ks_create(ofhe_ctx_t ctx, uint32_t log_n, uint32_t size_q, const uint64_t* q, const uint64_t* psi_q,
                       uint32_t size_p, const uint64_t* p, const uint64_t* psi_p, uint32_t num_part_q,
                       ofhe_ks_t* out) {
    return ofhe_hip_ks_create_ex(ctx, log_n, size_q, q, psi_q, size_p, p, psi_p, num_part_q, nullptr, out);
}

int ofhe_hip_ks_create_ex(ofhe_ctx_t ctx, uint32_t log_n, uint32_t size_q, const uint64_t* q, const uint64_t* psi_q,
                          uint32_t size_p, const uint64_t* p, const uint64_t* psi_p, uint32_t num_part_q,
                          const ofhe_ks_options* options, ofhe_ks_t* out) {
    if (!ctx || !q || !psi_q || !p || !psi_p || !out) return fail(OFHE_ERR_ARG, "NULL argument");
    const ofhe_ks_options opt = options ? *options : ofhe_ks_options{};
    if (opt.separate_cols > 1 || opt.separate_icol > 1 || opt.single_stream > 1)
        return fail(OFHE_ERR_ARG, "options.separate_cols / separate_icol / single_stream must be 0 or 1");
    if (size_q < 1 || size_p < 1 || size_q + size_p > 256) return fail(OFHE_ERR_ARG, "size_q + size_p must be in [2, 256]");
    if (num_part_q < 1 || num_part_q > size_q) return fail(OFHE_ERR_ARG, "num_part_q must be in [1, size_q]");
    const u32 alpha = (size_q + num_part_q - 1) / num_part_q;
    // rns-cryptoparameters.cpp:75-83
    if ((int32_t)(size_q - alpha * (num_part_q - 1)) <= 0)
        return fail(OFHE_ERR_ARG, "HYBRID key switching: can't distribute " + std::to_string(size_q) + " towers into " +
                                      std::to_string(num_part_q) + " digits");
    for (u32 j = 0; j < size_p; j++)
        for (u32 i = 0; i < size_q; i++)
            if (p[j] == q[i]) return fail(OFHE_ERR_ARG, "P and Q moduli must be distinct");
    std::vector<u64> mq(q, q + size_q), mp(p, p + size_p), all(mq), roots(psi_q, psi_q + size_q);
    all.insert(all.end(), mp.begin(), mp.end());
    roots.insert(roots.end(), psi_p, psi_p + size_p);
    ofhe_plan_t plan = nullptr;
    RCCHK(ofhe_hip_plan_create_ex(ctx, log_n, size_q + size_p, all.data(), roots.data(), &opt.plan, &plan));
    ofhe_ks_s* k = new (std::nothrow) ofhe_ks_s();
    if (!k) {
        ofhe_hip_plan_destroy(plan);
        return fail(OFHE_ERR_NOMEM, "key-switch allocation failed");
    }
    k->ctx = ctx;
    k->log_n = log_n;
    k->size_q = size_q;
    k->size_p = size_p;
    k->num_part_q = num_part_q;
    k->alpha = alpha;
    k->q = mq;
    k->p = mp;
    k->plan = plan;
    k->bcols = !opt.separate_cols;
    k->icol = !opt.separate_icol;
    k->chunk = opt.chunk;
    if (!opt.single_stream) {
        hipError_t e = hipSetDevice(ctx->device);
        for (int i = 0; i < KS_NSIDE && e == hipSuccess; i++)
            e = hipStreamCreateWithFlags(&k->side[i], hipStreamNonBlocking);
        if (e != hipSuccess) {
            for (auto& st : k->side)
                if (st) (void)hipStreamDestroy(st);
            ofhe_hip_plan_destroy(plan);
            delete k;
            return fail(OFHE_ERR_HIP, std::string("key-switch streams: ") + hipGetErrorString(e));
        }
    }
    *out = k;
    return OFHE_OK;
}

int ofhe_hip_ks_destroy(ofhe_ks_t k) {
    if (!k) return fail(OFHE_ERR_ARG, "key switch is NULL");
    if (k->ctx) (void)hipSetDevice(k->ctx->device);
    (void)hipDeviceSynchronize();
    for (auto& kv : k->levels) level_free(kv.second);
    for (auto& st : k->side)
        if (st) (void)hipStreamDestroy(st);
    if (k->plan) ofhe_hip_plan_destroy(k->plan);
    delete k;
    return OFHE_OK;
}

int ofhe_hip_ks_digits(ofhe_ks_t k, uint32_t size_ql, uint32_t* alpha, uint32_t* beta) {
    if (!k || !k->ctx) return fail(OFHE_ERR_STATE, "key switch is NULL or destroyed");
    if (size_ql < 1 || size_ql > k->size_q) return fail(OFHE_ERR_ARG, "size_ql must be in [1, size_q]");
    // keyswitch-hybrid.cpp:341-345
    u32 b = (size_ql + k->alpha - 1) / k->alpha;
    if (b > k->num_part_q) b = k->num_part_q;
    if (alpha) *alpha = k->alpha;
    if (beta) *beta = b;
    return OFHE_OK;
}

// Tables of one level l = size_ql - 1 (built once, kept resident).
static int level_get(ofhe_ks_t k, u32 size_ql, KsLevel** out) {
    std::lock_guard<std::mutex> lk(k->mu);
    auto it = k->levels.find(size_ql);
    if (it != k->levels.end()) {
        *out = it->second;
        return OFHE_OK;
    }
    u32 beta = 0;
    RCCHK(ofhe_hip_ks_digits(k, size_ql, nullptr, &beta));
    KsLevel* L = new (std::nothrow) KsLevel();
    if (!L) return fail(OFHE_ERR_NOMEM, "level allocation failed");
    const u32 P = k->size_p, l = size_ql;
    L->beta = beta;
    L->size_ql = l;
    int rc = OFHE_OK;
    for (u32 j = 0; j < L->beta && rc == OFHE_OK; j++) {
        // digit j (keyswitch-hybrid.cpp:352-378) and its complement
        // (m_paramsComplPartQ, rns-cryptoparameters.cpp:238-287)
        const u32 st = j * k->alpha, n = std::min(k->alpha, l - st);
        L->start.push_back(st);
        L->cnt.push_back(n);
        const u64* dq = k->q.data() + st;
        std::vector<u64> compl_;
        for (u32 i = 0; i < l; i++)
            if (i < st || i >= st + n) compl_.push_back(k->q[i]);
        compl_.insert(compl_.end(), k->p.begin(), k->p.end());
        const u32 C = (u32)compl_.size();
        std::vector<u64> hinv(n), hmod((size_t)n * C);
        for (u32 i = 0; i < n; i++) {
            // m_PartQlHatInvModq[j][n-1][i] (rns-cryptoparameters.cpp:289-312)
            hinv[i] = invmod(prod_mod(dq, n, i, dq[i]), dq[i]);
            // m_PartQlHatModp[l][j][i][c] (314-341)
            for (u32 c = 0; c < C; c++) hmod[(size_t)i * C + c] = prod_mod(dq, n, i, compl_[c]);
        }
        ofhe_bconv_t b = nullptr;
        rc = ofhe_hip_bconv_create(k->ctx, k->log_n, n, C, dq, compl_.data(), hinv.data(), hmod.data(), &b);
        if (rc == OFHE_OK) L->up.push_back(b);
    }
    if (rc == OFHE_OK) {
        // ApproxModDown tables: PHatInvModp, PHatModq, PInvModq (172-215)
        std::vector<u64> hinv(P), hmod((size_t)P * l);
        for (u32 j = 0; j < P; j++) {
            hinv[j] = invmod(prod_mod(k->p.data(), P, j, k->p[j]), k->p[j]);
            for (u32 i = 0; i < l; i++) hmod[(size_t)j * l + i] = prod_mod(k->p.data(), P, j, k->q[i]);
        }
        rc = ofhe_hip_bconv_create(k->ctx, k->log_n, P, l, k->p.data(), k->q.data(), hinv.data(), hmod.data(),
                                   &L->down);
    }
    if (rc == OFHE_OK) {
        const u64 N = 1ull << k->log_n;
        std::vector<KsTower> tow(l + P);
        for (u32 i = 0; i < l + P; i++) {
            const bool isq = i < l;
            const u64 m = isq ? k->q[i] : k->p[i - l];
            u64 mu[2], lr[3];
            barrett128(m, mu);
            limb_red_consts(m, lr);
            tow[i] = KsTower{m, mu[0], mu[1], (isq ? i : k->size_q + i - l) * N, lr[0], lr[1], lr[2]};
        }
        std::vector<TowerScalar> pinv(l), pmodq(l);
        for (u32 i = 0; i < l; i++) {
            const u64 pm = prod_mod(k->p.data(), P, P, k->q[i]);
            pinv[i] = scalar_of(k->q[i], invmod(pm, k->q[i]));
            pmodq[i] = scalar_of(k->q[i], pm);
        }
        const int dev = k->ctx->device;
        rc = alloc_upload(&L->d_tow, tow.data(), sizeof(KsTower) * tow.size(), "level upload", dev);
        if (rc == OFHE_OK)
            rc = alloc_upload(&L->d_pinv, pinv.data(), sizeof(TowerScalar) * pinv.size(), "level upload", dev);
        if (rc == OFHE_OK)
            rc = alloc_upload(&L->d_pmodq, pmodq.data(), sizeof(TowerScalar) * pmodq.size(), "level upload", dev);
    }
    if (rc != OFHE_OK) {
        level_free(L);
        return rc;
    }
    k->levels[size_ql] = L;
    *out = L;
    return OFHE_OK;
}

static int level_t_tables(ofhe_ks_t k, KsLevel* L, u64 t, const TowerScalar** out) {
    return cached_table(k->mu, L->tscale, t, "t tables", out,
                        [&] { return t_tables(k->p.data(), k->size_p, k->q.data(), L->size_ql, t); });
}

// The key-switch engine's ApproxModDown (P -> the level's Q towers) with
// plaintext modulus t (0: none)
static int ks_md_args(ofhe_ks_t k, KsLevel* L, u64 t, ModDownArgs* A) {
    const TowerScalar* tt = nullptr;
    if (t) RCCHK(level_t_tables(k, L, t, &tt));
    *A = ModDownArgs{k->plan, k->plan, 0, k->size_q, L->size_ql, k->size_p, L->down->args, L->d_pinv,
                     tt, tt ? tt + k->size_p : nullptr, k->bcols, k->icol};
    return OFHE_OK;
}

// Fork of the caller's stream onto the engine's two side streams, so that
// independent digits (ModUp) and the two ModDowns overlap: each alone is a
// sequence of short launches over a few towers that leaves the chip partly
// idle at its head and tail.  The join (explicit, or in the destructor on an
// error path) puts the caller's stream behind both; declare a KsFork after
// any stream-ordered Scratch its work uses, so it joins before they are freed.
struct KsFork {
    hipStream_t parent = nullptr;
    hipStream_t f[KS_NSIDE] = {};
    hipEvent_t ev[KS_NSIDE + 1] = {};
    bool forked = false;
    int open(ofhe_ks_t k, hipStream_t s) {
        parent = s;
        for (auto& x : f) x = s;
        if (!k->side[0]) return OFHE_OK;
        for (auto& e : ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIPCHK(hipEventRecord(ev[0], s));
        for (int i = 0; i < KS_NSIDE; i++) HIPCHK(hipStreamWaitEvent(k->side[i], ev[0], 0));
        for (int i = 0; i < KS_NSIDE; i++) f[i] = k->side[i];
        forked = true;
        return OFHE_OK;
    }
    int join() {
        if (!forked) return OFHE_OK;
        forked = false;
        for (int i = 0; i < KS_NSIDE; i++) {
            HIPCHK(hipEventRecord(ev[1 + i], f[i]));
            HIPCHK(hipStreamWaitEvent(parent, ev[1 + i], 0));
        }
        return OFHE_OK;
    }
    ~KsFork() {
        (void)join();
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

static int ks_check(ofhe_ks_t k, u32 size_ql, u32 batch) {
    if (!k || !k->ctx) return fail(OFHE_ERR_STATE, "key switch is NULL or destroyed");
    if (size_ql < 1 || size_ql > k->size_q) return fail(OFHE_ERR_ARG, "size_ql must be in [1, size_q]");
    if (batch == 0) return fail(OFHE_ERR_ARG, "batch must be >= 1");
    HIPCHK(hipSetDevice(k->ctx->device));
    return OFHE_OK;
}

// The prologue of an entry point that works at one level: the engine checks, then that level's tables
static int ks_enter(ofhe_ks_t k, u32 size_ql, u32 batch, KsLevel** L) {
    RCCHK(ks_check(k, size_ql, batch));
    return level_get(k, size_ql, L);
}

// EvalKeySwitchPrecomputeCore; with own_copy = false the digit's own towers
// are left out of its slot (KeySwitchCore's inner product reads them from c).
static int ks_precompute_impl(ofhe_ks_t k, KsLevel* L, uint32_t size_ql, const uint64_t* c, uint64_t* digits,
                              uint32_t batch, hipStream_t stream, bool own_copy) {
    KsFork fk;
    RCCHK(fk.open(k, stream));
    const u64 N = 1ull << k->log_n, l = size_ql, P = k->size_p, poly = k->words_qp(l), ds = L->beta * poly;
    // ModUp in chunks of ciphertexts (OFHE_KS_CHUNK), so that a chunk's
    // converted towers can still sit in the Infinity Cache when its forward
    // transform reads them
    const u32 cb = k->chunk && k->chunk < batch ? k->chunk : batch;
    for (u32 b0 = 0; b0 < batch; b0 += cb)
    for (u32 j = 0; j < L->beta; j++) {
        const u32 st = L->start[j], n = L->cnt[j];
        const u32 batch_ = std::min(cb, batch - b0);
        hipStream_t s = fk.f[j % KS_NSIDE];  // digits are independent
        u64* slot = digits + (u64)b0 * ds + j * poly;
        const uint64_t* c_ = c + (u64)b0 * l * N;
        // ApproxSwitchCRTBasis to the complement, written around the digit slot (388-406)
        BconvArgs B = L->up[j]->args;
        B.in_stride = B.out_stride = ds;
        B.gap_at = st;
        B.gap = n;
        B.lazy_out = 1;  // every complement tower goes through a forward NTT below
        const bool cols = k->bcols && l == k->size_q && bconv_cols_ok(k->plan, B);
        // partsCt[j] in coefficient form (keyswitch-hybrid.cpp:384-385); with
        // k->icol only its block pass here, its column pass inside the conversion
        if (cols && k->icol)
            RCCHK(plan_ntt_inv_block(k->plan, st, n, c_ + st * N, l * N, slot + st * N, ds, batch_, s));
        else
            RCCHK(plan_ntt_range(k->plan, true, st, n, c_ + st * N, slot + st * N, l * N, ds, batch_, s));
        if (cols) {
            // full level (slot towers = plan towers): the conversion writes the
            // complement's column-pass output, the block passes finish it (394)
            RCCHK(bconv_cols_run(k->plan, 0, B, slot + st * N, slot, batch_, s, k->icol ? (int)st : -1));
            if (st) RCCHK(plan_ntt_fwd_block(k->plan, 0, st, slot, ds, batch_, s));
            RCCHK(plan_ntt_fwd_block(k->plan, st + n, (u32)(l + P) - st - n, slot + (st + n) * N, ds, batch_, s));
            if (own_copy) RCCHK(copy_rows(slot + st * N, ds, c_ + st * N, l * N, (u64)n * N, batch_, s));
            continue;
        }
        RCCHK(bconv_run(B, slot + st * N, slot, batch_, s));
        // complement towers to evaluation form (394)
        RCCHK(plan_ntt_range(k->plan, false, 0, st, slot, slot, ds, ds, batch_, s));
        if (l == k->size_q) {
            // full level: the Q towers after the digit and the P towers are
            // adjacent both in the plan and in the slot -- one launch
            RCCHK(plan_ntt_range(k->plan, false, st + n, (u32)(l + P) - st - n, slot + (st + n) * N,
                                 slot + (st + n) * N, ds, ds, batch_, s));
        } else {
            RCCHK(plan_ntt_range(k->plan, false, st + n, (u32)l - st - n, slot + (st + n) * N, slot + (st + n) * N,
                                 ds, ds, batch_, s));
            RCCHK(plan_ntt_range(k->plan, false, k->size_q, (u32)P, slot + l * N, slot + l * N, ds, ds, batch_, s));
        }
        // the digit's own towers stay as given (evaluation form, 402-404)
        if (own_copy) RCCHK(copy_rows(slot + st * N, ds, c_ + st * N, l * N, (u64)n * N, batch_, s));
    }
    return fk.join();
}

int ofhe_hip_ks_precompute(ofhe_ks_t k, uint32_t size_ql, const uint64_t* c, uint64_t* digits, uint32_t batch,
                           void* stream) {
    KsLevel* L = nullptr;
    RCCHK(ks_enter(k, size_ql, batch, &L));
    if (!c || !digits) return fail(OFHE_ERR_ARG, "NULL data pointer");
    return ks_precompute_impl(k, L, size_ql, c, digits, batch, pick(stream), true);
}

// EvalFastKeySwitchCoreExt; c != NULL: the digits' own towers come from c
// (see ks_precompute_impl), which only the batch-stationary kernel supports.
static int ks_fast_core_ext_impl(ofhe_ks_t k, KsLevel* L, uint32_t size_ql, const uint64_t* digits,
                                 const uint64_t* key_b, const uint64_t* key_a, uint64_t* ct0, uint64_t* ct1,
                                 uint32_t batch, void* stream, const uint64_t* c) {
    const u32 towers = size_ql + k->size_p;
    const u64 key_stride = k->key_stride();
    if (L->beta <= 4) {
        // batch-stationary keys: one thread per (tower, OFHE_KS_CPT coefficients)
        const u64 rows = k->words_qp(size_ql) / OFHE_KS_CPT;
        dim3 g, blk(256);
        RCCHK(coeff_grid(rows, &g));
        hipStream_t s = pick(stream);
        KsOwn own{};
        for (u32 j = 0; j < L->beta; j++) {
            own.start[j] = L->start[j];
            own.cnt[j] = L->cnt[j];
        }
        const u64 c_stride = k->words_q(size_ql);
        // beta is in [1, 4] here (ofhe_hip_ks_digits); anything else took the beta = 4 kernel before too
        with_int<1, 2, 3, 4>(L->beta ? (int)L->beta : 4, [&](auto B_) {
            hipLaunchKernelGGL((k_ks_inner_bs<decltype(B_)::value, OFHE_KS_CPT>), g, blk, 0, s, L->d_tow, digits, key_b,
                               key_a, ct0, ct1, key_stride, batch, rows, k->log_n, towers, c, c_stride, own);
        });
    } else {
        if (c) return fail(OFHE_ERR_STATE, "internal: own-tower reads need beta <= 4");
        const u64 npairs = batch * k->words_qp(size_ql) / 2;
        hipLaunchKernelGGL(k_ks_inner, dim3(grid_for(npairs)), dim3(256), 0, pick(stream), L->d_tow, digits, key_b,
                           key_a, ct0, ct1, key_stride, L->beta, npairs, k->log_n, towers);
    }
    return post_launch();
}

int ofhe_hip_ks_fast_core_ext(ofhe_ks_t k, uint32_t size_ql, const uint64_t* digits, const uint64_t* key_b,
                              const uint64_t* key_a, uint64_t* ct0, uint64_t* ct1, uint32_t batch, void* stream) {
    KsLevel* L = nullptr;
    RCCHK(ks_enter(k, size_ql, batch, &L));
    if (!digits || !key_b || !key_a || !ct0 || !ct1) return fail(OFHE_ERR_ARG, "NULL data pointer");
    return ks_fast_core_ext_impl(k, L, size_ql, digits, key_b, key_a, ct0, ct1, batch, stream, nullptr);
}

static int ks_mod_down_impl(ofhe_ks_t k, KsLevel* L, const u64* x, u64* out, u64 t, u32 batch, hipStream_t s) {
    ModDownArgs A;
    RCCHK(ks_md_args(k, L, t, &A));
    return mod_down_run(A, x, k->words_qp(L->size_ql), &out, 1, k->words_q(L->size_ql), batch, s);
}

int ofhe_hip_ks_mod_down(ofhe_ks_t k, uint32_t size_ql, const uint64_t* x, uint64_t* out, uint64_t t, uint32_t batch,
                         void* stream) {
    KsLevel* L = nullptr;
    RCCHK(ks_enter(k, size_ql, batch, &L));
    if (!x || !out) return fail(OFHE_ERR_ARG, "NULL data pointer");
    return ks_mod_down_impl(k, L, x, out, t, batch, pick(stream));
}

// KeySwitchCore of c into out0 / out1, plus add0 / add1 when given (mod_down_run)
static int ks_core_impl(ofhe_ks_t k, KsLevel* L, u32 size_ql, const u64* c, const u64* key_b, const u64* key_a,
                        u64* out0, u64* out1, const u64* add0, const u64* add1, u64 t, u32 batch, hipStream_t s) {
    const u64 poly = k->words_qp(size_ql);
    Scratch dg, ct;
    RCCHK(dg.alloc((size_t)batch * L->beta * poly * 8, s, k->ctx));
    RCCHK(ct.alloc((size_t)2 * batch * poly * 8, s, k->ctx));
    u64* c0 = ct.w();
    u64* c1 = ct.w() + (u64)batch * poly;
    // the inner product reads each digit's own towers straight from c (beta <= 4),
    // so the precompute skips copying them into the digit slots
    const bool own_from_c = L->beta <= 4;
    RCCHK(ks_precompute_impl(k, L, size_ql, c, dg.w(), batch, s, !own_from_c));
    RCCHK(ks_fast_core_ext_impl(k, L, size_ql, dg.w(), key_b, key_a, c0, c1, batch, s, own_from_c ? c : nullptr));
    // both ModDowns in one set of launches over 2 x batch (c1 = c0 + batch * poly)
    ModDownArgs A;
    RCCHK(ks_md_args(k, L, t, &A));
    u64* const outs[2] = {out0, out1};
    const u64* const adds[2] = {add0, add1};
    return mod_down_run(A, c0, poly, outs, 2, k->words_q(size_ql), batch, s, add0 ? adds : nullptr);
}

int ofhe_hip_ks_core(ofhe_ks_t k, uint32_t size_ql, const uint64_t* c, const uint64_t* key_b, const uint64_t* key_a,
                     uint64_t* out0, uint64_t* out1, uint64_t t, uint32_t batch, void* stream) {
    KsLevel* L = nullptr;
    RCCHK(ks_enter(k, size_ql, batch, &L));
    if (!c || !key_b || !key_a || !out0 || !out1) return fail(OFHE_ERR_ARG, "NULL data pointer");
    return ks_core_impl(k, L, size_ql, c, key_b, key_a, out0, out1, nullptr, nullptr, t, batch, pick(stream));
}

// ---------------------------------------------------------------------------
// Hoisted rotations: many keys over one digit set
// ---------------------------------------------------------------------------
// inverse of an odd k modulo 2^32 (Newton: k is its own inverse mod 8)
static u32 inv_odd32(u32 k) {
    u32 x = k;
    for (int i = 0; i < 4; i++) x *= 2 - k * x;
    return x;
}

// an index that is 1 modulo 2N (id_mask = 2N - 1) is the identity: no rotation, no key read
static bool rot_is_id(u32 index, u32 id_mask) { return (index & id_mask) == 1; }

// The rules of a list of n rotations: every key given, every index odd.
// key_b = NULL checks the indices alone (the BSGS call tests them before it has
// an engine); id_mask = 2N - 1 lets identity steps go without keys (BSGS again),
// 0 exempts none.
static int rot_list_check(u32 n, const u32* index, const u64* const* key_b, const u64* const* key_a,
                          u32 id_mask = 0) {
    for (u32 r = 0; r < n; r++) {
        if (key_b && !rot_is_id(index[r], id_mask) && (!key_b[r] || !key_a[r]))
            return fail(OFHE_ERR_ARG, "NULL evaluation key pointer");
        if (index[r] % 2 == 0) return fail(OFHE_ERR_ARG, "Automorphism index not odd");  // poly-impl.h:333-334
    }
    return OFHE_OK;
}

// Argument checks shared by the two calls, and their level; kinv[r] = auto_index[r]^-1.
static int rot_check(ofhe_ks_t k, u32 size_ql, const u64* digits, u32 nrot, const u32* auto_index,
                     const u64* const* key_b, const u64* const* key_a, const u64* out0, const u64* out1, u32 batch,
                     std::vector<u32>& kinv, KsLevel** L) {
    RCCHK(ks_enter(k, size_ql, batch, L));
    if (!digits || !out0 || !out1) return fail(OFHE_ERR_ARG, "NULL data pointer");
    if (!auto_index || !key_b || !key_a) return fail(OFHE_ERR_ARG, "NULL index or key pointer array");
    if (nrot == 0) return fail(OFHE_ERR_ARG, "nrot must be >= 1");
    if (out0 == out1) return fail(OFHE_ERR_ARG, "out0 and out1 must be distinct buffers");
    RCCHK(rot_list_check(nrot, auto_index, key_b, key_a));
    kinv.resize(nrot);
    for (u32 r = 0; r < nrot; r++) kinv[r] = inv_odd32(auto_index[r]);
    return OFHE_OK;
}

// f(j0, n) for the chunks [j0, j0 + n) of at most KS_ROT_CAP items, the most one
// launch's arguments carry; or_once: one call f(0, 0) for an empty list, whose
// launch still has other work to do
template <class F>
static int rot_chunks(u32 total, bool or_once, F&& f) {
    if (!total && or_once) return f(0u, 0u);
    for (u32 j0 = 0; j0 < total; j0 += KS_ROT_CAP) RCCHK(f(j0, std::min(KS_ROT_CAP, total - j0)));
    return OFHE_OK;
}

// k_ks_inner_rot / k_ks_inner_rot_wide for nrot <= KS_ROT_CAP rotations
static int ks_inner_rot(ofhe_ks_t k, KsLevel* L, u32 size_ql, const u64* digits, const u64* c0, u32 nrot,
                        const u32* kinv, const u64* const* key_b, const u64* const* key_a, u64* out0, u64* out1,
                        u64 rot_stride, u32 batch, hipStream_t s) {
    KsRot R{};
    for (u32 r = 0; r < nrot; r++) {
        R.kb[r] = key_b[r];
        R.ka[r] = key_a[r];
        R.kinv[r] = kinv[r];
    }
    const u32 towers = size_ql + k->size_p;
    const u64 key_stride = k->key_stride(), nthreads = batch * k->words_qp(size_ql);
    dim3 g, blk(256);
    RCCHK(coeff_grid(nthreads, &g));
    const bool narrow = with_int<1, 2, 3, 4>((int)L->beta, [&](auto B_) {
        hipLaunchKernelGGL((k_ks_inner_rot<decltype(B_)::value>), g, blk, 0, s, L->d_tow, digits, c0, L->d_pmodq, R,
                           nrot, out0, out1, key_stride, rot_stride, nthreads, k->log_n, towers, size_ql);
    });
    if (!narrow)
        hipLaunchKernelGGL(k_ks_inner_rot_wide, g, blk, 0, s, L->d_tow, digits, c0, L->d_pmodq, R, nrot, out0, out1,
                           key_stride, rot_stride, nthreads, L->beta, k->log_n, towers, size_ql);
    return post_launch();
}

int ofhe_hip_ks_fast_rotation_ext(ofhe_ks_t k, uint32_t size_ql, const uint64_t* digits, const uint64_t* c0,
                                  uint32_t nrot, const uint32_t* auto_index, const uint64_t* const* key_b,
                                  const uint64_t* const* key_a, uint64_t* out0, uint64_t* out1, uint32_t batch,
                                  void* stream) {
    std::vector<u32> kinv;
    KsLevel* L = nullptr;
    RCCHK(rot_check(k, size_ql, digits, nrot, auto_index, key_b, key_a, out0, out1, batch, kinv, &L));
    const u64 rot_stride = batch * k->words_qp(size_ql);
    return rot_chunks(nrot, false, [&](u32 r0, u32 nr) {
        return ks_inner_rot(k, L, size_ql, digits, c0, nr, kinv.data() + r0, key_b + r0, key_a + r0,
                            out0 + r0 * rot_stride, out1 + r0 * rot_stride, rot_stride, batch, pick(stream));
    });
}

int ofhe_hip_ks_fast_rotation(ofhe_ks_t k, uint32_t size_ql, const uint64_t* digits, const uint64_t* c0,
                              uint32_t nrot, const uint32_t* auto_index, const uint64_t* const* key_b,
                              const uint64_t* const* key_a, uint64_t* out0, uint64_t* out1, uint64_t t,
                              uint32_t batch, void* stream) {
    std::vector<u32> kinv;
    KsLevel* L = nullptr;
    RCCHK(rot_check(k, size_ql, digits, nrot, auto_index, key_b, key_a, out0, out1, batch, kinv, &L));
    if (!c0) return fail(OFHE_ERR_ARG, "NULL data pointer");
    hipStream_t s = pick(stream);
    ModDownArgs A;
    RCCHK(ks_md_args(k, L, t, &A));
    const u32 l = L->size_ql;
    const u64 poly = k->words_qp(l), per_rot = batch * k->words_q(l);
    u32 one[KS_ROT_CAP];
    for (auto& v : one) v = 1;
    // the order of the reference: ModDown, += c0, then the automorphism
    // (ModDown and the automorphism do not commute bit for bit)
    return rot_chunks(nrot, false, [&](u32 r0, u32 nr) -> int {
        Scratch ct, md;
        RCCHK(ct.alloc((size_t)2 * nr * batch * poly * 8, s, k->ctx));
        RCCHK(md.alloc((size_t)2 * nr * per_rot * 8, s, k->ctx));
        // ct0 of every (rotation, batch entry), then ct1 of every one: the two
        // ModDowns of all rotations run as one launch set over nr * batch
        u64* ct1 = ct.w() + (u64)nr * batch * poly;
        u64* md1 = md.w() + (u64)nr * per_rot;
        RCCHK(ks_inner_rot(k, L, size_ql, digits, nullptr, nr, one, key_b + r0, key_a + r0, ct.w(), ct1,
                           (u64)batch * poly, batch, s));
        u64* const mds[2] = {md.w(), md1};
        RCCHK(mod_down_run(A, ct.w(), poly, mds, 2, k->words_q(l), nr * batch, s));
        KsRotIdx I{};
        for (u32 r = 0; r < nr; r++) I.kinv[r] = kinv[r0 + r];
        hipLaunchKernelGGL(k_add_automorphism, dim3(grid_for(per_rot), nr), dim3(256), 0, s, L->d_tow, md.w(), md1,
                           c0, out0 + r0 * per_rot, out1 + r0 * per_rot, I, per_rot, k->log_n, l);
        return post_launch();
    });
}

// ---------------------------------------------------------------------------
// BSGS linear transform (FHECKKSRNS::EvalLinearTransform, ckksrns-fhe.cpp:1484-1555;
// the loops of EvalCoeffsToSlots / EvalSlotsToCoeffs, 1636-1698): lt_kernels.hpp
// ---------------------------------------------------------------------------
static int ks_ext_impl(ofhe_ks_t k, KsLevel* L, const u64* c, u64* out, u32 batch, hipStream_t s) {
    const u32 towers = L->size_ql + k->size_p;
    const u64 nthreads = batch * k->words_qp(L->size_ql);
    dim3 g;
    RCCHK(coeff_grid(nthreads, &g));
    hipLaunchKernelGGL(k_ks_ext, g, dim3(256), 0, s, L->d_pmodq, c, out, nthreads, k->log_n, towers, L->size_ql);
    return post_launch();
}

int ofhe_hip_ks_ext(ofhe_ks_t k, uint32_t size_ql, const uint64_t* c, uint64_t* out, uint32_t batch, void* stream) {
    if (!c || !out) return fail(OFHE_ERR_ARG, "NULL data pointer");
    // ahead of the engine's checks, which would report a missing engine first
    if (batch == 0) return fail(OFHE_ERR_ARG, "batch must be >= 1");
    KsLevel* L = nullptr;
    RCCHK(ks_enter(k, size_ql, batch, &L));
    if (words_overlap(c, batch * k->words_q(size_ql), out, batch * k->words_qp(size_ql)))
        return fail(OFHE_ERR_ARG, "out must not alias c");
    return ks_ext_impl(k, L, c, out, batch, pick(stream));
}

// k_lt_inner for the sums rows[0..nsum) (diagonal rows; sum g is written at
// out + g * out_stride) over nterm terms: chunks of LT_SUM_CAP sums per launch
// and of LT_TERM_CAP terms, the later term chunks adding into the stored sums.
static int lt_inner_run(ofhe_ks_t k, KsLevel* L, u32 nterm, const u64* x0, const u64* x1, u64 x_stride,
                        const u64* diag, u64 diag_stride, const uint8_t* present, const u32* rows, u32 nsum,
                        u64* out0, u64* out1, u32 batch, hipStream_t s) {
    const u32 towers = L->size_ql + k->size_p;
    const u64 nthreads = batch * k->words_qp(L->size_ql);
    dim3 g, blk(256);
    RCCHK(coeff_grid(nthreads, &g));
    for (u32 g0 = 0; g0 < nsum; g0 += LT_SUM_CAP) {
        const u32 ns = std::min(LT_SUM_CAP, nsum - g0);
        for (u32 i0 = 0; i0 < nterm; i0 += LT_TERM_CAP) {
            const u32 nt = std::min(LT_TERM_CAP, nterm - i0);
            LtSums S{};
            for (u32 j = 0; j < ns; j++) {
                S.row[j] = rows[g0 + j];
                u32 m = 0;
                for (u32 i = 0; i < nt; i++)
                    if (!present || present[(size_t)rows[g0 + j] * nterm + i0 + i]) m |= 1u << i;
                S.mask[j] = m;
            }
            with_int<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>((int)nt, [&](auto NT_) {
                hipLaunchKernelGGL((k_lt_inner<decltype(NT_)::value>), g, blk, 0, s, L->d_tow, x0 + i0 * x_stride,
                                   x1 + i0 * x_stride, x_stride, diag + i0 * diag_stride, diag_stride,
                                   (u64)nterm * diag_stride, S, ns, out0 + g0 * nthreads, out1 + g0 * nthreads,
                                   nthreads, nthreads, k->log_n, towers, i0 ? 1u : 0u);
            });
            RCCHK(post_launch());
        }
    }
    return OFHE_OK;
}

// The aliasing policy of a pair of outputs of ow words each (that they are two
// buffers, out0 != out1, is tested ahead of the engine): they do not overlap ...
static int outputs_apart(const u64* out0, const u64* out1, u64 ow) {
    if (words_overlap(out0, ow, out1, ow)) return fail(OFHE_ERR_ARG, "out0 and out1 overlap");
    return OFHE_OK;
}
// ... and, first, neither overlaps a span of input words (a NULL span is an absent input)
struct WordSpan {
    const u64* p;
    u64 words;
};
static int outputs_check(const u64* out0, const u64* out1, u64 ow, std::initializer_list<WordSpan> inputs) {
    for (const u64* o : {out0, out1})
        for (const WordSpan& in : inputs)
            if (in.p && words_overlap(o, ow, in.p, in.words))
                return fail(OFHE_ERR_ARG, "outputs must not alias inputs");
    return outputs_apart(out0, out1, ow);
}

int ofhe_hip_ks_mult_ext_sum(ofhe_ks_t k, uint32_t size_ql, uint32_t nterm, const uint64_t* x0, const uint64_t* x1,
                             uint64_t x_stride, const uint64_t* diag, uint64_t diag_stride, const uint8_t* present,
                             uint32_t nsum, uint64_t* out0, uint64_t* out1, uint32_t batch, void* stream) {
    // the checks that need no engine first, then the engine, then those that need its dimensions
    if (!x0 || !x1 || !diag || !out0 || !out1) return fail(OFHE_ERR_ARG, "NULL data pointer");
    if (nterm == 0 || nsum == 0 || batch == 0) return fail(OFHE_ERR_ARG, "nterm, nsum and batch must be >= 1");
    if (out0 == out1) return fail(OFHE_ERR_ARG, "out0 and out1 must be distinct buffers");
    KsLevel* L = nullptr;
    RCCHK(ks_enter(k, size_ql, batch, &L));
    const u64 poly = k->words_qp(size_ql), per = batch * poly;
    if (diag_stride < poly) return fail(OFHE_ERR_ARG, "diag_stride smaller than one diagonal");
    if (x_stride < per) return fail(OFHE_ERR_ARG, "x_stride smaller than one term");
    const u64 xw = (u64)(nterm - 1) * x_stride + per;
    RCCHK(outputs_check(out0, out1, (u64)nsum * per,
                        {{x0, xw}, {x1, xw}, {diag, ((u64)nsum * nterm - 1) * diag_stride + poly}}));
    std::vector<u32> rows(nsum);
    for (u32 j = 0; j < nsum; j++) rows[j] = j;
    return lt_inner_run(k, L, nterm, x0, x1, x_stride, diag, diag_stride, present, rows.data(), nsum, out0, out1,
                        batch, pick(stream));
}

// k_lt_outer over nset digit sets (KS_ROT_CAP per launch, the later launches
// adding into the stored result) plus nadd addends of element 1
static int lt_outer_run(ofhe_ks_t k, KsLevel* L, const u64* digits, u32 nset, const u32* index,
                        const u64* const* key_b, const u64* const* key_a, const u64* add1, u32 nadd, u64* out0,
                        u64* out1, u32 batch, hipStream_t s) {
    const u32 towers = L->size_ql + k->size_p;
    const u64 poly = k->words_qp(L->size_ql), nthreads = batch * poly, key_stride = k->key_stride();
    dim3 g, blk(256);
    RCCHK(coeff_grid(nthreads, &g));
    return rot_chunks(nset, true, [&](u32 j0, u32 ns) {
        LtRot R{};
        for (u32 j = 0; j < ns; j++) {
            R.kb[j] = key_b[j0 + j];
            R.ka[j] = key_a[j0 + j];
            R.k[j] = index[j0 + j];
        }
        const u64* dg = digits ? digits + (u64)j0 * batch * L->beta * poly : nullptr;
        auto launch = [&](auto B_) {
            hipLaunchKernelGGL((k_lt_outer<decltype(B_)::value>), g, blk, 0, s, L->d_tow, dg, R, ns, add1,
                               j0 ? 0u : nadd, out0, out1, key_stride, nthreads, L->beta, k->log_n, towers, batch,
                               j0 ? 1u : 0u);
        };
        if (!with_int<1, 2, 3, 4>((int)L->beta, launch)) launch(std::integral_constant<int, 0>{});
        return post_launch();
    });
}

int ofhe_hip_ks_fast_rotation_ext_sum(ofhe_ks_t k, uint32_t size_ql, uint32_t nset, const uint64_t* digits,
                                      const uint32_t* auto_index, const uint64_t* const* key_b,
                                      const uint64_t* const* key_a, const uint64_t* addend1, uint32_t nadd,
                                      uint64_t* out0, uint64_t* out1, uint32_t batch, void* stream) {
    if (!digits || !out0 || !out1) return fail(OFHE_ERR_ARG, "NULL data pointer");
    if (!auto_index || !key_b || !key_a) return fail(OFHE_ERR_ARG, "NULL index or key pointer array");
    if (nset == 0 || batch == 0) return fail(OFHE_ERR_ARG, "nset and batch must be >= 1");
    if (out0 == out1) return fail(OFHE_ERR_ARG, "out0 and out1 must be distinct buffers");
    if ((addend1 == nullptr) != (nadd == 0)) return fail(OFHE_ERR_ARG, "addend1 and nadd must be given together");
    RCCHK(rot_list_check(nset, auto_index, key_b, key_a));
    KsLevel* L = nullptr;
    RCCHK(ks_enter(k, size_ql, batch, &L));
    const u64 per = batch * k->words_qp(size_ql);
    RCCHK(outputs_check(out0, out1, per, {{digits, (u64)nset * L->beta * per}, {addend1, (u64)nadd * per}}));
    return lt_outer_run(k, L, digits, nset, auto_index, key_b, key_a, addend1, nadd, out0, out1, batch,
                        pick(stream));
}

int ofhe_hip_ks_bsgs_transform(ofhe_ks_t k, uint32_t size_ql, const ofhe_bsgs* tr, const uint64_t* c0,
                               const uint64_t* c1, uint64_t* out0, uint64_t* out1, uint64_t t, uint32_t batch,
                               void* stream) {
    // the checks that need no engine first, then the engine, then those that need its dimensions
    if (!tr || !c0 || !c1 || !out0 || !out1 || !tr->diag) return fail(OFHE_ERR_ARG, "NULL data pointer");
    if (!tr->baby_index || !tr->giant_index || !tr->baby_key_b || !tr->baby_key_a || !tr->giant_key_b ||
        !tr->giant_key_a)
        return fail(OFHE_ERR_ARG, "NULL index or key pointer array");
    const u32 nb = tr->nbaby, ng = tr->ngiant;
    if (nb == 0 || ng == 0 || batch == 0) return fail(OFHE_ERR_ARG, "nbaby, ngiant and batch must be >= 1");
    if (out0 == out1) return fail(OFHE_ERR_ARG, "out0 and out1 must be distinct buffers");
    RCCHK(rot_list_check(nb, tr->baby_index, nullptr, nullptr));
    RCCHK(rot_list_check(ng, tr->giant_index, nullptr, nullptr));
    KsLevel* L = nullptr;
    RCCHK(ks_enter(k, size_ql, batch, &L));
    const u32 l = size_ql;
    const u64 poly = k->words_qp(l), per = batch * poly, qw = k->words_q(l), qper = batch * qw;
    if (tr->diag_stride < poly) return fail(OFHE_ERR_ARG, "diag_stride smaller than one diagonal");
    const u32 m2 = (u32)((2ull << k->log_n) - 1);
    auto is_id = [&](u32 idx) { return rot_is_id(idx, m2); };
    RCCHK(rot_list_check(nb, tr->baby_index, tr->baby_key_b, tr->baby_key_a, m2));
    RCCHK(rot_list_check(ng, tr->giant_index, tr->giant_key_b, tr->giant_key_a, m2));
    RCCHK(outputs_check(out0, out1, qper,
                        {{c0, qper}, {c1, qper}, {tr->diag, ((u64)nb * ng - 1) * tr->diag_stride + poly}}));
    hipStream_t s = pick(stream);
    ModDownArgs A;
    RCCHK(ks_md_args(k, L, t, &A));

    // giant steps: the non-identity ones first, then the identity ones
    std::vector<u32> rows, gidx;
    std::vector<const u64*> gkb, gka;
    for (int pass = 0; pass < 2; pass++)
        for (u32 j = 0; j < ng; j++)
            if (is_id(tr->giant_index[j]) == (pass == 1)) {
                rows.push_back(j);
                if (pass == 0) {
                    gidx.push_back(tr->giant_index[j]);
                    gkb.push_back(tr->giant_key_b[j]);
                    gka.push_back(tr->giant_key_a[j]);
                }
            }
    const u32 nrot = (u32)gidx.size(), nid = ng - nrot;

    // 1-2. R_i, both elements, over Ql|P: [nbaby][batch][l+P][N] each
    Scratch rb, dg;
    RCCHK(rb.alloc((size_t)2 * nb * per * 8, s, k->ctx));
    u64* r0 = rb.w();
    u64* r1 = r0 + (u64)nb * per;
    bool any_rot = false;
    for (u32 i = 0; i < nb; i++) any_rot |= !is_id(tr->baby_index[i]);
    if (any_rot) {
        RCCHK(dg.alloc((size_t)L->beta * per * 8, s, k->ctx));
        RCCHK(ks_precompute_impl(k, L, l, c1, dg.w(), batch, s, true));
    }
    for (u32 i = 0; i < nb;) {
        if (is_id(tr->baby_index[i])) {  // KeySwitchExt(ct, true), ckksrns-fhe.cpp:1521
            RCCHK(ks_ext_impl(k, L, c0, r0 + i * per, batch, s));
            RCCHK(ks_ext_impl(k, L, c1, r1 + i * per, batch, s));
            i++;
            continue;
        }
        u32 n = 0, kinv[KS_ROT_CAP];  // a run of rotations: EvalFastRotationExt(ct, ., digits, true), 1513-1515
        for (; i + n < nb && n < KS_ROT_CAP && !is_id(tr->baby_index[i + n]); n++)
            kinv[n] = inv_odd32(tr->baby_index[i + n]);
        RCCHK(ks_inner_rot(k, L, l, dg.w(), c0, n, kinv, tr->baby_key_b + i, tr->baby_key_a + i, r0 + i * per,
                           r1 + i * per, per, batch, s));
        i += n;
    }

    // 3. I_j: element 0 then element 1 of the rotated giants (one ModDown batch),
    // the identity giants' second elements, and their first elements behind the
    // two outer sums, whose ModDown they share (step 7)
    Scratch ib, ou;
    RCCHK(ib.alloc((size_t)(2 * nrot + nid) * per * 8, s, k->ctx));
    RCCHK(ou.alloc((size_t)(2 + nid) * per * 8, s, k->ctx));
    u64* i0r = ib.w();
    u64* i1r = i0r + (u64)nrot * per;
    u64* i1d = i1r + (u64)nrot * per;
    u64* i0d = ou.w() + 2 * per;
    if (nrot)
        RCCHK(lt_inner_run(k, L, nb, r0, r1, per, tr->diag, tr->diag_stride, tr->present, rows.data(), nrot, i0r,
                           i1r, batch, s));
    if (nid)
        RCCHK(lt_inner_run(k, L, nb, r0, r1, per, tr->diag, tr->diag_stride, tr->present, rows.data() + nrot, nid,
                           i0d, i1d, batch, s));

    // 4. KeySwitchDown of every rotated giant's sum, both elements, as one batch (1536)
    Scratch md, dg2;
    RCCHK(md.alloc((size_t)(2 * nrot + nid) * qper * 8, s, k->ctx));
    u64* md0 = md.w();
    u64* md1 = md0 + (u64)nrot * qper;
    u64* mdid = md1 + (u64)nrot * qper;
    if (nrot) {
        u64* const outs[2] = {md0, md1};
        RCCHK(mod_down_run(A, i0r, poly, outs, 2, qw, nrot * batch, s));
    }

    // 5-6. the rotated giants' second elements decomposed as one batch (1544),
    // key-switched, rotated and summed (1545); outer1 follows outer0
    if (nrot) {
        RCCHK(dg2.alloc((size_t)nrot * L->beta * per * 8, s, k->ctx));
        RCCHK(ks_precompute_impl(k, L, l, md1, dg2.w(), nrot * batch, s, true));
    }
    RCCHK(lt_outer_run(k, L, nrot ? dg2.w() : nullptr, nrot, gidx.data(), gkb.data(), gka.data(), nid ? i1d : nullptr,
                       nid, ou.w(), ou.w() + per, batch, s));

    // 7-8. the last KeySwitchDown (1549) together with KeySwitchDownFirstElement
    // of the identity giants (1529), whose result is not needed earlier: one set
    // of launches over 2 + nid polynomials per entry; then += first (1551)
    std::vector<u64*> outs{out0, out1};
    for (u32 j = 0; j < nid; j++) outs.push_back(mdid + (u64)j * qper);
    RCCHK(mod_down_run(A, ou.w(), poly, outs.data(), 2 + nid, qw, batch, s));
    dim3 g;
    RCCHK(coeff_grid(qper, &g));
    return rot_chunks(nrot, true, [&](u32 j0, u32 ns) {
        LtIdx I{};
        for (u32 j = 0; j < ns; j++) I.k[j] = gidx[j0 + j];
        hipLaunchKernelGGL(k_lt_first, g, dim3(256), 0, s, L->d_tow, out0, md0 + (u64)j0 * qper, I, ns, mdid,
                           j0 ? 0u : nid, out0, qper, k->log_n, l);
        return post_launch();
    });
}

// ---------------------------------------------------------------------------
// Element maps
// ---------------------------------------------------------------------------
int ofhe_hip_switch_modulus(ofhe_ctx_t ctx, const uint64_t* src, uint64_t* dst, uint64_t n, uint64_t old_q,
                            uint64_t new_q, void* stream) {
    if (!ctx || ((!src || !dst) && n)) return fail(OFHE_ERR_ARG, "NULL argument");
    if (old_q < 2 || new_q < 2) return fail(OFHE_ERR_ARG, "moduli must be >= 2");
    if (!n) return OFHE_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_switch_modulus, dim3(grid_for(n)), dim3(256), 0, pick(stream), src, dst, (u64)n, (u64)old_q,
                       (u64)new_q);
    return post_launch();
}

int ofhe_hip_automorphism(ofhe_plan_t p, uint32_t k, int eval_form, const uint64_t* src, uint64_t* dst,
                          uint32_t batch, void* stream) {
    if (!p || !p->ctx) return fail(OFHE_ERR_STATE, "plan is NULL or destroyed");
    if (!src || !dst || batch == 0) return fail(OFHE_ERR_ARG, "bad data argument");
    if (src == dst) return fail(OFHE_ERR_ARG, "automorphism is out of place (dst must not alias src)");
    if (k % 2 == 0) return fail(OFHE_ERR_ARG, "Automorphism index not odd");  // poly-impl.h:333-334
    HIPCHK(hipSetDevice(p->ctx->device));
    const u64 total = (u64)batch * p->towers << p->log_n;
    with_bool(eval_form != 0, [&](auto ev) {
        hipLaunchKernelGGL(k_automorphism<decltype(ev)::value>, dim3(grid_for(total)), dim3(256), 0, pick(stream),
                           p->d_tc, src, dst, k, total, p->log_n, p->towers);
    });
    return post_launch();
}

// ---------------------------------------------------------------------------
// Rescaling on the device: DCRTPolyImpl::DropLastElementAndScale (CKKS / BFV,
// dcrtpoly-impl.h:746-768) and DCRTPolyImpl::ModReduce (BGV, 792-812), the
// callers that take the path's INTT -> SwitchModulus -> NTT steps one tower
// down.  Evaluation form runs INTT(last tower) -> k_switch_scale<SW_SCALE> ->
// the fused forward-subtract block pass, using
//   x a + NTT(sw c) = (x - NTT(sw (-c a^-1))) a      (rescale, a = qlInvModq_i)
//   (x + NTT(sw t)) a = (x - NTT(sw (-t))) a           (mod-reduce)
// with the canonical residues of the reference's own order of operations.
// ---------------------------------------------------------------------------
// a scalar table of the plan, keyed by its own content
static int plan_table(ofhe_plan_t p, const std::vector<u64>& words, const u64** out) {
    return cached_table(p->tab_mu, p->tabs, words, "rescale tables", out,
                        [&]() -> const std::vector<u64>& { return words; });
}

// The rescaling tables of L towers q[0..L), the one place that knows their
// layout and algebra.  A row of sw (SwArgs::tab) is six words
// [q, w, w', a, a', 0], of which the device reads w as tab[6 t + 1]; a row of sc
// is the TowerScalar [q, a, a'] of the forward-subtract pass, which only
// evaluation form runs.  w multiplies the lifted last tower:
//   SW_AXPY (rescale)     coefficient form c,  evaluation form -(c a^-1)
//   SW_XPYA (mod-reduce)  coefficient form t,  evaluation form -t
//   SW_SCALE              1: the bare lift (CRTDecompose), with neither a nor sc
// and a, a' stand in sw where k_switch_scale itself multiplies by a (coefficient
// form) and in every mod-reduce row.  c and a are per tower, reduced here; a[i]
// must be invertible mod q[i] for SW_AXPY in evaluation form.
enum { SWR_Q = 0, SWR_W = 1, SWR_A = 3, SWR_WORDS = 6 };
static RsTab rs_build(const u64* q, u32 L, int mode, bool eval, const u64* c, const u64* a, u64 t, u64 pre = 1) {
    RsTab T;
    T.mode = mode;
    T.pre = pre;
    T.sw.assign(SWR_WORDS * (size_t)L, 0);
    for (u32 i = 0; i < L; i++) {
        const u64 qi = q[i];
        u64* row = &T.sw[SWR_WORDS * (size_t)i];
        u64 w = 1;
        if (mode == SW_AXPY) w = eval ? qi - mulmod(c[i] % qi, invmod(a[i] % qi, qi), qi) : c[i];
        if (mode == SW_XPYA) w = eval ? qi - t % qi : t;
        const TowerScalar W = scalar_of(qi, w);
        row[SWR_Q] = qi, row[SWR_W] = W.s, row[SWR_W + 1] = W.sp;
        if (mode == SW_SCALE) continue;
        const TowerScalar S = scalar_of(qi, a[i]);
        if (mode == SW_XPYA || !eval) row[SWR_A] = S.s, row[SWR_A + 1] = S.sp;
        if (eval) T.sc.insert(T.sc.end(), {S.q, S.s, S.sp});
    }
    return T;
}

static int rescale_check(ofhe_plan_t p, u32 towers, const u64* x, u64 xs, const u64* out, u64 os, u32 batch) {
    if (!p || !p->ctx) return fail(OFHE_ERR_STATE, "plan is NULL or destroyed");
    if (!x || !out || batch == 0) return fail(OFHE_ERR_ARG, "bad data argument");
    // dcrtpoly-impl.h:720-723 (DropLastElement)
    if (towers < 2) return fail(OFHE_ERR_ARG, "Removing last element of DCRTPoly object renders it invalid!");
    if (towers > p->towers) return fail(OFHE_ERR_ARG, "towers exceeds the plan");
    const u64 N = 1ull << p->log_n;
    if (xs < towers * N || os < (towers - 1) * N) return fail(OFHE_ERR_ARG, "batch stride smaller than the towers");
    if (((xs | os) & 1) || (((uintptr_t)x | (uintptr_t)out) & 15))
        return fail(OFHE_ERR_ARG, "strides must be even and buffers 16-byte aligned");
    // In place only with equal strides: every launch then reads and writes a
    // word at the same address from the same thread.  With a packed output
    // (out_stride = (towers-1)N < x_stride) entry b's output would overwrite
    // towers of entry b-1's input that other workgroups still read.
    const u64 xw = (u64)(batch - 1) * xs + (u64)towers * N, ow = (u64)(batch - 1) * os + (u64)(towers - 1) * N;
    if (words_overlap(x, xw, out, ow) && !(x == out && xs == os))
        return fail(OFHE_ERR_ARG, "out overlaps x: in place needs out == x and out_stride == x_stride");
    return OFHE_OK;
}

// shared tail, on the tables T of rs_build.  nelem elements x[e] -> out[e] of `batch`
// entries each (evaluation form when nelem > 1): the last towers' INTT (one
// launch when the elements follow one another), the lift and the column pass
// run over nelem * batch polynomials, the pass that writes out[e] per element.
static int rescale_run(ofhe_plan_t p, u32 towers, const u64* const* xv, u64 xs, u64* const* outv, u64 os, u32 nelem,
                       bool eval, const RsTab& T, u32 batch, hipStream_t s) {
    HIPCHK(hipSetDevice(p->ctx->device));
    const u64* x = xv[0];
    u64* out = outv[0];
    const u32 bn = nelem * batch;
    const u32 L = towers - 1, log_n = p->log_n;
    const u64 N = 1ull << log_n;
    const u64 *dsw = nullptr, *dsc = nullptr;
    RCCHK(plan_table(p, T.sw, &dsw));
    if (eval) RCCHK(plan_table(p, T.sc, &dsc));
    const u64 ql = p->q[L];
    SwArgs A{};
    A.tab = dsw;
    A.ql = ql;
    A.pre = T.pre % ql;
    A.pre_p = shoup_pre(A.pre, ql);
    if (A.pre == 1) A.pre_p = 0;
    A.log_n = log_n;
    A.towers = L;
    const u32 bpr = (u32)((N / 2 + 255) / 256);  // two coefficients per thread
    dim3 g;
    RCCHK(coeff_grid((u64)bpr * bn * L * 256, &g, "batch too large for one launch"));
    if (!eval) {
        A.last = x + (u64)L * N;
        A.lstride = xs;
        A.x = x;
        A.xstride = xs;
        A.y = out;
        A.ystride = os;
        with_int<SW_AXPY, SW_XPYA>(T.mode, [&](auto m) {
            hipLaunchKernelGGL(k_switch_scale<decltype(m)::value>, g, dim3(256), 0, s, A, bpr);
        });
        RCCHK(post_launch());
        // DropLastElementAndScale switches the coefficient-form towers to
        // evaluation form (dcrtpoly-impl.h:765-766); ModReduce does not
        if (T.mode == SW_AXPY) return plan_ntt_range(p, false, 0, L, out, out, os, os, batch, s);
        return OFHE_OK;
    }
    Scratch sl, sy;
    RCCHK(sl.alloc((size_t)bn * N * 8, s, p->ctx));
    RCCHK(sy.alloc((size_t)bn * L * N * 8, s, p->ctx));
    bool dense = true;  // element e + 1 follows element e
    for (u32 e = 1; e < nelem; e++) dense = dense && xv[e] == x + (u64)e * batch * xs;
    if (dense)
        RCCHK(plan_ntt_range(p, true, L, 1, x + (u64)L * N, sl.w(), xs, N, bn, s));
    else
        for (u32 e = 0; e < nelem; e++)
            RCCHK(plan_ntt_range(p, true, L, 1, xv[e] + (u64)L * N, sl.w() + (u64)e * batch * N, xs, N, batch, s));
    const u64 ys = (u64)L * N;
    // the per-element tail: the forward-subtract block pass (log_n >= 12), or k_sub_scale
    auto tail = [&](bool block) {
        for (u32 e = 0; e < nelem; e++) {
            u64* ye = sy.w() + (u64)e * batch * ys;
            if (block)
                RCCHK(plan_ntt_fwd_sub(p, 0, L, ye, ys, xv[e], xs, outv[e], os, dsc, batch, s, 2));
            else
                RCCHK(sub_scale(reinterpret_cast<const TowerScalar*>(dsc), xv[e], ye, outv[e], xs, ys, os, batch, L,
                                log_n, s));
        }
        return (int)OFHE_OK;
    };
    if (log_n > 12 && p->split != SPLIT_T9) {
        // the lift happens in the column pass's loads (k_cols<.., SWS>): the
        // switched towers are never written to HBM before their transform
        RCCHK(plan_cols_switch(p, 0, L, sl.w(), N, ql, A.pre, dsw, sy.w(), ys, bn, s));
        return tail(true);
    }
    A.last = sl.w();
    A.lstride = N;
    A.y = sy.w();
    A.ystride = ys;
    hipLaunchKernelGGL(k_switch_scale<SW_SCALE>, g, dim3(256), 0, s, A, bpr);
    RCCHK(post_launch());
    if (log_n >= 12) {
        RCCHK(plan_ntt_fwd_sub(p, 0, L, sy.w(), ys, x, xs, out, os, dsc, bn, s, 1));  // the column pass (log_n > 12)
        return tail(true);
    }
    RCCHK(plan_ntt_range(p, false, 0, L, sy.w(), sy.w(), ys, ys, bn, s));
    return tail(false);
}

int ofhe_hip_drop_last_and_scale(ofhe_plan_t p, uint32_t towers, const uint64_t* x, uint64_t x_stride,
                                 uint64_t* out, uint64_t out_stride, int eval_form,
                                 const uint64_t* ql_ql_inv_modql_divql_modq, const uint64_t* ql_inv_modq,
                                 uint32_t batch, void* stream) {
    RCCHK(rescale_check(p, towers, x, x_stride, out, out_stride, batch));
    if (!ql_ql_inv_modql_divql_modq || !ql_inv_modq) return fail(OFHE_ERR_ARG, "NULL constants");
    const u32 L = towers - 1;
    for (u32 i = 0; eval_form && i < L; i++)
        if (ql_inv_modq[i] % p->q[i] == 0)
            return fail(OFHE_ERR_ARG, "ql_inv_modq[" + std::to_string(i) + "] is not invertible mod q_i");
    const RsTab T = rs_build(p->q.data(), L, SW_AXPY, eval_form != 0, ql_ql_inv_modql_divql_modq, ql_inv_modq, 0);
    return rescale_run(p, towers, &x, x_stride, &out, out_stride, 1, eval_form != 0, T, batch, pick(stream));
}

int ofhe_hip_mod_reduce(ofhe_plan_t p, uint32_t towers, const uint64_t* x, uint64_t x_stride, uint64_t* out,
                        uint64_t out_stride, int eval_form, uint64_t t, uint64_t neg_t_inv_modq,
                        const uint64_t* ql_inv_modq, uint32_t batch, void* stream) {
    RCCHK(rescale_check(p, towers, x, x_stride, out, out_stride, batch));
    if (!ql_inv_modq) return fail(OFHE_ERR_ARG, "NULL constants");
    const RsTab T = rs_build(p->q.data(), towers - 1, SW_XPYA, eval_form != 0, nullptr, ql_inv_modq, t, neg_t_inv_modq);
    return rescale_run(p, towers, &x, x_stride, &out, out_stride, 1, eval_form != 0, T, batch, pick(stream));
}

// ---------------------------------------------------------------------------
// BV key switching with digitSize = 0 (KeySwitchBV, keyswitch-bv.cpp:302-340):
// digit i of c is CRTDecompose(0)'s tower-i polynomial (dcrtpoly-impl.h:
// 266-288): c_i in coefficient form lifted into every tower (SwitchModulus)
// and transformed -- the fused lift + forward NTT of the rescaling path, one
// launch pair per digit -- then the key inner product (k_bv_inner).
// ---------------------------------------------------------------------------
int ofhe_hip_bv_precompute(ofhe_plan_t p, uint32_t towers, const uint64_t* c, uint64_t* digits, uint32_t batch,
                           void* stream) {
    if (!p || !p->ctx) return fail(OFHE_ERR_STATE, "plan is NULL or destroyed");
    if (!c || !digits || batch == 0) return fail(OFHE_ERR_ARG, "bad data argument");
    if (towers < 1 || towers > p->towers) return fail(OFHE_ERR_ARG, "towers must be in [1, plan towers]");
    if ((((uintptr_t)c | (uintptr_t)digits) & 15)) return fail(OFHE_ERR_ARG, "buffers must be 16-byte aligned");
    HIPCHK(hipSetDevice(p->ctx->device));
    hipStream_t s = pick(stream);
    const u32 T = towers, log_n = p->log_n;
    const u64 N = 1ull << log_n, TN = (u64)T * N;
    const u64* dsw = nullptr;
    RCCHK(plan_table(p, rs_build(p->q.data(), T, SW_SCALE, true, nullptr, nullptr, 0).sw, &dsw));
    Scratch sc;  // c in coefficient form
    RCCHK(sc.alloc((size_t)batch * TN * 8, s, p->ctx));
    RCCHK(plan_ntt_range(p, true, 0, T, c, sc.w(), TN, TN, batch, s));
    const u64 dstride = (u64)T * TN;  // words per batch entry of digits
    const bool fused = log_n > 12 && p->split != SPLIT_T9;
    const u32 bpr = (u32)((N / 2 + 255) / 256);
    dim3 g;
    RCCHK(coeff_grid((u64)bpr * batch * T * 256, &g, "batch too large for one launch"));
    for (u32 i = 0; i < T; i++) {
        u64* di = digits + (u64)i * TN;
        if (fused) {
            RCCHK(plan_cols_switch(p, 0, T, sc.w() + (u64)i * N, TN, p->q[i], 1, dsw, di, dstride, batch, s));
            RCCHK(plan_ntt_fwd_block(p, 0, T, di, dstride, batch, s));
            continue;
        }
        SwArgs A{};
        A.last = sc.w() + (u64)i * N;
        A.lstride = TN;
        A.y = di;
        A.ystride = dstride;
        A.tab = dsw;
        A.ql = p->q[i];
        A.pre = 1;
        A.log_n = log_n;
        A.towers = T;
        hipLaunchKernelGGL(k_switch_scale<SW_SCALE>, g, dim3(256), 0, s, A, bpr);
        RCCHK(post_launch());
        RCCHK(plan_ntt_range(p, false, 0, T, di, di, dstride, dstride, batch, s));
    }
    return OFHE_OK;
}

int ofhe_hip_bv_core(ofhe_plan_t p, uint32_t towers, const uint64_t* digits, const uint64_t* key_b,
                     const uint64_t* key_a, uint32_t key_towers, uint64_t* out0, uint64_t* out1, uint32_t batch,
                     void* stream) {
    if (!p || !p->ctx) return fail(OFHE_ERR_STATE, "plan is NULL or destroyed");
    if (!digits || !key_b || !key_a || !out0 || !out1 || batch == 0) return fail(OFHE_ERR_ARG, "bad data argument");
    if (towers < 1 || towers > p->towers) return fail(OFHE_ERR_ARG, "towers must be in [1, plan towers]");
    if (key_towers < towers) return fail(OFHE_ERR_ARG, "key_towers smaller than towers");
    if (towers > 256) return fail(OFHE_ERR_ARG, "at most 256 digits (128-bit accumulation)");
    HIPCHK(hipSetDevice(p->ctx->device));
    std::vector<u64> mu(3 * (size_t)towers);
    for (u32 t = 0; t < towers; t++) {
        mu[3 * t] = p->q[t];
        barrett128(p->q[t], &mu[3 * t + 1]);
    }
    const u64* dmu = nullptr;
    RCCHK(plan_table(p, mu, &dmu));
    BvArgs A{digits, key_b, key_a, out0, out1, dmu, towers, towers, key_towers, p->log_n};
    const u64 N = 1ull << p->log_n;
    const u32 bpr = (u32)((N + 255) / 256);
    dim3 g;
    RCCHK(coeff_grid((u64)bpr * batch * towers * 256, &g, "batch too large for one launch"));
    hipLaunchKernelGGL(k_bv_inner, g, dim3(256), 0, pick(stream), A, bpr);
    return post_launch();
}

// ---------------------------------------------------------------------------
// BV key switching with a digit size r (CRTDecompose(r), dcrtpoly-impl.h:
// 266-320): tower i of c in coefficient form is cut into w_i = ceil(bitlen(q_i)
// / r) windows of r bits (k_bv_windows), digit arrWindows[i] + j is window j of
// tower i lifted into every tower (SwitchModulus q_i -> q_k: a window can
// exceed q_i / 2 or q_k) and transformed -- the lift + forward NTT of
// ofhe_hip_bv_precompute, fed by window rows instead of tower rows.  r = 0, and
// any tower with a single window (that window is the tower), is lifted from
// the coefficient rows directly, so r = 0 gives ofhe_hip_bv_precompute's words.
// ---------------------------------------------------------------------------
static u32 bv_windows(u64 q, u32 r) { return r ? (msb64(q) + r - 1) / r : 1; }  // GetLengthForBase(2) = bit length
static u32 bv_digits(const u64* q, u32 towers, u32 r) {
    u32 n = 0;
    for (u32 i = 0; i < towers; i++) n += bv_windows(q[i], r);
    return n;
}

// Scratch bound of ofhe_hip_bv_key_switch with chunk_digits = 0: the chunk is the
// largest number of digits whose [batch][chunk][towers][N] words fit in it (at
// least one digit, at most all).  1 GiB: every chunk re-reads and re-writes the
// two outputs, and at N = 2^16, 16 towers, batch 4 chunks of 8 digits (256 MiB)
// measured 7 % behind the whole array, chunks of 32 within 2 %.
constexpr u64 BV_CHUNK_SCRATCH_BYTES = 1ull << 30;

// Key-stationary batch entries per thread of the inner product (ofhe_hip_bv_tune):
// 0 picks by batch size (bv_inner_nb), 1 is the plain loop.
static std::atomic<u32> g_bv_nb{0};
// The measured choice (tools/bv_digits_ab.py, DESIGN.md "BV key switching with a
// digit size"): the key-stationary kernel wins once the batch gives it several
// entries per thread and the launch still has BV_KS_MIN_THREADS threads; below
// that the grid is too small to keep the memory system busy and the plain loop
// (one thread per output word) is as fast or faster.
constexpr u64 BV_KS_MIN_THREADS = 1ull << 19;
static u32 bv_inner_nb(u32 batch, u32 towers, u32 log_n) {
    const u32 forced = g_bv_nb.load(std::memory_order_relaxed);
    if (forced) return forced;
    for (u32 nb : {4u, 2u})
        if (batch >= nb && ((u64)((batch + nb - 1) / nb) * towers << log_n) >= BV_KS_MIN_THREADS) return nb;
    return 1;
}

int ofhe_hip_bv_tune(uint32_t key_stationary) {
    if (key_stationary != 0 && key_stationary != 1 && key_stationary != 2 && key_stationary != 4)
        return fail(OFHE_ERR_ARG, "key_stationary must be 0 (auto), 1 (plain), 2 or 4");
    g_bv_nb.store(key_stationary, std::memory_order_relaxed);
    return OFHE_OK;
}

// the lift of `nb` rows (last + b * lstride, modulus ql) into the T towers of y + b * ystride, transformed
static int bv_lift(ofhe_plan_t p, u32 T, const u64* dsw, const u64* last, u64 lstride, u64 ql, u64* y, u64 ystride,
                   u32 nb, hipStream_t s) {
    const u32 log_n = p->log_n;
    if (log_n > 12 && p->split != SPLIT_T9) {
        RCCHK(plan_cols_switch(p, 0, T, last, lstride, ql, 1, dsw, y, ystride, nb, s));
        return plan_ntt_fwd_block(p, 0, T, y, ystride, nb, s);
    }
    const u64 N = 1ull << log_n;
    const u32 bpr = (u32)((N / 2 + 255) / 256);
    dim3 g;
    RCCHK(coeff_grid((u64)bpr * nb * T * 256, &g, "batch too large for one launch"));
    SwArgs A{};
    A.last = last;
    A.lstride = lstride;
    A.y = y;
    A.ystride = ystride;
    A.tab = dsw;
    A.ql = ql;
    A.pre = 1;
    A.log_n = log_n;
    A.towers = T;
    hipLaunchKernelGGL(k_switch_scale<SW_SCALE>, g, dim3(256), 0, s, A, bpr);
    RCCHK(post_launch());
    return plan_ntt_range(p, false, 0, T, y, y, ystride, ystride, nb, s);
}

// Digits [d0, d1) of CRTDecompose(r) of sc (c in coefficient form, [batch][T][N])
// into dig [batch][d1 - d0][T][N].  The windows of one source tower are lifted
// together: one launch pair with the windows as the batch (batch = 1), else
// one per batch entry or one per window, whichever is fewer.
static int bv_decompose_range(ofhe_plan_t p, u32 T, u32 r, const u64* sc, u32 d0, u32 d1, u64* dig, u32 batch,
                              hipStream_t s) {
    const u32 log_n = p->log_n, nc = d1 - d0;
    const u64 N = 1ull << log_n, TN = (u64)T * N;
    const u64* dsw = nullptr;
    RCCHK(plan_table(p, rs_build(p->q.data(), T, SW_SCALE, true, nullptr, nullptr, 0).sw, &dsw));
    u32 maxw = 0;  // the most windows any tower contributes to the range
    for (u32 i = 0, a = 0; i < T; a += bv_windows(p->q[i], r), i++) {
        const u32 w = bv_windows(p->q[i], r), lo = std::max(a, d0), hi = std::min(a + w, d1);
        if (w > 1 && lo < hi) maxw = std::max(maxw, hi - lo);
    }
    Scratch sw;  // [batch][nw][N] window rows of one tower at a time
    if (maxw) RCCHK(sw.alloc((size_t)batch * maxw * N * 8, s, p->ctx));
    const u32 bpr = (u32)((N / 2 + 255) / 256);
    for (u32 i = 0, a = 0; i < T; a += bv_windows(p->q[i], r), i++) {
        const u32 w = bv_windows(p->q[i], r), lo = std::max(a, d0), hi = std::min(a + w, d1);
        if (lo >= hi) continue;
        const u32 nw = hi - lo, e0 = lo - d0;
        const u64 qi = p->q[i];
        if (w == 1) {
            RCCHK(bv_lift(p, T, dsw, sc + (u64)i * N, TN, qi, dig + (u64)e0 * TN, (u64)nc * TN, batch, s));
            continue;
        }
        BvWinArgs W{sc + (u64)i * N, TN, sw.w(), r, lo - a, nw, log_n};
        dim3 g;
        RCCHK(coeff_grid((u64)bpr * batch * 256, &g, "batch too large for one launch"));
        hipLaunchKernelGGL(k_bv_windows, g, dim3(256), 0, s, W, bpr);
        RCCHK(post_launch());
        if (batch <= nw) {
            for (u32 b = 0; b < batch; b++)
                RCCHK(bv_lift(p, T, dsw, sw.w() + (u64)b * nw * N, N, qi, dig + ((u64)b * nc + e0) * TN, TN, nw, s));
        } else {
            for (u32 j = 0; j < nw; j++)
                RCCHK(bv_lift(p, T, dsw, sw.w() + (u64)j * N, (u64)nw * N, qi, dig + (u64)(e0 + j) * TN, (u64)nc * TN,
                              batch, s));
        }
    }
    return OFHE_OK;
}

// out = acc + sum_{d < nd} key[k0 + d] . digit_d (k_bv_inner_digits); acc NULL: zero
static int bv_inner_run(ofhe_plan_t p, u32 T, u32 nd, const u64* digits, const u64* kb, const u64* ka, u32 key_towers,
                        const u64* acc0, const u64* acc1, u64* out0, u64* out1, u32 batch, hipStream_t s) {
    std::vector<u64> mu(3 * (size_t)T);
    for (u32 t = 0; t < T; t++) {
        mu[3 * t] = p->q[t];
        barrett128(p->q[t], &mu[3 * t + 1]);
    }
    const u64* dmu = nullptr;
    RCCHK(plan_table(p, mu, &dmu));
    BvDigitArgs D{BvArgs{digits, kb, ka, out0, out1, dmu, nd, T, key_towers, p->log_n}, acc0, acc1, batch};
    const u64 N = 1ull << p->log_n;
    const u32 bpr = (u32)((N + 255) / 256);
    const u32 nb = bv_inner_nb(batch, T, p->log_n);
    dim3 g;
    RCCHK(coeff_grid((u64)bpr * ((batch + nb - 1) / nb) * T * 256, &g, "batch too large for one launch"));
    with_int<1, 2, 4>((int)nb, [&](auto n) {
        hipLaunchKernelGGL(k_bv_inner_digits<decltype(n)::value>, g, dim3(256), 0, s, D, bpr);
    });
    return post_launch();
}

static bool bv_aligned(std::initializer_list<const void*> ps) {
    for (const void* x : ps)
        if ((uintptr_t)x & 15) return false;
    return true;
}
static int bv_plan_check(ofhe_plan_t p, u32 towers) {
    if (!p || !p->ctx) return fail(OFHE_ERR_STATE, "plan is NULL or destroyed");
    if (towers < 1 || towers > p->towers) return fail(OFHE_ERR_ARG, "towers must be in [1, plan towers]");
    return OFHE_OK;
}
static const char* const BV_DIGIT_SIZE_MSG = "digit_size must be at most 30 (the reference forms 1 << digitSize in an int)";

int ofhe_hip_bv_digit_count(ofhe_plan_t p, uint32_t towers, uint32_t digit_size, uint32_t* count) {
    if (digit_size > 30) return fail(OFHE_ERR_ARG, BV_DIGIT_SIZE_MSG);
    if (!count) return fail(OFHE_ERR_ARG, "count is NULL");
    RCCHK(bv_plan_check(p, towers));
    *count = bv_digits(p->q.data(), towers, digit_size);
    return OFHE_OK;
}

int ofhe_hip_bv_precompute_digits(ofhe_plan_t p, uint32_t towers, uint32_t digit_size, const uint64_t* c,
                                  uint64_t* digits, uint32_t batch, void* stream) {
    if (!c || !digits || batch == 0) return fail(OFHE_ERR_ARG, "bad data argument");
    if (!bv_aligned({c, digits})) return fail(OFHE_ERR_ARG, "buffers must be 16-byte aligned");
    if (digit_size > 30) return fail(OFHE_ERR_ARG, BV_DIGIT_SIZE_MSG);
    RCCHK(bv_plan_check(p, towers));
    HIPCHK(hipSetDevice(p->ctx->device));
    hipStream_t s = pick(stream);
    const u64 TN = (u64)towers << p->log_n;
    Scratch sc;  // c in coefficient form
    RCCHK(sc.alloc((size_t)batch * TN * 8, s, p->ctx));
    RCCHK(plan_ntt_range(p, true, 0, towers, c, sc.w(), TN, TN, batch, s));
    return bv_decompose_range(p, towers, digit_size, sc.w(), 0, bv_digits(p->q.data(), towers, digit_size), digits,
                              batch, s);
}

int ofhe_hip_bv_core_digits(ofhe_plan_t p, uint32_t towers, uint32_t n_digits, const uint64_t* digits,
                            const uint64_t* key_b, const uint64_t* key_a, uint32_t key_towers, uint64_t* out0,
                            uint64_t* out1, uint32_t batch, void* stream) {
    if (!digits || !key_b || !key_a || !out0 || !out1 || batch == 0) return fail(OFHE_ERR_ARG, "bad data argument");
    if (!bv_aligned({digits, key_b, key_a, out0, out1})) return fail(OFHE_ERR_ARG, "buffers must be 16-byte aligned");
    if (n_digits == 0) return fail(OFHE_ERR_ARG, "n_digits must be >= 1");
    if (key_towers < towers) return fail(OFHE_ERR_ARG, "key_towers smaller than towers");
    if (digits == out0 || digits == out1 || out0 == out1)
        return fail(OFHE_ERR_ARG, "digits, out0 and out1 must be distinct buffers");
    RCCHK(bv_plan_check(p, towers));
    // the finest decomposition (digit_size = 1) bounds every digit count
    if (n_digits > bv_digits(p->q.data(), towers, 1))
        return fail(OFHE_ERR_ARG, "n_digits exceeds the digit count of these towers at digit_size = 1");
    const u64 w = (u64)batch * towers << p->log_n;
    RCCHK(outputs_apart(out0, out1, w));
    if (words_overlap(digits, w * n_digits, out0, w) || words_overlap(digits, w * n_digits, out1, w))
        return fail(OFHE_ERR_ARG, "digits overlaps an output");
    HIPCHK(hipSetDevice(p->ctx->device));
    return bv_inner_run(p, towers, n_digits, digits, key_b, key_a, key_towers, nullptr, nullptr, out0, out1, batch,
                        pick(stream));
}

// KeySwitchInPlace (keyswitch-bv.cpp:283-300) in one call: out0 = add0 + ct0,
// out1 = add1 + ct1, the decomposition and the inner product run chunk by chunk
// over a digit scratch of `chunk` digits; every chunk after the first adds into
// the outputs (the accumulate mode of k_bv_inner_digits).
int ofhe_hip_bv_key_switch(ofhe_plan_t p, uint32_t towers, uint32_t digit_size, const uint64_t* c,
                           const uint64_t* key_b, const uint64_t* key_a, uint32_t key_towers, const uint64_t* add0,
                           const uint64_t* add1, uint64_t* out0, uint64_t* out1, uint32_t chunk_digits, uint32_t batch,
                           void* stream) {
    if (!c || !key_b || !key_a || !out0 || !out1 || batch == 0) return fail(OFHE_ERR_ARG, "bad data argument");
    if (!bv_aligned({c, key_b, key_a, add0, add1, out0, out1}))
        return fail(OFHE_ERR_ARG, "buffers must be 16-byte aligned");
    if (digit_size > 30) return fail(OFHE_ERR_ARG, BV_DIGIT_SIZE_MSG);
    if (key_towers < towers) return fail(OFHE_ERR_ARG, "key_towers smaller than towers");
    if (out0 == out1) return fail(OFHE_ERR_ARG, "out0 and out1 must be distinct buffers");
    RCCHK(bv_plan_check(p, towers));
    const u32 log_n = p->log_n, nd = bv_digits(p->q.data(), towers, digit_size);
    const u64 TN = (u64)towers << log_n, w = (u64)batch * TN, kw = (u64)nd * key_towers << log_n;
    RCCHK(outputs_apart(out0, out1, w));
    u64* const outs[2] = {out0, out1};
    for (u64* o : outs) {
        // c is consumed (its INTT) before anything is written: an output may be c itself
        if (o != c && words_overlap(o, w, c, w)) return fail(OFHE_ERR_ARG, "an output overlaps c without starting at its address");
        if (words_overlap(o, w, key_b, kw) || words_overlap(o, w, key_a, kw))
            return fail(OFHE_ERR_ARG, "outputs must not alias the keys");
    }
    // an addend is read by the thread that writes the same word of its output, in the first chunk only
    if ((add0 && add0 != out0 && words_overlap(add0, w, out0, w)) || (add1 && add1 != out1 && words_overlap(add1, w, out1, w)) ||
        (add0 && words_overlap(add0, w, out1, w)) || (add1 && words_overlap(add1, w, out0, w)))
        return fail(OFHE_ERR_ARG, "an addend may alias only its own output (add0 == out0, add1 == out1)");
    HIPCHK(hipSetDevice(p->ctx->device));
    hipStream_t s = pick(stream);
    u32 chunk = chunk_digits;
    if (chunk == 0) chunk = (u32)std::max<u64>(1, BV_CHUNK_SCRATCH_BYTES / (w * 8));
    chunk = std::min(chunk, nd);
    Scratch sc, sd;  // c in coefficient form; one chunk of digits
    RCCHK(sc.alloc((size_t)w * 8, s, p->ctx));
    RCCHK(sd.alloc((size_t)w * chunk * 8, s, p->ctx));
    RCCHK(plan_ntt_range(p, true, 0, towers, c, sc.w(), TN, TN, batch, s));
    const u64 kstep = (u64)key_towers << log_n;
    for (u32 d0 = 0; d0 < nd; d0 += chunk) {
        const u32 d1 = std::min(nd, d0 + chunk);
        RCCHK(bv_decompose_range(p, towers, digit_size, sc.w(), d0, d1, sd.w(), batch, s));
        RCCHK(bv_inner_run(p, towers, d1 - d0, sd.w(), key_b + d0 * kstep, key_a + d0 * kstep, key_towers,
                           d0 ? out0 : add0, d0 ? out1 : add1, out0, out1, batch, s));
    }
    return OFHE_OK;
}

// ---------------------------------------------------------------------------
// CKKS / BGV multiplication on the HYBRID engine: EvalMult / EvalSquare with
// relinearisation (base-leveledshe.cpp:199-338, cores 657-750), Relinearize
// (341-372) and ModReduceInternalInPlace (ckksrns-leveledshe.cpp:107-132,
// bgvrns-leveledshe.cpp:45-77), composed from the tensor product, the key
// switch (whose ModDown takes the sums c0 + ab[0], c1 + ab[1] in its last pass)
// and rescale_run.  The rescaling tables come from the engine's moduli.
// ---------------------------------------------------------------------------
// Tables for dropping tower l = towers - 1 (ckksrns-cryptoparameters.cpp:66-87,
// bgvrns-cryptoparameters.cpp:91-107): a_i = qlInvModq[i] = q_l^-1 mod q_i;
// BGV: negtInvModq = -t^-1 mod q_l; CKKS: QlQlInvModqlDivqlModq[i] = q_i - a_i.
// With Q = prod_{j<l} q_j and b = Q^-1 mod q_l, b Q = 1 + k q_l and the table is
// k = floor(b Q / q_l) mod q_i; Q = 0 mod q_i gives k q_l = -1, k = -a_i.
// rs_build turns them into the words ofhe_hip_drop_last_and_scale /
// ofhe_hip_mod_reduce build from the caller's constants (evaluation form).
static int rs_tables(ofhe_ks_t k, u32 towers, u64 t, const RsTab** out) {
    std::lock_guard<std::mutex> lk(k->mu);
    const auto key = std::make_pair(towers, t);
    auto it = k->rescale.find(key);
    if (it == k->rescale.end()) {
        const u32 L = towers - 1;
        const u64 ql = k->q[L];
        std::vector<u64> a(L), c(L);
        for (u32 i = 0; i < L; i++) {
            a[i] = invmod(ql % k->q[i], k->q[i]);
            c[i] = k->q[i] - a[i];
        }
        it = k->rescale.emplace(key, rs_build(k->q.data(), L, t ? SW_XPYA : SW_AXPY, true, c.data(), a.data(), t,
                                              t ? ql - invmod(t % ql, ql) : 1)).first;
    }
    *out = &it->second;
    return OFHE_OK;
}

static int she_scheme_check(int scheme, u64 t) {
    if (scheme != OFHE_SHE_CKKS && scheme != OFHE_SHE_BGV) return fail(OFHE_ERR_ARG, "scheme must be OFHE_SHE_CKKS or OFHE_SHE_BGV");
    if (scheme == OFHE_SHE_CKKS && t != 0) return fail(OFHE_ERR_ARG, "OFHE_SHE_CKKS takes t = 0");
    if (scheme == OFHE_SHE_BGV && t < 2) return fail(OFHE_ERR_ARG, "OFHE_SHE_BGV needs a plaintext modulus t >= 2");
    return OFHE_OK;
}

// t (non-zero) is invertible modulo q[0..size_ql) and, with_p, modulo every p (the moduli are prime)
static int she_t_check(ofhe_ks_t k, u32 size_ql, u64 t, bool with_p) {
    if (!t) return OFHE_OK;
    for (u32 i = 0; i < size_ql; i++)
        if (t % k->q[i] == 0)
            return fail(OFHE_ERR_ARG, "t is not invertible modulo tower q[" + std::to_string(i) + "]");
    for (u32 j = 0; with_p && j < k->size_p; j++)
        if (t % k->p[j] == 0)
            return fail(OFHE_ERR_ARG, "t is not invertible modulo tower p[" + std::to_string(j) + "]");
    return OFHE_OK;
}

static bool she_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// `levels` >= 1 rescalings, one after another in the reference's order, of nelem
// elements x[e] (batch stride xs = l N) into out[e] (dense over l - levels towers);
// the levels in between live in scratch, in place from the second on
static int rescale_levels(ofhe_ks_t k, u32 l, int scheme, u64 t, u32 levels, u32 nelem, const u64* const* x,
                          u64* const* out, u32 batch, hipStream_t s) {
    std::vector<const RsTab*> tabs(levels);
    for (u32 lv = 0; lv < levels; lv++) RCCHK(rs_tables(k, l - lv, scheme == OFHE_SHE_BGV ? t : 0, &tabs[lv]));
    Scratch mid;
    const u64 ms = k->words_q(l - 1);
    if (levels > 1) RCCHK(mid.alloc((size_t)nelem * batch * ms * 8, s, k->ctx));
    std::vector<const u64*> cur(x, x + nelem);
    std::vector<u64*> nxt(nelem);
    u64 cs = k->words_q(l);
    for (u32 lv = 0; lv < levels; lv++) {
        const bool last = lv + 1 == levels;
        const u64 os = last ? k->words_q(l - levels) : ms;
        for (u32 e = 0; e < nelem; e++) nxt[e] = last ? out[e] : mid.w() + (u64)e * batch * ms;
        RCCHK(rescale_run(k->plan, l - lv, cur.data(), cs, nxt.data(), os, nelem, true, *tabs[lv], batch, s));
        cur.assign(nxt.begin(), nxt.end());
        cs = os;
    }
    return OFHE_OK;
}

int ofhe_hip_ks_rescale(ofhe_ks_t k, uint32_t size_ql, int scheme, uint64_t t, uint32_t levels, uint32_t nelem,
                        const uint64_t* const* x, uint64_t* const* out, uint32_t batch, void* stream) {
    // the checks that need no engine first, then the engine, then those that need its dimensions
    if (!x || !out) return fail(OFHE_ERR_ARG, "NULL element pointer array");
    if (nelem == 0 || batch == 0) return fail(OFHE_ERR_ARG, "nelem and batch must be >= 1");
    for (u32 e = 0; e < nelem; e++) {
        if (!x[e] || !out[e]) return fail(OFHE_ERR_ARG, "NULL data pointer");
        if (!she_aligned(x[e]) || !she_aligned(out[e])) return fail(OFHE_ERR_ARG, "buffers must be 16-byte aligned");
    }
    RCCHK(she_scheme_check(scheme, t));
    if (levels == 0) return fail(OFHE_ERR_ARG, "levels must be >= 1");
    if (levels >= size_ql) return fail(OFHE_ERR_ARG, "levels must be below size_ql");
    RCCHK(ks_check(k, size_ql, batch));
    RCCHK(she_t_check(k, size_ql, t, false));
    const u64 xw = batch * k->words_q(size_ql), ow = batch * k->words_q(size_ql - levels);
    for (u32 e = 0; e < nelem; e++) {
        for (u32 j = 0; j < nelem; j++)
            if (words_overlap(out[e], ow, x[j], xw) || (j != e && words_overlap(out[e], ow, out[j], ow)))
                return fail(OFHE_ERR_ARG, "an output overlaps an input or another output");
    }
    return rescale_levels(k, size_ql, scheme, t, levels, nelem, x, out, batch, pick(stream));
}

int ofhe_hip_ks_relinearize(ofhe_ks_t k, uint32_t size_ql, uint32_t nelem, const uint64_t* const* c,
                            const uint64_t* const* key_b, const uint64_t* const* key_a, uint64_t* out0,
                            uint64_t* out1, uint64_t t, uint32_t batch, void* stream) {
    if (!c || !key_b || !key_a) return fail(OFHE_ERR_ARG, "NULL element or key pointer array");
    if (!out0 || !out1) return fail(OFHE_ERR_ARG, "NULL data pointer");
    if (nelem < 3) return fail(OFHE_ERR_ARG, "relinearisation needs nelem >= 3 elements");
    if (batch == 0) return fail(OFHE_ERR_ARG, "batch must be >= 1");
    for (u32 j = 0; j < nelem; j++) {
        if (!c[j]) return fail(OFHE_ERR_ARG, "NULL data pointer");
        if (j >= 2 && (!key_b[j - 2] || !key_a[j - 2])) return fail(OFHE_ERR_ARG, "NULL evaluation key pointer");
        if (!she_aligned(c[j])) return fail(OFHE_ERR_ARG, "buffers must be 16-byte aligned");
    }
    if (!she_aligned(out0) || !she_aligned(out1)) return fail(OFHE_ERR_ARG, "buffers must be 16-byte aligned");
    if (out0 == out1) return fail(OFHE_ERR_ARG, "out0 and out1 must be distinct buffers");
    KsLevel* L = nullptr;
    RCCHK(ks_enter(k, size_ql, batch, &L));
    RCCHK(she_t_check(k, size_ql, t, true));
    const u64 w = batch * k->words_q(size_ql), kw = L->beta * k->key_stride();
    RCCHK(outputs_apart(out0, out1, w));
    u64* const outs[2] = {out0, out1};
    for (u32 o = 0; o < 2; o++) {
        for (u32 j = 0; j < nelem; j++)
            if (words_overlap(outs[o], w, c[j], w) && !(j == o && outs[o] == c[j]))
                return fail(OFHE_ERR_ARG, "outputs may alias only their own element (out0 == c[0], out1 == c[1])");
        for (u32 j = 0; j + 2 < nelem; j++)
            if (words_overlap(outs[o], w, key_b[j], kw) || words_overlap(outs[o], w, key_a[j], kw))
                return fail(OFHE_ERR_ARG, "outputs must not alias the keys");
    }
    // the second and later key switches add into the running output, in place
    for (u32 j = 2; j < nelem; j++)
        RCCHK(ks_core_impl(k, L, size_ql, c[j], key_b[j - 2], key_a[j - 2], out0, out1, j == 2 ? c[0] : out0,
                           j == 2 ? c[1] : out1, t, batch, pick(stream)));
    return OFHE_OK;
}

int ofhe_hip_ks_eval_mult(ofhe_ks_t k, uint32_t size_ql, const uint64_t* c0, const uint64_t* c1, const uint64_t* d0,
                          const uint64_t* d1, const uint64_t* key_b, const uint64_t* key_a, int scheme, uint64_t t,
                          uint32_t levels, uint64_t* out0, uint64_t* out1, uint32_t batch, void* stream) {
    if (!c0 || !c1 || !key_b || !key_a || !out0 || !out1) return fail(OFHE_ERR_ARG, "NULL data pointer");
    if (!d0 != !d1) return fail(OFHE_ERR_ARG, "d0 and d1: both given (EvalMult) or both NULL (EvalSquare)");
    if (batch == 0) return fail(OFHE_ERR_ARG, "batch must be >= 1");
    for (const void* p : {(const void*)c0, (const void*)c1, (const void*)d0, (const void*)d1, (const void*)out0,
                          (const void*)out1})
        if (!she_aligned(p)) return fail(OFHE_ERR_ARG, "buffers must be 16-byte aligned");
    RCCHK(she_scheme_check(scheme, t));
    if (levels >= size_ql) return fail(OFHE_ERR_ARG, "levels must be below size_ql");
    if (out0 == out1) return fail(OFHE_ERR_ARG, "out0 and out1 must be distinct buffers");
    KsLevel* L = nullptr;
    RCCHK(ks_enter(k, size_ql, batch, &L));
    RCCHK(she_t_check(k, size_ql, t, true));
    const u32 l = size_ql;
    const u64 N = 1ull << k->log_n, w = batch * k->words_q(l), ow = batch * k->words_q(l - levels);
    const u64 kw = L->beta * k->key_stride();
    RCCHK(outputs_apart(out0, out1, ow));
    for (const u64* o : {out0, out1}) {
        // the tensor product consumes the operands before anything is written: an
        // output may start where an operand starts (the InPlace forms)
        for (const u64* a : {c0, c1, d0, d1})
            if (a && o != a && words_overlap(o, ow, a, w))
                return fail(OFHE_ERR_ARG, "an output overlaps an operand without starting at its address");
        if (words_overlap(o, ow, key_b, kw) || words_overlap(o, ow, key_a, kw))
            return fail(OFHE_ERR_ARG, "outputs must not alias the keys");
    }
    if ((u64)((N / 2 + 255) / 256) * batch * l >= (1ull << 31))
        return fail(OFHE_ERR_ARG, "batch too large for one launch");
    hipStream_t s = pick(stream);
    Scratch T;  // the three elements of the product, one after another
    RCCHK(T.alloc((size_t)3 * w * 8, s, k->ctx));
    u64 *T0 = T.w(), *T1 = T0 + w, *T2 = T1 + w;
    RCCHK(tensor2_run(k->plan, l, c0, c1, d0, d1, T0, T1, T2, batch, s));
    if (levels == 0) return ks_core_impl(k, L, l, T2, key_b, key_a, out0, out1, T0, T1, t, batch, s);
    RCCHK(ks_core_impl(k, L, l, T2, key_b, key_a, T0, T1, T0, T1, t, batch, s));
    const u64* const xs[2] = {T0, T1};
    u64* const outs[2] = {out0, out1};
    return rescale_levels(k, l, scheme, t, levels, 2, xs, outs, batch, s);
}
