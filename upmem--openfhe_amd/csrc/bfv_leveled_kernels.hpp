// bfv_leveled_kernels.hpp -- the two per-coefficient loops HPSPOVERQLEVELED adds
// to the BFV multiplication once it drops levels (gfx950):
//   DCRTPolyImpl::ExpandCRTBasisQlHat  dcrtpoly-impl.h:1514-1534  (k_expand_ql_hat)
//   ScaleAndRound (dcrtpoly-impl.h:1876-1955) followed by ExpandCRTBasisQlHat in
//   one launch                                                     (k_scale_round_lift)
// l is the index of the last kept tower: Q_l = q_0 .. q_l, size_ql = l + 1.
#pragma once
#include "bfv_kernels.hpp"

namespace ofhe {

struct QlHatArgs {
    const u64* tab;  // [size_ql][3]: q_i, QlHatModq_i = (Q / Q_l) mod q_i, its Shoup precon
    u32 log_n, size_ql, size_q;
};

// ---------------------------------------------------------------------------
// ExpandCRTBasisQlHat, optionally fused with the += that follows it in
// RelinearizeCore (bfvrns-leveledshe.cpp:883-896):
//   out_i = x_i QlHatModq_i mod q_i (ModMulFastConstEq) [+ addend_i, ModAddFastEq]   i <= l
//   out_i = addend_i, or 0 without an addend                                          i >  l
// x [batch][size_ql][N], addend / out [batch][size_q][N]; the form of the data
// does not matter.  A pure stream: one (batch, tower) row per bpr blocks, so
// the tower's constants are wave-uniform; two words per lane, 16-byte accesses
// (N >= 2).  The rows cover `rt` towers of out: size_q, or size_ql when out is
// the addend's own buffer (its towers past l are already in place).  The zero
// towers load nothing.
// ---------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void k_expand_ql_hat(QlHatArgs A, const u64* __restrict__ x, const u64* addend,
                                                              u64* out, u32 bpr, u32 rt) {
    OFHE_VGPR_FLOOR();
    const u32 row = blockIdx.x / bpr;
    const u64 j = 2 * ((u64)(blockIdx.x % bpr) * blockDim.x + threadIdx.x);
    if (j >= (1ull << A.log_n)) return;
    const u32 b = row / rt, t = row % rt;
    const u64 e = (((u64)b * A.size_q + t) << A.log_n) + j;
    u64x2 r;
    if (t < A.size_ql) {
        const u64 q = A.tab[3 * t], w = A.tab[3 * t + 1], wp = A.tab[3 * t + 2];
        const u64x2 v = ld2_s(x + (((u64)b * A.size_ql + t) << A.log_n) + j);
        r.x = shoup_canon(v.x, w, wp, q);
        r.y = shoup_canon(v.y, w, wp, q);
        if (addend) {
            const u64x2 a = ld2_s(addend + e);
            r.x = modadd_fast(r.x, a.x, q);
            r.y = modadd_fast(r.y, a.y, q);
        }
    } else if (addend) {
        r = ld2_s(addend + e);
    } else {
        r.x = r.y = 0;
    }
    st2_s(out + e, r);
}

// ---------------------------------------------------------------------------
// ScaleAndRound to Q_l and ExpandCRTBasisQlHat in one launch: k_scale_round's
// loop (the same nu chain through nu_step, the same floor_u128, 128-bit sums
// and Barrett reductions, in the same order) whose store multiplies tower j by
// QlHatModq_j and writes it at the stride of size_q towers; each thread also
// zeroes towers size_o .. size_q - 1 of its coefficient.  The size_o
// intermediate towers are never written and read back.
// x: [batch][size_i + size_o][N] as k_scale_round; out: [batch][size_q][N].
// ---------------------------------------------------------------------------
template <int PT>
__global__ __launch_bounds__(256) void k_scale_round_lift(SrArgs A, QlHatArgs H, const u64* __restrict__ x,
                                                          u64* __restrict__ out, u32 batch) {
    OFHE_VGPR_FLOOR();
    const u32 N = 1u << A.log_n;
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (u64)batch * N) return;
    const u32 b = (u32)(gid >> A.log_n), ri = (u32)(gid & (N - 1));
    const u64* xb = x + ((u64)b * (A.size_i + A.size_o) << A.log_n) + ri;
    u64* ob = out + ((u64)b * H.size_q << A.log_n) + ri;
    const u64* xin = xb + (u64)A.in0 * N;
    const u64* xown = xb + (u64)A.own0 * N;
    const u32 row = A.size_i + 1;
    double nu = 0.5;
    u64 al = 0, ah = 0;
    for (u32 j0 = 0; j0 < A.size_o; j0 += PT) {
        u64 lo[PT], hi[PT];
#pragma unroll
        for (int j = 0; j < PT; j++) lo[j] = hi[j] = 0;
        const u32 jn = min((u32)PT, A.size_o - j0);
        for (u32 i = 0; i < A.size_i; i++) {
            const u64 xi = ld_s(xin + (u64)i * N);
            if (j0 == 0) nu = nu_step(nu, A.frac[i], u2d(xi));
#pragma unroll
            for (int j = 0; j < PT; j++) {
                if (j < (int)jn) {
                    u64 pl, ph;
                    mul128(xi, A.tab[(u64)(j0 + j) * row + i], pl, ph);
                    const u64 s = lo[j] + pl;
                    hi[j] += ph + (s < pl);
                    lo[j] = s;
                }
            }
        }
        if (j0 == 0) floor_u128(nu, al, ah);
#pragma unroll
        for (int j = 0; j < PT; j++) {
            if (j < (int)jn) {
                const u32 jj = j0 + j;
                u64 pl, ph;
                mul128(ld_s(xown + (u64)jj * N), A.tab[(u64)jj * row + A.size_i], pl, ph);
                const u64 s = lo[j] + pl;
                const u64 sh = hi[j] + ph + (s < pl);
                const u64 o = A.ov[jj], m0 = A.omu[2 * jj], m1 = A.omu[2 * jj + 1];
                const u64 cur = barrett128(s, sh, o, m0, m1);
                const u64 am = barrett128(al, ah, o, m0, m1);
                const u64 v = modadd_fast(cur, am, o);
                st_s(ob + (u64)jj * N, shoup_canon(v, H.tab[3 * jj + 1], H.tab[3 * jj + 2], o));
            }
        }
    }
    for (u32 jj = A.size_o; jj < H.size_q; jj++) st_s(ob + (u64)jj * N, 0);
}

}  // namespace ofhe
