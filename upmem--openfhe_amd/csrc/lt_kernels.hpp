// lt_kernels.hpp -- the baby-step/giant-step linear transform of CKKS
// bootstrapping (FHECKKSRNS::EvalLinearTransform, ckksrns-fhe.cpp:1484-1555, and
// the same double-hoisting loops of EvalCoeffsToSlots / EvalSlotsToCoeffs) over
// the extended basis Ql|P: KeySwitchExt, the plaintext-diagonal
// multiply-accumulate of the baby steps, and the giant steps' rotated key
// switches accumulated in registers.
//
// All kernels run one thread per (batch entry, tower, storage position) of
// [batch][towers][N] data; sums are the 30-bit limb sums of k_ks_inner_bs
// (at most 16 products below 2^60 per limb sum, limb_reduce's contract), so
// every output word is the canonical residue the reference's ModMul / ModAdd
// chain ends on.
#pragma once
#include "ks_kernels.hpp"

namespace ofhe {

// KeySwitchHYBRID::KeySwitchExt (keyswitch-hybrid.cpp:231-256) on one element:
// c * (P mod q_t) on the Q towers, zero on the P towers.
// c: [batch][size_ql][N] -> out: [batch][towers][N].
__global__ __launch_bounds__(256) void k_ks_ext(const TowerScalar* __restrict__ pmodq, const u64* __restrict__ c,
                                                u64* __restrict__ out, u64 nthreads, u32 log_n, u32 towers,
                                                u32 size_ql) {
    OFHE_VGPR_FLOOR();
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nthreads) return;
    const u32 row = (u32)(i >> log_n), s = (u32)(i & ((1ull << log_n) - 1));
    const u32 b = row / towers, t = row % towers;
    u64 v = 0;
    if (t < size_ql) {
        const TowerScalar ps = pmodq[t];
        v = shoup_canon(ld_s(c + (((u64)b * size_ql + t) << log_n) + s), ps.s, ps.sp, ps.q);
    }
    st_s(out + i, v);
}

// Sums per launch of k_lt_inner and terms per sum (the limb sums' cap).
constexpr u32 LT_SUM_CAP = 16;
constexpr u32 LT_TERM_CAP = 16;
struct LtSums {
    u32 row[LT_SUM_CAP];   // sum g reads the diagonals row[g] * row_stride + i * diag_stride
    u32 mask[LT_SUM_CAP];  // bit i: term i's diagonal is present
};

// Baby-stationary multiply-accumulate (EvalMultExt / EvalAddExtInPlace,
// ckksrns-fhe.cpp:2373-2396, over the inner loop of 1520-1526): a thread loads
// and limb-splits its 2 NT words of the terms x_i once (both elements) and
// walks the sums of the launch; per sum it loads the present diagonal words
// (one load serves both elements; the next sum's before the current one is
// reduced), accumulates and stores
//   out_e[g] = sum_{i present} x_e[i] * diag[row[g]][i]      e = 0, 1.
// x_e: [NT][batch][towers][N] with x_stride words between terms; the diagonals
// are [towers][N] each, shared by the batch entries; out_e: [nsum][batch][towers][N].
// An absent diagonal is never read (the mask is wave-uniform: a scalar branch).
// acc != 0: add the stored out_e[g] (a later chunk of more than 16 terms).
template <int NT>
__global__ __launch_bounds__(256) void k_lt_inner(const KsTower* __restrict__ tw, const u64* __restrict__ x0,
                                                  const u64* __restrict__ x1, u64 x_stride,
                                                  const u64* __restrict__ diag, u64 diag_stride, u64 row_stride,
                                                  LtSums S, u32 nsum, u64* out0, u64* out1, u64 out_stride,
                                                  u64 nthreads, u32 log_n, u32 towers, u32 acc) {
    OFHE_VGPR_FLOOR();
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nthreads) return;
    const u32 row = (u32)(i >> log_n), s = (u32)(i & ((1ull << log_n) - 1));
    const u32 t = row % towers;
    const KsTower T = tw[t];
    const LimbRed R{T.m, T.r60, T.r60p, T.mu1};
    const u64 inner = ((u64)t << log_n) + s;
    u32 xl[2][NT], xh[2][NT];
#pragma unroll
    for (int k = 0; k < NT; k++) {
        const u64 v0 = ld_s(x0 + (u64)k * x_stride + i), v1 = ld_s(x1 + (u64)k * x_stride + i);
        xl[0][k] = (u32)(v0 & LIMB_MASK);
        xh[0][k] = (u32)(v0 >> LIMB);
        xl[1][k] = (u32)(v1 & LIMB_MASK);
        xh[1][k] = (u32)(v1 >> LIMB);
    }
    u64 nd[NT];
    auto load = [&](u32 g) {
        const u64* d = diag + (u64)S.row[g] * row_stride + inner;
        const u32 m = S.mask[g];
#pragma unroll
        for (int k = 0; k < NT; k++) nd[k] = (m >> k) & 1 ? ld_s(d + (u64)k * diag_stride) : 0;
    };
    load(0);
    for (u32 g = 0; g < nsum; g++) {
        u64 a[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
        for (int k = 0; k < NT; k++) {
            const u32 d0 = (u32)(nd[k] & LIMB_MASK), d1 = (u32)(nd[k] >> LIMB);
#pragma unroll
            for (int e = 0; e < 2; e++) {
                a[e][0] = mad32(xl[e][k], d0, a[e][0]);
                a[e][1] = mad32(xl[e][k], d1, a[e][1]);
                a[e][2] = mad32(xh[e][k], d0, a[e][2]);
                a[e][3] = mad32(xh[e][k], d1, a[e][3]);
            }
        }
        if (g + 1 < nsum) load(g + 1);
        u64 r0 = limb_reduce<false>(a[0][0], a[0][1], a[0][2], a[0][3], R);
        u64 r1 = limb_reduce<false>(a[1][0], a[1][1], a[1][2], a[1][3], R);
        const u64 o = (u64)g * out_stride + i;
        if (acc) {
            r0 = csub(r0 + out0[o], T.m);
            r1 = csub(r1 + out1[o], T.m);
        }
        st_s(out0 + o, r0);
        st_s(out1 + o, r1);
    }
}

// Giant steps: sum over the digit sets j of the launch of
//   sigma_kj(sum_d digits_j[d] * key_j[d])
// (EvalFastRotationExt with addFirst = false, ckksrns-leveledshe.cpp:402-457,
// accumulated by EvalAddExtInPlace, ckksrns-fhe.cpp:1544-1545) in gather form:
// the thread of output position o reads set j's digit and key words at the
// position sigma_kj maps onto o -- rot_dest with the index itself in place of
// its inverse -- so the sum over the sets stays in registers and each output
// word is stored once.  Aligned 2^m blocks map onto aligned blocks: a wave
// still reads whole lines.  The limb sums are reduced every 16 products and
// the canonical partial sums added.  digits: [nset][batch][beta][towers][N].
// add1: [nadd][batch][towers][N] summed into element 1 (the identity giant
// steps' I_j[1], ckksrns-fhe.cpp:1528-1533), or nadd = 0.
// acc != 0: add the stored outputs (a later launch of more than KS_ROT_CAP
// sets; same thread, same word).
// BETA = 0: a runtime digit count (beta > 4).
struct LtRot {
    const u64* kb[KS_ROT_CAP];
    const u64* ka[KS_ROT_CAP];
    u32 k[KS_ROT_CAP];  // the automorphism indices themselves
};
template <int BETA>
__global__ __launch_bounds__(256) void k_lt_outer(const KsTower* __restrict__ tw, const u64* __restrict__ digits,
                                                  LtRot rot, u32 nset, const u64* __restrict__ add1, u32 nadd,
                                                  u64* out0, u64* out1, u64 key_stride, u64 nthreads, u32 beta_rt,
                                                  u32 log_n, u32 towers, u32 batch, u32 acc) {
    OFHE_VGPR_FLOOR();
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nthreads) return;
    const u32 row = (u32)(i >> log_n), o = (u32)(i & ((1ull << log_n) - 1));
    const u32 b = row / towers, t = row % towers;
    const KsTower T = tw[t];
    const LimbRed R{T.m, T.r60, T.r60p, T.mu1};
    const u32 beta = BETA ? BETA : beta_rt;
    const u64 poly = (u64)towers << log_n;
    const u64 inner = (u64)t << log_n;
    u64 a[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    u64 p0 = 0, p1 = 0;
    u32 cnt = 0;
    if (acc) {
        p0 = out0[i];
        p1 = out1[i];
    }
    for (u32 j = 0; j < nset; j++) {
        const u32 src = rot_dest(o, rot.k[j], log_n);
        const u64* d = digits + ((u64)j * batch + b) * beta * poly + inner + src;
        const u64* pb = rot.kb[j] + T.key_off + src;
        const u64* pa = rot.ka[j] + T.key_off + src;
        for (u32 e = 0; e < beta; e++) {
            const u64 x = ld_s(d + (u64)e * poly);
            const u64 w[2] = {ld_s(pb + (u64)e * key_stride), ld_s(pa + (u64)e * key_stride)};
            const u32 x0 = (u32)(x & LIMB_MASK), x1 = (u32)(x >> LIMB);
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const u32 w0 = (u32)(w[k] & LIMB_MASK), w1 = (u32)(w[k] >> LIMB);
                a[k][0] = mad32(x0, w0, a[k][0]);
                a[k][1] = mad32(x0, w1, a[k][1]);
                a[k][2] = mad32(x1, w0, a[k][2]);
                a[k][3] = mad32(x1, w1, a[k][3]);
            }
            if (++cnt == 16) {  // wave-uniform
                p0 = csub(p0 + limb_reduce<false>(a[0][0], a[0][1], a[0][2], a[0][3], R), T.m);
                p1 = csub(p1 + limb_reduce<false>(a[1][0], a[1][1], a[1][2], a[1][3], R), T.m);
#pragma unroll
                for (int k = 0; k < 2; k++) a[k][0] = a[k][1] = a[k][2] = a[k][3] = 0;
                cnt = 0;
            }
        }
    }
    if (cnt) {
        p0 = csub(p0 + limb_reduce<false>(a[0][0], a[0][1], a[0][2], a[0][3], R), T.m);
        p1 = csub(p1 + limb_reduce<false>(a[1][0], a[1][1], a[1][2], a[1][3], R), T.m);
    }
    for (u32 j = 0; j < nadd; j++) p1 = csub(p1 + ld_s(add1 + (u64)j * batch * poly + i), T.m);
    st_s(out0 + i, p0);
    st_s(out1 + i, p1);
}

// The first elements of the giant steps (ckksrns-fhe.cpp:1529, 1541-1542, 1551):
//   out[o] = base[o] + sum_j md0_j[src_j(o)] + sum_k mdid_k[o]
// over [batch][towers][N] (the Q towers only); md0: [nset][batch][towers][N], the
// ModDown of the non-identity giant steps' first elements, gathered as in
// k_lt_outer; mdid: [nid][batch][towers][N], the identity giant steps', as they
// are.  k_add_automorphism generalised to a sum.  base may be out (in place:
// same thread, same word).
struct LtIdx {
    u32 k[KS_ROT_CAP];  // the automorphism indices themselves
};
__global__ __launch_bounds__(256) void k_lt_first(const KsTower* __restrict__ tw, const u64* base,
                                                  const u64* __restrict__ md0, LtIdx rot, u32 nset,
                                                  const u64* __restrict__ mdid, u32 nid, u64* out, u64 nthreads,
                                                  u32 log_n, u32 towers) {
    OFHE_VGPR_FLOOR();
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nthreads) return;
    const u32 row = (u32)(i >> log_n), o = (u32)(i & ((1ull << log_n) - 1));
    const u64 m = tw[row % towers].m;
    const u64 rbase = (u64)row << log_n;
    u64 v = base[i];
    for (u32 j = 0; j < nset; j++)
        v = csub(v + ld_s(md0 + (u64)j * nthreads + rbase + rot_dest(o, rot.k[j], log_n)), m);
    for (u32 j = 0; j < nid; j++) v = csub(v + ld_s(mdid + (u64)j * nthreads + i), m);
    st_s(out + i, v);
}

}  // namespace ofhe
