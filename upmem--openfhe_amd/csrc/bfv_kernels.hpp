// bfv_kernels.hpp -- the BFV (HPS) multiplication's per-coefficient RNS loops
// on gfx950: the exact, floating-point-corrected basis switch
// DCRTPolyImpl::SwitchCRTBasis (dcrtpoly-impl.h:1178-1230) and the
// DCRTPoly-to-DCRTPoly ScaleAndRound (dcrtpoly-impl.h:1876-1955), both bit-exact
// with the reference's HAVE_INT128 && NATIVEINT == 64 branches, the value of
// the floating-point correction term included.
//
// Floating-point contract (the reference's baseline x86-64 build: SSE2 doubles,
// no fused multiply-add):
//   * nu starts at 0.5.  For source towers i = 0, 1, ... in that order:
//       nu = nu + (double(y_i) * qInv[i])      SwitchCRTBasis
//       nu = nu + (frac[i] * double(x_i))      ScaleAndRound
//   * every multiply and every add is rounded separately to IEEE double,
//     round-to-nearest-even: fp_mul / fp_add below are compiled with
//     contraction off, so a*b+c never becomes one v_fma_f64;
//   * no tree or cross-lane reordering of the sum, no float.  Where a kernel
//     spreads the source towers over lanes (k_switch_mma) the PRODUCTS are
//     computed where the y_i live and exchanged; every lane then performs the
//     additions itself, in tower order;
//   * double(uint64) is the correctly rounded conversion (values reach 2^60):
//     u2d is v_cvt_f64_u32 of both halves (exact), an exact scaling by 2^32
//     and ONE rounded add;
//   * alpha = floor(nu); nu >= 0.5 always (every term is >= 0).
#pragma once
#include "bconv_mma.hpp"

namespace ofhe {

__device__ __forceinline__ double u2d(u64 v) { return __ull2double_rn(v); }
__device__ __forceinline__ double fp_mul(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double fp_add(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
// nu + (a * b): two roundings.  The empty asm pins the rounded product in a
// register, so no later pass can fold it into the add.
__device__ __forceinline__ double nu_step(double nu, double a, double b) {
    double p = fp_mul(a, b);
    asm volatile("" : "+v"(p));
    return fp_add(nu, p);
}

// Tables of the exact switch, derived from the converter's moduli on its
// first exact call (ofhe_hip_switch_crt_basis) and cached in the handle.
struct ExactArgs {
    const double* qinv;  // [size_q]  1.0 / double(q_i)        (bfvrns-cryptoparameters.cpp:270-273, 441-444)
    const u64* aq;       // [size_q + 1][size_p]  a Q mod p_j  (bfvrns-cryptoparameters.cpp:343-350, 418-424)
};

// alpha = static_cast<usint>(nu) (dcrtpoly-impl.h:1209), in [0, size_q]: the
// bound keeps the table row inside alphaQModp whatever the inputs are.
__device__ __forceinline__ u32 alpha_of(double nu, u32 size_q) {
    const u32 a = (u32)nu;
    return a < size_q ? a : size_q;
}

// ---------------------------------------------------------------------------
// SwitchCRTBasis on the VALU, any number of sources: k_bconv's 128-bit sums
// (eltwise_kernels.hpp) with nu accumulated next to the first tile's y_i and
// ModSubFast(alphaQModp[alpha][j]) in the store (dcrtpoly-impl.h:1195-1226).
// One thread per (batch, ri); targets in tiles of PT towers.
// ---------------------------------------------------------------------------
template <int PT>
__global__ __launch_bounds__(256) void k_switch_wide(BconvArgs A, ExactArgs E, const u64* __restrict__ x,
                                                     u64* __restrict__ out, u32 batch) {
    OFHE_VGPR_FLOOR();
    const u32 N = 1u << A.log_n;
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (u64)batch * N) return;
    const u32 b = (u32)(gid >> A.log_n), ri = (u32)(gid & (N - 1));
    const u64* xb = x + (u64)b * A.in_stride + ri;
    u64* ob = out + (u64)b * A.out_stride + ri;
    double nu = 0.5;
    const u64* aq = nullptr;
    for (u32 j0 = 0; j0 < A.size_p; j0 += PT) {
        u64 lo[PT], hi[PT];
#pragma unroll
        for (int j = 0; j < PT; j++) lo[j] = hi[j] = 0;
        const u32 jn = min((u32)PT, A.size_p - j0);
        for (u32 i = 0; i < A.size_q; i++) {
            const u64 y = shoup_canon(ld_s(xb + (u64)i * N), A.qhinv[2 * i], A.qhinv[2 * i + 1], A.qv[i]);
            if (j0 == 0) nu = nu_step(nu, u2d(y), E.qinv[i]);
            const u64* qm = A.qhmodp + (u64)i * A.size_p + j0;
#pragma unroll
            for (int j = 0; j < PT; j++) {
                if (j < (int)jn) {
                    u64 pl, ph;
                    mul128(y, qm[j], pl, ph);
                    const u64 s = lo[j] + pl;
                    hi[j] += ph + (s < pl);
                    lo[j] = s;
                }
            }
        }
        if (j0 == 0) aq = E.aq + (u64)alpha_of(nu, A.size_q) * A.size_p;
#pragma unroll
        for (int j = 0; j < PT; j++) {
            if (j < (int)jn) {
                const u32 jj = j0 + j;
                const u32 jo = jj >= A.gap_at ? jj + A.gap : jj;
                const u64 p = A.pv[jj];
                const u64 r = barrett128(lo[j], hi[j], p, A.pmu[2 * jj], A.pmu[2 * jj + 1]);
                ob[(u64)jo * N] = modsub_fast(r, aq[jj], p);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// SwitchCRTBasis on the VALU, <= 16 sources: k_bconv_limb's 30-bit limb sums.
// The canonical y_i are computed once per coefficient (nu with them) and kept
// as limbs in the thread's own LDS column across the target tiles.
// ---------------------------------------------------------------------------
template <int PT>
__global__ __launch_bounds__(256) void k_switch_limb(BconvArgs A, ExactArgs E, const u64* __restrict__ x,
                                                     u64* __restrict__ out, u32 batch) {
    OFHE_VGPR_FLOOR();
    __shared__ u64 ys[BCONV_LIMB_QMAX][256];
    const u32 N = 1u << A.log_n;
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (u64)batch * N) return;
    const u32 b = (u32)(gid >> A.log_n), ri = (u32)(gid & (N - 1));
    const u64* xb = x + (u64)b * A.in_stride + ri;
    u64* ob = out + (u64)b * A.out_stride + ri;
    const u32 ppad = (A.size_p + PT - 1) / PT * PT;
    const u32 tid = threadIdx.x;
    double nu = 0.5;
    for (u32 i = 0; i < A.size_q; i++) {
        const u64 y = shoup_canon(ld_s(xb + (u64)i * N), A.qhinv[2 * i], A.qhinv[2 * i + 1], A.qv[i]);
        nu = nu_step(nu, u2d(y), E.qinv[i]);
        ys[i][tid] = (y & LIMB_MASK) | ((y >> LIMB) << 32);
    }
    const u64* aq = E.aq + (u64)alpha_of(nu, A.size_q) * A.size_p;
    for (u32 j0 = 0; j0 < A.size_p; j0 += PT) {
        u64 a0[PT], a1[PT], a2[PT], a3[PT];
#pragma unroll
        for (int j = 0; j < PT; j++) a0[j] = a1[j] = a2[j] = a3[j] = 0;
#pragma unroll OFHE_BCONV_UNROLL
        for (u32 i = 0; i < A.size_q; i++) {
            const u64 yy = ys[i][tid];
            const u32 y0 = lo32(yy), y1 = hi32(yy);
            const u64* cl = A.qhlimb + (u64)i * ppad + j0;
#pragma unroll
            for (int j = 0; j < PT; j++) {
                const u64 c = cl[j];
                a0[j] = mad32(y0, lo32(c), a0[j]);
                a1[j] = mad32(y0, hi32(c), a1[j]);
                a2[j] = mad32(y1, lo32(c), a2[j]);
                a3[j] = mad32(y1, hi32(c), a3[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < PT; j++) {
            const u32 jj = j0 + j;
            if (jj < A.size_p) {
                const u32 jo = jj >= A.gap_at ? jj + A.gap : jj;
                const LimbRed R{A.pv[jj], A.pred[3 * jj], A.pred[3 * jj + 1], A.pred[3 * jj + 2]};
                const u64 r = limb_reduce<true>(a0[j], a1[j], a2[j], a3[j], R);
                st_s(ob + (u64)jo * N, modsub_fast(r, aq[jj], R.m));
            }
        }
    }
}

// ---------------------------------------------------------------------------
// SwitchCRTBasis on the matrix cores (<= 64 sources, N >= 32): k_bconv_mma's
// integer GEMM (bconv_mma.hpp, same fragment table, same LDS image, same
// grid) with canonical outputs and the correction in the store epilogue.
// A wave holds 32 coefficients; lane c + 32 h has the y_i of sources
// 4 s + 2 h + {0, 1} of K-step s.  Each lane forms the products
// double(y_i) * qInv[i] of its own sources, the two lane halves exchange them
// (one 64-lane swap per product), and BOTH lanes of a coefficient then add all
// four products of the K-step to nu in tower order -- so the sum is the
// reference's left-to-right sum and both lanes hold the same alpha.  Sources
// past size_q contribute +0.0, which leaves nu unchanged.
// ---------------------------------------------------------------------------
template <int KS, bool SPQ>
__global__ __launch_bounds__(BCONV_MMA_THREADS, OFHE_BCONV_MMA_WAVES) void k_switch_mma(
    BconvArgs A, ExactArgs E, const u64* __restrict__ x, u64* __restrict__ out, u32 batch) {
    OFHE_VGPR_FLOOR();
    constexpr bool WIDE = KS > 8;
    extern __shared__ __attribute__((aligned(16))) unsigned char bm_lds[];
    const u32 tiles = A.mm_tiles, tpc = A.mm_tpc;
    const u32 t0 = blockIdx.y * tpc;
    const u32 nt = min(tpc, tiles - t0);
    i32x4* frag = reinterpret_cast<i32x4*>(bm_lds);                          // [nt][KS][64]
    BmRed* red = reinterpret_cast<BmRed*>(bm_lds + (size_t)nt * KS * 1024);  // [4 nt]
    BmSrc* src = reinterpret_cast<BmSrc*>(red + 4 * nt);                     // [4 KS]
    {
        const i32x4* gf = reinterpret_cast<const i32x4*>(A.mm_tab) + (size_t)t0 * KS * 64;
        const i32x4* gr = reinterpret_cast<const i32x4*>(A.mm_tab) + (size_t)tiles * KS * 64 + (size_t)t0 * 16;
        const i32x4* gs = reinterpret_cast<const i32x4*>(A.mm_tab) + (size_t)tiles * KS * 64 + (size_t)tiles * 16;
        i32x4* lf = frag;
        i32x4* lr = reinterpret_cast<i32x4*>(red);
        i32x4* ls = reinterpret_cast<i32x4*>(src);
        for (u32 k = threadIdx.x; k < nt * KS * 64; k += blockDim.x) lf[k] = gf[k];
        for (u32 k = threadIdx.x; k < nt * 16; k += blockDim.x) lr[k] = gr[k];
        for (u32 k = threadIdx.x; k < KS * 8; k += blockDim.x) ls[k] = gs[k];
    }
    __syncthreads();
    const BmW W = bm_weights();
    const u32 lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const u32 N = 1u << A.log_n;
    const u64 groups = ((u64)batch << A.log_n) >> 5;
    const u32 wpb = blockDim.x >> 6;
    const u64 gstep = (u64)gridDim.x * wpb;
    // g is the same for every lane of a wave, so the lane exchange below always
    // runs with the whole wave active
    for (u64 g = (u64)blockIdx.x * wpb + (threadIdx.x >> 6); g < groups; g += gstep) {
        const u64 e = (g << 5) + c;
        const u64 b = e >> A.log_n;
        const u32 ri = (u32)(e & (N - 1));
        const u64* xb = x + b * A.in_stride + ri;
        u64* ob = out + b * A.out_stride + ri;
        i32x4 bf[KS];
        double nu = 0.5;
#pragma unroll
        for (int s = 0; s < KS; s++) {
            u64 d[2];
            double pr[2];
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const u32 i = 4 * s + 2 * h + u;
                u64 y = 0;
                double qi = 0.0;
                if (i < A.size_q) {
                    const BmSrc S = src[i];
                    y = shoup_canon(ld_s(xb + (u64)i * N), S.w, S.wp, S.q);
                    qi = E.qinv[i];
                }
                d[u] = digits8(y);
                pr[u] = fp_mul(u2d(y), qi);
            }
            bf[s] = i32x4{(int)lo32(d[0]), (int)hi32(d[0]), (int)lo32(d[1]), (int)hi32(d[1])};
            const double o0 = __shfl_xor(pr[0], 32, 64), o1 = __shfl_xor(pr[1], 32, 64);
            // towers 4 s, 4 s + 1 live in the h = 0 lane, 4 s + 2, 4 s + 3 in the h = 1 lane
            double a0 = h ? o0 : pr[0], a1 = h ? o1 : pr[1], a2 = h ? pr[0] : o0, a3 = h ? pr[1] : o1;
            asm volatile("" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3));
            nu = fp_add(fp_add(fp_add(fp_add(nu, a0), a1), a2), a3);
        }
        const u64* aq = E.aq + (u64)alpha_of(nu, A.size_q) * A.size_p;
        for (u32 t = 0; t < nt; t++) {
            i32x16 acc = {};
#pragma unroll
            for (int s = 0; s < KS; s++)
                acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(frag[(t * KS + s) * 64 + lane], bf[s], acc, 0, 0, 0);
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const u32 j = 4 * (t0 + t) + 2 * h + u;
                if (j < A.size_p) {
                    int C[8];
#pragma unroll
                    for (int k = 0; k < 8; k++) C[k] = acc[8 * u + k];
                    const u32 jo = j >= A.gap_at ? j + A.gap : j;
                    const BmRed R = red[4 * t + 2 * h + u];
                    const u64 r = bm_reduce<false, SPQ, WIDE>(C, R, W);
                    st_s(ob + (u64)jo * N, modsub_fast(r, aq[j], R.p));
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// ScaleAndRound, DCRTPoly -> DCRTPoly (dcrtpoly-impl.h:1876-1955).
// x: [batch][size_i + size_o towers][N]; the size_i summed towers start at
// tower in0, the output basis' own towers at tower own0.  One thread per
// (batch, ri): nu over the summed towers, then per output tower the 128-bit
// sum of size_i + 1 products, BarrettUint128ModUint64 and + (alpha mod o_j).
// Both reference branches (alpha as a native word, 1911-1931; as a 128-bit
// integer, 1933-1951) compute floor(nu) mod o_j: floor(nu) is taken exactly
// from the double's mantissa and exponent as a 128-bit integer and reduced,
// also at nu == 2^64, where the reference's cast is undefined.
// ---------------------------------------------------------------------------
struct SrArgs {
    const u64* tab;      // [size_o][size_i + 1]   tOSHatInvModsDivsModo
    const double* frac;  // [size_i]               tOSHatInvModsDivsFrac
    const u64* ov;       // [size_o]
    const u64* omu;      // [size_o][2]            floor(2^128 / o_j)
    u32 log_n, size_i, size_o, in0, own0;
};

// floor(nu) for 0.5 <= nu < 2^127, exact
__device__ __forceinline__ void floor_u128(double nu, u64& lo, u64& hi) {
    const u64 bits = (u64)__double_as_longlong(nu);
    const int ex = (int)((bits >> 52) & 0x7FF) - 1075;  // nu = m 2^ex
    const u64 m = (bits & ((1ull << 52) - 1)) | (1ull << 52);
    if (ex >= 64) {
        lo = 0;
        hi = m << min(ex - 64, 11);  // m < 2^53 and nu < 2^127: the shift is at most 10
    } else if (ex > 0) {
        lo = m << ex;
        hi = m >> (64 - ex);
    } else {
        lo = ex > -64 ? m >> (-ex) : 0;
        hi = 0;
    }
}

template <int PT>
__global__ __launch_bounds__(256) void k_scale_round(SrArgs A, const u64* __restrict__ x, u64* __restrict__ out,
                                                     u32 batch) {
    OFHE_VGPR_FLOOR();
    const u32 N = 1u << A.log_n;
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (u64)batch * N) return;
    const u32 b = (u32)(gid >> A.log_n), ri = (u32)(gid & (N - 1));
    const u64* xb = x + ((u64)b * (A.size_i + A.size_o) << A.log_n) + ri;
    u64* ob = out + ((u64)b * A.size_o << A.log_n) + ri;
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
                ob[(u64)jj * N] = modadd_fast(cur, am, o);
            }
        }
    }
}

}  // namespace ofhe
