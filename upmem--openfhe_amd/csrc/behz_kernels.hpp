// behz_kernels.hpp -- the BFV (BEHZ) multiplication's per-coefficient RNS loops
// on gfx950, bit-exact with the reference's HAVE_INT128 && NATIVEINT == 64
// branches (integers only, no floating point):
//   k_behz_q_to_bsk   DCRTPolyImpl::FastBaseConvqToBskMontgomery  dcrtpoly-impl.h:2098-2187
//   k_behz_floor      DCRTPolyImpl::FastRNSFloorq                 dcrtpoly-impl.h:2212-2271
//   k_behz_sk         DCRTPolyImpl::FastBaseConvSK                dcrtpoly-impl.h:2309-2411
//   k_behz_floor_sk   the two above for one coefficient in one launch
// "Bsk" is the size_b towers of B followed by msk (size_b + 1 towers).  One
// thread per (batch, coefficient); k_switch_wide's 128-bit sums (at most 255
// products below 2^120 each, the reference's DoubleNativeInt limit); targets
// in tiles of PT towers, the sources' twisted values recomputed per tile.
// k_behz_q_to_bsk_limb is the first function on k_bconv_limb's 30-bit limb
// sums for at most BCONV_LIMB_QMAX sources.
//
// FastBaseConvSK's negative correction is the centred value: for
// alpha > floor(msk / 2) the reference forms alpha.ModSubFast(msk, q_j), i.e.
// alpha + q_j - msk in unsigned words, which is the residue of alpha - msk
// only while msk - alpha <= q_j.  Here (msk - alpha) B mod q_j is added
// instead, which is that residue for every q_j and equals the reference
// wherever it does not wrap (always when msk < 2 min q_j).
#pragma once
#include "bfv_kernels.hpp"

namespace ofhe {

// Target towers per tile of the BEHZ kernels.
constexpr int BEHZ_PT = 4;
// k_behz_floor_sk keeps the size_b + 1 floor residues of a coefficient in the
// thread's LDS column: at most this many B towers (17 columns of 256 words,
// 34 KiB a workgroup, four workgroups a CU).  Past it the multiplication runs
// k_behz_floor and k_behz_sk.
constexpr u32 BEHZ_FUSED_BMAX = 16;

struct BehzArgs {
    const u64* qv;   // [size_q]
    const u64* qmu;  // [size_q][2]      floor(2^128 / q_i)
    const u64* bv;   // [size_b + 1]     Bsk, msk last
    const u64* bmu;  // [size_b + 1][2]  floor(2^128 / bsk_j)
    // FastBaseConvqToBskMontgomery
    const u64* mtq;  // [size_q][2]      mtildeQHatInvModq, Shoup precon
    const u64* qhb;  // [size_q][size_b + 1]  QHatModbsk
    const u64* qhm;  // [size_q]         QHatModmtilde
    const u64* qhl;  // [size_q][size_b + 1 rounded up to BCONV_PT]  QHatModbsk as 30-bit limbs (k_bconv_limb's form)
    const u64* bred; // [size_b + 1][3]  limb_reduce constants of Bsk
    const u64* qmb;  // [size_b + 1][2]  QModbsk, precon
    const u64* mib;  // [size_b + 1][2]  mtildeInvModbsk, precon
    // FastRNSFloorq
    const u64* tqh;  // [size_q][2]      tQHatInvModq, precon
    const u64* qib;  // [size_q][size_b + 1]  qInvModbsk
    const u64* tqb;  // [size_b + 1][2]  tQInvModbsk, precon
    // FastBaseConvSK
    const u64* bhi;  // [size_b][2]      BHatInvModb, precon
    const u64* bhq;  // [size_b][size_q] BHatModq
    const u64* bhm;  // [size_b]         BHatModmsk
    const u64* bmq;  // [size_q][2]      BModq, precon
    u64 binv, binv_pre;  // BInvModmsk, precon
    u32 neg_qinv_mt;     // negQInvModmtilde (< 2^16)
    u32 log_n, size_q, size_b;
};

// (lo, hi) += a * b
__device__ __forceinline__ void acc128(u64& lo, u64& hi, u64 a, u64 b) {
    u64 pl, ph;
    mul128(a, b, pl, ph);
    const u64 s = lo + pl;
    hi += ph + (s < pl);
    lo = s;
}

// The small Montgomery reduction's store value for Bsk tower jj (modulus m):
// ((r_j QModbsk_j + c) mod m) mtildeInvModbsk_j mod m, r_j the centred r
// (dcrtpoly-impl.h:2168-2184).
__device__ __forceinline__ u64 behz_mont_reduce(const BehzArgs& A, u32 jj, u64 m, u64 c, u32 r) {
    const u64 rj = r >= 0x8000u ? (u64)r + m - 0x10000u : (u64)r;  // 2^16 < every Bsk modulus
    u64 v = shoup_canon(rj, A.qmb[2 * jj], A.qmb[2 * jj + 1], m);
    v = modadd_fast(v, c, m);
    return shoup_canon(v, A.mib[2 * jj], A.mib[2 * jj + 1], m);
}

// ---------------------------------------------------------------------------
// FastBaseConvqToBskMontgomery, coefficient form.  x: [batch][size_q][N]
// (row stride in_stride), out: [batch][size_b + 1][N] (row stride out_stride).
//   y_i = ModMulFastConst(x_i, mtildeQHatInvModq_i)                 (2103-2111)
//   c_j = Barrett(sum_i y_i QHatModbsk[i][j])                       (2114-2126)
//   r   = ((sum_i y_i QHatModmtilde[i]) mod 2^16) negQInvModmtilde mod 2^16
//                                                                   (2150-2166)
//   out_j = ((r_j QModbsk_j + c_j) mod b_j) mtildeInvModbsk_j mod b_j, r_j the
//   centred r (r >= 2^15: r + b_j - 2^16)                           (2168-2184)
// r is accumulated next to the first tile's sums, so it is complete before
// the first store.
// ---------------------------------------------------------------------------
template <int PT>
__global__ __launch_bounds__(256) void k_behz_q_to_bsk(BehzArgs A, const u64* __restrict__ x, u64 in_stride,
                                                       u64* __restrict__ out, u64 out_stride, u32 batch) {
    OFHE_VGPR_FLOOR();
    const u32 N = 1u << A.log_n;
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (u64)batch * N) return;
    const u32 b = (u32)(gid >> A.log_n), ri = (u32)(gid & (N - 1));
    const u64* xb = x + (u64)b * in_stride + ri;
    u64* ob = out + (u64)b * out_stride + ri;
    const u32 nb = A.size_b + 1;
    u32 rm = 0, r = 0;
    for (u32 j0 = 0; j0 < nb; j0 += PT) {
        u64 lo[PT], hi[PT];
#pragma unroll
        for (int j = 0; j < PT; j++) lo[j] = hi[j] = 0;
        const u32 jn = min((u32)PT, nb - j0);
        for (u32 i = 0; i < A.size_q; i++) {
            const u64 y = shoup_canon(ld_s(xb + (u64)i * N), A.mtq[2 * i], A.mtq[2 * i + 1], A.qv[i]);
            if (j0 == 0) rm += lo32(y) * lo32(A.qhm[i]);  // only the low 16 bits are kept
            const u64* c = A.qhb + (u64)i * nb + j0;
#pragma unroll
            for (int j = 0; j < PT; j++)
                if (j < (int)jn) acc128(lo[j], hi[j], y, c[j]);
        }
        if (j0 == 0) r = ((rm & 0xffffu) * A.neg_qinv_mt) & 0xffffu;
#pragma unroll
        for (int j = 0; j < PT; j++) {
            if (j < (int)jn) {
                const u32 jj = j0 + j;
                const u64 m = A.bv[jj];
                const u64 c = barrett128(lo[j], hi[j], m, A.bmu[2 * jj], A.bmu[2 * jj + 1]);
                st_s(ob + (u64)jj * N, behz_mont_reduce(A, jj, m, c, r));
            }
        }
    }
}

// The same with k_bconv_limb's 30-bit limb sums, size_q <= BCONV_LIMB_QMAX: the
// y_i are computed once per coefficient (r with them) and kept as limbs in the
// thread's own LDS column across the target tiles; four v_mad_u64_u32 per
// term and no carries, limb_reduce gives the value BarrettUint128ModUint64
// gives.  The limb table is zero-padded to a multiple of PT columns.
template <int PT>
__global__ __launch_bounds__(256) void k_behz_q_to_bsk_limb(BehzArgs A, const u64* __restrict__ x, u64 in_stride,
                                                            u64* __restrict__ out, u64 out_stride, u32 batch) {
    OFHE_VGPR_FLOOR();
    __shared__ u64 ys[BCONV_LIMB_QMAX][256];
    const u32 N = 1u << A.log_n;
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (u64)batch * N) return;
    const u32 b = (u32)(gid >> A.log_n), ri = (u32)(gid & (N - 1));
    const u64* xb = x + (u64)b * in_stride + ri;
    u64* ob = out + (u64)b * out_stride + ri;
    const u32 nb = A.size_b + 1, ppad = (nb + PT - 1) / PT * PT, tid = threadIdx.x;
    u32 rm = 0;
    for (u32 i = 0; i < A.size_q; i++) {
        const u64 y = shoup_canon(ld_s(xb + (u64)i * N), A.mtq[2 * i], A.mtq[2 * i + 1], A.qv[i]);
        rm += lo32(y) * lo32(A.qhm[i]);
        ys[i][tid] = (y & LIMB_MASK) | ((y >> LIMB) << 32);
    }
    const u32 r = ((rm & 0xffffu) * A.neg_qinv_mt) & 0xffffu;
    for (u32 j0 = 0; j0 < nb; j0 += PT) {
        u64 a0[PT], a1[PT], a2[PT], a3[PT];
#pragma unroll
        for (int j = 0; j < PT; j++) a0[j] = a1[j] = a2[j] = a3[j] = 0;
#pragma unroll OFHE_BCONV_UNROLL
        for (u32 i = 0; i < A.size_q; i++) {
            const u64 yy = ys[i][tid];
            const u32 y0 = lo32(yy), y1 = hi32(yy);
            const u64* cl = A.qhl + (u64)i * ppad + j0;
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
            if (jj < nb) {
                const LimbRed R{A.bv[jj], A.bred[3 * jj], A.bred[3 * jj + 1], A.bred[3 * jj + 2]};
                const u64 c = limb_reduce<true>(a0[j], a1[j], a2[j], a3[j], R);
                st_s(ob + (u64)jj * N, behz_mont_reduce(A, jj, R.m, c, r));
            }
        }
    }
}

// ---------------------------------------------------------------------------
// FastRNSFloorq of one coefficient.  xq: its Q residues, xbsk: its Bsk
// residues (tower stride N); put(j, v) takes output tower j.
//   y_i = x_i tQHatInvModq_i mod q_i                                 (2230-2240)
//   conv_j = Barrett(sum_i y_i qInvModbsk[i][j])                     (2243-2254)
//   out_j = ModSubFast(x_{Q+j} tQInvModbsk_j mod b_j, conv_j)        (2258-2268)
// The input is only read (the reference twists its Q towers in place and
// then discards them).
// ---------------------------------------------------------------------------
template <int PT, class Put>
__device__ __forceinline__ void behz_floor_coeff(const BehzArgs& A, const u64* xq, const u64* xbsk, u32 N, Put&& put) {
    const u32 nb = A.size_b + 1;
    for (u32 j0 = 0; j0 < nb; j0 += PT) {
        u64 lo[PT], hi[PT];
#pragma unroll
        for (int j = 0; j < PT; j++) lo[j] = hi[j] = 0;
        const u32 jn = min((u32)PT, nb - j0);
        for (u32 i = 0; i < A.size_q; i++) {
            const u64 y = shoup_canon(ld_s(xq + (u64)i * N), A.tqh[2 * i], A.tqh[2 * i + 1], A.qv[i]);
            const u64* c = A.qib + (u64)i * nb + j0;
#pragma unroll
            for (int j = 0; j < PT; j++)
                if (j < (int)jn) acc128(lo[j], hi[j], y, c[j]);
        }
#pragma unroll
        for (int j = 0; j < PT; j++) {
            if (j < (int)jn) {
                const u32 jj = j0 + j;
                const u64 m = A.bv[jj];
                const u64 conv = barrett128(lo[j], hi[j], m, A.bmu[2 * jj], A.bmu[2 * jj + 1]);
                const u64 own = shoup_canon(ld_s(xbsk + (u64)jj * N), A.tqb[2 * jj], A.tqb[2 * jj + 1], m);
                put(jj, modsub_fast(own, conv, m));
            }
        }
    }
}

// ---------------------------------------------------------------------------
// FastBaseConvSK of one coefficient.  z(i) gives z_i = x_i BHatInvModb_i mod
// b_i (2331-2338), xmsk the msk residue; ob: output, tower stride N.
//   S_j = Barrett(sum_i z_i BHatModq[i][j])                          (2340-2351)
//   alpha = ((Barrett(sum_i z_i BHatModmsk_i) - x_msk) mod msk) BInvModmsk mod msk
//                                                                    (2355-2373)
//   out_j = (S_j - alpha_c BModq_j) mod q_j, alpha_c = alpha - msk for
//   alpha > floor(msk / 2) (2376-2389; the centred value, see the top of the
//   file).  alpha is accumulated next to the first tile's sums.
// ---------------------------------------------------------------------------
template <int PT, class Z>
__device__ __forceinline__ void behz_sk_coeff(const BehzArgs& A, Z&& z, u64 xmsk, u64* ob, u32 N) {
    const u64 msk = A.bv[A.size_b];
    u64 alo = 0, ahi = 0, mag = 0;
    bool neg = false;
    for (u32 j0 = 0; j0 < A.size_q; j0 += PT) {
        u64 lo[PT], hi[PT];
#pragma unroll
        for (int j = 0; j < PT; j++) lo[j] = hi[j] = 0;
        const u32 jn = min((u32)PT, A.size_q - j0);
        for (u32 i = 0; i < A.size_b; i++) {
            const u64 zi = z(i);
            if (j0 == 0) acc128(alo, ahi, zi, A.bhm[i]);
            const u64* c = A.bhq + (u64)i * A.size_q + j0;
#pragma unroll
            for (int j = 0; j < PT; j++)
                if (j < (int)jn) acc128(lo[j], hi[j], zi, c[j]);
        }
        if (j0 == 0) {
            u64 a = barrett128(alo, ahi, msk, A.bmu[2 * A.size_b], A.bmu[2 * A.size_b + 1]);
            a = shoup_canon(modsub_fast(a, xmsk, msk), A.binv, A.binv_pre, msk);
            neg = a > (msk >> 1);
            mag = neg ? msk - a : a;  // |alpha_c|
        }
#pragma unroll
        for (int j = 0; j < PT; j++) {
            if (j < (int)jn) {
                const u32 jj = j0 + j;
                const u64 m = A.qv[jj];
                const u64 s = barrett128(lo[j], hi[j], m, A.qmu[2 * jj], A.qmu[2 * jj + 1]);
                const u64 ab = shoup_canon(mag, A.bmq[2 * jj], A.bmq[2 * jj + 1], m);  // |alpha_c| B mod q_j
                st_s(ob + (u64)jj * N, neg ? modadd_fast(s, ab, m) : modsub_fast(s, ab, m));
            }
        }
    }
}

// FastRNSFloorq.  x: [batch][size_q + size_b + 1][N] coefficient form, out:
// [batch][size_b + 1][N]; row strides in words.
template <int PT>
__global__ __launch_bounds__(256) void k_behz_floor(BehzArgs A, const u64* __restrict__ x, u64 in_stride,
                                                    u64* __restrict__ out, u64 out_stride, u32 batch) {
    OFHE_VGPR_FLOOR();
    const u32 N = 1u << A.log_n;
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (u64)batch * N) return;
    const u32 b = (u32)(gid >> A.log_n), ri = (u32)(gid & (N - 1));
    const u64* xb = x + (u64)b * in_stride + ri;
    u64* ob = out + (u64)b * out_stride + ri;
    behz_floor_coeff<PT>(A, xb, xb + (u64)A.size_q * N, N, [&](u32 j, u64 v) { st_s(ob + (u64)j * N, v); });
}

// FastBaseConvSK.  x: [batch][size_b + 1][N], out: [batch][size_q][N].
template <int PT>
__global__ __launch_bounds__(256) void k_behz_sk(BehzArgs A, const u64* __restrict__ x, u64 in_stride,
                                                 u64* __restrict__ out, u64 out_stride, u32 batch) {
    OFHE_VGPR_FLOOR();
    const u32 N = 1u << A.log_n;
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (u64)batch * N) return;
    const u32 b = (u32)(gid >> A.log_n), ri = (u32)(gid & (N - 1));
    const u64* xb = x + (u64)b * in_stride + ri;
    behz_sk_coeff<PT>(
        A, [&](u32 i) { return shoup_canon(ld_s(xb + (u64)i * N), A.bhi[2 * i], A.bhi[2 * i + 1], A.bv[i]); },
        ld_s(xb + (u64)A.size_b * N), out + (u64)b * out_stride + ri, N);
}

// FastRNSFloorq then FastBaseConvSK (bfvrns-leveledshe.cpp:390-401) of one
// coefficient: the floor's size_b + 1 residues go to the thread's own LDS
// column ([size_b + 1][256] words of dynamic LDS, size_b <= BEHZ_FUSED_BMAX),
// are twisted there (z_i), and feed the SK sums; they never reach memory.
// Every thread touches its own column only, so no barrier is needed.
// x: [batch][size_q + size_b + 1][N], out: [batch][size_q][N].
template <int PT>
__global__ __launch_bounds__(256) void k_behz_floor_sk(BehzArgs A, const u64* __restrict__ x, u64 in_stride,
                                                       u64* __restrict__ out, u64 out_stride, u32 batch) {
    OFHE_VGPR_FLOOR();
    extern __shared__ __attribute__((aligned(16))) u64 behz_col[];  // [size_b + 1][256]
    const u32 N = 1u << A.log_n;
    const u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (u64)batch * N) return;
    const u32 b = (u32)(gid >> A.log_n), ri = (u32)(gid & (N - 1));
    const u64* xb = x + (u64)b * in_stride + ri;
    u64* col = behz_col + threadIdx.x;
    behz_floor_coeff<PT>(A, xb, xb + (u64)A.size_q * N, N, [&](u32 j, u64 v) { col[j * 256] = v; });
    for (u32 i = 0; i < A.size_b; i++)
        col[i * 256] = shoup_canon(col[i * 256], A.bhi[2 * i], A.bhi[2 * i + 1], A.bv[i]);
    behz_sk_coeff<PT>(A, [&](u32 i) { return col[i * 256]; }, col[A.size_b * 256], out + (u64)b * out_stride + ri, N);
}

}  // namespace ofhe
