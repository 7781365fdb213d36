// bfv_decrypt_kernels.hpp -- the two ends of a BFV computation on gfx950:
// decryption's ScaleAndRound to the plaintext modulus t and encryption's
// TimesQovert, bit-exact with the reference's NATIVEINT == 64 build.
//
//   DCRTPolyImpl::ScaleAndRound -> NativePoly, HPS family   dcrtpoly-impl.h:1537-1814
//   DCRTPolyImpl::ScaleAndRound -> NativePoly, BEHZ         dcrtpoly-impl.h:2005-2049
//   NativeVectorT::MultiplyAndRound + SwitchModulus (one tower)
//                                 mubintvecnat.cpp:420-435, ubintnat.h:536-540, bfvrns-pke.cpp:233-245
//   PKERNS::DecryptCore                                     rns-pke.cpp:199-224 (k_decrypt_core, bgv_decrypt_kernels.hpp)
//   DCRTPolyImpl::TimesQovert                               dcrtpoly-impl.h:1015-1031
//
// Floating-point contract (that of bfv_kernels.hpp: the reference uses double
// throughout, SSE2, no fused multiply-add).  With the eight loops of
// dcrtpoly-impl.h:1547-1803 labelled A-H as UnitTestBFVrnsDecrypt.cpp:126-148
// labels them:
//   * floatSum starts at 0.5 (t a power of two, A-D) or 0.0 (E-H).  For towers
//     i = 0, 1, ... in that order floatSum = floatSum + (double(x_i) * frac[i]);
//     in the split loops (C, D, G, H) this is done for lo = x_i - (hi << qMSBHf)
//     with frac[i], then for hi = x_i >> qMSBHf with fracB[i];
//   * A-D: out = (intSum + uint64(floatSum)) & (t - 1), intSum modulo 2^64 (the
//     exact products of A / C and the reduced ones of B / D are congruent mod t);
//   * E-H: intSum is the sum of the exact products (E, G) or of the products
//     reduced mod t (F, H; the two give different doubles), then
//       floatSum = floatSum + double(intSum);  quot = uint64(floatSum * tInv);
//       floatSum = floatSum - (td * double(quot));  out = uint64(floatSum + 0.5)
//     written as computed (it may equal t, as the reference's may);
//   * every multiply, add and subtract is rounded separately (fp_mul / fp_add /
//     nu_step), double(uint64) is u2d; nothing is fused or reordered;
//   * one tower: MR(y) = uint64(td * (double(y) / double(q)) + 0.5) with one
//     correctly rounded IEEE division (fp_div), multiply and add separate.
#pragma once
#include "bfv_kernels.hpp"
#include "bgv_decrypt_kernels.hpp"
#include "ntt_kernels.hpp"

namespace ofhe {

__device__ __forceinline__ double fp_div(double a, double b) {
#pragma clang fp contract(off)
    return a / b;
}

// NativeIntegerT::ModMulFastConst (ubintnat.h:1475-1480) for any a < 2^64,
// w < m < 2^63, wp = floor(w 2^64 / m): the exact quotient estimate is at most
// one short, so one conditional subtraction gives the canonical a w mod m.
__device__ __forceinline__ u64 shoup_exact(u64 a, u64 w, u64 wp, u64 m) {
    return csub(a * w - mulhi_exact(a, wp) * m, m);
}

// Towers whose words a thread requests before it consumes the first: the loads
// of a tile are in flight together (one thread per coefficient leaves only
// batch * N threads to hide the memory latency; DESIGN.md "BFV decryption").
constexpr int DEC_TILE = 8;

enum { DEC_A = 0, DEC_B, DEC_C, DEC_D, DEC_E, DEC_F, DEC_G, DEC_H };

struct DecArgs {
    const u64* qv;        // [size_q]
    const u64* w;         // [size_q][2]  HPS: tQHatInvModqDivqModt, precon mod t; BEHZ: tgammaQHatInvModq, precon mod q_i
    const u64* wb;        // [size_q][2]  HPS: tQHatInvModqBDivqModt, precon mod t; BEHZ: negInvqModtgamma, precon mod tgamma
    const double* frac;   // [size_q]     tQHatInvModqDivqFrac
    const double* fracb;  // [size_q]     tQHatInvModqBDivqFrac
    const u64* qmu;       // [size_q][2]  floor(2^128 / q_i)   (DecryptCore: CoreArgs)
    const u64* tiq;       // [size_q][2]  tInvModq, precon mod q_i (TimesQovert)
    u64 t, tgamma, nqt, nqt_pre;  // NegQModt and its precon mod t
    double td, tinv;
    u64 sw_q;   // one tower: q[0] and the SwitchModulus constants of q[0] -> t (arith.hpp's sw_mod, on the host)
    SwMod sw;
    u32 log_n, size_q, half;  // half = qMSBHf
};

// ---------------------------------------------------------------------------
// ScaleAndRound to t, HPS family: x [batch][size_q][N] -> out [batch][N].  One
// thread per (batch entry, coefficient) (grid_for's grid: a stride loop only
// past its cap), towers in order with a stride of N
// words, loaded in tiles of DEC_TILE; BR is the reference's loop (DEC_A .. DEC_H).
// ---------------------------------------------------------------------------
template <int BR>
__global__ __launch_bounds__(256) void k_dec_scale_round(DecArgs A, const u64* __restrict__ x, u64* __restrict__ out,
                                                         u32 batch) {
    OFHE_VGPR_FLOOR();
    constexpr bool POW2 = BR < DEC_E;
    constexpr bool SPLIT = (BR & 2) != 0;     // C, D, G, H
    constexpr bool REDUCED = (BR & 1) != 0;   // B, D, F, H
    const u32 N = 1u << A.log_n;
    const u64 total = (u64)batch << A.log_n, step = (u64)gridDim.x * blockDim.x;
    for (u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x; gid < total; gid += step) {
        const u32 b = (u32)(gid >> A.log_n), ri = (u32)(gid & (N - 1));
        const u64* xb = x + ((u64)b * A.size_q << A.log_n) + ri;
        double fs = POW2 ? 0.5 : 0.0;
        u64 is = 0;
        for (u32 i0 = 0; i0 < A.size_q; i0 += DEC_TILE) {
            // the tile's words are requested together; the chain then takes them in tower order
            u64 v[DEC_TILE];
#pragma unroll
            for (int k = 0; k < DEC_TILE; k++) v[k] = i0 + k < A.size_q ? ld_s(xb + (u64)(i0 + k) * N) : 0;
#pragma unroll
            for (int k = 0; k < DEC_TILE; k++) {
                const u32 i = i0 + k;
                if (i >= A.size_q) break;
                u64 lo = v[k];
                if (SPLIT) {
                    const u64 hi = lo >> A.half;
                    lo -= hi << A.half;
                    fs = nu_step(fs, u2d(lo), A.frac[i]);
                    fs = nu_step(fs, u2d(hi), A.fracb[i]);
                    // mod 2^64 the exact and the reduced products of A-D are the same word mod t
                    if (REDUCED && !POW2)
                        is += shoup_exact(lo, A.w[2 * i], A.w[2 * i + 1], A.t) +
                              shoup_exact(hi, A.wb[2 * i], A.wb[2 * i + 1], A.t);
                    else
                        is += lo * A.w[2 * i] + hi * A.wb[2 * i];
                } else {
                    fs = nu_step(fs, u2d(lo), A.frac[i]);
                    if (REDUCED && !POW2)
                        is += shoup_exact(lo, A.w[2 * i], A.w[2 * i + 1], A.t);
                    else
                        is += lo * A.w[2 * i];
                }
            }
        }
        u64 r;
        if (POW2) {
            r = (is + (u64)fs) & (A.t - 1);
        } else {
            fs = fp_add(fs, u2d(is));
            const u64 quot = (u64)fp_mul(fs, A.tinv);
            double p = fp_mul(A.td, u2d(quot));
            asm volatile("" : "+v"(p));
            fs = fp_add(fs, -p);
            r = (u64)fp_add(fs, 0.5);
        }
        st_s(out + gid, r);
    }
}

// ---------------------------------------------------------------------------
// ScaleAndRound to t, BEHZ (gamma = 2^26, integers only).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dec_scale_round_behz(DecArgs A, const u64* __restrict__ x,
                                                              u64* __restrict__ out, u32 batch) {
    OFHE_VGPR_FLOOR();
    const u32 N = 1u << A.log_n;
    const u64 total = (u64)batch << A.log_n, step = (u64)gridDim.x * blockDim.x;
    for (u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x; gid < total; gid += step) {
        const u32 b = (u32)(gid >> A.log_n), ri = (u32)(gid & (N - 1));
        const u64* xb = x + ((u64)b * A.size_q << A.log_n) + ri;
        u64 s = 0;
        for (u32 i0 = 0; i0 < A.size_q; i0 += DEC_TILE) {
            u64 v[DEC_TILE];
#pragma unroll
            for (int k = 0; k < DEC_TILE; k++) v[k] = i0 + k < A.size_q ? ld_s(xb + (u64)(i0 + k) * N) : 0;
#pragma unroll
            for (int k = 0; k < DEC_TILE; k++) {
                const u32 i = i0 + k;
                if (i >= A.size_q) break;
                const u64 y = shoup_exact(v[k], A.w[2 * i], A.w[2 * i + 1], A.qv[i]);
                s = csub(s + shoup_exact(y, A.wb[2 * i], A.wb[2 * i + 1], A.tgamma), A.tgamma);
            }
        }
        st_s(out + gid, (s + (s & ((1ull << 26) - 1))) >> 26);
    }
}

// ---------------------------------------------------------------------------
// One tower: MultiplyAndRound(t, q) then SwitchModulus(t) (bfvrns-pke.cpp:233-245).
// ---------------------------------------------------------------------------
__device__ __forceinline__ u64 mul_round1(u64 y, double td, double qd) {
    double d = fp_div(u2d(y), qd);
    asm volatile("" : "+v"(d));
    double p = fp_mul(td, d);
    asm volatile("" : "+v"(p));
    return (u64)fp_add(p, 0.5);
}

__global__ __launch_bounds__(256) void k_dec_one_tower(DecArgs A, const u64* __restrict__ x, u64* __restrict__ out,
                                                       u64 total) {
    OFHE_VGPR_FLOOR();
    const u64 step = (u64)gridDim.x * blockDim.x;
    const u64 q = A.sw_q;
    const double qd = u2d(q);
    for (u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x; gid < total; gid += step) {
        const u64 v = ld_s(x + gid);
        u64 r;
        if (v > (q >> 1)) {
            r = q - mul_round1(q - v, A.td, qd);
        } else {
            r = mul_round1(v, A.td, qd);
            if (r >= q) r = umod64(r, q);
        }
        st_s(out + gid, switch_mod1(r, A.sw));
    }
}

// ---------------------------------------------------------------------------
// TimesQovert: out_i = ((x_i NegQModt) mod t) tInvModq[i] mod q_i, one thread
// per word of [batch][size_q][N]; out may be x.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_times_q_over_t(DecArgs A, const u64* x, u64* out, u64 total) {
    OFHE_VGPR_FLOOR();
    const u64 step = (u64)gridDim.x * blockDim.x;
    for (u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x; gid < total; gid += step) {
        const u32 i = (u32)(gid >> A.log_n) % A.size_q;
        const u64 y = shoup_exact(x[gid], A.nqt, A.nqt_pre, A.t);
        out[gid] = shoup_exact(y, A.tiq[2 * i], A.tiq[2 * i + 1], A.qv[i]);
    }
}

}  // namespace ofhe
