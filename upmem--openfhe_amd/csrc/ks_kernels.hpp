// ks_kernels.hpp -- element kernels of ApproxModUp / ApproxModDown, the
// HYBRID key-switching inner product, SwitchModulus and automorphisms.
//
// All are HBM streams over [batch][towers][N] data with explicit batch
// strides (words), so they can address a tower range of a wider polynomial
// (the Q part of a Q|P polynomial, one digit slot of the key-switch digits)
// without copies.  Each thread handles two adjacent coefficients (16-byte
// accesses); N >= 2 keeps pairs inside one tower.
#pragma once
#include "eltwise_kernels.hpp"

namespace ofhe {

// one scalar per tower: s and its Shoup precon for modulus q
struct TowerScalar {
    u64 q, s, sp;
};
static_assert(sizeof(TowerScalar) == 24, "PlanArgs::scal reads TowerScalar as [towers][3] words");

// (pair index) -> (batch entry, tower, coefficient) for `towers` towers of N
struct PairIndex {
    u32 b, t, c;
};
__device__ __forceinline__ PairIndex pair_index(u64 i, u32 log_n, u32 towers) {
    const u64 e = 2 * i;
    const u32 row = (u32)(e >> log_n);  // batch * towers < 2^32 for any buffer that fits in HBM: 32-bit divide
    return PairIndex{row / towers, row % towers, (u32)(e & ((1ull << log_n) - 1))};
}

// out = x * s_t mod q_t (NativeVectorT::ModMulEq(scalar), mubintvecnat.cpp:310-332)
__global__ __launch_bounds__(256) void k_scale_towers(const TowerScalar* __restrict__ ts, const u64* x, u64* out,
                                                      u64 xstride, u64 ostride, u64 npairs, u32 log_n,
                                                      u32 towers) {
    OFHE_VGPR_FLOOR();
    const u64 step = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < npairs; i += step) {
        const PairIndex p = pair_index(i, log_n, towers);
        const TowerScalar c = ts[p.t];
        const u64 inner = ((u64)p.t << log_n) + p.c;
        const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(x + p.b * xstride + inner);
        *reinterpret_cast<ulonglong2*>(out + p.b * ostride + inner) =
            make_ulonglong2(shoup_canon(v.x, c.s, c.sp, c.q), shoup_canon(v.y, c.s, c.sp, c.q));
    }
}

// out = (x - y mod q_t) * s_t mod q_t: the last step of ApproxModDown,
// (m_vectors[i] - partPSwitchedToQ[i]) * PInvModq[i] (dcrtpoly-impl.h:1172).
__global__ __launch_bounds__(256) void k_sub_scale(const TowerScalar* __restrict__ ts, const u64* x, const u64* y,
                                                   u64* out, u64 xstride, u64 ystride, u64 ostride, u64 npairs,
                                                   u32 log_n, u32 towers) {
    OFHE_VGPR_FLOOR();
    const u64 step = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < npairs; i += step) {
        const PairIndex p = pair_index(i, log_n, towers);
        const TowerScalar c = ts[p.t];
        const u64 inner = ((u64)p.t << log_n) + p.c;
        const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(x + p.b * xstride + inner);
        const ulonglong2 b = *reinterpret_cast<const ulonglong2*>(y + p.b * ystride + inner);
        const u64 d0 = a.x < b.x ? a.x + c.q - b.x : a.x - b.x;  // ModSubFastEq
        const u64 d1 = a.y < b.y ? a.y + c.q - b.y : a.y - b.y;
        *reinterpret_cast<ulonglong2*>(out + p.b * ostride + inner) =
            make_ulonglong2(shoup_canon(d0, c.s, c.sp, c.q), shoup_canon(d1, c.s, c.sp, c.q));
    }
}

// k_sub_scale plus an addend laid out as out (ModAddFastEq): the
// relinearisation sums of base-leveledshe.cpp:352-360 in ApproxModDown's last
// step.  add may be out itself: a thread reads the words it writes, first.
__global__ __launch_bounds__(256) void k_sub_scale_add(const TowerScalar* __restrict__ ts, const u64* x, const u64* y,
                                                       const u64* add, u64* out, u64 xstride, u64 ystride,
                                                       u64 ostride, u64 npairs, u32 log_n, u32 towers) {
    OFHE_VGPR_FLOOR();
    const u64 step = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < npairs; i += step) {
        const PairIndex p = pair_index(i, log_n, towers);
        const TowerScalar c = ts[p.t];
        const u64 inner = ((u64)p.t << log_n) + p.c;
        const ulonglong2 a = *reinterpret_cast<const ulonglong2*>(x + p.b * xstride + inner);
        const ulonglong2 b = *reinterpret_cast<const ulonglong2*>(y + p.b * ystride + inner);
        const ulonglong2 e = *reinterpret_cast<const ulonglong2*>(add + p.b * ostride + inner);
        const u64 d0 = a.x < b.x ? a.x + c.q - b.x : a.x - b.x;  // ModSubFastEq
        const u64 d1 = a.y < b.y ? a.y + c.q - b.y : a.y - b.y;
        *reinterpret_cast<ulonglong2*>(out + p.b * ostride + inner) =
            make_ulonglong2(modadd_fast(e.x, shoup_canon(d0, c.s, c.sp, c.q), c.q),
                            modadd_fast(e.y, shoup_canon(d1, c.s, c.sp, c.q), c.q));
    }
}

// Tower of the extended basis Ql|P for the key-switch inner product.
struct KsTower {
    u64 m;                // modulus
    u64 mu_lo, mu_hi;     // floor(2^128 / m)
    u64 key_off;          // word offset of this tower inside one key polynomial (QP layout)
    u64 r60, r60p, mu1;   // limb_reduce constants
};

// EvalFastKeySwitchCoreExt (keyswitch-hybrid.cpp:452-478):
//   ct0[i] = sum_j digits_j[i] * b_j[key(i)],  ct1[i] = sum_j digits_j[i] * a_j[key(i)]
// The reference accumulates canonical ModMul / ModAdd terms; the sum of exact
// 128-bit products reduced once by BarrettUint128ModUint64 is the same
// canonical residue (beta <= 2^8 terms below 2^120 cannot overflow 128 bits).
__global__ __launch_bounds__(256) void k_ks_inner(const KsTower* __restrict__ tw, const u64* __restrict__ digits,
                                                  const u64* __restrict__ kb, const u64* __restrict__ ka,
                                                  u64* __restrict__ ct0, u64* __restrict__ ct1, u64 key_stride,
                                                  u32 beta, u64 npairs, u32 log_n, u32 towers) {
    OFHE_VGPR_FLOOR();
    const u64 step = (u64)gridDim.x * blockDim.x;
    const u64 poly = (u64)towers << log_n;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < npairs; i += step) {
        const PairIndex p = pair_index(i, log_n, towers);
        const KsTower T = tw[p.t];
        const u64 inner = ((u64)p.t << log_n) + p.c;
        const u64* d = digits + (u64)p.b * beta * poly + inner;
        const u64* pb = kb + T.key_off + p.c;
        const u64* pa = ka + T.key_off + p.c;
        u64 b0l = 0, b0h = 0, b1l = 0, b1h = 0, a0l = 0, a0h = 0, a1l = 0, a1h = 0;
        for (u32 j = 0; j < beta; j++) {
            const ulonglong2 x = *reinterpret_cast<const ulonglong2*>(d + (u64)j * poly);
            const ulonglong2 vb = *reinterpret_cast<const ulonglong2*>(pb + (u64)j * key_stride);
            const ulonglong2 va = *reinterpret_cast<const ulonglong2*>(pa + (u64)j * key_stride);
            u64 l, h;
            mul128(x.x, vb.x, l, h);
            b0l += l;
            b0h += h + (b0l < l);
            mul128(x.y, vb.y, l, h);
            b1l += l;
            b1h += h + (b1l < l);
            mul128(x.x, va.x, l, h);
            a0l += l;
            a0h += h + (a0l < l);
            mul128(x.y, va.y, l, h);
            a1l += l;
            a1h += h + (a1l < l);
        }
        const u64 o = (u64)p.b * poly + inner;
        *reinterpret_cast<ulonglong2*>(ct0 + o) = make_ulonglong2(barrett128(b0l, b0h, T.m, T.mu_lo, T.mu_hi),
                                                                  barrett128(b1l, b1h, T.m, T.mu_lo, T.mu_hi));
        *reinterpret_cast<ulonglong2*>(ct1 + o) = make_ulonglong2(barrett128(a0l, a0h, T.m, T.mu_lo, T.mu_hi),
                                                                  barrett128(a1l, a1h, T.m, T.mu_lo, T.mu_hi));
    }
}

// Same product, batch-stationary keys: a thread owns (tower, C coefficients)
// and walks the batch, so each key word is read once per launch instead of
// once per ciphertext.  Sums use the 30-bit limb split and limb_reduce of
// k_bconv_limb (beta <= 16 terms below 2^60 per limb sum).  BETA is the exact
// digit count (no masked slots), and the next ciphertext's digits are loaded
// before the current one is reduced, so one load latency hides behind a
// whole iteration of arithmetic.  C = 1 halves the per-thread state of C = 2
// (more waves in flight).  SQ counters (configs[4]): 149 VALU instructions per
// ciphertext per thread, two thirds of them limb_reduce, at ~66 % of the VALU
// issue peak; a two-deep prefetch (6 loads in flight) measured no gain.
#ifndef OFHE_KS_CPT
#define OFHE_KS_CPT 1
#endif
template <int C>
struct Words {
    u64 v[C];
};
template <int C>
__device__ __forceinline__ Words<C> ldw(const u64* p) {
    Words<C> w;
    if constexpr (C == 2) {
        const u64x2 t = ld2_s(p);
        w.v[0] = t.x;
        w.v[1] = t.y;
    } else {
        w.v[0] = ld_s(p);
    }
    return w;
}
template <int C>
__device__ __forceinline__ void stw(u64* p, const u64* v) {
    if constexpr (C == 2) {
        u64x2 t;
        t.x = v[0];
        t.y = v[1];
        st2_s(p, t);
    } else {
        st_s(p, v[0]);
    }
}

// Digit j's own towers [own.start[j], own.start[j] + own.cnt[j]) are the
// ciphertext's evaluation-form towers unchanged (keyswitch-hybrid.cpp:402-404);
// when `c` is given they are read from it (c: [batch][size_ql][N], stride
// c_stride) instead of from a copy in the digit slot, so KeySwitchCore skips
// writing and re-reading that copy.
struct KsOwn {
    u32 start[4], cnt[4];
};
template <int BETA, int C>
__global__ __launch_bounds__(256) void k_ks_inner_bs(const KsTower* __restrict__ tw, const u64* __restrict__ digits,
                                                     const u64* __restrict__ kb, const u64* __restrict__ ka,
                                                     u64* __restrict__ ct0, u64* __restrict__ ct1, u64 key_stride,
                                                     u32 batch, u64 nthreads, u32 log_n, u32 towers,
                                                     const u64* __restrict__ c_in, u64 c_stride, KsOwn own) {
    OFHE_VGPR_FLOOR();
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nthreads) return;
    const u64 e = C * i;
    const u32 t = (u32)(e >> log_n), c = (u32)(e & ((1ull << log_n) - 1));
    const KsTower T = tw[t];
    const LimbRed R{T.m, T.r60, T.r60p, T.mu1};
    const u64 poly = (u64)towers << log_n;
    const u64 inner = ((u64)t << log_n) + c;
    u64 kl[BETA][2 * C];  // (b[0..C), a[0..C)) as (lo30 | hi30 << 32)
#pragma unroll
    for (int j = 0; j < BETA; j++) {
        const u64 off = T.key_off + c + (u64)j * key_stride;
        const Words<C> vb = ldw<C>(kb + off), va = ldw<C>(ka + off);
#pragma unroll
        for (int k = 0; k < C; k++) {
            kl[j][k] = (vb.v[k] & LIMB_MASK) | ((vb.v[k] >> LIMB) << 32);
            kl[j][C + k] = (va.v[k] & LIMB_MASK) | ((va.v[k] >> LIMB) << 32);
        }
    }
    // one ciphertext: BETA digit words -> ct0/ct1 words of batch entry b
    auto one = [&](const Words<C> (&x)[BETA], u32 b) {
        u64 acc[2 * C][4];  // k < C: ct0 coefficient k; k >= C: ct1 coefficient k - C
#pragma unroll
        for (int k = 0; k < 2 * C; k++) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0;
#pragma unroll
        for (int j = 0; j < BETA; j++) {
#pragma unroll
            for (int k = 0; k < 2 * C; k++) {
                const u64 xv = x[j].v[k % C];
                const u32 x0 = (u32)(xv & LIMB_MASK), x1 = (u32)(xv >> LIMB);
                const u64 kw = kl[j][k];
                acc[k][0] = mad32(x0, lo32(kw), acc[k][0]);
                acc[k][1] = mad32(x0, hi32(kw), acc[k][1]);
                acc[k][2] = mad32(x1, lo32(kw), acc[k][2]);
                acc[k][3] = mad32(x1, hi32(kw), acc[k][3]);
            }
        }
        u64 r[2 * C];
#pragma unroll
        for (int k = 0; k < 2 * C; k++) r[k] = limb_reduce<false>(acc[k][0], acc[k][1], acc[k][2], acc[k][3], R);
        const u64 o = (u64)b * poly + inner;
        stw<C>(ct0 + o, r);
        stw<C>(ct1 + o, r + C);
    };
    auto load = [&](Words<C> (&x)[BETA], u32 b) {
        const u64* d = digits + (u64)b * BETA * poly + inner;
#pragma unroll
        for (int j = 0; j < BETA; j++) {
            const bool mine = c_in && t - own.start[j] < own.cnt[j];  // wave-uniform for N >= 64 C
            x[j] = ldw<C>(mine ? c_in + (u64)b * c_stride + inner : d + (u64)j * poly);
        }
    };
    Words<C> xn[BETA];
    load(xn, 0);
    for (u32 b = 0; b < batch; b++) {
        Words<C> x[BETA];
#pragma unroll
        for (int j = 0; j < BETA; j++) x[j] = xn[j];
        if (b + 1 < batch) load(xn, b + 1);
        one(x, b);
    }
}

// Hoisted rotations: LeveledSHECKKSRNS::EvalFastRotationExt
// (ckksrns-leveledshe.cpp:402-457) and the inner product of
// LeveledSHEBase::EvalFastRotation (base-leveledshe.cpp:471-513) for up to
// KS_ROT_CAP rotations of one digit set per launch.  The per-rotation key
// pointers and automorphism indices travel in the kernel arguments (nothing
// is staged); kinv[r] is the inverse of rotation r's index k modulo 2^32,
// hence modulo 2N.
constexpr u32 KS_ROT_CAP = 16;
struct KsRot {
    const u64* kb[KS_ROT_CAP];
    const u64* ka[KS_ROT_CAP];
    u32 kinv[KS_ROT_CAP];
};
struct KsRotIdx {
    u32 kinv[KS_ROT_CAP];
};

// AutomorphismTransform(k) in evaluation form (poly-impl.h:338-364) sets
// dst[rev(j)] = src[rev(j')] with 2 j' + 1 = k (2 j + 1) mod 2N.  A thread
// that holds the value of storage position s = rev(j') therefore writes it to
// rev(j) with 2 j + 1 = k^-1 (2 j' + 1) mod 2N (the product wraps mod 2^32,
// which 2N divides).  Aligned blocks of 2^m storage words map onto aligned
// blocks of 2^m words, so a wave's 64 stores fill whole 128-byte lines.
__device__ __forceinline__ u32 rot_dest(u32 s, u32 kinv, u32 log_n) {
    const u32 j = __builtin_bitreverse32(s) >> (32 - log_n);
    const u32 jk = kinv * (2 * j + 1);
    return __builtin_bitreverse32((jk >> 1) & ((1u << log_n) - 1)) >> (32 - log_n);
}

// Digit-stationary inner product: a thread owns one (batch entry, tower,
// storage position), loads and limb-splits its BETA digit words once and
// walks the rotations of the launch: per rotation it loads the 2 BETA key
// words (the next rotation's before the current one is reduced), accumulates
// the 30-bit limb sums of k_ks_inner_bs, reduces, adds c0 * (P mod q_t) on
// the Q towers when c0 is given (addFirst) and stores at the position the
// rotation's automorphism sends its word to.  Outputs: [nrot][batch][towers][N]
// with rot_stride words between rotations.  With kinv = 1 it is the plain
// multi-key inner product of the non-Ext path.  (An exchange of the
// workgroup's results through LDS, so that the stores leave in position
// order, measured the same as this scatter: DESIGN.md "Hoisted rotations".)
template <int BETA>
__global__ __launch_bounds__(256) void k_ks_inner_rot(const KsTower* __restrict__ tw, const u64* __restrict__ digits,
                                                      const u64* __restrict__ c0,
                                                      const TowerScalar* __restrict__ pmodq, KsRot rot, u32 nrot,
                                                      u64* __restrict__ out0, u64* __restrict__ out1, u64 key_stride,
                                                      u64 rot_stride, u64 nthreads, u32 log_n, u32 towers,
                                                      u32 size_ql) {
    OFHE_VGPR_FLOOR();
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nthreads) return;
    const u32 row = (u32)(i >> log_n), s = (u32)(i & ((1ull << log_n) - 1));
    const u32 b = row / towers, t = row % towers;
    const KsTower T = tw[t];
    const LimbRed R{T.m, T.r60, T.r60p, T.mu1};
    const u64 poly = (u64)towers << log_n;
    const u64 inner = (u64)t << log_n;
    u32 x0[BETA], x1[BETA];
#pragma unroll
    for (int j = 0; j < BETA; j++) {
        const u64 v = ld_s(digits + ((u64)b * BETA + j) * poly + inner + s);
        x0[j] = (u32)(v & LIMB_MASK);
        x1[j] = (u32)(v >> LIMB);
    }
    u64 add = 0;  // c0 * PModq on the Q towers (ckksrns-leveledshe.cpp:436-445)
    if (c0 && t < size_ql) {
        const TowerScalar ps = pmodq[t];
        add = shoup_canon(ld_s(c0 + (((u64)b * size_ql + t) << log_n) + s), ps.s, ps.sp, ps.q);
    }
    const u64 koff = T.key_off + s;
    u64 nb[BETA], na[BETA];
    auto load = [&](u32 r) {
        const u64* pb = rot.kb[r] + koff;
        const u64* pa = rot.ka[r] + koff;
#pragma unroll
        for (int j = 0; j < BETA; j++) {
            nb[j] = ld_s(pb + (u64)j * key_stride);
            na[j] = ld_s(pa + (u64)j * key_stride);
        }
    };
    load(0);
    for (u32 r = 0; r < nrot; r++) {
        u64 acc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
        for (int j = 0; j < BETA; j++) {
            const u64 w[2] = {nb[j], na[j]};
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const u32 w0 = (u32)(w[k] & LIMB_MASK), w1 = (u32)(w[k] >> LIMB);
                acc[k][0] = mad32(x0[j], w0, acc[k][0]);
                acc[k][1] = mad32(x0[j], w1, acc[k][1]);
                acc[k][2] = mad32(x1[j], w0, acc[k][2]);
                acc[k][3] = mad32(x1[j], w1, acc[k][3]);
            }
        }
        if (r + 1 < nrot) load(r + 1);
        const u64 r0 = csub(limb_reduce<false>(acc[0][0], acc[0][1], acc[0][2], acc[0][3], R) + add, T.m);
        const u64 r1 = limb_reduce<false>(acc[1][0], acc[1][1], acc[1][2], acc[1][3], R);
        const u64 o = (u64)r * rot_stride + (u64)b * poly + inner + rot_dest(s, rot.kinv[r], log_n);
        st_s(out0 + o, r0);
        st_s(out1 + o, r1);
    }
}

// The same for beta > 4: a runtime digit count, the digits re-read per
// rotation, exact 128-bit sums and barrett128 as in k_ks_inner.
__global__ __launch_bounds__(256) void k_ks_inner_rot_wide(const KsTower* __restrict__ tw,
                                                           const u64* __restrict__ digits,
                                                           const u64* __restrict__ c0,
                                                           const TowerScalar* __restrict__ pmodq, KsRot rot, u32 nrot,
                                                           u64* __restrict__ out0, u64* __restrict__ out1,
                                                           u64 key_stride, u64 rot_stride, u64 nthreads, u32 beta,
                                                           u32 log_n, u32 towers, u32 size_ql) {
    OFHE_VGPR_FLOOR();
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nthreads) return;
    const u32 row = (u32)(i >> log_n), s = (u32)(i & ((1ull << log_n) - 1));
    const u32 b = row / towers, t = row % towers;
    const KsTower T = tw[t];
    const u64 poly = (u64)towers << log_n;
    const u64 inner = (u64)t << log_n;
    const u64* d = digits + (u64)b * beta * poly + inner + s;
    u64 add = 0;
    if (c0 && t < size_ql) {
        const TowerScalar ps = pmodq[t];
        add = shoup_canon(ld_s(c0 + (((u64)b * size_ql + t) << log_n) + s), ps.s, ps.sp, ps.q);
    }
    const u64 koff = T.key_off + s;
    for (u32 r = 0; r < nrot; r++) {
        const u64* pb = rot.kb[r] + koff;
        const u64* pa = rot.ka[r] + koff;
        u64 bl = 0, bh = 0, al = 0, ah = 0;
        for (u32 j = 0; j < beta; j++) {
            const u64 x = d[(u64)j * poly];
            u64 l, h;
            mul128(x, ld_s(pb + (u64)j * key_stride), l, h);
            bl += l;
            bh += h + (bl < l);
            mul128(x, ld_s(pa + (u64)j * key_stride), l, h);
            al += l;
            ah += h + (al < l);
        }
        const u64 o = (u64)r * rot_stride + (u64)b * poly + inner + rot_dest(s, rot.kinv[r], log_n);
        st_s(out0 + o, csub(barrett128(bl, bh, T.m, T.mu_lo, T.mu_hi) + add, T.m));
        st_s(out1 + o, barrett128(al, ah, T.m, T.mu_lo, T.mu_hi));
    }
}

// Tail of EvalFastRotation (base-leveledshe.cpp:500-505) for the rotations of
// one launch (blockIdx.y): out0 = sigma_k(md0 + c0), out1 = sigma_k(md1) over
// [nrot][batch][towers][N]; md0, md1 are the two ModDown results, c0:
// [batch][towers][N], shared by the rotations.
__global__ __launch_bounds__(256) void k_add_automorphism(const KsTower* __restrict__ tw,
                                                          const u64* __restrict__ md0, const u64* __restrict__ md1,
                                                          const u64* __restrict__ c0, u64* __restrict__ out0,
                                                          u64* __restrict__ out1, KsRotIdx rot, u64 per_rot,
                                                          u32 log_n, u32 towers) {
    OFHE_VGPR_FLOOR();
    const u64 step = (u64)gridDim.x * blockDim.x;
    const u32 kinv = rot.kinv[blockIdx.y];
    const u64 base = (u64)blockIdx.y * per_rot;
    for (u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x; e < per_rot; e += step) {
        const u32 row = (u32)(e >> log_n), s = (u32)(e & ((1ull << log_n) - 1));
        const u64 m = tw[row % towers].m;
        const u64 o = base + ((u64)row << log_n) + rot_dest(s, kinv, log_n);
        st_s(out0 + o, csub(ld_s(md0 + base + e) + ld_s(c0 + e), m));
        st_s(out1 + o, ld_s(md1 + base + e));
    }
}

// NativeVectorT::SwitchModulus (mubintvecnat.cpp:111-136), value for value.
__global__ __launch_bounds__(256) void k_switch_modulus(const u64* src, u64* dst, u64 n, u64 om, u64 nm) {
    OFHE_VGPR_FLOOR();
    const u64 step = (u64)gridDim.x * blockDim.x;
    const u64 half = om >> 1;
    const bool up = nm > om;
    const u64 diff = up ? nm - om : nm - (om % nm);
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        u64 v = src[i];
        if (v > half) v += diff;
        if (!up && v >= nm) v %= nm;
        dst[i] = v;
    }
}

// Rescaling callers of SwitchModulus (dcrtpoly-impl.h:746-768 and 792-812):
// the dropped tower's coefficients v (canonical mod ql), optionally scaled
// first by pre (ModReduce's delta *= negtInvModq), are lifted into every
// remaining q_i and combined per tower with the scalars of tab[i] =
// (q_i, w_i, w_i', a_i, a_i', 0):
//   SW_SCALE  y = sw(v) w                   (evaluation form; the NTT and the
//                                            x a / (x - .) a step follow in
//                                            the fused forward-subtract pass)
//   SW_AXPY   y = x a + sw(v) w             (DropLastElementAndScale, coefficient form)
//   SW_XPYA   y = (x + sw(v) w) a           (ModReduce, coefficient form)
// one thread per (batch entry, tower, coefficient); canonical outputs.
enum { SW_SCALE = 0, SW_AXPY = 1, SW_XPYA = 2 };
struct SwArgs {
    const u64* last;  // [batch] rows of N (stride lstride)
    u64 lstride;
    const u64* x;     // [batch][towers][N] (stride xstride), SW_AXPY / SW_XPYA
    u64 xstride;
    u64* y;           // [batch][towers][N] (stride ystride)
    u64 ystride;
    const u64* tab;   // [towers][6]
    u64 ql, pre, pre_p;  // pre: scalar on v mod ql first (1: none)
    u32 log_n, towers;
};
// two coefficients per thread (16-byte accesses); w = 1 (DropLastElementAndScale
// with the reference's constants, where QlQlInvModqlDivqlModq = -qlInvModq)
// skips the multiply
template <int MODE>
__global__ __launch_bounds__(256) void k_switch_scale(SwArgs A, u32 bpr) {
    OFHE_VGPR_FLOOR();
    const u32 row = blockIdx.x / bpr, b = row / A.towers, t = row % A.towers;  // bpr blocks per row
    const u64 N = 1ull << A.log_n;
    const u64 j = 2 * ((u64)(blockIdx.x % bpr) * blockDim.x + threadIdx.x);
    if (j >= N) return;
    const u64* T = A.tab + 6 * (u64)t;
    const u64 q = T[0], w = T[1], wp = T[2], a = T[3], ap = T[4];
    const SwMod sm = sw_mod(A.ql, q);
    const ulonglong2 lv = *reinterpret_cast<const ulonglong2*>(A.last + b * A.lstride + j);
    u64 r[2] = {lv.x, lv.y};
    ulonglong2 xv = make_ulonglong2(0, 0);
    if (MODE != SW_SCALE) xv = *reinterpret_cast<const ulonglong2*>(A.x + b * A.xstride + (u64)t * N + j);
    const u64 xs[2] = {xv.x, xv.y};
#pragma unroll
    for (int k = 0; k < 2; k++) {
        u64 v = r[k];
        if (A.pre != 1) v = shoup_canon(v, A.pre, A.pre_p, A.ql);
        v = switch_mod1(v, sm);
        if (w != 1) v = shoup_canon(v, w, wp, q);
        if (MODE == SW_AXPY) v = csub(shoup_canon(xs[k], a, ap, q) + v, q);
        if (MODE == SW_XPYA) v = shoup_canon(csub(xs[k] + v, q), a, ap, q);
        r[k] = v;
    }
    st2_s(A.y + b * A.ystride + (u64)t * N + j, u64x2{r[0], r[1]});
}

// KeySwitchBV::EvalFastKeySwitchCore (keyswitch-bv.cpp:314-340):
//   ct0 = sum_i bv[i] . d_i,  ct1 = sum_i av[i] . d_i   (per tower, mod q_t)
// over `nd` digits.  One thread per (batch entry, tower, coefficient): the
// products are summed exactly in 128 bits (nd <= 256 terms below 2^120) and
// reduced once (BarrettUint128ModUint64, utilities-int.h:61-103) -- the
// canonical residue the reference's per-term ModMul / ModAdd chain ends on.
struct BvArgs {
    const u64* d;     // [batch][nd][towers][N]
    const u64* kb;    // [nd][key_towers][N]
    const u64* ka;
    u64* o0;          // [batch][towers][N]
    u64* o1;
    const u64* mu;    // [towers][3]: q, floor(2^128 / q) lo, hi
    u32 nd, towers, key_towers, log_n;
};
__global__ __launch_bounds__(256) void k_bv_inner(BvArgs A, u32 bpr) {
    OFHE_VGPR_FLOOR();
    const u32 row = blockIdx.x / bpr, b = row / A.towers, t = row % A.towers;
    const u64 N = 1ull << A.log_n;
    const u64 j = (u64)(blockIdx.x % bpr) * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const u64 dstep = (u64)A.towers * N, kstep = (u64)A.key_towers * N;
    const u64* dp = A.d + (u64)b * A.nd * dstep + (u64)t * N + j;
    const u64* bp = A.kb + (u64)t * N + j;
    const u64* ap = A.ka + (u64)t * N + j;
    u64 l0 = 0, h0 = 0, l1 = 0, h1 = 0;
    for (u32 i = 0; i < A.nd; i++) {
        const u64 dv = ld_s(dp + i * dstep);
        u64 lo, hi;
        mul128(bp[i * kstep], dv, lo, hi);
        l0 += lo;
        h0 += hi + (l0 < lo);
        mul128(ap[i * kstep], dv, lo, hi);
        l1 += lo;
        h1 += hi + (l1 < lo);
    }
    const u64 q = A.mu[3 * t], ml = A.mu[3 * t + 1], mh = A.mu[3 * t + 2];
    const u64 o = (u64)b * A.towers * N + (u64)t * N + j;
    st_s(A.o0 + o, barrett128(l0, h0, q, ml, mh));
    st_s(A.o1 + o, barrett128(l1, h1, q, ml, mh));
}

// PolyImpl::BaseDecompose (poly-impl.h:516-542) for CRTDecompose(r), r > 0
// (dcrtpoly-impl.h:290-320): windows j0 .. j0 + nw - 1 of one source tower's
// coefficients, win_j[x] = (coef[x] >> (j r)) & (2^r - 1), written as rows
// [batch][nw][N].  One thread per (batch entry, coefficient pair): the pair is
// loaded once and every window of it stored (16-byte accesses); j r < 60 for
// every window of a modulus below 2^60, so the shifts are defined.
struct BvWinArgs {
    const u64* coef;  // [batch] rows of N (stride cstride): the source tower, coefficient form
    u64 cstride;
    u64* win;         // [batch][nw][N]
    u32 r, j0, nw, log_n;
};
__global__ __launch_bounds__(256) void k_bv_windows(BvWinArgs A, u32 bpr) {
    OFHE_VGPR_FLOOR();
    const u32 b = blockIdx.x / bpr;
    const u64 N = 1ull << A.log_n;
    const u64 j = 2 * ((u64)(blockIdx.x % bpr) * blockDim.x + threadIdx.x);
    if (j >= N) return;
    const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(A.coef + b * A.cstride + j);
    const u64 mask = (1ull << A.r) - 1;
    u64* w = A.win + (u64)b * A.nw * N + j;
    for (u32 k = 0; k < A.nw; k++) {
        const u32 sh = (A.j0 + k) * A.r;
        st2_s(w + (u64)k * N, u64x2{(v.x >> sh) & mask, (v.y >> sh) & mask});
    }
}

// EvalFastKeySwitchCore over any number of digits (digitSize > 0: nd is the
// number of windows, not of towers) and KeySwitchInPlace's additions
// (keyswitch-bv.cpp:283-300): o = acc + sum_i key[i] . d_i, acc canonical and
// laid out as o (possibly o itself) or NULL for zero.  acc enters the 128-bit
// sum before the one reduction; the sum is folded to its residue every
// BV_FOLD terms (a residue and 256 products of words below 2^60 stay below
// 2^128), so nd is unbounded and the canonical result does not depend on the
// grouping.  NB > 1 keeps the key words stationary: a thread holds the
// accumulators of NB consecutive batch entries and loads each (key_b, key_a)
// word pair once for all of them.
constexpr u32 BV_FOLD = 256;
struct BvDigitArgs {
    BvArgs a;
    const u64* acc0;  // [batch][towers][N] or NULL
    const u64* acc1;
    u32 batch;
};
template <int NB>
__global__ __launch_bounds__(256) void k_bv_inner_digits(BvDigitArgs D, u32 bpr) {
    OFHE_VGPR_FLOOR();
    const BvArgs& A = D.a;
    const u32 row = blockIdx.x / bpr, g = row / A.towers, t = row % A.towers;
    const u64 N = 1ull << A.log_n;
    const u64 j = (u64)(blockIdx.x % bpr) * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const u32 b0 = g * NB;
    const u32 nb = D.batch - b0 < (u32)NB ? D.batch - b0 : (u32)NB;  // the last group may be short
    const u64 dstep = (u64)A.towers * N, kstep = (u64)A.key_towers * N, bstep = (u64)A.nd * dstep;
    const u64 o = (u64)b0 * dstep + (u64)t * N + j;
    const u64* dp = A.d + (u64)b0 * bstep + (u64)t * N + j;
    const u64* bp = A.kb + (u64)t * N + j;
    const u64* ap = A.ka + (u64)t * N + j;
    const u64 q = A.mu[3 * t], ml = A.mu[3 * t + 1], mh = A.mu[3 * t + 2];
    u64 l0[NB], h0[NB], l1[NB], h1[NB];
#pragma unroll
    for (int k = 0; k < NB; k++) {
        const bool on = (u32)k < nb;
        l0[k] = on && D.acc0 ? ld_s(D.acc0 + o + k * dstep) : 0;
        l1[k] = on && D.acc1 ? ld_s(D.acc1 + o + k * dstep) : 0;
        h0[k] = h1[k] = 0;
    }
    for (u32 i0 = 0; i0 < A.nd; i0 += BV_FOLD) {
        const u32 i1 = A.nd - i0 < BV_FOLD ? A.nd : i0 + BV_FOLD;
        if (i0) {
#pragma unroll
            for (int k = 0; k < NB; k++) {
                l0[k] = barrett128(l0[k], h0[k], q, ml, mh);
                l1[k] = barrett128(l1[k], h1[k], q, ml, mh);
                h0[k] = h1[k] = 0;
            }
        }
        for (u32 i = i0; i < i1; i++) {
            const u64 kbv = bp[i * kstep], kav = ap[i * kstep];
#pragma unroll
            for (int k = 0; k < NB; k++) {
                if ((u32)k >= nb) break;
                const u64 dv = ld_s(dp + k * bstep + i * dstep);
                u64 lo, hi;
                mul128(kbv, dv, lo, hi);
                l0[k] += lo;
                h0[k] += hi + (l0[k] < lo);
                mul128(kav, dv, lo, hi);
                l1[k] += lo;
                h1[k] += hi + (l1[k] < lo);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NB; k++) {
        if ((u32)k >= nb) break;
        st_s(A.o0 + o + k * dstep, barrett128(l0[k], h0[k], q, ml, mh));
        st_s(A.o1 + o + k * dstep, barrett128(l1[k], h1[k], q, ml, mh));
    }
}

// PolyImpl::AutomorphismTransform(k) (poly-impl.h:338-364).  One thread per
// index j of one (batch, tower) row:
//   evaluation form:  dst[rev(j)] = src[rev(((k (2j+1)) >> 1) mod n)]
//   coefficient form: dst[(j k) mod n] = bit_logn(j k) ? q - src[j] : src[j]
// (products taken mod 2n, which is what the reference's wrapping uint32
// arithmetic keeps, 2n dividing 2^32).
template <bool EVAL>
__global__ __launch_bounds__(256) void k_automorphism(const TowerConst* __restrict__ tcs, const u64* src, u64* dst,
                                                      u32 k, u64 total, u32 log_n, u32 towers) {
    OFHE_VGPR_FLOOR();
    const u64 step = (u64)gridDim.x * blockDim.x;
    const u64 n = 1ull << log_n, mask = n - 1, m2 = 2 * n - 1;
    for (u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
        const u64 row = e >> log_n;
        const u64 j = e & mask;
        const u64 base = row << log_n;
        if (EVAL) {
            const u64 jk = ((u64)k * (2 * j + 1)) & m2;
            const u32 jrev = __builtin_bitreverse32((u32)j) >> (32 - log_n);
            const u32 irev = __builtin_bitreverse32((u32)((jk >> 1) & mask)) >> (32 - log_n);
            dst[base + jrev] = src[base + irev];
        } else {
            const u64 q = tcs[(u32)row % towers].q;
            const u64 jk = ((u64)k * j) & m2;
            const u64 v = src[base + j];
            dst[base + (jk & mask)] = ((jk >> log_n) & 1) ? q - v : v;
        }
    }
}

}  // namespace ofhe
