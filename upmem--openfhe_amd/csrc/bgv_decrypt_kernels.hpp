// bgv_decrypt_kernels.hpp -- the last step of a BGV / CKKS computation on
// gfx950: PKERNS::DecryptCore and the chain of ModReduce steps Q_l -> q_0 that
// PKEBGVRNS::Decrypt runs, bit-exact with the reference's NATIVEINT == 64
// build.  Integers only.
//
//   PKERNS::DecryptCore                         rns-pke.cpp:199-224
//   PKEBGVRNS::Decrypt                          bgvrns-pke.cpp:44-99
//   DCRTPolyImpl::ModReduce                     dcrtpoly-impl.h:792-812
//   NativeVectorT::SwitchModulus                mubintvecnat.cpp:111-136
//   NativeVectorT::Mod / ModByTwoEq             mubintvecnat.cpp:139-166, 379-384
//   PolyImpl::DecryptionCRTInterpolate          poly-impl.h:566-575
#pragma once
#include "ntt_kernels.hpp"

namespace ofhe {

// ---------------------------------------------------------------------------
// DecryptCore: b = c0 + c1 s (+ c2 s^2), towerwise, canonical.  c*: [batch]
// [size_q][N], s: [>= size_q][N] of which the first size_q towers are read (the
// reference's DropLastElements, rns-pke.cpp:205-208), all in evaluation form;
// one thread per word.  out may be c0: a thread reads its word of c0 before it
// writes the same word of out, and no other thread touches it.
// ---------------------------------------------------------------------------
struct CoreArgs {
    const u64* qv;   // [size_q]
    const u64* qmu;  // [size_q][2]  floor(2^128 / q_i)
    u32 log_n, size_q;
};
template <bool THREE>
__global__ __launch_bounds__(256) void k_decrypt_core(CoreArgs A, const u64* c0, const u64* __restrict__ c1,
                                                      const u64* __restrict__ c2, const u64* __restrict__ s, u64* out,
                                                      u64 total) {
    OFHE_VGPR_FLOOR();
    const u64 step = (u64)gridDim.x * blockDim.x;
    for (u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x; gid < total; gid += step) {
        const u32 row = (u32)(gid >> A.log_n), i = row % A.size_q;
        const u64 q = A.qv[i], m0 = A.qmu[2 * i], m1 = A.qmu[2 * i + 1];
        const u64 sv = s[((u64)i << A.log_n) + (gid & ((1ull << A.log_n) - 1))];
        u64 lo, hi;
        mul128(ld_s(c1 + gid), sv, lo, hi);
        u64 acc = csub(ld_s(c0 + gid) + barrett128(lo, hi, q, m0, m1), q);
        if (THREE) {
            mul128(sv, sv, lo, hi);
            const u64 s2 = barrett128(lo, hi, q, m0, m1);
            mul128(ld_s(c2 + gid), s2, lo, hi);
            acc = csub(acc + barrett128(lo, hi, q, m0, m1), q);
        }
        st_s(out + gid, acc);
    }
}

// ---------------------------------------------------------------------------
// The reduction chain.  For one coefficient with residues x_0 .. x_l the
// reference runs, for j = l down to 1 (ModReduce in coefficient form),
//   delta = x_j negtInvModq[j] mod q_j
//   x_i   = (x_i + SwitchModulus(delta, q_j -> q_i) t mod q_i) qlInvModq[j][i] mod q_i     i < j
// with canonical words at every step.  Every step is a ring identity mod q_i,
// so the canonical x_i it ends on does not depend on how the intermediate
// words are represented; the kernel uses that twice:
//   * (x + d t) a = x a + d (t a): the two fixed multipliers a = qlInvModq[j][i]
//     and ta = (t mod q_i) a mod q_i are preconditioned (Shoup) on the host, the
//     two lazy products are summed in one multiply-add chain (shoup_lazy_acc)
//     and the sum, below 8 q_i < 2^63, is the next step's x_i as it stands.
//     A word is made canonical only where the reference's value is observed:
//     delta (SwitchModulus compares it with q_j >> 1) and the words written out;
//   * SwitchModulus's result is only ever multiplied mod q_i, and shoup_lazy
//     takes any 64-bit word, so its remainder is never formed: the lift is
//     d = delta > (q_j >> 1) ? delta + diff : delta with the reference's own
//     diff of either branch (q_i - q_j when q_i > q_j, else q_i - q_j mod q_i),
//     d < q_j + q_i < 2^61, congruent mod q_i to the reference's word.
// gfx950 has no 64-bit multiplier; a step is 18 32-bit multiplies.
//
// One thread per (batch entry, coefficient).  A launch reads `live` towers,
// retires the top k <= BGV_CHAIN_K of them and writes the `live - k` that are
// left: x [batch][live][N] -> out [batch][live - k][N].  The k retired residues
// sit in registers, statically indexed (the triangle among them is unrolled,
// guarded by the wave-uniform k), and become their deltas in place; the lower
// towers then stream through one at a time, each taking its k steps, the next
// tower's word requested before the current one's steps.  All constants are
// read with wave-uniform indices (scalar loads).  `plain` (only with live - k
// == 1) applies NativeVectorT::Mod(t) to the one word left.
// ---------------------------------------------------------------------------
constexpr int BGV_CHAIN_K = 8;  // DESIGN.md "BGV decryption": where the cap is and why

enum { BGV_MT_TWO = 0, BGV_MT_UP = 1, BGV_MT_DOWN = 2 };  // NativeVectorT::Mod: t == 2, t > q_0, t <= q_0
enum { BGV_TW = 4, BGV_PW = 6 };                          // words per tower row, per pair row

struct ChainArgs {
    const u64* tw;  // [size_q][4]   q_i, 2^64 - q_i, negtInvModq[i] and its precon mod q_i
    const u64* pw;  // [j (j - 1) / 2 + i][6], i < j:  a, a', ta, ta', diff(q_j -> q_i), 0
    u64 t, mt_diff;  // Mod t on tower 0: t - q_0 (t > q_0) or t - q_0 mod t
    u32 mt_mode, log_n;
};

// one ModReduce step of x (any word congruent to x_i, below 2^64) by the canonical delta of tower j
__device__ __forceinline__ u64 chain_step(u64 x, u64 delta, u64 half_j, const u64* __restrict__ P,
                                          const Mod<false>& M) {
    const u64 d = delta > half_j ? delta + P[4] : delta;
    return shoup_lazy_acc(x, P[0], P[1], M, shoup_lazy(d, P[2], P[3], M));
}
__device__ __forceinline__ Mod<false> chain_mod(const u64* __restrict__ T) {
    return Mod<false>{T[0], 0, 0, T[1], 0, 0, 0};
}
// NativeVectorT::Mod(t) of a canonical word mod q_0 (mubintvecnat.cpp:139-166; t == 2: ModByTwoEq, 379-384)
__device__ __forceinline__ u64 mod_t1(u64 v, u64 half, const ChainArgs& A) {
    if (A.mt_mode == BGV_MT_TWO) return 1 & (v ^ (u64)(v > half));
    if (v > half) v += A.mt_diff;
    if (A.mt_mode == BGV_MT_DOWN && v >= A.t) v = umod64(v, A.t);
    return v;
}

template <int KT>
__global__ __launch_bounds__(256) void k_bgv_chain(ChainArgs A, const u64* __restrict__ x, u64* __restrict__ out,
                                                   u32 live, u32 k, u32 plain, u32 batch) {
    OFHE_VGPR_FLOOR();
    const u32 N = 1u << A.log_n, base = live - k;  // base: the towers left, >= 1
    const u64 total = (u64)batch << A.log_n, step = (u64)gridDim.x * blockDim.x;
    for (u64 gid = (u64)blockIdx.x * blockDim.x + threadIdx.x; gid < total; gid += step) {
        const u32 b = (u32)(gid >> A.log_n), ri = (u32)(gid & (N - 1));
        const u64* xb = x + ((u64)b * live << A.log_n) + ri;
        u64 e[KT];  // e[m]: tower base + m, then its delta
#pragma unroll
        for (int m = 0; m < KT; m++) e[m] = (u32)m < k ? ld_s(xb + (u64)(base + m) * N) : 0;
        u64 nx = ld_s(xb);
#pragma unroll
        for (int m = KT - 1; m >= 0; m--) {
            if ((u32)m >= k) continue;
            const u32 j = base + m;
            const u64* Tj = A.tw + BGV_TW * (u64)j;
            const u64 qj = Tj[0], d = shoup_canon(e[m], Tj[2], Tj[3], qj);
            e[m] = d;
            const u64* Pj = A.pw + BGV_PW * ((u64)j * (j - 1) / 2 + base);
#pragma unroll
            for (int m2 = 0; m2 < m; m2++)
                e[m2] = chain_step(e[m2], d, qj >> 1, Pj + BGV_PW * m2, chain_mod(A.tw + BGV_TW * (u64)(base + m2)));
        }
        u64* ob = out + ((u64)b * base << A.log_n) + ri;
        for (u32 i = 0; i < base; i++) {
            u64 v = nx;
            if (i + 1 < base) nx = ld_s(xb + (u64)(i + 1) * N);
            const u64* Ti = A.tw + BGV_TW * (u64)i;
            const Mod<false> M = chain_mod(Ti);
#pragma unroll
            for (int m = KT - 1; m >= 0; m--) {
                if ((u32)m >= k) continue;
                const u32 j = base + m;
                v = chain_step(v, e[m], A.tw[BGV_TW * (u64)j] >> 1, A.pw + BGV_PW * ((u64)j * (j - 1) / 2 + i), M);
            }
            const u64 q = Ti[0];
            v = csub(csub(csub(v, 4 * q), 2 * q), q);
            if (plain) v = mod_t1(v, q >> 1, A);
            st_s(ob + (u64)i * N, v);
        }
    }
}

}  // namespace ofhe
