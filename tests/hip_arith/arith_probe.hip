// arith_probe.hip -- runs the library's lazy-reduction helpers on the device,
// one helper per invocation, on operand tuples read from a file.
//
//   arith_probe_bin <helper> <operands.bin> <results.bin>
//
// The helpers are the ones in csrc/arith.hpp, at the top of
// csrc/ntt_kernels.hpp and bm_reduce of csrc/bconv_mma.hpp, included unchanged;
// nothing of the library is linked.  tests/test_gpu_arith.py writes the
// operands, runs this program and compares every word with Python integers.
//
// operands.bin (u64 words): MAGIC, groups; then per group K[8] (wave-uniform
// constants: they travel as kernel arguments, one launch per group), n, and
// n tuples of IN words.  results.bin: n tuples of OUT words per group, in
// order.  Thread i of a launch reads tuple i and writes result i -- no index
// depends on data.  Every HIP call is checked; any error is a non-zero exit.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../upmem--openfhe_amd/csrc/bconv_mma.hpp"

using namespace ofhe;

#define CHK(x)                                                                              \
    do {                                                                                    \
        hipError_t e_ = (x);                                                                \
        if (e_ != hipSuccess) {                                                             \
            std::fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            std::exit(2);                                                                   \
        }                                                                                   \
    } while (0)

static const u64 MAGIC = 0x54495241454846ull;  // "FHEARIT"

struct Consts {
    u64 k[8];
};

// K = (q, L - 32 or 0, 1, ...): the constants load_mod() builds from TowerConst
template <bool SPQ, bool QA = false>
__device__ __forceinline__ Mod<SPQ, QA> mk_mod(const Consts& K) {
    const u64 q = K.k[0];
    return Mod<SPQ, QA>{q, 4 * q, 8 * q, 0 - q, 0 - 4 * q, 0 - 8 * q, (u32)K.k[1], (u32)K.k[2]};
}

// one functor per helper: IN operand words, OUT result words
template <bool QA>
struct HMulhiApprox {
    static constexpr int IN = 2, OUT = 1;
    static __device__ void run(const Consts& K, const u64* a, u64* r) { r[0] = mulhi_approx<QA>(a[0], a[1], (u32)K.k[2]); }
};
struct HMulhiExact {
    static constexpr int IN = 2, OUT = 1;
    static __device__ void run(const Consts&, const u64* a, u64* r) { r[0] = mulhi_exact(a[0], a[1]); }
};
struct HMul128 {
    static constexpr int IN = 2, OUT = 2;
    static __device__ void run(const Consts&, const u64* a, u64* r) { mul128(a[0], a[1], r[0], r[1]); }
};
struct HCsub {
    static constexpr int IN = 2, OUT = 1;
    static __device__ void run(const Consts&, const u64* a, u64* r) { r[0] = csub(a[0], a[1]); }
};
struct HCsubS {  // K[0] = m (wave-uniform)
    static constexpr int IN = 1, OUT = 1;
    static __device__ void run(const Consts& K, const u64* a, u64* r) { r[0] = csub_s(a[0], K.k[0]); }
};
template <bool SPQ, bool QA = false>
struct HShoup {  // (a, w, w')
    static constexpr int IN = 3, OUT = 1;
    static __device__ void run(const Consts& K, const u64* a, u64* r) { r[0] = shoup_lazy(a[0], a[1], a[2], mk_mod<SPQ, QA>(K)); }
};
template <bool SPQ>
struct HShoupAcc {  // (a, w, w', acc)
    static constexpr int IN = 4, OUT = 1;
    static __device__ void run(const Consts& K, const u64* a, u64* r) {
        r[0] = shoup_lazy_acc(a[0], a[1], a[2], mk_mod<SPQ>(K), a[3]);
    }
};
// single-operand reductions, K[3] selects
enum { R_FOLD, R_CANON_SPQ, R_CANON4, R_CANON8, R_CANON_FWD, R_RED8, R_RED16, R_RED16_GS };
template <int WHICH, bool SPQ>
struct HRed {
    static constexpr int IN = 1, OUT = 1;
    static __device__ void run(const Consts& K, const u64* a, u64* r) {
        const Mod<SPQ> M = mk_mod<SPQ>(K);
        const u64 x = a[0];
        r[0] = WHICH == R_FOLD        ? fold_spq(x, M)
               : WHICH == R_CANON_SPQ ? canon_spq(x, M)
               : WHICH == R_CANON4    ? canon4(x, M.q)
               : WHICH == R_CANON8    ? canon8(x, M.q)
               : WHICH == R_CANON_FWD ? canon_fwd(x, M)
               : WHICH == R_RED8      ? red8(x, M)
               : WHICH == R_RED16     ? red16(x, M)
                                      : red16_gs(x, M);
    }
};
template <bool SPQ>
struct HCtBfly {  // (x, y, w, w'), K[3] = cs
    static constexpr int IN = 4, OUT = 2;
    static __device__ void run(const Consts& K, const u64* a, u64* r) {
        u64 x = a[0], y = a[1];
        ct_bfly_cs(x, y, Tw{a[2], a[3]}, mk_mod<SPQ>(K), K.k[3] != 0);
        r[0] = x;
        r[1] = y;
    }
};
template <bool SPQ>
struct HGsBfly {
    static constexpr int IN = 4, OUT = 2;
    static __device__ void run(const Consts& K, const u64* a, u64* r) {
        u64 x = a[0], y = a[1];
        gs_bfly(x, y, Tw{a[2], a[3]}, mk_mod<SPQ>(K));
        r[0] = x;
        r[1] = y;
    }
};
struct HBarrettRef {  // K = (q, -, -, mu, nshift)
    static constexpr int IN = 2, OUT = 1;
    static __device__ void run(const Consts& K, const u64* a, u64* r) { r[0] = barrett_ref(a[0], a[1], K.k[0], K.k[3], (u32)K.k[4]); }
};
template <bool V2>
struct HMont {  // K = (q, -, -, qinv)
    static constexpr int IN = 2, OUT = 1;
    static __device__ void run(const Consts& K, const u64* a, u64* r) {
        r[0] = V2 ? mont_mul2(a[0], a[1], K.k[0], K.k[3]) : mont_mul(a[0], a[1], K.k[0], K.k[3]);
    }
};
struct HBarrett128 {  // (lo, hi), K = (m, -, -, mu_lo, mu_hi)
    static constexpr int IN = 2, OUT = 1;
    static __device__ void run(const Consts& K, const u64* a, u64* r) { r[0] = barrett128(a[0], a[1], K.k[0], K.k[3], K.k[4]); }
};
struct HSwitchMod {  // K = (old modulus, new modulus)
    static constexpr int IN = 1, OUT = 1;
    static __device__ void run(const Consts& K, const u64* a, u64* r) { r[0] = switch_mod1(a[0], sw_mod(K.k[0], K.k[1])); }
};
template <bool LAZY, bool SPQ, bool WIDE>
struct HBmReduce {  // eight partial sums (int32, sign-extended words), K = BmRed
    static constexpr int IN = 8, OUT = 1;
    static __device__ void run(const Consts& K, const u64* a, u64* r) {
        int C[8];
        for (int b = 0; b < 8; b++) C[b] = (int)(long long)a[b];
        const BmRed R{K.k[0], K.k[1], K.k[2], K.k[3], K.k[4], K.k[5], K.k[6], K.k[7]};
        r[0] = bm_reduce<LAZY, SPQ, WIDE>(C, R, bm_weights());
    }
};

template <class H>
__global__ __launch_bounds__(256) void k_probe(Consts K, const u64* __restrict__ in, u64* __restrict__ out, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 a[H::IN], r[H::OUT];
    for (int k = 0; k < H::IN; k++) a[k] = in[(size_t)i * H::IN + k];
    H::run(K, a, r);
    for (int k = 0; k < H::OUT; k++) out[(size_t)i * H::OUT + k] = r[k];
}

template <class H>
static void launch(const Consts& K, const u64* in, u64* out, u32 n) {
    hipLaunchKernelGGL(k_probe<H>, dim3((n + 255) / 256), dim3(256), 0, 0, K, in, out, n);
}

struct Entry {
    const char* name;
    int in, out;
    void (*launch)(const Consts&, const u64*, u64*, u32);
};
#define E(name, ...) {name, __VA_ARGS__::IN, __VA_ARGS__::OUT, &launch<__VA_ARGS__>}
static const Entry kTable[] = {
    E("mulhi_approx", HMulhiApprox<false>),
    E("mulhi_approx_qa", HMulhiApprox<true>),  // not on the shipped path (every kernel uses Mod<SPQ, false>)
    E("mulhi_exact", HMulhiExact),
    E("mul128", HMul128),
    E("csub", HCsub),
    E("csub_s", HCsubS),
    E("shoup_lazy", HShoup<false>),
    E("shoup_lazy_spq", HShoup<true>),
    E("shoup_lazy_qa", HShoup<false, true>),      // not on the shipped path
    E("shoup_lazy_spq_qa", HShoup<true, true>),   // not on the shipped path
    E("shoup_lazy_acc", HShoupAcc<false>),
    E("shoup_lazy_acc_spq", HShoupAcc<true>),
    E("fold_spq", HRed<R_FOLD, true>),
    E("canon_spq", HRed<R_CANON_SPQ, true>),
    E("canon4", HRed<R_CANON4, false>),
    E("canon8", HRed<R_CANON8, false>),
    E("canon_fwd", HRed<R_CANON_FWD, false>),
    E("canon_fwd_spq", HRed<R_CANON_FWD, true>),
    E("red8", HRed<R_RED8, false>),
    E("red8_spq", HRed<R_RED8, true>),
    E("red16", HRed<R_RED16, false>),
    E("red16_spq", HRed<R_RED16, true>),
    E("red16_gs", HRed<R_RED16_GS, false>),
    E("red16_gs_spq", HRed<R_RED16_GS, true>),
    E("ct_bfly_cs", HCtBfly<false>),
    E("ct_bfly_cs_spq", HCtBfly<true>),
    E("gs_bfly", HGsBfly<false>),
    E("gs_bfly_spq", HGsBfly<true>),
    E("barrett_ref", HBarrettRef),
    E("mont_mul", HMont<false>),
    E("mont_mul2", HMont<true>),  // not on the shipped path (mont_mul is the one kernels call)
    E("barrett128", HBarrett128),
    E("switch_mod1", HSwitchMod),
    E("bm_reduce", HBmReduce<false, false, false>),
    E("bm_reduce_wide", HBmReduce<false, false, true>),
    E("bm_reduce_spq", HBmReduce<false, true, false>),
    E("bm_reduce_spq_wide", HBmReduce<false, true, true>),
    E("bm_reduce_lazy", HBmReduce<true, false, false>),
    E("bm_reduce_lazy_wide", HBmReduce<true, false, true>),
    E("bm_reduce_lazy_spq", HBmReduce<true, true, false>),
    E("bm_reduce_lazy_spq_wide", HBmReduce<true, true, true>),
};

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--list")) {
        for (const Entry& e : kTable) std::printf("%s %d %d\n", e.name, e.in, e.out);
        return 0;
    }
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s <helper> <operands.bin> <results.bin> | --list\n", argv[0]);
        return 1;
    }
    const Entry* ent = nullptr;
    for (const Entry& e : kTable)
        if (!std::strcmp(e.name, argv[1])) ent = &e;
    if (!ent) {
        std::fprintf(stderr, "unknown helper %s\n", argv[1]);
        return 1;
    }
    std::vector<u64> file;
    {
        FILE* f = std::fopen(argv[2], "rb");
        if (!f) {
            std::perror(argv[2]);
            return 1;
        }
        std::fseek(f, 0, SEEK_END);
        const long bytes = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        if (bytes < 16 || bytes % 8) {
            std::fprintf(stderr, "%s: bad size %ld\n", argv[2], bytes);
            return 1;
        }
        file.resize((size_t)bytes / 8);
        if (std::fread(file.data(), 8, file.size(), f) != file.size()) {
            std::fprintf(stderr, "%s: short read\n", argv[2]);
            return 1;
        }
        std::fclose(f);
    }
    if (file[0] != MAGIC) {
        std::fprintf(stderr, "%s: bad magic\n", argv[2]);
        return 1;
    }
    // validate the whole layout before touching the device
    const u64 groups = file[1];
    struct Group {
        size_t k_at, in_at, out_at;
        u32 n;
    };
    std::vector<Group> gs;
    size_t at = 2, out_words = 0, max_in = 0, max_out = 0;
    for (u64 g = 0; g < groups; g++) {
        if (at + 9 > file.size()) {
            std::fprintf(stderr, "group %llu: truncated header\n", (unsigned long long)g);
            return 1;
        }
        const u64 n = file[at + 8];
        if (n == 0 || n > (1u << 24) || at + 9 + n * ent->in > file.size()) {
            std::fprintf(stderr, "group %llu: bad tuple count\n", (unsigned long long)g);
            return 1;
        }
        gs.push_back(Group{at, at + 9, out_words, (u32)n});
        at += 9 + (size_t)n * ent->in;
        out_words += (size_t)n * ent->out;
        if ((size_t)n * ent->in > max_in) max_in = (size_t)n * ent->in;
        if ((size_t)n * ent->out > max_out) max_out = (size_t)n * ent->out;
    }
    if (at != file.size() || gs.empty()) {
        std::fprintf(stderr, "%s: trailing or missing data\n", argv[2]);
        return 1;
    }
    std::vector<u64> res(out_words);
    u64 *d_in = nullptr, *d_out = nullptr;
    CHK(hipMalloc(&d_in, max_in * 8));
    CHK(hipMalloc(&d_out, max_out * 8));
    for (const Group& g : gs) {
        Consts K;
        std::memcpy(K.k, &file[g.k_at], sizeof K.k);
        CHK(hipMemcpy(d_in, &file[g.in_at], (size_t)g.n * ent->in * 8, hipMemcpyHostToDevice));
        CHK(hipMemset(d_out, 0xEE, (size_t)g.n * ent->out * 8));
        ent->launch(K, d_in, d_out, g.n);
        CHK(hipGetLastError());
        CHK(hipDeviceSynchronize());
        CHK(hipMemcpy(&res[g.out_at], d_out, (size_t)g.n * ent->out * 8, hipMemcpyDeviceToHost));
    }
    CHK(hipFree(d_in));
    CHK(hipFree(d_out));
    FILE* f = std::fopen(argv[3], "wb");
    if (!f) {
        std::perror(argv[3]);
        return 1;
    }
    if (std::fwrite(res.data(), 8, res.size(), f) != res.size() || std::fclose(f) != 0) {
        std::fprintf(stderr, "%s: write failed\n", argv[3]);
        return 1;
    }
    std::printf("%s: %zu groups, %zu result words\n", ent->name, gs.size(), res.size());
    return 0;
}
