// BGV decryption through the C++ adapter (ofhe_dcrt.hpp): BgvDecrypt::
// ModReduceChain and Decrypt and the free DecryptCore against the direct C ABI
// calls they wrap, on the same device data:
//   ofhe_hip_bgv_mod_reduce_chain, ofhe_hip_bgv_decrypt, ofhe_hip_decrypt_core
// (bgvrns-pke.cpp:44-99, rns-pke.cpp:199-224, dcrtpoly-impl.h:792-812), at
// N = 2^10 over a chain of 4 towers, batch 2, at the full chain and one level
// down; an encryption of a known plaintext decrypts through the adapter in both
// formats; ScalingFactor against its definition (no device).  No oracle is
// linked.  One sub-test per run: chain | decrypt | core | message | errors |
// scaling.  Prints "bgv_decrypt <sub-test>: <n> failures".
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../upmem--openfhe_amd/host/ofhe_dcrt.hpp"

using namespace ofhe;
typedef unsigned __int128 u128;

static uint64_t mulmod(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)((u128)a * b % q); }
static uint64_t powmod(uint64_t b, uint64_t e, uint64_t q) {
    uint64_t r = 1 % q;
    b %= q;
    for (; e; e >>= 1, b = mulmod(b, b, q))
        if (e & 1) r = mulmod(r, b, q);
    return r;
}
static uint64_t inv(uint64_t a, uint64_t p) { return powmod(a % p, p - 2, p); }  // p prime
static bool is_prime(uint64_t n) {
    if (n < 2) return false;
    const uint64_t bases[] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37};
    for (auto b : bases)
        if (n % b == 0) return n == b;
    uint64_t d = n - 1;
    int s = 0;
    while (!(d & 1)) d >>= 1, s++;
    for (auto b : bases) {
        uint64_t x = powmod(b, d, n);
        if (x == 1 || x == n - 1) continue;
        bool comp = true;
        for (int r = 1; r < s && comp; r++)
            if ((x = mulmod(x, x, n)) == n - 1) comp = false;
        if (comp) return false;
    }
    return true;
}
// the first prime = 1 mod m below 2^bits
static uint64_t prime_below(unsigned bits, uint32_t m) {
    uint64_t q = (1ull << bits) + 1;
    do q -= m;
    while (!is_prime(q));
    return q;
}
static uint64_t root_of_unity(uint64_t m, uint64_t q) {
    for (uint64_t c = 2;; c++) {
        const uint64_t psi = powmod(c, (q - 1) / m, q);
        if (powmod(psi, m / 2, q) == q - 1) return psi;
    }
}
static std::shared_ptr<DCRTParams> params(uint32_t m, const std::vector<uint64_t>& q) {
    std::vector<uint64_t> r;
    for (auto x : q) r.push_back(root_of_unity(m, x));
    return std::make_shared<DCRTParams>(m, q, r);
}

static int failures = 0;
static void expect(bool ok, const char* what) {
    if (!ok) {
        failures++;
        std::printf("FAIL %s\n", what);
    }
}
#define ABI(call) check((call), #call)

static std::vector<uint64_t> fetch(const DeviceBuffer& d) {
    std::vector<uint64_t> h(d.size());
    d.download(h.data());
    return h;
}
template <class F>
static bool throws(F&& f) {
    try {
        f();
    } catch (const math_error&) {
        return true;
    }
    return false;
}

static const uint32_t LOG_N = 10, M = 2u << LOG_N, N = M / 2, BATCH = 2;
static const uint64_t T = 65537;

struct Setup {
    std::vector<uint64_t> q;
    std::shared_ptr<DCRTParams> Q;
    std::shared_ptr<BgvDecrypt> dec;
    std::mt19937_64 rng{4242};
    Setup() {
        // 50-, 60-, 40- and 59-bit towers: SwitchModulus goes up and down along the chain
        for (unsigned bits : {50u, 60u, 40u, 59u}) q.push_back(prime_below(bits, M));
        Q = params(M, q);
        dec = BgvDecryptCache::get(Q, T);
    }
    DCRTPolyHip uniform(const std::shared_ptr<DCRTParams>& P, Format f, uint32_t b) {
        const size_t sq = P->Towers();
        std::vector<uint64_t> v((size_t)b * sq * N);
        for (size_t i = 0; i < v.size(); i++) v[i] = rng() % P->Moduli()[(i / N) % sq];
        DCRTPolyHip x(P, f, b);
        x.SetValues(v, f);
        return x;
    }
};

static void sub_chain() {
    Setup S;
    expect(BgvDecryptCache::get(S.Q, T) == S.dec, "the cache returns the handle it built");
    expect(BgvDecryptCache::get(S.Q, 257) != S.dec, "another t is another handle");
    DeviceBuffer out(S.Q->manager(), (size_t)BATCH * N);
    for (size_t size_ql : {4, 3, 1}) {
        auto Ql = S.Q->Slice(0, size_ql);
        DCRTPolyHip x = S.uniform(Ql, Format::COEFFICIENT, BATCH);
        const auto x_in = x.GetValues();
        for (int plain : {0, 1}) {
            ABI(ofhe_hip_bgv_mod_reduce_chain(S.dec->handle(), (uint32_t)size_ql, plain, x.data(), out.get(), BATCH,
                                              nullptr));
            expect(S.dec->ModReduceChain(x, plain != 0) == fetch(out), "ModReduceChain");
        }
        expect(x.GetValues() == x_in, "ModReduceChain leaves its input");
        if (size_ql == 1) expect(S.dec->ModReduceChain(x, false) == x_in, "one tower: the word itself");
    }
    S.Q->manager()->sync();
}

static void sub_decrypt() {
    Setup S;
    DCRTPolyHip s = S.uniform(S.Q, Format::EVALUATION, 1);
    DeviceBuffer out(S.Q->manager(), (size_t)BATCH * N);
    for (size_t size_ql : {4, 3})
        for (Format f : {Format::EVALUATION, Format::COEFFICIENT})
            for (size_t elements : {2, 3}) {
                auto Ql = S.Q->Slice(0, size_ql);
                std::vector<DCRTPolyHip> cv;
                for (size_t k = 0; k < elements; k++) cv.push_back(S.uniform(Ql, f, BATCH));
                const auto c1_in = cv[1].GetValues();
                ABI(ofhe_hip_bgv_decrypt(S.dec->handle(), S.Q->plan(), (uint32_t)size_ql, (uint32_t)elements,
                                         f == Format::EVALUATION, cv[0].data(), cv[1].data(),
                                         elements == 3 ? cv[2].data() : nullptr, s.data(), out.get(), BATCH, nullptr));
                expect(S.dec->Decrypt(cv, s) == fetch(out), "Decrypt");
                expect(cv[1].GetValues() == c1_in && cv[1].GetFormat() == f, "Decrypt leaves its inputs");
            }
    S.Q->manager()->sync();
}

static void sub_core() {
    Setup S;
    DCRTPolyHip s = S.uniform(S.Q, Format::EVALUATION, 1);
    for (size_t size_ql : {4, 3})
        for (Format f : {Format::EVALUATION, Format::COEFFICIENT})
            for (size_t elements : {2, 3})
                for (bool coeff_out : {false, true}) {
                    auto Ql = S.Q->Slice(0, size_ql);
                    std::vector<DCRTPolyHip> cv;
                    for (size_t k = 0; k < elements; k++) cv.push_back(S.uniform(Ql, f, BATCH));
                    DeviceBuffer out(S.Q->manager(), cv[0].words());
                    ABI(ofhe_hip_decrypt_core(Ql->plan(), (uint32_t)size_ql, (uint32_t)elements,
                                              f == Format::EVALUATION, coeff_out, cv[0].data(), cv[1].data(),
                                              elements == 3 ? cv[2].data() : nullptr, s.data(), out.get(), BATCH,
                                              nullptr));
                    DCRTPolyHip b = DecryptCore(cv, s, coeff_out);
                    expect(b.GetValues() == fetch(out), "DecryptCore");
                    expect(b.GetFormat() == (coeff_out ? Format::COEFFICIENT : Format::EVALUATION) &&
                               b.GetParams()->Moduli() == Ql->Moduli() && b.Batch() == BATCH,
                           "DecryptCore: the result's format, basis and batch");
                }
    // the same value from the adapter's own operators
    DCRTPolyHip c0 = S.uniform(S.Q, Format::EVALUATION, 1), c1 = S.uniform(S.Q, Format::EVALUATION, 1);
    expect(DecryptCore({c0, c1}, s).GetValues() == c0.Plus(c1.Times(s)).GetValues(),
           "DecryptCore = c0 + c1 s by the operators");
    S.Q->manager()->sync();
}

// c0 + c1 s = m + t e over 3 towers decrypts, in both formats, to m (q_1 q_2)^-1 mod t
static void sub_message() {
    Setup S;
    const size_t size_ql = 3;
    auto Ql = S.Q->Slice(0, size_ql);
    std::vector<uint64_t> msg(N), vv(size_ql * N), sv(S.q.size() * N);
    for (uint32_t i = 0; i < N; i++) {
        msg[i] = S.rng() % T;
        const int e = (int)(S.rng() % 7) - 3, sc = (int)(S.rng() % 3) - 1;
        const int64_t v = (int64_t)msg[i] + (int64_t)T * e;
        for (size_t k = 0; k < size_ql; k++) vv[k * N + i] = v < 0 ? S.q[k] - (uint64_t)(-v) : (uint64_t)v;
        for (size_t k = 0; k < S.q.size(); k++) sv[k * N + i] = sc < 0 ? S.q[k] - 1 : (uint64_t)sc;
    }
    DCRTPolyHip V(Ql, Format::COEFFICIENT), s(S.Q, Format::COEFFICIENT), sl(Ql, Format::COEFFICIENT);
    V.SetValues(vv, Format::COEFFICIENT);
    s.SetValues(sv, Format::COEFFICIENT);
    sl.SetValues(std::vector<uint64_t>(sv.begin(), sv.begin() + size_ql * N), Format::COEFFICIENT);
    V.SetFormat(Format::EVALUATION);
    s.SetFormat(Format::EVALUATION);
    sl.SetFormat(Format::EVALUATION);
    DCRTPolyHip a = S.uniform(Ql, Format::EVALUATION, 1);
    std::vector<DCRTPolyHip> ct;
    ct.push_back(V.Minus(a.Times(sl)));
    ct.push_back(std::move(a));
    const uint64_t scale = mulmod(inv(S.q[1] % T, T), inv(S.q[2] % T, T), T);
    std::vector<uint64_t> want(N);
    for (uint32_t i = 0; i < N; i++) want[i] = mulmod(msg[i], scale, T);
    expect(S.dec->Decrypt(ct, s) == want, "decrypt of an encryption, EVALUATION form");
    for (auto& c : ct) c.SetFormat(Format::COEFFICIENT);
    expect(S.dec->Decrypt(ct, s) == want, "decrypt of an encryption, COEFFICIENT form");
    // the scaling factor that undoes it: ModReduce factors q_l mod t
    const std::vector<uint64_t> factors{0, S.q[1] % T, S.q[2] % T};
    expect(BgvDecrypt::ScalingFactor(1, factors, size_ql, T) == scale, "ScalingFactor is the plaintext's factor");
    S.Q->manager()->sync();
}

static void sub_errors() {
    Setup S;
    auto Ql = S.Q->Slice(0, 3);
    DCRTPolyHip s = S.uniform(S.Q, Format::EVALUATION, 1), c = S.uniform(Ql, Format::EVALUATION, BATCH);
    DCRTPolyHip other = S.uniform(S.Q->Slice(1, 2), Format::EVALUATION, BATCH);
    DCRTPolyHip sc = S.uniform(S.Q, Format::COEFFICIENT, 1), cc = S.uniform(Ql, Format::COEFFICIENT, BATCH);
    expect(throws([&] { S.dec->ModReduceChain(c, true); }), "ModReduceChain of an EVALUATION-form input");
    expect(throws([&] { S.dec->ModReduceChain(S.uniform(S.Q->Slice(1, 2), Format::COEFFICIENT, 1), true); }),
           "ModReduceChain over towers that are not the chain's first");
    expect(throws([&] { S.dec->Decrypt({c}, s); }), "Decrypt of one element");
    expect(throws([&] { S.dec->Decrypt({c, cc}, s); }), "Decrypt of mixed formats");
    expect(throws([&] { S.dec->Decrypt({c, c}, sc); }), "Decrypt with a COEFFICIENT-form key");
    expect(throws([&] { S.dec->Decrypt({other, other}, s); }), "Decrypt over towers that are not the key's first");
    expect(throws([&] { DecryptCore({c, c}, S.uniform(Ql->Slice(0, 2), Format::EVALUATION, 1)); }),
           "DecryptCore with a key shorter than the ciphertext");
    expect(throws([&] { BgvDecrypt(S.Q, 1); }), "t = 1");
    expect(throws([&] { BgvDecrypt(S.Q, S.q[2]); }), "t not invertible modulo a tower");
    S.Q->manager()->sync();
}

static void sub_scaling() {
    const uint64_t t = 65537;
    const std::vector<uint64_t> f{11, 65536, 3, 40000, 2};
    for (size_t size_ql = 1; size_ql <= f.size(); size_ql++)
        for (uint64_t sf : std::vector<uint64_t>{1, 12345, t - 1, t + 5}) {
            uint64_t want = sf % t;
            for (size_t i = 0; i + 1 < size_ql; i++) want = mulmod(want, inv(f[size_ql - 1 - i], t), t);
            expect(BgvDecrypt::ScalingFactor(sf, f, size_ql, t) == want, "ScalingFactor against its definition");
        }
    expect(BgvDecrypt::ScalingFactor(7, {}, 1, t) == 7, "one tower: nothing to undo");
    expect(BgvDecrypt::ScalingFactor(5, {0, 4}, 2, 9) == 8, "a composite t: 5 * 4^-1 = 5 * 7 = 35 = 8 mod 9");
    expect(throws([&] { BgvDecrypt::ScalingFactor(1, {1, 6}, 2, 9); }), "a factor that is not invertible");
    expect(throws([&] { BgvDecrypt::ScalingFactor(1, {1, 5}, 3, 7); }), "fewer factors than levels");
    expect(throws([&] { BgvDecrypt::ScalingFactor(1, {1}, 1, 1); }), "t = 1");
}

int main(int argc, char** argv) {
    const char* which = argc > 1 ? argv[1] : "";
    const struct {
        const char* name;
        void (*run)();
    } subs[] = {{"chain", sub_chain},     {"decrypt", sub_decrypt}, {"core", sub_core},
                {"message", sub_message}, {"errors", sub_errors},   {"scaling", sub_scaling}};
    for (const auto& s : subs)
        if (!std::strcmp(which, s.name)) {
            try {
                s.run();
            } catch (const std::exception& e) {
                std::printf("bgv_decrypt %s failed: %s\n", which, e.what());
                return 1;
            }
            std::printf("bgv_decrypt %s: %d failures\n", which, failures);
            return failures ? 1 : 0;
        }
    std::printf("usage: test_bgv_decrypt_bin chain|decrypt|core|message|errors|scaling\n");
    return 2;
}
