// BFV decryption through the C++ adapter (ofhe_dcrt.hpp): BfvDecrypt::
// ScaleAndRound and Decrypt and DCRTPolyHip::TimesQovert against the direct C
// ABI calls they wrap, on the same device data:
//   ofhe_hip_bfv_decrypt_scale_round, ofhe_hip_bfv_decrypt, ofhe_hip_times_q_over_t
// (bfvrns-pke.cpp:205-248, rns-pke.cpp:199-224, dcrtpoly-impl.h:1537-1814,
// 2005-2049, 1015-1031), for the HPS family and BEHZ at N = 2^10, Q = 3,
// batch 2, and on one tower.  The tables (bfvrns-cryptoparameters.cpp:87-94,
// 446-495, 853-884) are computed here; an encryption of a known plaintext,
// made with TimesQovert, decrypts through the adapter.  No oracle is linked.
// Prints "decrypt: <n> failures".
#include <cstdio>
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
// 60-bit primes = 1 mod m, descending
static std::vector<uint64_t> chain(uint32_t m, int count) {
    uint64_t q = (1ull << 60) + 1;
    std::vector<uint64_t> out;
    while ((int)out.size() < count) {
        q -= m;
        if (is_prime(q)) out.push_back(q);
    }
    return out;
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
static uint64_t prod_mod(const std::vector<uint64_t>& ms, size_t skip, uint64_t m) {
    uint64_t r = 1 % m;
    for (size_t k = 0; k < ms.size(); k++)
        if (k != skip) r = mulmod(r, ms[k] % m, m);
    return r;
}
static uint64_t inv_mod_any(uint64_t a, uint64_t m) {  // a^-1 mod m by the extended Euclidean algorithm
    __int128 r0 = m, r1 = a % m, s0 = 0, s1 = 1;
    while (r1) {
        const __int128 k = r0 / r1, r2 = r0 - k * r1, s2 = s0 - k * s1;
        r0 = r1, r1 = r2, s0 = s1, s1 = s2;
    }
    return (uint64_t)((s0 % (__int128)m + m) % m);
}

// floor(X 2^shift / q) mod t and double(X 2^shift mod q) / double(q) for X = t h, h < q < 2^60, t < 2^32,
// shift <= 30: X 2^shift < 2^122
static void div_parts(uint64_t t, uint64_t h, unsigned shift, uint64_t q, uint64_t* modt, double* frac) {
    const u128 X = ((u128)t * h) << shift;
    *modt = (uint64_t)(X / q % t);
    *frac = (double)(int64_t)(X % q) / (double)(int64_t)q;
}

// the decryption tables of q and t (bfvrns-cryptoparameters.cpp:87-94, 446-495, 853-884)
static BfvDecryptTables decrypt_tables(const std::vector<uint64_t>& q, uint64_t t) {
    BfvDecryptTables T;
    const unsigned hf = (64 - __builtin_clzll(q[0])) >> 1;
    const uint64_t tgamma = t << 26;
    for (size_t i = 0; i < q.size(); i++) {
        const uint64_t h = inv(prod_mod(q, i, q[i]), q[i]);
        uint64_t w;
        double f;
        div_parts(t, h, 0, q[i], &w, &f);
        T.tQHatInvModqDivqModt.push_back(w);
        T.tQHatInvModqDivqFrac.push_back(f);
        div_parts(t, h, hf, q[i], &w, &f);
        T.tQHatInvModqBDivqModt.push_back(w);
        T.tQHatInvModqBDivqFrac.push_back(f);
        T.tgammaQHatInvModq.push_back(mulmod(mulmod(h, 1ull << 26, q[i]), t, q[i]));
        T.negInvqModtgamma.push_back(mulmod(tgamma - 1, inv_mod_any(q[i], tgamma), tgamma));
        T.tInvModq.push_back(inv(t, q[i]));
    }
    T.negQModt = t - prod_mod(q, q.size(), t);
    return T;
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

static void parity(int technique, uint32_t sq) {
    const uint32_t log_n = 10, m = 2u << log_n, n = m / 2, batch = 2;
    const uint64_t t = 65537;
    const auto q = chain(m, sq);
    auto PQ = params(m, q);
    HipManager* mgr = PQ->manager();
    BfvDecrypt dec(PQ, t, technique, decrypt_tables(q, t));
    expect(dec.Branch() == (sq == 1 ? OFHE_BFV_DECRYPT_ONE_TOWER : technique == OFHE_BFV_BEHZ ? OFHE_BFV_DECRYPT_BEHZ : 6),
           "the loop that runs (G for 60-bit towers and t = 65537)");
    std::mt19937_64 rng(777 + technique + sq);
    auto uniform = [&](Format f, uint32_t b) {
        std::vector<uint64_t> v((size_t)b * sq * n);
        for (size_t i = 0; i < v.size(); i++) v[i] = rng() % q[(i / n) % sq];
        DCRTPolyHip x(PQ, f, b);
        x.SetValues(v, f);
        return x;
    };
    // ScaleAndRound
    DCRTPolyHip x = uniform(Format::COEFFICIENT, batch);
    DeviceBuffer out(mgr, (size_t)batch * n);
    ABI(ofhe_hip_bfv_decrypt_scale_round(dec.handle(), x.data(), out.get(), batch, nullptr));
    expect(dec.ScaleAndRound(x) == fetch(out), "ScaleAndRound");
    // TimesQovert
    DCRTPolyHip y = uniform(Format::COEFFICIENT, batch);
    DeviceBuffer ty(mgr, y.words());
    ABI(ofhe_hip_times_q_over_t(dec.handle(), y.data(), ty.get(), batch, nullptr));
    y.TimesQovert(dec);
    expect(y.GetValues() == fetch(ty), "TimesQovert");
    // Decrypt: 2 and 3 elements, both formats
    DCRTPolyHip s = uniform(Format::EVALUATION, 1);
    for (Format f : {Format::EVALUATION, Format::COEFFICIENT})
        for (size_t elements : {2, 3}) {
            std::vector<DCRTPolyHip> cv;
            for (size_t k = 0; k < elements; k++) cv.push_back(uniform(f, batch));
            const auto c1_in = cv[1].GetValues();
            ABI(ofhe_hip_bfv_decrypt(dec.handle(), PQ->plan(), (uint32_t)elements, f == Format::EVALUATION, cv[0].data(),
                                     cv[1].data(), elements == 3 ? cv[2].data() : nullptr, s.data(), out.get(), batch,
                                     nullptr));
            expect(dec.Decrypt(cv, s) == fetch(out), "Decrypt");
            expect(cv[1].GetValues() == c1_in && cv[1].GetFormat() == f, "Decrypt leaves its inputs");
        }
    // an encryption made with TimesQovert decrypts: c0 = TimesQovert(msg) + e - a s, c1 = a
    std::vector<uint64_t> msg(n), mv((size_t)sq * n), ev((size_t)sq * n);
    for (uint32_t i = 0; i < n; i++) {
        msg[i] = rng() % t;
        const int e = (int)(rng() % 7) - 3;
        for (uint32_t k = 0; k < sq; k++) {
            mv[(size_t)k * n + i] = msg[i];
            ev[(size_t)k * n + i] = e < 0 ? q[k] - (uint64_t)(-e) : (uint64_t)e;
        }
    }
    DCRTPolyHip M(PQ, Format::COEFFICIENT), E(PQ, Format::COEFFICIENT);
    M.SetValues(mv, Format::COEFFICIENT);
    E.SetValues(ev, Format::COEFFICIENT);
    M.TimesQovert(dec);
    DCRTPolyHip b = M.Plus(E);
    b.SetFormat(Format::EVALUATION);
    DCRTPolyHip a = uniform(Format::EVALUATION, 1);
    std::vector<DCRTPolyHip> ct;
    ct.push_back(b.Minus(a.Times(s)));
    ct.push_back(std::move(a));
    auto plain = dec.Decrypt(ct, s);
    for (auto& v : plain) v %= t;
    expect(plain == msg, "encrypt with TimesQovert, decrypt");

    auto throws = [&](auto&& f) {
        try {
            f();
        } catch (const math_error&) {
            return true;
        }
        return false;
    };
    expect(throws([&] { dec.ScaleAndRound(s); }), "ScaleAndRound of an EVALUATION-form input");
    expect(throws([&] { dec.Decrypt({ct[0]}, s); }), "Decrypt of one element");
    expect(throws([&] { dec.Decrypt(ct, x); }), "Decrypt with a COEFFICIENT-form key");
    mgr->sync();
}

int main() {
    try {
        parity(OFHE_BFV_HPS, 3);
        parity(OFHE_BFV_BEHZ, 3);
        parity(OFHE_BFV_HPSPOVERQ, 1);
        parity(OFHE_BFV_BEHZ, 1);
    } catch (const std::exception& e) {
        std::printf("decrypt failed: %s\n", e.what());
        return 1;
    }
    std::printf("decrypt: %d failures\n", failures);
    return failures ? 1 : 0;
}
