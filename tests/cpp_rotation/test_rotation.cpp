// Hoisted rotations through the C++ adapter (ofhe_dcrt.hpp):
// KeySwitchHybrid::FastRotationPrecompute / FastRotation / FastRotationExt
// against the step-by-step composition of the C ABI calls they replace, on
// the same device buffers:
//   Ext      ofhe_hip_ks_fast_core_ext, ofhe_hip_modmul_scalar (c0 * PModq),
//            ofhe_hip_modadd_vv, ofhe_hip_automorphism
//   non-Ext  ofhe_hip_ks_fast_core_ext, ofhe_hip_ks_mod_down,
//            ofhe_hip_modadd_vv (+= c0), ofhe_hip_automorphism
// (ckksrns-leveledshe.cpp:402-457, base-leveledshe.cpp:471-513).  N = 2^10,
// Q = 4, P = 2, dnum = 2, 3 rotations with distinct keys, batch 2.  No oracle
// is linked.  A wrong-shape key and a COEFFICIENT-form c0 must throw
// math_error.  Prints "rotation: <n> failures".
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
// 60-bit primes = 1 mod m, descending, and a primitive m-th root of each
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

static int failures = 0;
static void expect(bool ok, const char* what, uint32_t r = 0) {
    if (!ok) {
        failures++;
        std::printf("FAIL %s (rotation %u)\n", what, r);
    }
}
#define ABI(call) check((call), #call)

int main() {
    const uint32_t log_n = 10, m = 2u << log_n, n = m / 2, batch = 2, sq = 4, sp = 2, dnum = 2, nrot = 3;
    try {
        auto all = chain(m, sq + sp);
        std::vector<uint64_t> q(all.begin(), all.begin() + sq), p(all.begin() + sq, all.end());
        auto PQ = params(m, q), PP = params(m, p), PQP = params(m, all);
        KeySwitchHybrid ks(*PQ, *PP, dnum);
        HipManager* mgr = PQ->manager();
        std::vector<uint64_t> pmodq;  // m_PModq
        for (auto qi : q) {
            uint64_t r = 1;
            for (auto pj : p) r = mulmod(r, pj % qi, qi);
            pmodq.push_back(r);
        }
        std::mt19937_64 rng(77);
        auto uniform = [&](const std::shared_ptr<DCRTParams>& P, uint32_t rows, Format f) {
            const auto& mods = P->Moduli();
            std::vector<uint64_t> v((size_t)rows * mods.size() * n);
            for (size_t i = 0; i < v.size(); i++) v[i] = rng() % mods[(i / n) % mods.size()];
            DCRTPolyHip x(P, f, rows);
            x.SetValues(v, f);
            return x;
        };
        DCRTPolyHip C0 = uniform(PQ, batch, Format::EVALUATION), C1 = uniform(PQ, batch, Format::EVALUATION);
        std::vector<DCRTPolyHip> KB, KA;
        for (uint32_t r = 0; r < nrot; r++) {
            KB.push_back(uniform(PQP, dnum, Format::EVALUATION));
            KA.push_back(uniform(PQP, dnum, Format::EVALUATION));
        }
        std::vector<KeySwitchHybrid::RotationKey> keys;
        for (uint32_t r = 0; r < nrot; r++) keys.emplace_back(&KB[r], &KA[r]);
        const std::vector<uint32_t> idx{5, 2 * n - 1, 2 * n + 25};
        const auto c0_in = C0.GetValues(), kb0_in = KB[0].GetValues();

        auto digits = ks.FastRotationPrecompute(C1);
        const size_t poly = (size_t)(sq + sp) * n, qpoly = (size_t)sq * n;
        expect(digits.size_ql == sq && digits.batch == batch && digits.buf.size() == (size_t)batch * 2 * poly,
               "FastRotationPrecompute shape");
        const auto digits_in = [&] {
            std::vector<uint64_t> h(digits.buf.size());
            digits.buf.download(h.data());
            return h;
        }();

        auto ext_add = ks.FastRotationExt(&C0, digits, idx, keys, PQP);
        auto ext = ks.FastRotationExt(nullptr, digits, idx, keys, PQP);
        auto rot0 = ks.FastRotation(C0, digits, idx, keys);
        auto rot_t = ks.FastRotation(C0, digits, idx, keys, 65537);
        expect(ext_add.size() == nrot && ext.size() == nrot && rot0.size() == nrot && rot_t.size() == nrot,
               "one pair per rotation");

        // the composition, rotation by rotation
        DeviceBuffer ct0(mgr, batch * poly), ct1(mgr, batch * poly), e0(mgr, batch * poly), e1(mgr, batch * poly);
        DeviceBuffer cm(mgr, batch * qpoly), md0(mgr, batch * qpoly), md1(mgr, batch * qpoly), o0(mgr, batch * qpoly),
            o1(mgr, batch * qpoly);
        auto same = [&](const DeviceBuffer& d, const DCRTPolyHip& x) {
            std::vector<uint64_t> h(d.size());
            d.download(h.data());
            return h == x.GetValues();
        };
        for (uint32_t r = 0; r < nrot; r++) {
            ABI(ofhe_hip_ks_fast_core_ext(ks.handle(), sq, digits.buf.get(), KB[r].data(), KA[r].data(), ct0.get(),
                                          ct1.get(), batch, nullptr));
            for (uint64_t t : {0ull, 65537ull}) {
                ABI(ofhe_hip_ks_mod_down(ks.handle(), sq, ct0.get(), md0.get(), t, batch, nullptr));
                ABI(ofhe_hip_ks_mod_down(ks.handle(), sq, ct1.get(), md1.get(), t, batch, nullptr));
                ABI(ofhe_hip_modadd_vv(PQ->plan(), md0.get(), C0.data(), md0.get(), batch, nullptr));
                ABI(ofhe_hip_automorphism(PQ->plan(), idx[r], 1, md0.get(), o0.get(), batch, nullptr));
                ABI(ofhe_hip_automorphism(PQ->plan(), idx[r], 1, md1.get(), o1.get(), batch, nullptr));
                const auto& got = t ? rot_t[r] : rot0[r];
                expect(same(o0, got.first) && same(o1, got.second), t ? "FastRotation t = 65537" : "FastRotation", r);
            }
            ABI(ofhe_hip_automorphism(PQP->plan(), idx[r], 1, ct0.get(), e0.get(), batch, nullptr));
            ABI(ofhe_hip_automorphism(PQP->plan(), idx[r], 1, ct1.get(), e1.get(), batch, nullptr));
            expect(same(e0, ext[r].first) && same(e1, ext[r].second), "FastRotationExt", r);
            ABI(ofhe_hip_modmul_scalar(PQ->plan(), C0.data(), pmodq.data(), cm.get(), batch, nullptr));
            for (uint32_t b = 0; b < batch; b++)  // the Q towers of entry b
                ABI(ofhe_hip_modadd_vv(PQ->plan(), ct0.get() + b * poly, cm.get() + b * qpoly, ct0.get() + b * poly, 1,
                                       nullptr));
            ABI(ofhe_hip_automorphism(PQP->plan(), idx[r], 1, ct0.get(), e0.get(), batch, nullptr));
            expect(same(e0, ext_add[r].first) && same(e1, ext_add[r].second), "FastRotationExt, addFirst", r);
            expect(ext_add[r].first.GetParams() == PQP && rot0[r].first.GetParams() == PQ &&
                       rot0[r].second.Batch() == batch && ext[r].first.GetFormat() == Format::EVALUATION,
                   "result params", r);
        }
        {
            std::vector<uint64_t> h(digits.buf.size());
            digits.buf.download(h.data());
            expect(h == digits_in && C0.GetValues() == c0_in && KB[0].GetValues() == kb0_in, "inputs unchanged");
        }

        // argument checks of the adapter
        auto throws = [&](auto&& f) {
            try {
                f();
            } catch (const math_error&) {
                return true;
            }
            return false;
        };
        DCRTPolyHip narrow = uniform(PQ, dnum, Format::EVALUATION);  // a key over Q only
        std::vector<KeySwitchHybrid::RotationKey> bad = keys;
        bad[1] = {&narrow, &KA[1]};
        expect(throws([&] { ks.FastRotation(C0, digits, idx, bad); }), "wrong-shape key, FastRotation");
        expect(throws([&] { ks.FastRotationExt(&C0, digits, idx, bad, PQP); }), "wrong-shape key, FastRotationExt");
        DCRTPolyHip coeff = uniform(PQ, batch, Format::COEFFICIENT);
        expect(throws([&] { ks.FastRotation(coeff, digits, idx, keys); }), "COEFFICIENT c0, FastRotation");
        expect(throws([&] { ks.FastRotationExt(&coeff, digits, idx, keys, PQP); }), "COEFFICIENT c0, FastRotationExt");
        expect(throws([&] { ks.FastRotationPrecompute(coeff); }), "COEFFICIENT c1, FastRotationPrecompute");
        expect(throws([&] { ks.FastRotation(C0, digits, {5, 6, 7}, keys); }), "even index");
        expect(throws([&] { ks.FastRotation(C0, digits, {5}, keys); }), "index / key count");
        // still usable afterwards
        auto again = ks.FastRotation(C0, digits, idx, keys);
        expect(again[2].first.GetValues() == rot0[2].first.GetValues(), "usable after the errors");
        mgr->sync();
    } catch (const std::exception& e) {
        std::printf("rotation failed: %s\n", e.what());
        return 1;
    }
    std::printf("rotation: %d failures\n", failures);
    return failures ? 1 : 0;
}
