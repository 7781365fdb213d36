// BFV (BEHZ) multiplication through the C++ adapter (ofhe_dcrt.hpp):
// BehzBasis::FastBaseConvqToBskMontgomery, FastRNSFloorq, FastBaseConvSK and
// BfvMultBehz against the direct C ABI calls they wrap, step by step on the
// same device data:
//   ofhe_hip_behz_expand x 4, ofhe_hip_eval_mult_core (Q|Bsk), ofhe_hip_ntt_inv,
//   ofhe_hip_behz_floor, ofhe_hip_behz_conv_sk; ofhe_hip_behz_floor_sk fused and
//   in two launches
// (bfvrns-leveledshe.cpp:275-297, 383-403, dcrtpoly-impl.h:2050-2208, 2212-2271,
// 2309-2411).  N = 2^10, Q = 2, B = 2 (+ msk), batch 2, true tables
// (bfvrns-cryptoparameters.cpp:724-851) computed here.  The reference's N = 8
// known answer of FastBaseConvqToBskMontgomery
// (UnitTestBFVrnsCRTOperations.cpp:197-287) is carried as literal numbers.
// No oracle is linked.  Prints "behz: <n> failures".
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
// the smallest primitive m-th root of unity mod q, as the reference's RootOfUnity
// returns it (nbtheory-impl.h:183-231): the known answer is in evaluation form
static uint64_t root_of_unity(uint64_t m, uint64_t q) {
    for (uint64_t c = 2;; c++) {
        const uint64_t psi = powmod(c, (q - 1) / m, q);
        if (powmod(psi, m / 2, q) != q - 1) continue;
        uint64_t best = psi, cur = psi;
        const uint64_t sq = mulmod(psi, psi, q);
        for (uint64_t k = 3; k < m; k += 2) {
            cur = mulmod(cur, sq, q);
            if (cur < best) best = cur;
        }
        return best;
    }
}
static std::shared_ptr<DCRTParams> params(uint32_t m, const std::vector<uint64_t>& q) {
    std::vector<uint64_t> r;
    for (auto x : q) r.push_back(root_of_unity(m, x));
    return std::make_shared<DCRTParams>(m, q, r);
}
// prod_{k != skip} ms[k] mod m (skip = ms.size(): the whole product)
static uint64_t prod_mod(const std::vector<uint64_t>& ms, size_t skip, uint64_t m) {
    uint64_t r = 1 % m;
    for (size_t k = 0; k < ms.size(); k++)
        if (k != skip) r = mulmod(r, ms[k] % m, m);
    return r;
}

// the BEHZ tables of q, Bsk = b | msk and t (bfvrns-cryptoparameters.cpp:724-851)
static BehzTables behz_tables(const std::vector<uint64_t>& q, const std::vector<uint64_t>& bsk, uint64_t t) {
    const uint64_t mt = 1ull << 16, msk = bsk.back();
    const std::vector<uint64_t> b(bsk.begin(), bsk.end() - 1);
    BehzTables T;
    for (size_t i = 0; i < q.size(); i++) {
        const uint64_t hinv = inv(prod_mod(q, i, q[i]), q[i]);
        T.tQHatInvModq.push_back(mulmod(hinv, t, q[i]));
        T.mtildeQHatInvModq.push_back(mulmod(hinv, mt, q[i]));
        T.QHatModmtilde.push_back(prod_mod(q, i, mt));
        T.BModq.push_back(prod_mod(b, b.size(), q[i]));
        for (auto bj : bsk) {
            T.QHatModbsk.push_back(prod_mod(q, i, bj));
            T.qInvModbsk.push_back(inv(q[i], bj));
        }
    }
    const uint64_t qm = prod_mod(q, q.size(), mt);
    for (uint64_t v = 1; v < mt; v += 2)
        if ((v * qm + 1) % mt == 0) T.negQInvModmtilde = v;
    for (auto bj : bsk) {
        const uint64_t Qb = prod_mod(q, q.size(), bj);
        T.QModbsk.push_back(Qb);
        T.mtildeInvModbsk.push_back(inv(mt, bj));
        T.tQInvModbsk.push_back(mulmod(inv(Qb, bj), t, bj));
    }
    for (size_t i = 0; i < b.size(); i++) {
        T.BHatInvModb.push_back(inv(prod_mod(b, i, b[i]), b[i]));
        T.BHatModmsk.push_back(prod_mod(b, i, msk));
        for (auto qj : q) T.BHatModq.push_back(prod_mod(b, i, qj));
    }
    T.BInvModmsk = inv(prod_mod(b, b.size(), msk), msk);
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

static std::vector<uint64_t> join(const std::vector<uint64_t>& a, const std::vector<uint64_t>& b) {
    std::vector<uint64_t> r(a);
    r.insert(r.end(), b.begin(), b.end());
    return r;
}

static void known_answer() {
    const std::vector<uint64_t> q{1152921504606846577ull, 1152921504606846097ull},
        bsk{1152921504606845777ull, 1152921504606845473ull, 1152921504606844913ull};
    const std::vector<uint64_t> x{611651427055975783ull, 739811248882229946ull,  790810915716521716ull,
                                  536363726228107588ull, 647651536262422014ull,  322042217691169971ull,
                                  138609670727909932ull, 793736138075446811ull,  846754661443099927ull,
                                  602279558317502186ull, 342175723088143584ull,  904036735987820179ull,
                                  1124341799555345257ull, 885339199454111253ull, 417243638107713607ull,
                                  548811148460128084ull};
    const std::vector<uint64_t> ans{524228833460429474ull, 692928367413813885ull, 465662343623521646ull,
                                    107498520099165490ull, 81602760285107383ull,  482417615916109741ull,
                                    249076385001962496ull, 719980682178715834ull, 474506930637362424ull,
                                    723790960760608304ull, 7991172453764409ull,   738286918217632692ull,
                                    933904287195446155ull, 98490114749039532ull,  293617451261147895ull,
                                    1050780276990075548ull, 612459830520599999ull, 273948808875966259ull,
                                    276211279884817131ull, 805184382328000673ull, 605603488049806384ull,
                                    756318612975583592ull, 1014214483788531002ull, 480836070509458175ull};
    auto PQ = params(16, q), PB = params(16, bsk), PQB = params(16, join(q, bsk));
    BehzBasis basis(PQ, PB, PQB, 65537, behz_tables(q, bsk, 65537));
    DCRTPolyHip a(PQ, Format::EVALUATION);
    a.SetValues(x, Format::EVALUATION);
    DCRTPolyHip got = basis.FastBaseConvqToBskMontgomery(a);
    expect(got.GetValues() == join(x, ans) && got.GetFormat() == Format::EVALUATION && got.GetParams() == PQB,
           "FastBaseConvqToBskMontgomery known answer, N = 8");
}

static void parity() {
    const uint32_t log_n = 10, m = 2u << log_n, n = m / 2, batch = 2, sq = 2, sb = 2, sk = sb + 1;
    const uint64_t t = 65537;
    auto all = chain(m, sq + sk);
    std::vector<uint64_t> q(all.begin(), all.begin() + sq), bsk(all.begin() + sq, all.end());
    auto PQ = params(m, q), PB = params(m, bsk), PQB = params(m, all);
    HipManager* mgr = PQ->manager();
    BehzBasis basis(PQ, PB, PQB, t, behz_tables(q, bsk, t));
    std::mt19937_64 rng(4242);
    auto uniform = [&](const std::shared_ptr<DCRTParams>& P, Format f) {
        const auto& mods = P->Moduli();
        std::vector<uint64_t> v((size_t)batch * mods.size() * n);
        for (size_t i = 0; i < v.size(); i++) v[i] = rng() % mods[(i / n) % mods.size()];
        DCRTPolyHip x(P, f, batch);
        x.SetValues(v, f);
        return x;
    };
    auto same = [&](const DeviceBuffer& d, const DCRTPolyHip& x) {
        std::vector<uint64_t> h(d.size());
        d.download(h.data());
        return h == x.GetValues();
    };
    const size_t qw = (size_t)sq * n, kw = (size_t)sk * n, qkw = qw + kw;
    DCRTPolyHip C0 = uniform(PQ, Format::EVALUATION), C1 = uniform(PQ, Format::EVALUATION),
                D0 = uniform(PQ, Format::EVALUATION), D1 = uniform(PQ, Format::EVALUATION);
    const auto c0_in = C0.GetValues(), d1_in = D1.GetValues();

    // the single-step members against their C ABI calls
    DCRTPolyHip xc = uniform(PQ, Format::COEFFICIENT), xqb = uniform(PQB, Format::COEFFICIENT),
                xb = uniform(PB, Format::COEFFICIENT);
    DeviceBuffer ex(mgr, batch * qkw), fl(mgr, batch * kw), sk_out(mgr, batch * qw), fs(mgr, batch * qw);
    for (const DCRTPolyHip* v : {&xc, &C0}) {
        ABI(ofhe_hip_behz_expand(basis.handle(), PQ->plan(), PB->plan(), v->GetFormat() == Format::EVALUATION, v->data(),
                                 ex.get(), batch, nullptr));
        DCRTPolyHip got = basis.FastBaseConvqToBskMontgomery(*v);
        expect(same(ex, got) && got.GetFormat() == Format::EVALUATION && got.GetParams() == PQB,
               "FastBaseConvqToBskMontgomery");
    }
    ABI(ofhe_hip_behz_floor(basis.handle(), xqb.data(), fl.get(), batch, nullptr));
    DCRTPolyHip floored = basis.FastRNSFloorq(xqb);
    expect(same(fl, floored) && floored.GetParams() == PB && floored.GetFormat() == Format::COEFFICIENT, "FastRNSFloorq");
    ABI(ofhe_hip_behz_conv_sk(basis.handle(), xb.data(), sk_out.get(), batch, nullptr));
    DCRTPolyHip conv = basis.FastBaseConvSK(xb);
    expect(same(sk_out, conv) && conv.GetParams() == PQ, "FastBaseConvSK");
    DCRTPolyHip chained = basis.FastBaseConvSK(floored);
    for (int fused = 0; fused <= 2; fused++) {
        ABI(ofhe_hip_behz_floor_sk(basis.handle(), fused, xqb.data(), fs.get(), batch, nullptr));
        expect(same(fs, chained), "floor_sk equals FastRNSFloorq then FastBaseConvSK");
    }

    // BfvMultBehz against the composition
    auto got = basis.BfvMultBehz(C0, C1, D0, D1);
    expect(got.size() == 3 && got[0].GetFormat() == Format::COEFFICIENT && got[2].GetParams() == PQ, "BfvMultBehz shape");
    std::vector<DeviceBuffer> E, T;
    for (int k = 0; k < 4; k++) E.emplace_back(mgr, batch * qkw);
    for (int k = 0; k < 3; k++) T.emplace_back(mgr, batch * qkw);
    const DCRTPolyHip* in[4] = {&C0, &C1, &D0, &D1};
    for (int k = 0; k < 4; k++)
        ABI(ofhe_hip_behz_expand(basis.handle(), PQ->plan(), PB->plan(), 1, in[k]->data(), E[k].get(), batch, nullptr));
    ABI(ofhe_hip_eval_mult_core(PQB->plan(), E[0].get(), E[1].get(), E[2].get(), E[3].get(), T[0].get(), T[1].get(),
                                T[2].get(), batch, nullptr));
    for (int k = 0; k < 3; k++) {
        ABI(ofhe_hip_ntt_inv(PQB->plan(), T[k].get(), batch, nullptr));
        DeviceBuffer f(mgr, batch * kw), o(mgr, batch * qw);
        ABI(ofhe_hip_behz_floor(basis.handle(), T[k].get(), f.get(), batch, nullptr));
        ABI(ofhe_hip_behz_conv_sk(basis.handle(), f.get(), o.get(), batch, nullptr));
        expect(same(o, got[k]), "BfvMultBehz");
    }
    expect(C0.GetValues() == c0_in && D1.GetValues() == d1_in, "inputs unchanged");

    // argument checks of the adapter
    auto throws = [&](auto&& f) {
        try {
            f();
        } catch (const math_error&) {
            return true;
        }
        return false;
    };
    expect(throws([&] { basis.BfvMultBehz(xc, C1, D0, D1); }), "COEFFICIENT-form input");
    expect(throws([&] { basis.FastRNSFloorq(C0); }), "FastRNSFloorq over another basis");
    expect(throws([&] { basis.FastBaseConvSK(xqb); }), "FastBaseConvSK over another basis");
    expect(throws([&] { BehzBasis(PQ, PB, PQ, t, behz_tables(q, bsk, t)); }), "QBsk of the wrong size");
    expect(throws([&] { BehzBasis(PQ, PB, PQB, t, behz_tables(q, {bsk[0], bsk[2]}, t)); }), "tables of another size");
    auto again = basis.BfvMultBehz(C0, C1, D0, D1);
    expect(again[1].GetValues() == got[1].GetValues(), "usable after the errors");
    mgr->sync();
}

int main() {
    try {
        known_answer();
        parity();
    } catch (const std::exception& e) {
        std::printf("behz failed: %s\n", e.what());
        return 1;
    }
    std::printf("behz: %d failures\n", failures);
    return failures ? 1 : 0;
}
