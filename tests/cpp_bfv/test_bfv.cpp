// BFV (HPS family) multiplication through the C++ adapter (ofhe_dcrt.hpp):
// BaseConverter::SwitchCRTBasis, ExpandCRTBasis, ScaleAndRound and
// BfvMult::EvalMult against the direct C ABI calls they wrap, step by step on
// the same device data:
//   HPS        ofhe_hip_expand_crt_basis x 4, ofhe_hip_eval_mult_core (Q|R),
//              ofhe_hip_ntt_inv, ofhe_hip_scale_and_round, ofhe_hip_switch_crt_basis
//   HPSPOVERQ  ofhe_hip_expand_crt_basis x 2; for d0, d1 ofhe_hip_ntt_inv,
//              ofhe_hip_approx_switch_crt_basis (mNegRlQHatInvModq / qInvModr),
//              ofhe_hip_switch_crt_basis R -> Q, ofhe_hip_ntt_fwd over Q|R; the
//              tensor product, ofhe_hip_ntt_inv, ofhe_hip_scale_and_round
// (bfvrns-leveledshe.cpp:168-408, dcrtpoly-impl.h:1178-1230, 1311-1358,
// 1413-1466, 1876-1955).  N = 2^10, Q = 2, R = 3 (HPS) / 2 (HPSPOVERQ), batch 2.
// The CRT tables are the true ones; the ScaleAndRound tables are random words
// and fractions (both sides read the same handle).  The reference's N = 8 known
// answer of SwitchCRTBasis (UnitTestBFVrnsCRTOperations.cpp:290-376) is carried
// as literal numbers.  No oracle is linked.  Prints "bfv: <n> failures".
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
// prod_{k != skip} ms[k] mod m
static uint64_t prod_mod(const std::vector<uint64_t>& ms, size_t skip, uint64_t m) {
    uint64_t r = 1 % m;
    for (size_t k = 0; k < ms.size(); k++)
        if (k != skip) r = mulmod(r, ms[k] % m, m);
    return r;
}
// (M / m_i)^-1 mod m_i and (M / m_i) mod t_j, [i][j] flattened
static void crt_tables(const std::vector<uint64_t>& ms, const std::vector<uint64_t>& ts, std::vector<uint64_t>& hinv,
                       std::vector<uint64_t>& hmod) {
    for (size_t i = 0; i < ms.size(); i++) {
        hinv.push_back(powmod(prod_mod(ms, i, ms[i]), ms[i] - 2, ms[i]));
        for (auto t : ts) hmod.push_back(prod_mod(ms, i, t));
    }
}

static int failures = 0;
static void expect(bool ok, const char* what, int tech = -1) {
    if (!ok) {
        failures++;
        std::printf("FAIL %s (technique %d)\n", what, tech);
    }
}
#define ABI(call) check((call), #call)

static void known_answer() {
    const std::vector<uint64_t> q{1152921504606846577ull, 1152921504606846097ull},
        r{1152921504606845777ull, 1152921504606845473ull};
    const std::vector<uint64_t> rl{955839852875274614ull,  186398073668078476ull, 710455872402389881ull,
                                   1065981546244475424ull, 1049296073052489283ull, 578396240339812092ull,
                                   26954876970280156ull,   1019223053257416912ull, 874592295621923164ull,
                                   585167928946466637ull,  612704504638527027ull, 551633899923050545ull,
                                   758002500979691774ull,  694035684451390662ull, 625796987487151016ull,
                                   96319544173820807ull};
    const std::vector<uint64_t> ql{805568738929329616ull, 1078766251747424582ull, 785656076316475932ull,
                                   599125608237504784ull, 541576441836927290ull,  152721755350883626ull,
                                   574857357780891061ull, 1081393409810468825ull, 434562805454153184ull,
                                   312761043978375123ull, 509951653046700586ull,  879239171041671808ull,
                                   385039618723450975ull, 638710747265582661ull,  246115869294473638ull,
                                   352338293114574371ull};
    auto PQ = params(16, q), PR = params(16, r);
    std::vector<uint64_t> hinv, hmod;
    crt_tables(r, q, hinv, hmod);
    BaseConverter r_to_q(*PR, *PQ, hinv, hmod);
    DCRTPolyHip x(PR, Format::COEFFICIENT);
    x.SetValues(rl, Format::COEFFICIENT);
    expect(r_to_q.SwitchCRTBasis(x, PQ).GetValues() == ql, "SwitchCRTBasis known answer, N = 8");
}

static void technique(BfvMult::Technique tech) {
    const uint32_t log_n = 10, m = 2u << log_n, n = m / 2, batch = 2, sq = 2, sr = tech == BfvMult::HPS ? 3 : 2;
    auto all = chain(m, sq + sr);
    std::vector<uint64_t> q(all.begin(), all.begin() + sq), r(all.begin() + sq, all.end());
    auto PQ = params(m, q), PR = params(m, r), PQR = params(m, all);
    HipManager* mgr = PQ->manager();
    std::vector<uint64_t> qhinv, qhmodr, rhinv, rhmodq, neg, qinvmodr;
    crt_tables(q, r, qhinv, qhmodr);
    crt_tables(r, q, rhinv, rhmodq);
    for (size_t i = 0; i < sq; i++) {  // mNegRlQHatInvModq, qInvModr (bfvrns-cryptoparameters.cpp:501-523)
        neg.push_back(q[i] - mulmod(prod_mod(r, r.size(), q[i]), qhinv[i], q[i]));
        for (auto rj : r) qinvmodr.push_back(powmod(q[i] % rj, rj - 2, rj));
    }
    std::mt19937_64 rng(2024 + tech);
    const bool out_is_q = tech == BfvMult::HPSPOVERQ;
    const auto& outs = out_is_q ? q : r;
    const size_t si = out_is_q ? sr : sq;
    std::vector<std::vector<uint64_t>> table;
    std::vector<double> frac;
    for (auto o : outs) {
        table.emplace_back();
        for (size_t i = 0; i <= si; i++) table.back().push_back(rng() % o);
    }
    for (size_t i = 0; i < si; i++) frac.push_back((double)(rng() >> 11) / 9007199254740992.0);
    BfvMult mult(tech, PQ, PR, PQR, qhinv, qhmodr, rhinv, rhmodq, table, frac, neg, qinvmodr);

    auto uniform = [&](const std::shared_ptr<DCRTParams>& P, Format f) {
        const auto& mods = P->Moduli();
        std::vector<uint64_t> v((size_t)batch * mods.size() * n);
        for (size_t i = 0; i < v.size(); i++) v[i] = rng() % mods[(i / n) % mods.size()];
        DCRTPolyHip x(P, f, batch);
        x.SetValues(v, f);
        return x;
    };
    DCRTPolyHip C0 = uniform(PQ, Format::EVALUATION), C1 = uniform(PQ, Format::EVALUATION),
                D0 = uniform(PQ, Format::EVALUATION), D1 = uniform(PQ, Format::EVALUATION);
    const auto c0_in = C0.GetValues(), d1_in = D1.GetValues();
    auto same = [&](const DeviceBuffer& d, const DCRTPolyHip& x) {
        std::vector<uint64_t> h(d.size());
        d.download(h.data());
        return h == x.GetValues();
    };
    const size_t qw = (size_t)sq * n, rw = (size_t)sr * n, qrw = qw + rw;

    // the single-step members against their C ABI calls
    DCRTPolyHip xc = uniform(PQ, Format::COEFFICIENT), xqr = uniform(PQR, Format::COEFFICIENT);
    DeviceBuffer sw(mgr, batch * rw), ex(mgr, batch * qrw), so(mgr, batch * (out_is_q ? qw : rw));
    ABI(ofhe_hip_switch_crt_basis(mult.QToR().handle(), xc.data(), sw.get(), batch, nullptr));
    expect(same(sw, mult.QToR().SwitchCRTBasis(xc, PR)), "SwitchCRTBasis", tech);
    for (const DCRTPolyHip* v : {&xc, &C0}) {
        ABI(ofhe_hip_expand_crt_basis(PQ->plan(), PR->plan(), mult.QToR().handle(),
                                      v->GetFormat() == Format::EVALUATION, v->data(), ex.get(), batch, nullptr));
        DCRTPolyHip got = ExpandCRTBasis(*v, PR, PQR, mult.QToR());
        expect(same(ex, got) && got.GetFormat() == Format::EVALUATION && got.GetParams() == PQR, "ExpandCRTBasis", tech);
    }
    ABI(ofhe_hip_scale_and_round(mult.Scale().handle(), xqr.data(), so.get(), batch, nullptr));
    expect(same(so, mult.Scale()(xqr, out_is_q ? PQ : PR)), "ScaleAndRound", tech);

    // EvalMult against the composition
    auto got = mult.EvalMult(C0, C1, D0, D1);
    expect(got.size() == 3 && got[0].GetFormat() == Format::COEFFICIENT && got[2].GetParams() == PQ, "EvalMult shape",
           tech);
    std::vector<DeviceBuffer> E, T;
    for (int k = 0; k < 4; k++) E.emplace_back(mgr, batch * qrw);
    for (int k = 0; k < 3; k++) T.emplace_back(mgr, batch * qrw);
    const DCRTPolyHip* in[4] = {&C0, &C1, &D0, &D1};
    for (int k = 0; k < 4; k++) {
        if (tech == BfvMult::HPS || k < 2) {
            ABI(ofhe_hip_expand_crt_basis(PQ->plan(), PR->plan(), mult.QToR().handle(), 1, in[k]->data(), E[k].get(),
                                          batch, nullptr));
            continue;
        }
        // FastExpandCRTBasisPloverQ between SetFormat(COEFFICIENT) and SetFormat(EVALUATION)
        DeviceBuffer coef(mgr, batch * qw), pr(mgr, batch * rw), pq(mgr, batch * qw);
        ABI(ofhe_hip_copy_device(mgr->ctx(), coef.get(), in[k]->data(), batch * qw * 8, nullptr));
        ABI(ofhe_hip_ntt_inv(PQ->plan(), coef.get(), batch, nullptr));
        ABI(ofhe_hip_approx_switch_crt_basis(mult.QToRNeg()->handle(), coef.get(), pr.get(), batch, nullptr));
        ABI(ofhe_hip_switch_crt_basis(mult.RToQ().handle(), pr.get(), pq.get(), batch, nullptr));
        for (uint32_t b = 0; b < batch; b++) {
            ABI(ofhe_hip_copy_device(mgr->ctx(), E[k].get() + b * qrw, pq.get() + b * qw, qw * 8, nullptr));
            ABI(ofhe_hip_copy_device(mgr->ctx(), E[k].get() + b * qrw + qw, pr.get() + b * rw, rw * 8, nullptr));
        }
        ABI(ofhe_hip_ntt_fwd(PQR->plan(), E[k].get(), batch, nullptr));
    }
    ABI(ofhe_hip_eval_mult_core(PQR->plan(), E[0].get(), E[1].get(), E[2].get(), E[3].get(), T[0].get(), T[1].get(),
                                T[2].get(), batch, nullptr));
    for (int k = 0; k < 3; k++) {
        ABI(ofhe_hip_ntt_inv(PQR->plan(), T[k].get(), batch, nullptr));
        DeviceBuffer s(mgr, batch * (out_is_q ? qw : rw)), o(mgr, batch * qw);
        ABI(ofhe_hip_scale_and_round(mult.Scale().handle(), T[k].get(), s.get(), batch, nullptr));
        if (tech == BfvMult::HPS) {
            ABI(ofhe_hip_switch_crt_basis(mult.RToQ().handle(), s.get(), o.get(), batch, nullptr));
            expect(same(o, got[k]), "EvalMult", tech);
        } else {
            expect(same(s, got[k]), "EvalMult", tech);
        }
    }
    expect(C0.GetValues() == c0_in && D1.GetValues() == d1_in, "inputs unchanged", tech);

    // argument checks of the adapter
    auto throws = [&](auto&& f) {
        try {
            f();
        } catch (const math_error&) {
            return true;
        }
        return false;
    };
    expect(throws([&] { mult.EvalMult(xc, C1, D0, D1); }), "COEFFICIENT-form input", tech);
    expect(throws([&] { mult.QToR().SwitchCRTBasis(C0, PR); }), "EVALUATION-form SwitchCRTBasis", tech);
    expect(throws([&] { mult.Scale()(C0, PR); }), "EVALUATION-form ScaleAndRound", tech);
    auto again = mult.EvalMult(C0, C1, D0, D1);
    expect(again[1].GetValues() == got[1].GetValues(), "usable after the errors", tech);
    mgr->sync();
}

int main() {
    try {
        known_answer();
        technique(BfvMult::HPS);
        technique(BfvMult::HPSPOVERQ);
    } catch (const std::exception& e) {
        std::printf("bfv failed: %s\n", e.what());
        return 1;
    }
    std::printf("bfv: %d failures\n", failures);
    return failures ? 1 : 0;
}
