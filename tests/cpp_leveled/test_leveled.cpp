// HPSPOVERQLEVELED with dropped levels through the C++ adapter (ofhe_dcrt.hpp):
// BfvLevel::EvalMult / EvalSquare / Relinearize / ScaleAndRoundExpand and
// DCRTPolyHip::ExpandCRTBasisQlHat against the same steps through the earlier
// public C ABI calls, on the same device data, one sub-test per level:
//   EvalMult     ofhe_hip_ntt_inv, ofhe_hip_scale_and_round (the drop),
//                ofhe_hip_expand_crt_basis; for d0, d1 ofhe_hip_ntt_inv,
//                ofhe_hip_approx_switch_crt_basis (mNegRlQHatInvModq(l) / qInvModr,
//                all size_q sources), ofhe_hip_switch_crt_basis R_l -> Q_l,
//                ofhe_hip_ntt_fwd over Q_l|R_l; ofhe_hip_eval_mult_core,
//                ofhe_hip_ntt_inv, ofhe_hip_scale_and_round, then the lift as
//                ofhe_hip_modmul_scalar into a zeroed polynomial over Q
//   Relinearize  ofhe_hip_ntt_inv, the drop, ofhe_hip_ntt_fwd, ofhe_hip_ks_core at
//                l + 1 towers, the lift, ofhe_hip_modadd_vv
// (bfvrns-leveledshe.cpp:235-274, 367-382, 845-899, dcrtpoly-impl.h:1413-1466,
// 1514-1534).  N = 2^10, Q = R = 4, P = 2, dnum = 2, batch 2.  The CRT tables and
// QlHatModq are the true ones; the ScaleAndRound tables are random words and
// fractions (both sides read the same handles).  No oracle is linked.
// `test_leveled_bin levels` prints FindLevelsToDrop on a grid and touches no device.
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
static void expect(bool ok, const char* what, int l = -1) {
    if (!ok) {
        failures++;
        std::printf("FAIL %s (l = %d)\n", what, l);
    }
}
#define ABI(call) check((call), #call)

static BfvLevelTables level_tables(const std::vector<uint64_t>& q, const std::vector<uint64_t>& r, uint32_t l,
                                   std::mt19937_64& rng) {
    const size_t sq = q.size(), L = l + 1;
    const std::vector<uint64_t> ql(q.begin(), q.begin() + L), rl(r.begin(), r.begin() + L);
    BfvLevelTables T;
    T.l = l;
    crt_tables(ql, rl, T.QlHatInvModq, T.QlHatModr);
    crt_tables(rl, ql, T.RlHatInvModr, T.RlHatModq);
    for (size_t i = 0; i < sq; i++) {  // mNegRlQHatInvModq(l) with the full Q, qInvModr (bfvrns-cryptoparameters.cpp:501-523)
        const uint64_t qhinv = powmod(prod_mod(q, i, q[i]), q[i] - 2, q[i]);
        T.negRlQHatInvModq.push_back(q[i] - mulmod(prod_mod(rl, rl.size(), q[i]), qhinv, q[i]));
        for (auto rj : rl) T.qInvModr.push_back(powmod(q[i] % rj, rj - 2, rj));
    }
    for (size_t i = 0; i < L; i++) {  // QlHatModq(l)[i] = (Q / Q_l) mod q_i (:621-631)
        uint64_t v = 1;
        for (size_t k = L; k < sq; k++) v = mulmod(v, q[k] % q[i], q[i]);
        T.QlHatModq.push_back(v);
    }
    auto random_sr = [&](size_t si, std::vector<std::vector<uint64_t>>& table, std::vector<double>& frac) {
        for (size_t j = 0; j < L; j++) {
            table.emplace_back();
            for (size_t i = 0; i <= si; i++) table.back().push_back(rng() % ql[j]);
        }
        for (size_t i = 0; i < si; i++) frac.push_back((double)(rng() >> 11) / 9007199254740992.0);
    };
    if (L < sq) random_sr(sq - L, T.QlQHatInvModqDivqModq, T.QlQHatInvModqDivqFrac);
    random_sr(L, T.tQlSlHatInvModsDivsModq, T.tQlSlHatInvModsDivsFrac);
    return T;
}

static void level(uint32_t l) {
    const uint32_t log_n = 10, m = 2u << log_n, n = m / 2, batch = 2, sq = 4, sp = 2, dnum = 2, L = l + 1;
    auto all = chain(m, 2 * sq + sp);
    const std::vector<uint64_t> q(all.begin(), all.begin() + sq), r(all.begin() + sq, all.begin() + 2 * sq),
        p(all.begin() + 2 * sq, all.end());
    std::vector<uint64_t> qp(q);
    qp.insert(qp.end(), p.begin(), p.end());
    auto PQ = params(m, q), PR = params(m, r), PP = params(m, p), PQP = params(m, qp);
    HipManager* mgr = PQ->manager();
    std::mt19937_64 rng(77 + l);
    const BfvLevelTables T = level_tables(q, r, l, rng);
    int built = 0;
    auto tables = [&](uint32_t) {
        built++;
        return T;
    };
    auto lv = BfvLevelCache::get(PQ, PR, 65537, l, tables);
    expect(BfvLevelCache::get(PQ, PR, 65537, l, tables) == lv && built == 1, "the level is cached", l);
    const bool dropped = L < sq;
    expect((lv->Drop() != nullptr) == dropped && lv->Level() == l && lv->ParamsQl()->Towers() == L, "level shape", l);
    auto PQl = lv->ParamsQl(), PRl = lv->ParamsRl(), PQlRl = lv->ParamsQlRl();

    auto uniform = [&](const std::shared_ptr<DCRTParams>& P, Format f, uint32_t b) {
        const auto& mods = P->Moduli();
        std::vector<uint64_t> v((size_t)b * mods.size() * n);
        for (size_t i = 0; i < v.size(); i++) v[i] = rng() % mods[(i / n) % mods.size()];
        DCRTPolyHip x(P, f, b);
        x.SetValues(v, f);
        return x;
    };
    auto same = [&](const DeviceBuffer& d, const DCRTPolyHip& x) {
        std::vector<uint64_t> h(d.size());
        d.download(h.data());
        return h == x.GetValues();
    };
    const size_t qw = (size_t)sq * n, lw = (size_t)L * n, qrw = 2 * lw;
    // ExpandCRTBasisQlHat as ofhe_hip_modmul_scalar into a zeroed polynomial over Q
    auto lift = [&](const uint64_t* x, DeviceBuffer& out) {
        DeviceBuffer t(mgr, batch * lw);
        ABI(ofhe_hip_modmul_scalar(PQl->plan(), x, T.QlHatModq.data(), t.get(), batch, nullptr));
        ABI(ofhe_hip_zero(mgr->ctx(), out.get(), batch * qw * 8, nullptr));
        for (uint32_t b = 0; b < batch; b++)
            ABI(ofhe_hip_copy_device(mgr->ctx(), out.get() + b * qw, t.get() + b * lw, lw * 8, nullptr));
    };
    // x over Q, evaluation form -> coefficient form over Q_l (the drop)
    auto to_ql = [&](const DCRTPolyHip& x, DeviceBuffer& out) {
        DeviceBuffer coef(mgr, batch * qw);
        ABI(ofhe_hip_copy_device(mgr->ctx(), coef.get(), x.data(), batch * qw * 8, nullptr));
        if (x.GetFormat() == Format::EVALUATION) ABI(ofhe_hip_ntt_inv(PQ->plan(), coef.get(), batch, nullptr));
        if (dropped)
            ABI(ofhe_hip_scale_and_round(lv->Drop()->handle(), coef.get(), out.get(), batch, nullptr));
        else
            ABI(ofhe_hip_copy_device(mgr->ctx(), out.get(), coef.get(), batch * qw * 8, nullptr));
    };

    // DCRTPolyHip::ExpandCRTBasisQlHat and ScaleAndRoundExpand
    {
        DCRTPolyHip x = uniform(PQl, Format::EVALUATION, batch), y = uniform(PQlRl, Format::COEFFICIENT, batch);
        DeviceBuffer want(mgr, batch * qw), mid(mgr, batch * lw);
        lift(x.data(), want);
        x.ExpandCRTBasisQlHat(*lv);
        expect(same(want, x) && x.GetParams() == PQ && x.GetFormat() == Format::EVALUATION, "ExpandCRTBasisQlHat", l);
        ABI(ofhe_hip_scale_and_round(lv->Scale().handle(), y.data(), mid.get(), batch, nullptr));
        lift(mid.get(), want);
        expect(same(want, lv->ScaleAndRoundExpand(y)), "ScaleAndRoundExpand", l);
    }

    // EvalMult against the composition
    DCRTPolyHip C0 = uniform(PQ, Format::EVALUATION, batch), C1 = uniform(PQ, Format::EVALUATION, batch),
                D0 = uniform(PQ, Format::EVALUATION, batch), D1 = uniform(PQ, Format::EVALUATION, batch);
    const auto c0_in = C0.GetValues(), d1_in = D1.GetValues();
    auto got = lv->EvalMult(C0, C1, D0, D1);
    expect(got.size() == 3 && got[0].GetFormat() == Format::COEFFICIENT && got[2].GetParams() == PQ, "EvalMult shape", l);
    std::vector<DeviceBuffer> E, P3;
    for (int k = 0; k < 4; k++) E.emplace_back(mgr, batch * qrw);
    for (int k = 0; k < 3; k++) P3.emplace_back(mgr, batch * qrw);
    const DCRTPolyHip* in[4] = {&C0, &C1, &D0, &D1};
    for (int k = 0; k < 2; k++) {
        DeviceBuffer xl(mgr, batch * lw);
        to_ql(*in[k], xl);
        ABI(ofhe_hip_expand_crt_basis(PQl->plan(), PRl->plan(), lv->QlToRl().handle(), 0, xl.get(), E[k].get(), batch,
                                      nullptr));
    }
    for (int k = 2; k < 4; k++) {
        // FastExpandCRTBasisPloverQ between SetFormat(COEFFICIENT) and SetFormat(EVALUATION)
        DeviceBuffer coef(mgr, batch * qw), pr(mgr, batch * lw), pq(mgr, batch * lw);
        ABI(ofhe_hip_copy_device(mgr->ctx(), coef.get(), in[k]->data(), batch * qw * 8, nullptr));
        ABI(ofhe_hip_ntt_inv(PQ->plan(), coef.get(), batch, nullptr));
        ABI(ofhe_hip_approx_switch_crt_basis(lv->QToRlNeg().handle(), coef.get(), pr.get(), batch, nullptr));
        ABI(ofhe_hip_switch_crt_basis(lv->RlToQl().handle(), pr.get(), pq.get(), batch, nullptr));
        for (uint32_t b = 0; b < batch; b++) {
            ABI(ofhe_hip_copy_device(mgr->ctx(), E[k].get() + b * qrw, pq.get() + b * lw, lw * 8, nullptr));
            ABI(ofhe_hip_copy_device(mgr->ctx(), E[k].get() + b * qrw + lw, pr.get() + b * lw, lw * 8, nullptr));
        }
        ABI(ofhe_hip_ntt_fwd(PQlRl->plan(), E[k].get(), batch, nullptr));
    }
    ABI(ofhe_hip_eval_mult_core(PQlRl->plan(), E[0].get(), E[1].get(), E[2].get(), E[3].get(), P3[0].get(),
                                P3[1].get(), P3[2].get(), batch, nullptr));
    for (int k = 0; k < 3; k++) {
        ABI(ofhe_hip_ntt_inv(PQlRl->plan(), P3[k].get(), batch, nullptr));
        DeviceBuffer s(mgr, batch * lw), o(mgr, batch * qw);
        ABI(ofhe_hip_scale_and_round(lv->Scale().handle(), P3[k].get(), s.get(), batch, nullptr));
        lift(s.get(), o);
        expect(same(o, got[k]), "EvalMult", l);
    }
    expect(C0.GetValues() == c0_in && D1.GetValues() == d1_in, "inputs unchanged", l);
    auto sq2 = lv->EvalSquare(C0, C1), mm = lv->EvalMult(C0, C1, C0, C1);
    expect(sq2[1].GetValues() == mm[1].GetValues() && sq2[2].GetValues() == mm[2].GetValues(), "EvalSquare", l);

    // Relinearize against the composition, 3 and 2 elements, both formats
    auto ks = KsCache::get(*PQ, *PP, dnum);
    DCRTPolyHip KB = uniform(PQP, Format::EVALUATION, dnum), KA = uniform(PQP, Format::EVALUATION, dnum);
    for (int count : {3, 2}) {
        for (Format f : {Format::EVALUATION, Format::COEFFICIENT}) {
            DCRTPolyHip X0 = uniform(PQ, f, batch), X1 = uniform(PQ, f, batch), X2 = uniform(PQ, f, batch);
            std::vector<const DCRTPolyHip*> cv{&X0, &X1};
            if (count == 3) cv.push_back(&X2);
            auto res = lv->Relinearize(cv, KB, KA, ks->handle());
            DeviceBuffer xl(mgr, batch * lw), a0(mgr, batch * lw), a1(mgr, batch * lw), l0(mgr, batch * qw),
                l1(mgr, batch * qw);
            to_ql(*cv.back(), xl);
            ABI(ofhe_hip_ntt_fwd(PQl->plan(), xl.get(), batch, nullptr));
            ABI(ofhe_hip_ks_core(ks->handle(), L, xl.get(), KB.data(), KA.data(), a0.get(), a1.get(), 0, batch,
                                 nullptr));
            lift(a0.get(), l0);
            lift(a1.get(), l1);
            DCRTPolyHip E0(X0), E1(X1);
            E0.SetFormat(Format::EVALUATION);
            E1.SetFormat(Format::EVALUATION);
            ABI(ofhe_hip_modadd_vv(PQ->plan(), E0.data(), l0.get(), l0.get(), batch, nullptr));
            if (count == 3) ABI(ofhe_hip_modadd_vv(PQ->plan(), E1.data(), l1.get(), l1.get(), batch, nullptr));
            expect(same(l0, res.first) && same(l1, res.second) && res.first.GetFormat() == Format::EVALUATION,
                   count == 3 ? "Relinearize, 3 elements" : "Relinearize, 2 elements", l);
        }
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
    DCRTPolyHip xc = uniform(PQ, Format::COEFFICIENT, batch);
    expect(throws([&] { lv->EvalMult(xc, C1, D0, D1); }), "COEFFICIENT-form input", l);
    expect(throws([&] { xc.ExpandCRTBasisQlHat(*lv); }) || !dropped, "ExpandCRTBasisQlHat over another basis", l);
    expect(throws([&] { lv->Relinearize({&C0}, KB, KA, ks->handle()); }), "one element", l);
    expect(throws([&] { lv->Relinearize({&C0, &xc}, KB, KA, ks->handle()); }), "mixed formats", l);
    auto again = lv->EvalMult(C0, C1, D0, D1);
    expect(again[1].GetValues() == got[1].GetValues(), "usable after the errors", l);
    mgr->sync();
}

// FindLevelsToDrop on the grid tests/test_cpp_leveled.py compares with bfv_tables.levels_to_drop
static void levels_grid() {
    for (uint32_t sizeQ : {3u, 8u, 16u})
        for (double bits : {30.0, 50.0, 60.0})
            for (uint32_t log_n : {11u, 14u, 16u})
                for (uint64_t t : {17ull, 65537ull})
                    for (int hybrid = 0; hybrid < 2; hybrid++)
                        for (int ks = 0; ks < 2; ks++)
                            for (uint32_t depth = 0; depth < 10; depth += 3) {
                                LevelsToDropParams cp;
                                cp.plaintextModulus = t;
                                cp.ringDimension = 1u << log_n;
                                cp.hybrid = hybrid != 0;
                                cp.numPerPartQ = 2;
                                cp.numPartQ = 3;
                                cp.sizeQ = sizeQ;
                                std::printf("%u %g %u %llu %d %d %u %u\n", sizeQ, bits, log_n, (unsigned long long)t, hybrid,
                                            ks, depth, FindLevelsToDrop(depth, cp, bits, ks != 0));
                            }
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "levels")) {
        levels_grid();
        return 0;
    }
    try {
        for (uint32_t l : {0u, 1u, 3u}) level(l);
    } catch (const std::exception& e) {
        std::printf("leveled failed: %s\n", e.what());
        return 1;
    }
    std::printf("leveled: %d failures\n", failures);
    return failures ? 1 : 0;
}
