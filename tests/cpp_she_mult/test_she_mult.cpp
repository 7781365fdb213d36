// CKKS / BGV multiplication through the C++ adapter (ofhe_dcrt.hpp):
// KeySwitchHybrid::EvalMult / EvalSquare / Relinearize / Rescale reproduce the
// words that the Python restatement (tests/she_mult_ref.py) wrote to the
// fixture given as argv[1].
//
// The fixture is a stream of little-endian 64-bit words:
//   magic, log_n, sq, sp, dnum, l, batch, scheme, t, levels
//   q[sq], roots, p[sp], roots
//   c0, c1, d0, d1 [batch][l][N]; two keys, each key_b, key_a [dnum][sq + sp][N]
//   mult0, mult1, square0, square1 [batch][l - levels][N]      EvalMult / EvalSquare under key 0
//   relin0, relin1 [batch][l][N]                               Relinearize((c0, c1, d0, d1), keys)
//   resc0, resc1 [batch][l - levels][N]                        Rescale((c0, c1), levels)
// Bad arguments must throw math_error.  Prints "she mult: <n> failures".
#include <cstdio>
#include <fstream>
#include <vector>

#include "../../upmem--openfhe_amd/host/ofhe_dcrt.hpp"

using namespace ofhe;

static int failures = 0;
static void expect(bool ok, const char* what) {
    if (!ok) {
        failures++;
        std::printf("FAIL %s\n", what);
    }
}

struct Reader {
    std::vector<uint64_t> w;
    size_t at = 0;
    uint64_t one() { return w.at(at++); }
    std::vector<uint64_t> take(size_t n) {
        if (at + n > w.size()) throw std::runtime_error("fixture too short");
        std::vector<uint64_t> v(w.begin() + at, w.begin() + at + n);
        at += n;
        return v;
    }
};

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: %s fixture\n", argv[0]);
        return 2;
    }
    try {
        Reader f;
        {
            std::ifstream in(argv[1], std::ios::binary | std::ios::ate);
            if (!in) throw std::runtime_error("cannot open the fixture");
            f.w.resize((size_t)in.tellg() / 8);
            in.seekg(0);
            in.read(reinterpret_cast<char*>(f.w.data()), f.w.size() * 8);
        }
        if (f.one() != 0x5348454d31ull) throw std::runtime_error("not a multiplication fixture");
        const uint32_t log_n = f.one(), sq = f.one(), sp = f.one(), dnum = f.one(), l = f.one(), batch = f.one();
        const int scheme = (int)f.one();
        const uint64_t t = f.one();
        const uint32_t levels = f.one();
        const uint32_t m = 2u << log_n, n = m / 2;
        auto q = f.take(sq), rq = f.take(sq), p = f.take(sp), rp = f.take(sp);
        std::vector<uint64_t> ql(q.begin(), q.begin() + l), rql(rq.begin(), rq.begin() + l), qp(q), rqp(rq);
        qp.insert(qp.end(), p.begin(), p.end());
        rqp.insert(rqp.end(), rp.begin(), rp.end());
        std::vector<uint64_t> qlow(ql.begin(), ql.end() - levels);
        auto PQ = std::make_shared<DCRTParams>(m, q, rq), PP = std::make_shared<DCRTParams>(m, p, rp),
             PQl = std::make_shared<DCRTParams>(m, ql, rql), PQP = std::make_shared<DCRTParams>(m, qp, rqp);
        KeySwitchHybrid ks(*PQ, *PP, dnum);
        auto poly = [&](const std::shared_ptr<DCRTParams>& P, uint32_t rows) {
            DCRTPolyHip x(P, Format::EVALUATION, rows);
            x.SetValues(f.take((size_t)rows * P->Towers() * n), Format::EVALUATION);
            return x;
        };
        DCRTPolyHip C0 = poly(PQl, batch), C1 = poly(PQl, batch), D0 = poly(PQl, batch), D1 = poly(PQl, batch);
        DCRTPolyHip B0 = poly(PQP, dnum), A0 = poly(PQP, dnum), B1 = poly(PQP, dnum), A1 = poly(PQP, dnum);
        const auto c0_in = C0.GetValues(), d1_in = D1.GetValues();
        const size_t low = (size_t)batch * (l - levels) * n, full = (size_t)batch * l * n;
        auto lowered_ok = [&](const DCRTPolyHip& x) {
            return x.GetParams()->Moduli() == qlow && x.Batch() == batch && x.GetFormat() == Format::EVALUATION;
        };

        const auto m0 = f.take(low), m1 = f.take(low), s0 = f.take(low), s1 = f.take(low);
        auto mult = ks.EvalMult(C0, C1, D0, D1, B0, A0, scheme, t, levels);
        expect(mult.first.GetValues() == m0 && mult.second.GetValues() == m1, "EvalMult");
        expect(lowered_ok(mult.first) && lowered_ok(mult.second), "EvalMult result params");
        auto sqr = ks.EvalSquare(C0, C1, B0, A0, scheme, t, levels);
        expect(sqr.first.GetValues() == s0 && sqr.second.GetValues() == s1, "EvalSquare");
        expect(lowered_ok(sqr.first), "EvalSquare result params");

        const auto r0 = f.take(full), r1 = f.take(full);
        std::vector<KeySwitchHybrid::RelinKey> keys{{&B0, &A0}, {&B1, &A1}};
        auto rel = ks.Relinearize({&C0, &C1, &D0, &D1}, keys, t);
        expect(rel.first.GetValues() == r0 && rel.second.GetValues() == r1, "Relinearize");
        expect(rel.first.GetParams() == PQl && rel.second.Batch() == batch, "Relinearize result params");

        const auto e0 = f.take(low), e1 = f.take(low);
        auto res = ks.Rescale({&C0, &C1}, scheme, t, levels);
        expect(res.size() == 2 && res[0].GetValues() == e0 && res[1].GetValues() == e1, "Rescale");
        expect(lowered_ok(res[0]) && lowered_ok(res[1]), "Rescale result params");
        expect(C0.GetValues() == c0_in && D1.GetValues() == d1_in, "inputs unchanged");
        expect(f.at == f.w.size(), "the whole fixture was read");

        // argument checks of the adapter and of the entry points behind it
        auto throws = [&](auto&& fn) {
            try {
                fn();
            } catch (const math_error&) {
                return true;
            }
            return false;
        };
        DCRTPolyHip coeff(PQl, Format::COEFFICIENT, batch), wide(PQP, Format::EVALUATION, batch),
            other(PQl, Format::EVALUATION, batch + 1);
        expect(throws([&] { ks.EvalMult(coeff, C1, D0, D1, B0, A0, scheme, t, levels); }), "COEFFICIENT operand");
        expect(throws([&] { ks.EvalMult(C0, C1, D0, other, B0, A0, scheme, t, levels); }), "batch mismatch");
        expect(throws([&] { ks.EvalMult(C0, C1, D0, D1, C0, A0, scheme, t, levels); }), "key over the wrong basis");
        expect(throws([&] { ks.EvalSquare(wide, wide, B0, A0, scheme, t, levels); }), "more towers than Q");
        expect(throws([&] { ks.EvalSquare(C0, C1, B0, A0, scheme, t, l); }), "levels >= towers");
        expect(throws([&] { ks.EvalSquare(C0, C1, B0, A0, scheme, t ? 0 : 3, levels); }), "t against the scheme");
        expect(throws([&] { ks.EvalSquare(C0, C1, B0, A0, OFHE_SHE_BGV, q[0], levels); }), "t not invertible");
        expect(throws([&] { ks.Relinearize({&C0, &C1}, {}, t); }), "two elements");
        expect(throws([&] { ks.Relinearize({&C0, &C1, &D0}, keys, t); }), "key count");
        expect(throws([&] { ks.Relinearize({&C0, &C1, &coeff}, {keys[0]}, t); }), "COEFFICIENT element");
        expect(throws([&] { ks.Rescale({}, scheme, t, levels); }), "no elements");
        expect(throws([&] { ks.Rescale({&C0}, scheme, t, 0); }), "levels 0");
        expect(throws([&] { ks.Rescale({&C0}, scheme, t, l); }), "levels >= towers, Rescale");
        // still usable afterwards
        expect(ks.EvalMult(C0, C1, D0, D1, B0, A0, scheme, t, levels).first.GetValues() == m0, "usable after the errors");
        PQ->manager()->sync();
    } catch (const std::exception& e) {
        std::printf("she mult failed: %s\n", e.what());
        return 1;
    }
    std::printf("she mult: %d failures\n", failures);
    return failures ? 1 : 0;
}
