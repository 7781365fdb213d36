// BV key switching with a digit size through the C++ adapter (ofhe_dcrt.hpp):
// KeySwitchBV::EvalKeySwitchPrecomputeCore / EvalFastKeySwitchCore /
// KeySwitchCore / KeySwitchInPlace reproduce the words that the Python
// restatement (tests/bv_digits_ref.py) wrote to the fixture given as argv[1].
//
// The fixture is a stream of little-endian 64-bit words:
//   magic, log_n, T, l, batch, digitSize
//   q[T], roots
//   c, add0, add1 [batch][l][N]; key_b, key_a [digits of Q][T][N]
//   digits [batch][digits of Ql][l][N]
//   ct0, ct1 [batch][l][N]                       KeySwitchCore(c)
//   two0 [batch][l][N]                           KeySwitchInPlace((add0, c)): (two0, ct1)
//   three0, three1 [batch][l][N]                 KeySwitchInPlace((add0, add1, c))
// Bad arguments must throw math_error.  Prints "bv: <n> failures".
//
// "count <file>" needs no device: the file holds magic, the number of cases and
// per case T, towers, digitSize, the expected DigitCount and q[T]; prints
// "bv count: <n> failures".
#include <cstdio>
#include <cstring>
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
    explicit Reader(const char* path) {
        std::ifstream in(path, std::ios::binary | std::ios::ate);
        if (!in) throw std::runtime_error("cannot open the fixture");
        w.resize((size_t)in.tellg() / 8);
        in.seekg(0);
        in.read(reinterpret_cast<char*>(w.data()), w.size() * 8);
    }
    uint64_t one() { return w.at(at++); }
    std::vector<uint64_t> take(size_t n) {
        if (at + n > w.size()) throw std::runtime_error("fixture too short");
        std::vector<uint64_t> v(w.begin() + at, w.begin() + at + n);
        at += n;
        return v;
    }
};

template <class F>
static bool throws(F&& fn) {
    try {
        fn();
    } catch (const math_error&) {
        return true;
    }
    return false;
}

static int count_mode(const char* path) {
    Reader f(path);
    if (f.one() != 0x4256434e54ull) throw std::runtime_error("not a digit-count fixture");
    const uint64_t cases = f.one();
    for (uint64_t k = 0; k < cases; k++) {
        const uint32_t T = f.one(), towers = f.one(), r = f.one(), want = f.one();
        const auto q = f.take(T);
        if (KeySwitchBV::DigitCount(q, towers, r) != want) {
            failures++;
            std::printf("FAIL DigitCount case %llu\n", (unsigned long long)k);
        }
    }
    expect(f.at == f.w.size(), "the whole fixture was read");
    const std::vector<uint64_t> q{(1ull << 40) - 87, (1ull << 30) - 35};
    expect(throws([&] { KeySwitchBV::DigitCount(q, 2, 31); }), "digitSize 31");
    expect(throws([&] { KeySwitchBV::DigitCount(q, 3, 10); }), "more towers than moduli");
    expect(throws([&] { KeySwitchBV::DigitCount(q, 0, 10); }), "no towers");
    std::printf("bv count: %d failures\n", failures);
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: %s fixture | count fixture\n", argv[0]);
        return 2;
    }
    try {
        if (argc >= 3 && !std::strcmp(argv[1], "count")) return count_mode(argv[2]);
        Reader f(argv[1]);
        if (f.one() != 0x4256444947ull) throw std::runtime_error("not a BV fixture");
        const uint32_t log_n = f.one(), T = f.one(), l = f.one(), batch = f.one(), r = f.one();
        const uint32_t m = 2u << log_n, n = m / 2;
        auto q = f.take(T), rq = f.take(T);
        std::vector<uint64_t> ql(q.begin(), q.begin() + l), rql(rq.begin(), rq.begin() + l);
        auto PQ = std::make_shared<DCRTParams>(m, q, rq), PQl = std::make_shared<DCRTParams>(m, ql, rql);
        const uint32_t nk = KeySwitchBV::DigitCount(q, T, r), nd = KeySwitchBV::DigitCount(q, l, r);
        KeySwitchBV ks(PQ, r);
        auto poly = [&](const std::shared_ptr<DCRTParams>& P, uint32_t rows) {
            DCRTPolyHip x(P, Format::EVALUATION, rows);
            x.SetValues(f.take((size_t)rows * P->Towers() * n), Format::EVALUATION);
            return x;
        };
        DCRTPolyHip C = poly(PQl, batch), A0 = poly(PQl, batch), A1 = poly(PQl, batch);
        KeySwitchBV::Key key{poly(PQ, nk), poly(PQ, nk)};
        const auto c_in = C.GetValues();
        const size_t full = (size_t)batch * l * n;
        const auto want_d = f.take(full * nd), ct0 = f.take(full), ct1 = f.take(full), two0 = f.take(full),
                   three0 = f.take(full), three1 = f.take(full);
        expect(f.at == f.w.size(), "the whole fixture was read");

        auto d = ks.EvalKeySwitchPrecomputeCore(C);
        expect(d.n_digits == nd && d.batch == batch && d.poly.GetValues() == want_d, "EvalKeySwitchPrecomputeCore");
        auto fast = ks.EvalFastKeySwitchCore(d, key, PQl);
        expect(fast.first.GetValues() == ct0 && fast.second.GetValues() == ct1, "EvalFastKeySwitchCore");
        auto core = ks.KeySwitchCore(C, key);
        expect(core.first.GetValues() == ct0 && core.second.GetValues() == ct1, "KeySwitchCore");
        expect(core.first.GetParams() == PQl && core.second.Batch() == batch &&
                   core.first.GetFormat() == Format::EVALUATION, "KeySwitchCore result params");
        expect(C.GetValues() == c_in, "input unchanged");
        std::vector<DCRTPolyHip> two;
        two.push_back(A0);
        two.push_back(C);
        ks.KeySwitchInPlace(two, key);
        expect(two.size() == 2 && two[0].GetValues() == two0 && two[1].GetValues() == ct1, "KeySwitchInPlace, two elements");
        std::vector<DCRTPolyHip> three;
        three.push_back(A0);
        three.push_back(A1);
        three.push_back(C);
        ks.KeySwitchInPlace(three, key);
        expect(three.size() == 2 && three[0].GetValues() == three0 && three[1].GetValues() == three1,
               "KeySwitchInPlace, three elements");

        // argument checks of the adapter
        DCRTPolyHip coeff(PQl, Format::COEFFICIENT, batch), other(PQl, Format::EVALUATION, batch + 1);
        KeySwitchBV low(PQl, r);  // its keys would be over Ql: C's level is fine, a polynomial over Q is above it
        DCRTPolyHip top(PQ, Format::EVALUATION, batch);
        KeySwitchBV::Key few{DCRTPolyHip(PQ, Format::EVALUATION, nd - 1), DCRTPolyHip(PQ, Format::EVALUATION, nd - 1)};
        KeySwitchBV::Key wrong{DCRTPolyHip(PQl, Format::EVALUATION, nk), DCRTPolyHip(PQl, Format::EVALUATION, nk)};
        expect(throws([&] { KeySwitchBV(PQ, 31); }), "digitSize 31");
        expect(throws([&] { ks.KeySwitchCore(coeff, key); }), "COEFFICIENT input");
        expect(throws([&] { ks.EvalKeySwitchPrecomputeCore(coeff); }), "COEFFICIENT input, precompute");
        if (l < T) expect(throws([&] { low.KeySwitchCore(top, wrong); }), "a level above the key's");
        expect(throws([&] { ks.KeySwitchCore(C, few); }), "too few key digits");
        if (l < T) expect(throws([&] { ks.KeySwitchCore(C, wrong); }), "key over the wrong basis");
        expect(throws([&] { ks.EvalFastKeySwitchCore(d, few, PQl); }), "too few key digits, fast core");
        if (l < T) expect(throws([&] { ks.EvalFastKeySwitchCore(d, key, PQ); }), "paramsQl of another level");
        std::vector<DCRTPolyHip> bad;
        bad.push_back(A0);
        expect(throws([&] { ks.KeySwitchInPlace(bad, key); }), "one element");
        bad.push_back(other);
        expect(throws([&] { ks.KeySwitchInPlace(bad, key); }), "batch mismatch");
        // still usable afterwards
        expect(ks.KeySwitchCore(C, key).first.GetValues() == ct0, "usable after the errors");
        PQ->manager()->sync();
    } catch (const std::exception& e) {
        std::printf("bv failed: %s\n", e.what());
        return 1;
    }
    std::printf("bv: %d failures\n", failures);
    return failures ? 1 : 0;
}
