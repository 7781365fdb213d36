// The refusals of the C++ adapter (ofhe_dcrt.hpp) and of the two hook helpers
// that share its code (hooks::converter, hooks::PutEvalKey), pinned: the
// program builds the smallest object of every adapter class, makes one
// refused call per case and prints
//   case name <TAB> exception class <TAB> what()
// per case ("NO THROW" where nothing was thrown, which fails the run).  The
// pytest compares the output byte for byte with
// tests/golden/adapter_messages.txt, recorded from the headers as they were
// before the adapter's rules were given one owner each.
//
// Every case is refused on the host, by the adapter's own checks or by the
// C ABI's argument validation, before any kernel is launched; the objects
// the cases are made on hold zeros or arbitrary table words (the create
// functions reduce tables, they do not verify them).
//
// Throw statements of ofhe_dcrt.hpp without a case (line numbers of the
// header the golden file was recorded from):
//   679   DCRTPolyHip::Save "stream write failed": needs a failing stream
//   1444  KeySwitchHybrid::lowered "Removing last element ...": both callers
//         (Rescale, mult) refuse levels >= towers themselves first, so no
//         argument reaches it
// Line 75 (check(): a non-zero C ABI status) is covered where the ABI refuses
// an argument on the host (a bad modulus, an even automorphism index, a
// handle made without the tables a call needs, a NULL engine); ABI statuses
// that only a failed allocation, copy or launch would produce have no case.
// Of the hooks header only converter's and PutEvalKey's own throws are
// pinned here; the other hooks' messages are not.
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../upmem--openfhe_amd/host/ofhe_openfhe_hooks.hpp"

using namespace ofhe;
typedef unsigned __int128 u128;

static int g_silent = 0;
template <class F>
static void refuse(const std::string& name, F&& f) {
    const char* cls = "NO THROW";
    std::string what;
    try {
        f();
        g_silent++;
    } catch (const deserialize_error& e) {
        cls = "deserialize_error", what = e.what();
    } catch (const not_implemented_error& e) {
        cls = "not_implemented_error", what = e.what();
    } catch (const math_error& e) {
        cls = "math_error", what = e.what();
    }
    std::printf("%s\t%s\t%s\n", name.c_str(), cls, what.c_str());
}

// --- small host number theory for the parameters ---
static uint64_t mulmod(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)((u128)a * b % q); }
static uint64_t powmod(uint64_t b, uint64_t e, uint64_t q) {
    uint64_t r = 1 % q;
    for (b %= q; e; e >>= 1, b = mulmod(b, b, q))
        if (e & 1) r = mulmod(r, b, q);
    return r;
}
static bool is_prime(uint64_t n) {
    for (uint64_t p : {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37})
        if (n % p == 0) return n == p;
    uint64_t d = n - 1;
    int s = 0;
    while (!(d & 1)) d >>= 1, s++;
    for (uint64_t a : {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37}) {
        uint64_t x = powmod(a, d, n);
        if (x == 1 || x == n - 1) continue;
        bool comp = true;
        for (int r = 1; r < s && comp; r++) {
            x = mulmod(x, x, n);
            if (x == n - 1) comp = false;
        }
        if (comp) return false;
    }
    return true;
}
// `count` primes = 1 mod m, downwards from 2^bits, and a primitive m-th root of each
static void chain(unsigned bits, uint64_t m, size_t count, std::vector<uint64_t>& q, std::vector<uint64_t>& r) {
    for (uint64_t x = (1ull << bits) + 1; q.size() < count;) {
        do x -= m;
        while (!is_prime(x));
        uint64_t psi = 0;
        for (uint64_t c = 2;; c++) {
            psi = powmod(c, (x - 1) / m, x);
            if (powmod(psi, m / 2, x) == x - 1) break;
        }
        q.push_back(x);
        r.push_back(psi);
    }
}
static std::vector<uint64_t> cut(const std::vector<uint64_t>& v, size_t a, size_t n) {
    return std::vector<uint64_t>(v.begin() + a, v.begin() + a + n);
}
static std::vector<uint64_t> cat(std::vector<uint64_t> a, const std::vector<uint64_t>& b) {
    a.insert(a.end(), b.begin(), b.end());
    return a;
}
typedef std::shared_ptr<DCRTParams> Params;
typedef std::vector<uint64_t> Words;
static const Format EV = Format::EVALUATION, CO = Format::COEFFICIENT;

// the hooks' tower type: what hooks::view reads of the reference's PolyImpl
struct TowerParams {
    struct Int {
        uint64_t v;
        uint64_t ConvertToInt() const { return v; }
    } q, psi;
    uint32_t n;
    const Int& GetModulus() const { return q; }
    const Int& GetRootOfUnity() const { return psi; }
    uint32_t GetRingDimension() const { return n; }
};
struct Tower {
    std::shared_ptr<TowerParams> p;
    std::vector<uint64_t> w;
    Format f;
    const std::shared_ptr<TowerParams>& GetParams() const { return p; }
    Format GetFormat() const { return f; }
    uint64_t& operator[](size_t i) { return w[i]; }
    const uint64_t& operator[](size_t i) const { return w[i]; }
};
typedef std::vector<Tower> Towers;
static Towers towers(uint32_t n, const Words& q, const Words& r, Format f) {
    Towers t;
    for (size_t i = 0; i < q.size(); i++)
        t.push_back(Tower{std::make_shared<TowerParams>(TowerParams{{q[i]}, {r[i]}, n}), Words(n, 0), f});
    return t;
}

static void poly_cases() {
    const uint32_t m = 16;
    Words q, r, q32, r32;
    chain(22, m, 2, q, r);
    chain(22, 32, 1, q32, r32);
    auto P1 = std::make_shared<DCRTParams>(m, cut(q, 0, 1), cut(r, 0, 1));
    auto P1b = std::make_shared<DCRTParams>(m, cut(q, 1, 1), cut(r, 1, 1));
    auto P2 = std::make_shared<DCRTParams>(m, q, r);
    auto P32 = std::make_shared<DCRTParams>(32, q32, r32);
    HipManager* mgr = P1->manager();

    refuse("PlanCache::get empty", [&] { PlanCache::get(0, 3, {}, {}); });
    refuse("PlanCache::get sizes", [&] { PlanCache::get(0, 3, q, cut(r, 0, 1)); });
    {
        Staging st(mgr, 8);
        Words h(16);
        std::vector<const uint64_t*> src{h.data(), h.data() + 8};
        std::vector<uint64_t*> dst{h.data(), h.data() + 8};
        refuse("Staging::gather", [&] { st.gather(src, 8); });
        refuse("Staging::scatter", [&] { st.scatter(dst, 8); });
        refuse("Staging::put_towers", [&] { st.put_towers(src, 8); });
        refuse("Staging::get_towers", [&] { st.get_towers(dst, 8); });
    }
    refuse("DCRTParams order 2", [&] { DCRTParams(2, q, r); });
    refuse("DCRTParams order 12", [&] { DCRTParams(12, q, r); });
    refuse("DCRTParams no roots", [&] { DCRTParams(m, q, {}); });
    refuse("DCRTParams no moduli", [&] { DCRTParams(m, {}, {}); });
    refuse("DCRTParams order 12, no roots", [&] { DCRTParams(12, q, {}); });
    refuse("DCRTParams modulus not 1 mod m", [&] { DCRTParams(m, {q[0] + 2}, {3}); });

    DCRTPolyHip e1(P1, EV), c1(P1, CO), e1b(P1b, EV), e2(P2, EV), c2(P2, CO), e32(P32, EV), c32(P32, CO),
        e1x2(P1, EV, 2), c1x2(P1, CO, 2);
    refuse("SetValues size", [&] { e1.SetValues(Words(7), EV); });
    refuse("DropLastElementAndScale constants", [&] { DCRTPolyHip(e2).DropLastElementAndScale({}, {1}); });
    refuse("DropLastElementAndScale constants 2", [&] { DCRTPolyHip(e2).DropLastElementAndScale({1}, {}); });
    refuse("DropLastElementAndScale one tower", [&] { DCRTPolyHip(e1).DropLastElementAndScale({}, {}); });
    refuse("ModReduce constants", [&] { DCRTPolyHip(e2).ModReduce(3, 1, {}); });
    refuse("ModReduce one tower", [&] { DCRTPolyHip(e1).ModReduce(3, 1, {}); });
    refuse("Times scalars", [&] { e2.Times(Words(1, 1)); });
    refuse("Plus integers", [&] { e2.Plus(Words(3, 1)); });
    refuse("Plus integers, COEFFICIENT", [&] { c2.Plus(Words(1, 1)); });
    refuse("Minus integers", [&] { e2.Minus(Words(1, 1)); });
    refuse("AutomorphismTransform even", [&] { e1.AutomorphismTransform(2); });
    refuse("MulViaNTT forms", [&] { e1.MulViaNTT(e1); });
    refuse("MulViaNTT forms 2", [&] { c1.MulViaNTT(c1); });
    refuse("MulViaNTT forms and ring", [&] { e1.MulViaNTT(e32); });
    refuse("MulViaNTT ring", [&] { c1.MulViaNTT(e32); });
    refuse("MulViaNTT towers", [&] { c1.MulViaNTT(e2); });
    refuse("MulViaNTT modulus", [&] { c1.MulViaNTT(e1b); });
    refuse("MulViaNTT batch", [&] { c1.MulViaNTT(e1x2); });

    // the element-wise family: every rung of check_compat per operation, then two faults at once
    struct Op {
        const char* name;
        void (*run)(DCRTPolyHip&, const DCRTPolyHip&);
        bool eval_only;
    };
    const Op ops[] = {
        {"Plus", [](DCRTPolyHip& a, const DCRTPolyHip& b) { a.Plus(b); }, false},
        {"Minus", [](DCRTPolyHip& a, const DCRTPolyHip& b) { a.Minus(b); }, false},
        {"Times", [](DCRTPolyHip& a, const DCRTPolyHip& b) { a.Times(b); }, true},
        {"operator+=", [](DCRTPolyHip& a, const DCRTPolyHip& b) { a += b; }, false},
        {"operator-=", [](DCRTPolyHip& a, const DCRTPolyHip& b) { a -= b; }, false},
        {"operator*=", [](DCRTPolyHip& a, const DCRTPolyHip& b) { a *= b; }, true},
        {"operator+", [](DCRTPolyHip& a, const DCRTPolyHip& b) { a + b; }, false},
        {"operator-", [](DCRTPolyHip& a, const DCRTPolyHip& b) { a - b; }, false},
        {"operator*", [](DCRTPolyHip& a, const DCRTPolyHip& b) { a * b; }, true},
    };
    for (const Op& o : ops) {
        const std::string n(o.name);
        refuse(n + " ring", [&] { o.run(e1, e32); });
        refuse(n + " format", [&] { o.run(e1, c1); });
        refuse(n + " format 2", [&] { o.run(c1, e1); });
        if (o.eval_only) refuse(n + " COEFFICIENT", [&] { o.run(c1, c1); });
        refuse(n + " towers", [&] { o.run(e1, e2); });
        refuse(n + " modulus", [&] { o.run(e1, e1b); });
        refuse(n + " batch", [&] { o.run(e1, e1x2); });
        refuse(n + " ring and format", [&] { o.run(e1, c32); });
        refuse(n + " format and towers", [&] { o.run(e1, c2); });
        refuse(n + " COEFFICIENT and towers", [&] { o.run(c1, c2); });
        refuse(n + " COEFFICIENT and batch", [&] { o.run(c1, c1x2); });
        refuse(n + " towers and batch", [&] { o.run(e2, e1x2); });
    }

    // Load: one record of e2 (T = 2, n = 8) patched per check.  Offsets: T 0; tower 0: n 8, words 16,
    // modulus 80, format 88, co 92, rd 96, q 100, root 108; tower 1 at 116 likewise; then format 224,
    // co 228, rd 232, T 236, and the params of tower 0 at 244 (co, rd, q, root 260), of tower 1 at 268
    std::ostringstream os;
    e2.Save(os);
    const std::string rec = os.str();
    auto load = [&](const std::string& s, uint32_t batch = 1) {
        std::istringstream is(s);
        DCRTPolyHip::Load(is, batch);
    };
    auto patched = [&](size_t off, auto v) {
        std::string s = rec;
        std::memcpy(&s[off], &v, sizeof v);
        return s;
    };
    refuse("Load batch 0", [&] { load(rec, 0); });
    refuse("Load no towers", [&] { load(patched(0, (uint64_t)0)); });
    refuse("Load too many towers", [&] { load(patched(0, (uint64_t)4097)); });
    refuse("Load ring dimension 3", [&] { load(patched(8, (uint64_t)3)); });
    refuse("Load ring dimension 2^18", [&] { load(patched(8, (uint64_t)1 << 18)); });
    refuse("Load tower modulus", [&] { load(patched(80, q[0] + 1)); });
    refuse("Load tower ring", [&] { load(patched(96, (uint32_t)4)); });
    refuse("Load tower order", [&] { load(patched(92, (uint32_t)32)); });
    refuse("Load tower formats", [&] { load(patched(196, (uint32_t)1)); });
    refuse("Load value above modulus", [&] { load(patched(16, ~(uint64_t)0)); });
    refuse("Load params format", [&] { load(patched(224, (uint32_t)1)); });
    refuse("Load params order", [&] { load(patched(228, (uint32_t)32)); });
    refuse("Load params ring", [&] { load(patched(232, (uint32_t)4)); });
    refuse("Load params towers", [&] { load(patched(236, (uint64_t)3)); });
    refuse("Load params root", [&] { load(patched(260, r[0] + 1)); });
    refuse("Load params modulus", [&] { load(patched(252, q[0] + 1)); });
    {
        std::string s = rec;
        for (size_t off : {(size_t)88, (size_t)196, (size_t)224}) {
            const uint32_t two = 2;
            std::memcpy(&s[off], &two, 4);
        }
        refuse("Load unknown format", [&] { load(s); });
        std::ostringstream o2;
        c2.Save(o2);
        refuse("Load batch of two formats", [&] { load(rec + o2.str(), 2); });
        refuse("Load unknown format in a batch of two formats", [&] { load(o2.str() + s, 2); });
    }
    refuse("Load truncated", [&] { load(rec.substr(0, 10)); });
    refuse("Load truncated words", [&] { load(rec.substr(0, 40)); });
    refuse("Load empty", [&] { load(""); });
    refuse("Load batch 2 of one record", [&] { load(rec, 2); });
}

// the HYBRID engine at N = 2^12: Q of 3 towers, P of 2, two digits
static void keyswitch_cases(uint32_t m, const Words& q, const Words& r) {
    const uint32_t n = m / 2, dnum = 2, B = 2;
    const Words qQ = cut(q, 0, 3), rQ = cut(r, 0, 3), qP = cut(q, 3, 2), rP = cut(r, 3, 2);
    auto PQ = std::make_shared<DCRTParams>(m, qQ, rQ), PP = std::make_shared<DCRTParams>(m, qP, rP);
    auto PQP = std::make_shared<DCRTParams>(m, cat(qQ, qP), cat(rQ, rP));
    auto PQl = std::make_shared<DCRTParams>(m, cut(q, 0, 2), cut(r, 0, 2));
    auto PQlP = std::make_shared<DCRTParams>(m, cat(cut(q, 0, 2), qP), cat(cut(r, 0, 2), rP));
    auto PQl2 = std::make_shared<DCRTParams>(m, cut(q, 1, 2), cut(r, 1, 2));  // two towers, another basis
    auto PW = std::make_shared<DCRTParams>(m, cut(q, 0, 4), cut(r, 0, 4));    // more towers than Q
    auto ks = KsCache::get(*PQ, *PP, dnum);
    HipManager* mgr = PQ->manager();

    DCRTPolyHip c(PQl, EV, B), cc(PQl, CO, B), cB(PQl, EV, B + 1), cO(PQl2, EV, B), cW(PW, EV, B), cQ(PQ, EV, B),
        cWc(PW, CO, B);
    DCRTPolyHip kb(PQP, EV, dnum), ka(PQP, EV, dnum), k1(PQP, EV, 1), kq(PQ, EV, dnum);

    refuse("KeySwitchCore form", [&] { ks->KeySwitchCore(cc, kb, ka); });
    refuse("KeySwitchCore towers", [&] { ks->KeySwitchCore(cW, kb, ka); });
    refuse("KeySwitchCore key b batch", [&] { ks->KeySwitchCore(c, k1, ka); });
    refuse("KeySwitchCore key a batch", [&] { ks->KeySwitchCore(c, kb, k1); });
    refuse("KeySwitchCore key b towers", [&] { ks->KeySwitchCore(c, kq, ka); });
    refuse("KeySwitchCore key a towers", [&] { ks->KeySwitchCore(c, kb, kq); });
    refuse("KeySwitchCore form and towers", [&] { ks->KeySwitchCore(cWc, kb, ka); });
    refuse("KeySwitchCore form and key", [&] { ks->KeySwitchCore(cc, k1, ka); });
    refuse("KeySwitchCore towers and key", [&] { ks->KeySwitchCore(cW, kb, kq); });

    // the multiplication family
    auto mult = [&](const char* w, const DCRTPolyHip& a0, const DCRTPolyHip& a1, const DCRTPolyHip& b0,
                    const DCRTPolyHip& b1, const DCRTPolyHip& xb, const DCRTPolyHip& xa, uint32_t levels = 0) {
        refuse(std::string("EvalMult ") + w, [&] { ks->EvalMult(a0, a1, b0, b1, xb, xa, OFHE_SHE_CKKS, 0, levels); });
    };
    auto square = [&](const char* w, const DCRTPolyHip& a0, const DCRTPolyHip& a1, const DCRTPolyHip& xb,
                      const DCRTPolyHip& xa, uint32_t levels = 0) {
        refuse(std::string("EvalSquare ") + w, [&] { ks->EvalSquare(a0, a1, xb, xa, OFHE_SHE_CKKS, 0, levels); });
    };
    mult("form", cc, c, c, c, kb, ka);
    mult("form of d1", c, c, c, cc, kb, ka);
    mult("basis", c, cO, c, c, kb, ka);
    mult("batch", c, c, cB, c, kb, ka);
    mult("towers", cW, cW, cW, cW, kb, ka);
    mult("key batch", c, c, c, c, k1, ka);
    mult("key towers", c, c, c, c, kb, kq);
    mult("levels", c, c, c, c, kb, ka, 2);
    mult("form and key", cc, c, c, c, k1, ka);
    mult("batch and key", c, c, c, cB, kb, kq);
    mult("towers and key", cW, cW, cW, cW, k1, ka);
    mult("key and levels", c, c, c, c, k1, ka, 2);
    mult("form and levels", c, cc, c, c, kb, ka, 5);
    mult("form and basis", cc, cO, c, c, kb, ka);
    mult("basis before form", c, cO, cc, c, kb, ka);
    square("form", c, cc, kb, ka);
    square("basis", c, cO, kb, ka);
    square("batch", c, cB, kb, ka);
    square("towers", cW, cW, kb, ka);
    square("key", c, c, kq, ka);
    square("levels", c, c, kb, ka, 2);
    square("form and key", cc, c, kb, k1);
    square("key and levels", c, c, kb, k1, 3);
    typedef KeySwitchHybrid::RelinKey RK;
    const std::vector<RK> two{{&kb, &ka}, {&kb, &ka}};
    refuse("Relinearize two elements", [&] { ks->Relinearize({&c, &c}, {}); });
    refuse("Relinearize no elements", [&] { ks->Relinearize({}, {}); });
    refuse("Relinearize key count", [&] { ks->Relinearize({&c, &c, &c}, two); });
    refuse("Relinearize two elements and key count", [&] { ks->Relinearize({&c, &c}, two); });
    refuse("Relinearize NULL element", [&] { ks->Relinearize({&c, nullptr, &c}, {RK{&kb, &ka}}); });
    refuse("Relinearize form", [&] { ks->Relinearize({&c, &c, &cc}, {RK{&kb, &ka}}); });
    refuse("Relinearize basis", [&] { ks->Relinearize({&c, &cO, &c}, {RK{&kb, &ka}}); });
    refuse("Relinearize batch", [&] { ks->Relinearize({&c, &c, &cB}, {RK{&kb, &ka}}); });
    refuse("Relinearize towers", [&] { ks->Relinearize({&cW, &cW, &cW}, {RK{&kb, &ka}}); });
    refuse("Relinearize key", [&] { ks->Relinearize({&c, &c, &c}, {RK{&k1, &ka}}); });
    refuse("Relinearize second key", [&] { ks->Relinearize({&c, &c, &c, &c}, {RK{&kb, &ka}, RK{&kb, &kq}}); });
    refuse("Relinearize form and key", [&] { ks->Relinearize({&c, &c, &cc}, {RK{&k1, &ka}}); });
    refuse("Relinearize towers and key", [&] { ks->Relinearize({&cW, &cW, &cW}, {RK{&kb, &kq}}); });
    refuse("Rescale no elements", [&] { ks->Rescale({}); });
    refuse("Rescale NULL element", [&] { ks->Rescale({nullptr}); });
    refuse("Rescale form", [&] { ks->Rescale({&c, &cc}); });
    refuse("Rescale basis", [&] { ks->Rescale({&c, &cO}); });
    refuse("Rescale batch", [&] { ks->Rescale({&c, &cB}); });
    refuse("Rescale towers", [&] { ks->Rescale({&cW}); });
    refuse("Rescale levels 0", [&] { ks->Rescale({&c}, OFHE_SHE_CKKS, 0, 0); });
    refuse("Rescale levels 2", [&] { ks->Rescale({&c}, OFHE_SHE_CKKS, 0, 2); });
    refuse("Rescale form and levels", [&] { ks->Rescale({&cc}, OFHE_SHE_CKKS, 0, 0); });
    refuse("Rescale towers and levels", [&] { ks->Rescale({&cW}, OFHE_SHE_CKKS, 0, 9); });

    // hoisted rotations: digits of two polynomials at level 2 (never computed: no call gets that far)
    refuse("FastRotationPrecompute form", [&] { ks->FastRotationPrecompute(cc); });
    refuse("FastRotationPrecompute towers", [&] { ks->FastRotationPrecompute(cW); });
    refuse("FastRotationPrecompute form and towers", [&] { ks->FastRotationPrecompute(cWc); });
    auto digits_at = [&](uint32_t l, uint32_t batch) {
        KeySwitchHybrid::HoistedDigits d;
        d.buf = DeviceBuffer(mgr, (size_t)batch * dnum * (l + 2) * n);
        d.size_ql = l;
        d.batch = batch;
        return d;
    };
    const auto dg = digits_at(2, B), dg3 = digits_at(3, B);
    KeySwitchHybrid::HoistedDigits none, no_level = digits_at(2, B);
    no_level.size_ql = 0;
    typedef KeySwitchHybrid::RotationKey RotK;
    const std::vector<uint32_t> idx{5, 25};
    const std::vector<RotK> keys{{&kb, &ka}, {&kb, &ka}}, keys1{{&kb, &ka}}, keys_null_b{{&kb, &ka}, {nullptr, &ka}},
        keys_null_a{{&kb, nullptr}, {&kb, &ka}}, keys_batch{{&kb, &ka}, {&k1, &ka}}, keys_batch_a{{&kb, &k1}, {&kb, &ka}},
        keys_towers{{&kq, &ka}, {&kb, &ka}}, keys_towers_a{{&kb, &ka}, {&kb, &kq}};
    struct Rot {
        const char* name;
        std::function<void(const DCRTPolyHip*, const KeySwitchHybrid::HoistedDigits&, const std::vector<uint32_t>&,
                           const std::vector<RotK>&)>
            run;
        bool takes_c0;
    };
    const Rot rots[] = {
        {"FastRotation", [&](auto* c0, auto& d, auto& ix, auto& k) { ks->FastRotation(*c0, d, ix, k); }, true},
        {"FastRotationExt", [&](auto* c0, auto& d, auto& ix, auto& k) { ks->FastRotationExt(c0, d, ix, k, PQlP); }, true},
        {"FastRotationExt without c0",
         [&](auto*, auto& d, auto& ix, auto& k) { ks->FastRotationExt(nullptr, d, ix, k, PQlP); }, false},
        {"FastRotationExtSum",
         [&](auto*, auto& d, auto& ix, auto& k) { ks->FastRotationExtSum(d, ix, k, nullptr, PQlP); }, false},
    };
    for (const Rot& o : rots) {
        const std::string w(o.name);
        refuse(w + " no digits", [&] { o.run(&c, none, idx, keys); });
        refuse(w + " digits without a level", [&] { o.run(&c, no_level, idx, keys); });
        if (o.takes_c0) {
            refuse(w + " form", [&] { o.run(&cc, dg, idx, keys); });
            refuse(w + " batch", [&] { o.run(&cB, dg, idx, keys); });
            refuse(w + " no digits and form", [&] { o.run(&cc, none, idx, keys); });
            refuse(w + " form and batch", [&] { DCRTPolyHip x(PQl, CO, B + 1); o.run(&x, dg, idx, keys); });
            refuse(w + " batch and key count", [&] { o.run(&cB, dg, idx, keys1); });
            refuse(w + " levels", [&] { o.run(&c, dg3, idx, keys); });
            refuse(w + " key and levels", [&] { o.run(&c, dg3, idx, keys_batch); });
            refuse(w + " form and levels", [&] { DCRTPolyHip x(PQ, CO, B); o.run(&x, dg, idx, keys); });
        }
        refuse(w + " no indices", [&] { o.run(&c, dg, {}, {}); });
        refuse(w + " key count", [&] { o.run(&c, dg, idx, keys1); });
        refuse(w + " NULL key b", [&] { o.run(&c, dg, idx, keys_null_b); });
        refuse(w + " NULL key a", [&] { o.run(&c, dg, idx, keys_null_a); });
        refuse(w + " key b batch", [&] { o.run(&c, dg, idx, keys_batch); });
        refuse(w + " key a batch", [&] { o.run(&c, dg, idx, keys_batch_a); });
        refuse(w + " key b towers", [&] { o.run(&c, dg, idx, keys_towers); });
        refuse(w + " key a towers", [&] { o.run(&c, dg, idx, keys_towers_a); });
        refuse(w + " key and the level's params", [&] { o.run(&c, dg3, idx, keys_towers); });
    }
    refuse("FastRotationExt params NULL", [&] { ks->FastRotationExt(&c, dg, idx, keys, nullptr); });
    refuse("FastRotationExt params towers", [&] { ks->FastRotationExt(&c, dg, idx, keys, PQP); });
    refuse("FastRotationExt levels and params", [&] { ks->FastRotationExt(&cQ, dg, idx, keys, PQP); });
    refuse("FastRotationExt without c0, params of another level", [&] { ks->FastRotationExt(nullptr, dg3, idx, keys, PQlP); });

    // the pieces of the BSGS linear transform
    DCRTPolyHip x(PQlP, EV, 2 * B), xc(PQlP, CO, 2 * B), xO(PQP, EV, 2 * B), x3(PQlP, EV, 3), xP(PP, EV, 2 * B),
        dgn(PQlP, EV, 4), dgc(PQlP, CO, 4);
    refuse("KeySwitchExt form", [&] { ks->KeySwitchExt(cc, PQlP); });
    refuse("KeySwitchExt towers", [&] { ks->KeySwitchExt(cW, PQlP); });
    refuse("KeySwitchExt params NULL", [&] { ks->KeySwitchExt(c, nullptr); });
    refuse("KeySwitchExt params towers", [&] { ks->KeySwitchExt(c, PQP); });
    refuse("KeySwitchExt form and params", [&] { ks->KeySwitchExt(cc, nullptr); });
    refuse("KeySwitchExt towers and params", [&] { ks->KeySwitchExt(cW, nullptr); });
    refuse("MultExtSum form", [&] { ks->MultExtSum(x, xc, 2, dgn, {}, 2); });
    refuse("MultExtSum form of the diagonals", [&] { ks->MultExtSum(x, x, 2, dgc, {}, 2); });
    refuse("MultExtSum only P", [&] { ks->MultExtSum(xP, xP, 2, DCRTPolyHip(PP, EV, 4), {}, 2); });
    refuse("MultExtSum bases", [&] { ks->MultExtSum(x, xO, 2, dgn, {}, 2); });
    refuse("MultExtSum basis of the diagonals", [&] { ks->MultExtSum(x, x, 2, DCRTPolyHip(PQP, EV, 4), {}, 2); });
    refuse("MultExtSum nterm 0", [&] { ks->MultExtSum(x, x, 0, dgn, {}, 2); });
    refuse("MultExtSum nsum 0", [&] { ks->MultExtSum(x, x, 2, dgn, {}, 0); });
    refuse("MultExtSum terms", [&] { ks->MultExtSum(x3, x3, 2, dgn, {}, 2); });
    refuse("MultExtSum term batches", [&] { ks->MultExtSum(x, DCRTPolyHip(PQlP, EV, 2), 2, dgn, {}, 2); });
    refuse("MultExtSum diagonals", [&] { ks->MultExtSum(x, x, 2, dgn, {}, 3); });
    refuse("MultExtSum presence", [&] { ks->MultExtSum(x, x, 2, dgn, std::vector<uint8_t>(3, 1), 2); });
    refuse("MultExtSum form and bases", [&] { ks->MultExtSum(xc, xO, 2, dgn, {}, 2); });
    refuse("MultExtSum bases and terms", [&] { ks->MultExtSum(x, xO, 0, dgn, {}, 2); });
    refuse("MultExtSum diagonals and presence", [&] { ks->MultExtSum(x, x, 2, dgn, std::vector<uint8_t>(3, 1), 3); });
    {
        const auto d3 = digits_at(2, 3);
        DCRTPolyHip add(PQlP, EV, 2), addc(PQlP, CO, 2), addO(PQP, EV, 2), add3(PQlP, EV, 3);
        const auto dgB = digits_at(2, 4);  // two sets of two
        refuse("FastRotationExtSum towers", [&] { ks->FastRotationExtSum(digits_at(4, 2), idx, keys, nullptr, PQlP); });
        refuse("FastRotationExtSum params NULL", [&] { ks->FastRotationExtSum(dg, idx, keys, nullptr, nullptr); });
        refuse("FastRotationExtSum params towers", [&] { ks->FastRotationExtSum(dg, idx, keys, nullptr, PQP); });
        refuse("FastRotationExtSum sets", [&] { ks->FastRotationExtSum(d3, idx, keys, nullptr, PQlP); });
        refuse("FastRotationExtSum addend form", [&] { ks->FastRotationExtSum(dgB, idx, keys, &addc, PQlP); });
        refuse("FastRotationExtSum addend batch", [&] { ks->FastRotationExtSum(dgB, idx, keys, &add3, PQlP); });
        refuse("FastRotationExtSum addend basis", [&] { ks->FastRotationExtSum(dgB, idx, keys, &addO, PQlP); });
        refuse("FastRotationExtSum key and params", [&] { ks->FastRotationExtSum(dg, idx, keys_batch, nullptr, PQP); });
        refuse("FastRotationExtSum params and sets", [&] { ks->FastRotationExtSum(d3, idx, keys, nullptr, PQP); });
        refuse("FastRotationExtSum sets and addend", [&] { ks->FastRotationExtSum(d3, idx, keys, &addc, PQlP); });
    }

    // LinearTransform: two baby and two giant steps over resident keys
    KeyCache::put("errors:good", DCRTPolyHip(PQP, EV, dnum), DCRTPolyHip(PQP, EV, dnum));
    KeyCache::put("errors:batch", DCRTPolyHip(PQP, EV, 1), DCRTPolyHip(PQP, EV, dnum));
    KeyCache::put("errors:batch a", DCRTPolyHip(PQP, EV, dnum), DCRTPolyHip(PQP, EV, 1));
    KeyCache::put("errors:towers", DCRTPolyHip(PQ, EV, dnum), DCRTPolyHip(PQP, EV, dnum));
    KeyCache::put("errors:towers a", DCRTPolyHip(PQP, EV, dnum), DCRTPolyHip(PQ, EV, dnum));
    KeyCache::put("errors:gone", DCRTPolyHip(PQP, EV, dnum), DCRTPolyHip(PQP, EV, dnum));
    KeyCache::erase("errors:gone");
    refuse("KeyCache::get missing", [&] { KeyCache::get("errors:none"); });
    refuse("KeyCache::get erased", [&] { KeyCache::get("errors:gone"); });
    KeySwitchHybrid::BsgsPlan plan;
    plan.babyIndex = {1, 5};  // 1: the identity step, its key id is not looked up
    plan.giantIndex = {2 * m + 1, 25};
    plan.babyKey = {"errors:none", "errors:good"};
    plan.giantKey = {"errors:none", "errors:good"};
    DCRTPolyHip diag(PQlP, EV, 4), diagc(PQlP, CO, 4), diagO(PQP, EV, 4), diag3(PQlP, EV, 3);
    auto lt = [&](const char* w, const DCRTPolyHip& a0, const DCRTPolyHip& a1, const KeySwitchHybrid::BsgsPlan& p,
                  const DCRTPolyHip& d) {
        refuse(std::string("LinearTransform ") + w, [&] { ks->LinearTransform(a0, a1, p, d); });
    };
    auto with = [&](auto&& edit) {
        KeySwitchHybrid::BsgsPlan p = plan;
        edit(p);
        return p;
    };
    lt("form", c, cc, plan, diag);
    lt("form of c0", cc, c, plan, diag);
    lt("form of the diagonals", c, c, plan, diagc);
    lt("towers", cW, cW, plan, diag);
    lt("bases", c, cO, plan, diag);
    lt("batches", c, cB, plan, diag);
    lt("no baby steps", c, c, with([](auto& p) { p.babyIndex.clear(), p.babyKey.clear(); }), diag);
    lt("no giant steps", c, c, with([](auto& p) { p.giantIndex.clear(), p.giantKey.clear(); }), diag);
    lt("baby key ids", c, c, with([](auto& p) { p.babyKey.pop_back(); }), diag);
    lt("giant key ids", c, c, with([](auto& p) { p.giantKey.push_back("errors:good"); }), diag);
    lt("diagonal towers", c, c, plan, diagO);
    lt("diagonal count", c, c, plan, diag3);
    lt("presence", c, c, with([](auto& p) { p.present.assign(3, 1); }), diag);
    lt("missing baby key", c, c, with([](auto& p) { p.babyKey[1] = "errors:none"; }), diag);
    lt("missing giant key", c, c, with([](auto& p) { p.giantKey[1] = "errors:gone"; }), diag);
    lt("key b batch", c, c, with([](auto& p) { p.babyKey[1] = "errors:batch"; }), diag);
    lt("key a batch", c, c, with([](auto& p) { p.giantKey[1] = "errors:batch a"; }), diag);
    lt("key b towers", c, c, with([](auto& p) { p.giantKey[1] = "errors:towers"; }), diag);
    lt("key a towers", c, c, with([](auto& p) { p.babyKey[1] = "errors:towers a"; }), diag);
    lt("form and bases", cc, cO, plan, diag);
    lt("bases and key ids", c, cO, with([](auto& p) { p.babyKey.pop_back(); }), diag);
    lt("key ids and diagonals", c, c, with([](auto& p) { p.babyKey.pop_back(); }), diag3);
    lt("diagonals and presence", c, c, with([](auto& p) { p.present.assign(3, 1); }), diag3);
    lt("presence and key", c, c, with([](auto& p) { p.present.assign(3, 1), p.babyKey[1] = "errors:batch"; }), diag);
    lt("bad baby key and missing giant key", c, c,
       with([](auto& p) { p.babyKey[1] = "errors:towers", p.giantKey[1] = "errors:none"; }), diag);
    lt("missing baby key and bad giant key", c, c,
       with([](auto& p) { p.babyKey[1] = "errors:none", p.giantKey[1] = "errors:batch"; }), diag);
    for (const char* id : {"errors:good", "errors:batch", "errors:batch a", "errors:towers", "errors:towers a"})
        KeyCache::erase(id);

    // ApproxModDown and the two expansions, with a converter of arbitrary table words
    BaseConverter p_to_q(*PP, *PQ, Words(2, 1), Words(6, 1)), q_to_p(*PQ, *PP, Words(3, 1), Words(6, 1));
    DCRTPolyHip y(PQP, EV, B), yc(PQP, CO, B);
    refuse("ApproxModDown form", [&] { ApproxModDown(yc, PQ, PP, p_to_q, Words(3, 1)); });
    refuse("ApproxModDown towers", [&] { ApproxModDown(y, PQl, PP, p_to_q, Words(2, 1)); });
    refuse("ApproxModDown PInvModq", [&] { ApproxModDown(y, PQ, PP, p_to_q, Words(2, 1)); });
    refuse("ApproxModDown form and towers", [&] { ApproxModDown(yc, PQl, PP, p_to_q, Words(2, 1)); });
    refuse("ApproxModDown towers and PInvModq", [&] { ApproxModDown(y, PQl, PP, p_to_q, Words(3, 1)); });
    refuse("ApproxModUp paramsQP", [&] { ApproxModUp(cQ, PP, PQlP, q_to_p); });
    refuse("ExpandCRTBasis paramsQP", [&] { ExpandCRTBasis(cQ, PP, PQlP, q_to_p); });
    refuse("ApproxSwitchCRTBasis form", [&] { q_to_p.ApproxSwitchCRTBasis(cQ, PP); });
    refuse("SwitchCRTBasis form", [&] { q_to_p.SwitchCRTBasis(cQ, PP); });

    // the two hook helpers that share the adapter's code
    refuse("hooks::converter QHatInvModq", [&] { hooks::converter(0, 12, qQ, qP, Words(2, 1), Words(6, 1), "hooks::Case"); });
    refuse("hooks::converter QHatModp", [&] { hooks::converter(0, 12, qQ, qP, Words(3, 1), Words(5, 1), "hooks::Case"); });
    refuse("hooks::converter both tables", [&] { hooks::converter(0, 12, qQ, qP, {}, {}, "hooks::Other"); });
    {
        const Towers good = towers(n, cat(qQ, qP), cat(rQ, rP), EV), coeff = towers(n, cat(qQ, qP), cat(rQ, rP), CO),
                     other = towers(n, cat(qP, qQ), cat(rP, rQ), EV), roots = towers(n, cat(qQ, qP), cat(rQ, rQ), EV);
        typedef std::vector<const Towers*> V;
        refuse("hooks::PutEvalKey no polynomials", [&] { hooks::PutEvalKey<Towers>("errors", V{}, V{}, 2); });
        refuse("hooks::PutEvalKey b and a counts", [&] { hooks::PutEvalKey<Towers>("errors", V{&good, &good}, V{&good}, 2); });
        refuse("hooks::PutEvalKey sizeP 0", [&] { hooks::PutEvalKey<Towers>("errors", V{&good}, V{&good}, 0); });
        refuse("hooks::PutEvalKey sizeP 5", [&] { hooks::PutEvalKey<Towers>("errors", V{&good}, V{&good}, 5); });
        refuse("hooks::PutEvalKey form", [&] { hooks::PutEvalKey<Towers>("errors", V{&good}, V{&coeff}, 2); });
        refuse("hooks::PutEvalKey bases", [&] { hooks::PutEvalKey<Towers>("errors", V{&good, &other}, V{&good, &good}, 2); });
        refuse("hooks::PutEvalKey roots", [&] { hooks::PutEvalKey<Towers>("errors", V{&good}, V{&roots}, 2); });
        refuse("hooks::PutEvalKey counts and sizeP", [&] { hooks::PutEvalKey<Towers>("errors", V{&good}, V{}, 0); });
        refuse("hooks::PutEvalKey sizeP and form", [&] { hooks::PutEvalKey<Towers>("errors", V{&coeff}, V{&coeff}, 5); });
        refuse("hooks::GetEvalKey missing", [&] { hooks::GetEvalKey("errors"); });
    }
}

// the BFV family at N = 2^12: Q and R of two towers each
static void bfv_cases(uint32_t m, const Words& q, const Words& r) {
    const uint32_t B = 2;
    const Words qQ = cut(q, 0, 2), rQ = cut(r, 0, 2), qR = cut(q, 2, 2), rR = cut(r, 2, 2);
    auto PQ = std::make_shared<DCRTParams>(m, qQ, rQ), PR = std::make_shared<DCRTParams>(m, qR, rR);
    auto PQR = std::make_shared<DCRTParams>(m, cat(qQ, qR), cat(rQ, rR));
    // Q's moduli, and Q_0's, in the ring of dimension 8: the same basis but for the ring
    auto PQ16 = std::make_shared<DCRTParams>(16, qQ, Words{powmod(r[0], m / 16, q[0]), powmod(r[1], m / 16, q[1])});
    auto PQl16 = std::make_shared<DCRTParams>(16, Words{q[0]}, Words{powmod(r[0], m / 16, q[0])});
    DCRTPolyHip e(PQ, EV, B), c(PQ, CO, B), eB(PQ, EV, B + 1), eR(PR, EV, B), cR(PR, CO, B), eQR(PQR, EV, B),
        cQR(PQR, CO, B);
    const std::vector<Words> rows22(2, Words(3, 1));
    const std::vector<double> frac2(2, 0.25);

    refuse("ScaleAndRound rows", [&] { ScaleAndRound(*PQ, *PR, false, std::vector<Words>(3, Words(3, 1)), frac2); });
    refuse("ScaleAndRound fractions", [&] { ScaleAndRound(*PQ, *PR, true, rows22, std::vector<double>(3, 0.25)); });
    refuse("ScaleAndRound row size", [&] { ScaleAndRound(*PQ, *PR, false, std::vector<Words>(2, Words(2, 1)), frac2); });
    refuse("ScaleAndRound rows and row size", [&] { ScaleAndRound(*PQ, *PR, false, std::vector<Words>(1, Words(2, 1)), frac2); });
    refuse("ScaleAndRound fraction outside [0, 1)", [&] { ScaleAndRound(*PQ, *PR, false, rows22, std::vector<double>(2, 1.5)); });
    {
        ScaleAndRound sr(*PQ, *PR, false, rows22, frac2);
        refuse("ScaleAndRound form", [&] { sr(eQR, PR); });
    }
    {
        BfvMult hps(BfvMult::HPS, PQ, PR, PQR, Words(2, 1), Words(4, 1), Words(2, 1), Words(4, 1), rows22, frac2);
        BfvMult pq(BfvMult::HPSPOVERQ, PQ, PR, PQR, Words(2, 1), Words(4, 1), Words(2, 1), Words(4, 1), rows22, frac2,
                   Words(2, 1), Words(4, 1));
        for (const BfvMult* bm : {&hps, &pq}) {
            const std::string w = bm == &hps ? "BfvMult::EvalMult HPS " : "BfvMult::EvalMult HPSPOVERQ ";
            refuse(w + "form", [&] { bm->EvalMult(e, c, e, e); });
            refuse(w + "basis", [&] { bm->EvalMult(e, e, eR, e); });
            refuse(w + "batch", [&] { bm->EvalMult(e, e, e, eB); });
            refuse(w + "form and basis", [&] { bm->EvalMult(cR, e, e, e); });
            refuse(w + "batch of c0", [&] { bm->EvalMult(eB, e, e, e); });
        }
        refuse("BfvMult QR", [&] {
            BfvMult(BfvMult::HPS, PQ, PR, PQ, Words(2, 1), Words(4, 1), Words(2, 1), Words(4, 1), rows22, frac2);
        });
    }
    // BEHZ: B of two towers and m_sk
    {
        const Words qK = cut(q, 2, 3), rK = cut(r, 2, 3);
        auto PK = std::make_shared<DCRTParams>(m, qK, rK), PQK = std::make_shared<DCRTParams>(m, cat(qQ, qK), cat(rQ, rK));
        auto P1 = std::make_shared<DCRTParams>(m, cut(q, 2, 1), cut(r, 2, 1));
        const size_t sq = 2, sk = 3, sb = 2;
        BehzTables T;
        T.tQHatInvModq.assign(sq, 1), T.QHatModbsk.assign(sq * sk, 1), T.QHatModmtilde.assign(sq, 1);
        T.qInvModbsk.assign(sq * sk, 1), T.mtildeQHatInvModq.assign(sq, 1), T.QModbsk.assign(sk, 1);
        T.mtildeInvModbsk.assign(sk, 1), T.tQInvModbsk.assign(sk, 1), T.BHatInvModb.assign(sb, 1);
        T.BHatModq.assign(sb * sq, 1), T.BHatModmsk.assign(sb, 1), T.BModq.assign(sq, 1);
        refuse("BehzBasis one Bsk tower", [&] { BehzBasis(PQ, P1, PQK, 65537, T); });
        refuse("BehzBasis QBsk towers", [&] { BehzBasis(PQ, PK, PQR, 65537, T); });
        BehzTables bad = T;
        bad.BModq.pop_back();
        refuse("BehzBasis tables", [&] { BehzBasis(PQ, PK, PQK, 65537, bad); });
        bad = T;
        bad.tQHatInvModq.push_back(1);
        refuse("BehzBasis first table", [&] { BehzBasis(PQ, PK, PQK, 65537, bad); });
        refuse("BehzBasis QBsk towers and tables", [&] { BehzBasis(PQ, PK, PQR, 65537, bad); });
        refuse("BehzBasis t", [&] { BehzBasis(PQ, PK, PQK, 1, T); });
        BehzBasis bz(PQ, PK, PQK, 65537, T);
        DCRTPolyHip eK(PK, EV, B), cK(PK, CO, B), eQK(PQK, EV, B), cQK(PQK, CO, B), e16(PQ16, EV, B);
        refuse("FastBaseConvqToBskMontgomery basis", [&] { bz.FastBaseConvqToBskMontgomery(eK); });
        refuse("FastBaseConvqToBskMontgomery ring", [&] { bz.FastBaseConvqToBskMontgomery(e16); });
        refuse("FastRNSFloorq basis", [&] { bz.FastRNSFloorq(c); });
        refuse("FastRNSFloorq form", [&] { bz.FastRNSFloorq(eQK); });
        refuse("FastRNSFloorq basis and form", [&] { bz.FastRNSFloorq(e); });
        refuse("FastBaseConvSK basis", [&] { bz.FastBaseConvSK(cQK); });
        refuse("FastBaseConvSK form", [&] { bz.FastBaseConvSK(eK); });
        refuse("FastBaseConvSK basis and form", [&] { bz.FastBaseConvSK(eQK); });
        refuse("BfvMultBehz form", [&] { bz.BfvMultBehz(e, e, c, e); });
        refuse("BfvMultBehz basis", [&] { bz.BfvMultBehz(e, eK, e, e); });
        refuse("BfvMultBehz batch", [&] { bz.BfvMultBehz(e, e, e, eB); });
        refuse("BfvMultBehz form and basis", [&] { bz.BfvMultBehz(cK, e, e, e); });
    }
    // decryption
    {
        BfvDecryptTables T;
        T.tQHatInvModqDivqModt.assign(2, 1), T.tQHatInvModqBDivqModt.assign(2, 1);
        T.tQHatInvModqDivqFrac.assign(2, 0.25), T.tQHatInvModqBDivqFrac.assign(2, 0.25);
        T.tgammaQHatInvModq.assign(2, 1), T.negInvqModtgamma.assign(2, 1), T.tInvModq.assign(2, 1);
        BfvDecryptTables bad = T;
        bad.tInvModq.push_back(1);
        refuse("BfvDecrypt integer table", [&] { BfvDecrypt(PQ, 65537, OFHE_BFV_HPS, bad); });
        bad = T;
        bad.tQHatInvModqBDivqFrac.pop_back();
        refuse("BfvDecrypt fraction table", [&] { BfvDecrypt(PQ, 65537, OFHE_BFV_HPS, bad); });
        bad.tQHatInvModqDivqModt.pop_back();
        refuse("BfvDecrypt both kinds of table", [&] { BfvDecrypt(PQ, 65537, OFHE_BFV_HPS, bad); });
        refuse("BfvDecrypt technique", [&] { BfvDecrypt(PQ, 65537, 77, T); });
        refuse("BfvDecrypt t", [&] { BfvDecrypt(PQ, 1, OFHE_BFV_HPS, T); });
        BfvDecrypt d(PQ, 65537, OFHE_BFV_HPS, T);
        BfvDecryptTables plain = T;
        plain.tInvModq.clear();
        BfvDecrypt d0(PQ, 65537, OFHE_BFV_HPS, plain);
        DCRTPolyHip s(PQ, EV, 1), sc(PQ, CO, 1), sR(PR, EV, 1), e16(PQ16, EV, B);
        refuse("BfvDecrypt::ScaleAndRound basis", [&] { d.ScaleAndRound(cR); });
        refuse("BfvDecrypt::ScaleAndRound ring", [&] { d.ScaleAndRound(DCRTPolyHip(PQ16, CO, B)); });
        refuse("BfvDecrypt::ScaleAndRound form", [&] { d.ScaleAndRound(e); });
        refuse("BfvDecrypt::ScaleAndRound basis and form", [&] { d.ScaleAndRound(eR); });
        refuse("Decrypt one element", [&] { d.Decrypt({e}, s); });
        refuse("Decrypt four elements", [&] { d.Decrypt({e, e, e, e}, s); });
        refuse("Decrypt basis", [&] { d.Decrypt({e, eR}, s); });
        refuse("Decrypt formats", [&] { d.Decrypt({e, c}, s); });
        refuse("Decrypt batches", [&] { d.Decrypt({e, e, eB}, s); });
        refuse("Decrypt basis of the key", [&] { d.Decrypt({e, e}, sR); });
        refuse("Decrypt form of the key", [&] { d.Decrypt({e, e}, sc); });
        refuse("Decrypt batch of the key", [&] { d.Decrypt({e, e}, e); });
        refuse("Decrypt count and basis", [&] { d.Decrypt({eR}, s); });
        refuse("Decrypt formats then basis", [&] { d.Decrypt({e, c, eR}, s); });
        refuse("Decrypt basis and format of one element", [&] { d.Decrypt({e, cR}, s); });
        refuse("Decrypt batches and key", [&] { d.Decrypt({e, eB}, sR); });
        refuse("Decrypt basis and form of the key", [&] { d.Decrypt({e, e}, DCRTPolyHip(PR, CO, 1)); });
        refuse("TimesQovert basis", [&] { DCRTPolyHip(eR).TimesQovert(d); });
        refuse("TimesQovert ring", [&] { DCRTPolyHip(e16).TimesQovert(d); });
        refuse("TimesQovert without its tables", [&] { DCRTPolyHip(e).TimesQovert(d0); });
    }
    // one level of HPSPOVERQLEVELED: l = 0 of two towers, and the full level
    {
        BfvLevelTables T;
        T.l = 0;
        T.QlHatInvModq.assign(1, 1), T.QlHatModr.assign(1, 1), T.RlHatInvModr.assign(1, 1), T.RlHatModq.assign(1, 1);
        T.negRlQHatInvModq.assign(2, 1), T.qInvModr.assign(2, 1);
        T.QlQHatInvModqDivqModq.assign(1, Words(2, 1)), T.QlQHatInvModqDivqFrac.assign(1, 0.25);
        T.tQlSlHatInvModsDivsModq.assign(1, Words(2, 1)), T.tQlSlHatInvModsDivsFrac.assign(1, 0.25);
        T.QlHatModq.assign(1, 1);
        auto PE = std::make_shared<DCRTParams>(m, cut(q, 2, 1), cut(r, 2, 1));
        BfvLevelTables bad = T;
        bad.l = 2;
        refuse("BfvLevel l", [&] { BfvLevel(PQ, PR, bad); });
        bad.l = 1;
        refuse("BfvLevel R towers", [&] { BfvLevel(PQ, PE, bad); });
        bad = T;
        bad.QlHatModq.push_back(1);
        refuse("BfvLevel QlHatModq", [&] { BfvLevel(PQ, PR, bad); });
        bad.l = 2;
        refuse("BfvLevel l and QlHatModq", [&] { BfvLevel(PQ, PR, bad); });
        bad = T;
        bad.QlQHatInvModqDivqFrac.clear();
        refuse("BfvLevel drop tables", [&] { BfvLevel(PQ, PR, bad); });
        bad.QlHatModq.clear();
        refuse("BfvLevel QlHatModq and drop tables", [&] { BfvLevel(PQ, PR, bad); });
        bad = T;
        bad.QlHatModq[0] = q[0];
        refuse("BfvLevel QlHatModq value", [&] { BfvLevel(PQ, PR, bad); });
        auto lv = BfvLevelCache::get(PQ, PR, 1, 0, [&](uint32_t) { return T; });
        DCRTPolyHip el(lv->ParamsQl(), EV, B), cl(lv->ParamsQlRl(), CO, B), elr(lv->ParamsQlRl(), EV, B);
        refuse("BfvLevel::EvalMult form", [&] { lv->EvalMult(e, e, c, e); });
        refuse("BfvLevel::EvalMult basis", [&] { lv->EvalMult(e, el, e, e); });
        refuse("BfvLevel::EvalMult batch", [&] { lv->EvalMult(e, e, e, eB); });
        refuse("BfvLevel::EvalMult form and basis", [&] { lv->EvalMult(cR, e, e, e); });
        refuse("BfvLevel::EvalSquare form", [&] { lv->EvalSquare(e, c); });
        refuse("BfvLevel::EvalSquare basis", [&] { lv->EvalSquare(eR, eR); });
        refuse("BfvLevel::Relinearize one element", [&] { lv->Relinearize({&e}, e, e, nullptr); });
        refuse("BfvLevel::Relinearize four elements", [&] { lv->Relinearize({&e, &e, &e, &e}, e, e, nullptr); });
        refuse("BfvLevel::Relinearize NULL element", [&] { lv->Relinearize({&e, nullptr}, e, e, nullptr); });
        refuse("BfvLevel::Relinearize formats", [&] { lv->Relinearize({&e, &e, &c}, e, e, nullptr); });
        refuse("BfvLevel::Relinearize basis", [&] { lv->Relinearize({&eR, &eR}, e, e, nullptr); });
        refuse("BfvLevel::Relinearize batches", [&] { lv->Relinearize({&e, &eB}, e, e, nullptr); });
        refuse("BfvLevel::Relinearize count and basis", [&] { lv->Relinearize({&eR}, e, e, nullptr); });
        refuse("BfvLevel::Relinearize no engine", [&] { lv->Relinearize({&e, &e, &e}, e, e, nullptr); });
        refuse("BfvLevel::ScaleAndRoundExpand form", [&] { lv->ScaleAndRoundExpand(elr); });
        refuse("BfvLevel::ScaleAndRoundExpand basis", [&] { lv->ScaleAndRoundExpand(c); });
        refuse("BfvLevel::ScaleAndRoundExpand form and basis", [&] { lv->ScaleAndRoundExpand(e); });
        refuse("ExpandCRTBasisQlHat basis", [&] { DCRTPolyHip(e).ExpandCRTBasisQlHat(*lv); });
        refuse("ExpandCRTBasisQlHat ring", [&] { DCRTPolyHip(PQl16, EV, B).ExpandCRTBasisQlHat(*lv); });
    }
}

int main() {
    try {
        poly_cases();
        const uint32_t m = 2u << 12;
        Words q, r;
        chain(50, m, 5, q, r);
        keyswitch_cases(m, q, r);
        bfv_cases(m, q, r);
        HipManager::getHip()->sync();
    } catch (const std::exception& e) {
        std::printf("adapter errors: setup failed: %s\n", e.what());
        return 2;
    }
    return g_silent ? 1 : 0;
}
