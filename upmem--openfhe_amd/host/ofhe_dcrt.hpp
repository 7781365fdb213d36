// ofhe_dcrt.hpp -- C++ host side of the gfx950 backend, above the C ABI.
//
// Mirrors the reference's interfaces for the hot path so OpenFHE-side code
// (and these tests) read the same way:
//   HipManager::getHip(dev)   <- PimManager::getPim(nr_dpus, profile)
//                                (src/core/include/pim/PimManager.h:23-29,44-85)
//   DeviceBuffer              <- PimData's device allocation (PimData.h:16-34, RAII)
//   DCRTPolyHip               <- DCRTPolyImpl's operator surface used by the
//                                schemes (lattice/hal/default/dcrtpoly.h:142-200,
//                                dcrtpoly-impl.h:410-416, 1034-1063, 2518-2524):
//                                SwitchFormat/SetFormat, Plus/Minus/Times and the
//                                in-place operators, scalar Times, ApproxSwitchCRTBasis.
//   PlanCache                 <- ChineseRemainderTransformFTTNat's static
//                                per-modulus twiddle maps (transformnat.h:352-368)
//   Staging                   <- the per-vector host->DPU push of PimData
//                                (PimData.h:16-21): towers gathered from
//                                separate host vectors into pinned memory, one
//                                transfer each way
//   BaseConverter::SwitchCRTBasis, ExpandCRTBasis, ScaleAndRound, BfvMult
//                             <- the BFV (HPS / HPSPOVERQ) multiplication steps
//                                (dcrtpoly-impl.h:1178-1230, 1311-1358, 1876-1955,
//                                bfvrns-leveledshe.cpp:168-408)
//   BehzBasis                 <- the BFV (BEHZ) multiplication steps
//                                FastBaseConvqToBskMontgomery, FastRNSFloorq,
//                                FastBaseConvSK (dcrtpoly-impl.h:2050-2208,
//                                2212-2271, 2309-2411, bfvrns-leveledshe.cpp:275-297,
//                                383-403)
//   BfvLevel / BfvLevelCache  <- HPSPOVERQLEVELED with dropped levels: EvalMult,
//                                EvalSquare, RelinearizeCore, ExpandCRTBasisQlHat
//                                (bfvrns-leveledshe.cpp:235-274, 367-382, 459-499,
//                                845-899, dcrtpoly-impl.h:1514-1534) and
//                                FindLevelsToDrop (bfvrns-leveledshe.cpp:77-166)
//   DecryptCore, BgvDecrypt / BgvDecryptCache
//                             <- PKERNS::DecryptCore (rns-pke.cpp:199-224), with
//                                coeff_out PKECKKSRNS::Decrypt / PKERNS::Decrypt up
//                                to their last line, and PKEBGVRNS::Decrypt with
//                                its scalingFactorInt (bgvrns-pke.cpp:44-99)
//   KsCache / KeyCache        <- the per-parameter-set HYBRID tables
//                                (rns-cryptoparameters.cpp:72-345) and the
//                                evaluation keys kept resident on the device
// Errors: any non-zero C-ABI status becomes ofhe::math_error, the analogue of
// OPENFHE_THROW(math_error, ...) (src/core/include/utils/exception.h:162).
// Device layout: a DCRTPolyHip of `batch` polynomials is one contiguous
// [batch][towers][N] buffer -- towers are contiguous, unlike the reference's
// std::vector<PolyImpl> (dcrtpoly.h:421), so one launch covers every tower.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <istream>
#include <map>
#include <ostream>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ofhe_hip.h"

namespace ofhe {

class math_error : public std::runtime_error {
public:
    explicit math_error(const std::string& m) : std::runtime_error(m) {}
};
class not_implemented_error : public std::runtime_error {
public:
    explicit not_implemented_error(const std::string& m) : std::runtime_error(m) {}
};
class deserialize_error : public std::runtime_error {  // lbcrypto::deserialize_error (utils/exception.h)
public:
    explicit deserialize_error(const std::string& m) : std::runtime_error(m) {}
};

inline void check(int rc, const char* what) {
    if (rc != OFHE_OK) throw math_error(std::string(what) + ": " + ofhe_hip_last_error());
}

// ---------------------------------------------------------------------------
// HipManager: lazily created per-device singleton, creation guarded by a
// mutex (PimManager.h:23-29); owns the device context and its stream.
// ---------------------------------------------------------------------------
class HipManager {
public:
    static HipManager* getHip(int device = 0) {
        static std::mutex mu;
        static std::map<int, std::unique_ptr<HipManager>> inst;
        std::lock_guard<std::mutex> lk(mu);
        auto& p = inst[device];
        if (!p) p.reset(new HipManager(device));
        return p.get();
    }
    ofhe_ctx_t ctx() const { return ctx_; }
    int device() const { return device_; }
    // Every adapter op runs on one stream (the device's null stream), and
    // buffers are allocated and released in that stream's order: a DCRTPoly
    // temporary may die right after the call that reads it -- its memory is
    // returned only once the queued work has finished, and nothing waits.
    void* allocate(size_t bytes) {
        void* p = nullptr;
        check(ofhe_hip_alloc_async(ctx_, bytes, &p, nullptr), "HipManager::allocate");
        return p;
    }
    void deallocate(void* p) { check(ofhe_hip_free_async(ctx_, p, nullptr), "HipManager::deallocate"); }
    void zero(void* dst, size_t bytes) { check(ofhe_hip_zero(ctx_, dst, bytes, nullptr), "HipManager::zero"); }
    // Host <-> device copies of the caller's (pageable) memory go through the
    // manager's two pinned staging buffers: the caller's words are copied into
    // one, a DMA from page-locked memory is queued on the stream (in the
    // stream's order, after the launches that produce or read `dst`), and an
    // event marks it.  A buffer is refilled only after the event of its last
    // DMA -- a wait for that one transfer, not for every launch queued on the
    // stream (round 5 drained the whole stream before and after each round).
    // copy_to_device returns once the caller's buffer has been read (the
    // copy_to_pim contract, PimManager.cpp:5-37), with the DMA possibly still
    // in flight; copy_from_device returns with the words in `dst`
    // (copy_from_pim, PimManager.cpp:39-54), overlapping each chunk's DMA
    // with the previous chunk's host copy.  No pageable hipMemcpyAsync: that
    // path's staging and ordering are the HIP runtime's own (round 4's driver
    // record read back stale words on it, DESIGN.md (c) "The round-4 adapter
    // failure").
    void copy_to_device(void* dst, const void* src, size_t bytes) {
        std::lock_guard<std::mutex> lk(stage_mu_);
        const size_t room = stage_room(bytes);
        for (size_t off = 0; off < bytes;) {
            const size_t n = std::min(bytes - off, room);
            const int k = next_;
            next_ ^= 1;
            stage_wait(k);  // the buffer's previous DMA has read it
            std::memcpy(stage_[k], static_cast<const char*>(src) + off, n);
            check(ofhe_hip_copy_to_device(ctx_, static_cast<char*>(dst) + off, stage_[k], n, nullptr),
                  "HipManager::copy_to_device");
            stage_mark(k);
            off += n;
        }
    }
    void copy_from_device(void* dst, const void* src, size_t bytes) {
        std::lock_guard<std::mutex> lk(stage_mu_);
        const size_t room = stage_room(bytes);
        size_t prev_off = 0, prev_n = 0;
        int prev = -1;
        for (size_t off = 0; off < bytes;) {
            const size_t n = std::min(bytes - off, room);
            const int k = next_;
            next_ ^= 1;
            stage_wait(k);
            check(ofhe_hip_copy_to_host(ctx_, stage_[k], static_cast<const char*>(src) + off, n, nullptr),
                  "HipManager::copy_from_device");
            stage_mark(k);
            if (prev >= 0) drain(prev, dst, prev_off, prev_n);
            prev = k, prev_off = off, prev_n = n;
            off += n;
        }
        if (prev >= 0) drain(prev, dst, prev_off, prev_n);
    }
    void sync() { check(ofhe_hip_sync(ctx_, nullptr), "HipManager::sync"); }
    // ofhe_hip_finalize refuses (OFHE_ERR_STATE) while DeviceBuffers still
    // hold blocks of the context's pool: the context is then left alive for
    // them (they free through the context handle, not through this object),
    // and process exit reclaims it.
    ~HipManager() {
        for (int k = 0; k < 2; k++) {
            if (ev_[k]) {
                (void)ofhe_hip_event_sync(ev_[k]);
                (void)ofhe_hip_event_destroy(ev_[k]);
            }
            if (stage_[k]) (void)ofhe_hip_host_free(ctx_, stage_[k]);
        }
        if (ctx_) (void)ofhe_hip_finalize(ctx_);
    }
    HipManager(const HipManager&) = delete;
    HipManager& operator=(const HipManager&) = delete;

private:
    explicit HipManager(int device) : device_(device) {
        check(ofhe_hip_init(device, &ctx_), "HipManager");
        for (int k = 0; k < 2; k++) check(ofhe_hip_event_create(ctx_, &ev_[k]), "HipManager staging event");
    }
    // bytes each staging buffer takes per round (grown to the request, capped
    // at kStageMax: larger copies go in rounds); caller holds stage_mu_
    static constexpr size_t kStageMax = size_t(32) << 20;
    size_t stage_room(size_t want) {
        want = std::min(std::max<size_t>(want, 1), kStageMax);
        if (stage_bytes_ < want) {
            size_t b = 4096;
            while (b < want) b <<= 1;
            for (int k = 0; k < 2; k++) {
                stage_wait(k);  // a queued DMA may still read the old buffer
                if (stage_[k]) check(ofhe_hip_host_free(ctx_, stage_[k]), "HipManager staging");
                stage_[k] = nullptr;
            }
            stage_bytes_ = 0;
            for (int k = 0; k < 2; k++) check(ofhe_hip_host_alloc(ctx_, b, &stage_[k]), "HipManager staging");
            stage_bytes_ = b;
        }
        return stage_bytes_;
    }
    void stage_mark(int k) {
        check(ofhe_hip_event_record(ev_[k], nullptr), "HipManager staging event");
        pending_[k] = true;
    }
    void stage_wait(int k) {
        if (!pending_[k]) return;
        check(ofhe_hip_event_sync(ev_[k]), "HipManager staging event");
        pending_[k] = false;
    }
    void drain(int k, void* dst, size_t off, size_t n) {
        stage_wait(k);  // the DMA (and, in stream order, its producers) has finished
        std::memcpy(static_cast<char*>(dst) + off, stage_[k], n);
    }
    int device_;
    ofhe_ctx_t ctx_ = nullptr;
    std::mutex stage_mu_;
    void* stage_[2] = {nullptr, nullptr};
    ofhe_event_t ev_[2] = {nullptr, nullptr};
    bool pending_[2] = {false, false};
    int next_ = 0;
    size_t stage_bytes_ = 0;
};

// RAII device buffer of uint64 words.
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(HipManager* m, size_t words) : m_(m), ctx_(m->ctx()), n_(words) {
        if (words) p_ = static_cast<uint64_t*>(m_->allocate(words * sizeof(uint64_t)));
    }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    DeviceBuffer(DeviceBuffer&& o) noexcept { swap(o); }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
        swap(o);
        return *this;
    }
    ~DeviceBuffer() {
        if (p_) (void)ofhe_hip_free_async(ctx_, p_, nullptr);  // stream-ordered, no wait
    }
    uint64_t* get() const { return p_; }
    size_t size() const { return n_; }
    void upload(const uint64_t* h) { m_->copy_to_device(p_, h, n_ * 8); }
    void zero() { m_->zero(p_, n_ * 8); }
    void download(uint64_t* h) const { m_->copy_from_device(h, p_, n_ * 8); }
    void copy_from(const DeviceBuffer& o) {
        check(ofhe_hip_copy_device(m_->ctx(), p_, o.p_, n_ * 8, nullptr), "DeviceBuffer::copy_from");
    }

private:
    void swap(DeviceBuffer& o) {
        std::swap(m_, o.m_);
        std::swap(ctx_, o.ctx_);
        std::swap(p_, o.p_);
        std::swap(n_, o.n_);
    }
    HipManager* m_ = nullptr;
    ofhe_ctx_t ctx_ = nullptr;
    uint64_t* p_ = nullptr;
    size_t n_ = 0;
};

// ---------------------------------------------------------------------------
// PlanCache: one resident NTT plan per (device, N, moduli, roots), shared by
// every DCRTParams over that basis and kept for the process lifetime, as the
// reference's static per-modulus maps keep their tables (transformnat.h:352-368,
// filled in PreCompute, transformnat-impl.h:708-763).
// ---------------------------------------------------------------------------
// Handle<S, destroy>: the one owner of a C-ABI handle -- move-only, destroyed
// exactly once by the ABI's own destroy function; get() is the raw handle.
template <auto Destroy>
struct HandleDeleter {
    template <class S>
    void operator()(S* h) const {
        Destroy(h);
    }
};
template <class S, auto Destroy>
using Handle = std::unique_ptr<S, HandleDeleter<Destroy>>;

// Cache<Key, T>::get(key, build): the one get-or-create -- a process-wide map
// under a mutex per call site; build() runs on a miss, with the lock held, and
// its result is kept for the process lifetime.  Always inlined, so a hit costs
// what the hand-written lookups did (profiles/adapter_host_ab.json).
template <class Key, class T>
struct Cache {
    template <class F>
    [[gnu::always_inline]] static inline std::shared_ptr<T> get(const Key& key, F&& build) {
        static std::mutex mu;
        static std::map<Key, std::shared_ptr<T>> map;
        std::lock_guard<std::mutex> lk(mu);
        auto& e = map[key];
        if (!e) e = build();
        return e;
    }
};

// NamedStore<T>: the one string-keyed table of shared objects (put / find /
// erase under a mutex); find returns null for an unknown id.
template <class T>
struct NamedStore {
    static void put(const std::string& id, std::shared_ptr<const T> v) {
        std::lock_guard<std::mutex> lk(mu());
        map()[id] = std::move(v);
    }
    static std::shared_ptr<const T> find(const std::string& id) {
        std::lock_guard<std::mutex> lk(mu());
        auto it = map().find(id);
        return it == map().end() ? nullptr : it->second;
    }
    static void erase(const std::string& id) {
        std::lock_guard<std::mutex> lk(mu());
        map().erase(id);
    }

private:
    static std::mutex& mu() {
        static std::mutex m;
        return m;
    }
    static std::map<std::string, std::shared_ptr<const T>>& map() {
        static std::map<std::string, std::shared_ptr<const T>> m;
        return m;
    }
};

class PlanHandle {
public:
    PlanHandle(HipManager* m, uint32_t log_n, const std::vector<uint64_t>& q, const std::vector<uint64_t>& r) {
        ofhe_plan_t p = nullptr;
        check(ofhe_hip_plan_create(m->ctx(), log_n, (uint32_t)q.size(), q.data(), r.data(), &p), "PlanCache");
        p_.reset(p);
    }
    ofhe_plan_t get() const { return p_.get(); }

private:
    Handle<ofhe_plan_s, ofhe_hip_plan_destroy> p_;
};

class PlanCache {
public:
    static std::shared_ptr<PlanHandle> get(int device, uint32_t log_n, const std::vector<uint64_t>& moduli,
                                           const std::vector<uint64_t>& roots) {
        if (moduli.size() != roots.size() || moduli.empty()) throw math_error("PlanCache: moduli/roots size mismatch");
        // the manager's statics first: destroyed after the cached plans
        HipManager* m = HipManager::getHip(device);
        return Cache<Key, PlanHandle>::get(Key{device, log_n, moduli, roots},
                                           [&] { return std::make_shared<PlanHandle>(m, log_n, moduli, roots); });
    }

private:
    struct Key {
        int device;
        uint32_t log_n;
        std::vector<uint64_t> q, r;
        bool operator<(const Key& o) const {
            if (device != o.device) return device < o.device;
            if (log_n != o.log_n) return log_n < o.log_n;
            if (q != o.q) return q < o.q;
            return r < o.r;
        }
    };
};

// ---------------------------------------------------------------------------
// Staging: pinned host buffer + device buffer of `words` u64.  A host-buffer
// integration gathers a DCRTPoly's towers (separate std::vectors in the
// reference, dcrtpoly.h:421) into it, uploads once, runs one launch over all
// towers, and scatters the result back.
// ---------------------------------------------------------------------------
class Staging {
public:
    Staging(HipManager* m, size_t words) : m_(m), dev_(m, words), n_(words) {
        void* h = nullptr;
        check(ofhe_hip_host_alloc(m_->ctx(), words * sizeof(uint64_t), &h), "Staging");
        host_ = static_cast<uint64_t*>(h);
        for (auto& e : ev_) check(ofhe_hip_event_create(m_->ctx(), &e), "Staging");
    }
    ~Staging() {
        if (host_) {
            (void)ofhe_hip_sync(m_->ctx(), nullptr);
            (void)ofhe_hip_host_free(m_->ctx(), host_);
        }
        for (auto& e : ev_)
            if (e) (void)ofhe_hip_event_destroy(e);
    }
    Staging(const Staging&) = delete;
    Staging& operator=(const Staging&) = delete;
    uint64_t* host() const { return host_; }
    uint64_t* dev() const { return dev_.get(); }
    size_t words() const { return n_; }
    // towers[t] points at n words (one PolyImpl's values); they land at t*n
    void gather(const std::vector<const uint64_t*>& towers, size_t n) {
        if (towers.size() * n > n_) throw math_error("Staging::gather: more words than the buffer holds");
        for (size_t t = 0; t < towers.size(); t++) std::memcpy(host_ + t * n, towers[t], n * sizeof(uint64_t));
    }
    void scatter(const std::vector<uint64_t*>& towers, size_t n) const {
        if (towers.size() * n > n_) throw math_error("Staging::scatter: more words than the buffer holds");
        for (size_t t = 0; t < towers.size(); t++) std::memcpy(towers[t], host_ + t * n, n * sizeof(uint64_t));
    }
    // pinned memory: DMA straight from / to the staging buffer
    // the first `words` words (default: all) each way
    void upload(size_t words = SIZE_MAX) {
        check(ofhe_hip_copy_to_device(m_->ctx(), dev(), host_, std::min(words, n_) * 8, nullptr), "Staging::upload");
    }
    void download(size_t words = SIZE_MAX) {
        check(ofhe_hip_copy_to_host(m_->ctx(), host_, dev(), std::min(words, n_) * 8, nullptr), "Staging::download");
        m_->sync();
    }

    // gather + upload, pipelined: towers go in chunks of ~kChunkBytes, each
    // chunk's host copies (one tower per OpenMP thread when the caller builds
    // with OpenMP, as OpenFHE does) run while the previous chunk's DMA is in
    // flight.  Chunks land in disjoint parts of the pinned buffer, and every
    // hook ends in get_towers' wait, so no chunk overwrites a buffer a DMA
    // still reads.  Tower t lands at word t * n of the device buffer.
    void put_towers(const std::vector<const uint64_t*>& towers, size_t n) {
        if (towers.size() * n > n_) throw math_error("Staging::put_towers: more words than the buffer holds");
        const size_t per = chunk_towers(n), T = towers.size();
        for (size_t t0 = 0; t0 < T; t0 += per) {
            const size_t t1 = std::min(T, t0 + per);
            copy_towers(t0, t1, [&](size_t t) { std::memcpy(host_ + t * n, towers[t], n * 8); });
            check(ofhe_hip_copy_to_device(m_->ctx(), dev() + t0 * n, host_ + t0 * n, (t1 - t0) * n * 8, nullptr),
                  "Staging::put_towers");
        }
    }
    // download + scatter, pipelined the other way: every chunk's DMA is
    // queued (in stream order, after the launch that produces it), and chunk
    // k is scattered once its event fires while chunk k + 1 is in flight.
    // Returns with every word in place (the reference's synchronous
    // copy_from_pim, PimManager.cpp:39-54).
    void get_towers(const std::vector<uint64_t*>& towers, size_t n) {
        if (towers.size() * n > n_) throw math_error("Staging::get_towers: more words than the buffer holds");
        const size_t per = chunk_towers(n), T = towers.size();
        size_t prev0 = 0, prev1 = 0, k = 0;
        auto scatter_chunk = [&](size_t a, size_t b, int e) {
            check(ofhe_hip_event_sync(ev_[e]), "Staging::get_towers");
            copy_towers(a, b, [&](size_t t) { std::memcpy(towers[t], host_ + t * n, n * 8); });
        };
        for (size_t t0 = 0; t0 < T; t0 += per, k++) {
            const size_t t1 = std::min(T, t0 + per);
            check(ofhe_hip_copy_to_host(m_->ctx(), host_ + t0 * n, dev() + t0 * n, (t1 - t0) * n * 8, nullptr),
                  "Staging::get_towers");
            check(ofhe_hip_event_record(ev_[k & 1], nullptr), "Staging::get_towers");
            if (k) scatter_chunk(prev0, prev1, (int)((k - 1) & 1));
            prev0 = t0, prev1 = t1;
        }
        if (k) scatter_chunk(prev0, prev1, (int)((k - 1) & 1));
    }

private:
    static constexpr size_t kChunkBytes = size_t(8) << 20;
    static size_t chunk_towers(size_t n) { return std::max<size_t>(1, kChunkBytes / (n * 8)); }
    template <class F>
    static void copy_towers(size_t t0, size_t t1, F f) {
#ifdef _OPENMP
#pragma omp parallel for schedule(static) if (t1 - t0 > 1)
#endif
        for (size_t t = t0; t < t1; t++) f(t);
    }
    HipManager* m_;
    DeviceBuffer dev_;
    size_t n_;
    uint64_t* host_ = nullptr;
    ofhe_event_t ev_[2] = {nullptr, nullptr};
};

// ---------------------------------------------------------------------------
// Parameters: (cyclotomic order, moduli, roots) as ILDCRTParams; the NTT plan
// comes from PlanCache, so parameter objects over the same basis share it.
// ---------------------------------------------------------------------------
// words [first, first + count) of a per-tower list: the one place a basis is cut
inline std::vector<uint64_t> towers_of(const std::vector<uint64_t>& v, size_t first, size_t count) {
    return std::vector<uint64_t>(v.begin() + first, v.begin() + first + count);
}

class DCRTParams {
public:
    DCRTParams(uint32_t cyclotomic_order, std::vector<uint64_t> moduli, std::vector<uint64_t> roots,
               int device = 0)
        : m_(cyclotomic_order), q_(std::move(moduli)), r_(std::move(roots)), mgr_(HipManager::getHip(device)) {
        if (m_ < 4 || (m_ & (m_ - 1))) throw math_error("CyclotomicOrder is not a power of two");
        if (q_.size() != r_.size() || q_.empty()) throw math_error("moduli/roots size mismatch");
        uint32_t n = m_ / 2, lg = 0;
        while ((1u << lg) < n) lg++;
        log_n_ = lg;
        plan_ = PlanCache::get(device, log_n_, q_, r_);
    }
    DCRTParams(const DCRTParams&) = delete;
    DCRTParams& operator=(const DCRTParams&) = delete;
    uint32_t GetCyclotomicOrder() const { return m_; }
    uint32_t GetRingDimension() const { return m_ / 2; }
    uint32_t LogN() const { return log_n_; }
    size_t Towers() const { return q_.size(); }
    const std::vector<uint64_t>& Moduli() const { return q_; }
    const std::vector<uint64_t>& Roots() const { return r_; }
    ofhe_plan_t plan() const { return plan_->get(); }
    HipManager* manager() const { return mgr_; }
    // the params of towers [first, first + count), and of these towers followed
    // by o's (cached plans of those bases)
    std::shared_ptr<DCRTParams> Slice(size_t first, size_t count) const {
        return std::make_shared<DCRTParams>(m_, towers_of(q_, first, count), towers_of(r_, first, count),
                                            mgr_->device());
    }
    std::shared_ptr<DCRTParams> Join(const DCRTParams& o) const {
        std::vector<uint64_t> q(q_), r(r_);
        q.insert(q.end(), o.q_.begin(), o.q_.end());
        r.insert(r.end(), o.r_.begin(), o.r_.end());
        return std::make_shared<DCRTParams>(m_, std::move(q), std::move(r), mgr_->device());
    }

private:
    uint32_t m_, log_n_ = 0;
    std::vector<uint64_t> q_, r_;
    HipManager* mgr_;
    std::shared_ptr<PlanHandle> plan_;
};

// DropLastElement `levels` times (dcrtpoly-impl.h:719-728): the params of the
// shorter chain
inline std::shared_ptr<DCRTParams> lowered(const DCRTParams& p, size_t levels) {
    if (levels >= p.Towers()) throw math_error("Removing last element of DCRTPoly object renders it invalid!");
    return p.Slice(0, p.Towers() - levels);
}

enum class Format { EVALUATION = 0, COEFFICIENT = 1 };

// ---------------------------------------------------------------------------
// DCRTPolyHip: `batch` DCRT polynomials resident on one device.  With one
// tower it is also the PimData op set (PimData.h:46-168: + - * and
// ModAdd/ModSub/ModMul with vector or scalar right-hand sides).
// ---------------------------------------------------------------------------
class BfvDecrypt;
class BfvLevel;

class DCRTPolyHip {
public:
    DCRTPolyHip(std::shared_ptr<DCRTParams> p, Format f, uint32_t batch = 1)
        : p_(std::move(p)), f_(f), batch_(batch),
          buf_(p_->manager(), (size_t)batch * p_->Towers() * p_->GetRingDimension()) {
        buf_.zero();
    }
    // a result buffer the producing op overwrites entirely: no zero fill
    struct Uninit {};
    DCRTPolyHip(std::shared_ptr<DCRTParams> p, Format f, uint32_t batch, Uninit)
        : p_(std::move(p)), f_(f), batch_(batch),
          buf_(p_->manager(), (size_t)batch * p_->Towers() * p_->GetRingDimension()) {}
    DCRTPolyHip(const DCRTPolyHip& o) : p_(o.p_), f_(o.f_), batch_(o.batch_), buf_(o.p_->manager(), o.buf_.size()) {
        buf_.copy_from(o.buf_);
    }
    DCRTPolyHip(DCRTPolyHip&&) = default;
    DCRTPolyHip& operator=(DCRTPolyHip&&) = default;
    // the uninitialised result of an op, over p in format f, and a pair of them
    static DCRTPolyHip result(std::shared_ptr<DCRTParams> p, Format f, uint32_t batch) {
        return DCRTPolyHip(std::move(p), f, batch, Uninit{});
    }
    static std::pair<DCRTPolyHip, DCRTPolyHip> result_pair(const std::shared_ptr<DCRTParams>& p, Format f,
                                                           uint32_t batch) {
        return {result(p, f, batch), result(p, f, batch)};
    }

    const std::shared_ptr<DCRTParams>& GetParams() const { return p_; }
    Format GetFormat() const { return f_; }
    uint32_t Batch() const { return batch_; }
    uint64_t* data() const { return buf_.get(); }
    size_t words() const { return buf_.size(); }

    // values[b][t][i] flattened; must be canonical (< q_t)
    void SetValues(const std::vector<uint64_t>& flat, Format f) {
        if (flat.size() != buf_.size()) throw math_error("SetValues: size mismatch");
        buf_.upload(flat.data());
        f_ = f;
    }
    std::vector<uint64_t> GetValues() const {
        std::vector<uint64_t> h(buf_.size());
        buf_.download(h.data());
        return h;
    }
    // tower t of batch entry b (GetElementAtIndex(t) analogue)
    std::vector<uint64_t> GetElementAtIndex(size_t t, uint32_t b = 0) const {
        auto all = GetValues();
        const size_t n = p_->GetRingDimension();
        const size_t off = ((size_t)b * p_->Towers() + t) * n;
        return std::vector<uint64_t>(all.begin() + off, all.begin() + off + n);
    }

    // SwitchFormat (dcrtpoly-impl.h:2518-2524 -> poly-impl.h:412-432)
    void SwitchFormat() {
        if (f_ == Format::COEFFICIENT) {
            check(ofhe_hip_ntt_fwd(p_->plan(), data(), batch_, nullptr), "SwitchFormat");
            f_ = Format::EVALUATION;
        } else {
            check(ofhe_hip_ntt_inv(p_->plan(), data(), batch_, nullptr), "SwitchFormat");
            f_ = Format::COEFFICIENT;
        }
    }
    void SetFormat(Format f) {
        if (f != f_) SwitchFormat();
    }

    DCRTPolyHip Plus(const DCRTPolyHip& rhs) const { return binary("Plus", ofhe_hip_modadd_vv, rhs, false); }
    DCRTPolyHip Minus(const DCRTPolyHip& rhs) const { return binary("Minus", ofhe_hip_modsub_vv, rhs, false); }
    // Times (dcrtpoly.h:185-200): EVALUATION format only
    DCRTPolyHip Times(const DCRTPolyHip& rhs) const { return binary("Times", ofhe_hip_modmul_vv, rhs, true); }
    // DropLastElementAndScale (dcrtpoly-impl.h:746-768; CKKS / BFV rescaling):
    // one tower fewer, on the params of the shorter chain.  The reference keeps
    // m_format while its coefficient-form towers come back in evaluation form
    // (lines 765-766); here the format tag follows the data (EVALUATION).
    void DropLastElementAndScale(const std::vector<uint64_t>& QlQlInvModqlDivqlModq,
                                 const std::vector<uint64_t>& qlInvModq) {
        const size_t T = p_->Towers(), n = p_->GetRingDimension();
        if (QlQlInvModqlDivqlModq.size() + 1 < T || qlInvModq.size() + 1 < T)
            throw math_error("DropLastElementAndScale: one constant per remaining tower required");
        DCRTPolyHip r = result(lowered(*p_, 1), Format::EVALUATION, batch_);
        check(ofhe_hip_drop_last_and_scale(p_->plan(), (uint32_t)T, data(), T * n, r.data(), (T - 1) * n,
                                           f_ == Format::EVALUATION, QlQlInvModqlDivqlModq.data(), qlInvModq.data(),
                                           batch_, nullptr),
              "DropLastElementAndScale");
        *this = std::move(r);
    }
    // ModReduce (dcrtpoly-impl.h:792-812; BGV modulus switching): one tower
    // fewer, format unchanged
    void ModReduce(uint64_t t, uint64_t negtInvModq, const std::vector<uint64_t>& qlInvModq) {
        const size_t T = p_->Towers(), n = p_->GetRingDimension();
        if (qlInvModq.size() + 1 < T) throw math_error("ModReduce: one constant per remaining tower required");
        DCRTPolyHip r = result(lowered(*p_, 1), f_, batch_);
        check(ofhe_hip_mod_reduce(p_->plan(), (uint32_t)T, data(), T * n, r.data(), (T - 1) * n,
                                  f_ == Format::EVALUATION, t, negtInvModq, qlInvModq.data(), batch_, nullptr),
              "ModReduce");
        *this = std::move(r);
    }

    // TimesQovert (dcrtpoly-impl.h:1015-1031), in place, with the tInvModq and
    // negQModt of d's tables (defined after BfvDecrypt)
    inline void TimesQovert(const BfvDecrypt& d);

    // ExpandCRTBasisQlHat (dcrtpoly-impl.h:1514-1534), in place: a polynomial
    // over Q_l of the level becomes one over Q, towers i <= l times
    // QlHatModq_i, the others zero; the format is kept (defined after BfvLevel)
    inline void ExpandCRTBasisQlHat(const BfvLevel& level);

    // Times(const std::vector<NativeInteger>&): one scalar per tower (Shoup)
    DCRTPolyHip Times(const std::vector<uint64_t>& scalars) const {
        return scalar("Times", "scalar", ofhe_hip_modmul_scalar, scalars);
    }
    // Plus / Minus with one integer per tower (dcrtpoly.h:162-163, 182-183;
    // dcrtpoly-impl.h:545-584).  PolyImpl::Plus(Integer) adds the constant
    // polynomial: in COEFFICIENT form only coefficient 0 changes
    // (ModAddAtIndex(0), poly-impl.h:213-220), in EVALUATION form every slot;
    // PolyImpl::Minus(Integer) subtracts from every word in either form
    // (poly-impl.h:223-227), as the reference does.
    DCRTPolyHip Plus(const std::vector<uint64_t>& crt) const {
        if (f_ != Format::COEFFICIENT) return scalar("Plus", "integer", ofhe_hip_modadd_scalar, crt);
        per_tower("Plus", "integer", crt);
        DCRTPolyHip r(*this);
        check(ofhe_hip_modadd_scalar_at(p_->plan(), r.data(), 0, crt.data(), r.data(), batch_, nullptr), "Plus");
        return r;
    }
    DCRTPolyHip Minus(const std::vector<uint64_t>& crt) const {
        return scalar("Minus", "integer", ofhe_hip_modsub_scalar, crt);
    }
    // Plus / Minus(const Integer&): the same integer in every tower
    DCRTPolyHip Plus(uint64_t v) const { return Plus(std::vector<uint64_t>(p_->Towers(), v)); }
    DCRTPolyHip Minus(uint64_t v) const { return Minus(std::vector<uint64_t>(p_->Towers(), v)); }
    DCRTPolyHip& operator+=(const DCRTPolyHip& rhs) {
        return binary_eq("operator+=", ofhe_hip_modadd_vv, rhs, false);
    }
    DCRTPolyHip& operator-=(const DCRTPolyHip& rhs) {
        return binary_eq("operator-=", ofhe_hip_modsub_vv, rhs, false);
    }
    DCRTPolyHip& operator*=(const DCRTPolyHip& rhs) {
        return binary_eq("operator*=", ofhe_hip_modmul_vv, rhs, true);
    }
    DCRTPolyHip operator+(const DCRTPolyHip& rhs) const { return Plus(rhs); }
    DCRTPolyHip operator-(const DCRTPolyHip& rhs) const { return Minus(rhs); }
    DCRTPolyHip operator*(const DCRTPolyHip& rhs) const { return Times(rhs); }

    // c = INTT(NTT(this) (.) rhs): this in COEFFICIENT, rhs in EVALUATION; the
    // result is COEFFICIENT.  Equal to SwitchFormat; *= rhs; SwitchFormat.
    DCRTPolyHip MulViaNTT(const DCRTPolyHip& rhs) const {
        if (f_ != Format::COEFFICIENT || rhs.f_ != Format::EVALUATION)
            throw not_implemented_error("MulViaNTT: needs COEFFICIENT x EVALUATION");
        check_compat(rhs, "MulViaNTT", false, false);
        DCRTPolyHip r = result(p_, Format::COEFFICIENT, batch_);
        check(ofhe_hip_ntt_mul_intt(p_->plan(), data(), rhs.data(), r.data(), batch_, nullptr), "MulViaNTT");
        return r;
    }

    // AutomorphismTransform(k) (dcrtpoly-impl.h:350-358 -> poly-impl.h:312-365)
    DCRTPolyHip AutomorphismTransform(uint32_t k) const {
        DCRTPolyHip r = result(p_, f_, batch_);
        check(ofhe_hip_automorphism(p_->plan(), k, f_ == Format::EVALUATION, data(), r.data(), batch_, nullptr),
              "AutomorphismTransform");
        return r;
    }

    bool operator==(const DCRTPolyHip& o) const {
        return f_ == o.f_ && p_->Moduli() == o.p_->Moduli() && GetValues() == o.GetValues();
    }

    // Serialization in the reference's field order, one DCRTPoly record per
    // batch entry:
    //   DCRTPolyImpl::save (dcrtpoly.h:349-354): "v" towers, "f" format, "p" params
    //   PolyImpl::save (poly.h:322-327):         "v" values, "f" format, "p" params
    //   NativeVectorT::save, binary (mubintvecnat.h:665-674): size_type count, the
    //     words as binary_data, then the modulus (one NativeInteger word)
    //   ElemParams::save (elemparams.h:224-231): "co", "rd", "cm", "ru"
    //   ILDCRTParams::save (ildcrtparams.h:351-355): its ElemParams, then "p" the
    //     per-tower ILNativeParams
    // Little-endian, with cereal's binary conventions for what the reference
    // writes itself: a uint64 size_type before every vector, enums as uint32
    // (Format, utils/inttypes.h:65).  Not written: cereal's own framing
    // (class-version words, shared_ptr ids, the polymorphic params' type
    // names) and the BigInteger fields ("bm", "br", ILDCRTParams' "m"); cereal
    // is an empty submodule in the reference snapshot, so its byte stream is
    // not reproduced or pinned here.
    void Save(std::ostream& os) const {
        const auto h = GetValues();
        const size_t T = p_->Towers(), n = p_->GetRingDimension();
        const uint32_t co = p_->GetCyclotomicOrder(), rd = p_->GetRingDimension();
        for (uint32_t b = 0; b < batch_; b++) {
            put<uint64_t>(os, T);
            for (size_t t = 0; t < T; t++) {
                put<uint64_t>(os, n);
                os.write(reinterpret_cast<const char*>(h.data() + ((size_t)b * T + t) * n), n * 8);
                put<uint64_t>(os, p_->Moduli()[t]);
                put<uint32_t>(os, (uint32_t)f_);
                put_native_params(os, co, rd, p_->Moduli()[t], p_->Roots()[t]);
            }
            put<uint32_t>(os, (uint32_t)f_);
            put<uint32_t>(os, co);
            put<uint32_t>(os, rd);
            put<uint64_t>(os, T);
            for (size_t t = 0; t < T; t++) put_native_params(os, co, rd, p_->Moduli()[t], p_->Roots()[t]);
        }
        if (!os) throw math_error("DCRTPolyHip::Save: stream write failed");
    }
    // The inverse of Save for `batch` consecutive records; every record must
    // carry the same basis and format, and every value must be <= its modulus.
    static DCRTPolyHip Load(std::istream& is, uint32_t batch = 1, int device = 0) {
        if (batch == 0) throw deserialize_error("DCRTPolyHip::Load: batch must be >= 1");
        std::vector<uint64_t> flat, q0, r0;
        uint32_t co0 = 0, f0 = 0;
        for (uint32_t b = 0; b < batch; b++) {
            const uint64_t T = get<uint64_t>(is);
            if (T < 1 || T > 4096) throw deserialize_error("DCRTPolyHip::Load: tower count out of range");
            std::vector<uint64_t> q(T), r(T), vals;
            uint32_t co = 0, f = 0;
            for (uint64_t t = 0; t < T; t++) {
                const uint64_t n = get<uint64_t>(is);
                if (n < 2 || n > (1u << 17) || (n & (n - 1))) throw deserialize_error("DCRTPolyHip::Load: ring dimension");
                const size_t off = vals.size();
                vals.resize(off + n);
                is.read(reinterpret_cast<char*>(vals.data() + off), n * 8);
                const uint64_t m = get<uint64_t>(is);
                const uint32_t tf = get<uint32_t>(is);
                uint32_t tco, trd;
                uint64_t tq, tr;
                get_native_params(is, tco, trd, tq, tr);
                if (tq != m || trd != n || tco != 2 * n) throw deserialize_error("DCRTPolyHip::Load: tower params disagree");
                if (t == 0) co = tco, f = tf;
                if (tco != co || tf != f) throw deserialize_error("DCRTPolyHip::Load: towers of different rings / formats");
                // NativeVectorT::load (mubintvecnat.h:684-702) takes the words as
                // they are; the library itself writes the representative q (a
                // negated zero of a coefficient-form AutomorphismTransform), so
                // words <= m load unchanged and Save -> Load round-trips every
                // library output.  Larger words are refused: the device kernels'
                // lazy bounds assume inputs below 2q.
                for (size_t i = off; i < off + n; i++)
                    if (vals[i] > m) throw deserialize_error("DCRTPolyHip::Load: value above its modulus");
                q[t] = m;
                r[t] = tr;
            }
            const uint32_t pf = get<uint32_t>(is), pco = get<uint32_t>(is), prd = get<uint32_t>(is);
            const uint64_t pT = get<uint64_t>(is);
            if (pf != f || pco != co || prd != co / 2 || pT != T) throw deserialize_error("DCRTPolyHip::Load: params disagree");
            for (uint64_t t = 0; t < T; t++) {
                uint32_t tco, trd;
                uint64_t tq, tr;
                get_native_params(is, tco, trd, tq, tr);
                if (tco != co || tq != q[t] || tr != r[t]) throw deserialize_error("DCRTPolyHip::Load: params disagree");
            }
            if (f > 1) throw deserialize_error("DCRTPolyHip::Load: unknown format");
            if (b == 0) q0 = q, r0 = r, co0 = co, f0 = f;
            if (q != q0 || r != r0 || co != co0 || f != f0)
                throw deserialize_error("DCRTPolyHip::Load: batch entries over different bases / formats");
            flat.insert(flat.end(), vals.begin(), vals.end());
        }
        auto P = std::make_shared<DCRTParams>(co0, q0, r0, device);
        DCRTPolyHip x = result(P, (Format)f0, batch);
        x.SetValues(flat, (Format)f0);
        return x;
    }

private:
    template <class T>
    static void put(std::ostream& os, T v) {
        os.write(reinterpret_cast<const char*>(&v), sizeof v);  // little-endian host (x86-64)
    }
    template <class T>
    static T get(std::istream& is) {
        T v{};
        if (!is.read(reinterpret_cast<char*>(&v), sizeof v)) throw deserialize_error("DCRTPolyHip::Load: truncated stream");
        return v;
    }
    // ILNativeParams = ElemParams' "co", "rd", "cm" (the tower modulus), "ru"
    static void put_native_params(std::ostream& os, uint32_t co, uint32_t rd, uint64_t q, uint64_t r) {
        put<uint32_t>(os, co);
        put<uint32_t>(os, rd);
        put<uint64_t>(os, q);
        put<uint64_t>(os, r);
    }
    static void get_native_params(std::istream& is, uint32_t& co, uint32_t& rd, uint64_t& q, uint64_t& r) {
        co = get<uint32_t>(is);
        rd = get<uint32_t>(is);
        q = get<uint64_t>(is);
        r = get<uint64_t>(is);
    }
    // the element-wise family: one body per shape, the ABI function and the op's name as arguments
    typedef int (*VvFn)(ofhe_plan_t, const uint64_t*, const uint64_t*, uint64_t*, uint32_t, void*);
    DCRTPolyHip binary(const char* op, VvFn fn, const DCRTPolyHip& rhs, bool eval_only) const {
        check_compat(rhs, op, eval_only);
        DCRTPolyHip r = result(p_, f_, batch_);
        check(fn(p_->plan(), data(), rhs.data(), r.data(), batch_, nullptr), op);
        return r;
    }
    DCRTPolyHip& binary_eq(const char* op, VvFn fn, const DCRTPolyHip& rhs, bool eval_only) {
        check_compat(rhs, op, eval_only);
        check(fn(p_->plan(), data(), rhs.data(), data(), batch_, nullptr), op);
        return *this;
    }
    void per_tower(const char* op, const char* what, const std::vector<uint64_t>& s) const {
        if (s.size() != p_->Towers()) throw math_error(std::string(op) + ": one " + what + " per tower required");
    }
    DCRTPolyHip scalar(const char* op, const char* what, VvFn fn, const std::vector<uint64_t>& s) const {
        per_tower(op, what, s);
        DCRTPolyHip r = result(p_, f_, batch_);
        check(fn(p_->plan(), data(), s.data(), r.data(), batch_, nullptr), op);
        return r;
    }

    void check_compat(const DCRTPolyHip& rhs, const char* op, bool eval_only, bool same_format = true) const {
        if (p_->GetRingDimension() != rhs.p_->GetRingDimension())
            throw math_error(std::string(op) + ": RingDimension missmatch");
        if (same_format && f_ != rhs.f_) throw not_implemented_error(std::string(op) + ": Format missmatch");
        if (eval_only && (f_ != Format::EVALUATION || rhs.f_ != Format::EVALUATION))
            throw not_implemented_error(std::string(op) + " for DCRTPolyHip supported only in Format::EVALUATION");
        if (p_->Towers() != rhs.p_->Towers()) throw math_error(std::string(op) + ": tower size mismatch");
        if (p_->Moduli() != rhs.p_->Moduli()) throw math_error(std::string(op) + ": Modulus missmatch");
        if (batch_ != rhs.batch_) throw math_error(std::string(op) + ": batch mismatch");
    }

    std::shared_ptr<DCRTParams> p_;
    Format f_;
    uint32_t batch_;
    DeviceBuffer buf_;
};

// The two argument rules the classes below share.  check_over: x is over the
// basis P (moduli and ring); the caller gives the words after "<op>" where they
// differ.  check_form: x is in format f.
inline void check_over(const DCRTPolyHip& x, const DCRTParams& P, const char* op,
                       const char* suffix = ": the polynomial is over another basis") {
    if (x.GetParams()->Moduli() != P.Moduli() || x.GetParams()->LogN() != P.LogN())
        throw math_error(std::string(op) + suffix);
}
inline void check_form(const DCRTPolyHip& x, Format f, const char* op) {
    if (x.GetFormat() != f)
        throw math_error(std::string(op) + (f == Format::EVALUATION ? ": EVALUATION" : ": COEFFICIENT") +
                         " form expected");
}

// ---------------------------------------------------------------------------
// ApproxSwitchCRTBasis (dcrtpoly-impl.h:1034-1063): x over basis Q (params of
// x) -> basis P (paramsP), both COEFFICIENT form.
// ---------------------------------------------------------------------------
class BaseConverter {
public:
    BaseConverter(const DCRTParams& Q, const DCRTParams& P, const std::vector<uint64_t>& QHatInvModq,
                  const std::vector<uint64_t>& QHatModp /* [sizeQ][sizeP] */) {
        ofhe_bconv_t h = nullptr;
        check(ofhe_hip_bconv_create(Q.manager()->ctx(), Q.LogN(), (uint32_t)Q.Towers(), (uint32_t)P.Towers(),
                                    Q.Moduli().data(), P.Moduli().data(), QHatInvModq.data(), QHatModp.data(), &h),
              "BaseConverter");
        h_.reset(h);
    }
    DCRTPolyHip ApproxSwitchCRTBasis(const DCRTPolyHip& x, const std::shared_ptr<DCRTParams>& paramsP) const {
        return switch_basis("ApproxSwitchCRTBasis", ofhe_hip_approx_switch_crt_basis, x, paramsP);
    }
    // SwitchCRTBasis (dcrtpoly-impl.h:1178-1230), the exact switch with the
    // floating-point overflow count: this converter must hold the true CRT
    // tables (QHatInvModq, QHatModp); alphaQModp and qInv are derived from its
    // moduli inside the backend.
    DCRTPolyHip SwitchCRTBasis(const DCRTPolyHip& x, const std::shared_ptr<DCRTParams>& paramsP) const {
        return switch_basis("SwitchCRTBasis", ofhe_hip_switch_crt_basis, x, paramsP);
    }

    ofhe_bconv_t handle() const { return h_.get(); }

private:
    DCRTPolyHip switch_basis(const char* op, int (*fn)(ofhe_bconv_t, const uint64_t*, uint64_t*, uint32_t, void*),
                             const DCRTPolyHip& x, const std::shared_ptr<DCRTParams>& paramsP) const {
        check_form(x, Format::COEFFICIENT, op);
        DCRTPolyHip out = DCRTPolyHip::result(paramsP, Format::COEFFICIENT, x.Batch());
        check(fn(h_.get(), x.data(), out.data(), x.Batch(), nullptr), op);
        return out;
    }
    Handle<ofhe_bconv_s, ofhe_hip_bconv_destroy> h_;
};

// The body of ApproxModUp and ExpandCRTBasis: x over Q (either format) ->
// paramsQP = Q|P in EVALUATION form through q_to_p.
inline DCRTPolyHip mod_up(const char* op,
                          int (*fn)(ofhe_plan_t, ofhe_plan_t, ofhe_bconv_t, int, const uint64_t*, uint64_t*, uint32_t,
                                    void*),
                          const DCRTPolyHip& x, const std::shared_ptr<DCRTParams>& paramsP,
                          const std::shared_ptr<DCRTParams>& paramsQP, const BaseConverter& q_to_p) {
    const auto& Q = x.GetParams();
    if (paramsQP->Towers() != Q->Towers() + paramsP->Towers()) throw math_error(std::string(op) + ": paramsQP size");
    DCRTPolyHip out = DCRTPolyHip::result(paramsQP, Format::EVALUATION, x.Batch());
    check(fn(Q->plan(), paramsP->plan(), q_to_p.handle(), x.GetFormat() == Format::EVALUATION, x.data(), out.data(),
             x.Batch(), nullptr),
          op);
    return out;
}
// ApproxModUp (dcrtpoly-impl.h:1085-1131): the approximate switch; q_to_p converts Q -> P.
inline DCRTPolyHip ApproxModUp(const DCRTPolyHip& x, const std::shared_ptr<DCRTParams>& paramsP,
                               const std::shared_ptr<DCRTParams>& paramsQP, const BaseConverter& q_to_p) {
    return mod_up("ApproxModUp", ofhe_hip_approx_mod_up, x, paramsP, paramsQP, q_to_p);
}
// ExpandCRTBasis with resultFormat = EVALUATION (dcrtpoly-impl.h:1311-1358):
// the exact switch; q_to_p holds the true CRT tables of Q -> P.
inline DCRTPolyHip ExpandCRTBasis(const DCRTPolyHip& x, const std::shared_ptr<DCRTParams>& paramsP,
                                  const std::shared_ptr<DCRTParams>& paramsQP, const BaseConverter& q_to_p) {
    return mod_up("ExpandCRTBasis", ofhe_hip_expand_crt_basis, x, paramsP, paramsQP, q_to_p);
}

// ScaleAndRound, DCRTPoly -> DCRTPoly (dcrtpoly-impl.h:1876-1955): x over Q|P
// (COEFFICIENT) -> P (outIsQ = false, HPS) or Q (outIsQ = true, HPSPOVERQ).
// tOSHatInvModsDivsModo is the reference's vector of rows (one per output
// tower, sizeI + 1 entries), tOSHatInvModsDivsFrac its vector of doubles.
class ScaleAndRound {
public:
    ScaleAndRound(const DCRTParams& Q, const DCRTParams& P, bool outIsQ,
                  const std::vector<std::vector<uint64_t>>& tOSHatInvModsDivsModo,
                  const std::vector<double>& tOSHatInvModsDivsFrac)
        : out_is_q_(outIsQ) {
        const size_t si = outIsQ ? P.Towers() : Q.Towers(), so = outIsQ ? Q.Towers() : P.Towers();
        if (tOSHatInvModsDivsModo.size() != so || tOSHatInvModsDivsFrac.size() != si)
            throw math_error("ScaleAndRound: table sizes do not match the bases");
        std::vector<uint64_t> flat;
        for (const auto& row : tOSHatInvModsDivsModo) {
            if (row.size() != si + 1) throw math_error("ScaleAndRound: table row size");
            flat.insert(flat.end(), row.begin(), row.end());
        }
        ofhe_scale_round_t h = nullptr;
        check(ofhe_hip_scale_round_create(Q.manager()->ctx(), Q.LogN(), (uint32_t)Q.Towers(), (uint32_t)P.Towers(),
                                          Q.Moduli().data(), P.Moduli().data(), outIsQ ? 1 : 0, flat.data(),
                                          tOSHatInvModsDivsFrac.data(), &h),
              "ScaleAndRound");
        h_.reset(h);
    }
    DCRTPolyHip operator()(const DCRTPolyHip& x, const std::shared_ptr<DCRTParams>& paramsOutput) const {
        check_form(x, Format::COEFFICIENT, "ScaleAndRound");
        DCRTPolyHip out = DCRTPolyHip::result(paramsOutput, Format::COEFFICIENT, x.Batch());
        check(ofhe_hip_scale_and_round(h_.get(), x.data(), out.data(), x.Batch(), nullptr), "ScaleAndRound");
        return out;
    }
    bool OutIsQ() const { return out_is_q_; }
    ofhe_scale_round_t handle() const { return h_.get(); }

private:
    Handle<ofhe_scale_round_s, ofhe_hip_scale_round_destroy> h_;
    bool out_is_q_;
};

// What every BFV EvalMult (HPS family, BEHZ, leveled) takes and returns: four
// EVALUATION-form operands over Q of one batch are checked, and the three
// outputs over Q in COEFFICIENT form come back uninitialised.
inline std::vector<DCRTPolyHip> bfv_mult_outputs(const char* op, const std::shared_ptr<DCRTParams>& Q,
                                                 const DCRTPolyHip& c0, const DCRTPolyHip& c1, const DCRTPolyHip& d0,
                                                 const DCRTPolyHip& d1) {
    for (const DCRTPolyHip* v : {&c0, &c1, &d0, &d1})
        if (v->GetFormat() != Format::EVALUATION || v->GetParams()->Moduli() != Q->Moduli() || v->Batch() != c0.Batch())
            throw math_error(std::string(op) + ": EVALUATION-form ciphertexts over Q of one batch expected");
    std::vector<DCRTPolyHip> out;
    for (int k = 0; k < 3; k++) out.push_back(DCRTPolyHip::result(Q, Format::COEFFICIENT, c0.Batch()));
    return out;
}

// LeveledSHEBFVRNS::EvalMult (bfvrns-leveledshe.cpp:168-408), HPS or HPSPOVERQ,
// for two 2-element ciphertexts, from the outputs of the reference's getters
// as vectors: QHatInvModq / QHatModr ([sizeQ][sizeR] flattened), RHatInvModr /
// RHatModq ([sizeR][sizeQ] flattened), the ScaleAndRound tables, and for
// HPSPOVERQ mNegRlQHatInvModq / qInvModr ([sizeQ][sizeR] flattened).
class BfvMult {
public:
    enum Technique { HPS = OFHE_BFV_HPS, HPSPOVERQ = OFHE_BFV_HPSPOVERQ };
    BfvMult(Technique tech, std::shared_ptr<DCRTParams> Q, std::shared_ptr<DCRTParams> R,
            std::shared_ptr<DCRTParams> QR, const std::vector<uint64_t>& QHatInvModq,
            const std::vector<uint64_t>& QHatModr, const std::vector<uint64_t>& RHatInvModr,
            const std::vector<uint64_t>& RHatModq, const std::vector<std::vector<uint64_t>>& tSHatInvModsDivsModo,
            const std::vector<double>& tSHatInvModsDivsFrac, const std::vector<uint64_t>& mNegRlQHatInvModq = {},
            const std::vector<uint64_t>& qInvModr = {})
        : Q_(std::move(Q)), R_(std::move(R)), QR_(std::move(QR)), q_to_r_(*Q_, *R_, QHatInvModq, QHatModr),
          r_to_q_(*R_, *Q_, RHatInvModr, RHatModq),
          sr_(*Q_, *R_, tech == HPSPOVERQ, tSHatInvModsDivsModo, tSHatInvModsDivsFrac) {
        if (tech == HPSPOVERQ) neg_.reset(new BaseConverter(*Q_, *R_, mNegRlQHatInvModq, qInvModr));
        ofhe_bfv_mult_t h = nullptr;
        check(ofhe_hip_bfv_mult_create(Q_->manager()->ctx(), (int)tech, Q_->plan(), R_->plan(), QR_->plan(),
                                       q_to_r_.handle(), r_to_q_.handle(), neg_ ? neg_->handle() : nullptr,
                                       sr_.handle(), &h),
              "BfvMult");
        h_.reset(h);
    }
    // {cvMult[0], cvMult[1], cvMult[2]} over Q in COEFFICIENT form, as the reference leaves them
    std::vector<DCRTPolyHip> EvalMult(const DCRTPolyHip& c0, const DCRTPolyHip& c1, const DCRTPolyHip& d0,
                                      const DCRTPolyHip& d1) const {
        auto out = bfv_mult_outputs("BfvMult::EvalMult", Q_, c0, c1, d0, d1);
        check(ofhe_hip_bfv_eval_mult(h_.get(), c0.data(), c1.data(), d0.data(), d1.data(), out[0].data(), out[1].data(),
                                     out[2].data(), c0.Batch(), nullptr),
              "BfvMult::EvalMult");
        return out;
    }
    const BaseConverter& QToR() const { return q_to_r_; }
    const BaseConverter& RToQ() const { return r_to_q_; }
    const BaseConverter* QToRNeg() const { return neg_.get(); }  // null for HPS
    const ScaleAndRound& Scale() const { return sr_; }
    ofhe_bfv_mult_t handle() const { return h_.get(); }

private:
    std::shared_ptr<DCRTParams> Q_, R_, QR_;
    BaseConverter q_to_r_, r_to_q_;
    ScaleAndRound sr_;
    std::unique_ptr<BaseConverter> neg_;
    Handle<ofhe_bfv_mult_s, ofhe_hip_bfv_mult_destroy> h_;
};

// The BEHZ tables as the reference's getters return them
// (CryptoParametersBFVRNS, bfvrns-cryptoparameters.cpp:724-851): matrices
// flattened row-major ([sizeQ][sizeBsk], [sizeB][sizeQ]).
struct BehzTables {
    std::vector<uint64_t> tQHatInvModq, QHatModbsk, QHatModmtilde, qInvModbsk, mtildeQHatInvModq;
    uint64_t negQInvModmtilde = 0;
    std::vector<uint64_t> QModbsk, mtildeInvModbsk, tQInvModbsk, BHatInvModb, BHatModq, BHatModmsk;
    uint64_t BInvModmsk = 0;
    std::vector<uint64_t> BModq;
};

// The BEHZ variant of the BFV multiplication (bfvrns-leveledshe.cpp:275-297,
// 383-403) over Q, Bsk = B|msk and QBsk = Q|Bsk:
//   FastBaseConvqToBskMontgomery  dcrtpoly-impl.h:2050-2208  Q (either format) -> Q|Bsk, EVALUATION
//   FastRNSFloorq                 dcrtpoly-impl.h:2212-2271  Q|Bsk -> Bsk, COEFFICIENT
//   FastBaseConvSK                dcrtpoly-impl.h:2309-2411  Bsk -> Q, COEFFICIENT (the centred
//                                 correction, see ofhe_hip.h)
//   BfvMultBehz                   EvalMult of two 2-element ciphertexts
// The reference's members change the polynomial in place; these return the result.
class BehzBasis {
public:
    BehzBasis(std::shared_ptr<DCRTParams> Q, std::shared_ptr<DCRTParams> Bsk, std::shared_ptr<DCRTParams> QBsk,
              uint64_t t, const BehzTables& T)
        : Q_(std::move(Q)), Bsk_(std::move(Bsk)), QBsk_(std::move(QBsk)) {
        const size_t sq = Q_->Towers(), sk = Bsk_->Towers();
        if (sk < 2 || QBsk_->Towers() != sq + sk) throw math_error("BehzBasis: QBsk must be Q's towers then Bsk's");
        const size_t sb = sk - 1;
        if (T.tQHatInvModq.size() != sq || T.QHatModbsk.size() != sq * sk || T.QHatModmtilde.size() != sq ||
            T.qInvModbsk.size() != sq * sk || T.mtildeQHatInvModq.size() != sq || T.QModbsk.size() != sk ||
            T.mtildeInvModbsk.size() != sk || T.tQInvModbsk.size() != sk || T.BHatInvModb.size() != sb ||
            T.BHatModq.size() != sb * sq || T.BHatModmsk.size() != sb || T.BModq.size() != sq)
            throw math_error("BehzBasis: table sizes do not match the bases");
        const ofhe_behz_tables tb{T.tQHatInvModq.data(), T.QHatModbsk.data(),  T.QHatModmtilde.data(),
                                  T.qInvModbsk.data(),   T.mtildeQHatInvModq.data(), &T.negQInvModmtilde,
                                  T.QModbsk.data(),      T.mtildeInvModbsk.data(),   T.tQInvModbsk.data(),
                                  T.BHatInvModb.data(),  T.BHatModq.data(),    T.BHatModmsk.data(),
                                  &T.BInvModmsk,         T.BModq.data()};
        ofhe_behz_t h = nullptr;
        check(ofhe_hip_behz_create(Q_->manager()->ctx(), Q_->LogN(), (uint32_t)sq, Q_->Moduli().data(), (uint32_t)sb,
                                   Bsk_->Moduli().data(), t, &tb, &h),
              "BehzBasis");
        h_.reset(h);
    }

    DCRTPolyHip FastBaseConvqToBskMontgomery(const DCRTPolyHip& x) const {
        check_over(x, *Q_, "FastBaseConvqToBskMontgomery");
        DCRTPolyHip out = DCRTPolyHip::result(QBsk_, Format::EVALUATION, x.Batch());
        check(ofhe_hip_behz_expand(h_.get(), Q_->plan(), Bsk_->plan(), x.GetFormat() == Format::EVALUATION, x.data(),
                                   out.data(), x.Batch(), nullptr),
              "FastBaseConvqToBskMontgomery");
        return out;
    }
    DCRTPolyHip FastRNSFloorq(const DCRTPolyHip& x) const {
        return coeff_step("FastRNSFloorq", ofhe_hip_behz_floor, x, QBsk_, Bsk_);
    }
    DCRTPolyHip FastBaseConvSK(const DCRTPolyHip& x) const {
        return coeff_step("FastBaseConvSK", ofhe_hip_behz_conv_sk, x, Bsk_, Q_);
    }
    // {cvMult[0], cvMult[1], cvMult[2]} over Q in COEFFICIENT form, as the reference leaves them
    std::vector<DCRTPolyHip> BfvMultBehz(const DCRTPolyHip& c0, const DCRTPolyHip& c1, const DCRTPolyHip& d0,
                                         const DCRTPolyHip& d1) const {
        auto out = bfv_mult_outputs("BfvMultBehz", Q_, c0, c1, d0, d1);
        check(ofhe_hip_bfv_eval_mult_behz(h_.get(), Q_->plan(), Bsk_->plan(), QBsk_->plan(), c0.data(), c1.data(),
                                          d0.data(), d1.data(), out[0].data(), out[1].data(), out[2].data(), c0.Batch(),
                                          nullptr),
              "BfvMultBehz");
        return out;
    }
    ofhe_behz_t handle() const { return h_.get(); }

private:
    // FastRNSFloorq and FastBaseConvSK: x over `from` in COEFFICIENT form -> `to`, COEFFICIENT
    DCRTPolyHip coeff_step(const char* op, int (*fn)(ofhe_behz_t, const uint64_t*, uint64_t*, uint32_t, void*),
                           const DCRTPolyHip& x, const std::shared_ptr<DCRTParams>& from,
                           const std::shared_ptr<DCRTParams>& to) const {
        check_over(x, *from, op);
        check_form(x, Format::COEFFICIENT, op);
        DCRTPolyHip out = DCRTPolyHip::result(to, Format::COEFFICIENT, x.Batch());
        check(fn(h_.get(), x.data(), out.data(), x.Batch(), nullptr), op);
        return out;
    }
    std::shared_ptr<DCRTParams> Q_, Bsk_, QBsk_;
    Handle<ofhe_behz_s, ofhe_hip_behz_destroy> h_;
};

// The decryption tables as the reference's getters return them
// (CryptoParametersBFVRNS, bfvrns-cryptoparameters.cpp:87-94, 446-495, 853-884).
// The HPS family reads the first four (the two B tables only where the reference
// fills them), BEHZ the next two; tInvModq / negQModt serve TimesQovert.  A
// table the technique does not read may stay empty.
struct BfvDecryptTables {
    std::vector<uint64_t> tQHatInvModqDivqModt, tQHatInvModqBDivqModt;
    std::vector<double> tQHatInvModqDivqFrac, tQHatInvModqBDivqFrac;
    std::vector<uint64_t> tgammaQHatInvModq, negInvqModtgamma, tInvModq;
    uint64_t negQModt = 0;
};

// PKEBFVRNS::Decrypt (bfvrns-pke.cpp:205-248) over Q for plaintext modulus t
// and technique OFHE_BFV_HPS / OFHE_BFV_HPSPOVERQ / OFHE_BFV_BEHZ:
//   ScaleAndRound  dcrtpoly-impl.h:1537-1814 / 2005-2049 (one tower: bfvrns-pke.cpp:233-245)
//                  Q, COEFFICIENT -> the batch * N words mod t, on the host
//   Decrypt        DecryptCore (rns-pke.cpp:199-224), INTT, ScaleAndRound: cv = 2 or 3
//                  elements over Q, all in one format; s the secret key, EVALUATION, batch 1
class BfvDecrypt {
public:
    BfvDecrypt(std::shared_ptr<DCRTParams> Q, uint64_t t, int technique, const BfvDecryptTables& T)
        : Q_(std::move(Q)) {
        const size_t sq = Q_->Towers();
        for (const auto* v : {&T.tQHatInvModqDivqModt, &T.tQHatInvModqBDivqModt, &T.tgammaQHatInvModq,
                              &T.negInvqModtgamma, &T.tInvModq})
            if (!v->empty() && v->size() != sq) throw math_error("BfvDecrypt: table sizes do not match the basis");
        for (const auto* v : {&T.tQHatInvModqDivqFrac, &T.tQHatInvModqBDivqFrac})
            if (!v->empty() && v->size() != sq) throw math_error("BfvDecrypt: table sizes do not match the basis");
        auto ptr = [](const auto& v) { return v.empty() ? nullptr : v.data(); };
        const ofhe_bfv_decrypt_tables tb{ptr(T.tQHatInvModqDivqModt), ptr(T.tQHatInvModqBDivqModt),
                                         ptr(T.tQHatInvModqDivqFrac), ptr(T.tQHatInvModqBDivqFrac),
                                         ptr(T.tgammaQHatInvModq),    ptr(T.negInvqModtgamma),
                                         ptr(T.tInvModq),             T.tInvModq.empty() ? nullptr : &T.negQModt};
        ofhe_bfv_decrypt_t h = nullptr;
        check(ofhe_hip_bfv_decrypt_create(Q_->manager()->ctx(), Q_->LogN(), (uint32_t)sq, Q_->Moduli().data(), t,
                                          technique, &tb, &h),
              "BfvDecrypt");
        h_.reset(h);
    }

    // the loop that runs: 0..7 for A..H, OFHE_BFV_DECRYPT_BEHZ, OFHE_BFV_DECRYPT_ONE_TOWER
    int Branch() const {
        int b = -1;
        check(ofhe_hip_bfv_decrypt_branch(h_.get(), &b), "BfvDecrypt::Branch");
        return b;
    }
    std::vector<uint64_t> ScaleAndRound(const DCRTPolyHip& x) const {
        check_over(x, *Q_, "ScaleAndRound");
        check_form(x, Format::COEFFICIENT, "ScaleAndRound");
        DeviceBuffer out(Q_->manager(), (size_t)x.Batch() * Q_->GetRingDimension());
        check(ofhe_hip_bfv_decrypt_scale_round(h_.get(), x.data(), out.get(), x.Batch(), nullptr), "ScaleAndRound");
        return fetch(out);
    }
    std::vector<uint64_t> Decrypt(const std::vector<DCRTPolyHip>& cv, const DCRTPolyHip& s) const {
        if (cv.size() != 2 && cv.size() != 3) throw math_error("Decrypt: 2 or 3 ciphertext elements expected");
        for (const auto& c : cv) {
            check_over(c, *Q_, "Decrypt");
            if (c.GetFormat() != cv[0].GetFormat() || c.Batch() != cv[0].Batch())
                throw math_error("Decrypt: elements of one format and one batch expected");
        }
        check_over(s, *Q_, "Decrypt");
        if (s.GetFormat() != Format::EVALUATION || s.Batch() != 1)
            throw math_error("Decrypt: the secret key in EVALUATION form, batch 1, expected");
        DeviceBuffer out(Q_->manager(), (size_t)cv[0].Batch() * Q_->GetRingDimension());
        check(ofhe_hip_bfv_decrypt(h_.get(), Q_->plan(), (uint32_t)cv.size(), cv[0].GetFormat() == Format::EVALUATION,
                                   cv[0].data(), cv[1].data(), cv.size() == 3 ? cv[2].data() : nullptr, s.data(),
                                   out.get(), cv[0].Batch(), nullptr),
              "Decrypt");
        return fetch(out);
    }
    const std::shared_ptr<DCRTParams>& GetParams() const { return Q_; }
    ofhe_bfv_decrypt_t handle() const { return h_.get(); }

private:
    static std::vector<uint64_t> fetch(const DeviceBuffer& d) {
        std::vector<uint64_t> h(d.size());
        d.download(h.data());
        return h;
    }
    std::shared_ptr<DCRTParams> Q_;
    Handle<ofhe_bfv_decrypt_s, ofhe_hip_bfv_decrypt_destroy> h_;
};

inline void DCRTPolyHip::TimesQovert(const BfvDecrypt& d) {
    check_over(*this, *d.GetParams(), "TimesQovert");
    check(ofhe_hip_times_q_over_t(d.handle(), data(), data(), batch_, nullptr), "TimesQovert");
}

// The rule DecryptCore and BgvDecrypt::Decrypt share (rns-pke.cpp:199-224): 2
// or 3 elements of one basis Q_l, one format and one batch, and the secret key
// in EVALUATION form, batch 1, over a chain whose first towers are Q_l (its
// DropLastElements).
inline void check_ciphertext(const std::vector<DCRTPolyHip>& cv, const DCRTPolyHip& s, const char* op) {
    if (cv.size() != 2 && cv.size() != 3) throw math_error(std::string(op) + ": 2 or 3 ciphertext elements expected");
    const auto& ql = cv[0].GetParams()->Moduli();
    for (const auto& c : cv) {
        check_over(c, *cv[0].GetParams(), op, ": elements over one basis expected");
        if (c.GetFormat() != cv[0].GetFormat() || c.Batch() != cv[0].Batch())
            throw math_error(std::string(op) + ": elements of one format and one batch expected");
    }
    const auto& q = s.GetParams()->Moduli();
    if (s.GetParams()->LogN() != cv[0].GetParams()->LogN() || q.size() < ql.size() ||
        !std::equal(ql.begin(), ql.end(), q.begin()))
        throw math_error(std::string(op) + ": the ciphertext's towers are not the first towers of the secret key's");
    if (s.GetFormat() != Format::EVALUATION || s.Batch() != 1)
        throw math_error(std::string(op) + ": the secret key in EVALUATION form, batch 1, expected");
}

// PKERNS::DecryptCore (rns-pke.cpp:199-224): b = c0 + c1 s (+ c2 s^2) over the
// ciphertext's towers, COEFFICIENT-form elements transformed first.  The result
// is in EVALUATION form, or with coeff_out in COEFFICIENT form, which is
// PKECKKSRNS::Decrypt (ckksrns-pke.cpp:44-97) and PKERNS::Decrypt
// (rns-pke.cpp:70-109) up to their last line: with one tower it is the
// NativePoly, with more the caller's CRTInterpolate follows on the host.
inline DCRTPolyHip DecryptCore(const std::vector<DCRTPolyHip>& cv, const DCRTPolyHip& s, bool coeff_out = false) {
    check_ciphertext(cv, s, "DecryptCore");
    const auto& Ql = cv[0].GetParams();
    DCRTPolyHip b = DCRTPolyHip::result(Ql, coeff_out ? Format::COEFFICIENT : Format::EVALUATION, cv[0].Batch());
    check(ofhe_hip_decrypt_core(Ql->plan(), (uint32_t)Ql->Towers(), (uint32_t)cv.size(),
                                cv[0].GetFormat() == Format::EVALUATION, coeff_out, cv[0].data(), cv[1].data(),
                                cv.size() == 3 ? cv[2].data() : nullptr, s.data(), b.data(), cv[0].Batch(), nullptr),
          "DecryptCore");
    return b;
}

// PKEBGVRNS::Decrypt (bgvrns-pke.cpp:44-99) over the chain Q for plaintext
// modulus t; the library builds negtInvModq and qlInvModq from the moduli.
//   ModReduceChain  the ModReduce steps Q_l -> q_0 (:55-60) of x over the first
//                   towers of Q, COEFFICIENT -> the batch * N words on the host:
//                   x_0 mod q_0, or with to_plaintext NativeVectorT::Mod(t) of it
//   Decrypt         cv = 2 or 3 elements over the first towers of Q; EVALUATION
//                   and COEFFICIENT elements take the reference's two branches
//   ScalingFactor   the scalingFactorInt of FLEXIBLEAUTO / FLEXIBLEAUTOEXT
//                   (:62-69, 82-89), host arithmetic on the caller's factors:
//                   factors[l] is GetModReduceFactorInt(l)
class BgvDecrypt {
public:
    BgvDecrypt(std::shared_ptr<DCRTParams> Q, uint64_t t) : Q_(std::move(Q)), t_(t) {
        ofhe_bgv_decrypt_t h = nullptr;
        check(ofhe_hip_bgv_decrypt_create(Q_->manager()->ctx(), Q_->LogN(), (uint32_t)Q_->Towers(),
                                          Q_->Moduli().data(), t, &h),
              "BgvDecrypt");
        h_.reset(h);
    }
    std::vector<uint64_t> ModReduceChain(const DCRTPolyHip& x, bool to_plaintext) const {
        check_form(x, Format::COEFFICIENT, "ModReduceChain");
        const uint32_t size_ql = level_of(x, "ModReduceChain");
        DeviceBuffer out(Q_->manager(), (size_t)x.Batch() * Q_->GetRingDimension());
        check(ofhe_hip_bgv_mod_reduce_chain(h_.get(), size_ql, to_plaintext, x.data(), out.get(), x.Batch(), nullptr),
              "ModReduceChain");
        return fetch(out);
    }
    std::vector<uint64_t> Decrypt(const std::vector<DCRTPolyHip>& cv, const DCRTPolyHip& s) const {
        check_ciphertext(cv, s, "Decrypt");
        check_over(s, *Q_, "Decrypt", ": the secret key is over another basis");
        const uint32_t size_ql = level_of(cv[0], "Decrypt");
        DeviceBuffer out(Q_->manager(), (size_t)cv[0].Batch() * Q_->GetRingDimension());
        check(ofhe_hip_bgv_decrypt(h_.get(), Q_->plan(), size_ql, (uint32_t)cv.size(),
                                   cv[0].GetFormat() == Format::EVALUATION, cv[0].data(), cv[1].data(),
                                   cv.size() == 3 ? cv[2].data() : nullptr, s.data(), out.get(), cv[0].Batch(),
                                   nullptr),
              "Decrypt");
        return fetch(out);
    }
    static uint64_t ScalingFactor(uint64_t scalingFactorInt, const std::vector<uint64_t>& factors, size_t sizeQl,
                                  uint64_t t) {
        if (t < 2 || sizeQl < 1 || (sizeQl > 1 && factors.size() < sizeQl))
            throw math_error("ScalingFactor: t >= 2 and one factor per level below sizeQl expected");
        unsigned __int128 sf = scalingFactorInt % t;
        for (size_t i = 0; i + 1 < sizeQl; i++) {
            // NativeInteger::ModInverse(t) by the extended Euclidean algorithm
            __int128 r0 = t, r1 = factors[sizeQl - 1 - i] % t, x0 = 0, x1 = 1;
            while (r1) {
                const __int128 qt = r0 / r1, r2 = r0 - qt * r1, x2 = x0 - qt * x1;
                r0 = r1, r1 = r2, x0 = x1, x1 = x2;
            }
            if (r0 != 1) throw math_error("ScalingFactor: a factor is not invertible mod t");
            sf = sf * (unsigned __int128)(x0 < 0 ? x0 + t : x0) % t;
        }
        return (uint64_t)sf;
    }
    const std::shared_ptr<DCRTParams>& GetParams() const { return Q_; }
    uint64_t GetPlaintextModulus() const { return t_; }
    ofhe_bgv_decrypt_t handle() const { return h_.get(); }

private:
    // x is over the first size_ql towers of Q
    uint32_t level_of(const DCRTPolyHip& x, const char* op) const {
        const auto &ql = x.GetParams()->Moduli(), &q = Q_->Moduli();
        if (x.GetParams()->LogN() != Q_->LogN() || ql.size() > q.size() || !std::equal(ql.begin(), ql.end(), q.begin()))
            throw math_error(std::string(op) + ": the polynomial is not over the first towers of the chain");
        return (uint32_t)ql.size();
    }
    static std::vector<uint64_t> fetch(const DeviceBuffer& d) {
        std::vector<uint64_t> h(d.size());
        d.download(h.data());
        return h;
    }
    std::shared_ptr<DCRTParams> Q_;
    uint64_t t_;
    Handle<ofhe_bgv_decrypt_s, ofhe_hip_bgv_decrypt_destroy> h_;
};

// BgvDecryptCache: one BgvDecrypt per (device, N, t, Q) -- the reference
// precomputes negtInvModq / qlInvModq once per CryptoParametersBGVRNS
// (bgvrns-cryptoparameters.cpp:91-107).
class BgvDecryptCache {
public:
    static std::shared_ptr<BgvDecrypt> get(const std::shared_ptr<DCRTParams>& Q, uint64_t t) {
        std::vector<uint64_t> key{(uint64_t)Q->manager()->device(), Q->LogN(), t};
        key.insert(key.end(), Q->Moduli().begin(), Q->Moduli().end());
        return Cache<std::vector<uint64_t>, BgvDecrypt>::get(key, [&] { return std::make_shared<BgvDecrypt>(Q, t); });
    }
};

// ApproxModDown (dcrtpoly-impl.h:1134-1175): x over Q|P (EVALUATION) -> Q.
inline DCRTPolyHip ApproxModDown(const DCRTPolyHip& x, const std::shared_ptr<DCRTParams>& paramsQ,
                                 const std::shared_ptr<DCRTParams>& paramsP, const BaseConverter& p_to_q,
                                 const std::vector<uint64_t>& PInvModq, uint64_t t = 0) {
    check_form(x, Format::EVALUATION, "ApproxModDown");
    if (x.GetParams()->Towers() != paramsQ->Towers() + paramsP->Towers())
        throw math_error("ApproxModDown: tower count mismatch");
    if (PInvModq.size() != paramsQ->Towers()) throw math_error("ApproxModDown: PInvModq size");
    DCRTPolyHip out = DCRTPolyHip::result(paramsQ, Format::EVALUATION, x.Batch());
    check(ofhe_hip_approx_mod_down(paramsQ->plan(), paramsP->plan(), p_to_q.handle(), PInvModq.data(), t, x.data(),
                                   out.data(), x.Batch(), nullptr),
          "ApproxModDown");
    return out;
}

// KeySwitchHYBRID (pke/lib/keyswitch/keyswitch-hybrid.cpp) for one parameter
// set: Q (element params), P (GetParamsP()) and dnum = numPartQ.  An
// evaluation key is a pair of DCRTPolyHip over Q|P with batch = numPartQ
// (the b and a vectors of EvalKeyRelin).
class KeySwitchHybrid {
public:
    KeySwitchHybrid(const DCRTParams& Q, const DCRTParams& P, uint32_t numPartQ) {
        ofhe_ks_t h = nullptr;
        check(ofhe_hip_ks_create(Q.manager()->ctx(), Q.LogN(), (uint32_t)Q.Towers(), Q.Moduli().data(),
                                 Q.Roots().data(), (uint32_t)P.Towers(), P.Moduli().data(), P.Roots().data(), numPartQ,
                                 &h),
              "KeySwitchHybrid");
        h_.reset(h);
        sizeQ_ = Q.Towers();
        sizeP_ = P.Towers();
        numPartQ_ = numPartQ;
    }

    // KeySwitchCore(a, evalKey) (keyswitch-hybrid.cpp:325-328): c is over Ql
    // (its params give the level), EVALUATION form.  t > 0 for BGV.
    std::pair<DCRTPolyHip, DCRTPolyHip> KeySwitchCore(const DCRTPolyHip& c, const DCRTPolyHip& key_b,
                                                      const DCRTPolyHip& key_a, uint64_t t = 0) const {
        check_form(c, Format::EVALUATION, "KeySwitchCore");
        const uint32_t l = (uint32_t)c.GetParams()->Towers();
        if (l > sizeQ_) throw math_error("KeySwitchCore: ciphertext has more towers than Q");
        check_key("KeySwitchCore", &key_b, &key_a);
        auto o = DCRTPolyHip::result_pair(c.GetParams(), Format::EVALUATION, c.Batch());
        check(ofhe_hip_ks_core(h_.get(), l, c.data(), key_b.data(), key_a.data(), o.first.data(), o.second.data(), t,
                               c.Batch(), nullptr),
              "KeySwitchCore");
        return o;
    }

    // one relinearisation key: the b and a polynomials, as KeySwitchCore takes them
    typedef std::pair<const DCRTPolyHip*, const DCRTPolyHip*> RelinKey;

    // LeveledSHEBase::EvalMult(ct1, ct2, evalKey) (base-leveledshe.cpp:199-218)
    // followed by `levels` rescalings (ModReduceInternalInPlace:
    // ckksrns-leveledshe.cpp:107-132 for OFHE_SHE_CKKS, t = 0;
    // bgvrns-leveledshe.cpp:45-77 for OFHE_SHE_BGV with plaintext modulus t).
    // The result is over the first Towers() - levels moduli of the operands.
    std::pair<DCRTPolyHip, DCRTPolyHip> EvalMult(const DCRTPolyHip& c0, const DCRTPolyHip& c1, const DCRTPolyHip& d0,
                                                 const DCRTPolyHip& d1, const DCRTPolyHip& key_b,
                                                 const DCRTPolyHip& key_a, int scheme = OFHE_SHE_CKKS, uint64_t t = 0,
                                                 uint32_t levels = 0) const {
        return mult("EvalMult", c0, c1, &d0, &d1, key_b, key_a, scheme, t, levels);
    }
    // LeveledSHEBase::EvalSquare(ct, evalKey) (base-leveledshe.cpp:262-280), then `levels` rescalings
    std::pair<DCRTPolyHip, DCRTPolyHip> EvalSquare(const DCRTPolyHip& c0, const DCRTPolyHip& c1,
                                                   const DCRTPolyHip& key_b, const DCRTPolyHip& key_a,
                                                   int scheme = OFHE_SHE_CKKS, uint64_t t = 0,
                                                   uint32_t levels = 0) const {
        return mult("EvalSquare", c0, c1, nullptr, nullptr, key_b, key_a, scheme, t, levels);
    }
    // LeveledSHEBase::Relinearize (base-leveledshe.cpp:350-372): cv has 3 or
    // more elements, keys[j - 2] = (b, a) switches element j
    std::pair<DCRTPolyHip, DCRTPolyHip> Relinearize(const std::vector<const DCRTPolyHip*>& cv,
                                                    const std::vector<RelinKey>& keys, uint64_t t = 0) const {
        if (cv.size() < 3) throw math_error("Relinearize: 3 or more ciphertext elements expected");
        if (keys.size() + 2 != cv.size()) throw math_error("Relinearize: one evaluation key per element past the second");
        const uint32_t l = she_level("Relinearize", cv);
        std::vector<const uint64_t*> c;
        for (const DCRTPolyHip* e : cv) c.push_back(e->data());
        for (const RelinKey& k : keys) check_key("Relinearize", k.first, k.second);
        const KeyPtrs k = key_ptrs(keys);
        const DCRTPolyHip& f = *cv[0];
        auto o = DCRTPolyHip::result_pair(f.GetParams(), Format::EVALUATION, f.Batch());
        check(ofhe_hip_ks_relinearize(h_.get(), l, (uint32_t)cv.size(), c.data(), k.b.data(), k.a.data(),
                                      o.first.data(), o.second.data(), t, f.Batch(), nullptr),
              "Relinearize");
        return o;
    }
    // ModReduceInternalInPlace (ckksrns-leveledshe.cpp:107-132, bgvrns-leveledshe.cpp:45-77) of every
    // element of cv: `levels` >= 1 towers dropped, the results over the lowered params
    std::vector<DCRTPolyHip> Rescale(const std::vector<const DCRTPolyHip*>& cv, int scheme = OFHE_SHE_CKKS,
                                     uint64_t t = 0, uint32_t levels = 1) const {
        if (cv.empty()) throw math_error("Rescale: one or more ciphertext elements expected");
        const uint32_t l = she_level("Rescale", cv);
        if (levels < 1 || levels >= l) throw math_error("Rescale: levels must be in [1, towers - 1]");
        auto lp = lowered(*cv[0]->GetParams(), levels);
        std::vector<DCRTPolyHip> out;
        std::vector<const uint64_t*> x;
        std::vector<uint64_t*> o;
        for (const DCRTPolyHip* e : cv) {
            out.push_back(DCRTPolyHip::result(lp, Format::EVALUATION, e->Batch()));
            x.push_back(e->data());
        }
        for (DCRTPolyHip& r : out) o.push_back(r.data());
        check(ofhe_hip_ks_rescale(h_.get(), l, scheme, t, levels, (uint32_t)cv.size(), x.data(), o.data(),
                                  cv[0]->Batch(), nullptr),
              "Rescale");
        return out;
    }

    // The digits of one ciphertext's c1 (EvalKeySwitchPrecomputeCore), kept on
    // the device for any number of hoisted rotations.
    struct HoistedDigits {
        DeviceBuffer buf;        // [batch][beta][size_ql + sizeP][N]
        uint32_t size_ql = 0, batch = 0;
    };
    // one evaluation key per rotation: the b and a polynomials, as KeySwitchCore takes them
    typedef std::pair<const DCRTPolyHip*, const DCRTPolyHip*> RotationKey;
    typedef std::vector<std::pair<DCRTPolyHip, DCRTPolyHip>> Rotations;

    // LeveledSHEBase::EvalFastRotationPrecompute (base-leveledshe.cpp:462-469)
    HoistedDigits FastRotationPrecompute(const DCRTPolyHip& c1) const {
        check_form(c1, Format::EVALUATION, "FastRotationPrecompute");
        const uint32_t l = (uint32_t)c1.GetParams()->Towers();
        if (l > sizeQ_) throw math_error("FastRotationPrecompute: ciphertext has more towers than Q");
        uint32_t beta = 0;
        check(ofhe_hip_ks_digits(h_.get(), l, nullptr, &beta), "FastRotationPrecompute");
        HoistedDigits d;
        d.buf = DeviceBuffer(c1.GetParams()->manager(),
                             (size_t)c1.Batch() * beta * (l + sizeP_) * c1.GetParams()->GetRingDimension());
        d.size_ql = l;
        d.batch = c1.Batch();
        check(ofhe_hip_ks_precompute(h_.get(), l, c1.data(), d.buf.get(), d.batch, nullptr), "FastRotationPrecompute");
        return d;
    }

    // LeveledSHEBase::EvalFastRotation (base-leveledshe.cpp:471-513) for every
    // index of autoIndex: one (c0', c1') pair per rotation over c0's params.
    Rotations FastRotation(const DCRTPolyHip& c0, const HoistedDigits& digits, const std::vector<uint32_t>& autoIndex,
                           const std::vector<RotationKey>& keys, uint64_t t = 0) const {
        rot_check("FastRotation", &c0, digits, autoIndex, keys);
        if (c0.GetParams()->Towers() != digits.size_ql)
            throw math_error("FastRotation: c0 and the digits are at different levels");
        return rot_run(c0.GetParams(), digits, autoIndex, keys, [&](const KeyPtrs& k, uint64_t* o0, uint64_t* o1) {
            check(ofhe_hip_ks_fast_rotation(h_.get(), digits.size_ql, digits.buf.get(), c0.data(),
                                            (uint32_t)autoIndex.size(), autoIndex.data(), k.b.data(), k.a.data(), o0,
                                            o1, t, digits.batch, nullptr),
                  "FastRotation");
        });
    }

    // LeveledSHECKKSRNS::EvalFastRotationExt (ckksrns-leveledshe.cpp:402-457):
    // pairs over the caller's Ql|P params; c0 = nullptr for addFirst = false.
    Rotations FastRotationExt(const DCRTPolyHip* c0, const HoistedDigits& digits,
                              const std::vector<uint32_t>& autoIndex, const std::vector<RotationKey>& keys,
                              const std::shared_ptr<DCRTParams>& paramsQlP) const {
        rot_check("FastRotationExt", c0, digits, autoIndex, keys);
        if (c0 && c0->GetParams()->Towers() != digits.size_ql)
            throw math_error("FastRotationExt: c0 and the digits are at different levels");
        if (!paramsQlP || paramsQlP->Towers() != digits.size_ql + sizeP_)
            throw math_error("FastRotationExt: paramsQlP must have the level's towers plus P");
        return rot_run(paramsQlP, digits, autoIndex, keys, [&](const KeyPtrs& k, uint64_t* o0, uint64_t* o1) {
            check(ofhe_hip_ks_fast_rotation_ext(h_.get(), digits.size_ql, digits.buf.get(), c0 ? c0->data() : nullptr,
                                                (uint32_t)autoIndex.size(), autoIndex.data(), k.b.data(),
                                                k.a.data(), o0, o1, digits.batch, nullptr),
                  "FastRotationExt");
        });
    }

    // ---- BSGS linear transform (FHECKKSRNS::EvalLinearTransform, ckksrns-fhe.cpp:1484-1555) ----
    // Polynomials that the C ABI takes as [count][batch][towers][N] are one
    // DCRTPolyHip whose Batch() is count * batch, count-major.

    // KeySwitchHYBRID::KeySwitchExt (keyswitch-hybrid.cpp:231-256) on one
    // element: c over Ql -> c * PModq on the Q towers of paramsQlP, zero on P.
    DCRTPolyHip KeySwitchExt(const DCRTPolyHip& c, const std::shared_ptr<DCRTParams>& paramsQlP) const {
        check_form(c, Format::EVALUATION, "KeySwitchExt");
        const uint32_t l = (uint32_t)c.GetParams()->Towers();
        ext_params("KeySwitchExt", paramsQlP, l);
        DCRTPolyHip out = DCRTPolyHip::result(paramsQlP, Format::EVALUATION, c.Batch());
        check(ofhe_hip_ks_ext(h_.get(), l, c.data(), out.data(), c.Batch(), nullptr), "KeySwitchExt");
        return out;
    }

    // EvalMultExt / EvalAddExtInPlace over the inner loop of 1520-1526:
    // out_e[j] = sum_i x_e[i] * diag[j * nterm + i].  x0, x1: nterm * batch
    // polynomials over Ql|P; diag: nsum * nterm; present: empty (all) or one
    // byte per diagonal.  Returns (out0, out1) with nsum * batch polynomials each.
    std::pair<DCRTPolyHip, DCRTPolyHip> MultExtSum(const DCRTPolyHip& x0, const DCRTPolyHip& x1, uint32_t nterm,
                                                   const DCRTPolyHip& diag, const std::vector<uint8_t>& present,
                                                   uint32_t nsum) const {
        const auto& op = x0.GetParams();
        for (const DCRTPolyHip* v : {&x0, &x1, &diag}) check_form(*v, Format::EVALUATION, "MultExtSum");
        if (op->Towers() <= sizeP_ || x1.GetParams()->Moduli() != op->Moduli() ||
            diag.GetParams()->Moduli() != op->Moduli())
            throw math_error("MultExtSum: the terms and the diagonals must be over one Ql|P basis");
        if (!nterm || !nsum || x0.Batch() % nterm || x1.Batch() != x0.Batch() || diag.Batch() != (size_t)nsum * nterm)
            throw math_error("MultExtSum: nterm * batch terms and nsum * nterm diagonals required");
        if (!present.empty() && present.size() != (size_t)nsum * nterm)
            throw math_error("MultExtSum: one presence byte per diagonal required");
        const uint32_t batch = x0.Batch() / nterm, l = (uint32_t)(op->Towers() - sizeP_);
        const uint64_t poly = (uint64_t)op->Towers() * op->GetRingDimension();
        auto o = DCRTPolyHip::result_pair(op, Format::EVALUATION, nsum * batch);
        check(ofhe_hip_ks_mult_ext_sum(h_.get(), l, nterm, x0.data(), x1.data(), batch * poly, diag.data(), poly,
                                       present.empty() ? nullptr : present.data(), nsum, o.first.data(),
                                       o.second.data(), batch, nullptr),
              "MultExtSum");
        return o;
    }

    // Sum over the digit sets of EvalFastRotationExt(., autoIndex[j], digits_j, false)
    // under keys[j] (1544-1545).  digits: FastRotationPrecompute of nset * batch
    // polynomials, set-major; addend1: nadd * batch polynomials over Ql|P added
    // to the second element, or nullptr.
    std::pair<DCRTPolyHip, DCRTPolyHip> FastRotationExtSum(const HoistedDigits& digits,
                                                           const std::vector<uint32_t>& autoIndex,
                                                           const std::vector<RotationKey>& keys,
                                                           const DCRTPolyHip* addend1,
                                                           const std::shared_ptr<DCRTParams>& paramsQlP) const {
        rot_check("FastRotationExtSum", nullptr, digits, autoIndex, keys);
        ext_params("FastRotationExtSum", paramsQlP, digits.size_ql);
        const uint32_t nset = (uint32_t)autoIndex.size();
        if (digits.batch % nset) throw math_error("FastRotationExtSum: the digits must hold nset * batch polynomials");
        const uint32_t batch = digits.batch / nset;
        if (addend1 && (addend1->GetFormat() != Format::EVALUATION || addend1->Batch() % batch ||
                        addend1->GetParams()->Moduli() != paramsQlP->Moduli()))
            throw math_error("FastRotationExtSum: addend1 must be nadd * batch EVALUATION polynomials over Ql|P");
        const KeyPtrs k = key_ptrs(keys);
        auto o = DCRTPolyHip::result_pair(paramsQlP, Format::EVALUATION, batch);
        check(ofhe_hip_ks_fast_rotation_ext_sum(h_.get(), digits.size_ql, nset, digits.buf.get(), autoIndex.data(),
                                                k.b.data(), k.a.data(), addend1 ? addend1->data() : nullptr,
                                                addend1 ? addend1->Batch() / batch : 0, o.first.data(),
                                                o.second.data(), batch, nullptr),
              "FastRotationExtSum");
        return o;
    }

    // One BSGS level: indices, key ids and presence.  An index = 1 mod 2N is
    // the reference's no-rotation branch and its key id is ignored.
    struct BsgsPlan {
        std::vector<uint32_t> babyIndex, giantIndex;  // automorphism indices (FindAutomorphismIndex2nComplex)
        std::vector<std::string> babyKey, giantKey;   // KeyCache ids of the rotation keys
        std::vector<uint8_t> present;                 // [ngiant * nbaby], empty: every diagonal exists
    };
    // (c0, c1) over Ql -> the transform's (c0', c1') over Ql; diag: ngiant *
    // nbaby polynomials over Ql|P, diag[j * nbaby + i] for giant j and baby i,
    // uploaded once at setup.  Defined after KeyCache.
    std::pair<DCRTPolyHip, DCRTPolyHip> LinearTransform(const DCRTPolyHip& c0, const DCRTPolyHip& c1,
                                                        const BsgsPlan& plan, const DCRTPolyHip& diag,
                                                        uint64_t t = 0) const;

    ofhe_ks_t handle() const { return h_.get(); }

private:
    void ext_params(const char* op, const std::shared_ptr<DCRTParams>& paramsQlP, size_t l) const {
        if (l > sizeQ_) throw math_error(std::string(op) + ": ciphertext has more towers than Q");
        if (!paramsQlP || paramsQlP->Towers() != l + sizeP_)
            throw math_error(std::string(op) + ": paramsQlP must have the level's towers plus P");
    }
    // The evaluation-key rule, known here alone: numPartQ polynomials over Q|P each
    void check_key(const char* op, const DCRTPolyHip* key_b, const DCRTPolyHip* key_a) const {
        if (!key_b || !key_a || key_b->Batch() != numPartQ_ || key_a->Batch() != numPartQ_ ||
            key_b->GetParams()->Towers() != sizeQ_ + sizeP_ || key_a->GetParams()->Towers() != sizeQ_ + sizeP_)
            throw math_error(std::string(op) + ": evaluation key must be numPartQ polynomials over Q|P");
    }
    // The (b, a) pointer lists the C ABI takes, from a list of keys; a NULL pair (an identity step) stays NULL
    struct KeyPtrs {
        std::vector<const uint64_t*> b, a;
    };
    static KeyPtrs key_ptrs(const std::vector<RotationKey>& keys) {
        KeyPtrs k;
        for (const auto& key : keys) {
            k.b.push_back(key.first ? key.first->data() : nullptr);
            k.a.push_back(key.second ? key.second->data() : nullptr);
        }
        return k;
    }
    // every element in EVALUATION form, over one basis of at most Q's towers, of one batch: the level
    uint32_t she_level(const char* op, const std::vector<const DCRTPolyHip*>& cv) const {
        const std::string w(op);
        for (const DCRTPolyHip* e : cv) {
            if (!e) throw math_error(w + ": NULL ciphertext element");
            check_form(*e, Format::EVALUATION, op);
            if (e->GetParams()->Moduli() != cv[0]->GetParams()->Moduli() || e->Batch() != cv[0]->Batch())
                throw math_error(w + ": elements over one basis and of one batch expected");
        }
        const size_t l = cv[0]->GetParams()->Towers();
        if (l > sizeQ_) throw math_error(w + ": ciphertext has more towers than Q");
        return (uint32_t)l;
    }
    std::pair<DCRTPolyHip, DCRTPolyHip> mult(const char* op, const DCRTPolyHip& c0, const DCRTPolyHip& c1,
                                             const DCRTPolyHip* d0, const DCRTPolyHip* d1, const DCRTPolyHip& key_b,
                                             const DCRTPolyHip& key_a, int scheme, uint64_t t, uint32_t levels) const {
        std::vector<const DCRTPolyHip*> cv{&c0, &c1};
        if (d0) cv.insert(cv.end(), {d0, d1});
        const uint32_t l = she_level(op, cv);
        check_key(op, &key_b, &key_a);
        if (levels >= l) throw math_error(std::string(op) + ": levels must be below the towers of the operands");
        auto lp = levels ? lowered(*c0.GetParams(), levels) : c0.GetParams();
        auto o = DCRTPolyHip::result_pair(lp, Format::EVALUATION, c0.Batch());
        check(ofhe_hip_ks_eval_mult(h_.get(), l, c0.data(), c1.data(), d0 ? d0->data() : nullptr,
                                    d1 ? d1->data() : nullptr, key_b.data(), key_a.data(), scheme, t, levels,
                                    o.first.data(), o.second.data(), c0.Batch(), nullptr),
              op);
        return o;
    }
    void rot_check(const char* op, const DCRTPolyHip* c0, const HoistedDigits& digits,
                   const std::vector<uint32_t>& autoIndex, const std::vector<RotationKey>& keys) const {
        const std::string w(op);
        if (!digits.buf.get() || !digits.size_ql) throw math_error(w + ": empty digits");
        if (c0) check_form(*c0, Format::EVALUATION, op);
        if (c0 && c0->Batch() != digits.batch) throw math_error(w + ": batch mismatch");
        if (autoIndex.empty() || autoIndex.size() != keys.size())
            throw math_error(w + ": one evaluation key per automorphism index required");
        for (const auto& k : keys) check_key(op, k.first, k.second);
    }
    // The C ABI writes [nrot][batch][towers][N]; every rotation gets a
    // DCRTPolyHip of its own, filled by one device copy.
    template <class F>
    Rotations rot_run(const std::shared_ptr<DCRTParams>& op, const HoistedDigits& digits,
                      const std::vector<uint32_t>& autoIndex, const std::vector<RotationKey>& keys, F call) const {
        const KeyPtrs k = key_ptrs(keys);
        const size_t per = (size_t)digits.batch * op->Towers() * op->GetRingDimension(), nrot = autoIndex.size();
        DeviceBuffer all0(op->manager(), nrot * per), all1(op->manager(), nrot * per);
        call(k, all0.get(), all1.get());
        Rotations out;
        for (size_t r = 0; r < nrot; r++) {
            auto o = DCRTPolyHip::result_pair(op, Format::EVALUATION, digits.batch);
            check(ofhe_hip_copy_device(op->manager()->ctx(), o.first.data(), all0.get() + r * per, per * 8, nullptr),
                  "FastRotation");
            check(ofhe_hip_copy_device(op->manager()->ctx(), o.second.data(), all1.get() + r * per, per * 8, nullptr),
                  "FastRotation");
            out.push_back(std::move(o));
        }
        return out;
    }

    Handle<ofhe_ks_s, ofhe_hip_ks_destroy> h_;
    size_t sizeQ_ = 0, sizeP_ = 0;
    uint32_t numPartQ_ = 0;
};

// KsCache: one KeySwitchHybrid per (device, N, Q, P, dnum) -- the reference
// precomputes its HYBRID CRT tables once per CryptoParametersRNS
// (rns-cryptoparameters.cpp:72-345).
class KsCache {
public:
    static std::shared_ptr<KeySwitchHybrid> get(const DCRTParams& Q, const DCRTParams& P, uint32_t numPartQ) {
        std::vector<uint64_t> key{(uint64_t)Q.manager()->device(), Q.LogN(), numPartQ, Q.Towers()};
        key.insert(key.end(), Q.Moduli().begin(), Q.Moduli().end());
        key.insert(key.end(), P.Moduli().begin(), P.Moduli().end());
        return Cache<std::vector<uint64_t>, KeySwitchHybrid>::get(
            key, [&] { return std::make_shared<KeySwitchHybrid>(Q, P, numPartQ); });
    }
};

// KeyCache: evaluation keys resident on the device, uploaded once per key
// (when EvalMultKeyGen / EvalAtIndexKeyGen store them) and looked up by the
// caller's key id (e.g. the EvalKey's tag) at every key switch.
class KeyCache {
public:
    struct Key {
        DCRTPolyHip b, a;  // numPartQ polynomials over Q|P each (EvalKeyRelin's b and a vectors)
    };
    static std::shared_ptr<const Key> put(const std::string& id, DCRTPolyHip b, DCRTPolyHip a) {
        auto k = std::make_shared<const Key>(Key{std::move(b), std::move(a)});
        NamedStore<Key>::put(id, k);
        return k;
    }
    static std::shared_ptr<const Key> get(const std::string& id) {
        auto k = NamedStore<Key>::find(id);
        if (!k) throw math_error("KeyCache: no evaluation key '" + id + "'");
        return k;
    }
    static void erase(const std::string& id) { NamedStore<Key>::erase(id); }
};

// KeySwitchBV (pke/lib/keyswitch/keyswitch-bv.cpp) for one parameter set: Q
// (element params) and digitSize (CryptoParametersRNS::GetDigitSize(); 0: one
// digit per tower, r > 0: base-2^r digits, DCRTPolyImpl::CRTDecompose(r)).  An
// evaluation key is held as KeySwitchHybrid holds its keys: one DCRTPolyHip per
// half (EvalKeyRelin's b and a vectors) over Q, whose batch index is the digit.
class KeySwitchBV {
public:
    typedef KeyCache::Key Key;
    // EvalKeySwitchPrecomputeCore's digits, kept on the device: `batch` entries of n_digits polynomials
    struct Digits {
        DCRTPolyHip poly;  // [batch][n_digits] polynomials over the level's towers, EVALUATION form
        uint32_t n_digits, batch;
    };

    KeySwitchBV(std::shared_ptr<DCRTParams> Q, uint32_t digitSize) : Q_(std::move(Q)), r_(digitSize) {
        if (r_ > kMaxDigitSize) throw math_error("KeySwitchBV: digitSize must be at most 30");
    }
    uint32_t GetDigitSize() const { return r_; }

    // CRTDecompose(digitSize)'s nWindows over the first `towers` of `moduli`; no device
    static uint32_t DigitCount(const std::vector<uint64_t>& moduli, size_t towers, uint32_t digitSize) {
        if (digitSize > kMaxDigitSize) throw math_error("DigitCount: digitSize must be at most 30");
        if (towers < 1 || towers > moduli.size()) throw math_error("DigitCount: towers must be in [1, moduli]");
        uint32_t n = 0;
        for (size_t i = 0; i < towers; i++) {
            uint32_t bits = 0;
            for (uint64_t q = moduli[i]; q; q >>= 1) bits++;
            n += digitSize ? (bits + digitSize - 1) / digitSize : 1;
        }
        return n;
    }

    // EvalKeySwitchPrecomputeCore (keyswitch-bv.cpp:308-312): c over Ql (its params give the level)
    Digits EvalKeySwitchPrecomputeCore(const DCRTPolyHip& c) const {
        const uint32_t l = level("EvalKeySwitchPrecomputeCore", c);
        const uint32_t nd = DigitCount(Q_->Moduli(), l, r_);
        Digits d{DCRTPolyHip::result(c.GetParams(), Format::EVALUATION, c.Batch() * nd), nd, c.Batch()};
        check(ofhe_hip_bv_precompute_digits(Q_->plan(), l, r_, c.data(), d.poly.data(), c.Batch(), nullptr),
              "EvalKeySwitchPrecomputeCore");
        return d;
    }

    // EvalFastKeySwitchCore (keyswitch-bv.cpp:314-338): (ct0, ct1) over paramsQl, the key cut to its towers
    std::pair<DCRTPolyHip, DCRTPolyHip> EvalFastKeySwitchCore(const Digits& digits, const Key& key,
                                                              const std::shared_ptr<DCRTParams>& paramsQl) const {
        check_form(digits.poly, Format::EVALUATION, "EvalFastKeySwitchCore");
        check_over(digits.poly, *paramsQl, "EvalFastKeySwitchCore", ": the digits are over another basis than paramsQl");
        const uint32_t l = level("EvalFastKeySwitchCore", digits.poly);
        if (!digits.n_digits || digits.poly.Batch() != digits.batch * digits.n_digits)
            throw math_error("EvalFastKeySwitchCore: batch * n_digits digit polynomials expected");
        check_key("EvalFastKeySwitchCore", key, digits.n_digits);
        auto o = DCRTPolyHip::result_pair(paramsQl, Format::EVALUATION, digits.batch);
        check(ofhe_hip_bv_core_digits(Q_->plan(), l, digits.n_digits, digits.poly.data(), key.b.data(), key.a.data(),
                                      (uint32_t)Q_->Towers(), o.first.data(), o.second.data(), digits.batch, nullptr),
              "EvalFastKeySwitchCore");
        return o;
    }

    // KeySwitchCore (keyswitch-bv.cpp:302-306), the digits produced and consumed in chunks on the device
    std::pair<DCRTPolyHip, DCRTPolyHip> KeySwitchCore(const DCRTPolyHip& c, const Key& key) const {
        const uint32_t l = level("KeySwitchCore", c);
        check_key("KeySwitchCore", key, DigitCount(Q_->Moduli(), l, r_));
        auto o = DCRTPolyHip::result_pair(c.GetParams(), Format::EVALUATION, c.Batch());
        run("KeySwitchCore", l, c, key, nullptr, nullptr, o.first, o.second);
        return o;
    }

    // KeySwitchInPlace (keyswitch-bv.cpp:283-300) on the elements of a ciphertext: c0 += ct0, and c1 = ct1
    // (two elements) or c1 += ct1 with the third element dropped (three)
    void KeySwitchInPlace(std::vector<DCRTPolyHip>& cv, const Key& key) const {
        if (cv.size() != 2 && cv.size() != 3) throw math_error("KeySwitchInPlace: 2 or 3 ciphertext elements expected");
        const DCRTPolyHip& c = cv.back();
        const uint32_t l = level("KeySwitchInPlace", c);
        for (const DCRTPolyHip& e : cv) {
            check_form(e, Format::EVALUATION, "KeySwitchInPlace");
            if (e.GetParams()->Moduli() != c.GetParams()->Moduli() || e.Batch() != c.Batch())
                throw math_error("KeySwitchInPlace: elements over one basis and of one batch expected");
        }
        check_key("KeySwitchInPlace", key, DigitCount(Q_->Moduli(), l, r_));
        // two elements: c1 is both the input and, once consumed, the output
        run("KeySwitchInPlace", l, c, key, &cv[0], cv.size() == 3 ? &cv[1] : nullptr, cv[0], cv[1]);
        if (cv.size() == 3) cv.pop_back();
    }

private:
    static constexpr uint32_t kMaxDigitSize = 30;  // the reference forms 1 << digitSize in an int
    uint32_t level(const char* op, const DCRTPolyHip& c) const {
        check_form(c, Format::EVALUATION, op);
        const size_t l = c.GetParams()->Towers();
        if (l > Q_->Towers()) throw math_error(std::string(op) + ": ciphertext has more towers than Q");
        if (c.GetParams()->LogN() != Q_->LogN() || c.GetParams()->Moduli() != towers_of(Q_->Moduli(), 0, l))
            throw math_error(std::string(op) + ": the polynomial is not over the first towers of Q");
        return (uint32_t)l;
    }
    void check_key(const char* op, const Key& key, uint32_t n_digits) const {
        check_over(key.b, *Q_, op, ": evaluation key must be polynomials over Q");
        check_over(key.a, *Q_, op, ": evaluation key must be polynomials over Q");
        check_form(key.b, Format::EVALUATION, op);
        check_form(key.a, Format::EVALUATION, op);
        if (key.b.Batch() < n_digits || key.a.Batch() < n_digits)
            throw math_error(std::string(op) + ": evaluation key has fewer polynomials than the level has digits");
    }
    void run(const char* op, uint32_t l, const DCRTPolyHip& c, const Key& key, const DCRTPolyHip* add0,
             const DCRTPolyHip* add1, DCRTPolyHip& out0, DCRTPolyHip& out1) const {
        check(ofhe_hip_bv_key_switch(Q_->plan(), l, r_, c.data(), key.b.data(), key.a.data(), (uint32_t)Q_->Towers(),
                                     add0 ? add0->data() : nullptr, add1 ? add1->data() : nullptr, out0.data(),
                                     out1.data(), 0, c.Batch(), nullptr),
              op);
    }
    std::shared_ptr<DCRTParams> Q_;
    uint32_t r_;
};

inline std::pair<DCRTPolyHip, DCRTPolyHip> KeySwitchHybrid::LinearTransform(const DCRTPolyHip& c0,
                                                                            const DCRTPolyHip& c1,
                                                                            const BsgsPlan& plan,
                                                                            const DCRTPolyHip& diag,
                                                                            uint64_t t) const {
    for (const DCRTPolyHip* v : {&c0, &c1, &diag}) check_form(*v, Format::EVALUATION, "LinearTransform");
    const size_t l = c0.GetParams()->Towers(), nb = plan.babyIndex.size(), ng = plan.giantIndex.size();
    if (l > sizeQ_ || c1.GetParams()->Moduli() != c0.GetParams()->Moduli() || c1.Batch() != c0.Batch())
        throw math_error("LinearTransform: c0 and c1 must be one ciphertext over Ql");
    if (!nb || !ng || plan.babyKey.size() != nb || plan.giantKey.size() != ng)
        throw math_error("LinearTransform: one key id per baby and giant step required");
    if (diag.GetParams()->Towers() != l + sizeP_ || diag.Batch() != nb * ng)
        throw math_error("LinearTransform: ngiant * nbaby diagonals over Ql|P required");
    if (!plan.present.empty() && plan.present.size() != nb * ng)
        throw math_error("LinearTransform: one presence byte per diagonal required");
    const uint64_t two_n = 2 * (uint64_t)c0.GetParams()->GetRingDimension();
    std::vector<std::shared_ptr<const KeyCache::Key>> hold;  // resident keys stay alive through the call
    KeyPtrs k[2];  // baby, giant
    for (int g = 0; g < 2; g++) {
        const auto& idx = g ? plan.giantIndex : plan.babyIndex;
        const auto& ids = g ? plan.giantKey : plan.babyKey;
        std::vector<RotationKey> keys(idx.size(), RotationKey{nullptr, nullptr});  // the identity steps stay NULL
        for (size_t i = 0; i < idx.size(); i++) {
            if (idx[i] % two_n == 1) continue;
            hold.push_back(KeyCache::get(ids[i]));
            keys[i] = {&hold.back()->b, &hold.back()->a};
            check_key("LinearTransform", keys[i].first, keys[i].second);
        }
        k[g] = key_ptrs(keys);
    }
    ofhe_bsgs tr{};
    tr.nbaby = (uint32_t)nb;
    tr.ngiant = (uint32_t)ng;
    tr.baby_index = plan.babyIndex.data();
    tr.giant_index = plan.giantIndex.data();
    tr.baby_key_b = k[0].b.data();
    tr.baby_key_a = k[0].a.data();
    tr.giant_key_b = k[1].b.data();
    tr.giant_key_a = k[1].a.data();
    tr.diag = diag.data();
    tr.diag_stride = (uint64_t)(l + sizeP_) * c0.GetParams()->GetRingDimension();
    tr.present = plan.present.empty() ? nullptr : plan.present.data();
    auto o = DCRTPolyHip::result_pair(c0.GetParams(), Format::EVALUATION, c0.Batch());
    check(ofhe_hip_ks_bsgs_transform(h_.get(), (uint32_t)l, &tr, c0.data(), c1.data(), o.first.data(), o.second.data(),
                                     t, c0.Batch(), nullptr),
          "LinearTransform");
    return o;
}

// The tables of one level l of HPSPOVERQLEVELED as the reference's getters
// return them (CryptoParametersBFVRNS, bfvrns-cryptoparameters.cpp:156-188,
// 352-364, 501-523, 558-631), matrices flattened row-major.  l is the index of
// the last kept tower.
struct BfvLevelTables {
    uint32_t l = 0;
    std::vector<uint64_t> QlHatInvModq, QlHatModr;        // [l+1], [l+1][l+1]      GetQlHatInvModq(l), GetQlHatModr(l) as [i][j]
    std::vector<uint64_t> RlHatInvModr, RlHatModq;        // [l+1], [l+1][l+1]      GetRlHatInvModr(l), GetRlHatModq(l) as [j][i]
    std::vector<uint64_t> negRlQHatInvModq, qInvModr;     // [sizeQ], [sizeQ][l+1]  GetmNegRlQHatInvModq(l), GetqInvModr() cut to l+1 columns
    std::vector<std::vector<uint64_t>> QlQHatInvModqDivqModq;    // [l+1][sizeQ-l]  GetQlQHatInvModqDivqModq(l)
    std::vector<double> QlQHatInvModqDivqFrac;                   // [sizeQ-l-1]     GetQlQHatInvModqDivqFrac(l)
    std::vector<std::vector<uint64_t>> tQlSlHatInvModsDivsModq;  // [l+1][l+2]      GettQlSlHatInvModsDivsModq(l)
    std::vector<double> tQlSlHatInvModsDivsFrac;                 // [l+1]           GettQlSlHatInvModsDivsFrac(l)
    std::vector<uint64_t> QlHatModq;                             // [l+1]           GetQlHatModq(l)
};

// FindLevelsToDrop (bfvrns-leveledshe.cpp:77-166) with the quantities it reads
// from the crypto parameters as plain arguments, in the reference's order of
// operations (doubles).  The kept level is l = sizeQ - 1 - the result.
struct LevelsToDropParams {
    double sigma = 3.19, assurance = 36;       // GetDistributionParameter, GetAssuranceMeasure
    uint64_t plaintextModulus = 65537;
    uint32_t ringDimension = 0, digitSize = 0;  // digitSize = relinWindow
    bool hybrid = true;                         // GetKeySwitchTechnique() == HYBRID
    uint32_t numPerPartQ = 1, numPartQ = 1, thresholdParties = 1;
    bool gaussianSecret = false, extendedEncryption = false;
    uint32_t sizeQ = 1;
};
inline uint32_t FindLevelsToDrop(uint32_t multiplicativeDepth, const LevelsToDropParams& cp, double dcrtBits,
                                 bool keySwitch = false) {
    const double sigma = cp.sigma, alpha = cp.assurance, p = static_cast<double>(cp.plaintextModulus);
    const uint32_t n = cp.ringDimension, k = cp.numPerPartQ, numPartQ = cp.numPartQ;
    const double Bkey = cp.gaussianSecret ? std::sqrt((double)cp.thresholdParties) * sigma * std::sqrt(alpha)
                                          : (double)cp.thresholdParties;
    const double w = cp.digitSize == 0 ? std::pow(2, dcrtBits) : std::pow(2, (double)cp.digitSize);
    const double Berr = sigma * std::sqrt(alpha);
    auto delta = [](uint32_t nn) -> double { return (2. * std::sqrt((double)nn)); };
    auto Vnorm = [&](uint32_t nn) -> double {
        if (cp.extendedEncryption) return (1. + delta(nn) * Bkey) / 2.;
        return Berr * (1. + 2. * delta(nn) * Bkey);
    };
    auto noiseKS = [&](uint32_t nn, double logqPrev, double ww) -> double {
        if (cp.hybrid) return k * (numPartQ * delta(nn) * Berr + delta(nn) * Bkey + 1.0) / 2;
        return delta(nn) * (std::floor(logqPrev / (std::log(2) * dcrtBits)) + 1) * ww * Berr;
    };
    auto C1 = [&](uint32_t nn) -> double { return delta(nn) * delta(nn) * p * Bkey; };
    auto C2 = [&](uint32_t nn, double logqPrev) -> double {
        return delta(nn) * delta(nn) * Bkey * Bkey / 2.0 + noiseKS(nn, logqPrev, w);
    };
    auto logqBFV = [&](uint32_t nn, double logqPrev) -> double {
        if (multiplicativeDepth > 0)
            return std::log(4 * p) + (multiplicativeDepth - 1) * std::log(C1(nn)) +
                   std::log(C1(nn) * Vnorm(nn) + multiplicativeDepth * C2(nn, logqPrev));
        return std::log(p * (4 * (Vnorm(nn))));
    };
    double logqPrev = 6. * std::log(10);
    double logq = logqBFV(n, logqPrev);
    while (std::fabs(logq - logqPrev) > std::log(1.001)) {
        logqPrev = logq;
        logq = logqBFV(n, logqPrev);
    }
    const double loge = logq / std::log(2) - 2 - std::log2(p);
    const double logExtra = keySwitch ? std::log2(noiseKS(n, logq, w)) : std::log2(delta(n));
    int32_t levels = (int32_t)std::floor((loge - 2 * (double)multiplicativeDepth - 16 - logExtra) / dcrtBits);
    if (levels < 0)
        levels = 0;
    else if (levels > static_cast<int32_t>(cp.sizeQ) - 1)
        levels = (int32_t)cp.sizeQ - 1;
    return (uint32_t)levels;
}

// One level of HPSPOVERQLEVELED: LeveledSHEBFVRNS::EvalMult / EvalSquare
// (bfvrns-leveledshe.cpp:235-274, 316-330, 367-382, 459-499) and RelinearizeCore
// (845-899) at the level l of the tables, for ciphertexts over Q with the
// auxiliary basis R (as many towers as Q).  The caller chooses l
// (FindLevelsToDrop) and asks BfvLevelCache for the level.
class BfvLevel {
public:
    BfvLevel(std::shared_ptr<DCRTParams> Q, const std::shared_ptr<DCRTParams>& R, const BfvLevelTables& T)
        : Q_(std::move(Q)), l_(T.l) {
        const size_t sizeQ = Q_->Towers(), L = (size_t)T.l + 1;
        if (L > sizeQ || R->Towers() < L) throw math_error("BfvLevel: l must be in [0, sizeQ - 1] and R hold l + 1 towers");
        Ql_ = Q_->Slice(0, L);
        Rl_ = R->Slice(0, L);
        QlRl_ = Ql_->Join(*Rl_);
        if (T.QlHatModq.size() != L) throw math_error("BfvLevel: QlHatModq must have l + 1 entries");
        ql_to_rl_.reset(new BaseConverter(*Ql_, *Rl_, T.QlHatInvModq, T.QlHatModr));
        rl_to_ql_.reset(new BaseConverter(*Rl_, *Ql_, T.RlHatInvModr, T.RlHatModq));
        neg_.reset(new BaseConverter(*Q_, *Rl_, T.negRlQHatInvModq, T.qInvModr));
        if (L < sizeQ)
            drop_.reset(new ScaleAndRound(*Ql_, *Q_->Slice(L, sizeQ - L), true, T.QlQHatInvModqDivqModq,
                                          T.QlQHatInvModqDivqFrac));
        sr_.reset(new ScaleAndRound(*Ql_, *Rl_, true, T.tQlSlHatInvModsDivsModq, T.tQlSlHatInvModsDivsFrac));
        ofhe_bfv_level_t h = nullptr;
        check(ofhe_hip_bfv_level_create(Q_->manager()->ctx(), T.l, Q_->plan(), Ql_->plan(), Rl_->plan(), QlRl_->plan(),
                                        ql_to_rl_->handle(), rl_to_ql_->handle(), neg_->handle(),
                                        drop_ ? drop_->handle() : nullptr, sr_->handle(), T.QlHatModq.data(), &h),
              "BfvLevel");
        h_.reset(h);
    }

    // {cvMult[0], cvMult[1], cvMult[2]} over Q in COEFFICIENT form, as the reference leaves them
    std::vector<DCRTPolyHip> EvalMult(const DCRTPolyHip& c0, const DCRTPolyHip& c1, const DCRTPolyHip& d0,
                                      const DCRTPolyHip& d1) const {
        auto out = bfv_mult_outputs("BfvLevel::EvalMult", Q_, c0, c1, d0, d1);
        check(ofhe_hip_bfv_eval_mult_leveled(h_.get(), c0.data(), c1.data(), d0.data(), d1.data(), out[0].data(),
                                             out[1].data(), out[2].data(), c0.Batch(), nullptr),
              "BfvLevel::EvalMult");
        return out;
    }
    // EvalSquare (bfvrns-leveledshe.cpp:459-499): the values of EvalMult(c, c)
    std::vector<DCRTPolyHip> EvalSquare(const DCRTPolyHip& c0, const DCRTPolyHip& c1) const {
        return EvalMult(c0, c1, c0, c1);
    }
    // RelinearizeCore (bfvrns-leveledshe.cpp:845-899) of cv (3 or 2 elements over
    // Q, all in one format) with the evaluation key (key_b, key_a): {cv[0], cv[1]}
    // over Q in EVALUATION form.  ks is the HYBRID engine of Q (KsCache).
    std::pair<DCRTPolyHip, DCRTPolyHip> Relinearize(const std::vector<const DCRTPolyHip*>& cv, const DCRTPolyHip& key_b,
                                                    const DCRTPolyHip& key_a, const ofhe_ks_t ks) const {
        if (cv.size() != 2 && cv.size() != 3) throw math_error("BfvLevel::Relinearize: 2 or 3 elements expected");
        for (const DCRTPolyHip* v : cv)
            if (!v || v->GetFormat() != cv[0]->GetFormat() || v->GetParams()->Moduli() != Q_->Moduli() ||
                v->Batch() != cv[0]->Batch())
                throw math_error("BfvLevel::Relinearize: elements over Q in one format and of one batch expected");
        auto o = DCRTPolyHip::result_pair(Q_, Format::EVALUATION, cv[0]->Batch());
        check(ofhe_hip_bfv_relinearize_leveled(h_.get(), ks, (uint32_t)cv.size(),
                                               cv[0]->GetFormat() == Format::EVALUATION, cv[0]->data(), cv[1]->data(),
                                               cv.size() == 3 ? cv[2]->data() : nullptr, key_b.data(), key_a.data(),
                                               o.first.data(), o.second.data(), cv[0]->Batch(), nullptr),
              "BfvLevel::Relinearize");
        return o;
    }
    // ScaleAndRound to Q_l and ExpandCRTBasisQlHat in one launch: x over Q_l R_l
    // (COEFFICIENT) -> Q
    DCRTPolyHip ScaleAndRoundExpand(const DCRTPolyHip& x) const {
        if (x.GetFormat() != Format::COEFFICIENT || x.GetParams()->Moduli() != QlRl_->Moduli())
            throw math_error("BfvLevel::ScaleAndRoundExpand: a COEFFICIENT-form polynomial over Ql|Rl expected");
        DCRTPolyHip out = DCRTPolyHip::result(Q_, Format::COEFFICIENT, x.Batch());
        check(ofhe_hip_scale_round_expand_ql_hat(h_.get(), x.data(), out.data(), x.Batch(), nullptr),
              "BfvLevel::ScaleAndRoundExpand");
        return out;
    }
    uint32_t Level() const { return l_; }
    const std::shared_ptr<DCRTParams>& ParamsQ() const { return Q_; }
    const std::shared_ptr<DCRTParams>& ParamsQl() const { return Ql_; }
    const std::shared_ptr<DCRTParams>& ParamsRl() const { return Rl_; }
    const std::shared_ptr<DCRTParams>& ParamsQlRl() const { return QlRl_; }
    const BaseConverter& QlToRl() const { return *ql_to_rl_; }
    const BaseConverter& RlToQl() const { return *rl_to_ql_; }
    const BaseConverter& QToRlNeg() const { return *neg_; }
    const ScaleAndRound* Drop() const { return drop_.get(); }  // null at l = sizeQ - 1
    const ScaleAndRound& Scale() const { return *sr_; }
    ofhe_bfv_level_t handle() const { return h_.get(); }

private:
    std::shared_ptr<DCRTParams> Q_, Ql_, Rl_, QlRl_;
    uint32_t l_;
    std::unique_ptr<BaseConverter> ql_to_rl_, rl_to_ql_, neg_;
    std::unique_ptr<ScaleAndRound> drop_, sr_;
    Handle<ofhe_bfv_level_s, ofhe_hip_bfv_level_destroy> h_;
};

inline void DCRTPolyHip::ExpandCRTBasisQlHat(const BfvLevel& level) {
    check_over(*this, *level.ParamsQl(), "ExpandCRTBasisQlHat", ": the polynomial is not over the level's Q_l");
    DCRTPolyHip r = result(level.ParamsQ(), f_, batch_);
    check(ofhe_hip_expand_ql_hat(level.handle(), data(), nullptr, r.data(), batch_, nullptr), "ExpandCRTBasisQlHat");
    *this = std::move(r);
}

// BfvLevelCache: one BfvLevel per (device, N, Q, R, t-dependent tables' owner,
// l) -- the reference precomputes every level's tables once per
// CryptoParametersBFVRNS; `tables(l)` is called only on a miss.  owner
// distinguishes parameter sets that share Q and R but not t.
class BfvLevelCache {
public:
    template <class F>
    static std::shared_ptr<BfvLevel> get(const std::shared_ptr<DCRTParams>& Q, const std::shared_ptr<DCRTParams>& R,
                                         uint64_t owner, uint32_t l, F&& tables) {
        std::vector<uint64_t> key{(uint64_t)Q->manager()->device(), Q->LogN(), owner, l, Q->Towers()};
        key.insert(key.end(), Q->Moduli().begin(), Q->Moduli().end());
        key.insert(key.end(), R->Moduli().begin(), R->Moduli().end());
        return Cache<std::vector<uint64_t>, BfvLevel>::get(key,
                                                           [&] { return std::make_shared<BfvLevel>(Q, R, tables(l)); });
    }
};

}  // namespace ofhe
