// Host-side runtime of libeeg2video_hip: error plumbing, the stream-ordered workspace cache and the
// weight store keyed by the reference's state-dict names.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/eeg2video_hip.h"
#include "prof.h"

namespace e2v {

struct Error : std::runtime_error {
    e2v_status code;
    Error(e2v_status c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define E2V_HIP(expr)                                                                                   \
    do {                                                                                                \
        if (::e2v::dry_run()) break;                                                                    \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            throw ::e2v::Error(E2V_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e));            \
    } while (0)

#define E2V_REQUIRE(cond, code, msg)                         \
    do {                                                     \
        if (!(cond)) throw ::e2v::Error((code), (msg));      \
    } while (0)

// ---- E2V_POOL_GUARD: a debug facility for the bounds tests -----------------------------------------------------
// While the switch is N > 0, every block the library hands to its own kernels -- pool blocks, dev_alloc blocks, the GroupNorm
// workspaces -- lies inside a larger hipMalloc block: N KiB of guard zone, the payload, and a second guard zone that starts at the
// payload's exact last byte.  Guards AND payload are filled with 0x7FC07FC0 (a NaN as fp32 and, per 16-bit half, as bf16 and as IEEE
// half) before the block is handed out, so a kernel that stores outside its tensor changes a guard, and one whose result depends on
// memory it never wrote produces NaNs.  The zones are compared with the pattern by a small kernel queued on the context's stream
// (misc.hip: one workgroup per zone pair, plain loads, one thread writes the result slot); e2v_op_pool_guard_report collects.
// Each queued comparison keeps a result slot (8 bytes on the device, a record on the host) until the next report: a guarded run that
// never reports grows by 128 KiB of device memory per 16384 released blocks.
constexpr uint32_t kGuardPattern = 0x7FC07FC0u;
int pool_guard_kib();                                        // the switch, read live (bgemm.hip: the knob table)
// queue the comparison of [lead, lead + guard) and [trail, trail + guard) with the pattern, in 16-bit units: slot[0] / slot[1] receive the
// index of the first altered unit of each zone, or 0xFFFFFFFF (misc.hip)
void pool_guard_check(const void* lead, const void* trail, size_t guard_bytes, uint32_t* slot, hipStream_t s);

struct GuardBlock {                                          // one guarded allocation: [base | guard | payload ... | guard | slack]
    void* base = nullptr;
    size_t total = 0, guard = 0, payload = 0;
    char* lead() const { return static_cast<char*>(base); }
    char* data() const { return static_cast<char*>(base) + guard; }
    char* trail() const { return data() + payload; }
};

// The tally of one context: result slots on the device (one pair per queued comparison), what each pair belongs to on the host.
class GuardTally {
public:
    ~GuardTally() { for (uint32_t* c : chunks_) (void)hipFree(c); }
    // queue the comparison of b's two zones on s
    void check(const GuardBlock& b, const char* kind, hipStream_t s) {
        if (used_ == chunks_.size() * kSlots) {
            uint32_t* c = nullptr;
            if (hipMalloc((void**)&c, kSlots * 2 * sizeof(uint32_t)) != hipSuccess) throw Error(E2V_EHIP, "hipMalloc guard tally");
            chunks_.push_back(c);
        }
        uint32_t* slot = chunks_[used_ / kSlots] + 2 * (used_ % kSlots);
        pool_guard_check(b.lead(), b.trail(), b.guard, slot, s);       // (throws when the launch is refused: the slot stays free)
        pending_.push_back({kind, b.payload});
        ++used_;
    }
    // after the stream has been synchronised: fold the queued comparisons into the totals
    void collect() {
        std::vector<uint32_t> host(2 * kSlots);
        for (size_t i = 0; i < used_; i += kSlots) {
            const size_t n = std::min(kSlots, used_ - i);
            if (hipMemcpy(host.data(), chunks_[i / kSlots], n * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
                throw Error(E2V_EHIP, "hipMemcpy guard tally");
            for (size_t k = 0; k < n; ++k)
                for (int side = 0; side < 2; ++side)
                    if (host[2 * k + side] != 0xFFFFFFFFu) {
                        ++violations_;
                        text_ += std::string(pending_[i + k].kind) + " block, payload " + std::to_string(pending_[i + k].payload) + " bytes: " +
                                 (side ? "trailing" : "leading") + " guard altered, first at byte offset " +
                                 std::to_string((size_t)host[2 * k + side] * 2 / 4 * 4) + " of the zone\n";
                    }
        }
        checked_ += (int64_t)used_;
        used_ = 0;
        pending_.clear();
    }
    // totals since the previous call
    void take(int64_t& checked, int64_t& violations, std::string& text) {
        checked = checked_; violations = violations_; text.swap(text_);
        checked_ = violations_ = 0; text_.clear();
    }

private:
    static constexpr size_t kSlots = 16384;
    struct Pending { const char* kind; size_t payload; };
    std::vector<uint32_t*> chunks_;
    std::vector<Pending> pending_;
    size_t used_ = 0;
    int64_t checked_ = 0, violations_ = 0;
    std::string text_;
};

// a guarded block around `bytes` of payload, all of it poisoned on stream s (null: synchronously).  The caller keeps base for hipFree.
inline GuardBlock guard_alloc(size_t bytes, size_t guard, hipStream_t s, bool sync) {
    GuardBlock b;
    b.guard = guard; b.payload = bytes;
    b.total = guard + (bytes + 255) / 256 * 256 + guard;
    hipError_t e = hipMalloc(&b.base, b.total);
    if (e != hipSuccess) throw Error(E2V_EHIP, std::string("hipMalloc guarded block: ") + hipGetErrorString(e));
    e = hipMemsetD32Async((hipDeviceptr_t)b.base, (int)kGuardPattern, b.total / 4, s);
    if (e == hipSuccess && sync) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipFree(b.base); throw Error(E2V_EHIP, std::string("poisoning a guarded block: ") + hipGetErrorString(e)); }
    return b;
}

// Stream-ordered workspace cache.  All work of a ctx runs on one stream at a time, so a buffer handed
// back is immediately reusable by later launches on that stream; blocks are kept by size and reused,
// which makes steady-state calls allocation-free (hipMalloc only while the shape mix is new).
class Pool {
public:
    ~Pool() { trim(); }
    // the context's current stream and tally, for the guarded mode (E2V_POOL_GUARD)
    void bind(const hipStream_t* stream, GuardTally* tally) { stream_ = stream; tally_ = tally; }
    // e2v_destroy: blocks released from here on are not compared any more (the caller's stream may be gone, nobody reads the tally)
    void closing() { closing_ = true; }
    float* get(size_t floats) { return get_bytes(floats * sizeof(float)); }
    float* get_bytes(size_t exact) {
        size_t bytes = ((exact + 255) / 256) * 256;
        if (bytes == 0) bytes = 256;
        if (dry_run()) return dry_fake_ptr(bytes);           // (put() does not know the address and ignores it)
        ++gets_;
        const int guard_kib = pool_guard_kib();
        if (guard_kib != guard_kib_) {                       // the switch flipped: no block of the other kind is recycled into this run
            trim();
            guard_kib_ = guard_kib;
        }
        if (guard_kib > 0) return get_guarded(exact, (size_t)guard_kib * 1024);
        auto it = free_.lower_bound(bytes);
        if (it != free_.end() && it->first <= bytes + bytes / 4) {
            void* p = it->second;
            size_t sz = it->first;
            free_.erase(it);
            live_[p] = sz;
            return static_cast<float*>(p);
        }
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            trim();
            e = hipMalloc(&p, bytes);
        }
        if (e != hipSuccess) throw Error(E2V_EHIP, std::string("hipMalloc workspace: ") + hipGetErrorString(e));
        total_ += bytes;
        live_[p] = bytes;
        return static_cast<float*>(p);
    }
    void put(float* p) {
        if (!p) return;
        auto it = live_.find(p);
        if (it == live_.end()) {
            if (!guarded_.empty()) put_guarded(p);
            return;
        }
        free_.emplace(it->second, p);
        live_.erase(it);
    }
    void trim() {
        for (auto& kv : free_) {
            (void)hipFree(kv.second);
            total_ -= kv.first;
        }
        free_.clear();
        for (auto& kv : gfree_) {                            // (hipFree waits for the comparisons queued on these blocks)
            (void)hipFree(kv.second.base);
            total_ -= kv.first;
        }
        gfree_.clear();
    }
    size_t bytes() const { return total_; }
    int64_t gets() const { return gets_; }                   // blocks handed out so far (e2v_op_pool_gets: what a guarded run must have checked)
    // e2v_op_pool_guard_report: queue the comparison of the guarded blocks that are still live
    void check_live(hipStream_t s) {
        for (auto& kv : guarded_) tally_->check(kv.second, "pool (live)", s);
    }

private:
    float* get_guarded(size_t exact, size_t guard) {
        const hipStream_t s = stream_ ? *stream_ : nullptr;
        const size_t need = guard + (exact + 255) / 256 * 256 + guard;
        GuardBlock b;
        auto it = gfree_.lower_bound(need);
        if (it != gfree_.end() && it->first <= need + need / 4 && it->second.guard == guard) {
            b = it->second;
            gfree_.erase(it);
            b.payload = exact;
            hipError_t e = hipMemsetD32Async((hipDeviceptr_t)b.base, (int)kGuardPattern, b.total / 4, s);
            if (e != hipSuccess) throw Error(E2V_EHIP, std::string("poisoning a guarded block: ") + hipGetErrorString(e));
        } else {
            b = guard_alloc(exact, guard, s, false);
            total_ += b.total;
        }
        guarded_[b.data()] = b;
        return reinterpret_cast<float*>(b.data());
    }
    void put_guarded(float* p) {
        auto it = guarded_.find(p);
        if (it == guarded_.end()) return;
        const GuardBlock b = it->second;
        guarded_.erase(it);
        gfree_.emplace(b.total, b);                          // (filed first: a throw below must not leak it)
        if (closing_) return;
        try {
            tally_->check(b, "pool", stream_ ? *stream_ : nullptr);
        } catch (const Error&) {                             // (put runs in destructors; a block that could not be checked is not counted)
        }
    }
    std::multimap<size_t, void*> free_;
    std::unordered_map<void*, size_t> live_;
    std::multimap<size_t, GuardBlock> gfree_;                // guarded blocks by total size
    std::unordered_map<void*, GuardBlock> guarded_;          // live guarded blocks by payload address
    const hipStream_t* stream_ = nullptr;
    GuardTally* tally_ = nullptr;
    int guard_kib_ = 0;
    bool closing_ = false;
    int64_t gets_ = 0;
    size_t total_ = 0;
};

// channel-last activation [rows][C] living in the pool; fp32, or bf16 (bf16-activation mode: `p` then points at 2-byte elements)
struct Act {
    float* p = nullptr;
    int64_t rows = 0;
    int C = 0;
    Pool* pool = nullptr;
    bool bf16 = false;
    float* rb = nullptr;           // row-block sums that came with the tensor (IgemmArgs::rbsum: [rows / 64][C][2]), pool-owned; null: none
    Act() = default;
    Act(Pool& pl, int64_t r, int c, bool half = false)
        : p(pl.get_bytes((size_t)r * c * (half ? 2 : 4))), rows(r), C(c), pool(&pl), bf16(half) {}      // (the exact size: a guard zone starts at the tensor's last byte)
    size_t bytes() const { return (size_t)rows * C * (bf16 ? 2 : 4); }
    const float* at(int64_t elem) const {          // address of element `elem` (counted in elements of the storage type)
        return reinterpret_cast<const float*>(reinterpret_cast<const char*>(p) + (size_t)elem * (bf16 ? 2 : 4));
    }
    Act(const Act&) = delete;
    Act& operator=(const Act&) = delete;
    Act(Act&& o) noexcept { *this = std::move(o); }
    Act& operator=(Act&& o) noexcept {
        if (this != &o) {
            reset();
            p = o.p; rows = o.rows; C = o.C; pool = o.pool; bf16 = o.bf16; rb = o.rb;
            o.p = nullptr; o.pool = nullptr; o.rb = nullptr;
        }
        return *this;
    }
    ~Act() { reset(); }
    void reset() {
        if (p && pool) pool->put(p);
        if (rb && pool) pool->put(rb);
        p = nullptr; rb = nullptr;
    }
};

struct WTensor {
    float* d = nullptr;             // device, torch layout, fp32
    std::vector<int64_t> shape;
    size_t numel = 0;
    bool loaded = false;
};

}  // namespace e2v
