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

// ---- device memory: one owning block type ------------------------------------------------------------------------------------------
// Every block the library allocates for itself -- workspace-pool blocks, weight layouts (dev_alloc), the GroupNorm workspaces, the
// timestep buffer, uploaded tensors, temporaries -- is a DevBlock: [guard | payload | pad to 256 | guard] inside one hipMalloc block,
// owned by exactly one DevBlock object (move-only; the destructor frees).  guard == 0 is the payload alone, the normal case.
//
// E2V_POOL_GUARD, a debug facility for the bounds tests: while the switch is N > 0, the blocks handed to the
// library's own kernels -- pool blocks, dev_alloc blocks, the GroupNorm workspaces -- are allocated with guard = N KiB; the second
// guard zone starts at the payload's exact last byte.  Guards AND payload are filled with 0x7FC07FC0 (a NaN as fp32 and, per 16-bit
// half, as bf16 and as IEEE half) before the block is handed out, so a kernel that stores outside its tensor changes a guard, and one
// whose result depends on memory it never wrote produces NaNs.  The zones are compared with the pattern by a small kernel queued on
// the context's stream (misc.hip: one workgroup per zone pair, plain loads, one thread writes the result slot);
// e2v_op_pool_guard_report collects.  Each queued comparison keeps a result slot (8 bytes on the device, a record on the host) until
// the next report: a guarded run that never reports grows by 128 KiB of device memory per 16384 released blocks.
constexpr uint32_t kGuardPattern = 0x7FC07FC0u;
int pool_guard_kib();                                        // the switch, read live (bgemm.hip: the knob table)
// queue the comparison of [lead, lead + guard) and [trail, trail + guard) with the pattern, in 16-bit units: slot[0] / slot[1] receive the
// index of the first altered unit of each zone, or 0xFFFFFFFF (misc.hip)
void pool_guard_check(const void* lead, const void* trail, size_t guard_bytes, uint32_t* slot, hipStream_t s);

struct DevBlock {
    void* base = nullptr;
    size_t total = 0, guard = 0, payload = 0;                // total == 0 with a base: the address a dry run handed out, nothing owned
    DevBlock() = default;
    DevBlock(const DevBlock&) = delete;
    DevBlock& operator=(const DevBlock&) = delete;
    DevBlock(DevBlock&& o) noexcept { *this = std::move(o); }
    DevBlock& operator=(DevBlock&& o) noexcept {
        if (this != &o) {
            release();
            base = o.base; total = o.total; guard = o.guard; payload = o.payload;
            o.base = nullptr; o.total = o.guard = o.payload = 0;
        }
        return *this;
    }
    ~DevBlock() { release(); }
    void release() {
        if (total) (void)hipFree(base);
        base = nullptr; total = guard = payload = 0;
    }
    explicit operator bool() const { return base != nullptr; }
    char* lead() const { return static_cast<char*>(base); }
    char* data() const { return static_cast<char*>(base) + guard; }
    char* trail() const { return data() + payload; }
    float* f32() const { return reinterpret_cast<float*>(data()); }
};

// fill guards and payload of a guarded block with the pattern on stream s
inline void dev_block_poison(const DevBlock& b, hipStream_t s, bool sync) {
    hipError_t e = hipMemsetD32Async((hipDeviceptr_t)b.base, (int)kGuardPattern, b.total / 4, s);
    if (e == hipSuccess && sync) e = hipStreamSynchronize(s);
    if (e != hipSuccess) throw Error(E2V_EHIP, std::string("poisoning a guarded block: ") + hipGetErrorString(e));
}

// THE allocation: `bytes` of payload, between two zones of `guard` bytes when guard > 0 and then poisoned on stream s (sync: and waited
// for).  A dry run (e2v_op_describe_dispatch) gets a distinct address nobody dereferences and owns nothing.
inline DevBlock dev_block(size_t bytes, size_t guard, hipStream_t s, bool sync) {
    DevBlock b;
    b.payload = bytes;
    if (dry_run()) { b.base = dry_fake_ptr(bytes); return b; }
    const size_t total = guard ? guard + (bytes + 255) / 256 * 256 + guard : bytes;
    const hipError_t e = hipMalloc(&b.base, total);
    if (e != hipSuccess) { b.base = nullptr; throw Error(E2V_EHIP, std::string("hipMalloc device block: ") + hipGetErrorString(e)); }
    b.total = total; b.guard = guard;
    if (guard) dev_block_poison(b, s, sync);
    return b;
}

// A grow-only buffer (the GroupNorm workspaces, the timestep buffer).  Work queued on s may still read the block it replaces, so
// growing waits for the stream first.
struct GrowBuf {
    DevBlock blk;
    void* ensure(size_t bytes, size_t guard, hipStream_t s) {
        if (!blk || blk.payload < bytes) {
            E2V_HIP(hipStreamSynchronize(s));
            blk.release();
            blk = dev_block(bytes, guard, s, true);
        }
        return blk.data();
    }
};

// The tally of one context: result slots on the device (one pair per queued comparison), what each pair belongs to on the host.
class GuardTally {
public:
    ~GuardTally() { for (uint32_t* c : chunks_) (void)hipFree(c); }
    // queue the comparison of b's two zones on s
    void check(const DevBlock& b, const char* kind, hipStream_t s) {
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

// Stream-ordered workspace cache.  All work of a ctx runs on one stream at a time, so a buffer handed
// back is immediately reusable by later launches on that stream; blocks are kept by size and reused,
// which makes steady-state calls allocation-free (hipMalloc only while the shape mix is new).
class Pool {
public:
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
        // unguarded: the payload is the 256-rounded size; guarded: the exact one (a guard zone starts at the tensor's last byte).  Blocks
        // are filed by their total size: reuse takes the smallest one of at least this size and at most a quarter larger.
        const size_t guard = (size_t)guard_kib * 1024;
        const size_t payload = guard ? exact : bytes;
        const size_t need = guard ? guard + (exact + 255) / 256 * 256 + guard : bytes;
        const hipStream_t s = stream_ ? *stream_ : nullptr;
        DevBlock b;
        auto it = free_.lower_bound(need);
        while (it != free_.end() && it->first <= need + need / 4 && it->second.guard != guard) ++it;    // (a block of the other kind, released after the flip)
        if (it != free_.end() && it->first <= need + need / 4) {
            b = std::move(it->second);
            free_.erase(it);
            if (guard) {
                b.payload = exact;
                try {
                    dev_block_poison(b, s, false);
                } catch (const Error&) {                     // (b is freed on the way out)
                    total_ -= b.total;
                    throw;
                }
            }
        } else {
            try {
                b = dev_block(payload, guard, s, false);
            } catch (const Error&) {                         // out of memory: give the cached blocks back and try once more
                trim();
                b = dev_block(payload, guard, s, false);
            }
            total_ += b.total;
        }
        float* p = b.f32();
        live_.emplace(p, std::move(b));
        return p;
    }
    void put(float* p) {
        if (!p) return;
        auto it = live_.find(p);
        if (it == live_.end()) return;
        const auto filed = free_.emplace(it->second.total, std::move(it->second));      // (filed first: a throw below must not leak it)
        live_.erase(it);
        if (filed->second.guard == 0 || closing_) return;
        try {
            tally_->check(filed->second, "pool", stream_ ? *stream_ : nullptr);
        } catch (const Error&) {                             // (put runs in destructors; a block that could not be checked is not counted)
        }
    }
    void trim() {                                            // (hipFree waits for the comparisons queued on these blocks)
        for (auto& kv : free_) total_ -= kv.first;
        free_.clear();
    }
    size_t bytes() const { return total_; }
    int64_t gets() const { return gets_; }                   // blocks handed out so far (e2v_op_pool_gets: what a guarded run must have checked)
    // e2v_op_pool_guard_report: queue the comparison of the guarded blocks that are still live
    void check_live(hipStream_t s) {
        for (auto& kv : live_)
            if (kv.second.guard) tally_->check(kv.second, "pool (live)", s);
    }

private:
    std::multimap<size_t, DevBlock> free_;                   // by total size
    std::unordered_map<void*, DevBlock> live_;               // by payload address
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
    DevBlock mem;                   // device, torch layout, fp32 (unguarded: DESIGN section 5)
    float* d() const { return mem.f32(); }
    std::vector<int64_t> shape;
    size_t numel = 0;
    bool loaded = false;
};

}  // namespace e2v
