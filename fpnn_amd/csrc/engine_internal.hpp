// engine_internal.hpp -- what the engine's host translation units (engine.hip,
// host_frames.hip) share: the engine and key-set objects behind the C-ABI handles, error
// reporting, scratch growth and the host-frame pipelines' slots and copy pool.  Host code
// only; no k_*.hip includes it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/fpnn_aes.h"
#include "hostcopy.hpp"
#include "numa_place.hpp"
#include "aes_common.hpp"
#include "kernels.hpp"
#include "scratch_plan.hpp"

namespace fpnn_aes {

inline thread_local std::string g_last_error;  // fpnn_aes_last_error

// FPNN_AES_DEBUG_FAIL_CALL=N (tests only): the N-th host-data call of the process (cfb_host,
// package_host, stream_host, stream_recv -- the calls the C++ classes make) returns
// FPNN_AES_ERR_DEVICE as a failed device would, so the drop-in's failure contract can be
// driven through FPNN's own IO code (fail_policy.hpp, tests/test_gpu_dropin.py).
inline int debug_fail_point() {
    static const long long at = [] {
        const char *v = getenv("FPNN_AES_DEBUG_FAIL_CALL");
        return v ? atoll(v) : 0ll;
    }();
    if (at <= 0) return 0;
    static std::atomic<long long> calls{0};
    if (calls.fetch_add(1, std::memory_order_relaxed) + 1 != at) return 0;
    g_last_error = "injected device error (FPNN_AES_DEBUG_FAIL_CALL)";
    return FPNN_AES_ERR_DEVICE;
}

inline int hip_fail(hipError_t err, const char *what) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s (%d)", what, hipGetErrorString(err), (int)err);
    g_last_error = buf;
    return FPNN_AES_ERR_HIP;
}

#define HIP_TRY(expr)                                                 \
    do {                                                              \
        hipError_t _e = (expr);                                       \
        if (_e != hipSuccess) return fpnn_aes::hip_fail(_e, #expr);   \
    } while (0)

struct EventPair {
    hipEvent_t beg, end;
};

// memcpy job of the host-frame gather/scatter
struct CopyJob {
    uint8_t *dst;
    const uint8_t *src;
    uint64_t n;
};

// Pinned host memory on `node` (the engine's NUMA placement; < 0: the runtime's default).
// hipHostMallocNumaUser makes the allocation follow the calling thread's memory policy,
// which NumaPreferScope points at the node for the call.
inline hipError_t pinned_host_alloc(int node, void **p, size_t n) {
    NumaPreferScope prefer(node);
    return hipHostMalloc(p, n, prefer.active() ? hipHostMallocNumaUser : 0u);
}

// One slot of the host-frame pipeline (fpnn_aes_package_host / fpnn_aes_stream_host):
// pinned + device staging and its own stream, so the copies of one chunk overlap the
// kernel of the other.
struct HostSlot {
    uint8_t *h = nullptr, *d = nullptr;
    uint64_t cap = 0;
    hipStream_t st = nullptr;
    hipEvent_t done = nullptr;    // chunk's D2H finished
    hipEvent_t staged = nullptr;  // chunk's H2D finished (the engine stream may cipher it)
    hipEvent_t kdone = nullptr;   // chunk's kernel finished (the slot stream may copy it back)
    bool busy = false;
    std::vector<CopyJob> scatter;  // staged output -> callers' buffers, run after `done`
    uint64_t scatter_bytes = 0;
    // package chunks scatter whole frames [first, first + count) straight from the staged
    // out_off array instead (no per-frame job list)
    const fpnn_aes_host_frame *frames = nullptr;
    uint32_t first = 0, count = 0;
    uint64_t pre = 0, out_at = 0;
    const uint64_t *out_off = nullptr;  // pinned, inside h
};

// One slot of the host-mapped frame pipeline (frames in memory registered with
// fpnn_aes_host_register): device staging for one chunk (input | output | descriptors),
// the pinned descriptor block the host fills, and the events that hand the chunk from
// the move stream to the engine stream and back.
struct MapSlot {
    uint8_t *d = nullptr;  // device: in | out | desc
    uint64_t dcap = 0;
    uint8_t *h = nullptr;  // pinned: desc
    uint64_t hcap = 0;
    hipEvent_t gathered = nullptr;  // chunk staged in HBM (the engine stream may cipher it)
    hipEvent_t ciphered = nullptr;  // cipher done (the move stream may scatter)
    hipEvent_t done = nullptr;      // the slot's descriptors went H2D (its pinned block is free)
    bool busy = false;
};

// Persistent host workers for the host-frame path.  Gathering 1M separate 1 KiB frames
// into pinned staging (and scattering the results back) is the host-memory-bound part
// of fpnn_aes_package_host; threads are kept across calls so a chunk does not pay
// thread start-up.  run(k, fn) calls fn(0..k-1) across the caller and k-1 workers.
class HostPool {
public:
    // workers run on the engine's NUMA placement (numa_place.hpp: the GPU's node's CPUs)
    HostPool(unsigned workers, const NumaPlacement &pl) : pl_(pl) {
        for (unsigned t = 0; t < workers; t++) th_.emplace_back([this, t] { loop(t + 1); });
    }
    ~HostPool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    // parts a host-frame call splits its copies into: this pool's threads + the caller,
    // shared fairly among the engines whose host-frame calls run at the same moment (every
    // engine has a pool of min(16, cores) threads: several IO threads flushing at once would
    // otherwise oversubscribe the box's CPU share many times over)
    // (per device: the GPU box grants each GPU its own CPU share)
    unsigned parts() const {
        const unsigned all = max_parts();
        const unsigned active = std::max(1u, g_host_active[device_ & 63].load(std::memory_order_relaxed));
        return std::max(1u, all / active);
    }
    unsigned max_parts() const { return (unsigned)th_.size() + 1; }
    void set_device(int d) { device_ = d; }
    static std::atomic<unsigned> g_host_active[64];  // (host_frames.hip)

    template <class F>
    void run(unsigned want, const F &fn) {
        want = std::max(1u, std::min(want, max_parts()));
        if (want == 1) {
            fn(0u);
            return;
        }
        const std::function<void(unsigned)> f(fn);
        {
            std::lock_guard<std::mutex> lk(mu_);
            fn_ = &f;
            active_ = want;
            pending_ = want - 1;
            gen_++;
        }
        cv_.notify_all();
        f(0);
        std::unique_lock<std::mutex> lk(mu_);
        done_cv_.wait(lk, [this] { return pending_ == 0; });
        fn_ = nullptr;
    }

    // memcpy jobs split into contiguous, byte-balanced ranges
    void copy(const std::vector<CopyJob> &jobs, uint64_t total, unsigned want) {
        want = std::max(1u, std::min<unsigned>(want, (unsigned)std::min<size_t>(jobs.size(), max_parts())));
        std::vector<size_t> cut(want + 1, jobs.size());
        cut[0] = 0;
        uint64_t acc = 0;
        unsigned p = 1;
        for (size_t i = 0; i < jobs.size() && p < want; i++) {
            acc += jobs[i].n;
            while (p < want && acc >= total * p / want) cut[p++] = i + 1;
        }
        run(want, [&](unsigned q) {
            for (size_t i = cut[q]; i < cut[q + 1]; i++) copy_streaming(jobs[i].dst, jobs[i].src, jobs[i].n);
            copy_fence();
        });
    }

private:
    void loop(unsigned me) {
        (void)numa_pin_thread(pl_);
        uint64_t seen = 0;
        for (;;) {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
            if (stop_) return;
            seen = gen_;
            if (me >= active_) continue;
            const std::function<void(unsigned)> *f = fn_;
            lk.unlock();
            (*f)(me);
            lk.lock();
            if (--pending_ == 0) done_cv_.notify_one();
        }
    }

    const NumaPlacement pl_;
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_, done_cv_;
    const std::function<void(unsigned)> *fn_ = nullptr;
    unsigned active_ = 0, pending_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
    int device_ = 0;
};

// a host-frame call in progress on a device (HostPool::parts shares the copy threads
// among the calls of that device)
struct HostActive {
    int d;
    explicit HostActive(int device) : d(device & 63) { HostPool::g_host_active[d].fetch_add(1, std::memory_order_relaxed); }
    ~HostActive() { HostPool::g_host_active[d].fetch_sub(1, std::memory_order_relaxed); }
};

// One growing device buffer of the engine: pointer and capacity (elements); kZeroed: the whole
// new capacity is zeroed on the stream when it grows.
template <class T, bool kZeroed>
struct Scratch {
    T *p = nullptr;
    uint64_t cap = 0;
    int ensure(fpnn_aes_engine *e, uint64_t need);
};

}  // namespace fpnn_aes

using fpnn_aes::RaggedPlan;  // (an element type of the scratch list)

struct fpnn_aes_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int num_cus = 256;
    fpnn_aes::Variant variant;
    uint8_t *d_tables = nullptr;  // t0le[256] (1 KiB), sbox[256], td0le[256] (1 KiB), isbox[256]
    // growing scratch, one Scratch per line of scratch_plan.hpp's list: e->bstart.p, e->bstart.cap, ...
#define X(name, type, zeroed) fpnn_aes::Scratch<type, zeroed> name;
    FPNN_AES_SCRATCH_BUFFERS(X)
#undef X
    uint64_t *d_total = nullptr;  // ragged block total (bstart[count]), device only
    // device-side consistency checks (kFault*): a pinned word kernels may set, read when the
    // stream is idle (fpnn_aes_engine_sync, synchronous calls) and reported as FPNN_AES_ERR_DEVICE
    uint32_t *h_fault = nullptr;
    uint32_t *d_fault = nullptr;
    uint8_t *h_sstate = nullptr;  // the pinned twin of sstate
    uint64_t cap_hsstate = 0;
    bool pools = false;            // stream-ordered allocation from `mpool` for the scratch
    hipMemPool_t mpool = nullptr;  // the engine's own memory pool (keeps freed scratch for reuse)
    std::vector<void *> deferred;  // grown-out scratch awaiting an idle stream (no pools)
    // K0 (k_small.hip): pinned staging of the small synchronous calls, its device view,
    // and the sequence number the kernel stores when a call is done
    uint8_t *h_small = nullptr;
    uint8_t *d_small = nullptr;
    uint32_t small_seq = 0;
    // K0s: the resident small-call server's mailbox (pinned), its device view, the last
    // request number and the epoch of the last server launched (0: none yet)
    fpnn_aes::SmallMailbox *h_mb = nullptr;
    fpnn_aes::SmallMailbox *d_mb = nullptr;
    uint32_t mb_seq = 0;
    uint32_t srv_epoch = 0;
    // the last batch work this engine queued while small-call servers exist on the device
    // (a server relaunch on another engine waits for it: batch_fence)
    hipEvent_t batch_ev = nullptr;
    std::atomic<bool> batch_pending{false};  // batch kernels about to be queued (batch_signal)
    std::atomic<bool> batch_ev_live{false};  // batch_ev marks the end of queued batch work
    uint64_t srv_idle_ticks = 0, srv_life_ticks = 0;
    // host staging for fpnn_aes_cfb_host
    uint8_t *h_stage = nullptr;
    uint8_t *d_stage = nullptr;
    uint64_t cap_stage = 0;
    // host-frame pipeline
    fpnn_aes::HostSlot hs[3];  // chunk i on slot i % 3: gather(i) runs beside scatter(i - 2)
    fpnn_aes::MapSlot ms[4];   // host-mapped chunks: gather(t) + scatter(t - 2) || cipher(t - 1), upload(t + 1)
    hipStream_t map_stream = nullptr;  // host-mapped moves (both PCIe directions in one launch)
    const char *host_path = "";  // "host_staged" / "host_mapped": the last host-frame call's path
    std::unique_ptr<fpnn_aes::HostPool> pool;  // created on first use
    fpnn_aes::NumaPlacement numa;    // where the pinned arenas and the pool's threads live
    // the address-audit build (audit.hpp): the extent table kernels check against
    fpnn_aes::AuditTable *d_aud = nullptr;
    // instrumentation
    bool timing = false;
    const char *last_kernel[2] = {"", ""};  // base name of the last main kernel per direction
    std::vector<fpnn_aes::EventPair> ev[2];
    size_t ev_used[2] = {0, 0};
};

struct fpnn_aes_keyset {
    fpnn_aes_engine *e = nullptr;  // creating engine (may be destroyed before the key set)
    int device = 0;
    fpnn_aes::DevKey *d_keys = nullptr;
    uint4 *d_eiv = nullptr;  // E_k(IV) per slot (launch_slot_eiv after every write)
    uint32_t count = 0;
    int nrounds = 0;
    uint32_t keylen = 0;
    // updatable tables (fpnn_aes_keyset_reserve / _set)
    uint32_t capacity = 0;
    fpnn_aes::DevKey *h_up = nullptr;    // pinned upload staging
    uint32_t cap_up = 0;       // DevKeys
    hipEvent_t up_done = nullptr;  // last upload out of h_up
    bool up_pending = false;
};

namespace fpnn_aes {

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// Scratch growth on the call path never frees synchronously: hipFree waits for the whole
// device, so one thread's first large call would stall every other engine's queued work.
// With stream-ordered pools the old buffer is released by hipFreeAsync behind the work
// already queued on this engine's stream; without them it is kept until the stream is
// next idle (engine_sync, the end of a synchronous host call, engine_destroy).
template <class T, bool kZeroed>
int Scratch<T, kZeroed>::ensure(fpnn_aes_engine *e, uint64_t need) {
    if (need <= cap) return FPNN_AES_OK;
    const uint64_t n = scratch_next_cap(cap, need);
    T *np = nullptr;
    if (e->pools) HIP_TRY(hipMallocFromPoolAsync(reinterpret_cast<void **>(&np), n * sizeof(T), e->mpool, e->stream));
    else HIP_TRY(hipMalloc(reinterpret_cast<void **>(&np), n * sizeof(T)));
    if (p) {
        if (e->pools) HIP_TRY(hipFreeAsync(p, e->stream));
        else e->deferred.push_back(p);
    }
    p = np;
    cap = n;
    if (kZeroed) HIP_TRY(hipMemsetAsync(p, 0, cap * sizeof(T), e->stream));
    return FPNN_AES_OK;
}

// every buffer to at least what `need` asks of it (scratch_plan.hpp: the need_* functions)
inline int scratch_ensure(fpnn_aes_engine *e, const ScratchNeed &need) {
    int rc = FPNN_AES_OK;
#define X(name, type, zeroed) if (rc == FPNN_AES_OK) rc = e->name.ensure(e, need.n[SC_##name]);
    FPNN_AES_SCRATCH_BUFFERS(X)
#undef X
    return rc;
}

// the device and kernel constants the scratch sizes depend on
inline ScratchShape scratch_shape(const fpnn_aes_engine *e) {
    return {(uint64_t)e->num_cus, kThreads / 64, block_map_small_max(), block_map_onepass_words, kLengthOrderWords};
}

// The engine's stream is idle: release grown-out scratch, and report (once) a consistency
// check a kernel failed since the last look (kernels.hpp, kFault*).
int stream_idle(fpnn_aes_engine *e);

// one device batch on the engine's stream: run_encrypt / run_decrypt, the package and
// stream entry points' common part
int run_batch(fpnn_aes_engine *e, bool encrypt, const fpnn_aes_batch *b, uint8_t *iv_state, uint32_t *pos_state,
              bool stream);
// the same for a stream batch of one frame per stream whose keys and (iv, pos) are addressed by
// key-table slot: segment i at slot state_slot[i] of b->keys and of the device state arrays
int run_batch_at(fpnn_aes_engine *e, bool encrypt, const fpnn_aes_batch *b, const uint32_t *state_slot,
                 uint32_t slot_bound, uint8_t *iv_state, uint32_t *pos_state);

}  // namespace fpnn_aes
