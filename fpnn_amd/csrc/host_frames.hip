// host_frames.hip -- many frames from host memory in one call: fpnn_aes_package_host,
// fpnn_aes_stream_host, their _multi forms and the registry of host-mapped memory.  Host
// code only: the bytes are ciphered by engine.hip's device batches (run_encrypt / run_decrypt).
//   staged: chunks gathered into pinned staging by the copy pool, H2D / D2H on slot streams
//   mapped: frames in registered memory, gathered and scattered by the GPU (k_move_segments)
#include <chrono>
#include <unordered_map>

#include "engine_internal.hpp"
#include "stream_plan.hpp"

using namespace fpnn_aes;

std::atomic<unsigned> HostPool::g_host_active[64];

namespace {

// Host threads for gathering/scattering frames: FPNN_AES_HOST_THREADS, default
// min(16, hardware threads) -- the GPU box grants a 16-CPU share per GPU.
unsigned host_threads() {
    unsigned hw = std::thread::hardware_concurrency();
    unsigned n = std::min(16u, hw ? hw : 1u);
    if (const char *v = getenv("FPNN_AES_HOST_THREADS")) n = (unsigned)std::max(1, atoi(v));
    return std::min(n, 64u);  // package chunks keep per-part sums in a 64-entry array
}

HostPool *pool_of(fpnn_aes_engine *e) {
    if (!e->pool) {
        e->pool.reset(new HostPool(host_threads() - 1, e->numa));
        e->pool->set_device(e->device);
    }
    return e->pool.get();
}

// parts for `bytes` of copying: about 1 MiB per thread at least
unsigned copy_parts(fpnn_aes_engine *e, uint64_t bytes) {
    // 1 MiB per copy thread (256 KiB / 64 KiB grains measured within run-to-run spread on
    // the IO-plumbing echo, profiles/r05/io_multi/r05cg_*; the A/B switch was removed in round 6)
    constexpr int grain = 20;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(pool_of(e)->parts(), bytes >> grain));
}

// entries [a, b) of `cnt` that part p of `parts` works on
void part_range(uint32_t cnt, unsigned p, unsigned parts, uint32_t &a, uint32_t &b) {
    a = (uint32_t)((uint64_t)cnt * p / parts);
    b = (uint32_t)((uint64_t)cnt * (p + 1) / parts);
}

// psum[p]: the bytes of fr[0 .. cnt) in front of part p's range; true: all lengths are equal
bool part_sums(fpnn_aes_engine *e, const fpnn_aes_host_frame *fr, uint32_t cnt, unsigned parts, uint64_t (&psum)[65]) {
    uint8_t same[64];
    psum[0] = 0;
    pool_of(e)->run(parts, [&](unsigned p) {
        uint32_t a, b;
        part_range(cnt, p, parts, a, b);
        uint64_t sum = 0;
        bool eq = true;
        for (uint32_t t = a; t < b; t++) {
            sum += fr[t].len;
            eq = eq && fr[t].len == fr[0].len;
        }
        psum[p + 1] = sum;
        same[p] = eq;
    });
    bool uniform = true;
    for (unsigned p = 0; p < parts; p++) {
        psum[p + 1] += psum[p];
        uniform = uniform && same[p];
    }
    return uniform;
}

int slot_reserve(HostSlot &s, int node, uint64_t need) {
    if (!s.st) {
        HIP_TRY(hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&s.staged, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&s.kdone, hipEventDisableTiming));
    }
    if (need <= s.cap) return FPNN_AES_OK;
    uint64_t n = s.cap ? s.cap : (8u << 20);
    while (n < need) n *= 2;
    if (s.h) (void)hipHostFree(s.h);
    if (s.d) (void)hipFree(s.d);
    s.h = nullptr;
    s.d = nullptr;
    s.cap = 0;
    HIP_TRY(pinned_host_alloc(node, reinterpret_cast<void **>(&s.h), n));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.d), n));
    s.cap = n;
    return FPNN_AES_OK;
}

// FPNN_AES_HOST_STATS=1: per-call breakdown of the host-frame pipeline on stderr
struct HostStats {
    bool on = getenv("FPNN_AES_HOST_STATS") != nullptr;
    double gather = 0, scatter = 0, wait = 0;
    double drain_from = 0;  // mapped: when the final drain began
    static double now() {
        return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
    }
};

// part p of `parts` of a package chunk's scatter (whole frames, straight from the staged out_off array)
void scatter_frames_part(const HostSlot &s, unsigned p, unsigned parts) {
    uint32_t a, b;
    part_range(s.count, p, parts, a, b);
    for (uint32_t t = a; t < b; t++) {
        const fpnn_aes_host_frame &f = s.frames[s.first + t];
        copy_streaming(f.dst, s.h + s.out_at + s.out_off[t], f.len + s.pre);
    }
    copy_fence();
}

// wait for a slot's chunk and scatter its outputs to the callers' buffers
int slot_drain(fpnn_aes_engine *e, HostSlot &s, HostStats &st) {
    if (!s.busy) return FPNN_AES_OK;
    s.busy = false;
    const double t0 = st.on ? HostStats::now() : 0;
    HIP_TRY(hipEventSynchronize(s.done));
    const double t1 = st.on ? HostStats::now() : 0;
    if (s.frames) {
        const unsigned parts = copy_parts(e, s.scatter_bytes);
        pool_of(e)->run(parts, [&](unsigned p) { scatter_frames_part(s, p, parts); });
        s.frames = nullptr;
    } else {
        pool_of(e)->copy(s.scatter, s.scatter_bytes, copy_parts(e, s.scatter_bytes));
    }
    if (st.on) {
        st.wait += t1 - t0;
        st.scatter += HostStats::now() - t1;
    }
    return FPNN_AES_OK;
}

// fpnn_aes_stream_host_at: frames[i].key_slot names a slot of the live key table, for the key
// and for the state; iv_state / pos_state are then the DEVICE arrays fpnn_aes_stream_open wrote
// (slot_bound entries), every chunk is ciphered by slot where the state lies (run_batch_at),
// and the compact state block below is not used.
struct HostAt {
    uint32_t slot_bound;
};

// stream-state scratch of the host-frame calls: device (Scratch: no free on the call path)
// and its pinned twin (grown only between calls' uses: the engine stream is drained)
int sstate_reserve(fpnn_aes_engine *e, uint64_t bytes) {
    if (int rc = e->sstate.ensure(e, bytes)) return rc;
    if (bytes > e->cap_hsstate) {
        uint64_t c = e->cap_hsstate ? e->cap_hsstate : 4096;
        while (c < bytes) c *= 2;
        HIP_TRY(hipStreamSynchronize(e->stream));  // a previous call's state copies are done
        if (e->h_sstate) (void)hipHostFree(e->h_sstate);
        e->h_sstate = nullptr;
        e->cap_hsstate = 0;
        HIP_TRY(pinned_host_alloc(e->numa.node, reinterpret_cast<void **>(&e->h_sstate), c));
        e->cap_hsstate = c;
    }
    return FPNN_AES_OK;
}

// ---- staged frames -------------------------------------------------------------------------

// Where a staged chunk's parts lie in its slot, pinned (h) and device (d) staging alike:
//   input | in_off u64 | out_off u64 | len u32 | slot u32 (cnt entries each) | output
struct ChunkLayout {
    uint32_t cnt = 0;
    uint64_t in_pad = 0, out_pad = 0, arr = 0, out_at = 0;
    uint64_t state0 = 0;       // stream: state index of the chunk's first segment
    int64_t uniform = -1;      // stream: every segment takes this many bytes (< 0: they differ)
    void set(uint32_t count, uint64_t in_b, uint64_t out_b) {
        cnt = count, in_pad = (in_b + 15) & ~15ull, out_pad = (out_b + 15) & ~15ull;
        arr = (uint64_t)count * (8 + 8 + 4 + 4), out_at = in_pad + ((arr + 15) & ~15ull);
    }
    uint64_t room() const { return in_pad + out_pad + arr + 64; }
    struct Arrays {
        uint64_t *in_off, *out_off;
        uint32_t *len, *slot;
    };
    Arrays arrays(uint8_t *base) const {
        uint64_t *off = reinterpret_cast<uint64_t *>(base + in_pad);
        uint32_t *len = reinterpret_cast<uint32_t *>(off + 2ull * cnt);
        return {off, off + cnt, len, len + cnt};
    }
};

// Package chunk: whole frames [si, j) with <= chunk_bytes input bytes (at least one frame),
// gathered frame-parallel: per-part byte sums, then offsets + arrays + gather per part.
// The chunk two back (`sc`, or null) is scattered by half the copy threads while the
// other half gathers this one (host memory, not one thread group, is the limit).
int stage_package_chunk(fpnn_aes_engine *e, HostStats &hst, HostSlot &s, HostSlot *sc,
                        const fpnn_aes_host_frame *frames, uint32_t n, uint64_t &si, uint64_t pre, uint64_t chunk_bytes,
                        ChunkLayout &c) {
    uint64_t j = si, in_b = 0;
    while (j < n && (j == si || in_b + frames[j].len <= chunk_bytes)) in_b += frames[j++].len;
    const uint32_t cnt = (uint32_t)(j - si);
    const uint64_t out_b = in_b + pre * cnt;
    c.set(cnt, in_b, out_b);
    if (int rc = slot_reserve(s, e->numa.node, c.room())) return rc;
    const ChunkLayout::Arrays h = c.arrays(s.h);
    const unsigned all = pool_of(e)->parts();
    const unsigned sparts = sc ? std::max(1u, all / 2) : 0;
    const unsigned parts = sc ? std::max(1u, all - sparts) : copy_parts(e, in_b);
    uint64_t psum[64 + 1];
    const fpnn_aes_host_frame *fr = frames + si;
    const double tg = hst.on ? HostStats::now() : 0;
    (void)part_sums(e, fr, cnt, parts, psum);
    uint8_t *h_in = s.h;
    pool_of(e)->run(parts + sparts, [&](unsigned p) {
        if (p >= parts) {
            scatter_frames_part(*sc, p - parts, sparts);
            return;
        }
        uint32_t a, b;
        part_range(cnt, p, parts, a, b);
        uint64_t io = psum[p], oo = psum[p] + pre * a;
        for (uint32_t t = a; t < b; t++) {
            const fpnn_aes_host_frame &f = fr[t];
            h.in_off[t] = io;
            h.out_off[t] = oo;
            h.len[t] = f.len;
            h.slot[t] = f.key_slot;
            copy_streaming(h_in + io, f.src, f.len);
            io += f.len;
            oo += f.len + pre;
        }
        copy_fence();
    });
    if (hst.on) hst.gather += HostStats::now() - tg;
    if (sc) sc->frames = nullptr;
    s.frames = frames;
    s.first = (uint32_t)si;
    s.count = cnt;
    s.pre = pre;
    s.out_at = c.out_at;
    s.out_off = h.out_off;
    s.scatter_bytes = out_b;
    si = j;
    return FPNN_AES_OK;
}

// Stream chunk: the plan's next pieces gathered back to back, one segment per stream the
// chunk touches; arrays and gather/scatter jobs come from the pieces.
int stage_stream_chunk(fpnn_aes_engine *e, HostStats &hst, HostSlot &s, const fpnn_aes_host_frame *frames,
                       StreamPlan &plan, uint64_t chunk_bytes, uint64_t quota, ChunkLayout &c) {
    std::vector<Piece> pieces;
    std::vector<ChunkSeg> cs;
    uint32_t uni;
    plan.next_chunk(chunk_bytes, quota, pieces, cs, c.state0, uni);
    if (uni) c.uniform = uni;
    const uint32_t cnt = (uint32_t)cs.size();
    const uint64_t in_b = cs.back().at + cs.back().len;
    c.set(cnt, in_b, in_b);
    if (int rc = slot_reserve(s, e->numa.node, c.room())) return rc;
    const ChunkLayout::Arrays h = c.arrays(s.h);
    for (uint32_t t = 0; t < cnt; t++) {
        h.in_off[t] = h.out_off[t] = cs[t].at;
        h.len[t] = (uint32_t)cs[t].len;
        h.slot[t] = cs[t].slot;
    }
    std::vector<CopyJob> gather;
    s.scatter.clear();
    s.scatter_bytes = in_b;
    uint64_t at = 0;
    for (const Piece &pc : pieces) {
        const fpnn_aes_host_frame &f = frames[pc.frame];
        gather.push_back({s.h + at, f.src + pc.off, pc.len});
        s.scatter.push_back({f.dst + pc.off, s.h + c.out_at + at, pc.len});
        at += pc.len;
    }
    const double tg = hst.on ? HostStats::now() : 0;
    pool_of(e)->copy(gather, in_b, copy_parts(e, in_b));
    if (hst.on) hst.gather += HostStats::now() - tg;
    return FPNN_AES_OK;
}

// The device batch over a chunk staged at d (input) and d + out_at (output): `count`
// segments of `uniform` bytes each, back to back (dense staging: the K2 / K1d fast paths),
// or, with uniform < 0, as the device arrays in_off / out_off / len say.
fpnn_aes_batch chunk_batch(uint8_t *d, uint64_t out_at, uint32_t count, const fpnn_aes_keyset *keys, uint64_t pre,
                           int64_t uniform, const uint64_t *in_off, const uint64_t *out_off, const uint32_t *len,
                           const uint32_t *slot) {
    fpnn_aes_batch b;
    memset(&b, 0, sizeof b);
    b.in = d;
    b.out = d + out_at;
    b.count = count;
    b.keys = keys;
    b.flags = pre ? FPNN_AES_F_WIRE_PREFIX : 0u;
    if (uniform >= 0) {
        b.stride = (uint64_t)uniform;
        b.uniform_len = (uint32_t)uniform;
    } else {
        b.in_off = in_off;
        b.out_off = out_off;
        b.len = len;
    }
    b.key_slot = keys->count > 1 ? slot : nullptr;
    return b;
}

// package: the chunk in the slot after k, if it is a package chunk still in flight, is
// waited for here and scattered beside the gather of the next chunk (stage_package_chunk)
int scatter_partner(fpnn_aes_engine *e, HostStats &hst, int k, HostSlot *&sc) {
    constexpr int kSlots = (int)(sizeof(e->hs) / sizeof(e->hs[0]));
    HostSlot &o = e->hs[(k + 1) % kSlots];
    sc = nullptr;
    if (!o.busy || !o.frames) return FPNN_AES_OK;
    const double tw = hst.on ? HostStats::now() : 0;
    HIP_TRY(hipEventSynchronize(o.done));
    if (hst.on) hst.wait += HostStats::now() - tw;
    o.busy = false;
    sc = &o;
    return FPNN_AES_OK;
}

// Host-frame pipeline shared by the package and stream entry points.
//   package: one segment per frame (key slot frames[i].key_slot, fresh chain).
//   stream : one segment per distinct stream slot = the concatenation of that
//            stream's frames in array order (CFB over a concatenation equals the
//            successive calls, base/rijndael.c:1171-1201 carries ivec/num), whose
//            state lives in iv_state/pos_state[slot] on the host.
// Chunks are gathered into pinned staging by the copy pool, then H2D and D2H run on the
// slot's stream and the kernel on the engine stream (events hand the chunk over) while
// the host gathers the next chunk.  Kernels of successive chunks are therefore ordered:
// they share the engine's scratch, and in stream mode a stream split across chunks
// continues from the state the previous chunk left.
int host_pipeline(fpnn_aes_engine *e, bool encrypt, bool stream, const fpnn_aes_host_frame *frames, uint32_t n,
                  const fpnn_aes_keyset *keys, uint32_t flags, uint8_t *iv_state, uint32_t *pos_state,
                  const HostAt *at = nullptr) {
    const HostActive active_call(e->device);
    const uint64_t pre = (!stream && (flags & FPNN_AES_F_WIRE_PREFIX)) ? 4 : 0;
    // input bytes per pipeline chunk.  (Quarter-call chunks for small calls, so one IO
    // cycle's 8 MiB flush would overlap its steps, measured slower: 1.37 against 0.83 ms
    // per flush, each chunk's copies getting fewer threads, gpurun_out r05d.)
    const uint64_t kChunk = 32ull << 20;
    // (package chunks walk `frames` directly)
    StreamPlan plan(frames, stream ? n : 0, !stream ? 0 : at ? at->slot_bound : keys->count);
    if (stream && plan.segs.empty()) return FPNN_AES_OK;
    e->host_path = "host_staged";
    const uint64_t nseg = stream ? plan.segs.size() : n;
    HostStats hst;
    const double t_call = hst.on ? HostStats::now() : 0;
    uint64_t nchunks = 0;
    DeviceGuard g(e->device);
    // order the slot streams after work already queued on the engine stream
    for (auto &sl : e->hs)
        if (int rc = slot_reserve(sl, e->numa.node, 0)) return rc;
    HIP_TRY(hipEventRecord(e->hs[0].kdone, e->stream));
    for (auto &sl : e->hs) HIP_TRY(hipStreamWaitEvent(sl.st, e->hs[0].kdone, 0));
    // ---- stream state: compact (iv, pos) of the touched streams on the device ----------
    uint8_t *d_state = nullptr, *h_state = nullptr;
    uint64_t chunk = kChunk, quota = 0;
    if (stream && !at) {
        if (int rc = sstate_reserve(e, nseg * 20)) return rc;
        h_state = e->h_sstate;
        d_state = e->sstate.p;
        // (a fresh d_state is stream-ordered on the engine stream: the upload below waits for it)
        HIP_TRY(hipEventRecord(e->hs[0].kdone, e->stream));
        HIP_TRY(hipStreamWaitEvent(e->hs[0].st, e->hs[0].kdone, 0));
        pack_stream_state(plan.segs, iv_state, pos_state, h_state);
    }
    if (stream) {
        // bigger chunks for few long streams (more chain steps per launch), quota per
        // stream so one chunk spans as many streams as it can
        // (the mapped path keeps fixed chunks and a floor of 1024: the difference is kept on purpose)
        chunk = std::min<uint64_t>(256ull << 20, std::max<uint64_t>(kChunk, plan.left / 4));
        quota = std::max<uint64_t>(16u << 10, (chunk / nseg + 15) & ~15ull);
        if (!at) (void)hipMemcpyAsync(d_state, h_state, nseg * 20, hipMemcpyHostToDevice, e->hs[0].st);
    }
    int rc = FPNN_AES_OK;
    uint64_t si = 0;  // package: next frame
    int k = 0;
    bool ciphered = false;
    constexpr int kSlots = (int)(sizeof(e->hs) / sizeof(e->hs[0]));
    while ((stream ? plan.left > 0 : si < n) && rc == FPNN_AES_OK) {
        HostSlot &s = e->hs[k];
        if ((rc = slot_drain(e, s, hst))) break;  // package: already scattered beside a gather
        ChunkLayout c;
        if (stream) {
            rc = stage_stream_chunk(e, hst, s, frames, plan, chunk, quota, c);
        } else {
            HostSlot *sc = nullptr;
            if (int rw = scatter_partner(e, hst, k, sc)) return rw;
            rc = stage_package_chunk(e, hst, s, sc, frames, n, si, pre, kChunk, c);
        }
        if (rc) break;
        nchunks++;
        HIP_TRY(hipMemcpyAsync(s.d, s.h, c.in_pad + c.arr, hipMemcpyHostToDevice, s.st));
        // The cipher runs on the engine stream: chunks share the engine's scratch (block
        // map, plan, length order, queue counter), so their kernels must not overlap --
        // and stream chunks continue from the state the previous chunk left.  The copies
        // of the slots still overlap each other and the kernels.
        HIP_TRY(hipEventRecord(s.staged, s.st));
        HIP_TRY(hipStreamWaitEvent(e->stream, s.staged, 0));
        // (stream encrypt, every stream taking the same quota: a uniform batch skips the
        // ragged length ordering, MappedStream::batch)
        const ChunkLayout::Arrays d = c.arrays(s.d);
        fpnn_aes_batch b = chunk_batch(s.d, c.out_at, c.cnt, keys, pre, encrypt ? c.uniform : int64_t(-1),
                                       d.in_off, pre ? d.out_off : nullptr, d.len, d.slot);
        if (at) {  // the chunk's slot array, uploaded with its descriptors, addresses key and state
            b.key_slot = nullptr;
            rc = run_batch_at(e, encrypt, &b, d.slot, at->slot_bound, iv_state, pos_state);
        } else {
            uint8_t *ivp = stream ? d_state + 16 * c.state0 : nullptr;
            uint32_t *posp = stream ? reinterpret_cast<uint32_t *>(d_state + 16 * nseg) + c.state0 : nullptr;
            rc = run_batch(e, encrypt, &b, ivp, posp, stream);
        }
        if (rc) break;
        HIP_TRY(hipEventRecord(s.kdone, e->stream));
        HIP_TRY(hipStreamWaitEvent(s.st, s.kdone, 0));
        HIP_TRY(hipMemcpyAsync(s.h + c.out_at, s.d + c.out_at, c.out_pad, hipMemcpyDeviceToHost, s.st));
        HIP_TRY(hipEventRecord(s.done, s.st));
        s.busy = true;
        ciphered = true;
        k = (k + 1) % kSlots;
    }
    for (auto &sl : e->hs) {
        const int r2 = slot_drain(e, sl, hst);
        if (!rc) rc = r2;
    }
    if (stream && !at) {
        if (!rc && ciphered) {
            const hipError_t err = hipMemcpy(h_state, d_state, nseg * 20, hipMemcpyDeviceToHost);
            if (err != hipSuccess) rc = hip_fail(err, "hipMemcpy(stream state)");
        }
        if (!rc) unpack_stream_state(plan.segs, h_state, iv_state, pos_state);
    }
    if (hst.on)
        fprintf(stderr, "[fpnn_aes host] %s %s: %u frames, %llu segments, %llu chunks, %.2f ms total, gather %.2f, "
                "scatter %.2f, wait %.2f ms, %u copy threads\n", stream ? "stream" : "package",
                encrypt ? "encrypt" : "decrypt", n, (unsigned long long)nseg, (unsigned long long)nchunks,
                1e3 * (HostStats::now() - t_call), 1e3 * hst.gather, 1e3 * hst.scatter, 1e3 * hst.wait,
                e->pool ? e->pool->parts() : 1u);
    return rc;
}

int check_host_frames(const fpnn_aes_engine *e, const fpnn_aes_host_frame *frames, uint32_t n,
                      const fpnn_aes_keyset *keys) {
    if (!e || !keys || (n && !frames)) return FPNN_AES_ERR_ARG;
    if (keys->device != e->device) return FPNN_AES_ERR_ARG;
    for (uint32_t i = 0; i < n; i++)
        if ((frames[i].len && (!frames[i].src || !frames[i].dst)) || frames[i].key_slot >= keys->count)
            return FPNN_AES_ERR_ARG;
    return FPNN_AES_OK;
}

// ---- host-mapped frames ------------------------------------------------------------------
// Host ranges registered with fpnn_aes_host_register (process-wide, portable: every GPU may
// access them).  A range's device-visible address is looked up per device on first use.
constexpr int kMapDevices = 64;
struct MappedRange {
    uintptr_t lo, hi;
    intptr_t delta[kMapDevices];  // device address - host address per device (INTPTR_MIN: not looked up)
};
std::mutex g_map_mu;
std::vector<MappedRange> g_mapped;  // sorted by lo, disjoint

// One call's view of the registry: the ranges and this device's address deltas.
struct MapView {
    std::vector<uintptr_t> lo, hi;
    std::vector<intptr_t> delta;
    // the range holding [p, p + n), or -1
    long find(const void *ptr, uint64_t n) const {
        const uintptr_t p = (uintptr_t)ptr;
        auto it = std::upper_bound(lo.begin(), lo.end(), p);
        if (it == lo.begin()) return -1;
        const size_t i = (size_t)(it - lo.begin()) - 1;
        return p + n <= hi[i] && p + n >= p ? (long)i : -1;
    }
    // find() that tries the last range hit first (frames of one arena: one search each)
    struct Cursor {
        long r = -1;
        long locate(const MapView &v, uintptr_t x, uint64_t n) {
            if (r < 0 || x < v.lo[r] || x + n > v.hi[r]) r = v.find((const void *)x, n);
            return r;
        }
    };
    // the device-visible address of x, which lies in range r
    uint64_t device(long r, uintptr_t x) const { return (uint64_t)((intptr_t)x + delta[r]); }
};

int map_view(int device, MapView &v) {
    std::lock_guard<std::mutex> lk(g_map_mu);
    v.lo.clear();
    v.hi.clear();
    v.delta.clear();
    if (device < 0 || device >= kMapDevices) return FPNN_AES_OK;  // (no mapped path there)
    for (auto &r : g_mapped) {
        if (r.delta[device] == INTPTR_MIN) {
            DeviceGuard g(device);
            void *dp = nullptr;
            HIP_TRY(hipHostGetDevicePointer(&dp, reinterpret_cast<void *>(r.lo), 0));
            r.delta[device] = (intptr_t)dp - (intptr_t)r.lo;
        }
        v.lo.push_back(r.lo);
        v.hi.push_back(r.hi);
        v.delta.push_back(r.delta[device]);
    }
    return FPNN_AES_OK;
}

// The first of fr[0 .. cnt) whose source (len bytes) or destination (len + pre bytes) does
// not lie in registered memory; cnt: none.  (Frames behind one found are not looked at.)
uint32_t first_unmapped(fpnn_aes_engine *e, const MapView &v, const fpnn_aes_host_frame *fr, uint32_t cnt, uint64_t pre) {
    const unsigned parts = cnt >= 16384 ? pool_of(e)->parts() : 1u;
    std::atomic<uint32_t> bad{cnt};
    pool_of(e)->run(parts, [&](unsigned p) {
        uint32_t a0, b0;
        part_range(cnt, p, parts, a0, b0);
        MapView::Cursor cs, cd;
        for (uint32_t q = a0; q < b0 && q < bad.load(std::memory_order_relaxed); q++) {
            const fpnn_aes_host_frame &f = fr[q];
            bool ok = true;
            if (f.len) ok = cs.locate(v, (uintptr_t)f.src, f.len) >= 0;
            if (ok && f.len + pre) ok = cd.locate(v, (uintptr_t)f.dst, f.len + pre) >= 0;
            if (!ok) {
                for (uint32_t cur = bad.load(); q < cur && !bad.compare_exchange_weak(cur, q);) {
                }
                return;
            }
        }
    });
    return bad.load();
}

int mslot_reserve(MapSlot &m, int node, uint64_t dneed, uint64_t hneed) {
    if (!m.gathered) {
        HIP_TRY(hipEventCreateWithFlags(&m.gathered, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&m.ciphered, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&m.done, hipEventDisableTiming));
    }
    if (dneed > m.dcap) {
        uint64_t c = m.dcap ? m.dcap : (16u << 20);
        while (c < dneed) c *= 2;
        if (m.d) (void)hipFree(m.d);
        m.d = nullptr;
        m.dcap = 0;
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&m.d), c));
        m.dcap = c;
    }
    if (hneed > m.hcap) {
        uint64_t c = m.hcap ? m.hcap : (1u << 20);
        while (c < hneed) c *= 2;
        if (m.h) (void)hipHostFree(m.h);
        m.h = nullptr;
        m.hcap = 0;
        HIP_TRY(pinned_host_alloc(node, reinterpret_cast<void **>(&m.h), c));
        m.hcap = c;
    }
    return FPNN_AES_OK;
}

// the slots' events and the move stream, before a mapped call's first HIP work
int mapped_begin(fpnn_aes_engine *e) {
    for (auto &m : e->ms)
        if (int rc = mslot_reserve(m, e->numa.node, 0, 0)) return rc;
    if (!e->map_stream) HIP_TRY(hipStreamCreateWithFlags(&e->map_stream, hipStreamNonBlocking));
    return FPNN_AES_OK;
}

// input bytes per full chunk of the mapped pipelines (FPNN_AES_MAP_CHUNK_MB, read once)
uint64_t map_chunk_bytes() {
    static const uint64_t bytes = [] {
        const char *x = getenv("FPNN_AES_MAP_CHUNK_MB");
        return (x && atoi(x) > 0 ? (uint64_t)atoi(x) : 32ull) << 20;
    }();
    return bytes;
}

// The move descriptors of a chunk, in the slot's pinned block and (same layout) at
// d + desc_at:   src u64 | so u64 | dst u64 | oo u64 | len u32   (n entries each)
// Entry i is gathered from address src[i] to staging offset so[i], and its result
// scattered from output offset oo[i] to address dst[i].  What follows (end()) is the mode's.
struct MoveDesc {
    uint64_t *src, *so, *dst, *oo;
    uint32_t *len;
    uint32_t n;
    MoveDesc(uint8_t *base, uint32_t count)
        : src(reinterpret_cast<uint64_t *>(base)), so(src + count), dst(so + count), oo(dst + count),
          len(reinterpret_cast<uint32_t *>(oo + count)), n(count) {}
    uint8_t *end() const { return reinterpret_cast<uint8_t *>(len + n); }
};

// What a mode's prepare() reports about the chunk it wrote into a slot's pinned block.
struct MapChunk {
    uint32_t moves = 0;   // entries of the move descriptors (0: no chunk in the slot)
    uint32_t prefix = 0;  // bytes the scatter writes in front of every entry's len
    uint64_t out_at = 0, desc_at = 0, desc_b = 0;  // device staging: in | out at out_at | desc at desc_at
    // the mode's own, for batch(): cipher segments, their common length (< 0: none), first state index
    uint32_t segs = 0;
    int64_t uniform = -1;
    uint64_t state0 = 0;
};

// What a mode's batch() hands the step loop to cipher a chunk.
struct MapCipher {
    fpnn_aes_batch b;
    uint8_t *iv = nullptr;  // stream mode: the (iv, pos) the chunk's first segment continues from
    uint32_t *pos = nullptr;
    // stream mode by slot (HostAt): iv / pos are the caller's device arrays of slot_bound
    // entries, segment i's key and state at state_slot[i]
    const uint32_t *state_slot = nullptr;
    uint32_t slot_bound = 0;
};

// Chunk t of a mapped call: the host writes its descriptors into its slot's pinned block
// (mode.prepare), the engine stream takes the block H2D -- the slot's `done` doubles as
// "descriptors on the device".  c.moves stays 0 where the call has no further chunk.
template <class Mode>
int stage_chunk(fpnn_aes_engine *e, HostStats &hst, Mode &mode, MapSlot &m, MapChunk &c) {
    c = MapChunk{};
    if (!mode.more()) return FPNN_AES_OK;
    if (m.busy) {  // the slot's previous pinned block went H2D
        const double tw = hst.on ? HostStats::now() : 0;
        if (hipError_t err = hipEventSynchronize(m.done)) return hip_fail(err, "hipEventSynchronize");
        if (hst.on) hst.wait += HostStats::now() - tw;
        m.busy = false;
    }
    const double tf = hst.on ? HostStats::now() : 0;
    int rc = FPNN_AES_OK;
    // the pinned block for the chunk's descriptors, the slot grown to hold the chunk (null: rc)
    auto room = [&](const MapChunk &cc) -> uint8_t * {
        const uint64_t dneed = cc.desc_at + cc.desc_b + 64, hneed = cc.desc_b + 64;
        if (dneed > m.dcap || hneed > m.hcap) {
            // growing frees the slot's buffers: let every queued use of them finish
            hipError_t err = hipStreamSynchronize(e->map_stream);
            if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
            rc = err ? hip_fail(err, "hipStreamSynchronize") : mslot_reserve(m, e->numa.node, dneed, hneed);
        }
        return rc ? nullptr : m.h;
    };
    if (!mode.prepare(c, room) || rc) {
        c.moves = 0;
        return rc;
    }
    if (hst.on) hst.gather += HostStats::now() - tf;  // (descriptor fill)
    HIP_TRY(hipMemcpyAsync(m.d + c.desc_at, m.h, c.desc_b, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipEventRecord(m.done, e->stream));
    m.busy = true;
    return FPNN_AES_OK;
}

// The rotation both mapped pipelines run.  Chunk t lives in slot t % 4 (HBM staging in | out
// | descriptors, pinned descriptor block).  Step t: on the move stream ONE launch gathers
// chunk t from host memory into its staging AND scatters chunk t - 2's results to the
// frames' destinations (both PCIe directions busy in one kernel); meanwhile the engine
// stream ciphers chunk t - 1 as an ordinary device batch and then uploads chunk t + 1's
// descriptors (written by the host threads during step t), so the move stream never waits
// for a copy.  Events hand each chunk between the two streams.  A mode provides
//   bool more()  the call has bytes left for a further chunk
//   bool prepare(MapChunk &c, room)  the next chunk's layout into c, then its descriptors
//        into the pinned block room(c) gives (false: no chunk after all, or room gave null)
//   MapCipher batch(const MapSlot &m, const MapChunk &c)  the device batch over a chunk
template <class Mode>
int mapped_steps(fpnn_aes_engine *e, bool encrypt, HostStats &hst, Mode &mode) {
    constexpr int kSlots = (int)(sizeof(e->ms) / sizeof(e->ms[0]));
    static_assert(kSlots >= 4, "a chunk's staging is live for three steps, plus the upload ahead");
    hipStream_t ms = e->map_stream;
    // the move stream starts after work already queued on the engine stream
    HIP_TRY(hipEventRecord(e->ms[0].ciphered, e->stream));
    HIP_TRY(hipStreamWaitEvent(ms, e->ms[0].ciphered, 0));
    MapChunk ch[kSlots];
    auto jobs_of = [&](int slot, MoveJob &gather, MoveJob &scatter) {
        const MapChunk &c = ch[slot];
        MapSlot &m = e->ms[slot];
        const MoveDesc d(m.d + c.desc_at, c.moves);
        gather = MoveJob{0, d.src, (uint64_t)(uintptr_t)m.d, d.so, d.len, 0, c.moves};
        scatter = MoveJob{(uint64_t)(uintptr_t)(m.d + c.out_at), d.oo, 0, d.dst, d.len, c.prefix, c.moves};
    };
    int rc = stage_chunk(e, hst, mode, e->ms[0], ch[0]);
    const MoveJob none{0, nullptr, 0, nullptr, nullptr, 0, 0};
    for (uint64_t t = 0; rc == FPNN_AES_OK; t++) {
        const int kt = (int)(t % kSlots), k1 = (int)((t + kSlots - 1) % kSlots), k2 = (int)((t + kSlots - 2) % kSlots);
        const bool gather_t = ch[kt].moves != 0;
        const bool cipher_t1 = t >= 1 && ch[k1].moves != 0;
        const bool scatter_t2 = t >= 2 && ch[k2].moves != 0;
        if (!gather_t && !cipher_t1 && !scatter_t2) break;
        // move stream: gather t || scatter t - 2
        MoveJob gj = none, sj = none, tmp;
        if (gather_t) {
            HIP_TRY(hipStreamWaitEvent(ms, e->ms[kt].done, 0));
            jobs_of(kt, gj, tmp);
        }
        if (scatter_t2) {
            HIP_TRY(hipStreamWaitEvent(ms, e->ms[k2].ciphered, 0));
            jobs_of(k2, tmp, sj);
        }
        HIP_TRY(launch_move_segments(gj, sj, ms));
        if (gather_t) HIP_TRY(hipEventRecord(e->ms[kt].gathered, ms));
        // engine stream: cipher t - 1, then upload chunk t + 1 (its slot's previous chunk,
        // t - 3, was scattered by step t - 1's launch, which the cipher waited for); the
        // cipher is queued before the host prepares chunk t + 1's descriptors (the engine
        // stream is not left empty while the host works)
        if (cipher_t1) {
            MapSlot &m = e->ms[k1];
            HIP_TRY(hipStreamWaitEvent(e->stream, m.gathered, 0));
            const MapCipher x = mode.batch(m, ch[k1]);
            if (x.state_slot) rc = run_batch_at(e, encrypt, &x.b, x.state_slot, x.slot_bound, x.iv, x.pos);
            else rc = run_batch(e, encrypt, &x.b, x.iv, x.pos, x.iv != nullptr);
            if (rc) break;
            HIP_TRY(hipEventRecord(m.ciphered, e->stream));
        }
        // host: chunk t + 1's descriptors while the GPU moves and ciphers
        // (chunk t + 1 exists only if chunk t - 1 does, for t >= 1: the upload always
        // follows a cipher; at t = 0 the slot is unused)
        if ((rc = stage_chunk(e, hst, mode, e->ms[(t + 1) % kSlots], ch[(t + 1) % kSlots]))) break;
        if (scatter_t2) ch[k2].moves = 0;  // (its slot's next chunk is prepared at step t + 1)
    }
    hst.drain_from = hst.on ? HostStats::now() : 0;
    HIP_TRY(hipStreamSynchronize(ms));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (int rf = stream_idle(e)) rc = rc ? rc : rf;
    for (auto &m : e->ms) m.busy = false;
    return rc;
}

// Package-mode host frames in registered memory: chunks of whole frames, one move entry and
// one cipher segment per frame (uniform lengths keep the dense K2 / K1d paths).  A chunk
// ends before the first frame that is not in registered memory, and no chunk follows it:
// the caller takes the rest through the staged path.
// Descriptor block of a chunk: the move descriptors, then slot u32 per frame.
struct MappedPackage {
    fpnn_aes_engine *e;
    const fpnn_aes_host_frame *frames;
    uint32_t n;
    const fpnn_aes_keyset *keys;
    uint64_t pre;
    const MapView &v;
    uint32_t si = 0;    // next frame
    bool stop = false;  // a frame outside registered memory ended the mapped chunks

    bool more() const { return si < n && !stop; }

    template <class Room>
    bool prepare(MapChunk &c, Room &&room) {
        const uint64_t kChunk = map_chunk_bytes();
        const uint32_t kMaxFrames = 1u << 20;  // frames per chunk (descriptor block <= 40 MiB)
        uint64_t in_b = 0;
        uint32_t j = si;
        while (j < n && (j == si || (in_b + frames[j].len <= kChunk && j - si < kMaxFrames))) in_b += frames[j++].len;
        uint32_t cnt = j - si;
        const fpnn_aes_host_frame *fr = frames + si;
        const uint32_t bad = first_unmapped(e, v, fr, cnt, pre);
        if (bad < cnt) {
            cnt = bad;
            j = si + cnt;
            stop = true;  // no chunk after this one
            if (!cnt) return false;
        }
        const unsigned parts = cnt >= 16384 ? pool_of(e)->parts() : 1u;
        uint64_t psum[64 + 1];
        // (uniform lengths without the prefix: dense uniform staging)
        if (part_sums(e, fr, cnt, parts, psum) && !pre) c.uniform = fr[0].len;
        in_b = psum[parts];
        const uint64_t out_b = in_b + pre * cnt;
        const uint64_t in_pad = (in_b + 255) & ~255ull, out_pad = (out_b + 255) & ~255ull;
        c.prefix = (uint32_t)pre;
        c.out_at = in_pad;
        c.desc_at = in_pad + out_pad;
        c.desc_b = (uint64_t)cnt * 40;
        uint8_t *block = room(c);
        if (!block) return false;
        const MoveDesc h(block, cnt);
        uint32_t *h_slot = reinterpret_cast<uint32_t *>(h.end());
        pool_of(e)->run(parts, [&](unsigned p) {
            uint32_t a0, b0;
            part_range(cnt, p, parts, a0, b0);
            uint64_t io = psum[p], oo = psum[p] + pre * a0;
            MapView::Cursor cs, cd;
            for (uint32_t q = a0; q < b0; q++) {
                const fpnn_aes_host_frame &f = fr[q];
                const uintptr_t xs = (uintptr_t)f.src, xd = (uintptr_t)f.dst;
                h.src[q] = f.len ? v.device(cs.locate(v, xs, f.len), xs) : 0;
                h.so[q] = io;
                h.dst[q] = f.len + pre ? v.device(cd.locate(v, xd, f.len + pre), xd) : 0;
                h.oo[q] = oo;
                h.len[q] = f.len;
                h_slot[q] = f.key_slot;
                io += f.len;
                oo += f.len + pre;
            }
        });
        c.moves = cnt;
        si = j;
        return true;
    }

    MapCipher batch(const MapSlot &m, const MapChunk &c) const {
        const MoveDesc d(m.d + c.desc_at, c.moves);
        return {chunk_batch(m.d, c.out_at, c.moves, keys, pre, c.uniform, d.so, d.oo, d.len,
                            reinterpret_cast<const uint32_t *>(d.end()))};
    }
};

int mapped_pipeline(fpnn_aes_engine *e, bool encrypt, const fpnn_aes_host_frame *frames, uint32_t n,
                    const fpnn_aes_keyset *keys, uint32_t flags, const MapView &v, uint32_t *done) {
    const HostActive active_call(e->device);
    HostStats hst;
    const double t_call = hst.on ? HostStats::now() : 0;
    DeviceGuard g(e->device);
    if (int rc = mapped_begin(e)) return rc;
    MappedPackage mode{e, frames, n, keys, (flags & FPNN_AES_F_WIRE_PREFIX) ? 4u : 0u, v};
    const int rc = mapped_steps(e, encrypt, hst, mode);
    *done = mode.si;
    e->host_path = "host_mapped";
    if (hst.on)
        fprintf(stderr, "[fpnn_aes host] mapped %s: %u frames, %.2f ms total, descriptors %.2f, slot waits %.2f, "
                "final drain %.2f ms, chunk %llu MiB\n", encrypt ? "encrypt" : "decrypt", n,
                1e3 * (HostStats::now() - t_call), 1e3 * hst.gather, 1e3 * hst.wait,
                1e3 * (HostStats::now() - hst.drain_from), (unsigned long long)(map_chunk_bytes() >> 20));
    return rc;
}

// Stream-mode host frames in registered memory: the chunking of the staged path (one
// segment per stream = its frames in array order, round-robin quotas so a chunk advances
// many chains) with the mapped moves, one move entry per piece.  The engine stream ciphers
// the chunks in order with the streams' carried (iv, pos), so a stream split across chunks
// continues from the state the previous chunk left.
// Descriptor block of a chunk: the move descriptors, then (8-aligned) per stream segment
// off u64 | len u32 | slot u32.
struct MappedStream {
    fpnn_aes_engine *e;
    const fpnn_aes_host_frame *frames;
    const fpnn_aes_keyset *keys;
    const MapView &v;
    StreamPlan &plan;
    bool encrypt;
    uint64_t chunk, quota;
    uint8_t *d_state;
    const HostAt *at;                // by slot: the caller's device state arrays (d_state unused)
    uint8_t *at_iv;
    uint32_t *at_pos;
    std::vector<Piece> pieces;
    std::vector<ChunkSeg> cs;

    struct SegDesc {
        uint64_t *off;
        uint32_t *len, *slot;
        SegDesc(uint8_t *after_moves, uint32_t ns)
            : off(reinterpret_cast<uint64_t *>(((uint64_t)(uintptr_t)after_moves + 7) & ~7ull)),
              len(reinterpret_cast<uint32_t *>(off + ns)), slot(len + ns) {}
    };

    bool more() const { return plan.left != 0; }

    template <class Room>
    bool prepare(MapChunk &c, Room &&room) {
        uint32_t uni;
        plan.next_chunk(chunk, quota, pieces, cs, c.state0, uni);
        // every stream takes the same quota (S1's middle chunks): a uniform batch, so the
        // encrypt skips the ragged length ordering (its bucket counters see one length:
        // 16 384 atomics on one word, ~1 ms per chunk in the r04q trace)
        if (encrypt && uni) c.uniform = uni;
        const uint32_t np = (uint32_t)pieces.size(), ns = (uint32_t)cs.size();
        const uint64_t in_b = cs.back().at + cs.back().len;
        const uint64_t in_pad = (in_b + 255) & ~255ull;
        c.out_at = in_pad;
        c.desc_at = 2 * in_pad;
        c.desc_b = (uint64_t)np * 36 + 8 + (uint64_t)ns * 16;
        uint8_t *block = room(c);
        if (!block) return false;
        const MoveDesc h(block, np);
        const unsigned parts = np >= 16384 ? pool_of(e)->parts() : 1u;
        std::vector<uint64_t> at(np);
        uint64_t a = 0;
        for (uint32_t q = 0; q < np; q++) {
            at[q] = a;
            a += pieces[q].len;
        }
        pool_of(e)->run(parts, [&](unsigned p) {
            uint32_t a0, b0;
            part_range(np, p, parts, a0, b0);
            MapView::Cursor cus, cud;
            for (uint32_t q = a0; q < b0; q++) {
                const Piece &pc = pieces[q];
                const fpnn_aes_host_frame &f = frames[pc.frame];
                const uintptr_t xs = (uintptr_t)f.src + pc.off, xd = (uintptr_t)f.dst + pc.off;
                h.src[q] = v.device(cus.locate(v, xs, pc.len), xs);
                h.so[q] = at[q];
                h.dst[q] = v.device(cud.locate(v, xd, pc.len), xd);
                h.oo[q] = at[q];
                h.len[q] = pc.len;
            }
        });
        const SegDesc sd(h.end(), ns);
        for (uint32_t q = 0; q < ns; q++) {
            sd.off[q] = cs[q].at;
            sd.len[q] = (uint32_t)cs[q].len;
            sd.slot[q] = cs[q].slot;
        }
        c.segs = ns;
        c.moves = np;
        return true;
    }

    MapCipher batch(const MapSlot &m, const MapChunk &c) const {
        const SegDesc sd(MoveDesc(m.d + c.desc_at, c.moves).end(), c.segs);
        if (at) {
            MapCipher x{chunk_batch(m.d, c.out_at, c.segs, keys, 0, c.uniform, sd.off, nullptr, sd.len, nullptr),
                        at_iv, at_pos, sd.slot, at->slot_bound};
            x.b.key_slot = nullptr;
            return x;
        }
        uint32_t *pos = reinterpret_cast<uint32_t *>(d_state + 16 * plan.segs.size());
        return {chunk_batch(m.d, c.out_at, c.segs, keys, 0, c.uniform, sd.off, nullptr, sd.len, sd.slot),
                d_state + 16 * c.state0, pos + c.state0};
    }
};

int mapped_stream_pipeline(fpnn_aes_engine *e, bool encrypt, const fpnn_aes_host_frame *frames, uint32_t n,
                           const fpnn_aes_keyset *keys, const MapView &v, uint8_t *iv_state, uint32_t *pos_state,
                           const HostAt *at = nullptr) {
    const HostActive active_call(e->device);
    HostStats hst;
    const double t_call = hst.on ? HostStats::now() : 0;
    StreamPlan plan(frames, n, at ? at->slot_bound : keys->count);  // streams in array order
    if (plan.segs.empty()) return FPNN_AES_OK;
    const uint64_t nseg = plan.segs.size();
    const double t_sorted = hst.on ? HostStats::now() : 0;
    DeviceGuard g(e->device);
    if (int rc = mapped_begin(e)) return rc;
    // ---- the streams' (iv, pos), compact, on the device (engine stream) ----
    uint8_t *h_state = nullptr, *d_state = nullptr;
    if (!at) {
        if (int rc = sstate_reserve(e, nseg * 20)) return rc;
        h_state = e->h_sstate, d_state = e->sstate.p;
        pack_stream_state(plan.segs, iv_state, pos_state, h_state);
        HIP_TRY(hipMemcpyAsync(d_state, h_state, nseg * 20, hipMemcpyHostToDevice, e->stream));
    }
    // Chunks of FPNN_AES_MAP_CHUNK_MB (as the package path: the moves of chunk t overlap the
    // cipher of chunk t - 1, so more, smaller chunks pipeline better than a few large ones),
    // each taking a quota from as many streams as fit: the encrypt of a chunk is one serial
    // CFB chain per stream, so its parallelism is the number of streams it spans.
    // (the staged path grows its chunks and keeps a floor of 16 Ki: the difference is kept on purpose)
    const uint64_t chunk = map_chunk_bytes();
    const uint64_t quota = std::max<uint64_t>(1024, (chunk / nseg + 15) & ~15ull);
    MappedStream mode{e, frames, keys, v, plan, encrypt, chunk, quota, d_state, at, iv_state, pos_state};
    const int rc = mapped_steps(e, encrypt, hst, mode);
    if (!rc && !at) {
        HIP_TRY(hipMemcpy(h_state, d_state, nseg * 20, hipMemcpyDeviceToHost));
        unpack_stream_state(plan.segs, h_state, iv_state, pos_state);
    }
    e->host_path = "host_mapped";
    if (hst.on)
        fprintf(stderr, "[fpnn_aes host] mapped stream %s: %u frames, %llu streams, %.2f ms total, sort %.2f, "
                "descriptors %.2f, slot waits %.2f, final drain %.2f ms\n", encrypt ? "encrypt" : "decrypt", n,
                (unsigned long long)nseg, 1e3 * (HostStats::now() - t_call), 1e3 * (t_sorted - t_call),
                1e3 * hst.gather, 1e3 * hst.wait, 1e3 * (HostStats::now() - hst.drain_from));
    return rc;
}

bool mapped_enabled() {
    const char *v = getenv("FPNN_AES_HOST_MAPPED");
    return !v || atoi(v) != 0;
}

}  // namespace

extern "C" {

int fpnn_aes_package_host(fpnn_aes_engine *e, int encrypt, const fpnn_aes_host_frame *frames, uint32_t n,
                          const fpnn_aes_keyset *keys, uint32_t flags) {
    if (int rc = check_host_frames(e, frames, n, keys)) return rc;
    if (int rc = debug_fail_point()) return rc;
    if (!encrypt && (flags & FPNN_AES_F_WIRE_PREFIX)) return FPNN_AES_ERR_ARG;
    if (flags & FPNN_AES_F_WIRE_PREFIX)
        for (uint32_t i = 0; i < n; i++)
            if (!frames[i].dst) return FPNN_AES_ERR_ARG;
    if (!n) return FPNN_AES_OK;
    if (mapped_enabled()) {  // every frame in registered host memory: the GPU moves the bytes
        MapView v;
        if (int rc = map_view(e->device, v)) return rc;
        const uint64_t pre = (flags & FPNN_AES_F_WIRE_PREFIX) ? 4 : 0;
        if (!v.lo.empty() && (!frames[0].len || v.find(frames[0].src, frames[0].len) >= 0) &&
            (!(frames[0].len + pre) || v.find(frames[0].dst, frames[0].len + pre) >= 0)) {
            // frames in registered memory from the first on: mapped until the first frame
            // that is not, the rest (if any) staged -- package frames are independent
            uint32_t done = 0;
            if (int rc = mapped_pipeline(e, encrypt != 0, frames, n, keys, flags, v, &done)) return rc;
            if (done == n) return FPNN_AES_OK;
            frames += done;
            n -= done;
            const int rc = host_pipeline(e, encrypt != 0, false, frames, n, keys, flags, nullptr, nullptr);
            if (done) e->host_path = "host_mapped+staged";
            return rc;
        }
    }
    return host_pipeline(e, encrypt != 0, false, frames, n, keys, flags, nullptr, nullptr);
}

int fpnn_aes_host_register(void *ptr, size_t len) {
    if (!ptr || !len) return FPNN_AES_ERR_ARG;
    const uintptr_t lo = (uintptr_t)ptr, hi = lo + len;
    if (hi < lo) return FPNN_AES_ERR_ARG;
    std::lock_guard<std::mutex> lk(g_map_mu);
    auto it = std::lower_bound(g_mapped.begin(), g_mapped.end(), lo,
                               [](const MappedRange &r, uintptr_t x) { return r.lo < x; });
    if ((it != g_mapped.end() && it->lo < hi) || (it != g_mapped.begin() && std::prev(it)->hi > lo)) {
        g_last_error = "fpnn_aes_host_register: range overlaps a registered range";
        return FPNN_AES_ERR_ARG;
    }
    HIP_TRY(hipHostRegister(ptr, len, hipHostRegisterPortable | hipHostRegisterMapped));
    MappedRange r;
    r.lo = lo;
    r.hi = hi;
    for (auto &d : r.delta) d = INTPTR_MIN;
    g_mapped.insert(it, r);
    return FPNN_AES_OK;
}

int fpnn_aes_host_unregister(void *ptr) {
    std::lock_guard<std::mutex> lk(g_map_mu);
    auto it = std::find_if(g_mapped.begin(), g_mapped.end(), [ptr](const MappedRange &r) { return r.lo == (uintptr_t)ptr; });
    if (it == g_mapped.end()) return FPNN_AES_ERR_ARG;
    g_mapped.erase(it);
    HIP_TRY(hipHostUnregister(ptr));
    return FPNN_AES_OK;
}

int fpnn_aes_host_is_mapped(const void *ptr, size_t len) {
    std::lock_guard<std::mutex> lk(g_map_mu);
    const uintptr_t p = (uintptr_t)ptr;
    for (const auto &r : g_mapped)
        if (p >= r.lo && p + len <= r.hi && p + len >= p) return 1;
    return 0;
}

int fpnn_aes_stream_host(fpnn_aes_engine *e, int encrypt, const fpnn_aes_host_frame *frames, uint32_t n,
                         const fpnn_aes_keyset *keys, uint8_t *iv_state, uint32_t *pos_state) {
    if (int rc = check_host_frames(e, frames, n, keys)) return rc;
    if (int rc = debug_fail_point()) return rc;
    if (n && (!iv_state || !pos_state)) return FPNN_AES_ERR_ARG;
    if (!n) return FPNN_AES_OK;
    if (mapped_enabled()) {  // every frame in registered host memory: the GPU moves the bytes
        MapView v;
        if (int rc = map_view(e->device, v)) return rc;
        if (!v.lo.empty() && first_unmapped(e, v, frames, n, 0) == n)  // (stream frames depend on each other)
            return mapped_stream_pipeline(e, encrypt != 0, frames, n, keys, v, iv_state, pos_state);
    }
    return host_pipeline(e, encrypt != 0, true, frames, n, keys, 0, iv_state, pos_state);
}

// Stream-mode host frames of connections that live in the key table on the device: key and
// (iv, pos) by table slot, the state in the device arrays fpnn_aes_stream_open wrote.  The host
// knows every slot, so a bad one fails here, before anything is queued or touched.
int fpnn_aes_stream_host_at(fpnn_aes_engine *e, int encrypt, const fpnn_aes_host_frame *frames, uint32_t n,
                            const fpnn_aes_keyset *keys, uint32_t slot_bound, uint8_t *iv_state, uint32_t *pos_state) {
    if (!e || !keys || (n && !frames)) return FPNN_AES_ERR_ARG;
    if (keys->device != e->device || keys->count == 0) return FPNN_AES_ERR_ARG;
    if (slot_bound > fpnn_aes_keyset_capacity(keys)) return FPNN_AES_ERR_ARG;
    for (uint32_t i = 0; i < n; i++)
        if ((frames[i].len && (!frames[i].src || !frames[i].dst)) || frames[i].key_slot >= slot_bound)
            return FPNN_AES_ERR_ARG;
    if (int rc = debug_fail_point()) return rc;
    if (n && (!iv_state || !pos_state || ((uintptr_t)iv_state & 15) || ((uintptr_t)pos_state & 3)))
        return FPNN_AES_ERR_ARG;
    if (!n) return FPNN_AES_OK;
    const HostAt at{slot_bound};
    if (mapped_enabled()) {  // every frame in registered host memory: the GPU moves the bytes
        MapView v;
        if (int rc = map_view(e->device, v)) return rc;
        if (!v.lo.empty() && first_unmapped(e, v, frames, n, 0) == n)  // (stream frames depend on each other)
            return mapped_stream_pipeline(e, encrypt != 0, frames, n, keys, v, iv_state, pos_state, &at);
    }
    return host_pipeline(e, encrypt != 0, true, frames, n, keys, 0, iv_state, pos_state, &at);
}

// ---- one host batch over several engines (GPUs) ------------------------------------------
// Each engine runs its share through its own host_pipeline in its own thread (engine 0's in
// the caller's), on that engine's NUMA node; errors are collected and the first one (by
// engine index) is returned, with its message.
static int run_multi(fpnn_aes_engine *const *engines, int n_engines, const std::function<int(int)> &fn) {
    std::vector<int> rc(n_engines, FPNN_AES_OK);
    std::vector<std::string> msg(n_engines);
    std::vector<std::thread> th;
    for (int k = 1; k < n_engines; k++)
        th.emplace_back([&, k] {
            (void)fpnn_aes::numa_pin_thread(engines[k]->numa);
            rc[k] = fn(k);
            if (rc[k]) msg[k] = g_last_error;
        });
    rc[0] = fn(0);
    if (rc[0]) msg[0] = g_last_error;
    for (auto &t : th) t.join();
    for (int k = 0; k < n_engines; k++)
        if (rc[k]) {
            g_last_error = "engine " + std::to_string(k) + ": " + msg[k];
            return rc[k];
        }
    return FPNN_AES_OK;
}

int fpnn_aes_package_host_multi(fpnn_aes_engine *const *engines, const fpnn_aes_keyset *const *keys, int n_engines,
                                int encrypt, const fpnn_aes_host_frame *frames, uint32_t n, uint32_t flags) {
    if (!engines || !keys || n_engines < 1 || (n && !frames)) return FPNN_AES_ERR_ARG;
    for (int k = 0; k < n_engines; k++)
        if (!engines[k] || !keys[k] || keys[k]->count != keys[0]->count || keys[k]->nrounds != keys[0]->nrounds)
            return FPNN_AES_ERR_ARG;
    if (n_engines == 1 || n < 2) return fpnn_aes_package_host(engines[0], encrypt, frames, n, keys[0], flags);
    // byte-balanced contiguous ranges of frames
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) total += frames[i].len;
    std::vector<uint32_t> cut(n_engines + 1, n);
    cut[0] = 0;
    uint64_t acc = 0;
    int p = 1;
    for (uint32_t i = 0; i < n && p < n_engines; i++) {
        acc += frames[i].len;
        while (p < n_engines && acc * n_engines >= total * p) cut[p++] = i + 1;
    }
    return run_multi(engines, n_engines, [&](int k) {
        return fpnn_aes_package_host(engines[k], encrypt, frames + cut[k], cut[k + 1] - cut[k], keys[k], flags);
    });
}

int fpnn_aes_stream_host_multi(fpnn_aes_engine *const *engines, const fpnn_aes_keyset *const *keys, int n_engines,
                               int encrypt, const fpnn_aes_host_frame *frames, uint32_t n, uint8_t *iv_state,
                               uint32_t *pos_state) {
    if (!engines || !keys || n_engines < 1 || (n && (!frames || !iv_state || !pos_state))) return FPNN_AES_ERR_ARG;
    for (int k = 0; k < n_engines; k++)
        if (!engines[k] || !keys[k] || keys[k]->count != keys[0]->count || keys[k]->nrounds != keys[0]->nrounds)
            return FPNN_AES_ERR_ARG;
    if (n_engines == 1 || n < 2)
        return fpnn_aes_stream_host(engines[0], encrypt, frames, n, keys[0], iv_state, pos_state);
    // whole streams to engines, longest first onto the least-loaded engine (a stream's frames
    // stay in order on one engine: its CFB state chains through them)
    std::unordered_map<uint32_t, uint64_t> bytes;
    for (uint32_t i = 0; i < n; i++) bytes[frames[i].key_slot] += frames[i].len;
    std::vector<std::pair<uint64_t, uint32_t>> order;
    order.reserve(bytes.size());
    for (const auto &kv : bytes) order.push_back({kv.second, kv.first});
    std::sort(order.begin(), order.end(), [](const std::pair<uint64_t, uint32_t> &a,
                                             const std::pair<uint64_t, uint32_t> &b) {
        return a.first != b.first ? a.first > b.first : a.second < b.second;
    });
    std::vector<uint64_t> load(n_engines, 0);
    std::unordered_map<uint32_t, int> owner;
    for (const auto &o : order) {
        const int k = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        owner[o.second] = k;
        load[k] += o.first;
    }
    std::vector<std::vector<fpnn_aes_host_frame>> part(n_engines);
    for (uint32_t i = 0; i < n; i++) part[owner[frames[i].key_slot]].push_back(frames[i]);
    return run_multi(engines, n_engines, [&](int k) {
        return fpnn_aes_stream_host(engines[k], encrypt, part[k].data(), (uint32_t)part[k].size(), keys[k], iv_state,
                                    pos_state);
    });
}

}  // extern "C"
