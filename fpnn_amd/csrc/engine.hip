// engine.hip -- implementation of the C-ABI declared in include/fpnn_aes.h.
//
// Host-side responsibilities only: argument checking, key-set management, growing the
// scratch and queuing the kernels on the engine's HIP stream.  Which kernel a batch runs on
// (uniform vs general layout, uniform vs per-packet keys, package vs stream, in-place) is
// dispatch_plan.hpp's decision, how much scratch it needs scratch_plan.hpp's.  There is no
// CPU cipher in this library: every byte of payload is transformed by the HIP kernels in
// k_encrypt.hip / k_decrypt.hip.
// (The calls that take many frames from host memory are in host_frames.hip.)
#include <sys/random.h>

#include <chrono>

#include "../../include/fpnn_ecdh.h"
#include "ecc.hpp"
#include "engine_internal.hpp"

using namespace fpnn_aes;

namespace {

// device table block: t0le (1 KiB) | sbox (256) | td0le (1 KiB) | isbox (256)
const uint32_t *t0le_of(const fpnn_aes_engine *e) { return reinterpret_cast<const uint32_t *>(e->d_tables); }
const uint8_t *sbox_of(const fpnn_aes_engine *e) { return e->d_tables + 1024; }
const uint32_t *td0le_of(const fpnn_aes_engine *e) { return reinterpret_cast<const uint32_t *>(e->d_tables + 1280); }
const uint8_t *isbox_of(const fpnn_aes_engine *e) { return e->d_tables + 2304; }

// slots the table's allocations hold (a key set made by _create / _from_schedules has no
// capacity of its own until it grows)
uint32_t table_slots(const fpnn_aes_keyset *ks) { return std::max(ks->capacity, ks->count); }

// what dispatch_plan.hpp reads of the engine and of a batch
DispatchShape dispatch_shape(const fpnn_aes_engine *e) {
    return {scratch_shape(e), kThreads, kFrameMaxBytes, e->variant.hyb_long, e->variant.hyb_quad_waves,
            e->variant.hyb_force, length_bucket_of};
}
BatchShape batch_shape(const fpnn_aes_batch *b) {
    return {b->count, b->stride, b->uniform_len, b->max_len, b->flags, b->in_off != nullptr, b->out_off != nullptr,
            b->len != nullptr, b->key_slot != nullptr, b->keys->count, b->in == b->out};
}
static_assert(F_WIRE_PREFIX == FPNN_AES_F_WIRE_PREFIX, "the plan reads the public flag");

void free_deferred(fpnn_aes_engine *e) {  // the engine's stream is idle
    for (void *p : e->deferred) (void)hipFree(p);
    e->deferred.clear();
}

}  // namespace

// The engine's stream is idle: release grown-out scratch, and report (once) a consistency
// check a kernel failed since the last look (kernels.hpp, kFault*).
int fpnn_aes::stream_idle(fpnn_aes_engine *e) {
    free_deferred(e);
    const uint32_t f = e->h_fault ? __atomic_exchange_n(e->h_fault, 0u, __ATOMIC_ACQ_REL) : 0u;
    if (!f) return FPNN_AES_OK;
    if ((f & kFaultLengthOrder) && e->buckets.p)  // start the next ragged call from a zero block
        (void)hipMemsetAsync(e->buckets.p, 0, e->buckets.cap * sizeof(uint32_t), e->stream);
    g_last_error = (f & kFaultLookback)      ? "block map: a look-back gave up waiting for a tile (results of that call invalid)"
                   : (f & kFaultLengthOrder) ? "length order: bucket counts did not add up to the batch (results of that call invalid)"
                   : (f & kFaultFrameTable)  ? "first_frame: not non-decreasing from 0 to count (results of that call invalid)"
                   : (f & kFaultKeySlot)     ? "key table: a slot index at or past slot_bound (that entry was not written)"
                                             : "device-side check failed";
    return FPNN_AES_ERR_DEVICE;
}

namespace {

// (below, with the small-call server)
void batch_signal(fpnn_aes_engine *e);
void batch_queued(fpnn_aes_engine *e);
void register_engine(fpnn_aes_engine *e);
void unregister_engine(fpnn_aes_engine *e);

// batch_signal for the lifetime of a call: the pending flag that batch_signal sets (and
// batch_queued clears once the kernels are queued) is cleared on EVERY exit, so a call
// that returns an error between the two never leaves other engines' server relaunches
// spinning out their batch_fence bound
struct BatchScope {
    fpnn_aes_engine *e;
    explicit BatchScope(fpnn_aes_engine *eng) : e(eng) { batch_signal(e); }
    ~BatchScope();
    BatchScope(const BatchScope &) = delete;
    BatchScope &operator=(const BatchScope &) = delete;
};

int timing_begin(fpnn_aes_engine *e, int which, EventPair **pair) {
    *pair = nullptr;
    if (!e->timing) return FPNN_AES_OK;
    auto &v = e->ev[which];
    if (e->ev_used[which] == v.size()) {
        EventPair p;
        HIP_TRY(hipEventCreate(&p.beg));
        HIP_TRY(hipEventCreate(&p.end));
        v.push_back(p);
    }
    *pair = &v[e->ev_used[which]++];
    HIP_TRY(hipEventRecord((*pair)->beg, e->stream));
    return FPNN_AES_OK;
}

// after the main kernel of a call: close its timing pair, remember what was launched
int timing_end(fpnn_aes_engine *e, EventPair *pair, int which) {
    e->last_kernel[which] = last_launched();
    batch_queued(e);
    if (pair) HIP_TRY(hipEventRecord(pair->end, e->stream));
    return FPNN_AES_OK;
}

int check_batch(const fpnn_aes_engine *e, const fpnn_aes_batch *b) {
    if (!e || !b || !b->keys) return FPNN_AES_ERR_ARG;
    if (b->count && (!b->in || !b->out)) return FPNN_AES_ERR_ARG;
    if (b->keys->device != e->device) return FPNN_AES_ERR_ARG;
    if (b->keys->count == 0) return FPNN_AES_ERR_ARG;
    return FPNN_AES_OK;
}

// The device state arrays of a stream call with n streams: there and 16-byte aligned when
// n > 0.  pos4: pos_state on a 4-byte grid as well -- the *_frames calls ask that of a call
// with streams, the one-frame _at encrypt of every call, the plain stream calls never.
int check_stream_state(uint64_t n, const uint8_t *iv_state, const uint32_t *pos_state, bool pos4) {
    if (n && (!iv_state || !pos_state || ((uintptr_t)iv_state & 15))) return FPNN_AES_ERR_ARG;
    if (pos4 && ((uintptr_t)pos_state & 3)) return FPNN_AES_ERR_ARG;
    return FPNN_AES_OK;
}

KBatch make_kbatch(const fpnn_aes_engine *e, const fpnn_aes_batch *b, uint8_t *iv_state, uint32_t *pos_state) {
    KBatch k;
    memset(&k, 0, sizeof k);
    k.in = b->in;
    k.out = b->out;
    k.count = b->count;
    k.stride = b->stride;
    k.uniform_len = b->uniform_len;
    k.flags = b->flags;
    k.in_off = b->in_off;
    k.out_off = b->out_off;
    k.len = b->len;
    k.key_slot = b->key_slot;
    k.keys = b->keys->d_keys;
    k.iv_state = iv_state;
    k.pos_state = pos_state;
    k.t0le = t0le_of(e);
    k.eiv = b->keys->d_eiv;
    return k;
}

// DevKey of a host schedule (rijndael_context layout, big-endian rk words) and, where given,
// the slot's IV
void devkey_from_schedule(DevKey *hk, const fpnn_aes_schedule *ctx, const uint8_t *iv = nullptr) {
    memset(hk, 0, sizeof *hk);
    for (int k = 0; k < 4 * (ctx->nrounds + 1); k++) hk->rk[k] = bswap32(ctx->rk[k]);
    hk->nrounds = (uint32_t)ctx->nrounds;
    hk->keylen = (uint32_t)(ctx->nrounds - 6) * 4;
    if (iv) memcpy(hk->iv, iv, 16);
}

#ifdef FPNN_AES_BOUNDS
// ---- the address-audit build (audit.hpp, `make audit`) ----------------------------------
// One call's extent table, built on the host: set() names a buffer's bytes (a null buffer is
// not checked), publish() puts the table on the device once the stream is drained.
struct AuditExtents {
    AuditTable t;
    AuditExtents() { memset(&t, 0, sizeof t); }
    void set(AuditBuf i, const void *p, uint64_t bytes) {
        if (!p) return;
        t.lo[i] = (uint64_t)(uintptr_t)p;
        t.hi[i] = t.lo[i] + bytes;
    }
    int publish(fpnn_aes_engine *e, AuditTable **aud) {
        if (!e->d_aud) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->d_aud), sizeof(AuditTable)));
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipMemcpy(e->d_aud, &t, sizeof t, hipMemcpyHostToDevice));
        *aud = e->d_aud;
        return FPNN_AES_OK;
    }
};

// Before an encrypt call: the extents of every buffer the call's kernels may touch, in the
// engine's table (synchronous; the audit build is a checker, not a product).  The scratch
// the call grows is grown here first so that its extent is known.
// frames: a *_frames call -- first_frame[] is registered and the state arrays hold one entry
// per stream; with state_slot (the _at calls) slot_bound entries, and state_slot[] and the
// per-segment slot scratch are registered (the latter also as key_slot: K1r's view of it).
int audit_begin(fpnn_aes_engine *e, const fpnn_aes_batch *b, const uint8_t *iv_state, const uint32_t *pos_state,
                KBatch &k, const FrameTable *frames = nullptr, const UdpTable *udp = nullptr,
                const fpnn_aes_keyset *data_keys = nullptr, const UdpRecvTable *recv = nullptr) {
    const uint64_t n = b->count;
    if (int rc = scratch_ensure(e, need_encrypt_ragged(scratch_shape(e), n, true))) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));  // (the descriptor arrays are read below)
    AuditExtents x;
    x.set(AB_IN_OFF, b->in_off, 8 * n);
    x.set(AB_OUT_OFF, b->out_off, 8 * n);
    x.set(AB_LEN, b->len, 4 * n);
    x.set(AB_SLOT, b->key_slot, 4 * n);
    const uint64_t slots = std::max<uint64_t>(b->keys->count, b->keys->capacity);
    x.set(AB_KEYS, b->keys->d_keys, sizeof(DevKey) * slots);
    x.set(AB_EIV, b->keys->d_eiv, 16 * slots);
    const uint64_t nstate = !frames ? n : frames->state_slot ? frames->slot_bound : frames->nstreams;
    x.set(AB_IV_STATE, iv_state, 16 * nstate);
    x.set(AB_POS_STATE, pos_state, 4 * nstate);
    x.set(AB_POS_SNAP, pos_state, 4 * nstate);
    if (frames) x.set(AB_FIRST_FRAME, frames->first_frame, 4 * ((uint64_t)frames->nstreams + 1));
    if (frames && frames->state_slot) {
        x.set(AB_STATE_SLOT, frames->state_slot, 4 * (uint64_t)frames->nstreams);
        x.set(AB_SEG_SLOT, frames->seg_slot, 4 * n);
        x.set(AB_SLOT, frames->seg_slot, 4 * n);
    }
    if (udp) {  // the UDP calls: frames names first_dgram[] and conn_slot[]
        if (data_keys) x.set(AB_UDP_DATA_KEYS, udp->data_keys, sizeof(DevKey) * (uint64_t)table_slots(data_keys));
        x.set(AB_UDP_FIRST_SECTION, udp->first_section, 4 * (n + 1));
        x.set(AB_UDP_SEC_OFF, udp->sec_off, 4 * (uint64_t)udp->nsections);
        x.set(AB_UDP_SEC_LEN, udp->sec_len, 4 * (uint64_t)udp->nsections);
    }
    if (recv) {  // the UDP receive calls: the walk tables and the take lists
        x.set(AB_UDP_SCAN, recv->scan, sizeof(UdpScan) * n);
        x.set(AB_UDP_PKGS, recv->pkgs, sizeof(UdpPkg) * n * recv->max_pkgs);
        x.set(AB_UDP_SECTIONS, recv->sections, sizeof(UdpSection) * n * recv->max_sections);
        x.set(AB_UDP_FIRST_TAKE, recv->first_take, 4 * ((uint64_t)frames->nstreams + 1));
        x.set(AB_UDP_TAKE, recv->take, 4 * (uint64_t)recv->ntake);
    }
    x.set(AB_PERM, e->perm.p, 4 * n);
    x.set(AB_SINK, e->sink.p, 16 * e->sink.cap);
    x.set(AB_BLOCK, e->buckets.p, 4 * (uint64_t)kLengthOrderWords);
    // the payload: the union of the segments' byte ranges (the kernels also check each
    // access against its own segment)
    std::vector<uint64_t> io(n), oo(n);
    std::vector<uint32_t> ln(n);
    if (b->in_off) HIP_TRY(hipMemcpy(io.data(), b->in_off, 8 * n, hipMemcpyDeviceToHost));
    else for (uint64_t i = 0; i < n; i++) io[i] = i * b->stride;
    if (b->out_off) HIP_TRY(hipMemcpy(oo.data(), b->out_off, 8 * n, hipMemcpyDeviceToHost));
    else oo = io;
    if (b->len) HIP_TRY(hipMemcpy(ln.data(), b->len, 4 * n, hipMemcpyDeviceToHost));
    else std::fill(ln.begin(), ln.end(), b->uniform_len);
    const uint64_t wire = (b->flags & FPNN_AES_F_WIRE_PREFIX) ? 4 : 0;
    uint64_t ilo = UINT64_MAX, ihi = 0, olo = UINT64_MAX, ohi = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (ln[i]) {
            ilo = std::min(ilo, io[i]);
            ihi = std::max(ihi, io[i] + ln[i]);
        }
        if (ln[i] + wire) {
            olo = std::min(olo, oo[i]);
            ohi = std::max(ohi, oo[i] + ln[i] + wire);
        }
    }
    if (ihi) x.set(AB_IN, b->in + ilo, ihi - ilo);
    else x.set(AB_IN, b->in, 1);  // (nothing may be read)
    if (ohi) x.set(AB_OUT, b->out + olo, ohi - olo);
    else x.set(AB_OUT, b->out, 1);
    // (the audit's own test: an `out` extent this many bytes short must be reported)
    if (const char *v = getenv("FPNN_AES_AUDIT_SHRINK_OUT"))
        if (x.t.hi[AB_OUT] > x.t.lo[AB_OUT] + (uint64_t)atoll(v)) x.t.hi[AB_OUT] -= (uint64_t)atoll(v);
    return x.publish(e, &k.aud);
}

// a key-table or stream-state write (k_keytable.hip): the table and the caller's arrays
int audit_begin_keytable(fpnn_aes_engine *e, const fpnn_aes_keyset *ks, KeyTableArgs &a) {
    AuditExtents x;
    const uint64_t slots = table_slots(ks);
    x.set(AB_KEYS, a.keys, sizeof(DevKey) * slots);
    x.set(AB_EIV, a.eiv, 16 * slots);
    x.set(AB_KT_SLOTS, a.slots, 4 * (uint64_t)a.count);
    x.set(AB_KT_RAW, a.raw, (uint64_t)ks->keylen * a.count);
    x.set(AB_KT_IVS, a.ivs, 16 * (uint64_t)a.count);
    x.set(AB_KT_OK, a.ok, a.count);
    x.set(AB_IV_STATE, a.iv_state, 16 * (uint64_t)a.slot_bound);
    x.set(AB_POS_STATE, a.pos_state, 4 * (uint64_t)a.slot_bound);
    return x.publish(e, &a.aud);
}

const char *audit_buf_name(uint32_t i) {
    static const char *const names[kAuditBufs] = {"in", "out", "in_off", "out_off", "len", "key_slot", "keys", "eiv",
                                                  "iv_state", "pos_state", "perm", "sink", "length-order block",
                                                  "pos_snap", "in (outside its segment)", "out (outside its segment)",
                                                  "first_frame", "slots", "raw keys", "ivs", "ok", "state_slot",
                                                  "segment slots", "data keys", "first_section", "sec_off",
                                                  "sec_len", "scan", "pkgs", "sections", "first_take", "take"};
    return i < kAuditBufs ? names[i] : "?";
}

// After the call's kernels: wait, and report the first access outside its extent.
int audit_end(fpnn_aes_engine *e, int rc) {
    if (rc != FPNN_AES_OK || !e->d_aud) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    AuditTable t;
    HIP_TRY(hipMemcpy(&t, e->d_aud, sizeof t, hipMemcpyDeviceToHost));
    if (!t.hits) return FPNN_AES_OK;
    char buf[640];
    snprintf(buf, sizeof buf,
             "address audit: %u access(es) outside their extent; first: %s (%s) line %u, workgroup %u thread %u, "
             "bytes [0x%llx, +%llu) against [0x%llx, 0x%llx)",
             t.hits, last_launched(), audit_buf_name(t.buf), t.site, t.block, t.thread, (unsigned long long)t.addr,
             (unsigned long long)t.len, (unsigned long long)t.elo, (unsigned long long)t.ehi);
    g_last_error = buf;
    fprintf(stderr, "[fpnn_aes audit] %s\n", buf);
    return FPNN_AES_ERR_DEVICE;
}
#else  // the product build: no table, and audit_end(e, rc) is rc
inline int audit_begin(fpnn_aes_engine *, const fpnn_aes_batch *, const uint8_t *, const uint32_t *, KBatch &,
                       const FrameTable * = nullptr, const UdpTable * = nullptr, const fpnn_aes_keyset * = nullptr,
                       const UdpRecvTable * = nullptr) {
    return FPNN_AES_OK;
}
inline int audit_begin_keytable(fpnn_aes_engine *, const fpnn_aes_keyset *, KeyTableArgs &) { return FPNN_AES_OK; }
inline int audit_end(fpnn_aes_engine *, int rc) { return rc; }
#endif

// The slot addressing of an _at call (fpnn_aes_stream_encrypt_at / _decrypt_at,
// fpnn_aes_stream_*_frames_at, fpnn_aes_stream_recv_at): stream j's state AND key at
// state_slot[j], checked against slot_bound on the device.
// one_frame: no first_frame, stream j is segment j.
struct SlotAddr {
    const uint32_t *state_slot;
    uint32_t slot_bound;
    bool one_frame;
};

// what every _at call asks of its slot addressing: the slot names key and state, so there is no
// second key addressing, and the bound never grows the table
int check_slot_addr(const fpnn_aes_batch *b, uint64_t nstreams, const SlotAddr *at) {
    if (b->key_slot || ((uintptr_t)at->state_slot & 3) || (nstreams && !at->state_slot)) return FPNN_AES_ERR_ARG;
    if (at->slot_bound > table_slots(b->keys)) return FPNN_AES_ERR_ARG;
    return FPNN_AES_OK;
}

// at (fpnn_aes_stream_encrypt_at, stream mode): the route is the same, and its kernel runs in its
// slot form (KEY_SLOT, k_stream_at.hip).
int run_encrypt_calls(fpnn_aes_engine *e, const fpnn_aes_batch *b, uint8_t *iv_state, uint32_t *pos_state, bool stream,
                      const SlotAddr *at = nullptr) {
    int rc = check_batch(e, b);
    if (rc) return rc;
    if (stream && (rc = check_stream_state(b->count, iv_state, pos_state, at != nullptr))) return rc;
    if (at && (rc = check_slot_addr(b, b->count, at))) return rc;
    if (!stream && (b->flags & FPNN_AES_F_WIRE_PREFIX) && (b->out_off == nullptr && b->in == b->out))
        return FPNN_AES_ERR_ARG;  // the 4-byte prefix needs a distinct output layout
    if (!b->count) return FPNN_AES_OK;
    DeviceGuard g(e->device);
    const BatchScope batch_scope(e);  // (an early return clears the pending flag)
    const EncryptRoute r = encrypt_route(dispatch_shape(e), batch_shape(b), {stream, at != nullptr});
    // (everything that can fail is done before the length order is queued: its block is
    // left dirty until its last reader runs)
    if ((rc = scratch_ensure(e, r.need))) return rc;
    KBatch k = make_kbatch(e, b, iv_state, pos_state);
    if (at) {
        k.state_slot = at->state_slot;
        k.slot_bound = at->slot_bound;
        k.slot_fault = e->d_fault;
        // (the audit build: state arrays of slot_bound entries, state_slot[] of count)
        const FrameTable f{nullptr, (uint32_t)b->count, at->slot_bound, e->d_fault, at->state_slot, nullptr};
        if ((rc = audit_begin(e, b, iv_state, pos_state, k, &f))) return rc;
    } else if ((rc = audit_begin(e, b, iv_state, pos_state, k))) {
        return rc;
    }
    uint32_t *block = nullptr;  // the length-order block (ragged batches)
    if (r.order) {
        if (r.order_pos) k.pos_snap = pos_state;  // bucket sizes read it (the encrypt kernel reads it later)
        block = e->buckets.p;
        if (e->variant.poison_order > 0) {  // (tests) bucket counts left over as if by a lost call
            e->variant.poison_order--;
            HIP_TRY(hipMemsetAsync(block, 0x01, kWireFlagWord / 2 * sizeof(uint32_t), e->stream));
        }
        HIP_TRY(launch_length_order(k, r.order_pos, e->perm.p, block, r.order_zeroes, e->d_fault, e->stream));
        k.perm = e->perm.p;
    }
    k.flags |= r.flags;  // (the cipher kernel's alone: the length order has read k without them)
    EventPair *ev;
    if ((rc = timing_begin(e, FPNN_AES_K_ENCRYPT, &ev))) {
        if (block) (void)hipMemsetAsync(block, 0, kLengthOrderWords * sizeof(uint32_t), e->stream);
        return rc;
    }
    const int nr = b->keys->nrounds;
    switch (r.family) {
    case ENC_HYBRID: {
        const HybridArgs h{block + kTicketWords, block, r.long_bucket, r.quad_waves, e->sink.p};
        if (at) HIP_TRY(launch_encrypt_hybrid_at(k, h, nr, r.grid, e->stream));
        else HIP_TRY(launch_encrypt_hybrid(k, h, nr, r.km, stream, r.grid, e->stream));
        break;
    }
    case ENC_COOP:
        if (at) HIP_TRY(launch_encrypt_coop_at(k, nr, r.layout, r.grid, r.threads, e->stream));
        else HIP_TRY(launch_encrypt_coop(k, nr, r.layout, r.km, stream, r.grid, r.threads, e->stream));
        break;
    case ENC_FRAMES:
        HIP_TRY(launch_encrypt_frames(k, nr, r.km, r.wire, r.grid, e->stream));
        break;
    case ENC_CHAINS:
        if (at) HIP_TRY(launch_encrypt_chains_at(k, nr, r.layout, r.grid, r.threads, e->stream));
        else HIP_TRY(launch_encrypt_chains(k, nr, r.layout, r.km, stream, r.grid, r.threads, e->stream));
        break;
    }
    return timing_end(e, ev, FPNN_AES_K_ENCRYPT);
}

int run_encrypt(fpnn_aes_engine *e, const fpnn_aes_batch *b, uint8_t *iv_state, uint32_t *pos_state, bool stream,
                const SlotAddr *at = nullptr) {
    return audit_end(e, run_encrypt_calls(e, b, iv_state, pos_state, stream, at));
}

struct SnapCopy {  // what the single-workgroup block map's state copy reads and writes (stream batches)
    const uint8_t *iv_from = nullptr;
    const uint32_t *pos_from = nullptr;
    uint4 *iv_to = nullptr;
    uint32_t *pos_to = nullptr;
};

// K1r on the batch k describes: block-map scan, per-wave plan and decrypt all on the device;
// the host never learns the block total, so nothing here waits for the GPU.  What can fail
// has come first: the caller has grown the scratch of its route.  before(small_map, snap)
// queues what the caller runs ahead of the block map (state snapshot or pre-pass), points k
// at it and says what a small (single-workgroup) block map copies as its snapshot.
template <class Before>
int decrypt_ragged(fpnn_aes_engine *e, const fpnn_aes_batch *b, KBatch &k, bool stream, KeyMode km, Before before) {
    const bool small_map = b->count <= block_map_small_max();
    SnapCopy snap;
    if (int rc = before(small_map, snap)) return rc;
    if (small_map)
        HIP_TRY(launch_block_map_small(k, stream, snap.iv_from, snap.pos_from, snap.iv_to, snap.pos_to, e->bstart.p,
                                       e->d_total, e->stream));
    else  // (its look-back words: zeros when grown, zeroed again by the kernel's last reader)
        HIP_TRY(launch_block_map_onepass(k, stream, e->bstart.p, e->lookback.p, e->lookback.cap, e->d_fault,
                                         e->d_total, e->stream));
    k.bstart = e->bstart.p;
    if (!k.in_off || !k.len) {  // K1r reads descriptor arrays: materialize the missing ones
        HIP_TRY(launch_ragged_desc(b->count, b->stride, b->uniform_len, k.in_off ? nullptr : e->desc_off.p,
                                   k.len ? nullptr : e->desc_len.p, e->stream));
        if (!k.in_off) k.in_off = e->desc_off.p;
        if (!k.len) k.len = e->desc_len.p;
    }
    if (!k.out_off) k.out_off = k.in_off;
    k.runs = (uint32_t)e->variant.k1r_runs;
    EventPair *ev = nullptr;
    if (int rc = timing_begin(e, FPNN_AES_K_DECRYPT, &ev)) return rc;
    // in place (in == out, identical offsets: fpnn_aes.h) the predecessor blocks of the
    // waves' first chunks are saved by a plan launch before any wave writes; otherwise
    // every wave finds its own at the start of the decrypt kernel (one launch fewer)
    HIP_TRY(launch_decrypt_ragged(k, b->keys->nrounds, km, stream, e->plan.p, e->sink.p, b->in == b->out, e->num_cus,
                                  e->stream));
    return timing_end(e, ev, FPNN_AES_K_DECRYPT);
}

int run_decrypt(fpnn_aes_engine *e, const fpnn_aes_batch *b, uint8_t *iv_state, uint32_t *pos_state, bool stream) {
    int rc = check_batch(e, b);
    if (rc) return rc;
    if (stream && (rc = check_stream_state(b->count, iv_state, pos_state, false))) return rc;
    if (b->flags & FPNN_AES_F_WIRE_PREFIX) return FPNN_AES_ERR_ARG;
    if (!b->count) return FPNN_AES_OK;
    DeviceGuard g(e->device);
    const BatchScope batch_scope(e);  // (an early return clears the pending flag)
    const DecryptRoute r = decrypt_route(dispatch_shape(e), batch_shape(b), {stream, false});
    if ((rc = scratch_ensure(e, r.need))) return rc;
    KBatch k = make_kbatch(e, b, iv_state, pos_state);
    EventPair *ev = nullptr;
    switch (r.family) {
    case DEC_RAGGED:  // stream batches (which always come here) snapshot their state first
        return decrypt_ragged(e, b, k, stream, r.km, [&](bool small_map, SnapCopy &snap) {
            if (!stream) return (int)FPNN_AES_OK;
            const uint64_t n = b->count;
            if (!small_map) {  // (the small block map copies the snapshot itself)
                HIP_TRY(hipMemcpyAsync(e->snap_iv.p, iv_state, 16ull * n, hipMemcpyDeviceToDevice, e->stream));
                HIP_TRY(hipMemcpyAsync(e->snap_pos.p, pos_state, 4ull * n, hipMemcpyDeviceToDevice, e->stream));
            }
            k.iv_snap = e->snap_iv.p;  // see KBatch::iv_snap
            k.pos_snap = e->snap_pos.p;
            snap = {iv_state, pos_state, e->snap_iv.p, e->snap_pos.p};
            return (int)FPNN_AES_OK;
        });
    case DEC_FRAMES:
        if ((rc = timing_begin(e, FPNN_AES_K_DECRYPT, &ev))) return rc;
        HIP_TRY(launch_decrypt_frames(k, b->keys->nrounds, r.km, r.grid, e->stream));
        break;
    case DEC_DENSE:
        k.total_blocks = r.total_blocks;
        k.nb_uniform = r.nb_uniform;
        k.magic = r.magic;
        if (r.boundary_save) {
            HIP_TRY(launch_boundary_save(k, e->boundary.p, r.nchunks, e->stream));
            k.boundary = e->boundary.p;
        }
        if ((rc = timing_begin(e, FPNN_AES_K_DECRYPT, &ev))) return rc;
        HIP_TRY(launch_decrypt_blocks(k, b->keys->nrounds, r.layout, r.km, r.boundary_save, r.grid, e->stream));
        break;
    }
    return timing_end(e, ev, FPNN_AES_K_DECRYPT);
}

// ---- many frames per stream in one call (fpnn_aes_stream_*_frames, k_stream_frames.hip) ----

int check_frames(const fpnn_aes_engine *e, const fpnn_aes_batch *b, const uint32_t *first_frame, uint32_t nstreams,
                 const uint8_t *iv_state, const uint32_t *pos_state, const SlotAddr *at) {
    const int rc = check_batch(e, b);
    if (rc) return rc;
    if (b->flags & FPNN_AES_F_WIRE_PREFIX) return FPNN_AES_ERR_ARG;
    if (int src = check_stream_state(nstreams, iv_state, pos_state, nstreams != 0)) return src;
    const bool need_first = !(at && at->one_frame);
    if (nstreams && ((need_first && !first_frame) || ((uintptr_t)first_frame & 3))) return FPNN_AES_ERR_ARG;
    if (at) return check_slot_addr(b, nstreams, at);
    return FPNN_AES_OK;
}

FrameTable frame_table(fpnn_aes_engine *e, const uint32_t *first_frame, uint32_t nstreams, const SlotAddr *at) {
    FrameTable f{first_frame, nstreams, 0u, e->d_fault, nullptr, nullptr};
    if (at) {
        f.state_slot = at->state_slot;
        f.slot_bound = at->slot_bound;
    }
    return f;
}

// Encrypt: K2f, one quad per stream, sized as K2c is (by quads needed, at most one workgroup
// per CU; further streams grid-stride).  Streams are visited in index order: no length order.
int run_encrypt_frames_calls(fpnn_aes_engine *e, const fpnn_aes_batch *b, const uint32_t *first_frame,
                             uint32_t nstreams, uint8_t *iv_state, uint32_t *pos_state, const SlotAddr *at) {
    int rc = check_frames(e, b, first_frame, nstreams, iv_state, pos_state, at);
    if (rc) return rc;
    if (!nstreams || !b->count) return FPNN_AES_OK;
    DeviceGuard g(e->device);
    const BatchScope batch_scope(e);  // (an early return clears the pending flag)
    KBatch k = make_kbatch(e, b, iv_state, pos_state);
    const FrameTable f = frame_table(e, first_frame, nstreams, at);
    if ((rc = audit_begin(e, b, iv_state, pos_state, k, &f))) return rc;
    const FramesRoute r = frames_route(dispatch_shape(e), batch_shape(b), at != nullptr, nstreams, true);
    EventPair *ev;
    if ((rc = timing_begin(e, FPNN_AES_K_ENCRYPT, &ev))) return rc;
    HIP_TRY(launch_encrypt_stream_frames(k, f, b->keys->nrounds, r.km, r.grid, r.threads, e->stream));
    return timing_end(e, ev, FPNN_AES_K_ENCRYPT);
}

// Decrypt: the state pre-pass fills K1r's per-segment snapshot, K1r decrypts every block in
// parallel and exports each segment's outgoing state into per-segment scratch, the commit
// gives every stream its last non-empty frame's.  The caller's state arrays are read by
// the pre-pass and K1r's plan only through the snapshot, and written by the commit alone.
int run_decrypt_frames_calls(fpnn_aes_engine *e, const fpnn_aes_batch *b, const uint32_t *first_frame,
                             uint32_t nstreams, uint8_t *iv_state, uint32_t *pos_state, const SlotAddr *at) {
    int rc = check_frames(e, b, first_frame, nstreams, iv_state, pos_state, at);
    if (rc) return rc;
    if (!nstreams || !b->count) return FPNN_AES_OK;
    DeviceGuard g(e->device);
    const BatchScope batch_scope(e);
    const FramesRoute r = frames_route(dispatch_shape(e), batch_shape(b), at != nullptr, nstreams, false);
    if ((rc = scratch_ensure(e, r.need))) return rc;
    KBatch k = make_kbatch(e, b, iv_state, pos_state);
    FrameTable f = frame_table(e, first_frame, nstreams, at);
    const KeyMode km = r.km;
    rc = decrypt_ragged(
        e, b, k, true, km,
        [&](bool, SnapCopy &snap) {
            if (at) {  // the walk writes every segment's key slot; the pre-pass's second launch and K1r read it
                f.seg_slot = e->sf_slot.p;
                k.key_slot = e->sf_slot.p;
            }
            if (int arc = audit_begin(e, b, iv_state, pos_state, k, &f)) return arc;
            // the pre-pass reads the ciphertext and the incoming state: before the block map (whose
            // block counts read pos_snap) and before any in-place write
            HIP_TRY(launch_stream_frames_state(k, f, b->keys->nrounds, km, e->snap_iv.p, e->snap_pos.p, e->sf_stream.p,
                                               e->sf_prev.p, e->num_cus, e->stream));
            k.iv_snap = e->snap_iv.p;
            k.pos_snap = e->snap_pos.p;
            // from here on "the state" is per segment: K1r exports into the scratch
            k.iv_state = reinterpret_cast<uint8_t *>(e->sf_iv.p);
            k.pos_state = e->sf_pos.p;
            // (a small block map's snapshot copy goes from the pre-pass's snapshot into the export
            // scratch, which K1r overwrites: the snapshot itself stays as the pre-pass wrote it)
            snap = {reinterpret_cast<const uint8_t *>(e->snap_iv.p), e->snap_pos.p, e->sf_iv.p, e->sf_pos.p};
            return (int)FPNN_AES_OK;
        });
    if (rc) return rc;
    k.iv_state = iv_state;
    k.pos_state = pos_state;
    k.len = b->len;  // (as the caller gave it: uniform_len otherwise)
    HIP_TRY(launch_stream_frames_commit(k, f, e->sf_iv.p, e->sf_pos.p, e->stream));
    batch_queued(e);  // (the call's batch work ends behind the commit)
    return FPNN_AES_OK;
}

int run_frames(fpnn_aes_engine *e, const fpnn_aes_batch *b, const uint32_t *first_frame, uint32_t nstreams,
               uint8_t *iv_state, uint32_t *pos_state, bool encrypt, const SlotAddr *at = nullptr) {
    return audit_end(e, encrypt ? run_encrypt_frames_calls(e, b, first_frame, nstreams, iv_state, pos_state, at)
                                : run_decrypt_frames_calls(e, b, first_frame, nstreams, iv_state, pos_state, at));
}

// ---- UDP v2 datagrams with data encryption (fpnn_aes_udp_encrypt / _decrypt, k_udp.hip) ----

static_assert(UDP_ARGS_KEYLEN == FPNN_AES_ERR_KEYLEN && UDP_ARGS_BAD == FPNN_AES_ERR_ARG, "udp_check_args returns public errors");

UdpArgs udp_args(const fpnn_aes_engine *e, const fpnn_aes_batch *b, const fpnn_aes_udp_data *u) {
    UdpArgs a = {};
    a.key_slot = b->key_slot != nullptr;
    a.flags = b->flags;
    a.u = u != nullptr;
    a.pkg_slots = table_slots(b->keys);
    a.nr_pkg = b->keys->nrounds;
    if (u) {
        a.data_keys = u->data_keys != nullptr;
        if (u->data_keys) {
            a.data_keys_same_engine = u->data_keys->e == e && u->data_keys->device == e->device;
            a.data_slots = table_slots(u->data_keys);
            a.nr_data = u->data_keys->nrounds;
        }
        a.nconn = u->nconn;
        a.nsections = u->nsections;
        a.slot_bound = u->slot_bound;
        a.first_dgram = (uintptr_t)u->first_dgram;
        a.conn_slot = (uintptr_t)u->conn_slot;
        a.iv_state = (uintptr_t)u->iv_state;
        a.pos_state = (uintptr_t)u->pos_state;
        a.first_section = (uintptr_t)u->first_section;
        a.sec_off = (uintptr_t)u->sec_off;
        a.sec_len = (uintptr_t)u->sec_len;
    }
    return a;
}

int check_udp(const fpnn_aes_engine *e, const fpnn_aes_batch *b, const fpnn_aes_udp_data *u) {
    if (int rc = check_batch(e, b)) return rc;
    return udp_check_args(udp_args(e, b, u));
}

UdpTable udp_table(fpnn_aes_engine *e, const fpnn_aes_udp_data *u) {
    return {u->data_keys ? u->data_keys->d_keys : nullptr, u->first_dgram, u->conn_slot, u->first_section, u->sec_off,
            u->sec_len, u->nconn, u->slot_bound, u->nsections, 0u, e->d_fault};
}

UdpShape udp_shape(const fpnn_aes_batch *b, const fpnn_aes_udp_data *u) {
    return {u->nconn, u->nsections, u->data_keys ? u->data_keys->nrounds : 0, b->keys->nrounds};
}

// Encrypt: K2u, one launch.
int run_udp_encrypt_calls(fpnn_aes_engine *e, const fpnn_aes_batch *b, const fpnn_aes_udp_data *u) {
    int rc = check_udp(e, b, u);
    if (rc) return rc;
    if (!u->nconn || !b->count) return FPNN_AES_OK;
    DeviceGuard g(e->device);
    const BatchScope batch_scope(e);  // (an early return clears the pending flag)
    const UdpRoute r = udp_route(dispatch_shape(e), batch_shape(b), udp_shape(b, u), true);
    if (!r.ok) return FPNN_AES_ERR_KEYLEN;
    KBatch k = make_kbatch(e, b, u->iv_state, u->pos_state);
    const UdpTable t = udp_table(e, u);
    const FrameTable f{u->first_dgram, u->nconn, u->slot_bound, e->d_fault, u->conn_slot, nullptr};
    if ((rc = audit_begin(e, b, u->iv_state, u->pos_state, k, &f, &t, u->data_keys))) return rc;
    EventPair *ev;
    if ((rc = timing_begin(e, FPNN_AES_K_ENCRYPT, &ev))) return rc;
    HIP_TRY(launch_udp_encrypt(k, t, r.nr_data, r.nr_pkg, r.grid, r.threads, e->stream));
    return timing_end(e, ev, FPNN_AES_K_ENCRYPT);
}

// Decrypt: both layers parallelise by block, so the call derives the descriptors the existing
// kernels take (k_udp_expand, into scratch no other kernel of the call uses) and queues them in
// order: the package decrypt of the datagrams in -> out with one key slot per datagram (K1k /
// K1r / D2s by the dispatch plan), then the slot-addressed *_frames decrypt of the sections in
// place in `out` under the data table (state pre-pass, K1r, commit).  The two steps share the
// K1r scratch one after the other on the stream; its zeroed buffers are returned to zeros by
// each step's own last reader.
int run_udp_decrypt_calls(fpnn_aes_engine *e, const fpnn_aes_batch *b, const fpnn_aes_udp_data *u) {
    int rc = check_udp(e, b, u);
    if (rc) return rc;
    if (!u->nconn || !b->count) return FPNN_AES_OK;
    DeviceGuard g(e->device);
    const UdpRoute r = udp_route(dispatch_shape(e), batch_shape(b), udp_shape(b, u), false);
    if (!r.ok) return FPNN_AES_ERR_KEYLEN;
    if ((rc = scratch_ensure(e, r.need))) return rc;
    uint32_t *const dg_slot = e->udp_u32.p, *const sec_n = dg_slot + b->count, *const conn_sec = sec_n + u->nsections;
    {
        const BatchScope batch_scope(e);
        const KBatch k = make_kbatch(e, b, u->iv_state, u->pos_state);
        HIP_TRY(launch_udp_expand(k, udp_table(e, u), dg_slot, e->udp_off.p, sec_n, conn_sec, e->num_cus, e->stream));
        batch_queued(e);
    }
    fpnn_aes_batch pb = *b;  // the datagrams, each under its connection's slot
    pb.key_slot = dg_slot;
    if ((rc = run_decrypt(e, &pb, nullptr, nullptr, false))) return rc;
    if (!u->nsections) return FPNN_AES_OK;
    fpnn_aes_batch sb;  // the sections: segments of `out`, in place
    memset(&sb, 0, sizeof sb);
    sb.in = sb.out = b->out;
    sb.count = u->nsections;
    sb.in_off = e->udp_off.p;
    sb.len = sec_n;
    sb.keys = u->data_keys;
    const SlotAddr at{u->conn_slot, u->slot_bound, false};
    return run_decrypt_frames_calls(e, &sb, conn_sec, u->nconn, u->iv_state, u->pos_state, &at);
}

// ---- UDP v2 receive (fpnn_aes_udp_recv / _recv_take, k_udp_recv.hip) ----

static_assert(sizeof(UdpScan) == sizeof(fpnn_aes_udp_scan) && sizeof(UdpPkg) == sizeof(fpnn_aes_udp_pkg) &&
                  sizeof(UdpSection) == sizeof(fpnn_aes_udp_section) && sizeof(UdpScan) == 8 && sizeof(UdpPkg) == 16 &&
                  sizeof(UdpSection) == 16,
              "the walk tables are the public structs");
static_assert(UDP_F_WALK_ONLY == FPNN_AES_UDP_F_WALK_ONLY && UDP_F_PLAIN == FPNN_AES_UDP_F_PLAIN &&
                  UDP_SHORT == FPNN_AES_UDP_SHORT && UDP_VERSION == FPNN_AES_UDP_VERSION && UDP_TYPE == FPNN_AES_UDP_TYPE &&
                  UDP_ACKS == FPNN_AES_UDP_ACKS && UDP_CLOSE == FPNN_AES_UDP_CLOSE && UDP_FULL == FPNN_AES_UDP_FULL &&
                  UDP_LONG == FPNN_AES_UDP_LONG,
              "the plan's and the kernels' values are the public ones");

// The receive calls: recv = [datagram key slots (k_udp_expand over no sections), package decrypt]
// unless PLAIN, the walk, and unless WALK_ONLY [k_udp_take over every package, the *_frames_at
// decrypt of its segments]; recv_take = the bracketed data step alone over the take lists.  The
// scratch and its layout are run_udp_decrypt_calls', with max_sections segments per datagram or
// taken package in place of the caller's sections.
int run_udp_recv_calls(fpnn_aes_engine *e, const fpnn_aes_batch *b, const fpnn_aes_udp_data *u, bool take,
                       uint32_t flags, uint32_t max_pkgs, uint32_t max_sections, const fpnn_aes_udp_scan *scan,
                       const fpnn_aes_udp_pkg *pkgs, const fpnn_aes_udp_section *sections, const uint32_t *first_take,
                       const uint32_t *take_list, uint32_t ntake) {
    if (int rc = check_batch(e, b)) return rc;
    UdpRecvArgs a = {};
    a.udp = udp_args(e, b, u);
    a.take = take;
    a.flags = flags;
    a.in_place = b->in == b->out && !b->out_off;
    a.count = b->count;
    a.max_pkgs = max_pkgs;
    a.max_sections = max_sections;
    a.ntake = ntake;
    a.scan = (uintptr_t)scan;
    a.pkgs = (uintptr_t)pkgs;
    a.sections = (uintptr_t)sections;
    a.first_take = (uintptr_t)first_take;
    a.take_list = (uintptr_t)take_list;
    int rc = udp_recv_check_args(a);
    if (rc) return rc;
    if (!u->nconn || !b->count || (take && !ntake)) return FPNN_AES_OK;
    DeviceGuard g(e->device);
    const UdpRecvRoute r = udp_recv_route(dispatch_shape(e), batch_shape(b), udp_shape(b, u), take, flags, max_sections, ntake);
    if (!r.ok) return FPNN_AES_ERR_KEYLEN;
    if ((rc = scratch_ensure(e, r.need))) return rc;
    const uint64_t ndg = r.package ? b->count : 0;
    uint32_t *const dg_slot = e->udp_u32.p, *const sec_n = dg_slot + ndg, *const conn_sec = sec_n + r.nseg;
    const UdpTable t = udp_table(e, u);
    const UdpRecvTable rt{const_cast<UdpScan *>(reinterpret_cast<const UdpScan *>(scan)),
                          const_cast<UdpPkg *>(reinterpret_cast<const UdpPkg *>(pkgs)),
                          const_cast<UdpSection *>(reinterpret_cast<const UdpSection *>(sections)),
                          max_pkgs, max_sections, take ? first_take : nullptr, take ? take_list : nullptr,
                          take ? ntake : 0u, 0u};
    const FrameTable f{u->first_dgram, u->nconn, u->slot_bound, e->d_fault, u->conn_slot, nullptr};
    if (r.package) {
        {
            const BatchScope batch_scope(e);
            const KBatch k = make_kbatch(e, b, u->iv_state, u->pos_state);
            HIP_TRY(launch_udp_expand(k, t, dg_slot, e->udp_off.p, sec_n, conn_sec, e->num_cus, e->stream));
            batch_queued(e);
        }
        fpnn_aes_batch pb = *b;  // the datagrams, each under its connection's slot
        pb.key_slot = dg_slot;
        if ((rc = run_decrypt(e, &pb, nullptr, nullptr, false))) return rc;
    }
    if (!take) {  // (the walk reads the datagrams where the package layer left them: in `out`)
        const BatchScope batch_scope(e);
        KBatch k = make_kbatch(e, b, u->iv_state, u->pos_state);
        if ((rc = audit_begin(e, b, u->iv_state, u->pos_state, k, &f, &t, u->data_keys, &rt))) return rc;
        HIP_TRY(launch_udp_walk(k, rt, e->num_cus, e->stream));
        batch_queued(e);
        if ((rc = audit_end(e, FPNN_AES_OK))) return rc;
    }
    if (!r.data) return FPNN_AES_OK;
    {
        const BatchScope batch_scope(e);
        KBatch k = make_kbatch(e, b, u->iv_state, u->pos_state);
        if ((rc = audit_begin(e, b, u->iv_state, u->pos_state, k, &f, &t, u->data_keys, &rt))) return rc;
        HIP_TRY(launch_udp_take(k, t, rt, e->udp_off.p, sec_n, conn_sec, e->num_cus, e->stream));
        batch_queued(e);
        if ((rc = audit_end(e, FPNN_AES_OK))) return rc;
    }
    fpnn_aes_batch sb;  // the segments: pieces of `out`, in place
    memset(&sb, 0, sizeof sb);
    sb.in = sb.out = b->out;
    sb.count = (uint32_t)r.nseg;
    sb.in_off = e->udp_off.p;
    sb.len = sec_n;
    sb.keys = u->data_keys;
    const SlotAddr at{u->conn_slot, u->slot_bound, false};
    return run_decrypt_frames_calls(e, &sb, conn_sec, u->nconn, u->iv_state, u->pos_state, &at);
}

}  // namespace

int fpnn_aes::run_batch(fpnn_aes_engine *e, bool encrypt, const fpnn_aes_batch *b, uint8_t *iv_state,
                        uint32_t *pos_state, bool stream) {
    return encrypt ? run_encrypt(e, b, iv_state, pos_state, stream) : run_decrypt(e, b, iv_state, pos_state, stream);
}

// One frame per stream by key-table slot (fpnn_aes_stream_encrypt_at / _decrypt_at).  Encrypt:
// run_encrypt's stream dispatch, the kernel in its slot form.  Decrypt: the slot-addressed
// *_frames path with a null frame table -- stream j is segment j -- as fpnn_aes_stream_recv_at.
int fpnn_aes::run_batch_at(fpnn_aes_engine *e, bool encrypt, const fpnn_aes_batch *b, const uint32_t *state_slot,
                           uint32_t slot_bound, uint8_t *iv_state, uint32_t *pos_state) {
    if (b && (b->flags & FPNN_AES_F_WIRE_PREFIX)) return FPNN_AES_ERR_ARG;
    const SlotAddr at{state_slot, slot_bound, true};
    if (encrypt) return run_encrypt(e, b, iv_state, pos_state, true, &at);
    if (!b) return FPNN_AES_ERR_ARG;
    return run_frames(e, b, nullptr, b->count, iv_state, pos_state, false, &at);
}

// ===========================================================================
// C-ABI

extern "C" {

// (fpnn_aes_strerror lives in the front library, front.cpp: it must work without this one)

const char *fpnn_aes_last_error(void) { return g_last_error.c_str(); }

const char *fpnn_aes_version(void) {
    return "fpnn_aes 0.4 (gfx950; T-tables 32-way replicated in LDS; v_perm addressing; "
           "decrypt: K1d dense/keyed, K1k lane keys, K1r ragged (no host sync; interior runs), K1 uniform, "
           "one lane per block; encrypt: K2 lane per chain, K2c quad per chain, K2h lanes + quads for ragged "
           "batches, K2f quad per stream over many frames per call (stream_encrypt_frames; stream_decrypt_frames: "
           "state pre-pass + K1r); single calls <= 16 KiB: K0s resident server (K0 per launch); "
           "ECDH: one lane per derivation, special-prime folds as carry chains; "
           "live key table: keyset_set_keys / keyset_clear / ecdh_accept, one lane per slot, queued; "
           "stream state by slot: stream_open / stream_close, stream_*_frames_at, stream_recv_at, "
           "stream_encrypt_at / stream_decrypt_at (K2 / K2c / K2h slot forms), stream_host_at)";
}

int fpnn_aes_setup_encrypt(fpnn_aes_schedule *ctx, const uint8_t *key, size_t keylen) {
    if (!ctx || !key) return FPNN_AES_ERR_ARG;
    const int nr = expand_key_be(ctx->rk, key, keylen);
    ctx->nrounds = nr;
    return nr ? FPNN_AES_OK : FPNN_AES_ERR_KEYLEN;
}

int fpnn_aes_setup_decrypt(fpnn_aes_schedule *ctx, const uint8_t *key, size_t keylen) {
    if (!ctx || !key) return FPNN_AES_ERR_ARG;
    const int nr = expand_key_dec_be(ctx->rk, key, keylen);
    ctx->nrounds = nr;
    return nr ? FPNN_AES_OK : FPNN_AES_ERR_KEYLEN;
}

int fpnn_aes_device_count(int *count) {
    if (!count) return FPNN_AES_ERR_ARG;
    int n = 0;
    hipError_t err = hipGetDeviceCount(&n);
    if (err != hipSuccess) {
        *count = 0;
        hip_fail(err, "hipGetDeviceCount");
        return FPNN_AES_ERR_NODEV;
    }
    *count = n;
    return FPNN_AES_OK;
}

int fpnn_aes_engine_create(int device, void *hip_stream, fpnn_aes_engine **out) {
    if (!out) return FPNN_AES_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) {
        g_last_error = "no HIP device with that index";
        return FPNN_AES_ERR_NODEV;
    }
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_last_error = std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950";
        return FPNN_AES_ERR_NODEV;
    }
    DeviceGuard g(device);
    fpnn_aes_engine *e = new fpnn_aes_engine();
    e->device = device;
    e->num_cus = prop.multiProcessorCount;
    {  // the GPU's NUMA node: pinned arenas and copy threads go there (numa_place.hpp)
        char bdf[64] = {0};
        e->numa = fpnn_aes::numa_placement(hipDeviceGetPCIBusId(bdf, sizeof bdf, device) == hipSuccess ? bdf : nullptr);
    }
    // K2h split (tests set these so that small batches exercise each session)
    if (const char *v = getenv("FPNN_AES_HYB_LONG")) e->variant.hyb_long = std::max(1, atoi(v));
    if (const char *v = getenv("FPNN_AES_HYB_QW")) e->variant.hyb_quad_waves = std::min(16, std::max(0, atoi(v)));
    if (const char *v = getenv("FPNN_AES_HYB_FORCE")) e->variant.hyb_force = atoi(v) != 0;
    if (const char *v = getenv("FPNN_AES_DEBUG_POISON_ORDER")) e->variant.poison_order = std::max(0, atoi(v));
    if (const char *v = getenv("FPNN_AES_K1R_RUNS")) e->variant.k1r_runs = atoi(v) != 0;
    {  // stream-ordered scratch allocation from a pool of the engine's own: it keeps freed
       // memory for reuse (release threshold: never) without changing the device's
       // default pool, which other code in the process allocates from
        int pools = 0;
        const char *v = getenv("FPNN_AES_POOLS");
        if ((!v || atoi(v) != 0) &&
            hipDeviceGetAttribute(&pools, hipDeviceAttributeMemoryPoolsSupported, device) == hipSuccess && pools) {
            hipMemPoolProps props;
            memset(&props, 0, sizeof props);
            props.allocType = hipMemAllocationTypePinned;
            props.handleTypes = hipMemHandleTypeNone;
            props.location.type = hipMemLocationTypeDevice;
            props.location.id = device;
            if (hipMemPoolCreate(&e->mpool, &props) == hipSuccess) {
                uint64_t keep = UINT64_MAX;
                (void)hipMemPoolSetAttribute(e->mpool, hipMemPoolAttrReleaseThreshold, &keep);
                e->pools = true;
            } else {
                (void)hipGetLastError();
                e->mpool = nullptr;
            }
        }
    }
    int rc = FPNN_AES_OK;
    do {
        if (hip_stream != FPNN_AES_OWN_STREAM) {
            e->stream = (hipStream_t)hip_stream;  // NULL: the null stream
        } else {
            hipError_t err = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
            if (err != hipSuccess) { rc = hip_fail(err, "hipStreamCreate"); break; }
            e->own_stream = true;
        }
        hipError_t err = hipMalloc(reinterpret_cast<void **>(&e->d_tables), 2 * (1024 + 256));
        if (err != hipSuccess) { rc = hip_fail(err, "hipMalloc(tables)"); break; }
        err = hipMemcpy(e->d_tables, kTables.t0le, 1024, hipMemcpyHostToDevice);
        if (err == hipSuccess) err = hipMemcpy(e->d_tables + 1024, kTables.sbox, 256, hipMemcpyHostToDevice);
        if (err == hipSuccess) err = hipMemcpy(e->d_tables + 1280, kTables.td0le, 1024, hipMemcpyHostToDevice);
        if (err == hipSuccess) err = hipMemcpy(e->d_tables + 2304, kTables.isbox, 256, hipMemcpyHostToDevice);
        if (err != hipSuccess) { rc = hip_fail(err, "hipMemcpy(tables)"); break; }
        err = hipMalloc(reinterpret_cast<void **>(&e->d_total), sizeof(uint64_t));
        if (err != hipSuccess) { rc = hip_fail(err, "hipMalloc(total)"); break; }
        err = hipHostMalloc(reinterpret_cast<void **>(&e->h_fault), 64, hipHostMallocCoherent);
        if (err == hipSuccess) {
            *e->h_fault = 0;
            err = hipHostGetDevicePointer(reinterpret_cast<void **>(&e->d_fault), e->h_fault, 0);
        }
        if (err != hipSuccess) { rc = hip_fail(err, "hipHostMalloc(fault)"); break; }
    } while (0);
    if (rc) {
        fpnn_aes_engine_destroy(e);
        return rc;
    }
    register_engine(e);
    *out = e;
    return FPNN_AES_OK;
}

int fpnn_aes_engine_destroy(fpnn_aes_engine *e) {
    if (!e) return FPNN_AES_OK;
    DeviceGuard g(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    (void)hipFree(e->d_tables);
#define X(name, type, zeroed) if (e->name.p) (void)(e->pools ? hipFreeAsync(e->name.p, e->stream) : hipFree(e->name.p));
    FPNN_AES_SCRATCH_BUFFERS(X)  // (every scratch buffer; the stream is idle)
#undef X
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    free_deferred(e);
    if (e->mpool) {  // (its blocks were freed above, behind the stream)
        (void)hipStreamSynchronize(e->stream);
        (void)hipMemPoolDestroy(e->mpool);
    }
    (void)hipFree(e->d_total);
    if (e->d_aud) (void)hipFree(e->d_aud);
    if (e->h_fault) (void)hipHostFree(e->h_fault);
    (void)hipFree(e->d_stage);
    if (e->h_stage) (void)hipHostFree(e->h_stage);
    if (e->h_small) (void)hipHostFree(e->h_small);
    if (e->h_mb) {  // the server left already (idle) or leaves now; the stream sync above waited
        __atomic_store_n(&e->h_mb->req.stop, 1u, __ATOMIC_RELEASE);
        if (e->stream) (void)hipStreamSynchronize(e->stream);
        (void)hipHostFree(e->h_mb);
    }
    if (e->h_sstate) (void)hipHostFree(e->h_sstate);
    for (auto &v : e->ev)
        for (auto &p : v) {
            (void)hipEventDestroy(p.beg);
            (void)hipEventDestroy(p.end);
        }
    for (auto &h : e->hs) {
        if (h.h) (void)hipHostFree(h.h);
        if (h.d) (void)hipFree(h.d);
        if (h.done) (void)hipEventDestroy(h.done);
        if (h.staged) (void)hipEventDestroy(h.staged);
        if (h.kdone) (void)hipEventDestroy(h.kdone);
        if (h.st) (void)hipStreamDestroy(h.st);
    }
    if (e->map_stream) (void)hipStreamSynchronize(e->map_stream);
    for (auto &m : e->ms) {
        if (m.h) (void)hipHostFree(m.h);
        if (m.d) (void)hipFree(m.d);
        if (m.gathered) (void)hipEventDestroy(m.gathered);
        if (m.ciphered) (void)hipEventDestroy(m.ciphered);
        if (m.done) (void)hipEventDestroy(m.done);
    }
    if (e->map_stream) (void)hipStreamDestroy(e->map_stream);
    unregister_engine(e);  // (no-op for an engine whose creation failed)
    if (e->batch_ev) (void)hipEventDestroy(e->batch_ev);
    if (e->own_stream && e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return FPNN_AES_OK;
}

int fpnn_aes_engine_sync(fpnn_aes_engine *e) {
    if (!e) return FPNN_AES_ERR_ARG;
    DeviceGuard g(e->device);
    HIP_TRY(hipStreamSynchronize(e->stream));
    return stream_idle(e);
}

void *fpnn_aes_engine_stream(fpnn_aes_engine *e) { return e ? (void *)e->stream : nullptr; }

// Devices the C++ classes' engine pool uses, in round-robin order (thread_engine.hpp).
static int pool_devices(int ndev, int *d, int cap) {
    int n = 0;
    if (const char *v = getenv("FPNN_AES_DEVICES")) {
        for (const char *p = v; *p && n < cap;) {
            char *end = nullptr;
            const long x = strtol(p, &end, 10);
            if (end == p) {
                p++;
                continue;
            }
            if (x >= 0 && x < ndev) d[n++] = (int)x;
            p = end;
        }
    } else if (const char *one = getenv("FPNN_AES_DEVICE")) {
        const int x = atoi(one);
        if (x >= 0 && x < ndev) d[n++] = x;
    } else {
        for (int i = 0; i < ndev && n < cap; i++) d[n++] = i;
    }
    return n;
}

int fpnn_aes_thread_engine_device(uint32_t k, int ndev) {
    int d[256];
    const int n = pool_devices(ndev, d, 256);
    return n ? d[k % (uint32_t)n] : -1;
}

int fpnn_aes_max_thread_engines(int ndev) {
    if (const char *v = getenv("FPNN_AES_MAX_ENGINES")) return std::max(1, atoi(v));
    int d[256];
    return std::max(1, 16 * pool_devices(ndev, d, 256));
}

int fpnn_aes_engine_reserve(fpnn_aes_engine *e, uint64_t max_segments, uint64_t max_blocks) {
    if (!e) return FPNN_AES_ERR_ARG;
    DeviceGuard g(e->device);
    // every call path at these bounds: calls within them then neither allocate nor memset
    return scratch_ensure(e, need_reserve(scratch_shape(e), max_segments, max_blocks));
}

uint64_t fpnn_aes_engine_scratch_bytes(fpnn_aes_engine *e) {
    uint64_t bytes = 0;
    if (!e) return 0;
#define X(name, type, zeroed) bytes += e->name.cap * sizeof(type);
    FPNN_AES_SCRATCH_BUFFERS(X)
#undef X
    return bytes;
}

// ---- key sets ---------------------------------------------------------------

int fpnn_aes_keyset_create(fpnn_aes_engine *e, uint32_t count, size_t keylen, const uint8_t *keys,
                           const uint8_t *ivs, int keys_on_host, fpnn_aes_keyset **out) {
    if (!e || !out || !keys || count == 0) return FPNN_AES_ERR_ARG;
    *out = nullptr;
    if (keylen != 16 && keylen != 24 && keylen != 32) return FPNN_AES_ERR_KEYLEN;
    DeviceGuard g(e->device);
    fpnn_aes_keyset *ks = new fpnn_aes_keyset();
    ks->e = e;
    ks->device = e->device;
    ks->count = count;
    ks->keylen = (uint32_t)keylen;
    ks->nrounds = (int)keylen / 4 + 6;
    uint8_t *d_raw = nullptr;
    size_t raw_bytes = 0;
    int rc = FPNN_AES_OK;
    do {
        hipError_t err = hipMalloc(reinterpret_cast<void **>(&ks->d_keys), sizeof(DevKey) * (size_t)count);
        if (err != hipSuccess) { rc = hip_fail(err, "hipMalloc(keys)"); break; }
        const uint8_t *k_dev = keys, *iv_dev = ivs;
        if (keys_on_host) {
            const size_t kb = (size_t)count * keylen, ib = ivs ? (size_t)count * 16 : 0;
            err = hipMalloc(reinterpret_cast<void **>(&d_raw), kb + ib);
            raw_bytes = kb + ib;
            if (err == hipSuccess) err = hipMemcpy(d_raw, keys, kb, hipMemcpyHostToDevice);
            if (err == hipSuccess && ivs) err = hipMemcpy(d_raw + kb, ivs, ib, hipMemcpyHostToDevice);
            if (err != hipSuccess) { rc = hip_fail(err, "upload(keys)"); break; }
            k_dev = d_raw;
            iv_dev = ivs ? d_raw + kb : nullptr;
        }
        err = launch_expand_keys(k_dev, (uint32_t)keylen, iv_dev, count, sbox_of(e), ks->d_keys, e->stream);
        if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void **>(&ks->d_eiv), sizeof(uint4) * (size_t)count);
        if (err == hipSuccess)
            err = launch_slot_eiv(ks->d_keys, 0, count, ks->nrounds, t0le_of(e), ks->d_eiv, e->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
        if (err != hipSuccess) { rc = hip_fail(err, "expand_keys"); break; }
    } while (0);
    if (d_raw) {  // the raw keys' upload: wiped behind the expansion that read it, then freed
        (void)hipMemsetAsync(d_raw, 0, raw_bytes, e->stream);
        (void)hipStreamSynchronize(e->stream);
        (void)hipFree(d_raw);
    }
    if (rc) {
        fpnn_aes_keyset_destroy(ks);
        return rc;
    }
    *out = ks;
    return FPNN_AES_OK;
}

int fpnn_aes_keyset_from_schedules(fpnn_aes_engine *e, uint32_t count, const fpnn_aes_schedule *ctx,
                                   const uint8_t *ivs, fpnn_aes_keyset **out) {
    if (!e || !out || !ctx || count == 0) return FPNN_AES_ERR_ARG;
    *out = nullptr;
    const int nr = ctx[0].nrounds;
    if (nr != 10 && nr != 12 && nr != 14) return FPNN_AES_ERR_KEYLEN;
    std::vector<DevKey> host(count);
    for (uint32_t i = 0; i < count; i++) {
        if (ctx[i].nrounds != nr) return FPNN_AES_ERR_ARG;
        devkey_from_schedule(&host[i], &ctx[i], ivs ? ivs + 16 * (size_t)i : nullptr);
    }
    DeviceGuard g(e->device);
    fpnn_aes_keyset *ks = new fpnn_aes_keyset();
    ks->e = e;
    ks->device = e->device;
    ks->count = count;
    ks->nrounds = nr;
    ks->keylen = (uint32_t)(nr - 6) * 4;
    hipError_t err = hipMalloc(reinterpret_cast<void **>(&ks->d_keys), sizeof(DevKey) * (size_t)count);
    if (err == hipSuccess) err = hipMemcpy(ks->d_keys, host.data(), sizeof(DevKey) * (size_t)count, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void **>(&ks->d_eiv), sizeof(uint4) * (size_t)count);
    if (err == hipSuccess) err = launch_slot_eiv(ks->d_keys, 0, count, nr, t0le_of(e), ks->d_eiv, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    if (err != hipSuccess) {
        int rc = hip_fail(err, "upload(schedules)");
        fpnn_aes_keyset_destroy(ks);
        return rc;
    }
    *out = ks;
    return FPNN_AES_OK;
}

int fpnn_aes_keyset_destroy(fpnn_aes_keyset *ks) {
    if (!ks) return FPNN_AES_OK;
    DeviceGuard g(ks->device);
    if (ks->up_done) {
        if (ks->up_pending) (void)hipEventSynchronize(ks->up_done);
        (void)hipEventDestroy(ks->up_done);
    }
    // Round keys, E_k(IV) and the staged schedules are wiped before their memory goes back
    // to the allocator.  (The creating engine may be gone, so not on its stream: wait for the
    // device, as hipFree does anyway, then clear on the null stream.)
    if (ks->h_up) {
        memset(ks->h_up, 0, sizeof(DevKey) * (size_t)ks->cap_up);
        (void)hipHostFree(ks->h_up);
    }
    const size_t slots = table_slots(ks);
    if (ks->d_keys || ks->d_eiv) (void)hipDeviceSynchronize();
    if (ks->d_keys) {
        (void)hipMemset(ks->d_keys, 0, sizeof(DevKey) * slots);
        (void)hipFree(ks->d_keys);  // hipFree waits for outstanding work on the device
    }
    if (ks->d_eiv) {
        (void)hipMemset(ks->d_eiv, 0, sizeof(uint4) * slots);
        (void)hipFree(ks->d_eiv);
    }
    delete ks;
    return FPNN_AES_OK;
}

int fpnn_aes_keyset_reserve(fpnn_aes_engine *e, uint32_t capacity, int nrounds, fpnn_aes_keyset **out) {
    if (!e || !out) return FPNN_AES_ERR_ARG;
    *out = nullptr;
    if (nrounds != 10 && nrounds != 12 && nrounds != 14) return FPNN_AES_ERR_KEYLEN;
    capacity = std::max<uint32_t>(capacity, 1);
    DeviceGuard g(e->device);
    fpnn_aes_keyset *ks = new fpnn_aes_keyset();
    ks->e = e;
    ks->device = e->device;
    ks->nrounds = nrounds;
    ks->keylen = (uint32_t)(nrounds - 6) * 4;
    ks->capacity = capacity;
    hipError_t err = hipMalloc(reinterpret_cast<void **>(&ks->d_keys), sizeof(DevKey) * (size_t)capacity);
    if (err == hipSuccess) err = hipMemsetAsync(ks->d_keys, 0, sizeof(DevKey) * (size_t)capacity, e->stream);
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void **>(&ks->d_eiv), sizeof(uint4) * (size_t)capacity);
    if (err == hipSuccess)  // (unset slots too: a batch naming one sees what the rounds would give)
        err = launch_slot_eiv(ks->d_keys, 0, capacity, nrounds, t0le_of(e), ks->d_eiv, e->stream);
    if (err == hipSuccess) err = hipEventCreateWithFlags(&ks->up_done, hipEventDisableTiming);
    if (err != hipSuccess) {
        const int rc = hip_fail(err, "keyset_reserve");
        fpnn_aes_keyset_destroy(ks);
        return rc;
    }
    *out = ks;
    return FPNN_AES_OK;
}

// Grow the table to at least `need` slots, keeping its contents (queued after everything
// before it); new slots are as fpnn_aes_keyset_reserve leaves them.  The old table is zeroed
// before it is freed.  Waits for the engine's stream when it grows; nothing otherwise.
static int keyset_grow(fpnn_aes_keyset *ks, uint32_t need) {
    const uint32_t have = table_slots(ks);
    if (need <= have) return FPNN_AES_OK;
    fpnn_aes_engine *e = ks->e;
    uint32_t cap = have;
    while (cap < need) cap = cap > 0x7fffffffu ? need : 2 * cap;
    DevKey *nk = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&nk), sizeof(DevKey) * (size_t)cap));
    HIP_TRY(hipMemsetAsync(nk + have, 0, sizeof(DevKey) * (size_t)(cap - have), e->stream));
    HIP_TRY(hipMemcpyAsync(nk, ks->d_keys, sizeof(DevKey) * (size_t)have, hipMemcpyDeviceToDevice, e->stream));
    uint4 *ne = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&ne), sizeof(uint4) * (size_t)cap));
    HIP_TRY(hipMemcpyAsync(ne, ks->d_eiv, sizeof(uint4) * (size_t)have, hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(launch_slot_eiv(nk, have, cap - have, ks->nrounds, t0le_of(e), ne, e->stream));
    // the old table: wiped behind its last readers, freed once the stream has run dry
    HIP_TRY(hipMemsetAsync(ks->d_keys, 0, sizeof(DevKey) * (size_t)have, e->stream));
    HIP_TRY(hipMemsetAsync(ks->d_eiv, 0, sizeof(uint4) * (size_t)have, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));  // the old table may still be read by queued kernels
    (void)hipFree(ks->d_keys);
    (void)hipFree(ks->d_eiv);
    ks->d_keys = nk;
    ks->d_eiv = ne;
    ks->capacity = cap;
    return FPNN_AES_OK;
}

int fpnn_aes_keyset_set(fpnn_aes_keyset *ks, uint32_t first, uint32_t count, const fpnn_aes_schedule *ctx,
                        const uint8_t *ivs) {
    if (!ks || !ks->e || (count && !ctx) || !ks->up_done) return FPNN_AES_ERR_ARG;
    if (count == 0) return FPNN_AES_OK;
    if ((uint64_t)first + count > 0xffffffffull) return FPNN_AES_ERR_RANGE;
    for (uint32_t i = 0; i < count; i++)
        if (ctx[i].nrounds != ks->nrounds) return FPNN_AES_ERR_KEYLEN;
    fpnn_aes_engine *e = ks->e;
    DeviceGuard g(ks->device);
    const uint32_t need = first + count;
    const int grc = keyset_grow(ks, need);
    if (grc) return grc;
    if (ks->up_pending) {  // the staging still feeds the previous upload
        HIP_TRY(hipEventSynchronize(ks->up_done));
        ks->up_pending = false;
    }
    if (count > ks->cap_up) {
        if (ks->h_up) (void)hipHostFree(ks->h_up);
        ks->h_up = nullptr;
        ks->cap_up = 0;
        const uint32_t c = std::max<uint32_t>(count, 256);
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&ks->h_up), sizeof(DevKey) * (size_t)c, 0));
        ks->cap_up = c;
    }
    for (uint32_t i = 0; i < count; i++)  // (every ctx[i].nrounds is the table's, checked above)
        devkey_from_schedule(&ks->h_up[i], &ctx[i], ivs ? ivs + 16 * (size_t)i : nullptr);
    HIP_TRY(hipMemcpyAsync(ks->d_keys + first, ks->h_up, sizeof(DevKey) * (size_t)count, hipMemcpyHostToDevice,
                           e->stream));
    HIP_TRY(hipEventRecord(ks->up_done, e->stream));
    HIP_TRY(launch_slot_eiv(ks->d_keys, first, count, ks->nrounds, t0le_of(e), ks->d_eiv, e->stream));
    ks->up_pending = true;
    ks->count = std::max(ks->count, need);
    return FPNN_AES_OK;
}

uint32_t fpnn_aes_keyset_count(const fpnn_aes_keyset *ks) { return ks ? ks->count : 0; }

int fpnn_aes_keyset_nrounds(const fpnn_aes_keyset *ks) { return ks ? ks->nrounds : 0; }

int fpnn_aes_keyset_get_schedule(fpnn_aes_keyset *ks, uint32_t slot, fpnn_aes_schedule *out) {
    if (!ks || !out || slot >= ks->count) return FPNN_AES_ERR_ARG;
    DeviceGuard g(ks->device);
    DevKey d;
    HIP_TRY(hipMemcpy(&d, ks->d_keys + slot, sizeof d, hipMemcpyDeviceToHost));
    memset(out, 0, sizeof *out);
    out->nrounds = (int)d.nrounds;
    for (int k = 0; k < 4 * ((int)d.nrounds + 1); k++) out->rk[k] = bswap32(d.rk[k]);
    return FPNN_AES_OK;
}

uint32_t fpnn_aes_keyset_capacity(const fpnn_aes_keyset *ks) { return ks ? table_slots(ks) : 0; }

// ---- writes into a live table, on the device (k_keytable.hip) --------------------
// The addressing part of a call: the host-known bound, the table grown to it (only then a
// wait), the kernel's view of the table.
static int keytable_args(fpnn_aes_keyset *ks, uint32_t first, uint32_t count, const uint32_t *slots,
                         uint32_t slot_bound, KeyTableArgs &a) {
    if (!slots && (uint64_t)first + count > 0xffffffffull) return FPNN_AES_ERR_RANGE;
    if ((uintptr_t)slots & 3u) return FPNN_AES_ERR_ARG;
    const uint32_t bound = slots ? slot_bound : first + count;
    DeviceGuard g(ks->device);
    const int rc = keyset_grow(ks, bound);
    if (rc) return rc;
    memset(&a, 0, sizeof a);
    a.keys = ks->d_keys;
    a.eiv = ks->d_eiv;
    a.slots = slots;
    a.first = first;
    a.count = count;
    a.slot_bound = bound;
    a.t0le = t0le_of(ks->e);
    a.fault = ks->e->d_fault;
    return FPNN_AES_OK;
}

// Queue the write (set: k_set_keys, else k_clear_slots) on the table's engine.
static int keytable_run(fpnn_aes_keyset *ks, KeyTableArgs &a, bool set) {
    fpnn_aes_engine *e = ks->e;
    DeviceGuard g(ks->device);
    const BatchScope batch_scope(e);  // (an early return clears the pending flag)
    if (int rc = audit_begin_keytable(e, ks, a)) return rc;
    HIP_TRY(set ? launch_set_keys(a, ks->keylen, e->stream) : launch_clear_slots(a, ks->nrounds, e->stream));
    batch_queued(e);
    ks->count = std::max(ks->count, a.slot_bound);
    return audit_end(e, FPNN_AES_OK);
}

int fpnn_aes_keyset_set_keys(fpnn_aes_keyset *ks, uint32_t first, uint32_t count, const uint32_t *slots,
                             uint32_t slot_bound, const uint8_t *keys, const uint8_t *ivs, const uint8_t *ok) {
    if (!ks || !ks->e || (count && !keys)) return FPNN_AES_ERR_ARG;
    if (count == 0) return FPNN_AES_OK;
    KeyTableArgs a;
    const int rc = keytable_args(ks, first, count, slots, slot_bound, a);
    if (rc) return rc;
    a.raw = keys;
    a.ivs = ivs;
    a.ok = ok;
    return keytable_run(ks, a, true);
}

int fpnn_aes_keyset_clear(fpnn_aes_keyset *ks, uint32_t first, uint32_t count, const uint32_t *slots,
                          uint32_t slot_bound) {
    if (!ks || !ks->e) return FPNN_AES_ERR_ARG;
    if (count == 0) return FPNN_AES_OK;
    KeyTableArgs a;
    const int rc = keytable_args(ks, first, count, slots, slot_bound, a);
    if (rc) return rc;
    return keytable_run(ks, a, false);
}

// ---- stream state by slot (k_keytable.hip) ---------------------------------------
// open: (IV of the slot, 0); close: all zero.  The table is read, never grown: the bound
// must lie within its allocations.
static int stream_state_run(fpnn_aes_keyset *ks, uint32_t first, uint32_t count, const uint32_t *slots,
                            uint32_t slot_bound, const uint8_t *ok, uint8_t *iv_state, uint32_t *pos_state, bool open) {
    if (!ks || !ks->e) return FPNN_AES_ERR_ARG;
    if (count == 0) return FPNN_AES_OK;
    if (!iv_state || !pos_state || ((uintptr_t)iv_state & 15u) || ((uintptr_t)pos_state & 3u) || ((uintptr_t)slots & 3u))
        return FPNN_AES_ERR_ARG;
    if (!slots && (uint64_t)first + count > 0xffffffffull) return FPNN_AES_ERR_RANGE;
    const uint32_t bound = slots ? slot_bound : first + count;
    if (bound > table_slots(ks)) return FPNN_AES_ERR_ARG;
    fpnn_aes_engine *e = ks->e;
    DeviceGuard g(ks->device);
    KeyTableArgs a;
    memset(&a, 0, sizeof a);
    a.keys = ks->d_keys;
    a.slots = slots;
    a.first = first;
    a.count = count;
    a.slot_bound = bound;
    a.ok = open ? ok : nullptr;
    a.iv_state = reinterpret_cast<uint4 *>(iv_state);
    a.pos_state = pos_state;
    a.fault = e->d_fault;
    const BatchScope batch_scope(e);  // (an early return clears the pending flag)
    if (int rc = audit_begin_keytable(e, ks, a)) return rc;
    HIP_TRY(open ? launch_stream_open(a, e->stream) : launch_stream_close(a, e->stream));
    batch_queued(e);
    return audit_end(e, FPNN_AES_OK);
}

int fpnn_aes_stream_open(fpnn_aes_keyset *ks, uint32_t first, uint32_t count, const uint32_t *slots,
                         uint32_t slot_bound, const uint8_t *ok, uint8_t *iv_state, uint32_t *pos_state) {
    return stream_state_run(ks, first, count, slots, slot_bound, ok, iv_state, pos_state, true);
}

int fpnn_aes_stream_close(fpnn_aes_keyset *ks, uint32_t first, uint32_t count, const uint32_t *slots,
                          uint32_t slot_bound, uint8_t *iv_state, uint32_t *pos_state) {
    return stream_state_run(ks, first, count, slots, slot_bound, nullptr, iv_state, pos_state, false);
}

// ---- batches ---------------------------------------------------------------------

int fpnn_aes_package_encrypt(fpnn_aes_engine *e, const fpnn_aes_batch *b) {
    return run_encrypt(e, b, nullptr, nullptr, false);
}

int fpnn_aes_package_decrypt(fpnn_aes_engine *e, const fpnn_aes_batch *b) {
    return run_decrypt(e, b, nullptr, nullptr, false);
}

int fpnn_aes_stream_encrypt(fpnn_aes_engine *e, const fpnn_aes_batch *b, uint8_t *iv_state, uint32_t *pos_state) {
    if (b && (b->flags & FPNN_AES_F_WIRE_PREFIX)) return FPNN_AES_ERR_ARG;
    return run_encrypt(e, b, iv_state, pos_state, true);
}

int fpnn_aes_stream_decrypt(fpnn_aes_engine *e, const fpnn_aes_batch *b, uint8_t *iv_state, uint32_t *pos_state) {
    return run_decrypt(e, b, iv_state, pos_state, true);
}

int fpnn_aes_stream_encrypt_frames(fpnn_aes_engine *e, const fpnn_aes_batch *b, const uint32_t *first_frame,
                                   uint32_t nstreams, uint8_t *iv_state, uint32_t *pos_state) {
    return run_frames(e, b, first_frame, nstreams, iv_state, pos_state, true);
}

int fpnn_aes_stream_decrypt_frames(fpnn_aes_engine *e, const fpnn_aes_batch *b, const uint32_t *first_frame,
                                   uint32_t nstreams, uint8_t *iv_state, uint32_t *pos_state) {
    return run_frames(e, b, first_frame, nstreams, iv_state, pos_state, false);
}

int fpnn_aes_stream_encrypt_at(fpnn_aes_engine *e, const fpnn_aes_batch *b, const uint32_t *state_slot,
                               uint32_t slot_bound, uint8_t *iv_state, uint32_t *pos_state) {
    return run_batch_at(e, true, b, state_slot, slot_bound, iv_state, pos_state);
}

int fpnn_aes_stream_decrypt_at(fpnn_aes_engine *e, const fpnn_aes_batch *b, const uint32_t *state_slot,
                               uint32_t slot_bound, uint8_t *iv_state, uint32_t *pos_state) {
    return run_batch_at(e, false, b, state_slot, slot_bound, iv_state, pos_state);
}

int fpnn_aes_stream_encrypt_frames_at(fpnn_aes_engine *e, const fpnn_aes_batch *b, const uint32_t *first_frame,
                                      uint32_t nstreams, const uint32_t *state_slot, uint32_t slot_bound,
                                      uint8_t *iv_state, uint32_t *pos_state) {
    const SlotAddr at{state_slot, slot_bound, false};
    return run_frames(e, b, first_frame, nstreams, iv_state, pos_state, true, &at);
}

int fpnn_aes_stream_decrypt_frames_at(fpnn_aes_engine *e, const fpnn_aes_batch *b, const uint32_t *first_frame,
                                      uint32_t nstreams, const uint32_t *state_slot, uint32_t slot_bound,
                                      uint8_t *iv_state, uint32_t *pos_state) {
    const SlotAddr at{state_slot, slot_bound, false};
    return run_frames(e, b, first_frame, nstreams, iv_state, pos_state, false, &at);
}

// ---- UDP v2 datagrams with data encryption ---------------------------------------

int fpnn_aes_udp_encrypt(fpnn_aes_engine *e, const fpnn_aes_batch *b, const fpnn_aes_udp_data *u) {
    return audit_end(e, run_udp_encrypt_calls(e, b, u));
}

int fpnn_aes_udp_decrypt(fpnn_aes_engine *e, const fpnn_aes_batch *b, const fpnn_aes_udp_data *u) {
    return audit_end(e, run_udp_decrypt_calls(e, b, u));
}

int fpnn_aes_udp_recv(fpnn_aes_engine *e, const fpnn_aes_batch *b, const fpnn_aes_udp_data *u, uint32_t flags,
                      uint32_t max_pkgs, uint32_t max_sections, fpnn_aes_udp_scan *scan, fpnn_aes_udp_pkg *pkgs,
                      fpnn_aes_udp_section *sections) {
    return audit_end(e, run_udp_recv_calls(e, b, u, false, flags, max_pkgs, max_sections, scan, pkgs, sections, nullptr,
                                           nullptr, 0));
}

int fpnn_aes_udp_recv_take(fpnn_aes_engine *e, const fpnn_aes_batch *b, const fpnn_aes_udp_data *u, uint32_t max_pkgs,
                           uint32_t max_sections, const fpnn_aes_udp_scan *scan, const fpnn_aes_udp_pkg *pkgs,
                           const fpnn_aes_udp_section *sections, const uint32_t *first_take, const uint32_t *take,
                           uint32_t ntake) {
    return audit_end(e, run_udp_recv_calls(e, b, u, true, 0, max_pkgs, max_sections, scan, pkgs, sections, first_take,
                                           take, ntake));
}

// ---- receive side: wire framing on the device ------------------------------------

int fpnn_aes_package_recv(fpnn_aes_engine *e, const fpnn_aes_batch *b, uint32_t max_len, uint32_t max_frames,
                          uint64_t *frame_off, uint32_t *frame_len, fpnn_aes_frame_scan *scan) {
    int rc = check_batch(e, b);
    if (rc) return rc;
    if ((rc = debug_fail_point())) return rc;
    if (b->out_off || b->flags) return FPNN_AES_ERR_ARG;
    if (!b->count) return FPNN_AES_OK;
    if (!frame_off || !frame_len || !scan || !max_frames) return FPNN_AES_ERR_ARG;
    const uint64_t slots = (uint64_t)b->count * max_frames;
    if (slots > 0xffffffffull) return FPNN_AES_ERR_RANGE;
    DeviceGuard g(e->device);
    const bool per_key = fpnn_aes::per_key(batch_shape(b));
    if ((rc = e->fr_off.ensure(e, slots))) return rc;
    if (per_key && (rc = e->fr_slot.ensure(e, slots))) return rc;
    KScan s;
    memset(&s, 0, sizeof s);
    s.buf = b->in;
    s.count = b->count;
    s.off = b->in_off;
    s.stride = b->stride;
    s.len = b->len;
    s.uniform_len = b->uniform_len;
    s.max_len = max_len;
    s.key_slot = per_key ? b->key_slot : nullptr;
    s.max_frames = max_frames;
    s.frame_off = frame_off;
    s.frame_len = frame_len;
    s.scan = reinterpret_cast<ScanResult *>(scan);
    s.abs_off = e->fr_off.p;
    s.abs_slot = per_key ? e->fr_slot.p : nullptr;
    static_assert(sizeof(ScanResult) == sizeof(fpnn_aes_frame_scan), "scan layout");
    const BatchScope batch_scope(e);  // (an early return clears the pending flag)
    HIP_TRY(launch_scan_frames(s, false, e->num_cus, e->stream));
    batch_queued(e);
    // every frame slot is one package segment (unused ones have length 0)
    fpnn_aes_batch fb;
    memset(&fb, 0, sizeof fb);
    fb.in = b->in;
    fb.out = b->out;
    fb.count = (uint32_t)slots;
    fb.in_off = e->fr_off.p;
    fb.len = frame_len;
    fb.key_slot = per_key ? e->fr_slot.p : nullptr;
    fb.keys = b->keys;
    fb.max_len = max_len;  // (every frame the scan accepts is within it: D2s for FPNN's quests)
    return run_decrypt(e, &fb, nullptr, nullptr, false);
}

// at: fpnn_aes_stream_recv_at -- the decrypt is the slot-addressed *_frames path with one
// frame per stream; the scan is per segment either way.
static int stream_recv_run(fpnn_aes_engine *e, const fpnn_aes_batch *b, const SlotAddr *at, uint8_t *iv_state,
                           uint32_t *pos_state, const uint32_t *carry, uint32_t max_len, uint32_t max_frames,
                           uint64_t *frame_off, uint32_t *frame_len, fpnn_aes_frame_scan *scan) {
    int rc = check_batch(e, b);
    if (rc) return rc;
    if ((rc = debug_fail_point())) return rc;
    if (!b->count) return FPNN_AES_OK;
    if (!frame_off || !frame_len || !scan || !max_frames) return FPNN_AES_ERR_ARG;
    if ((uint64_t)b->count * max_frames > 0xffffffffull) return FPNN_AES_ERR_RANGE;
    if (at) rc = run_frames(e, b, nullptr, b->count, iv_state, pos_state, false, at);
    else rc = run_decrypt(e, b, iv_state, pos_state, true);
    if (rc) return rc;
    DeviceGuard g(e->device);
    KScan s;
    memset(&s, 0, sizeof s);
    s.buf = b->out;
    s.count = b->count;
    s.off = b->out_off ? b->out_off : b->in_off;
    s.stride = b->stride;
    s.len = b->len;
    s.uniform_len = b->uniform_len;
    s.max_len = max_len;
    s.carry = carry;
    s.max_frames = max_frames;
    s.frame_off = frame_off;
    s.frame_len = frame_len;
    s.scan = reinterpret_cast<ScanResult *>(scan);
    const BatchScope batch_scope(e);  // (an early return clears the pending flag)
    HIP_TRY(launch_scan_frames(s, true, e->num_cus, e->stream));
    batch_queued(e);
    return FPNN_AES_OK;
}

int fpnn_aes_stream_recv(fpnn_aes_engine *e, const fpnn_aes_batch *b, uint8_t *iv_state, uint32_t *pos_state,
                         const uint32_t *carry, uint32_t max_len, uint32_t max_frames, uint64_t *frame_off,
                         uint32_t *frame_len, fpnn_aes_frame_scan *scan) {
    return stream_recv_run(e, b, nullptr, iv_state, pos_state, carry, max_len, max_frames, frame_off, frame_len, scan);
}

int fpnn_aes_stream_recv_at(fpnn_aes_engine *e, const fpnn_aes_batch *b, const uint32_t *state_slot,
                            uint32_t slot_bound, uint8_t *iv_state, uint32_t *pos_state, const uint32_t *carry,
                            uint32_t max_len, uint32_t max_frames, uint64_t *frame_off, uint32_t *frame_len,
                            fpnn_aes_frame_scan *scan) {
    const SlotAddr at{state_slot, slot_bound, true};
    return stream_recv_run(e, b, &at, iv_state, pos_state, carry, max_len, max_frames, frame_off, frame_len, scan);
}

// ---- single call from host memory ------------------------------------------------

}  // extern "C"

namespace {

// pinned + device staging of the synchronous single-call paths, grown on demand
int stage_reserve(fpnn_aes_engine *e, uint64_t need) {
    if (need <= e->cap_stage) return FPNN_AES_OK;
    uint64_t n = e->cap_stage ? e->cap_stage : 65536;
    while (n < need) n *= 2;
    if (e->h_stage) (void)hipHostFree(e->h_stage);
    if (e->d_stage) (void)hipFree(e->d_stage);
    e->h_stage = nullptr;
    e->d_stage = nullptr;
    e->cap_stage = 0;
    HIP_TRY(pinned_host_alloc(e->numa.node, reinterpret_cast<void **>(&e->h_stage), n));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&e->d_stage), n));
    e->cap_stage = n;
    return FPNN_AES_OK;
}

bool valid_rounds(int nr) { return nr == 10 || nr == 12 || nr == 14; }

// K0 for calls of up to kSmallMaxBytes (FPNN_AES_SMALL=0 routes them through the batch
// kernels, the A/B baseline).
bool small_enabled() {
    static const bool on = [] {
        const char *v = getenv("FPNN_AES_SMALL");
        return !v || atoi(v) != 0;
    }();
    return on;
}

// One small synchronous CFB call through K0 (k_small.hip): the bytes go into pinned
// staging, one launch ciphers them in place there, and the kernel's sequence-number store
// says the results are in.  The wait spins on that word; after 20 ms it falls back to the
// stream sync, which also reports a kernel that failed.
constexpr uint64_t kSmallStage = kSmallBodyAt + kSmallMaxBytes + 64;
int cfb_small_launch(fpnn_aes_engine *e, const fpnn_aes_schedule *ctx, bool encrypt, const uint8_t *in, uint8_t *out,
                     size_t len, uint8_t ivec[16], size_t *p_num) {
    if (!e->h_small) {
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e->h_small), kSmallStage, hipHostMallocCoherent));
        HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&e->d_small), e->h_small, 0));
    }
    const uint32_t pos = (uint32_t)*p_num;
    const uint32_t head = pos ? (uint32_t)std::min<size_t>(len, 16 - pos) : 0u;
    memcpy(e->h_small + kSmallBodyAt - head, in, len);
    SmallArgs a;
    a.io = e->d_small;
    a.len = (uint32_t)len;
    a.head = head;
    a.pos = pos;
    a.seq = ++e->small_seq;
    memcpy(&a.iv, ivec, 16);
    for (int k = 0; k < 4 * (ctx->nrounds + 1); k++) a.rk[k] = bswap32(ctx->rk[k]);
    a.t0le = t0le_of(e);
    a.state = reinterpret_cast<uint32_t *>(e->d_small + kSmallStage - 32);
    volatile uint32_t *hstate = reinterpret_cast<volatile uint32_t *>(e->h_small + kSmallStage - 32);
    const int which = encrypt ? FPNN_AES_K_ENCRYPT : FPNN_AES_K_DECRYPT;
    EventPair *ev;
    if (int rc = timing_begin(e, which, &ev)) return rc;
    HIP_TRY(launch_cfb_single(a, ctx->nrounds, encrypt, e->stream));
    if (int rc = timing_end(e, ev, which)) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0; __atomic_load_n(&hstate[5], __ATOMIC_ACQUIRE) != a.seq; spins++) {
        __builtin_ia32_pause();
        if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) {
            HIP_TRY(hipStreamSynchronize(e->stream));
            if (__atomic_load_n(&hstate[5], __ATOMIC_ACQUIRE) != a.seq) {
                g_last_error = "small-call kernel finished without publishing its result";
                return FPNN_AES_ERR_HIP;
            }
            break;
        }
    }
    memcpy(out, e->h_small + kSmallBodyAt - head, len);
    for (int i = 0; i < 4; i++) {
        const uint32_t w = hstate[i];
        memcpy(ivec + 4 * i, &w, 4);
    }
    *p_num = hstate[4];
    return FPNN_AES_OK;
}

// K0s, the resident server (FPNN_AES_SMALL_SERVER=0: a K0 launch per call instead).  The
// request goes into the mailbox, its number last (release); if no server of this engine is
// alive one is launched on the engine stream (it starts after whatever is queued there);
// the host spins until the server stores the number into resp.done.  A server that left
// (idle, lifetime) before seeing the request is relaunched; after 20 ms of spinning the
// stream sync -- which returns once the server has left, and reports a failed kernel --
// settles it.
// Batch-activity words, one per device (64-byte apart) in pinned host memory, created with
// the first server: the host bumps its device's word before it queues batch kernels, and
// every server of that device leaves after its current request (kernels.hpp,
// launch_cfb_server).  An idle server would otherwise hold a CU -- and its hardware queue,
// which the box shares among streams (GPU_MAX_HW_QUEUES = 4) -- for up to its 2 ms
// lifetime while a persistent batch grid waits for it.
std::atomic<uint32_t *> g_yield{nullptr};
std::mutex g_yield_mu;

uint32_t *yield_words() {
    uint32_t *y = g_yield.load(std::memory_order_acquire);
    if (y) return y;
    std::lock_guard<std::mutex> lk(g_yield_mu);
    y = g_yield.load(std::memory_order_relaxed);
    if (!y) {
        void *p = nullptr;
        if (hipHostMalloc(&p, 64 * 64, hipHostMallocCoherent | hipHostMallocPortable | hipHostMallocMapped) != hipSuccess)
            return nullptr;
        memset(p, 0, 64 * 64);
        y = static_cast<uint32_t *>(p);
        g_yield.store(y, std::memory_order_release);
    }
    return y;
}

// before batch kernels are queued on a device (no-op until a server ever ran): servers
// leave, and no server is relaunched until the work is done (batch_fence)
void batch_signal(fpnn_aes_engine *e) {
    if (uint32_t *y = g_yield.load(std::memory_order_acquire)) {
        e->batch_pending.store(true, std::memory_order_release);
        __atomic_fetch_add(y + 16 * (e->device & 63), 1u, __ATOMIC_RELEASE);
    }
}

BatchScope::~BatchScope() { e->batch_pending.store(false, std::memory_order_release); }

// Engines per device, for batch_fence.
struct DeviceEngines {
    std::mutex mu;
    std::vector<fpnn_aes_engine *> list;
};
DeviceEngines g_dev_engines[64];

void register_engine(fpnn_aes_engine *e) {
    DeviceEngines &d = g_dev_engines[e->device & 63];
    std::lock_guard<std::mutex> lk(d.mu);
    d.list.push_back(e);
}

void unregister_engine(fpnn_aes_engine *e) {
    DeviceEngines &d = g_dev_engines[e->device & 63];
    std::lock_guard<std::mutex> lk(d.mu);
    d.list.erase(std::remove(d.list.begin(), d.list.end(), e), d.list.end());
}

// after an engine queued batch kernels (once servers exist): remember where they end
void batch_queued(fpnn_aes_engine *e) {
    if (!g_yield.load(std::memory_order_acquire)) return;  // no server ever ran: nothing waits
    if (e->batch_ev || hipEventCreateWithFlags(&e->batch_ev, hipEventDisableTiming) == hipSuccess)
        if (hipEventRecord(e->batch_ev, e->stream) == hipSuccess) e->batch_ev_live.store(true, std::memory_order_release);
    e->batch_pending.store(false, std::memory_order_release);
}

// Before (re)launching a small-call server: wait until the batch work other engines queued
// on this device has finished.  A server launched meanwhile would take a CU from a
// persistent batch grid (every workgroup holds a static share of the work, so the whole
// call waits for that CU) -- servers leave when batch work is queued (batch_signal), and
// do not come back until it is done.  The per-call request waits for the batch instead,
// which it would do anyway: the batch grid holds every CU.
// The wait is bounded (kBatchFenceMs): an engine that queues batch after batch would
// otherwise starve the per-call path; past the bound the server is launched and waits for
// a CU like any kernel.
void batch_fence(fpnn_aes_engine *e) {
    constexpr int kBatchFenceMs = 5;
    DeviceEngines &d = g_dev_engines[e->device & 63];
    std::lock_guard<std::mutex> lk(d.mu);
    const auto t0 = std::chrono::steady_clock::now();
    auto late = [&]() { return std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(kBatchFenceMs); };
    for (fpnn_aes_engine *o : d.list) {
        if (o == e) continue;
        for (uint32_t spins = 0;; spins++) {
            if (o->batch_pending.load(std::memory_order_acquire)) {  // its kernels are being queued
                __builtin_ia32_pause();
            } else if (o->batch_ev_live.load(std::memory_order_acquire)) {
                const hipError_t q = hipEventQuery(o->batch_ev);
                if (q != hipErrorNotReady) {
                    if (q == hipSuccess) o->batch_ev_live.store(false, std::memory_order_release);
                    break;
                }
                __builtin_ia32_pause();
            } else {
                break;
            }
            if ((spins & 255) == 255 && late()) return;
        }
    }
}

bool server_enabled() {
    static const bool on = [] {
        const char *v = getenv("FPNN_AES_SMALL_SERVER");
        return !v || atoi(v) != 0;
    }();
    return on;
}

// Relaunch order: read the device's batch-activity value y0 FIRST, then wait out batch
// work (batch_fence), then launch the server with y0.  A batch that signals after the read
// makes the server leave at its first poll; one that signalled before it set its pending
// flag first (batch_signal), so the fence waits for it.  (Reading y0 after the fence let a
// batch slip in between: its server then never saw a change and held a CU through it.)
int launch_server(fpnn_aes_engine *e) {
    if (!e->srv_idle_ticks) {
        int khz = 0;  // device wall clock (wall_clock64), kHz
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, e->device) != hipSuccess || khz <= 0)
            khz = 100000;
        e->srv_idle_ticks = (uint64_t)khz / 20;   // 50 us without a request
        e->srv_life_ticks = (uint64_t)khz * 2;    // 2 ms in any case
    }
    uint32_t *yh = yield_words();
    if (!yh) return hip_fail(hipErrorOutOfMemory, "hipHostMalloc(yield)");
    uint32_t *yd = nullptr;
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&yd), yh + 16 * (e->device & 63), 0));
    const uint32_t y0 = __atomic_load_n(yh + 16 * (e->device & 63), __ATOMIC_ACQUIRE);
    batch_fence(e);
    const uint32_t epoch = ++e->srv_epoch;
    HIP_TRY(launch_cfb_server(e->d_mb, t0le_of(e), epoch, e->srv_idle_ticks, e->srv_life_ticks, yd, y0, e->stream));
    return FPNN_AES_OK;
}

int cfb_small_server(fpnn_aes_engine *e, const fpnn_aes_schedule *ctx, bool encrypt, const uint8_t *in, uint8_t *out,
                     size_t len, uint8_t ivec[16], size_t *p_num) {
    if (!e->h_mb) {
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&e->h_mb), sizeof(SmallMailbox), hipHostMallocCoherent));
        memset(e->h_mb, 0, sizeof(SmallMailbox));
        HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&e->d_mb), e->h_mb, 0));
    }
    SmallMailbox *mb = e->h_mb;
    const uint32_t pos = (uint32_t)*p_num;
    const uint32_t head = pos ? (uint32_t)std::min<size_t>(len, 16 - pos) : 0u;
    memcpy(mb->io + kSmallBodyAt - head, in, len);
    mb->req.op = encrypt ? 1u : 0u;
    mb->req.len = (uint32_t)len;
    mb->req.head = head;
    mb->req.pos = pos;
    mb->req.nrounds = (uint32_t)ctx->nrounds;
    memcpy(mb->req.iv, ivec, 16);
    for (int k = 0; k < 4 * (ctx->nrounds + 1); k++) mb->req.rk[k] = bswap32(ctx->rk[k]);
    const uint32_t seq = ++e->mb_seq;
    __atomic_store_n(&mb->req.seq, seq, __ATOMIC_RELEASE);
    const int which = encrypt ? FPNN_AES_K_ENCRYPT : FPNN_AES_K_DECRYPT;
    e->last_kernel[which] = "cfb_server";
    // a server is alive unless none was launched or the last one has stored its epoch
    if (e->srv_epoch == 0 || __atomic_load_n(&mb->resp.exited, __ATOMIC_ACQUIRE) == e->srv_epoch) {
        if (int rc = launch_server(e)) return rc;
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spins = 0; __atomic_load_n(&mb->resp.done, __ATOMIC_ACQUIRE) != seq; spins++) {
        __builtin_ia32_pause();
        if (__atomic_load_n(&mb->resp.exited, __ATOMIC_ACQUIRE) == e->srv_epoch &&
            __atomic_load_n(&mb->resp.done, __ATOMIC_ACQUIRE) != seq) {
            if (int rc = launch_server(e)) return rc;  // it left before seeing this request
            continue;
        }
        if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) {
            HIP_TRY(hipStreamSynchronize(e->stream));
            if (__atomic_load_n(&mb->resp.done, __ATOMIC_ACQUIRE) != seq) {
                g_last_error = "small-call server left without serving the request";
                return FPNN_AES_ERR_HIP;
            }
            break;
        }
    }
    memcpy(out, mb->io + kSmallBodyAt - head, len);
    memcpy(ivec, mb->resp.state, 16);
    *p_num = mb->resp.state[4];
    return FPNN_AES_OK;
}

int cfb_small(fpnn_aes_engine *e, const fpnn_aes_schedule *ctx, bool encrypt, const uint8_t *in, uint8_t *out,
              size_t len, uint8_t ivec[16], size_t *p_num) {
    DeviceGuard g(e->device);
    return server_enabled() ? cfb_small_server(e, ctx, encrypt, in, out, len, ivec, p_num)
                            : cfb_small_launch(e, ctx, encrypt, in, out, len, ivec, p_num);
}

// One synchronous rijndael.h call in the non-CFB modes (k_modes.hip).  Staging:
// [DevKey 272][iv 16][pos 4 | pad 12][in: in_bytes, 16-padded][out: out_bytes]
int modes_call(fpnn_aes_engine *e, const fpnn_aes_schedule *ctx, int mode, const uint8_t *in, uint64_t in_copy,
               uint64_t in_bytes, uint8_t *out, uint64_t out_copy, uint64_t nblocks, uint64_t len, uint8_t *ivec,
               size_t *p_num) {
    const uint64_t hdr = sizeof(DevKey) + 32;
    const uint64_t ipad = (in_bytes + 15) & ~15ull, opad = (std::max(out_copy, nblocks * 16) + 15) & ~15ull;
    DeviceGuard g(e->device);
    if (int rc = stage_reserve(e, hdr + ipad + opad)) return rc;
    devkey_from_schedule(reinterpret_cast<DevKey *>(e->h_stage), ctx);
    uint8_t *h_iv = e->h_stage + sizeof(DevKey);
    uint32_t *h_pos = reinterpret_cast<uint32_t *>(h_iv + 16);
    if (ivec) memcpy(h_iv, ivec, 16); else memset(h_iv, 0, 16);
    *h_pos = p_num ? (uint32_t)*p_num : 0u;
    if (in_copy) memcpy(e->h_stage + hdr, in, in_copy);
    if (ipad > in_copy) memset(e->h_stage + hdr + in_copy, 0, ipad - in_copy);  // CBC: zero padding
    HIP_TRY(hipMemcpyAsync(e->d_stage, e->h_stage, hdr + ipad, hipMemcpyHostToDevice, e->stream));
    ModeArgs a;
    a.in = e->d_stage + hdr;
    a.out = e->d_stage + hdr + ipad;
    a.nblocks = nblocks;
    a.len = len;
    a.key = reinterpret_cast<const DevKey *>(e->d_stage);
    a.iv = e->d_stage + sizeof(DevKey);
    a.pos = reinterpret_cast<uint32_t *>(a.iv + 16);
    a.t0le = t0le_of(e);
    a.td0le = td0le_of(e);
    a.isbox = isbox_of(e);
    HIP_TRY(launch_block_modes(a, ctx->nrounds, mode, e->num_cus, e->stream));
    e->last_kernel[FPNN_AES_K_ENCRYPT] = last_launched();
    HIP_TRY(hipMemcpyAsync(h_iv, a.iv, 32, hipMemcpyDeviceToHost, e->stream));
    if (out_copy) HIP_TRY(hipMemcpyAsync(e->h_stage + hdr + ipad, a.out, out_copy, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (int rf = stream_idle(e)) return rf;
    if (out_copy) memcpy(out, e->h_stage + hdr + ipad, out_copy);
    if (ivec && mode != MODE_CBC_DEC) memcpy(ivec, h_iv, 16);
    if (p_num) *p_num = *h_pos;
    return FPNN_AES_OK;
}

}  // namespace

extern "C" {

int fpnn_aes_ecb_host(fpnn_aes_engine *e, const fpnn_aes_schedule *ctx, int encrypt, const uint8_t *in, uint8_t *out,
                      size_t nblocks) {
    if (!e || !ctx || (nblocks && (!in || !out))) return FPNN_AES_ERR_ARG;
    if (!valid_rounds(ctx->nrounds)) return FPNN_AES_ERR_KEYLEN;
    if (!nblocks) return FPNN_AES_OK;
    return modes_call(e, ctx, encrypt ? MODE_ECB_ENC : MODE_ECB_DEC, in, 16ull * nblocks, 16ull * nblocks, out,
                      16ull * nblocks, nblocks, 0, nullptr, nullptr);
}

int fpnn_aes_cbc_host(fpnn_aes_engine *e, const fpnn_aes_schedule *ctx, int encrypt, const uint8_t *in, uint8_t *out,
                      size_t len, uint8_t ivec[16]) {
    if (!e || !ctx || !ivec || (len && (!in || !out))) return FPNN_AES_ERR_ARG;
    if (!valid_rounds(ctx->nrounds)) return FPNN_AES_ERR_KEYLEN;
    if (!len) return FPNN_AES_OK;
    const uint64_t nb = (len + 15) / 16, whole = 16 * nb;
    if (encrypt)  // reads len bytes (the last block zero-padded), writes whole blocks
        return modes_call(e, ctx, MODE_CBC_ENC, in, len, whole, out, whole, nb, len, ivec, nullptr);
    // decrypt reads whole blocks, writes len bytes; ivec := the last ciphertext block
    uint8_t last[16];
    memcpy(last, in + whole - 16, 16);  // before an in-place call overwrites it
    const int rc = modes_call(e, ctx, MODE_CBC_DEC, in, whole, whole, out, len, nb, len, ivec, nullptr);
    if (rc == FPNN_AES_OK) memcpy(ivec, last, 16);
    return rc;
}

int fpnn_aes_ofb_host(fpnn_aes_engine *e, const fpnn_aes_schedule *ctx, const uint8_t *in, uint8_t *out, size_t len,
                      uint8_t ivec[16], size_t *p_num) {
    if (!e || !ctx || !ivec || !p_num || (len && (!in || !out))) return FPNN_AES_ERR_ARG;
    if (!valid_rounds(ctx->nrounds)) return FPNN_AES_ERR_KEYLEN;
    if (*p_num > 15) return FPNN_AES_ERR_ARG;
    if (!len) return FPNN_AES_OK;
    return modes_call(e, ctx, MODE_OFB, in, len, len, out, len, 0, len, ivec, p_num);
}

int fpnn_aes_cfb_host(fpnn_aes_engine *e, const fpnn_aes_schedule *ctx, int encrypt, const uint8_t *in,
                      uint8_t *out, size_t len, uint8_t ivec[16], size_t *p_num) {
    if (!e || !ctx || !ivec || !p_num || (len && (!in || !out))) return FPNN_AES_ERR_ARG;
    if (int rc = debug_fail_point()) return rc;
    const int nr = ctx->nrounds;
    if (nr != 10 && nr != 12 && nr != 14) return FPNN_AES_ERR_KEYLEN;
    if (*p_num > 15) return FPNN_AES_ERR_ARG;
    if (len == 0) return FPNN_AES_OK;
    if (len > 0xffffffffull) return FPNN_AES_ERR_RANGE;
    if (len <= kSmallMaxBytes && small_enabled()) return cfb_small(e, ctx, encrypt != 0, in, out, len, ivec, p_num);
    DeviceGuard g(e->device);
    // staging layout: [DevKey 272][iv 16][pos 4 | pad 12][payload len] ... [out len]
    const uint64_t hdr = sizeof(DevKey) + 32;
    const uint64_t pay = (len + 15) & ~15ull;
    if (int rc = stage_reserve(e, hdr + 2 * pay)) return rc;
    devkey_from_schedule(reinterpret_cast<DevKey *>(e->h_stage), ctx);
    uint8_t *h_iv = e->h_stage + sizeof(DevKey);
    uint32_t *h_pos = reinterpret_cast<uint32_t *>(h_iv + 16);
    memcpy(h_iv, ivec, 16);
    *h_pos = (uint32_t)*p_num;
    memcpy(e->h_stage + hdr, in, len);
    // (Letting the kernels read and write the pinned staging block directly instead of the
    // three copies measured the same per-call time, 71 / 32 us: the launches and the sync
    // are the cost, not the copies.)
    HIP_TRY(hipMemcpyAsync(e->d_stage, e->h_stage, hdr + len, hipMemcpyHostToDevice, e->stream));

    fpnn_aes_keyset ks;
    ks.e = e;
    ks.device = e->device;
    ks.d_keys = reinterpret_cast<DevKey *>(e->d_stage);
    ks.count = 1;
    ks.nrounds = nr;
    ks.keylen = (uint32_t)(nr - 6) * 4;
    uint8_t *d_iv = e->d_stage + sizeof(DevKey);
    uint32_t *d_pos = reinterpret_cast<uint32_t *>(d_iv + 16);
    fpnn_aes_batch b;
    memset(&b, 0, sizeof b);
    b.in = e->d_stage + hdr;
    b.out = e->d_stage + hdr + pay;
    b.count = 1;
    b.uniform_len = (uint32_t)len;
    b.stride = 0;
    b.keys = &ks;
    int rc = encrypt ? run_encrypt(e, &b, d_iv, d_pos, true) : run_decrypt(e, &b, d_iv, d_pos, true);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(h_iv, d_iv, 32, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(e->h_stage + hdr + pay, e->d_stage + hdr + pay, len, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (int rf = stream_idle(e)) return rf;
    memcpy(out, e->h_stage + hdr + pay, len);
    memcpy(ivec, h_iv, 16);
    *p_num = *h_pos;
    return FPNN_AES_OK;
}

int fpnn_aes_device_alloc(fpnn_aes_engine *e, size_t bytes, void **out) {
    if (!e || !out) return FPNN_AES_ERR_ARG;
    *out = nullptr;
    DeviceGuard g(e->device);
    HIP_TRY(hipMalloc(out, bytes ? bytes : 1));
    return FPNN_AES_OK;
}

int fpnn_aes_device_free(fpnn_aes_engine *e, void *p) {
    if (!e) return FPNN_AES_ERR_ARG;
    if (!p) return FPNN_AES_OK;
    DeviceGuard g(e->device);
    HIP_TRY(hipFree(p));
    return FPNN_AES_OK;
}

int fpnn_aes_pinned_alloc(fpnn_aes_engine *e, size_t bytes, void **out) {
    if (!e || !out) return FPNN_AES_ERR_ARG;
    *out = nullptr;
    DeviceGuard g(e->device);
    HIP_TRY(pinned_host_alloc(e->numa.node, out, bytes ? bytes : 1));
    return FPNN_AES_OK;
}

int fpnn_aes_engine_numa(fpnn_aes_engine *e, int *node, int *device_node, int *ncpus) {
    if (!e) return FPNN_AES_ERR_ARG;
    if (node) *node = e->numa.node;
    if (device_node) *device_node = e->numa.device_node;
    if (ncpus) *ncpus = e->numa.ncpus;
    g_last_error = e->numa.why;
    return FPNN_AES_OK;
}

int fpnn_aes_pinned_free(fpnn_aes_engine *e, void *p) {
    if (!e) return FPNN_AES_ERR_ARG;
    if (!p) return FPNN_AES_OK;
    DeviceGuard g(e->device);
    HIP_TRY(hipHostFree(p));
    return FPNN_AES_OK;
}

int fpnn_aes_copy_async(fpnn_aes_engine *e, void *dst, const void *src, size_t bytes) {
    if (!e || (bytes && (!dst || !src))) return FPNN_AES_ERR_ARG;
    if (!bytes) return FPNN_AES_OK;
    DeviceGuard g(e->device);
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, e->stream));
    return FPNN_AES_OK;
}

int fpnn_aes_fill_synthetic(fpnn_aes_engine *e, uint8_t *dst, uint64_t nbytes, uint64_t seed, uint64_t byte_offset) {
    if (!e || (nbytes && !dst)) return FPNN_AES_ERR_ARG;
    DeviceGuard g(e->device);
    HIP_TRY(launch_fill_synthetic(dst, nbytes, seed, byte_offset, e->num_cus * 8, e->stream));
    return FPNN_AES_OK;
}

int fpnn_aes_engine_set_timing(fpnn_aes_engine *e, int enable) {
    if (!e) return FPNN_AES_ERR_ARG;
    e->timing = enable != 0;
    return FPNN_AES_OK;
}

int fpnn_aes_engine_kernel_stats(fpnn_aes_engine *e, int which, uint64_t *launches, double *total_ms) {
    if (!e || which < 0 || which > 1 || !launches || !total_ms) return FPNN_AES_ERR_ARG;
    DeviceGuard g(e->device);
    HIP_TRY(hipStreamSynchronize(e->stream));
    double sum = 0;
    for (size_t i = 0; i < e->ev_used[which]; i++) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, e->ev[which][i].beg, e->ev[which][i].end));
        sum += ms;
    }
    *launches = e->ev_used[which];
    *total_ms = sum;
    return FPNN_AES_OK;
}

const char *fpnn_aes_engine_last_kernel(fpnn_aes_engine *e, int which) {
    if (!e || which < 0 || which > 2) return "";
    if (which == FPNN_AES_K_HOST) return e->host_path;
    return e->last_kernel[which];
}

int fpnn_aes_engine_reset_stats(fpnn_aes_engine *e) {
    if (!e) return FPNN_AES_ERR_ARG;
    e->ev_used[0] = e->ev_used[1] = 0;
    return FPNN_AES_OK;
}

}  // extern "C"

// ---- ECDH key derivation (include/fpnn_ecdh.h, k_ecdh.hip) -------------------------------
namespace {

int ecdh_const(int curve, EccConst &c) {
    if (!ecc_fill_const(curve, c)) {
        g_last_error = "unknown ECDH curve";
        return FPNN_AES_ERR_ARG;
    }
    return FPNN_AES_OK;
}

bool aligned4(const void *p) { return ((uintptr_t)p & 3u) == 0; }

// the ecdh scratch held derived keys (or a private key): zero the bytes the call used, queued behind
// their last reader on the engine's stream.
int ecdh_wipe(fpnn_aes_engine *e, size_t bytes) {
    if (!e->ecdh.p || !bytes) return FPNN_AES_OK;
    DeviceGuard g(e->device);
    HIP_TRY(hipMemsetAsync(e->ecdh.p, 0, std::min<uint64_t>(bytes, e->ecdh.cap), e->stream));
    return FPNN_AES_OK;
}

int ecdh_launch(fpnn_aes_engine *e, int curve, const EccConst &c, const EcdhJob &j) {
    if (j.count == 0) return FPNN_AES_OK;
    if (!aligned4(j.priv) || !aligned4(j.pub) || !aligned4(j.key_out) || !aligned4(j.iv_out) ||
        !aligned4(j.pub_out)) {
        g_last_error = "ECDH device buffers must be 4-byte aligned";
        return FPNN_AES_ERR_ARG;
    }
    DeviceGuard g(e->device);
    const BatchScope batch_scope(e);  // (an early return clears the pending flag)
    HIP_TRY(launch_ecdh(c, j, curve, e->stream));
    batch_queued(e);
    return FPNN_AES_OK;
}

}  // namespace

extern "C" {

int fpnn_ecdh_curve(const char *name) {
    if (!name) return -1;
    for (int i = 0; i < ECC_NCURVES; i++)
        if (strcmp(name, ecc_curve_info(i).name) == 0) return i;
    return -1;
}

int fpnn_ecdh_secret_len(int curve) {
    return curve >= 0 && curve < ECC_NCURVES ? ecc_curve_info(curve).num_bytes : -1;
}

int fpnn_ecdh_private_len(int curve) {
    return curve >= 0 && curve < ECC_NCURVES ? (ecc_curve_info(curve).num_n_bits + 7) / 8 : -1;
}

const char *fpnn_ecdh_curve_name(int curve) {
    return curve >= 0 && curve < ECC_NCURVES ? ecc_curve_info(curve).name : nullptr;
}

int fpnn_ecdh_random_private(int curve, uint8_t *out) {
    EccConst c;
    if (!out || !ecc_fill_const(curve, c)) return 0;
    const int nw = c.nw, bits = c.num_n_bits;
    for (int tries = 0; tries < 64; tries++) {
        uint32_t k[8] = {0};
        size_t got = 0;
        while (got < sizeof(uint32_t) * nw) {
            const ssize_t r = getrandom(reinterpret_cast<uint8_t *>(k) + got, sizeof(uint32_t) * nw - got, 0);
            if (r < 0) {
                if (errno == EINTR) continue;
                return 0;
            }
            got += (size_t)r;
        }
        if (bits < 32 * nw) k[nw - 1] &= 0xFFFFFFFFu >> (32 * nw - bits);
        bool zero = true, below = false, decided = false;
        for (int w = nw - 1; w >= 0; w--) {
            zero = zero && k[w] == 0;
            if (!decided && k[w] != c.n[w]) {
                below = k[w] < c.n[w];
                decided = true;
            }
        }
        if (zero || !below) continue;
        const int pb = c.private_bytes;
        for (int i = 0; i < pb; i++) out[i] = (uint8_t)(k[(pb - 1 - i) / 4] >> (8 * ((pb - 1 - i) % 4)));
        return 1;
    }
    return 0;
}

int fpnn_ecdh_calc_keys(fpnn_aes_engine *e, int curve, const uint8_t *private_key, const uint8_t *peer_public,
                        uint32_t count, int keylen, uint8_t *keys, uint8_t *ivs, uint8_t *ok) {
    if (!e || !private_key || (count && (!peer_public || !keys || !ivs || !ok))) return FPNN_AES_ERR_ARG;
    if (keylen != 16 && keylen != 32) return FPNN_AES_ERR_KEYLEN;
    EccConst c;
    int rc = ecdh_const(curve, c);
    if (rc) return rc;
    ecc_set_uniform_scalar(c, private_key);
    EcdhJob j{};
    j.pub = peer_public;
    j.count = count;
    j.mode = ECDH_KEYS;
    j.keylen = keylen;
    j.key_out = keys;
    j.iv_out = ivs;
    j.ok_out = ok;
    return ecdh_launch(e, curve, c, j);
}

int fpnn_ecdh_calc_keys_client(fpnn_aes_engine *e, int curve, const uint8_t *private_keys,
                               const uint8_t *server_public, uint32_t count, int keylen, uint8_t *keys,
                               uint8_t *ivs, uint8_t *ok) {
    if (!e || !server_public || (count && (!private_keys || !keys || !ivs || !ok))) return FPNN_AES_ERR_ARG;
    if (keylen != 16 && keylen != 32) return FPNN_AES_ERR_KEYLEN;
    EccConst c;
    int rc = ecdh_const(curve, c);
    if (rc) return rc;
    ecc_set_uniform_point(c, server_public);
    EcdhJob j{};
    j.priv = private_keys;
    j.count = count;
    j.mode = ECDH_KEYS;
    j.keylen = keylen;
    j.key_out = keys;
    j.iv_out = ivs;
    j.ok_out = ok;
    return ecdh_launch(e, curve, c, j);
}

int fpnn_ecdh_public_keys(fpnn_aes_engine *e, int curve, const uint8_t *private_keys, uint32_t count,
                          uint8_t *public_keys, uint8_t *ok) {
    if (!e || (count && (!private_keys || !public_keys || !ok))) return FPNN_AES_ERR_ARG;
    EccConst c;
    int rc = ecdh_const(curve, c);  // px, py = G
    if (rc) return rc;
    EcdhJob j{};
    j.priv = private_keys;
    j.count = count;
    j.mode = ECDH_PUBLIC;
    j.pub_out = public_keys;
    j.ok_out = ok;
    return ecdh_launch(e, curve, c, j);
}

int fpnn_ecdh_keyset(fpnn_aes_engine *e, int curve, const uint8_t *private_key, const uint8_t *peer_public,
                     uint32_t count, int keylen, uint8_t *ok, fpnn_aes_keyset **out) {
    if (!e || !out || count == 0) return FPNN_AES_ERR_ARG;
    *out = nullptr;
    if (keylen != 16 && keylen != 32) return FPNN_AES_ERR_KEYLEN;
    DeviceGuard g(e->device);
    const size_t kb = (size_t)count * keylen, ib = (size_t)count * 16;
    int rc = e->ecdh.ensure(e, kb + ib + count);  // keys | ivs | ok, engine scratch
    if (rc) return rc;
    uint8_t *tmp = e->ecdh.p;
    rc = fpnn_ecdh_calc_keys(e, curve, private_key, peer_public, count, keylen, tmp, tmp + kb, ok ? ok : tmp + kb + ib);
    if (!rc) rc = fpnn_aes_keyset_create(e, count, (size_t)keylen, tmp, tmp + kb, 0, out);  // synchronizes
    const int wrc = ecdh_wipe(e, kb + ib + count);
    return rc ? rc : wrc;
}

int fpnn_ecdh_accept(fpnn_aes_engine *e, int curve, const uint8_t *private_key, const uint8_t *peer_public,
                     uint32_t count, fpnn_aes_keyset *ks, uint32_t first, const uint32_t *slots, uint32_t slot_bound,
                     uint8_t *ok) {
    if (!e || !private_key || !ks || ks->e != e || (count && !peer_public)) return FPNN_AES_ERR_ARG;
    if (ks->keylen != 16 && ks->keylen != 32) return FPNN_AES_ERR_KEYLEN;
    if (fpnn_ecdh_secret_len(curve) < 0) {
        g_last_error = "unknown ECDH curve";
        return FPNN_AES_ERR_ARG;
    }
    if (count == 0) return FPNN_AES_OK;
    KeyTableArgs a;
    int rc = keytable_args(ks, first, count, slots, slot_bound, a);  // (grows the table when the bound asks for it)
    if (rc) return rc;
    DeviceGuard g(e->device);
    const int keylen = (int)ks->keylen;
    const size_t kb = (size_t)count * keylen, ib = (size_t)count * 16;
    rc = scratch_ensure(e, need_ecdh_accept(count, (uint64_t)keylen));  // keys | ivs | ok, engine scratch
    if (rc) return rc;
    uint8_t *tmp = e->ecdh.p, *okp = ok ? ok : tmp + kb + ib;
    rc = fpnn_ecdh_calc_keys(e, curve, private_key, peer_public, count, keylen, tmp, tmp + kb, okp);
    if (!rc) {
        a.raw = tmp;
        a.ivs = tmp + kb;
        a.ok = okp;
        rc = keytable_run(ks, a, true);
    }
    const int wrc = ecdh_wipe(e, kb + ib + count);  // behind k_set_keys, the scratch's last reader
    return rc ? rc : wrc;
}

int fpnn_ecdh_calc_keys_host(fpnn_aes_engine *e, int curve, const uint8_t *private_key, const uint8_t *peer_public,
                             uint32_t count, int keylen, uint8_t *keys, uint8_t *ivs, uint8_t *ok) {
    if (!e || !private_key || (count && (!peer_public || !keys || !ivs || !ok))) return FPNN_AES_ERR_ARG;
    if (keylen != 16 && keylen != 32) return FPNN_AES_ERR_KEYLEN;
    const int sl = fpnn_ecdh_secret_len(curve);
    if (sl < 0) return FPNN_AES_ERR_ARG;
    if (count == 0) return FPNN_AES_OK;
    DeviceGuard g(e->device);
    const size_t pb = (size_t)count * 2 * sl, kb = (size_t)count * keylen, ib = (size_t)count * 16;
    int rc = e->ecdh.ensure(e, pb + kb + ib + count);  // peers | keys | ivs | ok
    if (rc) return rc;
    uint8_t *d = e->ecdh.p;
    do {
        hipError_t err = hipMemcpyAsync(d, peer_public, pb, hipMemcpyHostToDevice, e->stream);
        if (err != hipSuccess) { rc = hip_fail(err, "ecdh upload"); break; }
        if ((rc = fpnn_ecdh_calc_keys(e, curve, private_key, d, count, keylen, d + pb, d + pb + kb,
                                      d + pb + kb + ib)))
            break;
        err = hipMemcpyAsync(keys, d + pb, kb, hipMemcpyDeviceToHost, e->stream);
        if (err == hipSuccess) err = hipMemcpyAsync(ivs, d + pb + kb, ib, hipMemcpyDeviceToHost, e->stream);
        if (err == hipSuccess) err = hipMemcpyAsync(ok, d + pb + kb + ib, count, hipMemcpyDeviceToHost, e->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
        if (err != hipSuccess) { rc = hip_fail(err, "ecdh download"); break; }
    } while (0);
    const int wrc = ecdh_wipe(e, pb + kb + ib + count);
    return rc ? rc : wrc;
}

int fpnn_ecdh_calc_key_host(fpnn_aes_engine *e, const char *curve, const uint8_t *private_key, size_t private_len,
                            const uint8_t *peer_public, size_t peer_len, int keylen, uint8_t *key, uint8_t *iv) {
    if (!e) return FPNN_AES_ERR_ARG;
    // ECCKeyExchange::init + calcKey's own checks, in the reference's order
    const int cv = fpnn_ecdh_curve(curve);
    if (cv < 0 || (int)private_len != fpnn_ecdh_private_len(cv) || !private_key) return 0;
    if ((int)peer_len != 2 * fpnn_ecdh_secret_len(cv) || !peer_public) return 0;
    if (keylen != 16 && keylen != 32) return 0;
    if (!key || !iv) return FPNN_AES_ERR_ARG;
    DeviceGuard g(e->device);
    int rc = e->ecdh.ensure(e, 64 + 32 + 16 + 16);  // peer (<= 64) | key (32) | iv (16) | ok
    if (rc) return rc;
    uint8_t *d = e->ecdh.p;
    uint8_t res[32 + 16 + 1];
    do {
        hipError_t err = hipMemcpyAsync(d, peer_public, peer_len, hipMemcpyHostToDevice, e->stream);
        if (err != hipSuccess) { rc = hip_fail(err, "ecdh upload"); break; }
        if ((rc = fpnn_ecdh_calc_keys(e, cv, private_key, d, 1, keylen, d + 64, d + 96, d + 112))) break;
        err = hipMemcpyAsync(res, d + 64, sizeof res, hipMemcpyDeviceToHost, e->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
        if (err != hipSuccess) { rc = hip_fail(err, "ecdh download"); break; }
    } while (0);
    const int wrc = ecdh_wipe(e, 64 + 32 + 16 + 16);
    if (rc || wrc) return rc ? rc : wrc;
    if (!res[48]) return 0;
    memcpy(key, res, (size_t)keylen);
    memcpy(iv, res + 32, 16);
    return 1;
}

int fpnn_ecdh_public_key_host(fpnn_aes_engine *e, int curve, const uint8_t *private_key, uint8_t *public_key) {
    if (!e || !private_key || !public_key) return FPNN_AES_ERR_ARG;
    const int pl = fpnn_ecdh_private_len(curve), sl = fpnn_ecdh_secret_len(curve);
    if (pl < 0) return FPNN_AES_ERR_ARG;
    DeviceGuard g(e->device);
    int rc = e->ecdh.ensure(e, 32 + 64 + 16);  // private (<= 32) | public (<= 64) | ok
    if (rc) return rc;
    uint8_t *d = e->ecdh.p;
    uint8_t res[64 + 1];
    do {
        hipError_t err = hipMemcpyAsync(d, private_key, (size_t)pl, hipMemcpyHostToDevice, e->stream);
        if (err != hipSuccess) { rc = hip_fail(err, "ecdh upload"); break; }
        if ((rc = fpnn_ecdh_public_keys(e, curve, d, 1, d + 32, d + 96))) break;
        err = hipMemcpyAsync(res, d + 32, 64, hipMemcpyDeviceToHost, e->stream);
        if (err == hipSuccess) err = hipMemcpyAsync(res + 64, d + 96, 1, hipMemcpyDeviceToHost, e->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
        if (err != hipSuccess) { rc = hip_fail(err, "ecdh download"); break; }
    } while (0);
    const int wrc = ecdh_wipe(e, 32 + 64 + 16);  // (the private key went through it)
    if (rc || wrc) return rc ? rc : wrc;
    memcpy(public_key, res, (size_t)(2 * sl));
    return res[64] ? 1 : 0;
}

}  // extern "C"
