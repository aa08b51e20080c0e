// scratch_plan.hpp -- the engine's device scratch in one place: which buffers there are, how a
// capacity grows, and how many elements of each buffer every call path needs.  The call paths
// (engine.hip) size their scratch through need_*, fpnn_aes_engine_reserve takes the element-wise
// maximum, so "after reserve() no call within the bounds allocates or memsets" is a property of
// this header (tests/cpp/scratch_plan_test.cpp).  Plain C++, no HIP.  Not covered by reserve:
// fr_off / fr_slot (fpnn_aes_package_recv needs count x max_frames entries, and max_frames is no
// reserve argument), sstate, and what the ECDH calls other than fpnn_ecdh_accept ask of ecdh.
#pragma once

#include <cstdint>

namespace fpnn_aes {

// Every growing scratch buffer: X(name, element type, zeroed when grown).  The engine holds one
// Scratch per line (engine_internal.hpp: e->bstart.p, e->bstart.cap); teardown and reserve walk
// this list, so a new buffer is one line here plus its users.  A zeroed buffer starts as
// zeros and is zeroed again by its last reader (kernels.hpp).
#define FPNN_AES_SCRATCH_BUFFERS(X)                                                                         \
    X(bstart, uint64_t, false)   /* K1r block map: first block of every segment, count + 1 entries */      \
    X(boundary, uint4, false)    /* K1 / K1d in place: the block before every 64-block chunk */            \
    X(snap_iv, uint4, false)     /* stream decrypt: the incoming (iv, pos), see KBatch::iv_snap */         \
    X(snap_pos, uint32_t, false)                                                                            \
    X(perm, uint32_t, false)     /* ragged encrypt: longest-first order */                                 \
    X(buckets, uint32_t, true)   /* the length-order block (kLengthOrderWords) */                          \
    X(fr_off, uint64_t, false)   /* package receive: absolute body offset per frame slot */                \
    X(fr_slot, uint32_t, false)  /* package receive: key slot per frame slot */                            \
    X(plan, RaggedPlan, false)   /* K1r: one entry per wave of the decrypt grid */                         \
    X(sink, uint4, false)        /* K1r, K2h: 2 x uint4 per wave, stores of lanes with nothing to store */ \
    X(desc_off, uint64_t, false) /* K1r: materialized in_off / len of stride / uniform batches */          \
    X(desc_len, uint32_t, false)                                                                            \
    X(sf_stream, uint32_t, false) /* *_frames decrypt, per segment: its stream, */                         \
    X(sf_prev, uint32_t, false)   /* the stream's last non-empty frame before it, */                       \
    X(sf_iv, uint4, false)        /* the state K1r exports for it */                                       \
    X(sf_pos, uint32_t, false)                                                                              \
    X(sf_slot, uint32_t, false)   /* and (_at calls) its key slot */                                       \
    X(lookback, uint64_t, true)  /* one-pass block map: tickets, epoch, tile status */                     \
    X(ecdh, uint8_t, false)      /* ECDH: peers | keys | ivs | ok, bytes (wiped by every call: ecdh_wipe) */ \
    X(sstate, uint8_t, false)    /* stream host frames: (iv, pos) of the call's streams, bytes */              \
    X(udp_off, uint64_t, false)  /* UDP decrypt: every section as a segment of `out`, its offset */          \
    X(udp_u32, uint32_t, false)  /* and: datagram key slots | section lengths | connection section ranges */

enum ScratchId {
#define X(name, type, zeroed) SC_##name,
    FPNN_AES_SCRATCH_BUFFERS(X)
#undef X
    kScratchBufs
};

// capacity (elements) once a buffer of capacity `cap` holds `need`: 1024 first, then doubling
inline uint64_t scratch_next_cap(uint64_t cap, uint64_t need) {
    if (need <= cap) return cap;
    uint64_t n = cap ? cap : 1024;
    while (n < need) n *= 2;
    return n;
}

struct ScratchNeed {  // elements per buffer (0: the path does not touch it)
    uint64_t n[kScratchBufs] = {};
};

inline ScratchNeed scratch_max(ScratchNeed a, const ScratchNeed &b) {
    for (int i = 0; i < kScratchBufs; i++) a.n[i] = b.n[i] > a.n[i] ? b.n[i] : a.n[i];
    return a;
}

struct ScratchShape {  // what the sizes depend on besides the call: the device, the kernels' constants
    uint64_t num_cus, waves;              // waves per workgroup of the AES kernels (kThreads / 64)
    uint64_t small_max;                   // block_map_small_max()
    uint64_t (*onepass_words)(uint64_t);  // block_map_onepass_words
    uint64_t length_order_words;          // kLengthOrderWords
};

// Ragged decrypt (K1r) of n segments.  stream: the state snapshot; in_off / len: the caller
// supplies that descriptor array (otherwise it is materialized).
inline ScratchNeed need_decrypt_ragged(const ScratchShape &s, uint64_t n, bool stream, bool in_off, bool len) {
    ScratchNeed r;
    r.n[SC_bstart] = n + 1;
    r.n[SC_plan] = s.num_cus * s.waves;
    r.n[SC_sink] = 2 * s.num_cus * s.waves;
    if (n > s.small_max) r.n[SC_lookback] = s.onepass_words(n);
    if (!in_off) r.n[SC_desc_off] = n;
    if (!len) r.n[SC_desc_len] = n;
    if (stream) r.n[SC_snap_iv] = r.n[SC_snap_pos] = n;
    return r;
}

// *_frames decrypt of n segments: K1r on a stream batch plus the per-segment state; slots: _at
inline ScratchNeed need_decrypt_frames(const ScratchShape &s, uint64_t n, bool slots, bool in_off, bool len) {
    ScratchNeed r = need_decrypt_ragged(s, n, true, in_off, len);
    r.n[SC_sf_stream] = r.n[SC_sf_prev] = r.n[SC_sf_iv] = r.n[SC_sf_pos] = n;
    if (slots) r.n[SC_sf_slot] = n;
    return r;
}

// ragged encrypt in length order; hybrid: K2h
inline ScratchNeed need_encrypt_ragged(const ScratchShape &s, uint64_t n, bool hybrid) {
    ScratchNeed r;
    r.n[SC_perm] = n;
    r.n[SC_buckets] = s.length_order_words;
    if (hybrid) r.n[SC_sink] = 2 * s.num_cus * s.waves;
    return r;
}

// in-place dense decrypt (K1 / K1d) of `blocks` blocks: one saved block per 64-block chunk
inline ScratchNeed need_decrypt_dense_inplace(uint64_t blocks) {
    ScratchNeed r;
    r.n[SC_boundary] = (blocks + 63) / 64;
    return r;
}

// fpnn_ecdh_accept of `count` peers: key | iv (16) | ok (1) each
inline ScratchNeed need_ecdh_accept(uint64_t count, uint64_t keylen) {
    ScratchNeed r;
    r.n[SC_ecdh] = count * (keylen + 16 + 1);
    return r;
}

// fpnn_aes_udp_decrypt of `dgrams` datagrams and `sections` data sections of `conns` connections: the
// derived descriptors (k_udp.hip, k_udp_expand), the package decrypt of the datagrams on its route
// (pkg: decrypt_route's need) and the slot-addressed *_frames decrypt of the sections, whose
// descriptor arrays are the derived ones.  fpnn_aes_udp_encrypt (K2u) needs no scratch.
// fpnn_aes_udp_recv / _recv_take (k_udp_recv.hip) are the same composition with the sections found
// on the device: `sections` is then max_sections per datagram (or per taken package) whatever the
// datagrams hold, 0 under WALK_ONLY; `dgrams` the datagrams the package decrypt runs over (0: PLAIN,
// or recv_take).  The same buffers in the same layout, so reserve's promise covers those calls
// when max_segments >= max(dgrams, segments, conns).
inline ScratchNeed need_udp_decrypt(const ScratchShape &s, const ScratchNeed &pkg, uint64_t dgrams, uint64_t sections,
                                    uint64_t conns) {
    ScratchNeed r = pkg;
    r.n[SC_udp_off] = sections;
    r.n[SC_udp_u32] = dgrams + sections + conns + 1;
    if (sections) r = scratch_max(r, need_decrypt_frames(s, sections, true, true, true));
    return r;
}

// fpnn_aes_engine_reserve: every path above at its bounds.  Two entries exceed the maximum, as
// reserve has always given them: look-back words also below small_max, one more boundary entry.
inline ScratchNeed need_reserve(const ScratchShape &s, uint64_t max_segments, uint64_t max_blocks) {
    ScratchNeed r = need_decrypt_ragged(s, max_segments, true, false, false);
    r = scratch_max(r, need_decrypt_frames(s, max_segments, true, false, false));
    r = scratch_max(r, need_encrypt_ragged(s, max_segments, true));
    r = scratch_max(r, need_decrypt_dense_inplace(max_blocks));
    r = scratch_max(r, need_ecdh_accept(max_segments, 32));
    // (the UDP decrypt's package step is a ragged or an in-place dense decrypt: both are above)
    r = scratch_max(r, need_udp_decrypt(s, ScratchNeed{}, max_segments, max_segments, max_segments));
    r.n[SC_lookback] = s.onepass_words(max_segments);
    r.n[SC_boundary] += 1;
    return r;
}

}  // namespace fpnn_aes
