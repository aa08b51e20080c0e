// dispatch_plan.hpp -- which kernel a device batch call runs on, in one place: everything the
// host decides about a call before anything is queued (kernel family, layout, key mode, grid
// and workgroup, whether a length order or a boundary save runs first, the scratch the route
// needs), and nothing that has an effect.  The engine (engine.hip) checks the arguments, asks
// for the route, grows the scratch, sets up the audit and launches; the launchers (k_*.hip)
// still pick their own variant inside a family (K1d / K1k / K1 in k_decrypt.hip).  The
// thresholds are the ones include/fpnn_aes.h promises; tests/cpp/dispatch_plan_test.cpp pins
// every one of them at its edge.  Plain C++, no HIP.
#pragma once

#include <cstdint>

#include "scratch_plan.hpp"

namespace fpnn_aes {

constexpr uint32_t F_WIRE_PREFIX = 0x1u;     // == FPNN_AES_F_WIRE_PREFIX
constexpr uint32_t F_ALIGN_CHUNKS = 0x100u;  // internal (engine -> K2): line-align the chunks of each chain

// UNIFORM: segment i at i*stride, uniform_len bytes, key slot 0.  FULL: the same with
// uniform_len % 16 == 0 in package mode, so no block is partial (decrypt skips the
// byte-granular head/tail paths); with KEY_LANE, FULL also means dense (stride ==
// uniform_len) with key_slot[] holding one slot per packet (K1d keyed when
// uniform_len % 1024 == 0, else K1k).
// GENERAL: offset/length/slot arrays (decrypt: K1r, k_ragged.hip).
enum Layout { LAYOUT_UNIFORM = 0, LAYOUT_GENERAL = 1, LAYOUT_FULL = 2 };
// KEY_SLOT (stream encrypt only): per-lane keys as KEY_LANE, and the segment's (iv, pos)
// lives at its key slot -- KBatch::state_slot; launch_encrypt_*_at (kernels.hpp).
enum KeyMode { KEY_UNIFORM = 0, KEY_LANE = 1, KEY_SLOT = 2 };

// What the choice reads of an fpnn_aes_batch: sizes, and which arrays are there.
struct BatchShape {
    uint64_t count, stride;
    uint32_t uniform_len, max_len, flags;
    bool in_off, out_off, len, key_slot;  // the array is given
    uint32_t nkeys;                       // keys->count
    bool inplace;                         // in == out
};

// package or stream; at: slot-addressed (fpnn_aes_stream_*_at)
struct CallKind {
    bool stream, at;
};

// what the choice depends on besides the call: the device, the kernels' constants, and the
// engine's Variant (kernels.hpp) where the choice reads it
struct DispatchShape {
    ScratchShape scratch;                  // (num_cus: scratch.num_cus)
    int threads;                           // kThreads
    uint32_t frame_max_bytes;              // kFrameMaxBytes
    int hyb_long, hyb_quad_waves, hyb_force;  // Variant
    uint32_t (*length_bucket_of)(uint64_t);   // length_bucket_of (k_support.hip)
};

// the smallest power-of-two workgroup (at least one wave) that still spreads `lanes` over
// every CU, and its grid: at most one workgroup per CU (further work grid-strides)
struct Spread {
    int threads, grid;
};
inline Spread spread_over_cus(const DispatchShape &d, uint64_t lanes) {
    const uint64_t cus = d.scratch.num_cus;
    int threads = 64;
    while (threads < d.threads && (uint64_t)threads * cus < lanes) threads *= 2;
    const uint64_t want = (lanes + threads - 1) / threads;
    return {threads, (int)(want < cus ? (want ? want : 1) : cus)};
}

inline bool is_uniform_layout(const BatchShape &b) { return !b.in_off && !b.out_off && !b.len && !b.key_slot; }

// per-segment keys only when the table has more than one: key_slot[] over a one-key table is
// KEY_UNIFORM (and still LAYOUT_GENERAL: is_uniform_layout looks at the array alone)
inline bool per_key(const BatchShape &b) { return b.key_slot && b.nkeys > 1; }
inline KeyMode key_mode(const BatchShape &b) { return per_key(b) ? KEY_LANE : KEY_UNIFORM; }

// ceil(2^64 / d) for 2 <= d < 2^32 (no route divides by 1: d == 1 wraps to 0)
inline uint64_t magic_for(uint32_t d) {
    const unsigned __int128 one = (unsigned __int128)1 << 64;
    return (uint64_t)((one + d - 1) / d);
}

// ---- encrypt (fpnn_aes_package_encrypt, fpnn_aes_stream_encrypt, fpnn_aes_stream_encrypt_at) ----

enum EncryptFamily {
    ENC_CHAINS,  // K2: one lane per chain, 8-block chunks
    ENC_COOP,    // K2c: one quad per chain
    ENC_HYBRID,  // K2h: short chains one per lane, the longest on quads, both from work queues
    ENC_FRAMES   // K2s-DB: one lane per chain, whole frames at once
};

struct EncryptRoute {
    EncryptFamily family;
    Layout layout;
    KeyMode km;           // KEY_SLOT for an _at call: the family's kernel in its slot form
    int threads, grid;    // K2h and K2s-DB: whole workgroups, one per CU
    bool order;           // a length order is queued first (ragged: the longest chains first)
    bool order_pos;       // it orders by position too (bucket sizes read pos_state)
    bool order_zeroes;    // its scatter zeroes the length-order block (K2c follows; K2h zeroes it itself)
    uint32_t flags;       // ORed into KBatch::flags: F_ALIGN_CHUNKS or nothing
    uint32_t long_bucket, quad_waves;  // K2h: chains in buckets <= long_bucket on quads
    bool wire;            // K2s-DB: the 4-byte length prefix
    ScratchNeed need;
};

inline EncryptRoute encrypt_route(const DispatchShape &d, const BatchShape &b, CallKind c) {
    EncryptRoute r = {};
    r.layout = is_uniform_layout(b) ? LAYOUT_UNIFORM : LAYOUT_GENERAL;
    r.km = c.at ? KEY_SLOT : key_mode(b);
    // Few chains (fewer than the lanes of a full chip) or ragged lengths: one quad per
    // chain (K2c); otherwise one lane per chain with 8-block chunks (K2).
    const uint64_t full_chip = d.scratch.num_cus * (uint64_t)d.threads;

    // Ragged package batches of many short frames (the caller's max_len bound): one lane
    // per chain in grid-stride order (K2) -- Q1, 2 M x 145-B quests of 16 384 keyed
    // connections: 705 against K2h's 343 GiB/s (its work-queue atomics and length-order
    // indirection per chain; profiles/r05/ab_k2_short, ab_k2_align), from one chain per
    // GPU lane on (Q1h, 2 per lane: K2 767-770 against K2h 182-184 GiB/s,
    // profiles/r05/ab_k2_short_min).  Without a bound K2h, which also balances
    // Zipf-like lengths (C4 on K2: 88 GiB/s).
    const bool k2_ragged = b.len && !c.stream && b.max_len && b.max_len <= 2048 && b.count >= full_chip;
    if ((b.count < full_chip || b.len) && !k2_ragged) {
        const uint64_t lanes = 4 * b.count;
        // ragged with more chains than quads: K2h; with fewer every quad holds at most one
        // chain and K2c's grid stride is cheaper
        const bool hybrid = b.len && b.count > 1 && (lanes > full_chip || d.hyb_force);
        if (b.len && b.count > 1) {  // ragged: visit the longest chains first, similar lengths per wave
            r.order = true;
            // the slot form orders by length alone (the position is the slot's: kernels.hpp)
            r.order_pos = c.stream && !c.at;
            r.order_zeroes = !hybrid;
            r.need = need_encrypt_ragged(d.scratch, b.count, hybrid);
        }
        if (!hybrid) {
            const Spread sp = spread_over_cus(d, lanes);
            r.family = ENC_COOP;
            r.threads = sp.threads;
            r.grid = sp.grid;
            return r;
        }
        r.family = ENC_HYBRID;
        r.threads = d.threads;
        r.grid = (int)d.scratch.num_cus;
        r.flags = F_ALIGN_CHUNKS;
        r.long_bucket = d.length_bucket_of((uint64_t)d.hyb_long);
        r.quad_waves = (uint32_t)d.hyb_quad_waves;
        if (b.flags & F_WIRE_PREFIX) {
            // wire frames (htole32(len) || C): every chain on quads (k_hybrid.hip's
            // launcher takes the quads-only kernel for them)
            r.long_bucket = 127;
            r.quad_waves = 16;
        }
        return r;
    }
    // (not for ragged batches: a few 16-B aligned frames per wave made the whole wave run
    // their singles)
    if (!b.len) r.flags = F_ALIGN_CHUNKS;
    if (k2_ragged && b.max_len <= d.frame_max_bytes) {  // FPNN's quests: whole frames at once
        r.family = ENC_FRAMES;
        r.threads = d.threads;
        r.grid = (int)d.scratch.num_cus;
        r.wire = (b.flags & F_WIRE_PREFIX) != 0;
        return r;
    }
    // One lane per chain.  Workgroup size: the smallest power of two (>= one wave) that
    // still spreads the chains over every CU -- with few chains (C3: 4096 streams) a
    // 1024-thread workgroup would pack them onto a handful of CUs whose LDS they then
    // saturate, while the rest of the chip idles.
    const Spread sp = spread_over_cus(d, b.count);
    r.family = ENC_CHAINS;
    r.threads = sp.threads;
    r.grid = sp.grid;
    return r;
}

// ---- decrypt (fpnn_aes_package_decrypt, fpnn_aes_stream_decrypt) ----

enum DecryptFamily {
    DEC_DENSE,   // K1 / K1d / K1k (launch_decrypt_blocks): every segment's block count known on the host
    DEC_FRAMES,  // D2s: one lane per frame
    DEC_RAGGED   // K1r: block map, plan and decrypt on the device
};

struct DecryptRoute {
    DecryptFamily family;
    Layout layout;
    KeyMode km;
    uint64_t total_blocks;  // dense: nb_uniform * count, fewer than 2^32
    uint32_t nb_uniform;
    uint64_t magic;         // magic_for(nb_uniform)
    // dense in place (in == out): a wave may overwrite the ciphertext block another wave's
    // lane 0 still needs, so the block before every 64-block chunk is saved first (K1r saves
    // its waves' boundaries in its plan in any case)
    bool boundary_save;
    uint64_t nchunks;
    int grid;
    ScratchNeed need;
};

inline DecryptRoute decrypt_route(const DispatchShape &d, const BatchShape &b, CallKind c) {
    DecryptRoute r = {};
    r.layout = LAYOUT_GENERAL;
    r.km = key_mode(b);
    r.grid = (int)d.scratch.num_cus;
    // Uniform layout: every segment has the same block count, known on the host.  (Never in
    // stream mode: positions differ per stream.)
    uint64_t nb = 0;
    if (is_uniform_layout(b) && !c.stream) {
        nb = ((uint64_t)b.uniform_len + 15) >> 4;
        if (nb > 1 && nb * b.count < (1ull << 32)) r.layout = (b.uniform_len & 15) == 0 ? LAYOUT_FULL : LAYOUT_UNIFORM;
    } else if (!c.stream && r.km == KEY_LANE && !b.in_off && !b.out_off && !b.len && b.uniform_len >= 32 &&
               b.uniform_len % 16 == 0 && b.stride == b.uniform_len) {
        // dense whole-block packets, one key slot each: K1d with a wave-uniform key per
        // step when packets are whole 64-block chunks (C5), K1k with per-lane keys
        // otherwise (U1)
        nb = b.uniform_len >> 4;
        if (nb * b.count < (1ull << 32)) r.layout = LAYOUT_FULL;
    }
    if (r.layout != LAYOUT_GENERAL) {
        r.family = DEC_DENSE;
        r.total_blocks = nb * b.count;
        r.nb_uniform = (uint32_t)nb;
        r.magic = magic_for((uint32_t)nb);
        r.nchunks = (r.total_blocks + 63) >> 6;
        if (b.inplace) {
            r.boundary_save = true;
            r.need = need_decrypt_dense_inplace(r.total_blocks);
        }
        const uint64_t want = (r.nchunks + 63) / 64;  // 16 waves per workgroup x up to 4 chunks per wave step
        const uint64_t cap = d.scratch.num_cus;
        r.grid = (int)(want < cap ? (want ? want : 1) : cap);
        return r;
    }
    // Ragged package batches of FPNN's quests (the caller's max_len bound, at least one frame
    // per GPU lane): one lane per frame, its blocks decrypted as independent AES passes from
    // registers (D2s).  K1r's 64-block chunks span ~7 frames and key slots there.
    if (!c.stream && b.len && b.max_len && b.max_len <= d.frame_max_bytes &&
        b.count >= d.scratch.num_cus * (uint64_t)d.threads) {
        r.family = DEC_FRAMES;
        return r;
    }
    // K1r: stream batches (which always come here) snapshot their state first
    r.family = DEC_RAGGED;
    r.need = need_decrypt_ragged(d.scratch, b.count, c.stream, b.in_off, b.len);
    return r;
}

// ---- many frames per stream in one call (fpnn_aes_stream_*_frames, *_frames_at) ----

struct FramesRoute {
    KeyMode km;         // an _at call: every stream's key from its slot, whatever the table's size
    int threads, grid;  // encrypt: K2f, one quad per stream, sized as K2c is
    ScratchNeed need;   // decrypt: K1r on a stream batch plus the per-segment state
};

inline FramesRoute frames_route(const DispatchShape &d, const BatchShape &b, bool at, uint64_t nstreams, bool encrypt) {
    FramesRoute r = {};
    r.km = (at || per_key(b)) ? KEY_LANE : KEY_UNIFORM;
    const Spread sp = spread_over_cus(d, 4 * nstreams);
    r.threads = sp.threads;
    r.grid = sp.grid;
    if (!encrypt) r.need = need_decrypt_frames(d.scratch, b.count, at, b.in_off, b.len);
    return r;
}

// ---- UDP v2 datagrams with data encryption (fpnn_aes_udp_encrypt / _decrypt, k_udp.hip) ----

struct UdpShape {
    uint64_t nconn, nsections;
    int nr_data, nr_pkg;  // rounds of the two tables (nr_data: 0 without a data table)
};

// What the two calls check of their arguments before anything else (include/fpnn_aes.h), as
// plain values: which pointers are there (addresses, for their alignment), the tables' sizes
// and rounds.  Returns UDP_ARGS_OK, or the public error the call returns.
struct UdpArgs {
    bool key_slot;   // b->key_slot given
    uint32_t flags;  // b->flags
    bool u;          // the fpnn_aes_udp_data itself is there
    bool data_keys, data_keys_same_engine;
    uint32_t nconn, nsections, slot_bound;
    uintptr_t first_dgram, conn_slot, iv_state, pos_state, first_section, sec_off, sec_len;
    uint32_t pkg_slots, data_slots;  // capacity of b->keys and of data_keys
    int nr_pkg, nr_data;             // their rounds
};
enum : int { UDP_ARGS_OK = 0, UDP_ARGS_KEYLEN = -1 /* FPNN_AES_ERR_KEYLEN */, UDP_ARGS_BAD = -2 /* FPNN_AES_ERR_ARG */ };

inline int udp_check_args(const UdpArgs &a) {
    if (a.key_slot || a.flags || !a.u) return UDP_ARGS_BAD;
    if (a.data_keys ? !a.data_keys_same_engine : a.nsections != 0) return UDP_ARGS_BAD;
    const auto bad4 = [](uintptr_t p) { return !p || (p & 3); };
    if (a.nconn && (bad4(a.first_dgram) || bad4(a.conn_slot) || bad4(a.pos_state) || !a.iv_state || (a.iv_state & 15)))
        return UDP_ARGS_BAD;
    if (a.nsections && (bad4(a.first_section) || bad4(a.sec_off) || bad4(a.sec_len))) return UDP_ARGS_BAD;
    if (a.first_section & 3) return UDP_ARGS_BAD;  // (optional without sections, aligned when given)
    if (a.slot_bound > a.pkg_slots || (a.data_keys && a.slot_bound > a.data_slots)) return UDP_ARGS_BAD;
    if (a.nr_pkg == 12 || (a.data_keys && a.nr_data == 12)) return UDP_ARGS_KEYLEN;
    return UDP_ARGS_OK;
}

struct UdpRoute {
    bool ok;              // both round counts are 10 or 14 (createPair makes 16- and 32-byte keys)
    int nr_data, nr_pkg;  // encrypt: K2u's template arguments (without a data table: the package table's twice)
    int threads, grid;    // encrypt: one quad per connection, sized as K2c is
    // decrypt: the descriptors derived on the device, the package decrypt of the datagrams (one key
    // slot each: decrypt_route with key_slot) and the slot-addressed *_frames decrypt of the
    // sections, which are segments of `out` by offset and length arrays
    DecryptRoute pkg;
    ScratchNeed need;
};

inline bool udp_rounds_ok(int nr) { return nr == 10 || nr == 14; }

// b: the datagram batch as the caller gave it (key_slot is null there)
inline UdpRoute udp_route(const DispatchShape &d, const BatchShape &b, const UdpShape &u, bool encrypt) {
    UdpRoute r = {};
    r.nr_pkg = u.nr_pkg;
    r.nr_data = u.nr_data ? u.nr_data : u.nr_pkg;
    r.ok = udp_rounds_ok(r.nr_pkg) && udp_rounds_ok(r.nr_data);
    if (!r.ok) return r;
    if (encrypt) {
        const Spread sp = spread_over_cus(d, 4 * u.nconn);
        r.threads = sp.threads;
        r.grid = sp.grid;
        return r;
    }
    BatchShape pb = b;
    pb.key_slot = true;
    r.pkg = decrypt_route(d, pb, {false, false});
    r.need = need_udp_decrypt(d.scratch, r.pkg.need, b.count, u.nsections, u.nconn);
    return r;
}

// ---- UDP v2 receive (fpnn_aes_udp_recv / _recv_take, k_udp_recv.hip) ----

enum : uint32_t { UDP_F_WALK_ONLY = 1u /* FPNN_AES_UDP_F_WALK_ONLY */, UDP_F_PLAIN = 2u /* FPNN_AES_UDP_F_PLAIN */ };

// What the two calls check beyond udp_check_args (include/fpnn_aes.h), as plain values.  take:
// fpnn_aes_udp_recv_take (flags 0).
struct UdpRecvArgs {
    UdpArgs udp;  // the batch and the fpnn_aes_udp_data, as for fpnn_aes_udp_decrypt
    bool take;
    uint32_t flags;
    bool in_place;  // b->in == b->out and no b->out_off
    uint32_t count, max_pkgs, max_sections, ntake;
    uintptr_t scan, pkgs, sections, first_take, take_list;
};

inline int udp_recv_check_args(const UdpRecvArgs &a) {
    // the sections are outputs: none may come in (checked first: udp_check_args would accept them)
    if (a.udp.u && (a.udp.nsections || a.udp.first_section || a.udp.sec_off || a.udp.sec_len)) return UDP_ARGS_BAD;
    if (const int rc = udp_check_args(a.udp); rc == UDP_ARGS_BAD) return rc;
    if (a.flags & ~(UDP_F_WALK_ONLY | UDP_F_PLAIN)) return UDP_ARGS_BAD;
    if (a.take && a.flags) return UDP_ARGS_BAD;
    if ((a.flags & UDP_F_PLAIN) && !a.in_place) return UDP_ARGS_BAD;
    if (!a.udp.data_keys && !(a.flags & UDP_F_WALK_ONLY)) return UDP_ARGS_BAD;
    if (!a.max_pkgs || !a.max_sections) return UDP_ARGS_BAD;
    if ((uint64_t)a.count * a.max_pkgs > UINT32_MAX || (uint64_t)a.count * a.max_sections > UINT32_MAX)
        return UDP_ARGS_BAD;
    if (a.take && (uint64_t)a.ntake * a.max_sections > UINT32_MAX) return UDP_ARGS_BAD;
    if (a.count && (!a.scan || (a.scan & 1) || !a.pkgs || (a.pkgs & 3) || !a.sections || (a.sections & 3)))
        return UDP_ARGS_BAD;
    if (a.ntake && (!a.first_take || (a.first_take & 3) || !a.take_list || (a.take_list & 3))) return UDP_ARGS_BAD;
    return udp_check_args(a.udp);  // (OK or KEYLEN: an argument error comes before a key length's)
}

struct UdpRecvRoute {
    bool ok;          // as UdpRoute::ok
    bool package;     // the package decrypt of the datagrams runs (not PLAIN, not recv_take)
    bool data;        // the data decrypt runs (not WALK_ONLY)
    uint64_t nseg;    // its segments: max_sections per datagram, or per taken package
    DecryptRoute pkg; // the package decrypt's route: udp_route's
    ScratchNeed need;
};

// b: the datagram batch as the caller gave it
inline UdpRecvRoute udp_recv_route(const DispatchShape &d, const BatchShape &b, const UdpShape &u, bool take,
                                   uint32_t flags, uint32_t max_sections, uint32_t ntake) {
    UdpRecvRoute r = {};
    r.package = !take && !(flags & UDP_F_PLAIN);
    r.data = !(flags & UDP_F_WALK_ONLY);
    r.ok = udp_rounds_ok(u.nr_pkg) && (!u.nr_data || udp_rounds_ok(u.nr_data));
    if (!r.ok) return r;
    r.nseg = r.data ? (uint64_t)(take ? ntake : b.count) * max_sections : 0;
    if (r.package) r.pkg = udp_route(d, b, {u.nconn, 0, u.nr_data, u.nr_pkg}, false).pkg;
    r.need = need_udp_decrypt(d.scratch, r.pkg.need, r.package ? b.count : 0, r.nseg, u.nconn);
    return r;
}

}  // namespace fpnn_aes
