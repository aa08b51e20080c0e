// kernels.hpp -- internal launch interface between the C-ABI (engine.hip) and the
// HIP kernels (k_encrypt.hip, k_decrypt.hip, k_support.hip).  Not installed; the public boundary is include/fpnn_aes.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aes_common.hpp"
#include "audit.hpp"
#include "dispatch_plan.hpp"

namespace fpnn_aes {

// (F_WIRE_PREFIX, F_ALIGN_CHUNKS, Layout and KeyMode: dispatch_plan.hpp, which chooses them)

// Kernel-side view of one batch (passed by value as the kernel argument).
struct KBatch {
    const uint8_t *in;
    uint8_t *out;
    uint64_t count;
    uint64_t stride;
    uint32_t uniform_len;
    uint32_t flags;
    const uint64_t *in_off;
    const uint64_t *out_off;
    const uint32_t *len;
    const uint32_t *key_slot;
    const DevKey *keys;
    uint8_t *iv_state;    // stream mode: 16 B per segment (in/out)
    uint32_t *pos_state;  // stream mode: CFB position per segment (in/out)
    const uint32_t *t0le; // 1 KiB T0 source for the LDS image
    // block map (decrypt)
    uint64_t total_blocks;   // uniform layout: exact; general: copy of *total_ptr
    uint32_t nb_uniform;     // uniform layout: blocks per segment
    // The slot form of the stream encrypt kernels (KEY_SLOT, fpnn_aes_stream_encrypt_at) reads no
    // block map; its three arguments share the storage of three block-map fields, so the kernel
    // argument of every other kernel keeps its layout:
    //   state_slot[s]  segment s's key-table slot: its key is keys[state_slot[s]] and its state
    //                  entry state_slot[s] of iv_state / pos_state (key_slot is null)
    //   slot_bound     entries of the state arrays (at most the table's slots)
    //   slot_fault     gets kFaultKeySlot when a state_slot[] entry lies at or past slot_bound
    union {
        uint32_t runs;       // K1r: interior runs on (Variant::k1r_runs)
        uint32_t slot_bound;
    };
    uint64_t magic;          // ceil(2^64 / nb_uniform)
    union {
        const uint64_t *bstart;  // general: first virtual block of each segment (count + 1)
        const uint32_t *state_slot;
    };
    union {
        const uint4 *boundary;   // in-place: Cx block preceding each 64-block chunk
        uint32_t *slot_fault;
    };
    // stream decrypt: the (iv, pos) state as it was when the call was queued.  The
    // kernel writes the new state into iv_state/pos_state while other waves may still
    // be reading the old one, so every read goes to this snapshot.
    const uint4 *iv_snap;
    const uint32_t *pos_snap;
    // encrypt of ragged batches: segment visiting order (longest first), or null
    const uint32_t *perm;
    // package mode: E_k(IV) per key slot (the first keystream block of every chain of the
    // slot, fpnn_aes_keyset.d_eiv), or null (then computed)
    const uint4 *eiv;
    // the address-audit build's extent table (audit.hpp; null in the product build)
    AuditTable *aud;
};

// Per-engine dispatch settings that tests set (tests/conftest.py) so that small batches
// reach every session of the shipped kernels.  Round 4 removed the measured-and-rejected
// kernel variants (2-table LDS image, 1/4-block encrypt chunks, unfenced rounds, K2q, K1 on
// dense batches, the separate K1r plan launch for out-of-place batches); round 6 the A/B
// switches whose other side was measured slower (K2h's lane-session wire funnel, the K2c
// threshold, E_k(IV) off, K2's ragged / short-frame / fence / 4-block-chunk / line-
// alignment switches, the three-launch block map) -- their numbers stay in DESIGN.md.
struct Variant {
    // K2h: chains of at least hyb_long blocks (bucket-rounded) go to quads; hyb_quad_waves
    // of a workgroup's 16 waves start on them.  Round-3 sweep on C4 (profiles/r03/
    // sweep_c4_r03x.json): 1024 / 12 at 790-799 GiB/s against 738 for 512 / 8.
    int hyb_long = 1024;
    int hyb_quad_waves = 12;
    int hyb_force = 0;  // every ragged batch of more than one chain takes K2h (tests)
    // tests only: the next poison_order ragged encrypts find their length-order block's
    // counts dirty (FPNN_AES_DEBUG_POISON_ORDER), to check that the device reports it
    int poison_order = 0;
    // K1r: chunks inside one segment's interior take the lean loop (k_ragged.hip); 0 runs
    // every chunk through the general path (FPNN_AES_K1R_RUNS=0: tests reach the general
    // path at every chunk position)
    int k1r_runs = 1;
};

// Base name ("cfb_decrypt_dense", ...) of the main kernel the last launch_* call on this
// thread queued (the variant the dispatch actually chose; instrumentation and bench labels).
const char *last_launched();
void set_launched(const char *name);
// threads = workgroup size (64..1024, multiple of 64): few chains are spread over all
// CUs with small workgroups instead of packed into a few full ones.
// Frame scan of received segments (framing.hip).
enum : uint32_t { SCAN_OK = 0, SCAN_FULL = 1, SCAN_TOO_LARGE = 2, SCAN_BAD_MAGIC = 3, SCAN_BAD_MTYPE = 4,
                  SCAN_BAD_LENGTH = 5 };
struct ScanResult {  // == fpnn_aes_frame_scan
    uint32_t frames, status;
    uint64_t consumed;
};
struct KScan {
    const uint8_t *buf;       // package: received bytes; stream: decrypted plaintext
    uint64_t count;
    const uint64_t *off;      // segment starts (NULL: i * stride)
    uint64_t stride;
    const uint32_t *len;      // segment lengths (NULL: uniform_len)
    uint32_t uniform_len;
    uint32_t max_len;
    const uint32_t *carry;    // stream: plaintext bytes before each segment (NULL: 0)
    const uint32_t *key_slot; // package: segment key slots (NULL: 0)
    uint32_t max_frames;
    uint32_t pad;
    uint64_t *frame_off;      // [count * max_frames], relative to the segment (region) start
    uint32_t *frame_len;
    ScanResult *scan;         // [count]
    uint64_t *abs_off;        // package: absolute body offsets, for the decrypt batch
    uint32_t *abs_slot;       // package: key slot per frame slot (NULL: one key)
};

hipError_t launch_scan_frames(const KScan &s, bool stream, int num_cus, hipStream_t st);
hipError_t launch_encrypt_chains(const KBatch &b, int nrounds, Layout layout, KeyMode km, bool stream, int grid,
                                 int threads, hipStream_t st);
// K2s-DB (k_encrypt.hip): ragged package batches of short frames -- every len <=
// kFrameMaxBytes (the caller's fpnn_aes_batch.max_len) -- one lane per chain, the whole frame
// loaded, ciphered and stored at once while the lane's next frame loads; wire = the 4-byte
// length prefix (FPNN_AES_F_WIRE_PREFIX); grid = one workgroup per CU.
constexpr int kFrameMaxBlocks = 10;
constexpr uint32_t kFrameMaxBytes = 16u * kFrameMaxBlocks + 15u;  // 175: FPNN's 145-B quests and shorter
hipError_t launch_encrypt_frames(const KBatch &b, int nrounds, KeyMode km, bool wire, int grid, hipStream_t st);
// D2s: the same pipeline for package decrypts of short frames (one lane per frame, its
// blocks' AES passes independent of each other); grid = one workgroup per CU
hipError_t launch_decrypt_frames(const KBatch &b, int nrounds, KeyMode km, int grid, hipStream_t st);
// K2c: one 4-lane quad per chain (few / long chains); threads = workgroup size.
hipError_t launch_encrypt_coop(const KBatch &b, int nrounds, Layout layout, KeyMode km, bool stream, int grid,
                               int threads, hipStream_t st);
// Stream batches that carry many frames per stream (k_stream_frames.hip;
// fpnn_aes_stream_*_frames): stream j owns segments [first_frame[j], first_frame[j+1]) and
// b.iv_state / b.pos_state hold nstreams entries.  Every kernel clamps what it reads from
// first_frame into [0, count] (an empty range when it decreases) and stores
// kFaultFrameTable into *fault when the table is not monotone from 0 to count.
//
// The slot-addressed calls (fpnn_aes_stream_*_frames_at, fpnn_aes_stream_recv_at) set
// state_slot: stream j's state is entry state_slot[j] of b.iv_state / b.pos_state and its
// key is slot state_slot[j] of b.keys (b.key_slot is null then); the state arrays hold
// slot_bound entries.  A stream with state_slot[j] >= slot_bound is reported (kFaultKeySlot
// ORed into *fault): its state is neither read nor written, encrypt writes nothing for it,
// decrypt ciphers its segments under slot 0 from a zero state (bytes unspecified, inside
// its own segments).  state_slot == null is the identity: the calls above.
// first_frame == null (recv_at): stream j is segment j, nstreams == count.
struct FrameTable {
    const uint32_t *first_frame;  // nstreams + 1 entries, or null
    uint32_t nstreams;
    uint32_t slot_bound;          // (with state_slot)
    uint32_t *fault;
    const uint32_t *state_slot;   // nstreams entries, or null
    uint32_t *seg_slot;           // decrypt with state_slot: the walk writes every segment's key slot
                                  // here (count entries, engine scratch); K1r and the pre-pass's
                                  // second launch read it as b.key_slot
};
// K2f: encrypt, one quad per STREAM (K2c's cipher); the quad keeps (iv, pos) in registers
// across the stream's frames; grid and threads sized as K2c's, by quads needed.
hipError_t launch_encrypt_stream_frames(const KBatch &b, const FrameTable &f, int nrounds, KeyMode km, int grid,
                                        int threads, hipStream_t st);
// Decrypt: the state pre-pass.  K1r reads every segment's incoming (iv, pos) from
// b.iv_snap / b.pos_snap; these two launches fill that snapshot (snap_iv, snap_pos; count
// entries) from the streams' incoming state and the ciphertext alone, before anything is
// written: one lane per stream walks its frames' lengths (snap_pos, and per segment its
// stream and the last non-empty frame before it: seg_stream, seg_prev), then one lane per
// segment gathers the ciphertext block before its frame and runs at most one AES pass.
hipError_t launch_stream_frames_state(const KBatch &b, const FrameTable &f, int nrounds, KeyMode km, uint4 *snap_iv,
                                      uint32_t *snap_pos, uint32_t *seg_stream, uint32_t *seg_prev, int num_cus,
                                      hipStream_t st);
// After K1r, which exported every non-empty segment's outgoing state into seg_iv / seg_pos
// (per SEGMENT): stream j's state becomes that of its last non-empty frame; a stream
// without one keeps its own.
hipError_t launch_stream_frames_commit(const KBatch &b, const FrameTable &f, const uint4 *seg_iv,
                                       const uint32_t *seg_pos, hipStream_t st);
// UDP v2 datagrams with data encryption (k_udp.hip; fpnn_aes_udp_encrypt / _decrypt).  The
// KBatch describes the DATAGRAMS (b.keys: the package table; b.iv_state / b.pos_state: the data
// StreamEncryptor's state, slot_bound entries); connection j owns datagrams [first_dgram[j],
// first_dgram[j + 1]), datagram i sections [first_section[i], first_section[i + 1]), section s
// the bytes [sec_off[s], + sec_len[s]) of its datagram.  conn_slot[j] names the connection's
// slot in both tables and in the state arrays.  Both range tables have first_frame's contract
// (FrameTable) and every kernel clamps what it reads from them; sections ascend inside their
// datagram, and one that does not, or leaves it, is clamped into it and reported
// (kFaultFrameTable).  A connection with conn_slot[j] >= slot_bound is reported
// (kFaultKeySlot) and treated as a stream of the *_frames_at calls is.
struct UdpTable {
    const DevKey *data_keys;  // the data table's slots (null: the call has no section)
    const uint32_t *first_dgram, *conn_slot;
    const uint32_t *first_section, *sec_off, *sec_len;
    uint32_t nconn, slot_bound, nsections, pad;
    uint32_t *fault;
};
// K2u: encrypt, one quad per connection, data layer then package layer per datagram; grid and
// threads sized as K2c's, by quads needed.  nr_data, nr_pkg: 10 or 14.
hipError_t launch_udp_encrypt(const KBatch &b, const UdpTable &u, int nr_data, int nr_pkg, int grid, int threads,
                              hipStream_t st);
// Decrypt's descriptors for the existing kernels: dg_slot (count entries: every datagram's key
// slot), sec_abs / sec_n (nsections: every section as a segment of b.out), conn_sec (nconn + 1:
// every connection's section range).
hipError_t launch_udp_expand(const KBatch &b, const UdpTable &u, uint32_t *dg_slot, uint64_t *sec_abs, uint32_t *sec_n,
                             uint32_t *conn_sec, int num_cus, hipStream_t st);
// UDP v2 receive (k_udp_recv.hip; fpnn_aes_udp_recv / _recv_take).  The three walk tables, the
// device's mirrors of fpnn_aes_udp_scan / _pkg / _section (engine.hip asserts the sizes):
// datagram i's rows start at i * max_pkgs and i * max_sections.
struct UdpScan {
    uint16_t pkgs, sections;
    uint8_t version, status;
    uint16_t reserved;
};
struct UdpPkg {
    uint32_t seq;
    uint8_t type, flag, sign, status;
    uint16_t off, len;
    uint16_t first_section, nsections;
};
struct UdpSection {
    uint8_t type, flag;
    uint16_t pkg;
    uint16_t off, len;
    uint16_t package_id, reserved;
    uint32_t seg_index;
};
enum : uint8_t { UDP_OK = 0, UDP_SHORT = 1, UDP_VERSION = 2, UDP_TYPE = 3, UDP_ACKS = 4, UDP_CLOSE = 5, UDP_FULL = 6,
                 UDP_LONG = 7 };
struct UdpRecvTable {
    UdpScan *scan;
    UdpPkg *pkgs;
    UdpSection *sections;
    uint32_t max_pkgs, max_sections;
    const uint32_t *first_take, *take;  // recv_take: the packages to decrypt (null: all, in array order)
    uint32_t ntake, pad;
};
// k_udp_walk: one lane per datagram reads its package-plaintext in b.out and writes its scan
// entry and its package and section rows.
hipError_t launch_udp_walk(const KBatch &b, const UdpRecvTable &r, int num_cus, hipStream_t st);
// k_udp_take: the data layer's descriptors for the slot-addressed *_frames decrypt, a fixed
// max_sections segments per datagram (all packages) or per taken package: sec_abs / sec_n
// (nseg = items * max_sections entries: a section to decrypt as a segment of b.out, else length
// 0) and conn_sec (nconn + 1: connection j's segments).  What is read from the caller's tables
// is clamped and a breach reported (kFaultFrameTable).
hipError_t launch_udp_take(const KBatch &b, const UdpTable &u, const UdpRecvTable &r, uint64_t *sec_abs,
                           uint32_t *sec_n, uint32_t *conn_sec, int num_cus, hipStream_t st);
// K2h (k_hybrid.hip): ragged batches with more chains than quads.  Chains of perm[]
// in length buckets <= long_bucket run on quads (K2c's cipher), the rest one per lane
// (K2's); quad_waves waves per workgroup start on the long ones.  ctr: the 2 ticket
// words of the call's length-order block; buckets: its counts.
// A length-order block (launch_length_order): 128 bucket counts, 128 cursors, then
// (wire-prefix batches) a flag word, nonzero when some frame starts off the 4-byte grid,
// then K2h's two ticket counters, then a count of finished workgroups.  The block starts
// zeroed and its LAST reader zeroes it again once every workgroup is done with it: the
// bucket scatter's last workgroup when K2c follows, K2h's when K2h follows.  No memset
// launch per call, and a call captured in a graph finds the block zeroed on every replay.
constexpr int kWireFlagWord = 256;
constexpr int kTicketWords = 257;
constexpr int kDoneWord = 259;
constexpr int kLengthOrderWords = 260;

struct HybridArgs {
    uint32_t *ctr;
    const uint32_t *buckets;  // the call's length-order block
    uint32_t long_bucket;
    uint32_t quad_waves;
    uint4 *sink;      // 2 x uint4 per wave (grid * kThreads / 64 waves): stores with nothing to store
};
hipError_t launch_encrypt_hybrid(const KBatch &b, const HybridArgs &h, int nrounds, KeyMode km, bool stream, int grid,
                                 hipStream_t st);
// The slot forms of K2, K2c and K2h's stream paths (k_stream_at.hip, instantiated from the same
// kernel templates with KEY_SLOT; fpnn_aes_stream_encrypt_at): b.state_slot / b.slot_bound /
// b.slot_fault set, b.key_slot null, b.iv_state / b.pos_state of slot_bound entries.  A segment
// whose slot lies at or past the bound is reported (kFaultKeySlot): neither state is touched and
// no byte of it is written.  K2h's length order for these calls is by length alone (the
// engine queues launch_length_order with stream = false: the carried position, at most 15
// bytes, would have to be gathered through the slot).
hipError_t launch_encrypt_chains_at(const KBatch &b, int nrounds, Layout layout, int grid, int threads, hipStream_t st);
hipError_t launch_encrypt_coop_at(const KBatch &b, int nrounds, Layout layout, int grid, int threads, hipStream_t st);
hipError_t launch_encrypt_hybrid_at(const KBatch &b, const HybridArgs &h, int nrounds, int grid, hipStream_t st);
// length bucket of a block count (descending: bucket 0 = longest), as launch_length_order
uint32_t length_bucket_of(uint64_t nblocks);
// Ragged batches: perm[] = segment indices ordered by block count, longest first
// (quarter-octave buckets).  block: the length-order block (zero on entry); zero_after:
// nothing reads it after the scatter (K2c follows), so the scatter's last workgroup zeroes
// it; otherwise K2h does.  fault: as for the block map below -- gets kFaultLengthOrder when
// the bucket counts do not add up to b.count (a block not zero on entry); the scatter then
// writes no perm[] entry past the batch and K2h clamps what it reads, so a bad block gives
// FPNN_AES_ERR_DEVICE at the next sync instead of wild addresses.
hipError_t launch_length_order(const KBatch &b, bool stream, uint32_t *perm, uint32_t *block, bool zero_after,
                               uint32_t *fault, hipStream_t st);
// K1 / K1d / K1k for uniform and dense layouts (every segment's block count known on the host).
hipError_t launch_decrypt_blocks(const KBatch &b, int nrounds, Layout layout, KeyMode km, bool inplace, int grid,
                                 hipStream_t st);
// K1r (k_ragged.hip): ragged decrypt with no host round trip.  b.bstart[0..count] from
// launch_block_map_onepass / _small (bstart[count] = total blocks, device only); plan: one entry per
// wave of the grid (grid * kThreads / 64), filled by the plan kernel queued first.
struct RaggedPlan {
    uint64_t s0;  // segment holding the wave's first block
    uint64_t pad;
    uint4 fill;   // ciphertext block before it (same segment), saved before any write
};
// b.in_off, b.out_off and b.len must be device arrays (launch_ragged_desc writes the missing
// ones from stride / uniform_len; out_off may be in_off).
// sink: 2 x uint4 per wave of the grid, written by lanes with nothing to store, never read.
hipError_t launch_decrypt_ragged(const KBatch &b, int nrounds, KeyMode km, bool stream, RaggedPlan *plan, uint4 *sink,
                                 bool plan_launch, int grid, hipStream_t st);
hipError_t launch_ragged_desc(uint64_t count, uint64_t stride, uint32_t uniform_len, uint64_t *in_off, uint32_t *len,
                              hipStream_t st);
// In-place K1 / K1d: save the ciphertext block before every 64-block chunk.
hipError_t launch_boundary_save(const KBatch &b, uint4 *boundary, uint64_t nchunks, hipStream_t st);
// General-layout block map: bstart[0..count], the exclusive scan of per-segment block counts
// (bstart[count] = *total = total blocks, both device), in one launch (decoupled
// look-back); lb = block_map_onepass_words(count) words
// (lb_words = the buffer's capacity), zero when first used.  Everything the next launch
// needs is kept by the kernel itself -- tickets reset and the tile-status epoch advanced by
// its last workgroup -- so a launch captured in a graph and replayed stays correct.
// fault: a device-visible word (pinned host) that gets kFaultLookback if a look-back ever
// gave up waiting (the host reports FPNN_AES_ERR_DEVICE at the next sync).
constexpr uint32_t kFaultLookback = 1u;
constexpr uint32_t kFaultLengthOrder = 2u;
constexpr uint32_t kFaultFrameTable = 4u;  // a first_frame table not monotone from 0 to count (FrameTable)
uint64_t block_map_onepass_words(uint64_t count);
hipError_t launch_block_map_onepass(const KBatch &b, bool stream, uint64_t *bstart, uint64_t *lb, uint64_t lb_words,
                                    uint32_t *fault, uint64_t *total, hipStream_t st);
// The same for count <= block_map_small_max() in one workgroup; stream batches also
// copy (iv_state, pos_state) into the snapshot (snap_iv / snap_pos) on the way.
hipError_t launch_block_map_small(const KBatch &b, bool stream, const uint8_t *iv_state, const uint32_t *pos_state,
                                  uint4 *snap_iv, uint32_t *snap_pos, uint64_t *bstart, uint64_t *total,
                                  hipStream_t st);
uint64_t block_map_small_max();
// The rest of rijndael.h (k_modes.hip): ECB / CBC / OFB over one host call's buffers.
enum : int { MODE_ECB_ENC = 0, MODE_ECB_DEC = 1, MODE_CBC_ENC = 2, MODE_CBC_DEC = 3, MODE_OFB = 4 };
struct ModeArgs {
    const uint8_t *in;
    uint8_t *out;
    uint64_t nblocks;      // whole 16-byte blocks to process (ECB, CBC)
    uint64_t len;          // OFB: bytes
    const DevKey *key;     // encryption schedule, or the decryption schedule (ECB/CBC decrypt)
    uint8_t *iv;           // 16 B, in/out (CBC encrypt, OFB); CBC decrypt reads it
    uint32_t *pos;         // OFB position, in/out
    const uint32_t *t0le, *td0le;
    const uint8_t *isbox;
};
hipError_t launch_block_modes(const ModeArgs &a, int nrounds, int mode, int num_cus, hipStream_t st);
// K0 (k_small.hip): one synchronous CFB call of up to kSmallMaxBytes bytes, in place in
// pinned host staging: body at io + kSmallBodyAt (16-aligned), the head's bytes (pos != 0)
// right before it.  state (pinned): [ivec 16 B][pos u32][seq u32], the kernel stores seq
// last (system-scope release) once everything else is visible to the host.
constexpr uint32_t kSmallMaxBytes = 16384;
constexpr uint32_t kSmallBodyAt = 32;
struct SmallArgs {
    uint8_t *io;
    uint32_t len;   // bytes in the call (head + body)
    uint32_t head;  // min(len, (16 - pos) % 16): bytes finishing the current keystream block
    uint32_t pos;   // *p_num on entry
    uint32_t seq;
    uint4 iv;       // ivec on entry
    uint32_t rk[60];
    const uint32_t *t0le;
    uint32_t *state;
};
hipError_t launch_cfb_single(const SmallArgs &a, int nrounds, bool encrypt, hipStream_t st);
// K0s (k_small.hip): the resident form of K0 behind a mailbox in pinned host memory.  The
// host fills req (seq last, release), the server serves each new seq and stores it into
// resp.done after the results (io in place, resp.state = ivec + pos); it leaves after
// idle_ticks without a request, after life_ticks in any case, or when req.stop is set,
// storing its epoch into resp.exited.  Ticks of the device wall clock (wall_clock64).
struct alignas(16) SmallReq {
    uint32_t seq, op, len, head, pos, nrounds, stop, pad;  // op bit 0: encrypt
    uint32_t iv[4];
    uint32_t rk[60];  // block byte order
};
struct alignas(64) SmallResp {
    uint32_t done, exited, pad[2];
    uint32_t state[8];  // ivec (4 words), pos
};
struct SmallMailbox {
    SmallReq req;
    SmallResp resp;
    alignas(64) uint8_t io[kSmallBodyAt + kSmallMaxBytes + 64];
};
// yield: the device's batch-activity word (pinned host memory), y0 its value when the host
// launched the server: the host bumps it before it queues batch kernels; a server that sees
// it differ from y0 leaves after its current request (also one that only started after the
// bump), so no batch workgroup waits for a CU (or a hardware queue) a server holds.
hipError_t launch_cfb_server(SmallMailbox *mb, const uint32_t *t0le, uint32_t epoch, uint64_t idle_ticks,
                             uint64_t life_ticks, const uint32_t *yield, uint32_t y0, hipStream_t st);
// E_k(IV) of key slots [first, first + count) into eiv[first ...] (k_small.hip)
hipError_t launch_slot_eiv(const DevKey *keys, uint32_t first, uint32_t count, int nrounds, const uint32_t *t0le,
                           uint4 *eiv, hipStream_t st);
hipError_t launch_expand_keys(const uint8_t *keys, uint32_t keylen, const uint8_t *ivs, uint32_t count,
                              const uint8_t *sbox, DevKey *out, hipStream_t st);
// Writes into a live key table (k_keytable.hip; fpnn_aes_keyset_set_keys / _clear,
// fpnn_ecdh_accept).  Entry i < count goes to slot s_i = slots ? slots[i] : first + i; an
// entry with s_i >= slot_bound writes nothing and ORs kFaultKeySlot into *fault (the caller
// passes slot_bound <= the table's allocated slots; first + count when slots is null).
constexpr uint32_t kFaultKeySlot = 8u;  // a slots[] entry at or past the call's slot_bound
struct KeyTableArgs {
    DevKey *keys;
    uint4 *eiv;
    const uint32_t *slots;  // or null
    uint32_t first, count, slot_bound, pad;
    const uint8_t *raw;   // set_keys: count raw keys of the table's key length
    const uint8_t *ivs;   // set_keys: count * 16 bytes, or null (zero IVs)
    const uint8_t *ok;    // set_keys, stream_open: entries with ok[i] == 0 write nothing; or null
    uint4 *iv_state;      // stream_open / _close: the caller's state arrays, slot_bound entries
    uint32_t *pos_state;
    const uint32_t *t0le;
    uint32_t *fault;
    AuditTable *aud;      // the address-audit build's extent table (null in the product build)
};
// one lane per entry: the expanded DevKey and eiv[s_i] = E_k(IV) of the slot, in one launch
hipError_t launch_set_keys(const KeyTableArgs &a, uint32_t keylen, hipStream_t st);
// Stream state by slot (fpnn_aes_stream_open / _close), one lane per entry with the same
// addressing and slot_bound check; the table is only read.  open: iv_state[16 * s_i] = the
// slot's IV, pos_state[s_i] = 0, skipping entries with ok[i] == 0; close: both become zero.
hipError_t launch_stream_open(const KeyTableArgs &a, hipStream_t st);
hipError_t launch_stream_close(const KeyTableArgs &a, hipStream_t st);
// the slot as fpnn_aes_keyset_reserve leaves it: a zero DevKey and launch_slot_eiv's value for one
hipError_t launch_clear_slots(const KeyTableArgs &a, int nrounds, hipStream_t st);
// Host-mapped frame moves: a job copies n segments, segment i from address sbase + soff[i]
// to dbase + doff[i], len[i] + extra bytes (soff/doff/len device arrays; either side may be
// mapped host memory; a base of 0 makes the offsets absolute device-visible addresses).
// One launch runs two jobs concurrently (n = 0: none).
struct MoveJob {
    uint64_t sbase;
    const uint64_t *soff;
    uint64_t dbase;
    const uint64_t *doff;
    const uint32_t *len;
    uint32_t extra;
    uint32_t n;
};
hipError_t launch_move_segments(const MoveJob &a, const MoveJob &b, hipStream_t st);
hipError_t launch_fill_synthetic(uint8_t *dst, uint64_t nbytes, uint64_t seed, uint64_t byte_offset, int grid,
                                 hipStream_t st);

}  // namespace fpnn_aes
