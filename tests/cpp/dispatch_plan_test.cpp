// Which kernel a device batch call runs on (fpnn_amd/csrc/dispatch_plan.hpp) on the CPU: every
// threshold of the choice at its edge, on both sides.  The expected routes are literals, read off
// the rules include/fpnn_aes.h promises (and the engine's code before the choice had a header of
// its own); nothing here is computed by the plan or by a copy of its expressions.  Built and run
// by tests/test_dispatch_plan.py; prints one summary line, exits non-zero at the first miss.
#include "../../fpnn_amd/csrc/dispatch_plan.hpp"

#include <stdio.h>
#include <stdlib.h>

using namespace fpnn_aes;

static const char *g_case = "";
static unsigned g_cases = 0;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            fprintf(stderr, "%s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, g_case); \
            exit(1);                                                                \
        }                                                                           \
    } while (0)

// stand-ins for block_map_onepass_words and length_bucket_of
static uint64_t words(uint64_t n) { return 3 + (n + 2047) / 2048; }
static uint32_t bucket(uint64_t nblocks) { return (uint32_t)(nblocks / 16); }  // 1024 blocks: 64

// 256 CUs: a full chip is 262 144 lanes.  8 CUs: 8 192.
static DispatchShape shape(uint64_t num_cus) {
    return {ScratchShape{num_cus, 16, 16384, words, 260}, 1024, 175, 1024, 12, 0, bucket};
}
static const DispatchShape D = shape(256);
static const uint64_t FULL = 262144;

static const CallKind PACKAGE = {false, false}, STREAM = {true, false}, AT = {true, true};

// ---- batches ----
static BatchShape uniform(uint64_t count, uint32_t len) {  // no arrays, one key, out of place
    BatchShape b = {};
    b.count = count;
    b.stride = len;
    b.uniform_len = len;
    b.nkeys = 1;
    return b;
}
static BatchShape ragged(uint64_t count, uint32_t max_len = 0) {  // in_off[] and len[], one key
    BatchShape b = uniform(count, 0);
    b.in_off = b.len = true;
    b.max_len = max_len;
    return b;
}
static BatchShape keyed(uint64_t count, uint32_t len, uint64_t stride, uint32_t nkeys) {  // key_slot[] alone
    BatchShape b = uniform(count, len);
    b.stride = stride;
    b.key_slot = true;
    b.nkeys = nkeys;
    return b;
}

static bool no_need(const ScratchNeed &n) {
    for (int i = 0; i < kScratchBufs; i++)
        if (n.n[i]) return false;
    return true;
}

// ---- encrypt ----
struct Enc {
    EncryptFamily family;
    Layout layout;
    KeyMode km;
    int threads, grid;
    uint32_t flags;
    int order;  // 0: none; 1: by length, zeroed by the scatter; 2: by length, K2h zeroes; +4: by position too
};

static EncryptRoute enc(const char *name, const DispatchShape &d, const BatchShape &b, CallKind c, const Enc &x) {
    g_case = name;
    g_cases++;
    const EncryptRoute r = encrypt_route(d, b, c);
    CHECK(r.family == x.family);
    CHECK(r.layout == x.layout);
    CHECK(r.km == x.km);
    CHECK(r.threads == x.threads);
    CHECK(r.grid == x.grid);
    CHECK(r.flags == x.flags);
    CHECK(r.order == (x.order != 0));
    if (x.order) {
        CHECK(r.order_zeroes == ((x.order & 3) == 1));
        CHECK(r.order_pos == ((x.order & 4) != 0));
        // the length order's scratch: perm, the block, and K2h's sink (2 x uint4 per wave of the chip)
        CHECK(r.need.n[SC_perm] == b.count && r.need.n[SC_buckets] == 260);
        CHECK(r.need.n[SC_sink] == (x.family == ENC_HYBRID ? 2 * d.scratch.num_cus * 16 : 0));
    } else {
        CHECK(no_need(r.need));
    }
    if (x.family != ENC_FRAMES) CHECK(!r.wire);
    return r;
}

static void test_encrypt() {
    // uniform package: K2c below one chain per lane of the chip, K2 from there on
    enc("uniform full_chip - 1", D, uniform(FULL - 1, 1024), PACKAGE, {ENC_COOP, LAYOUT_UNIFORM, KEY_UNIFORM, 1024, 256, 0, 0});
    enc("uniform full_chip", D, uniform(FULL, 1024), PACKAGE, {ENC_CHAINS, LAYOUT_UNIFORM, KEY_UNIFORM, 1024, 256, F_ALIGN_CHUNKS, 0});
    enc("uniform 16 B full_chip - 1", D, uniform(FULL - 1, 16), PACKAGE, {ENC_COOP, LAYOUT_UNIFORM, KEY_UNIFORM, 1024, 256, 0, 0});
    enc("uniform 16 B full_chip", D, uniform(FULL, 16), PACKAGE, {ENC_CHAINS, LAYOUT_UNIFORM, KEY_UNIFORM, 1024, 256, F_ALIGN_CHUNKS, 0});
    enc("stream 4096 chains", D, uniform(4096, 1024), STREAM, {ENC_COOP, LAYOUT_UNIFORM, KEY_UNIFORM, 64, 256, 0, 0});
    enc("uniform 1024", D, uniform(1024, 1024), PACKAGE, {ENC_COOP, LAYOUT_UNIFORM, KEY_UNIFORM, 64, 64, 0, 0});
    enc("uniform 4097: two waves per workgroup", D, uniform(4097, 1024), PACKAGE, {ENC_COOP, LAYOUT_UNIFORM, KEY_UNIFORM, 128, 129, 0, 0});
    enc("stream full_chip", D, uniform(FULL, 64), STREAM, {ENC_CHAINS, LAYOUT_UNIFORM, KEY_UNIFORM, 1024, 256, F_ALIGN_CHUNKS, 0});
    enc("stream 2 x full_chip", D, uniform(2 * FULL, 64), STREAM, {ENC_CHAINS, LAYOUT_UNIFORM, KEY_UNIFORM, 1024, 256, F_ALIGN_CHUNKS, 0});

    // ragged: a length order from two chains on; K2h with more chains than quads
    enc("ragged 1", D, ragged(1), PACKAGE, {ENC_COOP, LAYOUT_GENERAL, KEY_UNIFORM, 64, 1, 0, 0});
    enc("ragged 2", D, ragged(2), PACKAGE, {ENC_COOP, LAYOUT_GENERAL, KEY_UNIFORM, 64, 1, 0, 1});
    enc("ragged 2 stream", D, ragged(2), STREAM, {ENC_COOP, LAYOUT_GENERAL, KEY_UNIFORM, 64, 1, 0, 1 + 4});
    enc("ragged 2 at", D, ragged(2), AT, {ENC_COOP, LAYOUT_GENERAL, KEY_SLOT, 64, 1, 0, 1});
    enc("ragged 65536", D, ragged(65536), PACKAGE, {ENC_COOP, LAYOUT_GENERAL, KEY_UNIFORM, 1024, 256, 0, 1});
    EncryptRoute r = enc("ragged 65537", D, ragged(65537), PACKAGE, {ENC_HYBRID, LAYOUT_GENERAL, KEY_UNIFORM, 1024, 256, F_ALIGN_CHUNKS, 2});
    CHECK(r.long_bucket == 64 && r.quad_waves == 12);
    r = enc("ragged 65537 stream", D, ragged(65537), STREAM, {ENC_HYBRID, LAYOUT_GENERAL, KEY_UNIFORM, 1024, 256, F_ALIGN_CHUNKS, 2 + 4});
    CHECK(r.long_bucket == 64 && r.quad_waves == 12);
    DispatchShape forced = D;
    forced.hyb_force = 1;
    forced.hyb_long = 512;
    forced.hyb_quad_waves = 8;
    r = enc("hyb_force 2", forced, ragged(2), PACKAGE, {ENC_HYBRID, LAYOUT_GENERAL, KEY_UNIFORM, 1024, 256, F_ALIGN_CHUNKS, 2});
    CHECK(r.long_bucket == 32 && r.quad_waves == 8);
    enc("hyb_force 1", forced, ragged(1), PACKAGE, {ENC_COOP, LAYOUT_GENERAL, KEY_UNIFORM, 64, 1, 0, 0});
    enc("hyb_force uniform", forced, uniform(1024, 64), PACKAGE, {ENC_COOP, LAYOUT_UNIFORM, KEY_UNIFORM, 64, 64, 0, 0});
    BatchShape wire = ragged(65537);
    wire.out_off = true;
    wire.flags = F_WIRE_PREFIX;
    r = enc("wire prefix on K2h", D, wire, PACKAGE, {ENC_HYBRID, LAYOUT_GENERAL, KEY_UNIFORM, 1024, 256, F_ALIGN_CHUNKS, 2});
    CHECK(r.long_bucket == 127 && r.quad_waves == 16);

    // the max_len bound (package, ragged, at least one chain per lane of the chip)
    enc("bound 2048", D, ragged(FULL, 2048), PACKAGE, {ENC_CHAINS, LAYOUT_GENERAL, KEY_UNIFORM, 1024, 256, 0, 0});
    enc("bound 2049", D, ragged(FULL, 2049), PACKAGE, {ENC_HYBRID, LAYOUT_GENERAL, KEY_UNIFORM, 1024, 256, F_ALIGN_CHUNKS, 2});
    enc("no bound", D, ragged(FULL, 0), PACKAGE, {ENC_HYBRID, LAYOUT_GENERAL, KEY_UNIFORM, 1024, 256, F_ALIGN_CHUNKS, 2});
    r = enc("bound 175", D, ragged(FULL, 175), PACKAGE, {ENC_FRAMES, LAYOUT_GENERAL, KEY_UNIFORM, 1024, 256, 0, 0});
    CHECK(!r.wire);
    wire = ragged(FULL, 175);
    wire.out_off = true;
    wire.flags = F_WIRE_PREFIX;
    r = enc("bound 175 wire", D, wire, PACKAGE, {ENC_FRAMES, LAYOUT_GENERAL, KEY_UNIFORM, 1024, 256, 0, 0});
    CHECK(r.wire);
    enc("bound 176", D, ragged(FULL, 176), PACKAGE, {ENC_CHAINS, LAYOUT_GENERAL, KEY_UNIFORM, 1024, 256, 0, 0});
    enc("bound 175 full_chip - 1", D, ragged(FULL - 1, 175), PACKAGE, {ENC_HYBRID, LAYOUT_GENERAL, KEY_UNIFORM, 1024, 256, F_ALIGN_CHUNKS, 2});
    enc("bound 2048 full_chip - 1", D, ragged(FULL - 1, 2048), PACKAGE, {ENC_HYBRID, LAYOUT_GENERAL, KEY_UNIFORM, 1024, 256, F_ALIGN_CHUNKS, 2});
    enc("bound 175 stream", D, ragged(FULL, 175), STREAM, {ENC_HYBRID, LAYOUT_GENERAL, KEY_UNIFORM, 1024, 256, F_ALIGN_CHUNKS, 2 + 4});
    enc("bound 2048 stream", D, ragged(FULL, 2048), STREAM, {ENC_HYBRID, LAYOUT_GENERAL, KEY_UNIFORM, 1024, 256, F_ALIGN_CHUNKS, 2 + 4});
    enc("bound 175 at", D, ragged(FULL, 175), AT, {ENC_HYBRID, LAYOUT_GENERAL, KEY_SLOT, 1024, 256, F_ALIGN_CHUNKS, 2});
    BatchShape b = uniform(FULL, 145);
    b.max_len = 175;
    enc("bound without len[]", D, b, PACKAGE, {ENC_CHAINS, LAYOUT_UNIFORM, KEY_UNIFORM, 1024, 256, F_ALIGN_CHUNKS, 0});
    b.count = FULL - 1;
    enc("bound without len[] full_chip - 1", D, b, PACKAGE, {ENC_COOP, LAYOUT_UNIFORM, KEY_UNIFORM, 1024, 256, 0, 0});

    // key mode and the slot form
    enc("key_slot[], one-key table", D, keyed(1024, 64, 64, 1), PACKAGE, {ENC_COOP, LAYOUT_GENERAL, KEY_UNIFORM, 64, 64, 0, 0});
    enc("key_slot[], 1000 keys", D, keyed(1024, 64, 64, 1000), PACKAGE, {ENC_COOP, LAYOUT_GENERAL, KEY_LANE, 64, 64, 0, 0});
    enc("key_slot[], 2 keys, K2", D, keyed(FULL, 64, 64, 2), PACKAGE, {ENC_CHAINS, LAYOUT_GENERAL, KEY_LANE, 1024, 256, F_ALIGN_CHUNKS, 0});
    b = ragged(FULL, 175);
    b.key_slot = true;
    b.nkeys = 1000;
    enc("K2s-DB keyed", D, b, PACKAGE, {ENC_FRAMES, LAYOUT_GENERAL, KEY_LANE, 1024, 256, 0, 0});
    b.nkeys = 1;
    enc("K2s-DB key_slot[], one-key table", D, b, PACKAGE, {ENC_FRAMES, LAYOUT_GENERAL, KEY_UNIFORM, 1024, 256, 0, 0});
    enc("at K2", D, uniform(FULL, 64), AT, {ENC_CHAINS, LAYOUT_UNIFORM, KEY_SLOT, 1024, 256, F_ALIGN_CHUNKS, 0});
    enc("at K2c", D, uniform(1024, 64), AT, {ENC_COOP, LAYOUT_UNIFORM, KEY_SLOT, 64, 64, 0, 0});
    enc("at K2h", D, ragged(65537), AT, {ENC_HYBRID, LAYOUT_GENERAL, KEY_SLOT, 1024, 256, F_ALIGN_CHUNKS, 2});

    // nothing hard-wired: 8 CUs, a full chip of 8192 lanes
    const DispatchShape S = shape(8);
    enc("8 CUs uniform 8191", S, uniform(8191, 1024), PACKAGE, {ENC_COOP, LAYOUT_UNIFORM, KEY_UNIFORM, 1024, 8, 0, 0});
    enc("8 CUs uniform 8192", S, uniform(8192, 1024), PACKAGE, {ENC_CHAINS, LAYOUT_UNIFORM, KEY_UNIFORM, 1024, 8, F_ALIGN_CHUNKS, 0});
    enc("8 CUs uniform 100", S, uniform(100, 1024), PACKAGE, {ENC_COOP, LAYOUT_UNIFORM, KEY_UNIFORM, 64, 7, 0, 0});
    enc("8 CUs ragged 2048", S, ragged(2048), PACKAGE, {ENC_COOP, LAYOUT_GENERAL, KEY_UNIFORM, 1024, 8, 0, 1});
    enc("8 CUs ragged 2049", S, ragged(2049), PACKAGE, {ENC_HYBRID, LAYOUT_GENERAL, KEY_UNIFORM, 1024, 8, F_ALIGN_CHUNKS, 2});
    enc("8 CUs bound 175", S, ragged(8192, 175), PACKAGE, {ENC_FRAMES, LAYOUT_GENERAL, KEY_UNIFORM, 1024, 8, 0, 0});
    enc("8 CUs bound 175, 8191", S, ragged(8191, 175), PACKAGE, {ENC_HYBRID, LAYOUT_GENERAL, KEY_UNIFORM, 1024, 8, F_ALIGN_CHUNKS, 2});
}

// ---- decrypt ----
struct Dec {
    DecryptFamily family;
    Layout layout;
    KeyMode km;
    uint32_t nb;
    uint64_t total_blocks, magic, nchunks;
    int grid;
};

static DecryptRoute dec(const char *name, const DispatchShape &d, const BatchShape &b, CallKind c, const Dec &x) {
    g_case = name;
    g_cases++;
    const DecryptRoute r = decrypt_route(d, b, c);
    CHECK(r.family == x.family);
    CHECK(r.layout == x.layout);
    CHECK(r.km == x.km);
    CHECK(r.nb_uniform == x.nb);
    CHECK(r.total_blocks == x.total_blocks);
    CHECK(r.magic == x.magic);
    CHECK(r.nchunks == x.nchunks);
    CHECK(r.grid == x.grid);
    if (x.family != DEC_DENSE) CHECK(!r.boundary_save);
    if (x.family == DEC_FRAMES) CHECK(no_need(r.need));
    return r;
}

// K1r's scratch for n segments: the block map, one plan entry and two sink entries per wave of the
// chip, the look-back words past small_max, the descriptor arrays the caller did not give, and the
// state snapshot of a stream batch
static void k1r_need(const DecryptRoute &r, uint64_t cus, uint64_t n, uint64_t lookback, uint64_t desc_off,
                     uint64_t desc_len, uint64_t snap) {
    CHECK(r.need.n[SC_bstart] == n + 1);
    CHECK(r.need.n[SC_plan] == 16 * cus && r.need.n[SC_sink] == 32 * cus);
    CHECK(r.need.n[SC_lookback] == lookback);
    CHECK(r.need.n[SC_desc_off] == desc_off && r.need.n[SC_desc_len] == desc_len);
    CHECK(r.need.n[SC_snap_iv] == snap && r.need.n[SC_snap_pos] == snap);
    CHECK(r.need.n[SC_boundary] == 0 && r.need.n[SC_perm] == 0 && r.need.n[SC_sf_stream] == 0);
}

static void test_decrypt() {
    const Dec K1R = {DEC_RAGGED, LAYOUT_GENERAL, KEY_UNIFORM, 0, 0, 0, 0, 256};
    const Dec K1R_KEYED = {DEC_RAGGED, LAYOUT_GENERAL, KEY_LANE, 0, 0, 0, 0, 256};
    // uniform package: dense from two blocks per segment on, below 2^32 blocks in all
    DecryptRoute r = dec("uniform 1000 x 1024", D, uniform(1000, 1024), PACKAGE,
                         {DEC_DENSE, LAYOUT_FULL, KEY_UNIFORM, 64, 64000, 288230376151711744ull, 1000, 16});
    CHECK(!r.boundary_save && no_need(r.need));
    dec("uniform 100000 x 1024", D, uniform(100000, 1024), PACKAGE,
        {DEC_DENSE, LAYOUT_FULL, KEY_UNIFORM, 64, 6400000, 288230376151711744ull, 100000, 256});
    dec("uniform 1000 x 1000", D, uniform(1000, 1000), PACKAGE,
        {DEC_DENSE, LAYOUT_UNIFORM, KEY_UNIFORM, 63, 63000, 292805461487453201ull, 985, 16});
    dec("uniform 1000 x 17", D, uniform(1000, 17), PACKAGE,
        {DEC_DENSE, LAYOUT_UNIFORM, KEY_UNIFORM, 2, 2000, 9223372036854775808ull, 32, 1});
    dec("uniform 1000 x 32", D, uniform(1000, 32), PACKAGE,
        {DEC_DENSE, LAYOUT_FULL, KEY_UNIFORM, 2, 2000, 9223372036854775808ull, 32, 1});
    r = dec("uniform 1000 x 16", D, uniform(1000, 16), PACKAGE, K1R);
    k1r_need(r, 256, 1000, 0, 1000, 1000, 0);
    r = dec("uniform 1000 x 1", D, uniform(1000, 1), PACKAGE, K1R);
    k1r_need(r, 256, 1000, 0, 1000, 1000, 0);
    r = dec("uniform 2^26 x 1024: 2^32 blocks", D, uniform(1ull << 26, 1024), PACKAGE, K1R);
    k1r_need(r, 256, 1ull << 26, 3 + 32768, 1ull << 26, 1ull << 26, 0);
    dec("uniform (2^26 - 1) x 1024", D, uniform((1ull << 26) - 1, 1024), PACKAGE,
        {DEC_DENSE, LAYOUT_FULL, KEY_UNIFORM, 64, 4294967232ull, 288230376151711744ull, 67108863, 256});
    r = dec("uniform stream", D, uniform(1000, 1024), STREAM, K1R);
    k1r_need(r, 256, 1000, 0, 1000, 1000, 1000);
    r = dec("uniform stream past small_max", D, uniform(16385, 1024), STREAM, K1R);
    k1r_need(r, 256, 16385, 3 + 9, 16385, 16385, 16385);

    // keyed dense: key_slot[] alone over a many-key table, whole blocks, stride == uniform_len
    dec("keyed 32", D, keyed(1000, 32, 32, 1000), PACKAGE,
        {DEC_DENSE, LAYOUT_FULL, KEY_LANE, 2, 2000, 9223372036854775808ull, 32, 1});
    dec("keyed 1472", D, keyed(1000, 1472, 1472, 1000), PACKAGE,
        {DEC_DENSE, LAYOUT_FULL, KEY_LANE, 92, 92000, 200508087757712518ull, 1438, 23});
    dec("keyed 16", D, keyed(1000, 16, 16, 1000), PACKAGE, K1R_KEYED);
    dec("keyed 40", D, keyed(1000, 40, 40, 1000), PACKAGE, K1R_KEYED);
    dec("keyed stride != uniform_len", D, keyed(1000, 48, 64, 1000), PACKAGE, K1R_KEYED);
    dec("keyed stream", D, keyed(1000, 32, 32, 1000), STREAM, K1R_KEYED);
    dec("keyed (2^26) x 1024", D, keyed(1ull << 26, 1024, 1024, 1000), PACKAGE, K1R_KEYED);
    r = dec("key_slot[], one-key table", D, keyed(1000, 1024, 1024, 1), PACKAGE, K1R);
    k1r_need(r, 256, 1000, 0, 1000, 1000, 0);
    BatchShape b = keyed(1000, 32, 32, 1000);
    b.in_off = true;
    r = dec("keyed with in_off[]", D, b, PACKAGE, K1R_KEYED);
    k1r_need(r, 256, 1000, 0, 0, 1000, 0);

    // D2s: len[] within the 175-byte bound, at least one frame per lane of the chip, package
    dec("D2s", D, ragged(FULL, 175), PACKAGE, {DEC_FRAMES, LAYOUT_GENERAL, KEY_UNIFORM, 0, 0, 0, 0, 256});
    b = ragged(FULL, 175);
    b.key_slot = true;
    b.nkeys = 1000;
    dec("D2s keyed", D, b, PACKAGE, {DEC_FRAMES, LAYOUT_GENERAL, KEY_LANE, 0, 0, 0, 0, 256});
    r = dec("D2s full_chip - 1", D, ragged(FULL - 1, 175), PACKAGE, K1R);
    k1r_need(r, 256, FULL - 1, 3 + 128, 0, 0, 0);
    dec("D2s bound 176", D, ragged(FULL, 176), PACKAGE, K1R);
    dec("D2s no bound", D, ragged(FULL, 0), PACKAGE, K1R);
    dec("D2s stream", D, ragged(FULL, 175), STREAM, K1R);
    b = uniform(FULL, 16);
    b.max_len = 175;
    dec("D2s bound without len[]", D, b, PACKAGE, K1R);

    // in place: dense batches save the block before every 64-block chunk first
    b = uniform(1000, 1024);
    b.inplace = true;
    r = dec("dense in place", D, b, PACKAGE, {DEC_DENSE, LAYOUT_FULL, KEY_UNIFORM, 64, 64000, 288230376151711744ull, 1000, 16});
    CHECK(r.boundary_save && r.need.n[SC_boundary] == 1000 && r.need.n[SC_bstart] == 0);
    b = uniform(1000, 1000);
    b.inplace = true;
    r = dec("dense in place 1000 B", D, b, PACKAGE, {DEC_DENSE, LAYOUT_UNIFORM, KEY_UNIFORM, 63, 63000, 292805461487453201ull, 985, 16});
    CHECK(r.boundary_save && r.need.n[SC_boundary] == 985);
    b = uniform(1000, 16);
    b.inplace = true;
    r = dec("K1r in place", D, b, PACKAGE, K1R);
    k1r_need(r, 256, 1000, 0, 1000, 1000, 0);

    const DispatchShape S = shape(8);
    dec("8 CUs uniform 1000 x 1024", S, uniform(1000, 1024), PACKAGE,
        {DEC_DENSE, LAYOUT_FULL, KEY_UNIFORM, 64, 64000, 288230376151711744ull, 1000, 8});
    dec("8 CUs D2s", S, ragged(8192, 175), PACKAGE, {DEC_FRAMES, LAYOUT_GENERAL, KEY_UNIFORM, 0, 0, 0, 0, 8});
    r = dec("8 CUs D2s 8191", S, ragged(8191, 175), PACKAGE, {DEC_RAGGED, LAYOUT_GENERAL, KEY_UNIFORM, 0, 0, 0, 0, 8});
    k1r_need(r, 8, 8191, 0, 0, 0, 0);
}

// ---- *_frames calls and package receive ----
static void frames(const char *name, const DispatchShape &d, const BatchShape &b, bool at, uint64_t nstreams, KeyMode km,
                   int threads, int grid) {
    g_case = name;
    g_cases++;
    const FramesRoute e = frames_route(d, b, at, nstreams, true);
    CHECK(e.km == km && e.threads == threads && e.grid == grid);
    CHECK(no_need(e.need));
    const FramesRoute r = frames_route(d, b, at, nstreams, false);
    CHECK(r.km == km);
    // K1r on a stream batch plus the per-segment state; the segments' key slots for an _at call
    CHECK(r.need.n[SC_bstart] == b.count + 1 && r.need.n[SC_snap_iv] == b.count && r.need.n[SC_snap_pos] == b.count);
    CHECK(r.need.n[SC_sf_stream] == b.count && r.need.n[SC_sf_prev] == b.count && r.need.n[SC_sf_iv] == b.count &&
          r.need.n[SC_sf_pos] == b.count);
    CHECK(r.need.n[SC_sf_slot] == (at ? b.count : 0));
    CHECK(r.need.n[SC_desc_off] == 0 && r.need.n[SC_desc_len] == 0);  // (in_off[] and len[] given)
}

static void test_frames_and_recv() {
    BatchShape many = ragged(5000);
    many.key_slot = true;
    many.nkeys = 1000;
    BatchShape one = many;
    one.nkeys = 1;
    frames("frames, one key", D, ragged(5000), false, 1, KEY_UNIFORM, 64, 1);
    frames("frames, key_slot[] over one key", D, one, false, 4096, KEY_UNIFORM, 64, 256);
    frames("frames, keyed", D, many, false, 4096, KEY_LANE, 64, 256);
    frames("frames at", D, ragged(5000), true, 4096, KEY_LANE, 64, 256);
    frames("frames at, 1 stream", D, ragged(5000), true, 1, KEY_LANE, 64, 1);
    frames("frames, 70000 streams", D, ragged(100000), false, 70000, KEY_UNIFORM, 1024, 256);
    frames("frames at, 70000 streams", D, ragged(100000), true, 70000, KEY_LANE, 1024, 256);
    frames("8 CUs frames, 100 streams", shape(8), ragged(5000), false, 100, KEY_UNIFORM, 64, 7);

    g_case = "per_key";
    g_cases += 3;
    CHECK(per_key(many));
    CHECK(!per_key(one));
    CHECK(!per_key(ragged(5000)));
}

int main() {
    test_encrypt();
    test_decrypt();
    test_frames_and_recv();
    printf("dispatch_plan ok: %u cases\n", g_cases);
    return 0;
}
