// The chunk planner of the stream-mode host-frame calls (fpnn_amd/csrc/stream_plan.hpp) on the
// CPU: random and hand-made frame lists through StreamPlan::next_chunk with small chunk
// sizes and quotas, every property of the plan checked against a bookkeeping of its own.
// Built and run by tests/test_stream_plan.py; prints one summary line, exits non-zero at
// the first broken property.
#include "../../fpnn_amd/csrc/stream_plan.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <random>
#include <set>

using namespace fpnn_aes;

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, g_case); \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

static char g_case[128] = "";
static uint64_t g_plans = 0, g_chunks = 0;

static fpnn_aes_host_frame frame(uint32_t slot, uint32_t len) {
    fpnn_aes_host_frame f;
    memset(&f, 0, sizeof f);
    f.len = len;
    f.key_slot = slot;
    return f;
}

// order / segs against a direct restatement: streams that carry bytes in slot order, each
// stream's frames in array order
static void check_groups(const std::vector<fpnn_aes_host_frame> &fr, const StreamPlan &plan) {
    std::map<uint32_t, std::vector<uint32_t>> by_slot;
    for (uint32_t i = 0; i < fr.size(); i++) by_slot[fr[i].key_slot].push_back(i);
    CHECK(plan.order.size() == fr.size());
    size_t s = 0;
    uint32_t first = 0;
    for (const auto &kv : by_slot) {
        uint64_t bytes = 0;
        for (size_t q = 0; q < kv.second.size(); q++) {
            CHECK(plan.order[first + q] == kv.second[q]);
            bytes += fr[kv.second[q]].len;
        }
        if (bytes) {  // a stream of empty frames only is absent from segs
            CHECK(s < plan.segs.size());
            CHECK(plan.segs[s].slot == kv.first && plan.segs[s].first == first);
            CHECK(plan.segs[s].nframes == kv.second.size() && plan.segs[s].bytes == bytes);
            s++;
        }
        first += (uint32_t)kv.second.size();
    }
    CHECK(s == plan.segs.size());
}

// Runs the whole plan; returns for every frame the set of chunks that carry a part of it.
static std::vector<std::set<uint64_t>> check_plan(const std::vector<fpnn_aes_host_frame> &fr, uint32_t nkeys,
                                                  uint64_t chunk_bytes, uint64_t quota) {
    StreamPlan plan(fr.data(), (uint32_t)fr.size(), nkeys);
    g_plans++;
    check_groups(fr, plan);
    const uint64_t nseg = plan.segs.size();
    uint64_t total = 0;
    std::vector<uint64_t> rem(nseg);
    std::vector<std::vector<Piece>> got(nseg);  // the pieces of each stream, in the order handed out
    for (uint64_t t = 0; t < nseg; t++) total += rem[t] = plan.segs[t].bytes;
    CHECK(plan.left == total);
    std::vector<std::set<uint64_t>> chunks_of(fr.size());
    std::vector<Piece> pieces;
    std::vector<ChunkSeg> cs;
    uint64_t state0 = 0, chunk = 0, expect0 = 0, left = total;
    uint32_t uni = 0;
    while (plan.next_chunk(chunk_bytes, quota, pieces, cs, state0, uni)) {
        CHECK(chunk++ <= total);  // every chunk takes a byte at least: the plan terminates
        g_chunks++;
        CHECK(!cs.empty() && state0 + cs.size() <= nseg);
        // round robin: the chunk starts at the first stream with bytes left at or after the
        // end of the previous one, from the first stream again once the last has been passed
        if (expect0 >= nseg) expect0 = 0;
        while (rem[expect0] == 0) expect0 = expect0 + 1 < nseg ? expect0 + 1 : 0;
        CHECK(state0 == expect0);
        uint64_t at = 0;
        bool same = true;
        size_t pi = 0;
        for (size_t q = 0; q < cs.size(); q++) {
            const uint64_t t = state0 + q;
            CHECK(cs[q].slot == plan.segs[t].slot);  // consecutive in segs from state0
            CHECK(cs[q].at == at);                   // back to back in the staging
            CHECK(cs[q].len == std::min(rem[t], quota));  // never more than quota per stream
            CHECK(at < chunk_bytes);  // no stream is added once the chunk holds chunk_bytes
            same = same && cs[q].len == cs[0].len;
            // the segment's pieces: exactly its bytes, frames of its stream
            uint64_t took = 0;
            while (took < cs[q].len) {
                CHECK(pi < pieces.size());
                const Piece &pc = pieces[pi++];
                CHECK(pc.len > 0 && pc.frame < fr.size() && fr[pc.frame].key_slot == cs[q].slot);
                CHECK((uint64_t)pc.off + pc.len <= fr[pc.frame].len);
                took += pc.len;
                got[t].push_back(pc);
                chunks_of[pc.frame].insert(chunk);
            }
            CHECK(took == cs[q].len);
            rem[t] -= cs[q].len;
            left -= cs[q].len;
            at += cs[q].len;
        }
        CHECK(pi == pieces.size());
        // the chunk went on while it held less than chunk_bytes and streams were left
        CHECK(at >= chunk_bytes || state0 + cs.size() == nseg);
        CHECK((uni != 0) == same && (!same || uni == cs[0].len));
        CHECK(plan.left == left);
        expect0 = state0 + cs.size();
    }
    CHECK(plan.left == 0 && left == 0);
    CHECK(!plan.next_chunk(chunk_bytes, quota, pieces, cs, state0, uni) && pieces.empty() && cs.empty());
    // per stream, the pieces of all chunks put together are that stream's frames in array
    // order, every byte once
    for (uint64_t t = 0; t < nseg; t++) {
        size_t pi = 0;
        for (uint32_t q = 0; q < plan.segs[t].nframes; q++) {
            const uint32_t fidx = plan.order[plan.segs[t].first + q];
            for (uint32_t off = 0; off < fr[fidx].len;) {
                CHECK(pi < got[t].size());
                CHECK(got[t][pi].frame == fidx && got[t][pi].off == off);
                off += got[t][pi++].len;
            }
        }
        CHECK(pi == got[t].size());
    }
    return chunks_of;
}

static const uint64_t kChunks[] = {64, 4096}, kQuotas[] = {16, 48, 1024};

static void check_all(const char *name, const std::vector<fpnn_aes_host_frame> &fr, uint32_t nkeys) {
    for (uint64_t cb : kChunks)
        for (uint64_t q : kQuotas) {
            snprintf(g_case, sizeof g_case, "%s, %zu frames, chunk %llu, quota %llu", name, fr.size(),
                     (unsigned long long)cb, (unsigned long long)q);
            check_plan(fr, nkeys, cb, q);
        }
}

static uint32_t random_len(std::mt19937_64 &rng) {
    switch (rng() % 8) {
    case 0: return 0;
    case 1: return 1 + rng() % 17;
    case 2: return 16 * (1 + rng() % 4);
    case 3: return 1000 + rng() % 9000;
    default: return 1 + rng() % 300;
    }
}

int main() {
    std::mt19937_64 rng(20261020);
    // random frame lists, the streams interleaved in the array
    for (int round = 0; round < 200; round++) {
        const uint32_t nstreams = 1 + rng() % 9, n = 1 + rng() % 200;
        std::vector<fpnn_aes_host_frame> fr;
        for (uint32_t i = 0; i < n; i++) fr.push_back(frame(rng() % nstreams, random_len(rng)));
        check_all("random", fr, nstreams + rng() % 3);
    }
    // empty frames at the start, in the middle and at the end of a stream; stream 1 has only
    // empty frames (check_groups: absent from segs), slot 3 has none at all
    {
        std::vector<fpnn_aes_host_frame> fr = {frame(0, 0), frame(1, 0), frame(0, 0), frame(2, 40), frame(0, 100),
                                               frame(0, 0), frame(1, 0), frame(0, 0), frame(0, 33), frame(2, 0),
                                               frame(2, 7),  frame(0, 0), frame(0, 0)};
        check_all("empty frames", fr, 4);
        StreamPlan plan(fr.data(), (uint32_t)fr.size(), 4);
        CHECK(plan.segs.size() == 2 && plan.segs[0].slot == 0 && plan.segs[1].slot == 2);
    }
    // one stream alone, with a frame that spans three chunks (130 bytes at 48 per chunk)
    {
        std::vector<fpnn_aes_host_frame> fr = {frame(5, 10), frame(5, 130), frame(5, 0), frame(5, 20)};
        check_all("one stream", fr, 6);
        snprintf(g_case, sizeof g_case, "one stream, the long frame");
        const auto chunks_of = check_plan(fr, 6, 64, 48);
        CHECK(chunks_of[1].size() == 3);  // 38 + 48 + 44 bytes behind the first frame's 10
        CHECK(chunks_of[0].size() == 1 && chunks_of[2].empty());
    }
    // several streams, one frame over three chunks among short ones
    {
        std::vector<fpnn_aes_host_frame> fr = {frame(0, 5), frame(1, 144), frame(2, 9), frame(0, 17), frame(2, 300)};
        check_all("long frame", fr, 3);
        const auto chunks_of = check_plan(fr, 3, 4096, 48);
        CHECK(chunks_of[1].size() == 3);
    }
    // nkeys > 4 n + 1024: the sparse grouping gives the same order and segments as the dense
    for (int round = 0; round < 20; round++) {
        const uint32_t n = 1 + rng() % 100, nstreams = 1 + rng() % 50;
        std::vector<fpnn_aes_host_frame> fr;
        for (uint32_t i = 0; i < n; i++) fr.push_back(frame(rng() % nstreams, random_len(rng)));
        snprintf(g_case, sizeof g_case, "sparse against dense, %u frames", n);
        const uint32_t dense_keys = nstreams, sparse_keys = 4 * n + 1025;
        CHECK((uint64_t)dense_keys <= 4ull * n + 1024 && (uint64_t)sparse_keys > 4ull * n + 1024);
        StreamPlan dense(fr.data(), n, dense_keys), sparse(fr.data(), n, sparse_keys);
        CHECK(dense.order == sparse.order && dense.segs.size() == sparse.segs.size());
        for (size_t t = 0; t < dense.segs.size(); t++) {
            const StreamSeg &a = dense.segs[t], &b = sparse.segs[t];
            CHECK(a.slot == b.slot && a.first == b.first && a.nframes == b.nframes && a.bytes == b.bytes);
        }
        check_all("sparse", fr, sparse_keys);
    }
    // the compact state block: (iv, pos) of the streams with bytes go in and come out, others stay
    {
        std::vector<fpnn_aes_host_frame> fr = {frame(3, 8), frame(1, 0), frame(0, 2)};
        StreamPlan plan(fr.data(), 3, 4);
        alignas(16) uint8_t block[2 * 20];
        uint8_t iv[64], iv2[64];
        uint32_t pos[4] = {17, 5, 6, 31}, pos2[4] = {9, 9, 9, 9};
        for (int i = 0; i < 64; i++) iv[i] = (uint8_t)(i * 7 + 1), iv2[i] = 0xEE;
        snprintf(g_case, sizeof g_case, "state block");
        pack_stream_state(plan.segs, iv, pos, block);
        CHECK(!memcmp(block, iv, 16) && !memcmp(block + 16, iv + 48, 16));
        const uint32_t *bp = reinterpret_cast<const uint32_t *>(block + 32);
        CHECK(bp[0] == (17 & 15) && bp[1] == (31 & 15));
        unpack_stream_state(plan.segs, block, iv2, pos2);
        CHECK(!memcmp(iv2, iv, 16) && !memcmp(iv2 + 48, iv + 48, 16) && iv2[16] == 0xEE && iv2[47] == 0xEE);
        CHECK(pos2[0] == 1 && pos2[3] == 15 && pos2[1] == 9 && pos2[2] == 9);
    }
    printf("stream_plan ok: %llu plans, %llu chunks\n", (unsigned long long)g_plans, (unsigned long long)g_chunks);
    return 0;
}
