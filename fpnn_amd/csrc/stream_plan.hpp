// stream_plan.hpp -- how fpnn_aes_stream_host cuts a call into pipeline chunks, for the staged
// and the host-mapped path alike (host_frames.hip).  Plain C++, no HIP: tests/cpp/stream_plan_test.cpp.
#pragma once

#include <string.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/fpnn_aes.h"

namespace fpnn_aes {

// A contiguous part of one frame's bytes, in staging order.
struct Piece {
    uint32_t frame, off, len;
};

// Stream-mode host frames grouped by stream: order[] lists the frame indices by key slot,
// each stream's frames in array order (a stable sort), and segs the streams that carry
// bytes, in slot order ({slot, first, nframes, bytes}: frames order[first .. +nframes)).
// A serial counting sort whose first pass also sums each slot's bytes, so the segments
// come from the histogram, not from a walk of frames[order[i]] (one cache miss per frame
// in arrival order).  A parallel form on the host pool (per-part histograms, prefix over
// slot ranges, per-part placement) measured 5-8 ms per 1M frames on the GPU box against
// this form's 3 (S1, gpurun_out r04k / r04l): four pool passes over a 16-CPU share cost
// more than they split.  Sparse slot ranges take std::stable_sort.
struct StreamSeg {
    uint32_t slot, first, nframes;
    uint64_t bytes;
};

inline void group_streams(const fpnn_aes_host_frame *frames, uint32_t n, uint32_t nkeys, std::vector<uint32_t> &order,
                          std::vector<StreamSeg> &segs) {
    order.resize(n);
    segs.clear();
    if ((uint64_t)nkeys > 4ull * n + 1024) {  // sparse
        for (uint32_t i = 0; i < n; i++) order[i] = i;
        std::stable_sort(order.begin(), order.end(),
                         [frames](uint32_t x, uint32_t y) { return frames[x].key_slot < frames[y].key_slot; });
        for (uint32_t i = 0; i < n;) {
            const uint32_t slot = frames[order[i]].key_slot;
            uint32_t j = i;
            uint64_t bytes = 0;
            while (j < n && frames[order[j]].key_slot == slot) bytes += frames[order[j++]].len;
            if (bytes) segs.push_back({slot, i, j - i, bytes});  // empty streams keep their state
            i = j;
        }
        return;
    }
    std::vector<uint32_t> cnt((size_t)nkeys + 1, 0);
    std::vector<uint64_t> byt(nkeys, 0);
    for (uint32_t i = 0; i < n; i++) {
        cnt[frames[i].key_slot + 1]++;
        byt[frames[i].key_slot] += frames[i].len;
    }
    for (uint32_t k = 0; k < nkeys; k++) {
        if (byt[k]) segs.push_back({k, cnt[k], cnt[k + 1], byt[k]});
        cnt[k + 1] += cnt[k];
    }
    for (uint32_t i = 0; i < n; i++) order[cnt[frames[i].key_slot]++] = i;
}

// One stream's share of a chunk: bytes [at, at + len) of the chunk's staging, key slot `slot`.
struct ChunkSeg {
    uint32_t slot;
    uint64_t at, len;
};

// The chunks of one call.  Round robin: each chunk takes up to `quota` bytes from each of a
// run of consecutive streams, so every kernel advances many CFB chains at once (the
// encrypt chain is serial: parallelism = streams per kernel).  A stream split across
// chunks continues from the state the earlier chunk left: chunks are ciphered in order.
struct StreamPlan {
    const fpnn_aes_host_frame *frames;
    std::vector<uint32_t> order;  // group_streams
    std::vector<StreamSeg> segs;
    std::vector<uint64_t> rem;    // per segment: bytes not yet in a chunk
    std::vector<uint32_t> fi, fo;  // per segment: frame cursor, offset inside that frame
    uint64_t left = 0;            // sum of rem
    uint64_t next = 0;            // round-robin cursor over segs

    StreamPlan(const fpnn_aes_host_frame *fr, uint32_t n, uint32_t nkeys) : frames(fr) {
        group_streams(frames, n, nkeys, order, segs);
        rem.resize(segs.size());
        fi.assign(segs.size(), 0);
        fo.assign(segs.size(), 0);
        for (size_t t = 0; t < segs.size(); t++) left += rem[t] = segs[t].bytes;
    }

    // The next chunk (false: every byte has been handed out): min(quota, what is left) bytes
    // of each of the segments state0, state0 + 1, ... until it holds chunk_bytes or the last
    // segment is reached; the next chunk starts behind them, or at the first segment again.
    // pieces: the frames' parts in staging order, back to back; segs_out: the segments'
    // shares; uniform_len: their common length, 0 if they differ.
    bool next_chunk(uint64_t chunk_bytes, uint64_t quota, std::vector<Piece> &pieces, std::vector<ChunkSeg> &segs_out,
                    uint64_t &state0, uint32_t &uniform_len) {
        pieces.clear();
        segs_out.clear();
        uniform_len = 0;
        if (left == 0) return false;
        const uint64_t nseg = segs.size();
        uint64_t t = next < nseg ? next : 0;
        while (rem[t] == 0) t = t + 1 < nseg ? t + 1 : 0;  // left > 0: terminates
        state0 = t;
        uint64_t in_b = 0;
        for (; t < nseg && in_b < chunk_bytes; t++) {
            const StreamSeg &sg = segs[t];
            const uint64_t take = std::min(rem[t], quota);
            uint64_t took = 0;
            while (took < take) {
                const uint32_t fidx = order[sg.first + fi[t]];
                const uint32_t flen = frames[fidx].len;
                const uint32_t part = (uint32_t)std::min<uint64_t>(flen - fo[t], take - took);
                if (part) pieces.push_back({fidx, fo[t], part});
                took += part;
                fo[t] += part;
                if (fo[t] == flen) {
                    fi[t]++;
                    fo[t] = 0;
                }
            }
            segs_out.push_back({sg.slot, in_b, take});
            rem[t] -= take;
            left -= take;
            in_b += take;
        }
        next = t;
        uniform_len = (uint32_t)segs_out[0].len;  // (segments lie back to back: equal lengths = a stride)
        for (const ChunkSeg &c : segs_out)
            if (c.len != uniform_len) uniform_len = 0;
        return true;
    }
};

// The compact state block of a call: iv[16] of every segment's stream, then their pos
// (u32), 20 bytes per segment -- what the chunks' kernels carry on the device.
inline void pack_stream_state(const std::vector<StreamSeg> &segs, const uint8_t *iv_state, const uint32_t *pos_state,
                              uint8_t *block) {
    uint32_t *pos = reinterpret_cast<uint32_t *>(block + 16 * segs.size());
    for (size_t t = 0; t < segs.size(); t++) {
        memcpy(block + 16 * t, iv_state + 16ull * segs[t].slot, 16);
        pos[t] = pos_state[segs[t].slot] & 15u;
    }
}

inline void unpack_stream_state(const std::vector<StreamSeg> &segs, const uint8_t *block, uint8_t *iv_state,
                                uint32_t *pos_state) {
    const uint32_t *pos = reinterpret_cast<const uint32_t *>(block + 16 * segs.size());
    for (size_t t = 0; t < segs.size(); t++) {
        memcpy(iv_state + 16ull * segs[t].slot, block + 16 * t, 16);
        pos_state[segs[t].slot] = pos[t];
    }
}

}  // namespace fpnn_aes
