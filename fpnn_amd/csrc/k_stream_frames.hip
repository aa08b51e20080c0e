// k_stream_frames.hip -- stream batches that carry MANY frames of each stream in one
// call (fpnn_aes_stream_encrypt_frames / _decrypt_frames, kernels.hpp FrameTable): a
// StreamEncryptor continues one CFB chain frame after frame (core/Encryptor.cpp:53-70)
// and FPNN's send queue holds several frames per connection and IO cycle
// (core/IOBuffer.cpp:47-74).
//
//   K2f   encrypt: one lane quad per stream (K2c's cipher, coop.hpp), the (iv, pos) state in
//         registers from the stream's first frame to its last
//   decrypt: the state pre-pass (two launches) that gives K1r (k_ragged.hip) every frame's
//         incoming state from ciphertext alone, and the per-stream commit that follows K1r
// Every kernel reaches a stream's state through stream_slot(): entry j of the state arrays
// for the calls above, entry state_slot[j] -- the connection's key-table slot, which is then
// its key slot too -- for the slot-addressed calls (fpnn_aes_stream_*_frames_at, _recv_at).
#include "coop.hpp"

namespace fpnn_aes {

namespace {

// Stream j's segments [f0, f1), clamped into the batch; a table that is not monotone from
// 0 to count is reported (kFaultFrameTable) and gives empty or overlapping ranges that
// still lie inside the batch.
__device__ __forceinline__ void stream_range(const KBatch &b, const FrameTable &f, uint32_t j, uint32_t &f0,
                                             uint32_t &f1) {
    const uint32_t cnt = (uint32_t)b.count;
    if (!f.first_frame) {  // one frame per stream: stream j is segment j
        f0 = min(j, cnt);
        f1 = min(j + 1u, cnt);
        return;
    }
    const uint32_t r0 = *FA_AT(b, AB_FIRST_FRAME, f.first_frame + j, 4);
    const uint32_t r1 = *FA_AT(b, AB_FIRST_FRAME, f.first_frame + j + 1, 4);
    const bool bad = r1 < r0 || r1 > cnt || (j == 0 && r0 != 0u) || (j + 1 == f.nstreams && r1 != cnt);
    f0 = min(r0, cnt);
    f1 = max(min(r1, cnt), f0);
    if (bad && f.fault) __hip_atomic_store(f.fault, kFaultFrameTable, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Where stream j's state lives, and in a slot-addressed call its key: entry s of the state
// arrays (slot s of b.keys).  Without state_slot that is j.  false: state_slot[j] lies at or
// past slot_bound -- reported, s = 0, and the caller touches no state for this stream.
__device__ __forceinline__ bool stream_slot(const KBatch &b, const FrameTable &f, uint32_t j, uint32_t &s) {
    s = j;
    if (!f.state_slot) return true;
    s = *FA_AT(b, AB_STATE_SLOT, f.state_slot + j, 4);
    if (s < f.slot_bound) return true;
    if (f.fault) __hip_atomic_fetch_or(f.fault, kFaultKeySlot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    s = 0u;
    return false;
}

// One frame's descriptor (no key slot: a stream's frames share one, read once per stream).
struct FrameDesc {
    const uint8_t *in;
    uint8_t *out;
    uint32_t len;
};

__device__ __forceinline__ FrameDesc frame_desc(const KBatch &b, uint64_t s) {
    FrameDesc d;
    const uint64_t io = b.in_off ? *FA_AT(b, AB_IN_OFF, b.in_off + s, 8) : s * b.stride;
    const uint64_t oo = b.out_off ? *FA_AT(b, AB_OUT_OFF, b.out_off + s, 8) : io;
    d.in = b.in + io;
    d.out = b.out + oo;
    d.len = b.len ? *FA_AT(b, AB_LEN, b.len + s, 4) : b.uniform_len;
    return d;
}

// bytes of a frame of `len` bytes that finish the keystream block carried at position n
__device__ __forceinline__ uint32_t head_bytes(uint32_t n, uint32_t len) { return n ? min(len, 16u - n) : 0u; }

}  // namespace

// ---------------------------------------------------------------------------
// K2f: per frame the work is K2c's STREAM path (k_encrypt.hip) -- the head bytes that
// finish the carried keystream block, 8-block steps with the next step's words already
// loading, single blocks, the partial tail -- and the chain is kept fed across frame
// boundaries: descriptors are read two frames ahead (frame k + 2's when frame k starts,
// so frame k + 1's are in registers by then), and the 8 words of frame k + 1's first
// step are loaded by frame k's LAST step in place of that step's dummy loads (at the
// frame's start when it has no 8-block step).  All of these loads are unconditional, for
// the reason the step loop of K2c documents: past the stream's end they re-read its last
// descriptor and the first DevKey (an L2 hit).
//
// ONE loop runs the steps of all of a stream's frames: an iteration is an 8-block step
// when the quad has one, else the frame's end (singles, tail) and the next frame's start
// (head).  The 16 quads of a wave hold 16 streams whose frames end at different blocks;
// with a step loop per frame inside a frame loop the wave stayed in every frame's step
// loop until its LONGEST of 16 frames was done -- C3's one-call encrypt ran at 61 GiB/s
// against 131.6 for the whole streams (mean frame 32 KiB, mean longest-of-16 ~ 60 KiB).
// Here a quad at a frame edge costs its wave only that edge's few blocks.
template <int NR, int KM, int NT>
__global__ __launch_bounds__(kThreads, 4) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_cfb_encrypt_stream_frames(
    KBatch b, FrameTable f) {
    __shared__ uint4 lds4[Lds<NT>::kBytes / 16];
    lds_fill_tables<NT>(lds4, b.t0le);
    __syncthreads();
    const Tables4<NT> T{reinterpret_cast<const char *>(lds4), LaneBase()};
    const int q = (int)(threadIdx.x & 3u);
    constexpr int CH = 8;
    const int wlo = 4 * q;  // block bytes [wlo, wlo + 4) belong to this lane
    const uint8_t *const dummy = reinterpret_cast<const uint8_t *>(b.keys) + wlo;  // 16 * CH readable bytes

    const uint64_t nquads = ((uint64_t)gridDim.x * blockDim.x) >> 2;
    for (uint64_t t = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2; t < f.nstreams; t += nquads) {
        uint32_t f0, f1, ss;
        if (!stream_slot(b, f, (uint32_t)t, ss)) continue;  // a slot past the bound: nothing is written
        stream_range(b, f, (uint32_t)t, f0, f1);
        if (f0 >= f1) continue;  // no segment: the state stays as it is
        const uint32_t slot = KM == KEY_UNIFORM ? 0u
                              : f.state_slot    ? ss
                              : b.key_slot      ? *FA_AT(b, AB_SLOT, b.key_slot + f0, 4)
                                                : 0u;
        const DevKey *key = FA_AT(b, AB_KEYS, b.keys + slot, sizeof(DevKey));
        uint32_t rkq[NR + 1];
#pragma unroll
        for (int r = 0; r <= NR; r++) rkq[r] = key->rk[4 * r + q];
        const uint32_t rkx = rkq[NR] ^ rkq[0];
        // this lane's word of the 16-byte feedback register, and the CFB position
        uint32_t iv = reinterpret_cast<const uint32_t *>(FA_AT(b, AB_IV_STATE, b.iv_state + 16ull * ss, 16))[q];
        uint32_t n = *FA_AT(b, AB_POS_STATE, b.pos_state + ss, 4) & 15u;

        FrameDesc cur = frame_desc(b, f0);
        FrameDesc nxt = frame_desc(b, min(f0 + 1u, f1 - 1u));
        FrameDesc nn = nxt;
        uint32_t k = f0;
        uint32_t hd = head_bytes(n, cur.len);
        bool big = ((cur.len - hd) >> 4) >= (uint32_t)CH;  // the frame has an 8-block step: a[] holds its first
        FA_DECL(a_ilo = (uintptr_t)cur.in, a_ihi = (uintptr_t)cur.in + cur.len, a_olo = 0, a_ohi = 0, a_nlo = 0,
                a_nhi = 0);
        uint32_t a[CH];
        {
            const uint8_t *pa = big ? cur.in + hd + wlo : dummy;
#pragma unroll
            for (int j = 0; j < CH; j++)
                a[j] = *reinterpret_cast<const uint32_u *>(big ? FA_SEG(b, AB_IN, pa + 16 * j, 4, a_ilo, a_ihi)
                                                               : FA_AT(b, AB_KEYS, pa + 16 * j, 4));
        }
        // the running frame
        const uint8_t *p = cur.in, *pn1 = dummy;
        uint8_t *o = cur.out;
        uint32_t nfull = 0, i = 0, tail = 0, hd1 = 0;
        bool big1 = false;
        // frame k starts: descriptors two ahead, the next frame's first step, the head bytes
        auto begin_frame = [&]() {
            nn = frame_desc(b, min(k + 2u, f1 - 1u));  // two frames ahead
            FA_SET(a_ilo, (uintptr_t)cur.in);
            FA_SET(a_ihi, (uintptr_t)cur.in + cur.len);
            FA_SET(a_olo, (uintptr_t)cur.out);
            FA_SET(a_ohi, (uintptr_t)cur.out + cur.len);
            FA_SET(a_nlo, (uintptr_t)nxt.in);
            FA_SET(a_nhi, (uintptr_t)nxt.in + nxt.len);
            // the next frame's first step (its position is known before this frame runs)
            hd1 = head_bytes((n + cur.len) & 15u, nxt.len);
            big1 = k + 1u < f1 && ((nxt.len - hd1) >> 4) >= (uint32_t)CH;
            pn1 = big1 ? nxt.in + hd1 + wlo : dummy;
            if (!big) {  // no 8-block step in this frame: a[] is free now
#pragma unroll
                for (int j = 0; j < CH; j++)
                    a[j] = *reinterpret_cast<const uint32_u *>(big1 ? FA_SEG(b, AB_IN, pn1 + 16 * j, 4, a_nlo, a_nhi)
                                                                    : FA_AT(b, AB_KEYS, pn1 + 16 * j, 4));
            }
            p = cur.in;
            o = cur.out;
            uint32_t rem = cur.len;
            if (n != 0 && rem != 0) {  // rest of the partially used keystream block
                const uint32_t take = hd;
                const int lo = max((int)n, wlo) - wlo, hi = min((int)(n + take), wlo + 4) - wlo;
                if (lo < hi) {
                    const uint32_t c = load_word_bytes(FA_RG(b, AB_IN, p - n + wlo, lo, hi, a_ilo, a_ihi), lo, hi) ^ iv;
                    store_word_bytes(FA_RG(b, AB_OUT, o - n + wlo, lo, hi, a_olo, a_ohi), c, lo, hi);
                    const uint32_t m = word_mask(lo, hi);
                    iv = (c & m) | (iv & ~m);
                }
                p += take;
                o += take;
                rem -= take;
                n = (n + take) & 15u;
            }
            nfull = rem >> 4;
            tail = rem & 15u;
            i = 0;
        };
        begin_frame();
        for (bool alive = true; alive;) {
            if (i + CH <= nfull) {  // ---- one 8-block step (a[] holds its words)
                // the next step's words; the frame's last step loads the NEXT FRAME's first
                // step instead (or the first DevKey when that frame has none)
                const bool more = i + 2 * CH <= nfull;
                const uint8_t *pn = more ? p + 16 * CH + wlo : pn1;
                uint32_t nx[CH], c[CH];
#pragma unroll
                for (int j = 0; j < CH; j++)
                    nx[j] = *reinterpret_cast<const uint32_u *>(
                        more   ? FA_SEG(b, AB_IN, pn + 16 * j, 4, a_ilo, a_ihi)
                        : big1 ? FA_SEG(b, AB_IN, pn + 16 * j, 4, a_nlo, a_nhi)
                               : FA_AT(b, AB_KEYS, pn + 16 * j, 4));
                // the chain carries C ^ rk[0] (aes_chain_column: its two XORs folded into the keys)
                uint32_t sw = iv ^ rkq[0];
#pragma unroll
                for (int j = 0; j < CH; j++) {
                    sw = aes_chain_column<NR, NT>(sw, rkq, rkx ^ a[j], T);
                    c[j] = sw ^ rkq[0];
                }
                iv = c[CH - 1];
                // the step's 8 words go out together (each quad's 128-B line in 8 back-to-back
                // stores), and the loaded words are handed on after the rounds: as in K2c
#pragma unroll
                for (int j = 0; j < CH; j++) asm volatile("" : "+v"(c[j]));
#pragma unroll
                for (int j = 0; j < CH; j++)
                    *reinterpret_cast<uint32_u *>(FA_SEG(b, AB_OUT, o + 16 * j + wlo, 4, a_olo, a_ohi)) = c[j];
#pragma unroll
                for (int j = 0; j < CH; j++) {
                    asm volatile("" : "+v"(nx[j]));
                    a[j] = nx[j];
                }
                p += 16 * CH;
                o += 16 * CH;
                i += CH;
            } else {  // ---- frame k ends, the next one starts
                if (i < nfull) {  // up to 7 single blocks, each one's word loading behind its predecessor's rounds
                    uint32_t pt = *reinterpret_cast<const uint32_u *>(FA_SEG(b, AB_IN, p + wlo, 4, a_ilo, a_ihi));
                    for (; i < nfull; i++) {
                        const bool more = i + 1 < nfull;
                        const uint32_t ptn = *reinterpret_cast<const uint32_u *>(
                            more ? FA_SEG(b, AB_IN, p + 16 + wlo, 4, a_ilo, a_ihi) : FA_AT(b, AB_KEYS, dummy, 4));
                        iv = aes_encrypt_column<NR, NT>(iv, rkq, T) ^ pt;
                        *reinterpret_cast<uint32_u *>(FA_SEG(b, AB_OUT, o + wlo, 4, a_olo, a_ohi)) = iv;
                        pt = ptn;
                        p += 16;
                        o += 16;
                    }
                }
                if (tail) {  // partial final block: the frame ends inside a keystream block
                    const uint32_t ks = aes_encrypt_column<NR, NT>(iv, rkq, T);
                    const int lo = 0, hi = min((int)tail, wlo + 4) - wlo;
                    if (hi > lo) {
                        const uint32_t c = load_word_bytes(FA_RG(b, AB_IN, p + wlo, lo, hi, a_ilo, a_ihi), lo, hi) ^ ks;
                        store_word_bytes(FA_RG(b, AB_OUT, o + wlo, lo, hi, a_olo, a_ohi), c, lo, hi);
                        const uint32_t m = word_mask(lo, hi);
                        iv = (c & m) | (ks & ~m);
                    } else {
                        iv = ks;
                    }
                    n = tail;
                }
                if (++k >= f1) {
                    alive = false;
                } else {
                    cur = nxt;
                    nxt = nn;
                    hd = hd1;
                    big = big1;
                    begin_frame();
                }
            }
        }
        reinterpret_cast<uint32_t *>(FA_AT(b, AB_IV_STATE, b.iv_state + 16ull * ss, 16))[q] = iv;
        if (q == 0) *FA_AT(b, AB_POS_STATE, b.pos_state + ss, 4) = n;
    }
}

// ---------------------------------------------------------------------------
// Decrypt pre-pass, first launch: one lane per stream walks its frames' lengths.
//   snap_pos[k]   the CFB position frame k starts at, (p0 + bytes of the frames before it) & 15
//   seg_stream[k] the stream frame k belongs to
//   seg_prev[k]   the last non-empty frame of the stream before k (~0: none)
//   seg_slot[k]   slot-addressed calls: the stream's key slot, for K1r's per-segment b.key_slot
__global__ __launch_bounds__(256) void k_stream_frames_walk(KBatch b, FrameTable f, uint32_t *__restrict__ snap_pos,
                                                            uint32_t *__restrict__ seg_stream,
                                                            uint32_t *__restrict__ seg_prev) {
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < f.nstreams; j += nthreads) {
        uint32_t f0, f1, ss;
        const bool live = stream_slot(b, f, (uint32_t)j, ss);
        stream_range(b, f, (uint32_t)j, f0, f1);
        if (f0 >= f1) continue;
        uint32_t n = live ? *FA_AT(b, AB_POS_STATE, b.pos_state + ss, 4) & 15u : 0u;
        uint32_t prev = ~0u;
        for (uint32_t k = f0; k < f1; k++) {
            const uint32_t len = b.len ? *FA_AT(b, AB_LEN, b.len + k, 4) : b.uniform_len;
            snap_pos[k] = n;
            seg_stream[k] = (uint32_t)j;
            seg_prev[k] = prev;
            if (f.seg_slot) *FA_AT(b, AB_SEG_SLOT, f.seg_slot + k, 4) = ss;
            if (len) prev = k;
            n = (n + len) & 15u;
        }
    }
}

// Second launch: one lane per segment, its frame's incoming ivec (base/rijndael.c:1186-1198
// unrolled; what K1r exports for a segment's last block, k_ragged.hip).  V = the p0 bytes
// of iv0 the stream's current block already holds -- at p0 == 0 all 16: iv0 is then the
// last complete ciphertext block, not yet enciphered -- then the stream's ciphertext of this
// call; the frame starts at Q = (p0 or 16) + (bytes of the frames before it), p = Q & 15:
//   Q < 16   ivec = V[0, Q) then iv0[Q, 16)                       (no block boundary yet)
//   else     C = V[Q - p - 16, Q - p), the last complete block;  ivec = C when p == 0,
//            else V[Q - p, Q) then E_K(C)[p, 16)
// The lane gathers the min(Q, 16 + p) bytes before Q backwards, over as many earlier
// frames as they span (seg_prev skips the empty ones) and into iv0 where they reach before
// the call.  A segment no stream owns (a malformed table) gets a zero state.
template <int NR, int KM>
__global__ __launch_bounds__(kThreads) void k_stream_frames_state(KBatch b, FrameTable f, uint4 *__restrict__ snap_iv,
                                                                  uint32_t *__restrict__ snap_pos,
                                                                  const uint32_t *__restrict__ seg_stream,
                                                                  const uint32_t *__restrict__ seg_prev) {
    constexpr int NT = 4;
    __shared__ uint4 lds4[Lds<NT>::kBytes / 16];
    lds_fill_tables<NT>(lds4, b.t0le);
    __syncthreads();
    const Tables4<NT> T{reinterpret_cast<const char *>(lds4), LaneBase()};
    RoundKeys<NR> rk;
    if (KM == KEY_UNIFORM) rk = load_round_keys<NR>(FA_AT(b, AB_KEYS, b.keys, sizeof(DevKey)));
    const uint32_t cnt = (uint32_t)b.count;
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < cnt; k += nthreads) {
        const uint32_t j = seg_stream[k];
        uint32_t f0 = 0, f1 = 0;
        if (j < f.nstreams) stream_range(b, f, j, f0, f1);
        if (!(k >= f0 && k < f1)) {  // not written by this call's walk
            snap_iv[k] = make_uint4(0, 0, 0, 0);
            snap_pos[k] = 0u;
            if (f.seg_slot) *FA_AT(b, AB_SEG_SLOT, f.seg_slot + k, 4) = 0u;  // (K1r reads every segment's)
            if (f.fault) __hip_atomic_store(f.fault, kFaultFrameTable, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            continue;
        }
        const uint32_t pk = snap_pos[k] & 15u;
        uint32_t ss;  // (a slot past the bound: a zero state; the walk has reported it)
        const bool live = stream_slot(b, f, j, ss);
        const uint32_t p0 = live ? *FA_AT(b, AB_POS_STATE, b.pos_state + ss, 4) & 15u : 0u;
        const uint4 iv0 = live ? *reinterpret_cast<const uint4 *>(FA_AT(b, AB_IV_STATE, b.iv_state + 16ull * ss, 16))
                               : make_uint4(0, 0, 0, 0);
        // w: the gathered bytes as one little-endian number, the earliest byte lowest
        uint64_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
        auto push = [&](uint32_t byte) {
            w3 = (w3 << 8) | (w2 >> 56);
            w2 = (w2 << 8) | (w1 >> 56);
            w1 = (w1 << 8) | (w0 >> 56);
            w0 = (w0 << 8) | byte;
        };
        const uint32_t need = 16u + pk;
        uint32_t got = 0;
        for (uint32_t s = seg_prev[k]; got < need && s >= f0 && s < k;) {
            const FrameDesc d = frame_desc(b, s);
            FA_DECL(a_ilo = (uintptr_t)d.in, a_ihi = (uintptr_t)d.in + d.len);
            const uint32_t take = min(d.len, need - got);
            for (uint32_t t = 0; t < take; t++)
                push(*FA_SEG(b, AB_IN, d.in + (d.len - 1u - t), 1, a_ilo, a_ihi));
            got += take;
            const uint32_t s2 = seg_prev[s];
            if (s2 >= s) break;  // ~0: the stream's first non-empty frame
            s = s2;
        }
        if (got < need) {  // the bytes before the call: iv0[0, p0), or all of iv0 at p0 == 0
            const uint32_t pre = p0 ? p0 : 16u;
            const uint32_t take = min(pre, need - got);
            for (uint32_t t = 0; t < take; t++) push(byte_of(iv0, (int)(pre - 1u - t)));
            got += take;
        }
        const uint4 lo16 = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
        const uint4 hi16 = make_uint4((uint32_t)w2, (uint32_t)(w2 >> 32), (uint32_t)w3, (uint32_t)(w3 >> 32));
        if (KM != KEY_UNIFORM) {
            const uint32_t slot = b.key_slot ? *FA_AT(b, AB_SLOT, b.key_slot + k, 4) : 0u;
            rk = load_round_keys<NR>(FA_AT(b, AB_KEYS, b.keys + slot, sizeof(DevKey)));
        }
        const uint4 e = aes_encrypt_block<NR, NT>(lo16, rk, T);  // (used when a boundary was passed and pk != 0)
        uint4 iv;
        if (got < need) iv = select_bytes(byte_mask(0, (int)min(got, 16u)), lo16, iv0);
        else iv = pk ? select_bytes(byte_mask(0, (int)pk), hi16, e) : lo16;
        snap_iv[k] = iv;
    }
}

// After K1r: stream j takes the state its last non-empty frame exported (into its slot's
// entry; a stream whose slot lies past the bound commits nothing).
__global__ __launch_bounds__(256) void k_stream_frames_commit(KBatch b, FrameTable f, const uint4 *__restrict__ seg_iv,
                                                              const uint32_t *__restrict__ seg_pos) {
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < f.nstreams; j += nthreads) {
        uint32_t f0, f1, ss;
        if (!stream_slot(b, f, (uint32_t)j, ss)) continue;
        stream_range(b, f, (uint32_t)j, f0, f1);
        for (uint32_t k = f1; k > f0;) {
            k--;
            const uint32_t len = b.len ? *FA_AT(b, AB_LEN, b.len + k, 4) : b.uniform_len;
            if (len) {
                *reinterpret_cast<uint4 *>(FA_AT(b, AB_IV_STATE, b.iv_state + 16ull * ss, 16)) = seg_iv[k];
                *FA_AT(b, AB_POS_STATE, b.pos_state + ss, 4) = seg_pos[k];
                break;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Launchers

template <int NR>
static void k2f_nr(const KBatch &b, const FrameTable &f, KeyMode km, int grid, int threads, hipStream_t st) {
    if (km == KEY_UNIFORM)
        hipLaunchKernelGGL((k_cfb_encrypt_stream_frames<NR, KEY_UNIFORM, 4>), dim3(grid), dim3(threads), 0, st, b, f);
    else
        hipLaunchKernelGGL((k_cfb_encrypt_stream_frames<NR, KEY_LANE, 4>), dim3(grid), dim3(threads), 0, st, b, f);
}

hipError_t launch_encrypt_stream_frames(const KBatch &b, const FrameTable &f, int nrounds, KeyMode km, int grid,
                                        int threads, hipStream_t st) {
    set_launched("cfb_encrypt_stream_frames");
    switch (nrounds) {
        case 10: k2f_nr<10>(b, f, km, grid, threads, st); break;
        case 12: k2f_nr<12>(b, f, km, grid, threads, st); break;
        case 14: k2f_nr<14>(b, f, km, grid, threads, st); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int NR>
static void state_nr(const KBatch &b, const FrameTable &f, KeyMode km, uint4 *snap_iv, uint32_t *snap_pos,
                     const uint32_t *seg_stream, const uint32_t *seg_prev, int grid, hipStream_t st) {
    if (km == KEY_UNIFORM)
        hipLaunchKernelGGL((k_stream_frames_state<NR, KEY_UNIFORM>), dim3(grid), dim3(kThreads), 0, st, b, f, snap_iv,
                           snap_pos, seg_stream, seg_prev);
    else
        hipLaunchKernelGGL((k_stream_frames_state<NR, KEY_LANE>), dim3(grid), dim3(kThreads), 0, st, b, f, snap_iv,
                           snap_pos, seg_stream, seg_prev);
}

hipError_t launch_stream_frames_state(const KBatch &b, const FrameTable &f, int nrounds, KeyMode km, uint4 *snap_iv,
                                      uint32_t *snap_pos, uint32_t *seg_stream, uint32_t *seg_prev, int num_cus,
                                      hipStream_t st) {
    if (nrounds != 10 && nrounds != 12 && nrounds != 14) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_stream_frames_walk, dim3(grid_for(f.nstreams, 256, 4 * num_cus)), dim3(256), 0, st, b, f,
                       snap_pos, seg_stream, seg_prev);
    const int grid = grid_for(b.count, kThreads, num_cus);
    switch (nrounds) {
        case 10: state_nr<10>(b, f, km, snap_iv, snap_pos, seg_stream, seg_prev, grid, st); break;
        case 12: state_nr<12>(b, f, km, snap_iv, snap_pos, seg_stream, seg_prev, grid, st); break;
        default: state_nr<14>(b, f, km, snap_iv, snap_pos, seg_stream, seg_prev, grid, st); break;
    }
    return hipGetLastError();
}

hipError_t launch_stream_frames_commit(const KBatch &b, const FrameTable &f, const uint4 *seg_iv,
                                       const uint32_t *seg_pos, hipStream_t st) {
    // (fault: the pre-pass has reported a bad table already)
    FrameTable g = f;
    g.fault = nullptr;
    hipLaunchKernelGGL(k_stream_frames_commit, dim3(grid_for(f.nstreams, 256, 1 << 20)), dim3(256), 0, st, b, g, seg_iv,
                       seg_pos);
    return hipGetLastError();
}

}  // namespace fpnn_aes
