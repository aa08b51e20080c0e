// k_keytable.hip -- writes into a LIVE key table, queued on the engine stream like a batch
// (fpnn_aes_keyset_set_keys / _clear, fpnn_ecdh_accept): a server's accept and close paths
// with no key byte in host memory.
//   k_set_keys    one lane per entry: raw key (16 / 24 / 32 bytes) + 16-byte IV -> the whole
//                 DevKey of the entry's slot (FIPS-197 expansion as k_expand_keys does it,
//                 base/rijndael.c:712-799: big-endian words, stored byte-swapped) AND
//                 eiv[slot] = E_k(IV), in the same lane: the round keys are in its registers
//                 already, and the package encrypt kernels take block 0 from eiv[], so the two
//                 must never be seen apart by a later batch.
//   k_clear_slots the slot becomes what a never-set slot of fpnn_aes_keyset_reserve holds: a
//                 zero DevKey and the E(0) the rounds give under all-zero round keys.
//   k_stream_open / k_stream_close (fpnn_aes_stream_open / _close): the stream state of a
//                 slot, (IV, 0) from the slot's DevKey and all zero, in the caller's arrays
//                 indexed by slot.
// Addressing, all kernels: slot s_i = slots ? slots[i] : first + i.  An entry with
// s_i >= slot_bound writes nothing and ORs kFaultKeySlot into the engine's fault word (the
// next sync returns FPNN_AES_ERR_DEVICE) -- the host sized the table for slot_bound, so no
// store can leave it whatever slots[] holds.  k_set_keys skips entries with ok[i] == 0.
//
// The cipher here is one block per key, so it does not bring up the 128 KiB replicated table
// image of the batch kernels: T0 alone (1 KiB, little-endian form) sits in LDS, T1..T3 are
// rotations of it and the final round's S-box byte is byte 1 of the T0 entry.  Lookups of a
// wave's lanes collide on banks; at one block per accepted connection that is noise beside
// the 17 scattered 16-byte stores of the DevKey.
#include "kernels.hpp"

namespace fpnn_aes {

namespace {

constexpr int kKtThreads = 256;  // == T0 entries: thread x loads T0[x]

__device__ __forceinline__ uint32_t t0_rot(const uint32_t *t0, uint32_t w, int j) {
    return __builtin_rotateleft32(t0[(w >> (8 * j)) & 0xffu], 8u * j);
}

__device__ __forceinline__ uint32_t sbox_of_t0(const uint32_t *t0, uint32_t x) { return (t0[x & 0xffu] >> 8) & 0xffu; }

// SubWord of a big-endian schedule word
__device__ __forceinline__ uint32_t sub_word(const uint32_t *t0, uint32_t t) {
    return (sbox_of_t0(t0, t >> 24) << 24) | (sbox_of_t0(t0, t >> 16) << 16) | (sbox_of_t0(t0, t >> 8) << 8) |
           sbox_of_t0(t0, t);
}

// One block under round keys rk[0 .. 4 * NR + 3] in block byte order (aes_encrypt_block's
// round, aes_device.hpp, with T_j = rotl(T0, 8 j)).
template <int NR>
__device__ __forceinline__ uint4 encrypt_block_t0(uint4 in, const uint32_t (&rk)[60], const uint32_t *t0) {
    uint32_t s0 = in.x ^ rk[0], s1 = in.y ^ rk[1], s2 = in.z ^ rk[2], s3 = in.w ^ rk[3];
#pragma unroll
    for (int r = 1; r < NR; r++) {
        const uint32_t a = t0_rot(t0, s0, 0) ^ t0_rot(t0, s1, 1) ^ t0_rot(t0, s2, 2) ^ t0_rot(t0, s3, 3) ^ rk[4 * r + 0];
        const uint32_t b = t0_rot(t0, s1, 0) ^ t0_rot(t0, s2, 1) ^ t0_rot(t0, s3, 2) ^ t0_rot(t0, s0, 3) ^ rk[4 * r + 1];
        const uint32_t c = t0_rot(t0, s2, 0) ^ t0_rot(t0, s3, 1) ^ t0_rot(t0, s0, 2) ^ t0_rot(t0, s1, 3) ^ rk[4 * r + 2];
        const uint32_t d = t0_rot(t0, s3, 0) ^ t0_rot(t0, s0, 1) ^ t0_rot(t0, s1, 2) ^ t0_rot(t0, s2, 3) ^ rk[4 * r + 3];
        s0 = a; s1 = b; s2 = c; s3 = d;
    }
    auto last = [&](uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t k) {
        return (sbox_of_t0(t0, a) | (sbox_of_t0(t0, b >> 8) << 8) | (sbox_of_t0(t0, c >> 16) << 16) |
                (sbox_of_t0(t0, d >> 24) << 24)) ^ k;
    };
    return make_uint4(last(s0, s1, s2, s3, rk[4 * NR + 0]), last(s1, s2, s3, s0, rk[4 * NR + 1]),
                      last(s2, s3, s0, s1, rk[4 * NR + 2]), last(s3, s0, s1, s2, rk[4 * NR + 3]));
}

// The entry's slot, or false (with the fault reported) when it lies at or past slot_bound.
__device__ __forceinline__ bool slot_of(const KeyTableArgs &a, uint32_t i, uint32_t &s) {
    s = a.slots ? *FA_AT(a, AB_KT_SLOTS, a.slots + i, 4) : a.first + i;
    if (s < a.slot_bound) return true;
    if (a.fault) __hip_atomic_fetch_or(a.fault, kFaultKeySlot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return false;
}

// DevKey of slot s = rk[] | nrounds, keylen, reserved | iv, as 17 16-byte stores
__device__ __forceinline__ void store_slot(const KeyTableArgs &a, uint32_t s, const uint32_t (&rk)[60], uint4 meta,
                                           uint4 iv, uint4 eiv) {
    uint4 *d = reinterpret_cast<uint4 *>(FA_AT(a, AB_KEYS, a.keys + s, sizeof(DevKey)));
#if FA_ON
    // (a DevKey is larger than the audit table's scratch: a reported store is dropped)
    if (a.aud && reinterpret_cast<uint8_t *>(d) == a.aud->scratch) return;
#endif
#pragma unroll
    for (int k = 0; k < 15; k++) d[k] = make_uint4(rk[4 * k], rk[4 * k + 1], rk[4 * k + 2], rk[4 * k + 3]);
    d[15] = meta;
    d[16] = iv;
    *FA_AT(a, AB_EIV, a.eiv + s, 16) = eiv;
}

template <int NK>
__global__ __launch_bounds__(kKtThreads) void k_set_keys(const KeyTableArgs a) {
    constexpr int NR = NK + 6, NW = 4 * (NR + 1);
    __shared__ uint32_t t0[256];
    t0[threadIdx.x] = a.t0le[threadIdx.x];
    __syncthreads();
    const uint32_t i = blockIdx.x * kKtThreads + threadIdx.x;
    if (i >= a.count) return;
    if (a.ok && *FA_AT(a, AB_KT_OK, a.ok + i, 1) == 0) return;
    uint32_t s;
    if (!slot_of(a, i, s)) return;
    // (byte loads: the caller's key and IV arrays carry no alignment promise)
    const uint8_t *key = FA_AT(a, AB_KT_RAW, a.raw + (uint64_t)i * (4 * NK), 4 * NK);
    uint32_t w[60];
#pragma unroll
    for (int k = 0; k < NK; k++)
        w[k] = ((uint32_t)key[4 * k] << 24) | ((uint32_t)key[4 * k + 1] << 16) | ((uint32_t)key[4 * k + 2] << 8) |
               key[4 * k + 3];
    uint32_t rcon = 1;
#pragma unroll
    for (int k = NK; k < NW; k++) {
        uint32_t t = w[k - 1];
        if (k % NK == 0) {
            t = sub_word(t0, (t << 8) | (t >> 24)) ^ (rcon << 24);
            rcon = ((rcon << 1) ^ ((rcon & 0x80) ? 0x1b : 0)) & 0xff;
        } else if (NK > 6 && k % NK == 4) {
            t = sub_word(t0, t);
        }
        w[k] = w[k - NK] ^ t;
    }
#pragma unroll
    for (int k = 0; k < 60; k++) w[k] = k < NW ? __builtin_bswap32(w[k]) : 0u;
    uint4 iv = make_uint4(0, 0, 0, 0);
    if (a.ivs) {
        const uint8_t *p = FA_AT(a, AB_KT_IVS, a.ivs + 16 * (uint64_t)i, 16);
        uint32_t v[4];
#pragma unroll
        for (int q = 0; q < 4; q++)
            v[q] = (uint32_t)p[4 * q] | ((uint32_t)p[4 * q + 1] << 8) | ((uint32_t)p[4 * q + 2] << 16) |
                   ((uint32_t)p[4 * q + 3] << 24);
        iv = make_uint4(v[0], v[1], v[2], v[3]);
    }
    store_slot(a, s, w, make_uint4((uint32_t)NR, 4u * NK, 0u, 0u), iv, encrypt_block_t0<NR>(iv, w, t0));
}

template <int NR>
__global__ __launch_bounds__(kKtThreads) void k_clear_slots(const KeyTableArgs a) {
    __shared__ uint32_t t0[256];
    t0[threadIdx.x] = a.t0le[threadIdx.x];
    __syncthreads();
    const uint32_t i = blockIdx.x * kKtThreads + threadIdx.x;
    if (i >= a.count) return;
    uint32_t s;
    if (!slot_of(a, i, s)) return;
    uint32_t w[60];
#pragma unroll
    for (int k = 0; k < 60; k++) w[k] = 0u;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    store_slot(a, s, w, zero, zero, encrypt_block_t0<NR>(zero, w, t0));
}

// Stream state by slot: a connection's StreamEncryptor starts from (_iv = the connection
// IV, _pos = 0) (core/Encryptor.h:44-61), and after fpnn_ecdh_accept that IV exists only in
// the slot's DevKey.  The table is read, the caller's state arrays (slot_bound entries) are
// written; a cleared or never-set slot holds a zero IV and gives an all-zero state.
__global__ __launch_bounds__(kKtThreads) void k_stream_open(const KeyTableArgs a) {
    const uint32_t i = blockIdx.x * kKtThreads + threadIdx.x;
    if (i >= a.count) return;
    if (a.ok && *FA_AT(a, AB_KT_OK, a.ok + i, 1) == 0) return;
    uint32_t s;
    if (!slot_of(a, i, s)) return;
    *FA_AT(a, AB_IV_STATE, a.iv_state + s, 16) = *reinterpret_cast<const uint4 *>(FA_AT(a, AB_KEYS, a.keys[s].iv, 16));
    *FA_AT(a, AB_POS_STATE, a.pos_state + s, 4) = 0u;
}

__global__ __launch_bounds__(kKtThreads) void k_stream_close(const KeyTableArgs a) {
    const uint32_t i = blockIdx.x * kKtThreads + threadIdx.x;
    if (i >= a.count) return;
    uint32_t s;
    if (!slot_of(a, i, s)) return;
    *FA_AT(a, AB_IV_STATE, a.iv_state + s, 16) = make_uint4(0, 0, 0, 0);
    *FA_AT(a, AB_POS_STATE, a.pos_state + s, 4) = 0u;
}

}  // namespace

hipError_t launch_stream_open(const KeyTableArgs &a, hipStream_t st) {
    if (a.count == 0) return hipSuccess;
    set_launched("stream_open");
    hipLaunchKernelGGL(k_stream_open, dim3((a.count + kKtThreads - 1) / kKtThreads), dim3(kKtThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_stream_close(const KeyTableArgs &a, hipStream_t st) {
    if (a.count == 0) return hipSuccess;
    set_launched("stream_close");
    hipLaunchKernelGGL(k_stream_close, dim3((a.count + kKtThreads - 1) / kKtThreads), dim3(kKtThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_set_keys(const KeyTableArgs &a, uint32_t keylen, hipStream_t st) {
    if (a.count == 0) return hipSuccess;
    set_launched("set_keys");
    const dim3 grid((a.count + kKtThreads - 1) / kKtThreads);
    switch (keylen) {
        case 16: hipLaunchKernelGGL(k_set_keys<4>, grid, dim3(kKtThreads), 0, st, a); break;
        case 24: hipLaunchKernelGGL(k_set_keys<6>, grid, dim3(kKtThreads), 0, st, a); break;
        case 32: hipLaunchKernelGGL(k_set_keys<8>, grid, dim3(kKtThreads), 0, st, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_clear_slots(const KeyTableArgs &a, int nrounds, hipStream_t st) {
    if (a.count == 0) return hipSuccess;
    set_launched("clear_slots");
    const dim3 grid((a.count + kKtThreads - 1) / kKtThreads);
    switch (nrounds) {
        case 10: hipLaunchKernelGGL(k_clear_slots<10>, grid, dim3(kKtThreads), 0, st, a); break;
        case 12: hipLaunchKernelGGL(k_clear_slots<12>, grid, dim3(kKtThreads), 0, st, a); break;
        case 14: hipLaunchKernelGGL(k_clear_slots<14>, grid, dim3(kKtThreads), 0, st, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace fpnn_aes
