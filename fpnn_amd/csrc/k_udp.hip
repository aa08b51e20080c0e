// k_udp.hip -- FPNN's UDP v2 transport with "enhanced" data encryption (fpnn_aes_udp_encrypt /
// _decrypt, kernels.hpp UdpTable): a UDPEncryptor holds two ciphers
// (core/UDP.v2/UDPCommon.v2.cpp:146-215) -- a StreamEncryptor under the data key, whose one CFB
// chain runs through the data sections of the connection's datagrams in send order, and a
// PackageEncryptor under the package key, which then ciphers every whole datagram with a fresh
// chain from the connection IV.
//
//   K2u   encrypt: one lane quad per CONNECTION (K2c's cipher, coop.hpp) walks the connection's
//         datagrams as K2f walks a stream's frames, both column schedules and the data layer's
//         (iv, pos) in registers from the connection's first section to its last
//   decrypt: k_udp_expand writes the descriptors the existing kernels take -- every datagram's
//         key slot, every section as a segment of `out`, every connection's section range --
//         and the engine queues the package decrypt and the *_frames_at decrypt behind it
#include "coop.hpp"
#include "udp_ranges.hpp"

namespace fpnn_aes {

namespace {

// Section s of a datagram of `len` bytes whose earlier sections end at prev_end: its bytes
// [lo, hi) inside the datagram.  Sections ascend, do not overlap and lie inside the datagram;
// one that does not is clamped to [prev_end, len) and reported.
__device__ __forceinline__ void section_range(const KBatch &b, const UdpTable &u, uint32_t s, uint32_t len,
                                              uint32_t prev_end, uint32_t &lo, uint32_t &hi) {
    const uint32_t off = *FA_AT(b, AB_UDP_SEC_OFF, u.sec_off + s, 4);
    const uint64_t end = (uint64_t)off + *FA_AT(b, AB_UDP_SEC_LEN, u.sec_len + s, 4);
    const bool bad = off < prev_end || end > len;
    lo = min(max(off, prev_end), len);
    hi = (uint32_t)min(max(end, (uint64_t)lo), (uint64_t)len);
    if (bad && u.fault) __hip_atomic_store(u.fault, kFaultFrameTable, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct DgramDesc {
    const uint8_t *in;
    uint8_t *out;
    uint32_t len;
};

__device__ __forceinline__ DgramDesc dgram_desc(const KBatch &b, uint64_t s) {
    DgramDesc d;
    const uint64_t io = b.in_off ? *FA_AT(b, AB_IN_OFF, b.in_off + s, 8) : s * b.stride;
    const uint64_t oo = b.out_off ? *FA_AT(b, AB_OUT_OFF, b.out_off + s, 8) : io;
    d.in = b.in + io;
    d.out = b.out + oo;
    d.len = b.len ? *FA_AT(b, AB_LEN, b.len + s, 4) : b.uniform_len;
    return d;
}

// One CFB run of the quad: `len` bytes p -> o under the column schedule rkq, continuing the
// chain state (iv: this lane's word of the feedback register; n: the position).  K2f's frame
// (k_stream_frames.hip) without its cross-frame prefetch: the head bytes that finish the
// carried keystream block, 8-block steps with the next step's words already loading, single
// blocks, the partial tail.  RB: the audit buffer p is read as (AB_IN, or AB_OUT for the
// package layer, which reads what the data layer and the gap copy left in `out`); [rlo, rhi)
// and [olo, ohi) are the datagram's own bytes on either side (the audit build checks them).
template <int NR, int NT, AuditBuf RB>
__device__ __forceinline__ void quad_cfb_run(const KBatch &b, const uint8_t *p, uint8_t *o, uint32_t len,
                                             const uint32_t *rkq, const Tables4<NT> &T, int wlo, const uint8_t *dummy,
                                             uint32_t &iv, uint32_t &n, uint64_t rlo, uint64_t rhi, uint64_t olo,
                                             uint64_t ohi) {
    constexpr int CH = 8;
    (void)rlo, (void)rhi, (void)olo, (void)ohi;
    uint32_t rem = len;
    if (n != 0 && rem != 0) {  // rest of the partially used keystream block
        const uint32_t take = min(rem, 16u - n);
        const int lo = max((int)n, wlo) - wlo, hi = min((int)(n + take), wlo + 4) - wlo;
        if (lo < hi) {
            const uint32_t c = load_word_bytes(FA_RG(b, RB, p - n + wlo, lo, hi, rlo, rhi), lo, hi) ^ iv;
            store_word_bytes(FA_RG(b, AB_OUT, o - n + wlo, lo, hi, olo, ohi), c, lo, hi);
            const uint32_t m = word_mask(lo, hi);
            iv = (c & m) | (iv & ~m);
        }
        p += take;
        o += take;
        rem -= take;
        n = (n + take) & 15u;
    }
    const uint32_t nfull = rem >> 4, tail = rem & 15u;
    uint32_t i = 0;
    if (nfull >= (uint32_t)CH) {
        const uint32_t rkx = rkq[NR] ^ rkq[0];
        uint32_t a[CH];
#pragma unroll
        for (int j = 0; j < CH; j++)
            a[j] = *reinterpret_cast<const uint32_u *>(FA_SEG(b, RB, p + wlo + 16 * j, 4, rlo, rhi));
        for (; i + CH <= nfull; i += CH) {
            // the next step's words (unconditional loads, as K2c's step loop: past the run's last
            // step they re-read the first DevKey, an L2 hit)
            const bool more = i + 2 * CH <= nfull;
            const uint8_t *pn = more ? p + 16 * CH + wlo : dummy;
            uint32_t nx[CH], c[CH];
#pragma unroll
            for (int j = 0; j < CH; j++)
                nx[j] = *reinterpret_cast<const uint32_u *>(more ? FA_SEG(b, RB, pn + 16 * j, 4, rlo, rhi)
                                                                 : FA_AT(b, AB_KEYS, pn + 16 * j, 4));
            uint32_t sw = iv ^ rkq[0];  // the chain carries C ^ rk[0] (aes_chain_column)
#pragma unroll
            for (int j = 0; j < CH; j++) {
                sw = aes_chain_column<NR, NT>(sw, rkq, rkx ^ a[j], T);
                c[j] = sw ^ rkq[0];
            }
            iv = c[CH - 1];
#pragma unroll
            for (int j = 0; j < CH; j++) asm volatile("" : "+v"(c[j]));
#pragma unroll
            for (int j = 0; j < CH; j++)
                *reinterpret_cast<uint32_u *>(FA_SEG(b, AB_OUT, o + 16 * j + wlo, 4, olo, ohi)) = c[j];
#pragma unroll
            for (int j = 0; j < CH; j++) {
                asm volatile("" : "+v"(nx[j]));
                a[j] = nx[j];
            }
            p += 16 * CH;
            o += 16 * CH;
        }
    }
    if (i < nfull) {  // up to 7 single blocks, each one's word loading behind its predecessor's rounds
        uint32_t pt = *reinterpret_cast<const uint32_u *>(FA_SEG(b, RB, p + wlo, 4, rlo, rhi));
        for (; i < nfull; i++) {
            const bool more = i + 1 < nfull;
            const uint32_t ptn = *reinterpret_cast<const uint32_u *>(more ? FA_SEG(b, RB, p + 16 + wlo, 4, rlo, rhi)
                                                                          : FA_AT(b, AB_KEYS, dummy, 4));
            iv = aes_encrypt_column<NR, NT>(iv, rkq, T) ^ pt;
            *reinterpret_cast<uint32_u *>(FA_SEG(b, AB_OUT, o + wlo, 4, olo, ohi)) = iv;
            pt = ptn;
            p += 16;
            o += 16;
        }
    }
    if (tail) {  // partial final block: the run ends inside a keystream block
        const uint32_t ks = aes_encrypt_column<NR, NT>(iv, rkq, T);
        const int lo = 0, hi = min((int)tail, wlo + 4) - wlo;
        if (hi > lo) {
            const uint32_t c = load_word_bytes(FA_RG(b, RB, p + wlo, lo, hi, rlo, rhi), lo, hi) ^ ks;
            store_word_bytes(FA_RG(b, AB_OUT, o + wlo, lo, hi, olo, ohi), c, lo, hi);
            const uint32_t m = word_mask(lo, hi);
            iv = (c & m) | (ks & ~m);
        } else {
            iv = ks;
        }
        n = tail;
    }
}

// bytes [lo, hi) of a datagram that no section covers, in -> out (out of place only): the quad's
// lanes take the 4-byte words in turn, lane 0 the last 1 - 3 bytes
__device__ __forceinline__ void quad_copy(const KBatch &b, const DgramDesc &d, uint32_t lo, uint32_t hi, int q,
                                          uint64_t ilo, uint64_t ihi, uint64_t olo, uint64_t ohi) {
    (void)ilo, (void)ihi, (void)olo, (void)ohi;
    const uint32_t words = (hi - lo) >> 2;
    for (uint32_t w = (uint32_t)q; w < words; w += 4u)
        *reinterpret_cast<uint32_u *>(FA_SEG(b, AB_OUT, d.out + lo + 4u * w, 4, olo, ohi)) =
            *reinterpret_cast<const uint32_u *>(FA_SEG(b, AB_IN, d.in + lo + 4u * w, 4, ilo, ihi));
    if (q == 0)
        for (uint32_t i = lo + 4u * words; i < hi; i++)
            *FA_SEG(b, AB_OUT, d.out + i, 1, olo, ohi) = *FA_SEG(b, AB_IN, d.in + i, 1, ilo, ihi);
}

}  // namespace

// ---------------------------------------------------------------------------
// K2u.  Per datagram, in one launch: the data layer ciphers the sections in -> out (the bytes
// between them are copied when the call is out of place), then the package layer ciphers the
// whole datagram in place in `out`.  The package layer's lane owns other bytes than the data
// layer's lane wrote (the two layers' block grids differ by the section's offset and the
// stream's position), so a wavefront-scope release / acquire stands between the two: a quad's
// lanes share one wave, whose accesses to one address stay in program order, and the fence
// keeps the compiler from moving the loads up.
//
// NRD / NRP: the rounds of the data key and of the package key -- (10, 14) x (10, 14): the
// tables may have different key lengths, and createPair makes no 24-byte key.  NT = 4, one
// workgroup per CU at 4 waves per SIMD as K2f: the kernel keeps no LDS window (the
// intermediate bytes pass through `out`, which the L2 holds), so the full 4-table image fits.
template <int NRD, int NRP, int NT>
__global__ __launch_bounds__(kThreads, 4) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_udp_encrypt(KBatch b,
                                                                                                        UdpTable u) {
    __shared__ uint4 lds4[Lds<NT>::kBytes / 16];
    lds_fill_tables<NT>(lds4, b.t0le);
    __syncthreads();
    const Tables4<NT> T{reinterpret_cast<const char *>(lds4), LaneBase()};
    const int q = (int)(threadIdx.x & 3u);
    const int wlo = 4 * q;  // block bytes [wlo, wlo + 4) belong to this lane
    const uint8_t *const dummy = reinterpret_cast<const uint8_t *>(b.keys) + wlo;  // 16 * 8 readable bytes
    const uint32_t cnt = (uint32_t)b.count;
    const bool copy = b.in != b.out;

    const uint64_t nquads = ((uint64_t)gridDim.x * blockDim.x) >> 2;
    for (uint64_t t = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2; t < u.nconn; t += nquads) {
        const uint32_t ss = *FA_AT(b, AB_STATE_SLOT, u.conn_slot + t, 4);
        if (ss >= u.slot_bound) {  // a slot past the bound: no state is touched, nothing is written
            if (u.fault) __hip_atomic_fetch_or(u.fault, kFaultKeySlot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            continue;
        }
        uint32_t d0, d1;
        table_range(b, AB_FIRST_FRAME, u.first_dgram, (uint32_t)t, u.nconn, cnt, u.fault, d0, d1);
        if (d0 >= d1) continue;  // no datagram: the state stays as it is
        const DevKey *kp = FA_AT(b, AB_KEYS, b.keys + ss, sizeof(DevKey));
        uint32_t rkp[NRP + 1], rkd[NRD + 1];
#pragma unroll
        for (int r = 0; r <= NRP; r++) rkp[r] = kp->rk[4 * r + q];
        const uint32_t piv0 = reinterpret_cast<const uint32_t *>(kp->iv)[q];
        if (u.data_keys) {  // (null: the call has no section, the data schedule is never used)
            const DevKey *kd = FA_AT(b, AB_UDP_DATA_KEYS, u.data_keys + ss, sizeof(DevKey));
#pragma unroll
            for (int r = 0; r <= NRD; r++) rkd[r] = kd->rk[4 * r + q];
        } else {
#pragma unroll
            for (int r = 0; r <= NRD; r++) rkd[r] = 0u;
        }
        // the data layer's state: this lane's word of the feedback register, and the position
        uint32_t iv = reinterpret_cast<const uint32_t *>(FA_AT(b, AB_IV_STATE, b.iv_state + 16ull * ss, 16))[q];
        uint32_t n = *FA_AT(b, AB_POS_STATE, b.pos_state + ss, 4) & 15u;
        bool any = false;  // a data byte was ciphered (otherwise the state keeps every bit)

        // the next datagram's descriptor and section range load while this one is ciphered
        DgramDesc nxt = dgram_desc(b, d0);
        uint32_t ns0, ns1;
        table_range(b, AB_UDP_FIRST_SECTION, u.first_section, d0, cnt, u.nsections, u.fault, ns0, ns1);
        for (uint32_t k = d0; k < d1; k++) {
            const DgramDesc d = nxt;
            const uint32_t s0 = ns0, s1 = ns1;
            const uint32_t kn = min(k + 1u, d1 - 1u);
            nxt = dgram_desc(b, kn);
            table_range(b, AB_UDP_FIRST_SECTION, u.first_section, kn, cnt, u.nsections, u.fault, ns0, ns1);
            const uint64_t ilo = (uintptr_t)d.in, ihi = ilo + d.len, olo = (uintptr_t)d.out, ohi = olo + d.len;
            uint32_t prev_end = 0;
            for (uint32_t s = s0; s < s1; s++) {
                uint32_t lo, hi;
                section_range(b, u, s, d.len, prev_end, lo, hi);
                if (copy) quad_copy(b, d, prev_end, lo, q, ilo, ihi, olo, ohi);
                any |= hi > lo;
                quad_cfb_run<NRD, NT, AB_IN>(b, d.in + lo, d.out + lo, hi - lo, rkd, T, wlo, dummy, iv, n, ilo, ihi, olo,
                                             ohi);
                prev_end = hi;
            }
            if (copy) quad_copy(b, d, prev_end, d.len, q, ilo, ihi, olo, ohi);
            // the data layer's and the copy's stores, by the other lanes of the quad, before the
            // package layer's loads of the same bytes
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            uint32_t piv = piv0, pn = 0;  // PackageEncryptor: a fresh chain from the connection IV
            quad_cfb_run<NRP, NT, AB_OUT>(b, d.out, d.out, d.len, rkp, T, wlo, dummy, piv, pn, olo, ohi, olo, ohi);
        }
        if (any) {
            reinterpret_cast<uint32_t *>(FA_AT(b, AB_IV_STATE, b.iv_state + 16ull * ss, 16))[q] = iv;
            if (q == 0) *FA_AT(b, AB_POS_STATE, b.pos_state + ss, 4) = n;
        }
    }
}

// ---------------------------------------------------------------------------
// Decrypt's descriptors, one launch, one lane per datagram, per section and per connection
// (every entry is written whatever the tables hold, so the kernels that follow read nothing
// stale and nothing outside the batch):
//   dg_slot[i]   datagram i's key slot, its connection's conn_slot (found by bisection in
//                first_dgram); 0 and a report when that lies at or past slot_bound, or when no
//                connection owns the datagram
//   sec_abs[s]   section s as a segment of `out`: its datagram's offset + sec_off[s], and
//   sec_n[s]     its length, both clamped into the datagram (length 0 when no datagram owns it)
//   conn_sec[j]  connection j's sections start at first_section[first_dgram[j]]; nconn + 1 entries
__global__ __launch_bounds__(256) void k_udp_expand(KBatch b, UdpTable u, uint32_t *__restrict__ dg_slot,
                                                    uint64_t *__restrict__ sec_abs, uint32_t *__restrict__ sec_n,
                                                    uint32_t *__restrict__ conn_sec) {
    const uint32_t cnt = (uint32_t)b.count;
    const uint32_t top = max(max(cnt, u.nsections), u.nconn + 1u);
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < top; x += nthreads) {
        const uint32_t i = (uint32_t)x;
        if (i < cnt) {
            const uint32_t j = owner_of(b, AB_FIRST_FRAME, u.first_dgram, u.nconn, i);
            uint32_t d0, d1;
            table_range(b, AB_FIRST_FRAME, u.first_dgram, j, u.nconn, cnt, u.fault, d0, d1);
            uint32_t slot = 0u;
            if (i >= d0 && i < d1) {
                slot = *FA_AT(b, AB_STATE_SLOT, u.conn_slot + j, 4);
                if (slot >= u.slot_bound) {
                    slot = 0u;
                    if (u.fault)
                        __hip_atomic_fetch_or(u.fault, kFaultKeySlot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            } else if (u.fault) {
                __hip_atomic_store(u.fault, kFaultFrameTable, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            dg_slot[i] = slot;
        }
        if (i < u.nsections) {
            const uint32_t k = owner_of(b, AB_UDP_FIRST_SECTION, u.first_section, cnt, i);
            uint32_t s0, s1;
            table_range(b, AB_UDP_FIRST_SECTION, u.first_section, k, cnt, u.nsections, u.fault, s0, s1);
            uint64_t abs = 0;
            uint32_t len = 0;
            if (i >= s0 && i < s1) {
                const DgramDesc d = dgram_desc(b, k);
                uint32_t prev_end = 0, lo, hi;
                if (i > s0) {  // (ascending: the section before this one ends at or before its start)
                    const uint64_t pe = (uint64_t)*FA_AT(b, AB_UDP_SEC_OFF, u.sec_off + i - 1, 4) +
                                        *FA_AT(b, AB_UDP_SEC_LEN, u.sec_len + i - 1, 4);
                    prev_end = (uint32_t)min(pe, (uint64_t)d.len);
                }
                section_range(b, u, i, d.len, prev_end, lo, hi);
                abs = (uint64_t)(d.out - b.out) + lo;
                len = hi - lo;
            } else if (u.fault) {
                __hip_atomic_store(u.fault, kFaultFrameTable, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            sec_abs[i] = abs;
            sec_n[i] = len;
        }
        if (i <= u.nconn) {
            const uint32_t dg = min(*FA_AT(b, AB_FIRST_FRAME, u.first_dgram + i, 4), cnt);
            conn_sec[i] = u.first_section ? min(*FA_AT(b, AB_UDP_FIRST_SECTION, u.first_section + dg, 4), u.nsections)
                                          : 0u;
        }
    }
}

// ---------------------------------------------------------------------------
// Launchers

template <int NRD>
static hipError_t k2u_nrp(const KBatch &b, const UdpTable &u, int nr_pkg, int grid, int threads, hipStream_t st) {
    switch (nr_pkg) {
        case 10: hipLaunchKernelGGL((k_udp_encrypt<NRD, 10, 4>), dim3(grid), dim3(threads), 0, st, b, u); break;
        case 14: hipLaunchKernelGGL((k_udp_encrypt<NRD, 14, 4>), dim3(grid), dim3(threads), 0, st, b, u); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_udp_encrypt(const KBatch &b, const UdpTable &u, int nr_data, int nr_pkg, int grid, int threads,
                              hipStream_t st) {
    set_launched("udp_encrypt");
    switch (nr_data) {
        case 10: return k2u_nrp<10>(b, u, nr_pkg, grid, threads, st);
        case 14: return k2u_nrp<14>(b, u, nr_pkg, grid, threads, st);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_udp_expand(const KBatch &b, const UdpTable &u, uint32_t *dg_slot, uint64_t *sec_abs, uint32_t *sec_n,
                             uint32_t *conn_sec, int num_cus, hipStream_t st) {
    const uint64_t top = std::max<uint64_t>(std::max<uint64_t>(b.count, u.nsections), (uint64_t)u.nconn + 1);
    hipLaunchKernelGGL(k_udp_expand, dim3(grid_for(top, 256, 8 * num_cus)), dim3(256), 0, st, b, u, dg_slot, sec_abs,
                       sec_n, conn_sec);
    return hipGetLastError();
}

}  // namespace fpnn_aes
