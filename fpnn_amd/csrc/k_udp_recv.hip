// k_udp_recv.hip -- the receive side of FPNN's UDP v2 transport with data encryption
// (fpnn_aes_udp_recv / _recv_take, kernels.hpp UdpRecvTable): where a datagram's data sections
// lie is known only from its package-plaintext, so the device walks it.
//
//   k_udp_walk   one lane per datagram restates the structural part of ARQParser
//                (core/UDP.v2/UDPParser.v2.cpp: parse :59-122, processAssembledPackage :124-159,
//                processPackage :313-346, parseCOMBINED :528-587, the header arithmetic of
//                parseDATA :672-742, parseACKS :840-870, parseUNA :872-892) over the bytes the
//                package decrypt left in `out`, and writes the scan entry, the package row and
//                the section row
//   k_udp_take   turns "every package" or the host's take lists into the descriptors of the
//                slot-addressed *_frames decrypt: each section to decrypt as a segment of `out`,
//                each connection's segment range
// No cipher runs here: the package layer before the walk and the data layer after the take are
// the queued package decrypt and *_frames_at decrypt, as fpnn_aes_udp_decrypt queues them.
#include "udp_ranges.hpp"

namespace fpnn_aes {

namespace {

// ARQType and ARQFlag (core/UDP.v2/UDPCommon.v2.h:18-42)
enum : uint32_t { T_DATA = 0x01, T_ACKS = 0x02, T_UNA = 0x03, T_ECDH = 0x04, T_HEARTBEAT = 0x05, T_FORCESYNC = 0x06,
                  T_CLOSE = 0x0F, T_COMBINED = 0x80, T_ASSEMBLED = 0x81 };
enum : uint32_t { F_DISCARDABLE = 0x01, F_SEGMENTED_MASK = 0x0c, F_CANCELLED = 0x80 };

struct Dgram {
    uint8_t *out;
    uint32_t len;
};

__device__ __forceinline__ Dgram dgram_out(const KBatch &b, uint64_t s) {
    Dgram d;
    const uint64_t io = b.in_off ? *FA_AT(b, AB_IN_OFF, b.in_off + s, 8) : s * b.stride;
    const uint64_t oo = b.out_off ? *FA_AT(b, AB_OUT_OFF, b.out_off + s, 8) : io;
    d.out = b.out + oo;
    d.len = b.len ? *FA_AT(b, AB_LEN, b.len + s, 4) : b.uniform_len;
    return d;
}

__device__ __forceinline__ void report(uint32_t *fault, uint32_t what) {
    if (fault) __hip_atomic_fetch_or(fault, what, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// One datagram's walk: its bytes (read one at a time: the headers lie at any alignment, and no
// read may cross the datagram's end), its two rows and what is used of them.
struct Walk {
    const KBatch &b;
    const uint8_t *p;  // the datagram in `out`
    uint32_t len;
    UdpPkg *pkgs;
    UdpSection *secs;
    uint32_t max_pkgs, max_secs, npkgs, nsecs;

    // byte i of the datagram; the callers' length checks keep i < len, and an i that is not
    // reads nothing
    __device__ __forceinline__ uint32_t u8(uint32_t i) const {
        if (i >= len) return 0u;
        return *FA_SEG(b, AB_OUT, p + i, 1, (uint64_t)(uintptr_t)p, (uint64_t)(uintptr_t)p + len);
    }
    __device__ __forceinline__ uint32_t be16(uint32_t i) const { return (u8(i) << 8) | u8(i + 1); }
    __device__ __forceinline__ uint32_t be32(uint32_t i) const { return (be16(i) << 16) | be16(i + 2); }

    // false: the section row is full
    __device__ __forceinline__ bool section(uint32_t type, uint32_t flag, uint32_t pkg, uint32_t off, uint32_t n,
                                            uint32_t package_id = 0, uint32_t seg_index = 0) {
        if (nsecs >= max_secs) return false;
        UdpSection s;
        s.type = (uint8_t)type;
        s.flag = (uint8_t)flag;
        s.pkg = (uint16_t)pkg;
        s.off = (uint16_t)off;
        s.len = (uint16_t)n;
        s.package_id = (uint16_t)package_id;
        s.reserved = 0;
        s.seg_index = seg_index;
        *FA_AT(b, AB_UDP_SECTIONS, secs + nsecs, sizeof s) = s;
        nsecs++;
        return true;
    }

    // parseDATA's header arithmetic (:672-742): `bytes` bytes at `at`
    __device__ __forceinline__ uint32_t data(uint32_t flag, uint32_t pkg, uint32_t at, uint32_t bytes) {
        const uint32_t seg = flag & F_SEGMENTED_MASK;
        if (seg == 0u) return section(T_DATA, flag, pkg, at, bytes) ? UDP_OK : UDP_FULL;
        const uint32_t hdr = 2u + (seg == 0x04u ? 1u : seg == 0x08u ? 2u : 4u);  // packageId + index (:709-742)
        if (bytes < hdr) return UDP_SHORT;  // (`bytes -= ...` would wrap)
        const uint32_t id = be16(at);
        const uint32_t index = seg == 0x04u ? u8(at + 2) : seg == 0x08u ? be16(at + 2) : be32(at + 2);
        return section(T_DATA, flag, pkg, at + hdr, bytes - hdr, id, index) ? UDP_OK : UDP_FULL;
    }

    // processPackage (:313-346) of the package at [off, off + n) of the datagram, n >= 8: its
    // status
    __device__ __forceinline__ uint32_t package(uint32_t pkg, uint32_t type, uint32_t flag, uint32_t off, uint32_t n) {
        switch (type) {
        case T_COMBINED: {  // parseCOMBINED (:528-587)
            if (n < 16u) return UDP_SHORT;
            uint32_t o = 8u;
            while (o < n) {
                if (o + 4u > n) return UDP_SHORT;  // (the component header itself crosses the end)
                const uint32_t t = u8(off + o), f = u8(off + o + 1), bytes = be16(off + o + 2);
                if (o + 4u + bytes > n) return UDP_SHORT;  // (:544)
                uint32_t st = UDP_OK;
                if (t == T_DATA) st = data(f, pkg, off + o + 4u, bytes);
                else if (t == T_ACKS) st = (bytes & 3u) ? UDP_ACKS : section(t, f, pkg, off + o + 4u, bytes) ? UDP_OK : UDP_FULL;
                else if (t == T_UNA) st = o + 8u > n ? UDP_SHORT : section(t, f, pkg, off + o + 4u, bytes) ? UDP_OK : UDP_FULL;  // (:888 reads 4 bytes)
                else if (t == T_FORCESYNC) st = section(t, f, pkg, off + o + 4u, bytes) ? UDP_OK : UDP_FULL;
                else if (t == T_CLOSE) return section(t, f, pkg, off + o + 4u, bytes) ? UDP_CLOSE : UDP_FULL;  // (:567-571)
                else return UDP_TYPE;  // (ECDH: :928-933)
                if (st != UDP_OK) return st;
                o += 4u + bytes;
            }
            return UDP_OK;
        }
        case T_DATA: return data(flag, pkg, off + 8u, n - 8u);
        case T_ACKS:  // parseACKS (:845-861)
            if ((n - 8u) & 3u) return UDP_ACKS;
            return section(type, flag, pkg, off + 8u, n - 8u) ? UDP_OK : UDP_FULL;
        case T_UNA:  // parseUNA (:874-880)
            if (n != 12u) return UDP_SHORT;
            return section(type, flag, pkg, off + 8u, 4u) ? UDP_OK : UDP_FULL;
        case T_FORCESYNC:
        case T_HEARTBEAT: return section(type, flag, pkg, off + 8u, n - 8u) ? UDP_OK : UDP_FULL;
        case T_CLOSE: return section(type, flag, pkg, off + 8u, n - 8u) ? UDP_CLOSE : UDP_FULL;  // (:336-340)
        default: return UDP_TYPE;
        }
    }

    // a package row for [off, off + n), its header at off + 1 .. off + 8, then its walk; the
    // status the datagram takes from it (OK also for CLOSE)
    __device__ __forceinline__ uint32_t package_row(uint32_t off, uint32_t n) {
        if (npkgs >= max_pkgs) return UDP_FULL;
        const uint32_t k = npkgs++, first = nsecs;
        const uint32_t type = u8(off + 1), flag = u8(off + 2);
        UdpPkg r;
        r.seq = be32(off + 4);
        r.type = (uint8_t)type;
        r.flag = (uint8_t)flag;
        r.sign = (uint8_t)u8(off + 3);
        r.off = (uint16_t)off;
        r.len = (uint16_t)n;
        r.first_section = (uint16_t)first;
        const uint32_t st = package(k, type, flag, off, n);
        r.status = (uint8_t)st;
        r.nsections = (uint16_t)(nsecs - first);
        *FA_AT(b, AB_UDP_PKGS, pkgs + k, sizeof r) = r;
        return st == UDP_CLOSE ? (uint32_t)UDP_OK : st;
    }
};

}  // namespace

__global__ __launch_bounds__(256) void k_udp_walk(KBatch b, UdpRecvTable r) {
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t maxp = min(r.max_pkgs, 0xFFFFu), maxs = min(r.max_sections, 0xFFFFu);  // (the counts are 16 bits)
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < b.count; i += nthreads) {
        const Dgram d = dgram_out(b, i);
        Walk w{b, d.out, d.len, r.pkgs + i * r.max_pkgs, r.sections + i * r.max_sections, maxp, maxs, 0u, 0u};
        uint32_t status = UDP_OK, version = 0u;
        if (d.len < 8u) status = UDP_SHORT;  // (:67)
        else if (d.len > 0xFFFFu) status = UDP_LONG;
        else if (w.u8(0) > 2u) status = UDP_VERSION;  // (:96-105)
        else {
            version = w.u8(0);
            if (w.u8(1) != T_ASSEMBLED) {
                status = w.package_row(0u, d.len);
            } else {  // processAssembledPackage (:124-159)
                uint32_t at = 2u;  // the included package's length field
                while (at < d.len && status == UDP_OK) {
                    if (at + 2u > d.len) {  // (a 1-byte remainder: the length field crosses the end)
                        status = UDP_SHORT;
                        break;
                    }
                    const uint32_t plen = w.be16(at);
                    // its header is 7 bytes (the version byte is the length field's second, :133);
                    // its bytes end at at + 2 + plen
                    if (plen < 7u || at + 2u + plen > d.len) {
                        status = UDP_SHORT;
                        break;
                    }
                    status = w.package_row(at + 1u, plen + 1u);
                    at += 2u + plen;
                }
            }
        }
        UdpScan s;
        s.pkgs = (uint16_t)w.npkgs;
        s.sections = (uint16_t)w.nsecs;
        s.version = (uint8_t)version;
        s.status = (uint8_t)status;
        s.reserved = 0;
        *FA_AT(b, AB_UDP_SCAN, r.scan + i, sizeof s) = s;
    }
}

// ---------------------------------------------------------------------------
// The data layer's descriptors.  Item t is datagram t (every package, in array order) or the
// t-th taken package; it owns segments [t * max_sections, (t + 1) * max_sections): segment r is
// the item's r-th section when that is to be decrypted (DATA, neither discardable nor cancelled:
// :695-703, :714, :769-775, :823-829), else it has length 0, which the *_frames decrypt skips.
// Connection j's segments are its items': [first[j], first[j + 1]) * max_sections, first being
// first_dgram or first_take.  Everything read from the caller's tables is clamped before it
// addresses memory: scan's counts to the rows, a package's section range to its datagram's
// used sections, a section's bytes to its datagram; a take entry must name a walked package of
// one of its own connection's datagrams.  A breach gives length 0 and a report.
__global__ __launch_bounds__(256) void k_udp_take(KBatch b, UdpTable u, UdpRecvTable r, uint64_t *__restrict__ sec_abs,
                                                  uint32_t *__restrict__ sec_n, uint32_t *__restrict__ conn_sec) {
    const uint32_t cnt = (uint32_t)b.count;
    const bool all = r.take == nullptr;
    const uint32_t items = all ? cnt : r.ntake;
    const uint64_t nseg = (uint64_t)items * r.max_sections;
    const uint64_t top = max(nseg, (uint64_t)u.nconn + 1u);
    const uint64_t nthreads = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < top; x += nthreads) {
        if (x < nseg) {
            const uint32_t t = (uint32_t)(x / r.max_sections), rr = (uint32_t)(x % r.max_sections);
            uint32_t dg = t, s0 = 0u, s1 = 0u;  // the item's sections [s0, s1) of datagram dg's row
            bool ok = true;
            if (all) {
                const UdpScan sc = *FA_AT(b, AB_UDP_SCAN, r.scan + dg, sizeof(UdpScan));
                s1 = min((uint32_t)sc.sections, r.max_sections);
            } else {
                const uint32_t j = owner_of(b, AB_UDP_FIRST_TAKE, r.first_take, u.nconn, t);
                uint32_t t0, t1, d0, d1;
                table_range(b, AB_UDP_FIRST_TAKE, r.first_take, j, u.nconn, r.ntake, u.fault, t0, t1);
                table_range(b, AB_FIRST_FRAME, u.first_dgram, j, u.nconn, cnt, u.fault, d0, d1);
                const uint32_t g = *FA_AT(b, AB_UDP_TAKE, r.take + t, 4);
                dg = g / r.max_pkgs;
                const uint32_t k = g % r.max_pkgs;
                ok = t >= t0 && t < t1 && dg >= d0 && dg < d1;  // (dg < d1 <= cnt)
                if (ok) {
                    const UdpScan sc = *FA_AT(b, AB_UDP_SCAN, r.scan + dg, sizeof(UdpScan));
                    ok = k < min((uint32_t)sc.pkgs, r.max_pkgs);
                    if (ok) {
                        const UdpPkg p = *FA_AT(b, AB_UDP_PKGS, r.pkgs + (uint64_t)dg * r.max_pkgs + k, sizeof(UdpPkg));
                        const uint32_t used = min((uint32_t)sc.sections, r.max_sections);
                        s0 = p.first_section;
                        s1 = s0 + p.nsections;
                        if (s1 > used) {
                            ok = false;
                            s0 = s1 = 0u;
                        }
                    }
                }
                if (!ok && rr == 0u) report(u.fault, kFaultFrameTable);
            }
            uint64_t abs = 0;
            uint32_t n = 0;
            if (ok && rr < s1 - s0) {
                const UdpSection s =
                    *FA_AT(b, AB_UDP_SECTIONS, r.sections + (uint64_t)dg * r.max_sections + s0 + rr, sizeof(UdpSection));
                if (s.type == T_DATA && !(s.flag & (F_DISCARDABLE | F_CANCELLED))) {
                    const Dgram d = dgram_out(b, dg);
                    const uint32_t lo = min((uint32_t)s.off, d.len), hi = min((uint32_t)s.off + s.len, d.len);
                    if ((uint32_t)s.off + s.len > d.len) report(u.fault, kFaultFrameTable);
                    abs = (uint64_t)(d.out - b.out) + lo;
                    n = hi - lo;
                }
            }
            sec_abs[x] = abs;
            sec_n[x] = n;
        }
        if (x <= u.nconn) {
            const uint32_t first = all ? min(*FA_AT(b, AB_FIRST_FRAME, u.first_dgram + x, 4), cnt)
                                       : min(*FA_AT(b, AB_UDP_FIRST_TAKE, r.first_take + x, 4), r.ntake);
            conn_sec[x] = first * r.max_sections;
        }
    }
}

// ---------------------------------------------------------------------------
// Launchers

hipError_t launch_udp_walk(const KBatch &b, const UdpRecvTable &r, int num_cus, hipStream_t st) {
    // (a datagram's walk is a few dozen byte loads: 4 workgroups per CU hide them, more datagrams
    // than that take further trips of the loop)
    set_launched("udp_walk");
    hipLaunchKernelGGL(k_udp_walk, dim3(grid_for(b.count, 256, 4 * num_cus)), dim3(256), 0, st, b, r);
    return hipGetLastError();
}

hipError_t launch_udp_take(const KBatch &b, const UdpTable &u, const UdpRecvTable &r, uint64_t *sec_abs,
                           uint32_t *sec_n, uint32_t *conn_sec, int num_cus, hipStream_t st) {
    const uint64_t items = r.take ? r.ntake : b.count;
    const uint64_t top = std::max<uint64_t>(items * r.max_sections, (uint64_t)u.nconn + 1);
    set_launched("udp_take");
    hipLaunchKernelGGL(k_udp_take, dim3(grid_for(top, 256, 8 * num_cus)), dim3(256), 0, st, b, u, r, sec_abs, sec_n,
                       conn_sec);
    return hipGetLastError();
}

}  // namespace fpnn_aes
