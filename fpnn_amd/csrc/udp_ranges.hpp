// udp_ranges.hpp -- the range tables of the UDP kernels (k_udp.hip, k_udp_recv.hip): first_dgram
// over the datagrams, first_section over the sections, first_take over the take list.  One
// contract, first_frame's (k_stream_frames.hip, stream_range), for clamping and reporting.
#pragma once

#include "segments.hpp"

namespace fpnn_aes {

// Entries [r0, r1) of a range table: item j of `items` owns [tab[j], tab[j + 1]) of `total`.
// Non-decreasing from 0 to total; what is read is clamped into [0, total], a table that breaks
// the contract is reported.
__device__ __forceinline__ void table_range(const KBatch &b, AuditBuf buf, const uint32_t *tab, uint32_t j,
                                            uint32_t items, uint32_t total, uint32_t *fault, uint32_t &r0,
                                            uint32_t &r1) {
    if (!tab) {  // (first_section of a call without sections)
        r0 = r1 = 0u;
        return;
    }
    const uint32_t t0 = *FA_AT(b, buf, tab + j, 4);
    const uint32_t t1 = *FA_AT(b, buf, tab + j + 1, 4);
    const bool bad = t1 < t0 || t1 > total || (j == 0 && t0 != 0u) || (j + 1 == items && t1 != total);
    r0 = min(t0, total);
    r1 = max(min(t1, total), r0);
    if (bad && fault) __hip_atomic_store(fault, kFaultFrameTable, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the last j in [0, items) with tab[j] <= x (0 when there is none): the owner of entry x by
// bisection (the caller checks x against the owner's clamped range)
__device__ __forceinline__ uint32_t owner_of(const KBatch &b, AuditBuf buf, const uint32_t *tab, uint32_t items,
                                             uint32_t x) {
    uint32_t lo = 0, hi = items;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (*FA_AT(b, buf, tab + mid, 4) <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace fpnn_aes
