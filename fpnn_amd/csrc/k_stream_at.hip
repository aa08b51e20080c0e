// k_stream_at.hip -- the slot forms of the stream encrypt kernels (fpnn_aes_stream_encrypt_at):
// K2 (k_cfb_encrypt_chains), K2c (k_cfb_encrypt_coop) and K2h (k_cfb_encrypt_hybrid, quad and
// lane session) instantiated with KEY_SLOT.  Segment s is the one pending frame of the
// connection in key-table slot state_slot[s]: the kernel takes its key from b.keys[slot] and
// its (iv, pos) from entry `slot` of the state arrays fpnn_aes_stream_open wrote, and writes
// the outgoing state back there -- no gather before the call and no scatter after it, and the
// length-ordered queues of K2h for the one-frame-per-connection IO cycle (kernels.hpp,
// launch_encrypt_*_at).
//
// The kernel templates are those of k_encrypt.hip and k_hybrid.hip, included here without
// their launchers: KEY_SLOT is a compile-time variant of them, every instantiation those two
// files make compiles as before, and the slot forms live in this file's code object (linked
// behind the older ones, Makefile).
#define FPNN_AES_KERNEL_TEMPLATES_ONLY
#include "k_encrypt.hip"
#include "k_hybrid.hip"

namespace fpnn_aes {

// K2: as enc_nr's stream forms (8-block chunks, 4 with AES-256 round keys per lane; plain round)
template <int NR>
static void chains_at_nr(const KBatch &b, Layout layout, int grid, int threads, hipStream_t st) {
    if (layout == LAYOUT_UNIFORM)
        hipLaunchKernelGGL((k_cfb_encrypt_chains<NR, LAYOUT_UNIFORM, KEY_SLOT, true, 4, 8, false>), dim3(grid),
                           dim3(threads), 0, st, b);
    else
        hipLaunchKernelGGL((k_cfb_encrypt_chains<NR, LAYOUT_GENERAL, KEY_SLOT, true, 4, 8, false>), dim3(grid),
                           dim3(threads), 0, st, b);
}

hipError_t launch_encrypt_chains_at(const KBatch &b, int nrounds, Layout layout, int grid, int threads, hipStream_t st) {
    set_launched("cfb_encrypt_chains_at");
    switch (nrounds) {
        case 10: chains_at_nr<10>(b, layout, grid, threads, st); break;
        case 12: chains_at_nr<12>(b, layout, grid, threads, st); break;
        case 14: chains_at_nr<14>(b, layout, grid, threads, st); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int NR>
static void coop_at_nr(const KBatch &b, Layout layout, int grid, int threads, hipStream_t st) {
    if (layout == LAYOUT_UNIFORM)
        hipLaunchKernelGGL((k_cfb_encrypt_coop<NR, LAYOUT_UNIFORM, KEY_SLOT, true, 4>), dim3(grid), dim3(threads), 0, st, b);
    else
        hipLaunchKernelGGL((k_cfb_encrypt_coop<NR, LAYOUT_GENERAL, KEY_SLOT, true, 4>), dim3(grid), dim3(threads), 0, st, b);
}

hipError_t launch_encrypt_coop_at(const KBatch &b, int nrounds, Layout layout, int grid, int threads, hipStream_t st) {
    set_launched("cfb_encrypt_coop_at");
    switch (nrounds) {
        case 10: coop_at_nr<10>(b, layout, grid, threads, st); break;
        case 12: coop_at_nr<12>(b, layout, grid, threads, st); break;
        case 14: coop_at_nr<14>(b, layout, grid, threads, st); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// K2h: as hybrid_nr's per-lane-key stream form (half-line steps in the lane session)
hipError_t launch_encrypt_hybrid_at(const KBatch &b, const HybridArgs &h, int nrounds, int grid, hipStream_t st) {
    set_launched("cfb_encrypt_hybrid_at");
#define FPNN_HYB_AT(NR) \
    hipLaunchKernelGGL((k_cfb_encrypt_hybrid<NR, KEY_SLOT, true, 4, 4, false, true, true>), dim3(grid), dim3(kThreads), 0, st, b, h)
    switch (nrounds) {
        case 10: FPNN_HYB_AT(10); break;
        case 12: FPNN_HYB_AT(12); break;
        case 14: FPNN_HYB_AT(14); break;
        default: return hipErrorInvalidValue;
    }
#undef FPNN_HYB_AT
    return hipGetLastError();
}

}  // namespace fpnn_aes
