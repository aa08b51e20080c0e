// The UDP receive calls' host-only decisions (fpnn_amd/csrc/dispatch_plan.hpp: udp_recv_check_args,
// udp_recv_route; scratch_plan.hpp: need_udp_decrypt over the segments) on the CPU: every argument error of
// fpnn_aes_udp_recv / _recv_take in include/fpnn_aes.h, which steps each flag combination runs and
// the scratch they need, against literals; and that fpnn_aes_engine_reserve with the header's
// bound covers both calls.  Built and run by tests/test_udp_recv_plan.py (also with the host
// sanitizers); prints one summary line, exits non-zero at the first miss.
#include "../../fpnn_amd/csrc/dispatch_plan.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

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

static uint64_t words(uint64_t n) { return 3 + (n + 2047) / 2048; }
static uint32_t bucket(uint64_t nblocks) { return (uint32_t)(nblocks / 16); }
static DispatchShape shape(uint64_t num_cus) {
    return {ScratchShape{num_cus, 16, 16384, words, 260}, 1024, 175, 1024, 12, 0, bucket};
}

// ---- arguments ----
static UdpRecvArgs good(bool take) {  // two connections, five datagrams, 8-slot tables of 16- and 32-byte keys
    UdpRecvArgs a = {};
    a.udp.u = a.udp.data_keys = a.udp.data_keys_same_engine = true;
    a.udp.nconn = 2;
    a.udp.slot_bound = 8;
    a.udp.first_dgram = 0x1000;
    a.udp.conn_slot = 0x2000;
    a.udp.iv_state = 0x3000;
    a.udp.pos_state = 0x4000;
    a.udp.pkg_slots = a.udp.data_slots = 8;
    a.udp.nr_pkg = 10;
    a.udp.nr_data = 14;
    a.take = take;
    a.in_place = true;
    a.count = 5;
    a.max_pkgs = 4;
    a.max_sections = 8;
    a.scan = 0x5002;  // (2-byte aligned is enough)
    a.pkgs = 0x6004;
    a.sections = 0x7004;
    if (take) {
        a.ntake = 3;
        a.first_take = 0x8000;
        a.take_list = 0x9000;
    }
    return a;
}

template <class F>
static void args(const char *name, bool take, int want, F change) {
    g_case = name;
    g_cases++;
    UdpRecvArgs a = good(take);
    change(a);
    CHECK(udp_recv_check_args(a) == want);
}

static void test_args() {
    const int OK = 0, KEYLEN = -1, ARG = -2;  // FPNN_AES_OK, _ERR_KEYLEN, _ERR_ARG
    for (bool take : {false, true}) {
        args("good", take, OK, [](UdpRecvArgs &) {});
        // the existing udp_check_args cases
        args("key_slot", take, ARG, [](UdpRecvArgs &a) { a.udp.key_slot = true; });
        args("b->flags", take, ARG, [](UdpRecvArgs &a) { a.udp.flags = 1; });
        args("u null", take, ARG, [](UdpRecvArgs &a) { a.udp.u = false; });
        args("data_keys of another engine", take, ARG, [](UdpRecvArgs &a) { a.udp.data_keys_same_engine = false; });
        uintptr_t UdpArgs::*const conn_ptrs[] = {&UdpArgs::first_dgram, &UdpArgs::conn_slot, &UdpArgs::pos_state,
                                                 &UdpArgs::iv_state};
        for (auto m : conn_ptrs) {
            args("null", take, ARG, [m](UdpRecvArgs &a) { a.udp.*m = 0; });
            args("misaligned", take, ARG, [m](UdpRecvArgs &a) { a.udp.*m += 2; });
            args("null, no connection", take, OK, [m](UdpRecvArgs &a) {
                a.udp.*m = 0;
                a.udp.nconn = 0;
            });
        }
        args("iv_state on a 4-byte grid only", take, ARG, [](UdpRecvArgs &a) { a.udp.iv_state += 4; });
        args("slot_bound above the package table", take, ARG, [](UdpRecvArgs &a) { a.udp.slot_bound = 9; });
        args("slot_bound above the data table", take, ARG, [](UdpRecvArgs &a) { a.udp.data_slots = 7; });
        args("24-byte package table", take, KEYLEN, [](UdpRecvArgs &a) { a.udp.nr_pkg = 12; });
        args("24-byte data table", take, KEYLEN, [](UdpRecvArgs &a) { a.udp.nr_data = 12; });
        args("argument errors come first", take, ARG, [](UdpRecvArgs &a) {
            a.udp.nr_pkg = 12;
            a.max_pkgs = 0;
        });
        // the sections are outputs
        args("nsections", take, ARG, [](UdpRecvArgs &a) { a.udp.nsections = 1; });
        args("first_section", take, ARG, [](UdpRecvArgs &a) { a.udp.first_section = 0x5000; });
        args("sec_off", take, ARG, [](UdpRecvArgs &a) { a.udp.sec_off = 0x5000; });
        args("sec_len", take, ARG, [](UdpRecvArgs &a) { a.udp.sec_len = 0x5000; });
        // the tables
        args("max_pkgs == 0", take, ARG, [](UdpRecvArgs &a) { a.max_pkgs = 0; });
        args("max_sections == 0", take, ARG, [](UdpRecvArgs &a) { a.max_sections = 0; });
        args("count * max_pkgs above 32 bits", take, ARG, [](UdpRecvArgs &a) {
            a.count = 1u << 20;
            a.max_pkgs = 1u << 12;
        });
        args("count * max_pkgs at 32 bits", take, OK, [](UdpRecvArgs &a) {
            a.count = 0xFFFFFFFFu;
            a.max_pkgs = a.max_sections = 1;
        });
        args("count * max_sections above 32 bits", take, ARG, [](UdpRecvArgs &a) {
            a.count = 1u << 20;
            a.max_sections = 1u << 12;
        });
        uintptr_t UdpRecvArgs::*const tabs[] = {&UdpRecvArgs::scan, &UdpRecvArgs::pkgs, &UdpRecvArgs::sections};
        for (auto m : tabs) {
            args("table null", take, ARG, [m](UdpRecvArgs &a) { a.*m = 0; });
            args("table misaligned", take, ARG, [m](UdpRecvArgs &a) { a.*m += 1; });
            args("table null, no datagram", take, OK, [m](UdpRecvArgs &a) {
                a.*m = 0;
                a.count = 0;
            });
        }
        args("pkgs on a 2-byte grid only", take, ARG, [](UdpRecvArgs &a) { a.pkgs += 2; });
        args("sections on a 2-byte grid only", take, ARG, [](UdpRecvArgs &a) { a.sections += 2; });
    }
    // recv alone: the flags
    args("WALK_ONLY", false, OK, [](UdpRecvArgs &a) { a.flags = UDP_F_WALK_ONLY; });
    args("PLAIN", false, OK, [](UdpRecvArgs &a) { a.flags = UDP_F_PLAIN; });
    args("PLAIN | WALK_ONLY", false, OK, [](UdpRecvArgs &a) { a.flags = UDP_F_PLAIN | UDP_F_WALK_ONLY; });
    args("unknown flag", false, ARG, [](UdpRecvArgs &a) { a.flags = 4; });
    args("unknown flag beside a known one", false, ARG, [](UdpRecvArgs &a) { a.flags = 0x80000001u; });
    args("PLAIN out of place", false, ARG, [](UdpRecvArgs &a) {
        a.flags = UDP_F_PLAIN;
        a.in_place = false;
    });
    args("out of place without PLAIN", false, OK, [](UdpRecvArgs &a) { a.in_place = false; });
    args("data_keys null", false, ARG, [](UdpRecvArgs &a) { a.udp.data_keys = false; });
    args("data_keys null with WALK_ONLY", false, OK, [](UdpRecvArgs &a) {
        a.udp.data_keys = false;
        a.flags = UDP_F_WALK_ONLY;
    });
    // recv_take alone: the lists
    args("data_keys null", true, ARG, [](UdpRecvArgs &a) { a.udp.data_keys = false; });
    args("flags on a take", true, ARG, [](UdpRecvArgs &a) { a.flags = UDP_F_WALK_ONLY; });
    args("first_take null", true, ARG, [](UdpRecvArgs &a) { a.first_take = 0; });
    args("take null", true, ARG, [](UdpRecvArgs &a) { a.take_list = 0; });
    args("first_take misaligned", true, ARG, [](UdpRecvArgs &a) { a.first_take += 2; });
    args("take misaligned", true, ARG, [](UdpRecvArgs &a) { a.take_list += 2; });
    args("no take, null lists", true, OK, [](UdpRecvArgs &a) { a.ntake = a.first_take = a.take_list = 0; });
    args("ntake * max_sections above 32 bits", true, ARG, [](UdpRecvArgs &a) {
        a.ntake = 1u << 30;
        a.max_sections = 8;
    });
}

// ---- routes ----
static BatchShape dgrams(uint64_t count, uint32_t len, bool inplace) {
    BatchShape b = {};
    b.count = count;
    b.stride = len;
    b.uniform_len = len;
    b.nkeys = 16384;
    b.inplace = inplace;
    return b;
}

static void test_route() {
    const DispatchShape D = shape(256);
    const BatchShape b = dgrams(1000, 1472, true);
    const UdpShape u = {100, 0, 14, 10};
    g_case = "single call: package decrypt, walk, data decrypt over count * max_sections segments";
    g_cases++;
    UdpRecvRoute r = udp_recv_route(D, b, u, false, 0, 3, 0);
    const UdpRoute dec = udp_route(D, b, {100, 3000, 14, 10}, false);
    CHECK(r.ok && r.package && r.data && r.nseg == 3000);
    CHECK(r.pkg.family == dec.pkg.family && r.pkg.km == KEY_LANE);
    for (int i = 0; i < kScratchBufs; i++) CHECK(r.need.n[i] == dec.need.n[i]);  // fpnn_aes_udp_decrypt of 3000 sections
    CHECK(r.need.n[SC_udp_off] == 3000 && r.need.n[SC_udp_u32] == 1000 + 3000 + 100 + 1 && r.need.n[SC_sf_slot] == 3000);
    g_case = "WALK_ONLY: the package decrypt alone";
    g_cases++;
    r = udp_recv_route(D, b, {100, 0, 0, 10}, false, UDP_F_WALK_ONLY, 3, 0);
    CHECK(r.ok && r.package && !r.data && r.nseg == 0);
    CHECK(r.need.n[SC_udp_off] == 0 && r.need.n[SC_udp_u32] == 1000 + 100 + 1 && r.need.n[SC_sf_slot] == 0);
    g_case = "PLAIN | WALK_ONLY: the walk alone, no scratch but the empty layout";
    g_cases++;
    r = udp_recv_route(D, b, u, false, UDP_F_PLAIN | UDP_F_WALK_ONLY, 3, 0);
    CHECK(r.ok && !r.package && !r.data && r.need.n[SC_udp_u32] == 100 + 1 && r.need.n[SC_bstart] == 0);
    g_case = "PLAIN: walk and data decrypt";
    g_cases++;
    r = udp_recv_route(D, b, u, false, UDP_F_PLAIN, 3, 0);
    CHECK(r.ok && !r.package && r.data && r.nseg == 3000 && r.need.n[SC_udp_u32] == 3000 + 100 + 1);
    CHECK(r.need.n[SC_boundary] == 0);
    g_case = "recv_take: ntake * max_sections segments";
    g_cases++;
    r = udp_recv_route(D, b, u, true, 0, 3, 700);
    CHECK(r.ok && !r.package && r.data && r.nseg == 2100);
    CHECK(r.need.n[SC_udp_off] == 2100 && r.need.n[SC_udp_u32] == 2100 + 100 + 1 && r.need.n[SC_sf_iv] == 2100);
    g_case = "key lengths";
    g_cases++;
    CHECK(!udp_recv_route(D, b, {100, 0, 12, 10}, false, 0, 3, 0).ok);
    CHECK(!udp_recv_route(D, b, {100, 0, 10, 12}, true, 0, 3, 7).ok);
    CHECK(udp_recv_route(D, b, {100, 0, 0, 14}, false, UDP_F_WALK_ONLY, 3, 0).ok);
}

// after reserve(max_segments, max_blocks) with max_segments >= max(count, nconn, count * max_sections) (recv)
// or max(nconn, ntake * max_sections) (recv_take) neither call grows scratch
static void test_reserve() {
    for (uint64_t cus : {256ull, 8ull}) {
        const DispatchShape D = shape(cus);
        for (uint64_t ms : {1ull, 1000ull, 1024ull, 20000ull}) {
            const uint64_t mb = ms * 92;
            const ScratchNeed res = need_reserve(D.scratch, ms, mb);
            for (uint32_t maxs : {1u, 3u, 8u})
                for (uint64_t items : {(uint64_t)0, (uint64_t)1, ms / maxs / 2, ms / maxs})
                    for (uint64_t nconn : {(uint64_t)1, ms / 2, ms})
                        for (int f = 0; f < 8; f++)
                            for (uint32_t flags = 0; flags < 4; flags++)
                                for (bool take : {false, true}) {
                                    if (take && flags) continue;
                                    if (items * maxs > ms) continue;  // (outside the bound)
                                    g_case = "reserve";
                                    g_cases++;
                                    // recv: `items` datagrams; recv_take: ms datagrams, `items` taken
                                    const uint64_t count = take ? ms : items;
                                    BatchShape b = dgrams(count, (f & 1) ? 1472 : 100, f & 2);
                                    if (f & 4) b.in_off = b.len = true;
                                    if ((uint64_t)((b.uniform_len + 15) / 16) * count > mb) continue;
                                    const UdpRecvRoute r =
                                        udp_recv_route(D, b, {nconn, 0, 14, 10}, take, flags, maxs, (uint32_t)items);
                                    CHECK(r.ok);
                                    for (int i = 0; i < kScratchBufs; i++) CHECK(r.need.n[i] <= res.n[i]);
                                }
        }
    }
}

int main() {
    test_args();
    test_route();
    test_reserve();
    printf("udp_recv_plan ok: %u cases\n", g_cases);
    return 0;
}
