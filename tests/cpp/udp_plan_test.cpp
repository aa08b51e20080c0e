// The UDP calls' host-only decisions (fpnn_amd/csrc/dispatch_plan.hpp: udp_check_args, udp_route;
// scratch_plan.hpp: need_udp_decrypt) on the CPU: every argument error of include/fpnn_aes.h,
// the route of the encrypt kernel (template choice, workgroup and grid) and the scratch the
// decrypt needs, against literals; and the promise of fpnn_aes_engine_reserve for both calls.
// Built and run by tests/test_udp_plan.py; prints one summary line, exits non-zero at the
// first miss.
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
static UdpArgs good() {  // two connections, three sections, 8-slot tables of 16- and 32-byte keys
    UdpArgs a = {};
    a.u = a.data_keys = a.data_keys_same_engine = true;
    a.nconn = 2;
    a.nsections = 3;
    a.slot_bound = 8;
    a.first_dgram = 0x1000;
    a.conn_slot = 0x2000;
    a.iv_state = 0x3000;
    a.pos_state = 0x4000;
    a.first_section = 0x5000;
    a.sec_off = 0x6000;
    a.sec_len = 0x7000;
    a.pkg_slots = a.data_slots = 8;
    a.nr_pkg = 10;
    a.nr_data = 14;
    return a;
}

template <class F>
static void args(const char *name, int want, F change) {
    g_case = name;
    g_cases++;
    UdpArgs a = good();
    change(a);
    CHECK(udp_check_args(a) == want);
}

static void test_args() {
    const int OK = 0, KEYLEN = -1, ARG = -2;  // FPNN_AES_OK, _ERR_KEYLEN, _ERR_ARG
    args("good", OK, [](UdpArgs &) {});
    args("key_slot", ARG, [](UdpArgs &a) { a.key_slot = true; });
    args("flags", ARG, [](UdpArgs &a) { a.flags = 1; });
    args("u null", ARG, [](UdpArgs &a) { a.u = false; });
    args("data_keys null with sections", ARG, [](UdpArgs &a) { a.data_keys = false; });
    args("data_keys null without sections", OK, [](UdpArgs &a) {
        a.data_keys = false;
        a.nsections = 0;
        a.first_section = a.sec_off = a.sec_len = 0;
    });
    args("data_keys of another engine", ARG, [](UdpArgs &a) { a.data_keys_same_engine = false; });
    // with nconn != 0: NULL or misaligned first_dgram, conn_slot or state arrays
    uintptr_t UdpArgs::*const conn_ptrs[] = {&UdpArgs::first_dgram, &UdpArgs::conn_slot, &UdpArgs::pos_state,
                                             &UdpArgs::iv_state};
    for (auto m : conn_ptrs) {
        args("null", ARG, [m](UdpArgs &a) { a.*m = 0; });
        args("misaligned", ARG, [m](UdpArgs &a) { a.*m += 2; });
        args("null, no connection", OK, [m](UdpArgs &a) {
            a.*m = 0;
            a.nconn = 0;
        });
    }
    args("iv_state on a 4-byte grid only", ARG, [](UdpArgs &a) { a.iv_state += 4; });
    args("pos_state on a 4-byte grid", OK, [](UdpArgs &a) { a.pos_state += 4; });
    // with sections: their three arrays
    uintptr_t UdpArgs::*const sec_ptrs[] = {&UdpArgs::first_section, &UdpArgs::sec_off, &UdpArgs::sec_len};
    for (auto m : sec_ptrs) {
        args("null", ARG, [m](UdpArgs &a) { a.*m = 0; });
        args("misaligned", ARG, [m](UdpArgs &a) { a.*m += 1; });
    }
    args("no sections: no section arrays", OK, [](UdpArgs &a) {
        a.nsections = 0;
        a.first_section = a.sec_off = a.sec_len = 0;
    });
    // slot_bound against the capacity of either table
    args("bound at both capacities", OK, [](UdpArgs &a) { a.slot_bound = 8; });
    args("bound above the package table", ARG, [](UdpArgs &a) { a.pkg_slots = 7; });
    args("bound above the data table", ARG, [](UdpArgs &a) { a.data_slots = 7; });
    args("bound 0", OK, [](UdpArgs &a) { a.slot_bound = 0; });
    // key lengths: 16 and 32 for each table, in every pair; 24 for neither
    for (int p : {10, 14})
        for (int d : {10, 14})
            args("pair", OK, [p, d](UdpArgs &a) {
                a.nr_pkg = p;
                a.nr_data = d;
            });
    args("24-byte package table", KEYLEN, [](UdpArgs &a) { a.nr_pkg = 12; });
    args("24-byte data table", KEYLEN, [](UdpArgs &a) { a.nr_data = 12; });
    args("argument errors come first", ARG, [](UdpArgs &a) {
        a.nr_pkg = 12;
        a.flags = 1;
    });
    args("nconn == 0", OK, [](UdpArgs &a) { a.nconn = 0; });
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

static void test_encrypt_route() {
    const DispatchShape D = shape(256);
    struct {
        const char *name;
        uint64_t nconn;
        int threads, grid;
    } const cases[] = {
        {"one connection", 1, 64, 1},
        {"16 connections: one wave", 16, 64, 1},
        {"17 connections", 17, 64, 2},
        {"4096 quads: a wave on every CU", 4096, 64, 256},
        {"4097", 4097, 128, 129},
        {"U2: 16 384 connections", 16384, 256, 256},
        {"a full chip of quads", 65536, 1024, 256},
        {"more than the chip's quads: the grid strides", 70000, 1024, 256},
        {"U2c", 262144, 1024, 256},
    };
    for (const auto &c : cases) {
        g_case = c.name;
        g_cases++;
        const UdpRoute r = udp_route(D, dgrams(4 * c.nconn, 1472, false), {c.nconn, 4 * c.nconn, 14, 10}, true);
        CHECK(r.ok && r.nr_data == 14 && r.nr_pkg == 10);
        CHECK(r.threads == c.threads && r.grid == c.grid);
        for (int i = 0; i < kScratchBufs; i++) CHECK(r.need.n[i] == 0);  // K2u needs no scratch
    }
    g_case = "no data table: the package rounds twice";
    g_cases++;
    const UdpRoute r = udp_route(D, dgrams(8, 64, false), {2, 0, 0, 14}, true);
    CHECK(r.ok && r.nr_data == 14 && r.nr_pkg == 14);
    g_case = "a 24-byte table has no kernel";
    g_cases++;
    CHECK(!udp_route(D, dgrams(8, 64, false), {2, 4, 12, 10}, true).ok);
    CHECK(!udp_route(D, dgrams(8, 64, false), {2, 4, 10, 12}, false).ok);
    const DispatchShape D8 = shape(8);
    g_case = "8 CUs";
    g_cases++;
    const UdpRoute r8 = udp_route(D8, dgrams(4000, 64, false), {1000, 4000, 10, 10}, true);
    CHECK(r8.threads == 512 && r8.grid == 8);
}

static void test_decrypt_route() {
    const DispatchShape D = shape(256);
    g_case = "U2 in place: dense keyed package decrypt, then the sections";
    g_cases++;
    UdpRoute r = udp_route(D, dgrams(1048576, 1472, true), {16384, 1048576, 14, 10}, false);
    CHECK(r.ok && r.pkg.family == DEC_DENSE && r.pkg.km == KEY_LANE && r.pkg.boundary_save);
    CHECK(r.need.n[SC_udp_off] == 1048576 && r.need.n[SC_udp_u32] == 1048576 + 1048576 + 16384 + 1);
    CHECK(r.need.n[SC_boundary] == 1048576ull * 92 / 64);
    CHECK(r.need.n[SC_sf_slot] == 1048576 && r.need.n[SC_sf_iv] == 1048576 && r.need.n[SC_snap_iv] == 1048576);
    CHECK(r.need.n[SC_bstart] == 1048576 + 1 && r.need.n[SC_desc_off] == 0 && r.need.n[SC_desc_len] == 0);
    g_case = "ragged datagrams: K1r twice";
    g_cases++;
    BatchShape b = dgrams(3000, 0, false);
    b.in_off = b.len = true;
    r = udp_route(D, b, {1000, 2500, 10, 14}, false);
    CHECK(r.ok && r.pkg.family == DEC_RAGGED && r.pkg.km == KEY_LANE);
    CHECK(r.need.n[SC_bstart] == 3001 && r.need.n[SC_sf_slot] == 2500 && r.need.n[SC_snap_iv] == 2500);
    CHECK(r.need.n[SC_udp_off] == 2500 && r.need.n[SC_udp_u32] == 3000 + 2500 + 1000 + 1);
    g_case = "no sections: the package decrypt alone";
    g_cases++;
    r = udp_route(D, b, {1000, 0, 0, 14}, false);
    CHECK(r.ok && r.need.n[SC_sf_slot] == 0 && r.need.n[SC_snap_iv] == 0 && r.need.n[SC_udp_off] == 0);
    CHECK(r.need.n[SC_udp_u32] == 3000 + 1000 + 1);
}

// after reserve(max_segments >= max(count, nsections, nconn), max_blocks) neither call grows scratch
static void test_reserve() {
    for (uint64_t cus : {256ull, 8ull}) {
        const DispatchShape D = shape(cus);
        for (uint64_t ms : {1ull, 1000ull, 1024ull, 20000ull}) {
            const uint64_t mb = ms * 92;
            const ScratchNeed res = need_reserve(D.scratch, ms, mb);
            const uint64_t ns[] = {0, 1, ms / 2, ms};
            for (uint64_t count : ns)
                for (uint64_t nsec : ns)
                    for (uint64_t nconn : ns)
                        for (int f = 0; f < 8; f++) {
                            g_case = "reserve";
                            g_cases++;
                            BatchShape b = dgrams(count, (f & 1) ? 1472 : 100, f & 2);
                            if (f & 4) b.in_off = b.len = true;
                            if ((uint64_t)((b.uniform_len + 15) / 16) * count > mb) continue;
                            const UdpRoute r = udp_route(D, b, {nconn, nsec, 14, 10}, false);
                            for (int i = 0; i < kScratchBufs; i++) CHECK(r.need.n[i] <= res.n[i]);
                        }
        }
    }
}

int main() {
    test_args();
    test_encrypt_route();
    test_decrypt_route();
    test_reserve();
    printf("udp_plan ok: %u cases\n", g_cases);
    return 0;
}
