// The engine's scratch sizes (fpnn_amd/csrc/scratch_plan.hpp) on the CPU: the capacity policy
// against a restatement of its rule, and the promise of fpnn_aes_engine_reserve -- what it asks
// of every buffer covers what every call path asks within its bounds, so such a call neither
// allocates nor memsets.  Built and run by tests/test_scratch_plan.py; prints one summary
// line, exits non-zero at the first broken property.
#include "../../fpnn_amd/csrc/scratch_plan.hpp"

#include <stdio.h>
#include <stdlib.h>

using namespace fpnn_aes;

static char g_case[160] = "";

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            fprintf(stderr, "%s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, g_case); \
            exit(1);                                                                \
        }                                                                           \
    } while (0)

// the rule itself: 1024 elements first, then doubling, until the need is covered
static uint64_t rule(uint64_t cap, uint64_t need) {
    if (need <= cap) return cap;
    uint64_t n = cap ? cap : 1024;
    while (n < need) n *= 2;
    return n;
}

static uint64_t g_policy = 0, g_contract = 0;

static void test_policy() {
    for (uint64_t need = 0; need <= 5000; need++) {
        snprintf(g_case, sizeof g_case, "policy cap 0 need %llu", (unsigned long long)need);
        const uint64_t c = scratch_next_cap(0, need);
        CHECK(c == rule(0, need));
        CHECK(need == 0 ? c == 0 : c >= 1024 && c >= need && (c & (c - 1)) == 0 && (c == 1024 || c / 2 < need));
        g_policy++;
    }
    // grown capacities (and ones no growth from 1024 reaches: the rule doubles whatever it holds)
    const uint64_t caps[] = {1024, 2048, 4096, 1ull << 20, 1ull << 33, 1000, 3000};
    for (uint64_t cap : caps) {
        const uint64_t needs[] = {0, 1, cap - 1, cap, cap + 1, 2 * cap - 1, 2 * cap, 2 * cap + 1, 5 * cap, 1ull << 40};
        for (uint64_t need : needs) {
            snprintf(g_case, sizeof g_case, "policy cap %llu need %llu", (unsigned long long)cap, (unsigned long long)need);
            const uint64_t c = scratch_next_cap(cap, need);
            CHECK(c == rule(cap, need));
            if (need <= cap) CHECK(c == cap);
            else CHECK(c >= need && c / 2 < need && c % cap == 0);
            g_policy++;
        }
    }
}

// stand-ins for block_map_onepass_words: any non-decreasing function of the segment count
static uint64_t words_a(uint64_t n) { return 3 + (n + 2047) / 2048; }
static uint64_t words_b(uint64_t n) { return 1 + n / 7; }

static void covered(const ScratchNeed &need, const ScratchNeed &res) {
    for (int i = 0; i < kScratchBufs; i++) CHECK(need.n[i] <= res.n[i]);
    g_contract++;
}

static void test_contract(const ScratchShape &s) {
    const uint64_t segs[] = {1, 1023, 1024, 16384, 16385, 100000};
    const uint64_t blks[] = {0, 1, 63, 64, 65, 65536, 66000 * 64ull, (1ull << 32) - 1};
    for (uint64_t ms : segs) {
        for (uint64_t mb : blks) {
            const ScratchNeed res = need_reserve(s, ms, mb);
            snprintf(g_case, sizeof g_case, "reserve(%llu, %llu), %llu CUs", (unsigned long long)ms, (unsigned long long)mb,
                     (unsigned long long)s.num_cus);
            // what reserve has always covered
            CHECK(res.n[SC_boundary] == (mb + 63) / 64 + 1);
            CHECK(res.n[SC_ecdh] == 49 * ms);
            CHECK(res.n[SC_lookback] == s.onepass_words(ms));
            CHECK(res.n[SC_bstart] == ms + 1 && res.n[SC_perm] == ms && res.n[SC_sf_slot] == ms);
            CHECK(res.n[SC_buckets] == s.length_order_words);
            // not its business (scratch_plan.hpp's header comment)
            CHECK(res.n[SC_fr_off] == 0 && res.n[SC_fr_slot] == 0 && res.n[SC_sstate] == 0);
            const uint64_t bl[] = {0, 1, mb / 2, mb ? mb - 1 : 0, mb};
            for (uint64_t b : bl) covered(need_decrypt_dense_inplace(b), res);
            if (mb != blks[0]) continue;  // the segment paths do not depend on max_blocks
            for (uint64_t n = 0; n <= ms; n++) {
                for (int f = 0; f < 8; f++) {
                    const bool x = f & 1, in_off = f & 2, len = f & 4;
                    covered(need_decrypt_ragged(s, n, x, in_off, len), res);
                    covered(need_decrypt_frames(s, n, x, in_off, len), res);
                }
                covered(need_encrypt_ragged(s, n, false), res);
                covered(need_encrypt_ragged(s, n, true), res);
                covered(need_ecdh_accept(n, 16), res);
                covered(need_ecdh_accept(n, 32), res);
            }
        }
    }
}

int main() {
    test_policy();
    // a whole chip and a single CU; both sides of small_max among the segment counts
    test_contract(ScratchShape{256, 16, 16384, words_a, 260});
    test_contract(ScratchShape{1, 16, 16384, words_b, 260});
    test_contract(ScratchShape{304, 16, 1024, words_a, 260});
    printf("scratch_plan ok: %llu policy cases, %llu covered needs\n", (unsigned long long)g_policy,
           (unsigned long long)g_contract);
    return 0;
}
