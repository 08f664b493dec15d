// pir_window_plan_test.cpp — the window plan and the balanced shard split of
// dpf-go_amd/csrc/pir_window_plan.hpp, stand-alone, under ASan + UBSan
// (tests/test_window_plan_cpu.py).  Prints "PLAN logN first nblocks: ..."
// lines for the windows named on the command line, else checks everything.
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

#include "pir_window_plan.hpp"

using namespace dpfh;

static int g_fail = 0;
#define CHECK(c)                                                                                              \
    do {                                                                                                      \
        if (!(c)) {                                                                                           \
            if (g_fail++ < 20) fprintf(stderr, "%s:%d: %s (logN %u fb %llu nb %llu)\n", __FILE__, __LINE__, #c, \
                                       g_logN, (unsigned long long)g_fb, (unsigned long long)g_nb);          \
        }                                                                                                     \
    } while (0)
static uint32_t g_logN;
static uint64_t g_fb, g_nb;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {   // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static void check_window(uint32_t logN, uint64_t fb, uint64_t nb) {
    g_logN = logN, g_fb = fb, g_nb = nb;
    CHECK(window_ok(logN, fb, nb));
    const WindowPlan w = window_plan(logN, fb, nb);
    const uint32_t stop = logN > 7 ? logN - 7 : 0;
    CHECK(w.prefix_bits <= stop);
    CHECK(w.prefix_bits + w.s == logN);
    CHECK(w.npieces >= 1 && w.npieces <= 33);
    CHECK(w.prefix_bits == 64 || w.first_prefix + w.npieces <= (1ull << w.prefix_bits));
    CHECK(w.piece_bytes == (logN < 7 ? 16 : (1ull << w.s) / 8));
    CHECK(w.row_bytes == w.npieces * w.piece_bytes);
    CHECK(w.row_offset % 16 == 0);
    if (logN < 7) {
        CHECK(w.route == kWindowSubtree && w.row_offset == 0 && w.prefix_bits == 0 && w.first_prefix == 0);
        return;
    }
    // The pieces tile [row_offset, row_offset + 16 * nblocks) of the row:
    // in blocks, piece p holds domain blocks [(first_prefix + p) << bs, ... + 2^bs).
    const uint32_t bs = w.s - 7;
    const uint64_t row0 = w.first_prefix << bs, row_blocks = w.npieces << bs;   // the row's first block, its blocks
    CHECK(row0 <= fb && fb + nb <= row0 + row_blocks);
    CHECK(w.row_offset == 16 * (fb - row0));
    CHECK(w.row_offset + 16 * nb <= w.row_bytes);
    // ... and every piece touches the window (none wasted at either end).
    CHECK(fb < row0 + (1ull << bs));
    CHECK(fb + nb > row0 + row_blocks - (1ull << bs));
    CHECK(row0 + row_blocks <= window_domain_blocks(logN));
    // The smallest aligned run of 2^eb blocks that holds the window, found by search.
    uint32_t eb = 0;
    while ((fb >> eb) != ((fb + nb - 1) >> eb)) ++eb;
    CHECK(eb == window_enclosing_log(fb, nb));
    const bool aligned = (nb & (nb - 1)) == 0 && fb % nb == 0;
    const bool enclosed = (1ull << eb) <= 2 * nb;            // at most twice the window: one subtree
    CHECK(!aligned || (enclosed && (1ull << eb) == nb));
    CHECK((w.route == kWindowSubtree) == enclosed);
    if (enclosed) {
        CHECK(w.npieces == 1 && bs == eb && w.first_prefix == fb >> eb && w.row_bytes == 16ull << eb);
        CHECK(!aligned || w.row_offset == 0);
        CHECK(row_blocks <= 2 * nb);
        return;
    }
    const uint32_t m = floor_log2(128 * nb);
    CHECK(w.s == (m < 11 ? 7u : m - 4));
    const uint64_t outside = row_blocks - nb;   // blocks evaluated outside the window
    if (w.s > 7) {
        // 16 <= window / piece < 32, so fewer than two pieces outside: at most 1/8 of the window.
        CHECK((nb >> bs) >= 16 && (nb >> bs) < 32);
        CHECK(outside < (2ull << bs));
        CHECK(8 * outside < nb);
    } else {
        CHECK(outside == 0 && w.npieces == nb);
    }
    // Sub-key lengths: reroot_key's, and the canonical one.
    const uint64_t klen = 33 + 18ull * stop;
    CHECK(window_sub_key_len(klen, w.prefix_bits) == 33 + 18ull * (w.s - 7));
    CHECK(window_canonical_sub_key_len(w) == 33 + 18ull * (w.s - 7));
    CHECK(window_sub_key_len(klen + 5, w.prefix_bits) == 38 + 18ull * (w.s - 7));
}

static void check_split() {
    for (uint64_t nrec : {0ull, 1ull, 255ull, 256ull, 257ull, 1000ull, 5123ull, 5ull << 21, (1ull << 24) + 1, ~0ull - 300})
        for (uint64_t n = 1; n <= 9; ++n) {
            const uint64_t sl = balanced_slice(nrec, n);
            g_logN = 0, g_fb = nrec, g_nb = n;
            const uint64_t sg = nrec / 256 + (nrec % 256 != 0), per = sl / 256;   // super-groups: all, per shard
            CHECK(sl % 256 == 0);
            // n shards of `per` super-groups hold them all; of one less they do not.
            CHECK(per >= sg / n && (per > sg / n || sg % n == 0));
            CHECK(per == 0 ? sg == 0 : (per - 1) <= (sg - 1) / n);
            if (nrec < (1ull << 40)) CHECK(sl == ((nrec + 255) / 256 + n - 1) / n * 256);   // shard g starts at g * this
        }
}

int main(int argc, char** argv) {
    if (argc > 1) {
        for (int i = 1; i + 2 < argc; i += 3) {
            const uint32_t logN = (uint32_t)strtoul(argv[i], nullptr, 10);
            const uint64_t fb = strtoull(argv[i + 1], nullptr, 10), nb = strtoull(argv[i + 2], nullptr, 10);
            if (!window_ok(logN, fb, nb)) {
                printf("PLAN %u %llu %llu: refused\n", logN, (unsigned long long)fb, (unsigned long long)nb);
                continue;
            }
            const WindowPlan w = window_plan(logN, fb, nb);
            printf("PLAN %u %llu %llu: route %u prefix_bits %u first_prefix %llu npieces %llu piece_bytes %llu row_bytes %llu "
                   "row_offset %llu\n",
                   logN, (unsigned long long)fb, (unsigned long long)nb, w.route, w.prefix_bits,
                   (unsigned long long)w.first_prefix, (unsigned long long)w.npieces, (unsigned long long)w.piece_bytes,
                   (unsigned long long)w.row_bytes, (unsigned long long)w.row_offset);
        }
        return 0;
    }
    uint64_t n = 0;
    for (uint32_t logN = 0; logN < 7; ++logN) check_window(logN, 0, 1), ++n;
    for (uint32_t logN = 7; logN <= 12; ++logN) {
        const uint64_t dom = window_domain_blocks(logN);
        for (uint64_t fb = 0; fb < dom; ++fb)
            for (uint64_t nb = 1; fb + nb <= dom; ++nb) check_window(logN, fb, nb), ++n;
    }
    for (uint32_t logN : {20u, 40u, 63u}) {
        const uint64_t dom = window_domain_blocks(logN);
        for (int i = 0; i < 20000; ++i) {
            const uint64_t nb = 1 + (rnd() >> (rnd() % 64)) % dom;
            const uint64_t fb = rnd() % (dom - nb + 1);
            check_window(logN, fb, nb), ++n;
            check_window(logN, dom - nb, nb), ++n;   // touches the last block of the domain
        }
        check_window(logN, dom - 1, 1), ++n;
        check_window(logN, 0, dom), ++n;
        check_window(logN, 1, dom - 1), ++n;
        check_window(logN, 0, dom - 1), ++n;
    }
    // Refusals.
    g_logN = 0, g_fb = 0, g_nb = 0;
    CHECK(!window_ok(64, 0, 1));
    CHECK(!window_ok(10, 0, 0));
    CHECK(!window_ok(10, 8, 1));
    CHECK(!window_ok(10, 7, 2));
    CHECK(!window_ok(10, 0, 9));
    CHECK(!window_ok(63, 1ull << 56, 1));
    CHECK(!window_ok(63, 1, ~0ull));
    CHECK(!window_ok(5, 0, 2));
    CHECK(window_records_ok(16, 128 * 37, 65536 - 128 * 37) && !window_records_ok(16, 128 * 37, 65536 - 128 * 37 + 1));
    CHECK(!window_records_ok(16, 64, 1) && !window_records_ok(64, 0, 1) && window_records_ok(63, 1ull << 62, 1ull << 62));
    CHECK(window_blocks_of(1) == 1 && window_blocks_of(128) == 1 && window_blocks_of(129) == 2 &&
          window_blocks_of(~0ull) == (1ull << 57));
    check_split();
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("pir_window_plan ok: %llu windows\n", (unsigned long long)n);
    return 0;
}
