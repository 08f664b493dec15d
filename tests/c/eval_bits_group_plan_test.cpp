// eval_bits_group_plan_test.cpp — replays the launch plan of k_eval_bits with a
// list coordinate (dpf-go_amd/csrc/eval_bits_plan.hpp: the keys of group g at
// group g's own point list) on the host, wave by wave and lane by lane, with
// the index functions the kernel itself calls.  Stand-alone, built with
// -fsanitize=address,undefined by tests/test_eval_bits_group_plan_cpu.py.
//
// Over npts x groups x keys per group x CU counts it asserts:
//   - every (key, unit) is owned by exactly one wave;
//   - every point index a lane loads, base + clamp, lies inside the key's OWN
//     list [g * npts, (g + 1) * npts) -- checked against an array of exactly
//     groups * npts points, so ASan sees an index past the lists;
//   - a tail lane loads g * npts + npts - 1, never a point of the next list,
//     and is outside the unit's mask;
//   - the row bytes written are those of the ungrouped plan: the first
//     eval_bits_stride(npts) bytes of every row once, none beyond;
//   - the form differs from the ungrouped one in the list fields only, and
//     keys_per_list = nkeys reproduces the ungrouped form field by field;
//   - a grid is refused at the ungrouped bound, and so are keys that are not
//     whole lists' worth and lists whose bytes overflow 64 bits.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "eval_bits_plan.hpp"

using namespace dpfh;

static int g_fail = 0;
#define CHECK(c, ...)                                  \
    do {                                               \
        if (!(c)) {                                    \
            if (++g_fail <= 20) {                      \
                fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #c); \
                fprintf(stderr, __VA_ARGS__);          \
                fprintf(stderr, "\n");                 \
            }                                          \
        }                                              \
    } while (0)

typedef unsigned long long ull;

static bool same_tree(const TreeForm& a, const TreeForm& b) {
    return a.d == b.d && a.block == b.block && a.W == b.W && a.ltop == b.ltop && a.units_log == b.units_log &&
           a.nunits == b.nunits && a.grid == b.grid && a.sub_base == b.sub_base && a.uniform == b.uniform &&
           a.nodes == b.nodes && a.raw == b.raw && a.cw_lds == b.cw_lds && a.walk == b.walk && a.l1 == b.l1 &&
           a.feedback == b.feedback && a.prio_small == b.prio_small;
}
// Every field but the two list fields.
static bool same_launch(const EvalBitsForm& a, const EvalBitsForm& b) {
    return a.L == b.L && a.kernel == b.kernel && a.block == b.block && a.grid == b.grid && a.units == b.units &&
           a.nwaves == b.nwaves && a.last_mask[0] == b.last_mask[0] && a.last_mask[1] == b.last_mask[1] &&
           same_tree(a.nodes, b.nodes);
}

static void replay(uint64_t groups, uint64_t kpg, uint64_t npts, uint64_t cus, uint32_t logN) {
    const uint32_t stop = logN > 7 ? logN - 7 : 0;
    const TreeKnobs knobs;
    const uint64_t nkeys = groups * kpg;
    const uint64_t fb = eval_frontier_bytes(nkeys, stop, npts);
    EvalBitsForm f, flat;
    memset(&f, 0, sizeof f);
    memset(&flat, 0, sizeof flat);
    const bool ok = eval_bits_form_lists(nkeys, kpg, npts, stop, logN, fb, cus, knobs, &f);
    CHECK(ok, "groups %llu kpg %llu npts %llu refused", (ull)groups, (ull)kpg, (ull)npts);
    CHECK(eval_bits_form(nkeys, npts, stop, logN, fb, cus, knobs, &flat), "ungrouped refused");
    if (!ok) return;
    CHECK(same_launch(f, flat), "the launch differs from the ungrouped one");
    CHECK(f.keys_per_list == kpg && f.nlists == groups, "lists %llu x %llu", (ull)f.nlists, (ull)f.keys_per_list);
    CHECK(flat.keys_per_list == nkeys && flat.nlists == 1, "the ungrouped form is one list");
    const uint64_t units = (npts + 127) / 128, stride = 16 * units;
    CHECK(f.units == units && eval_bits_stride(npts) == stride && f.nwaves == nkeys * units, "units");

    // The lists as the kernel sees them: exactly groups * npts points, point
    // j of list g holding its own (list, index).
    std::vector<uint64_t> xs(groups * npts);
    for (uint64_t g = 0; g < groups; ++g)
        for (uint64_t j = 0; j < npts; ++j) xs[g * npts + j] = (g << 32) | j;
    std::vector<uint8_t> owned(nkeys * units, 0);
    std::vector<uint8_t> rows(nkeys * (stride + 16), 0);   // one guard unit behind every row
    const uint64_t wpb = f.block / 64;
    for (uint64_t blk = 0; blk < f.grid; ++blk)
        for (uint64_t wib = 0; wib < wpb; ++wib) {
            const uint64_t w = blk * wpb + wib;           // the kernel's wave index
            if (w >= f.nwaves) continue;                  // not live
            const uint64_t key = w / f.units, unit = w - key * f.units;
            CHECK(key < nkeys && unit < units, "wave %llu", (ull)w);
            if (key >= nkeys || unit >= units) continue;
            ++owned[key * units + unit];
            const uint64_t list = eval_bits_list(key, f.keys_per_list);
            CHECK(list == key / kpg && list < groups, "list %llu of key %llu", (ull)list, (ull)key);
            const uint64_t base = eval_bits_list_base(list, npts);
            CHECK(base == list * npts, "base");
            const uint64_t off = eval_bits_unit_off(unit);
            CHECK(off + 16 <= stride, "span of unit %llu leaves the row", (ull)unit);
            for (uint64_t b = off; b < off + 16; ++b) ++rows[key * (stride + 16) + b];
            // Lanes: the first and the last two units of a key in full, of
            // the ones between (all alike) only the first and last lane.
            const bool full = unit < 1 || unit + 2 >= units;
            for (uint32_t half = 0; half < 2; ++half) {
                const uint64_t mask = eval_bits_mask(npts, unit, half);
                for (uint32_t lane = 0; lane < 64; lane += full ? 1 : 63) {
                    const uint64_t j = eval_bits_point(unit, lane, half);
                    const uint64_t at = base + eval_bits_clamp(j, npts);
                    CHECK(at >= list * npts && at < (list + 1) * npts, "index %llu leaves list %llu", (ull)at, (ull)list);
                    const uint64_t x = xs[at];            // what the lane loads
                    CHECK((x >> 32) == list, "key %llu read a point of list %llu", (ull)key, (ull)(x >> 32));
                    if (j < npts) {
                        CHECK((x & 0xffffffffu) == j && ((mask >> lane) & 1), "live lane");
                    } else {
                        CHECK(at == list * npts + npts - 1, "tail lane clamps to %llu", (ull)at);
                        CHECK(!((mask >> lane) & 1), "tail lane inside the mask");
                    }
                }
            }
        }
    for (uint64_t i = 0; i < nkeys * units; ++i) CHECK(owned[i] == 1, "(key, unit) %llu owned %u times", (ull)i, owned[i]);
    for (uint64_t k = 0; k < nkeys; ++k) {
        for (uint64_t b = 0; b < stride; ++b)
            CHECK(rows[k * (stride + 16) + b] == 1, "key %llu byte %llu written %u times", (ull)k, (ull)b,
                  rows[k * (stride + 16) + b]);
        for (uint64_t b = stride; b < stride + 16; ++b) CHECK(rows[k * (stride + 16) + b] == 0, "write past the span");
    }
}

static void limits() {
    const TreeKnobs knobs;
    const uint64_t cus = 256;
    EvalBitsForm f, g;
    // The grid bound is the ungrouped one: 8 waves per 512-thread workgroup.
    const uint64_t most = 8 * kMaxGrid;
    CHECK(eval_bits_form_lists(most, 8, 128, 13, 20, 0, cus, knobs, &f) && f.grid == kMaxGrid, "largest grid");
    CHECK(!eval_bits_form_lists(most + 8, 8, 128, 13, 20, 0, cus, knobs, &f), "one list too many");
    CHECK(eval_bits_form_lists(most / 2, 4, 129, 13, 20, 0, cus, knobs, &f) && f.grid == kMaxGrid, "two units per key");
    CHECK(!eval_bits_form_lists(most / 2 + 4, 4, 129, 13, 20, 0, cus, knobs, &f), "two units, one list too many");
    const uint64_t many[] = {6, 4098, most, most + 6};
    for (uint64_t nkeys : many)
        for (uint64_t npts : {1ull, 128ull, 1000ull, (1ull << 20) + 1})
            CHECK(eval_bits_form_lists(nkeys, 2, npts, 13, 20, 0, cus, knobs, &f) ==
                      eval_bits_form(nkeys, npts, 13, 20, 0, cus, knobs, &g),
                  "refused where the ungrouped form is not");
    // Keys that are not whole lists' worth, and no keys per list.
    CHECK(!eval_bits_form_lists(7, 2, 128, 13, 20, 0, cus, knobs, &f), "7 keys, 2 a list");
    CHECK(!eval_bits_form_lists(8, 0, 128, 13, 20, 0, cus, knobs, &f), "0 keys a list");
    // nlists * npts points: their count, and their bytes, must fit 64 bits.
    CHECK(!eval_bits_lists_ok(1ull << 32, 1ull << 32), "2^64 points");
    CHECK(!eval_bits_lists_ok(1ull << 40, 1ull << 30), "2^70 points");
    CHECK(!eval_bits_lists_ok(1ull << 31, 1ull << 30), "2^61 points are 2^64 bytes");
    CHECK(eval_bits_lists_ok((1ull << 31) - 1, 1ull << 30), "just below");
    CHECK(eval_bits_lists_ok(~0ull, 0) && eval_bits_lists_ok(0, ~0ull) && eval_bits_lists_ok(1, ~0ull >> 3), "edges");
    CHECK(!eval_bits_lists_ok(2, ~0ull >> 3), "twice the largest list");
    CHECK(!eval_bits_form_lists(1ull << 32, 1, 1ull << 32, 13, 20, 0, cus, knobs, &f), "form: 2^64 points");
    CHECK(!eval_bits_form_lists(1ull << 31, 1, 1ull << 30, 13, 20, 0, cus, knobs, &f), "form: 2^64 bytes");
    // keys_per_list = nkeys is the ungrouped form, field by field, frontier included.
    for (uint64_t nkeys : {1ull, 5ull, 4097ull})
        for (uint64_t npts : {1ull, 31ull, 32ull, 129ull, 4096ull}) {
            const uint64_t fb = eval_frontier_bytes(nkeys, 17, npts);
            memset(&f, 0, sizeof f);
            memset(&g, 0, sizeof g);
            CHECK(eval_bits_form_lists(nkeys, nkeys, npts, 17, 24, fb, cus, knobs, &f) &&
                      eval_bits_form(nkeys, npts, 17, 24, fb, cus, knobs, &g),
                  "accepted");
            CHECK(same_launch(f, g) && f.keys_per_list == g.keys_per_list && f.nlists == g.nlists && g.nlists == 1,
                  "nkeys %llu npts %llu", (ull)nkeys, (ull)npts);
            CHECK(f.L == eval_frontier_level(17, npts), "frontier level");
        }
    // The frontier is a key's own: the level of a grouped launch is the ungrouped one's, with the same fall-backs.
    const uint64_t fb = eval_frontier_bytes(6, 17, 4096);
    CHECK(eval_bits_form_lists(6, 2, 4096, 17, 24, fb, cus, knobs, &f) && f.L == 11, "full area");
    CHECK(eval_bits_form_lists(6, 2, 4096, 17, 24, fb - 1, cus, knobs, &f) && f.L == 0, "area one byte short");
    CHECK(eval_bits_form_lists(6, 2, 4096, 57, 64, ~0ull, cus, knobs, &f) && f.L == 0, "logN > 63");
}

int main() {
    const uint64_t npts[] = {1, 64, 127, 128, 129, 257, 1000};
    const uint64_t groups[] = {1, 3, 65};
    const uint64_t kpg[] = {1, 2, 5};
    const uint64_t cus[] = {4, 256};
    for (uint64_t n : npts)
        for (uint64_t g : groups)
            for (uint64_t k : kpg)
                for (uint64_t c : cus) replay(g, k, n, c, 40);
    replay(3, 2, 300, 256, 7);    // stop 0
    replay(3, 2, 300, 256, 63);
    limits();
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("eval_bits_group_plan ok\n");
    return 0;
}
