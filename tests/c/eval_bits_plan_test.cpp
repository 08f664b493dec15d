// eval_bits_plan_test.cpp — replays the launch plan of k_eval_bits
// (dpf-go_amd/csrc/eval_bits_plan.hpp) on the host, wave by wave and lane by
// lane, with the index functions the kernel itself calls.  Stand-alone, built
// with -fsanitize=address,undefined by tests/test_eval_bits_plan_cpu.py.
//
// Over npts x nkeys x CU counts it asserts:
//   - every (key, unit) is owned by exactly one wave;
//   - every row byte below the stride is written exactly once, none beyond;
//   - the last unit's masks have exactly npts - 128 (units - 1) valid lanes,
//     and every other unit's are full;
//   - a clamped index never exceeds npts - 1;
//   - a grid is refused exactly when it exceeds kMaxGrid;
//   - the frontier level equals eval_frontier_level(stop, npts) with the full
//     frontier area, and 0 (root walks) where eval_form falls back.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

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

static int popcount64(uint64_t x) { return __builtin_popcountll(x); }

// Replays one launch: the waves in grid order.  A key's waves follow one
// another (key = w / units), so one row of byte counters at a time suffices.
static void replay(uint64_t nkeys, uint64_t npts, uint64_t cus, uint32_t logN) {
    const uint32_t stop = logN > 7 ? logN - 7 : 0;
    const TreeKnobs knobs;
    const uint64_t fb = eval_frontier_bytes(nkeys, stop, npts);
    EvalBitsForm f;
    const bool ok = eval_bits_form(nkeys, npts, stop, logN, fb, cus, knobs, &f);
    CHECK(ok, "nkeys %llu npts %llu refused", (unsigned long long)nkeys, (unsigned long long)npts);
    if (!ok) return;
    const uint64_t units = (npts + 127) / 128, stride = 16 * units;
    CHECK(f.units == units && eval_bits_stride(npts) == stride, "units %llu", (unsigned long long)f.units);
    CHECK(f.nwaves == nkeys * units, "nwaves");
    CHECK(f.kernel == kEvalBitsPair, "kernel");
    CHECK(f.L == eval_frontier_level(stop, npts), "L %u", f.L);
    CHECK(f.block >= 64 && f.block <= (uint32_t)kBlock && f.block % 64 == 0 && (f.block & (f.block - 1)) == 0,
          "block %u", f.block);
    CHECK(f.block == pick_block(f.nwaves * 64, kBlock, cus), "block %u", f.block);
    CHECK(f.grid == (f.nwaves * 64 + f.block - 1) / f.block && f.grid <= kMaxGrid, "grid");
    // The last unit's valid lanes.
    const uint64_t tail = npts - 128 * (units - 1);
    CHECK((uint64_t)(popcount64(f.last_mask[0]) + popcount64(f.last_mask[1])) == tail, "tail lanes");
    CHECK(f.last_mask[0] == (tail >= 64 ? ~0ull : (1ull << tail) - 1), "mask 0");
    CHECK(f.last_mask[1] == (tail <= 64 ? 0ull : tail >= 128 ? ~0ull : (1ull << (tail - 64)) - 1), "mask 1");

    std::vector<uint8_t> key_seen(nkeys, 0), unit_seen(units, 0);
    // One guard unit past the stride: a write beyond the span is counted, not lost.
    std::vector<uint8_t> row(stride + 16, 0);
    uint64_t cur = ~0ull, owned = 0;
    auto close_row = [&] {
        if (cur == ~0ull) return;
        for (uint64_t b = 0; b < stride; ++b) CHECK(row[b] == 1, "key %llu byte %llu written %u times",
                                                    (unsigned long long)cur, (unsigned long long)b, row[b]);
        for (uint64_t b = stride; b < stride + 16; ++b) CHECK(row[b] == 0, "write past the span");
        for (uint64_t u = 0; u < units; ++u) CHECK(unit_seen[u] == 1, "unit %llu", (unsigned long long)u);
    };
    const uint64_t wpb = f.block / 64;
    for (uint64_t blk = 0; blk < f.grid; ++blk)
        for (uint64_t wib = 0; wib < wpb; ++wib) {
            const uint64_t w = blk * wpb + wib;           // the kernel's wave index
            if (w >= f.nwaves) continue;                  // not live
            const uint64_t key = w / f.units, unit = w - key * f.units;
            CHECK(key < nkeys && unit < units, "wave %llu", (unsigned long long)w);
            if (key >= nkeys || unit >= units) continue;
            if (key != cur) {
                close_row();
                CHECK(!key_seen[key], "key %llu revisited", (unsigned long long)key);
                key_seen[key] = 1;
                cur = key;
                std::fill(row.begin(), row.end(), 0);
                std::fill(unit_seen.begin(), unit_seen.end(), 0);
            }
            ++unit_seen[unit];
            ++owned;
            const uint64_t off = eval_bits_unit_off(unit);
            CHECK(off + 16 <= stride, "span of unit %llu leaves the row", (unsigned long long)unit);
            for (uint64_t b = off; b < off + 16 && b < row.size(); ++b) ++row[b];
            // Lanes: the first and the last two units of a key in full, of
            // the ones between (all alike) only the first and last lane.
            const bool full = unit < 1 || unit + 2 >= units;
            const uint64_t inner = full ? 0 : 0x7ffffffffffffffeull;   // lanes 1..62 of such a unit: not replayed
            uint64_t m[2] = {inner, inner};
            for (uint32_t half = 0; half < 2; ++half)
                for (uint32_t lane = 0; lane < 64; lane += full ? 1 : 63) {
                    const uint64_t j = eval_bits_point(unit, lane, half);
                    CHECK(j == 128 * unit + 64 * half + lane, "point");
                    const uint64_t c = eval_bits_clamp(j, npts);
                    CHECK(c <= npts - 1 && (j >= npts || c == j), "clamp %llu", (unsigned long long)c);
                    if (j < npts) m[half] |= 1ull << lane;
                }
            for (uint32_t half = 0; half < 2; ++half) {
                CHECK(m[half] == eval_bits_mask(npts, unit, half), "mask of unit %llu", (unsigned long long)unit);
                if (unit + 1 < units) CHECK(m[half] == ~0ull, "inner unit not full");
                else CHECK(m[half] == f.last_mask[half], "last mask");
            }
        }
    close_row();
    CHECK(owned == f.nwaves, "owned %llu of %llu", (unsigned long long)owned, (unsigned long long)f.nwaves);
    for (uint64_t k = 0; k < nkeys; ++k) CHECK(key_seen[k], "key %llu never visited", (unsigned long long)k);
}

// Refusal exactly above kMaxGrid, and the frontier fall-backs.
static void limits() {
    const TreeKnobs knobs;
    const uint64_t cus = 256;
    EvalBitsForm f;
    // 8 waves per 512-thread workgroup: kMaxGrid workgroups hold 8 * kMaxGrid units.
    const uint64_t most = 8 * kMaxGrid;
    CHECK(eval_bits_form(most, 128, 13, 20, 0, cus, knobs, &f) && f.grid == kMaxGrid, "largest grid");
    CHECK(eval_bits_form(most / 2, 129, 13, 20, 0, cus, knobs, &f) && f.grid == kMaxGrid,
          "largest grid, two units per key");
    CHECK(!eval_bits_form(most / 2 + 1, 129, 13, 20, 0, cus, knobs, &f), "two units too many");
    CHECK(!eval_bits_form(most + 1, 128, 13, 20, 0, cus, knobs, &f), "one unit too many");
    CHECK(!eval_bits_form(1ull << 40, 1ull << 20, 13, 20, 0, cus, knobs, &f), "huge");
    CHECK(!eval_bits_form(~0ull, ~0ull, 13, 20, 0, cus, knobs, &f), "wraps");
    for (uint64_t nkeys : {1ull, 3ull, 4097ull})
        for (uint64_t npts : {1ull, 128ull, 1000ull, (1ull << 20) + 1}) {
            const uint64_t nw = nkeys * ((npts + 127) / 128);
            const uint32_t b = pick_block(nw * 64, kBlock, cus);
            const bool fits = (nw * 64 + b - 1) / b <= kMaxGrid;
            CHECK(eval_bits_form(nkeys, npts, 13, 20, 0, cus, knobs, &f) == fits, "refusal rule");
        }
    // Frontier: the rule of eval_form.
    const uint64_t npts = 4096;
    const uint32_t stop = 17, logN = 24;
    const uint64_t fb = eval_frontier_bytes(5, stop, npts);
    CHECK(eval_frontier_level(stop, npts) == 11 && fb > 0, "frontier level");
    CHECK(eval_bits_form(5, npts, stop, logN, fb, cus, knobs, &f) && f.L == 11 && f.nodes.nodes &&
              f.nodes.ltop + f.nodes.d == 11, "full area");
    CHECK(eval_bits_form(5, npts, stop, logN, fb - 1, cus, knobs, &f) && f.L == 0, "area one byte short");
    CHECK(eval_bits_form(5, npts, stop, logN, 0, cus, knobs, &f) && f.L == 0, "no area");
    CHECK(eval_bits_form(5, npts, 57, 64, ~0ull, cus, knobs, &f) && f.L == 0, "logN > 63");
    CHECK(eval_bits_form(5, 31, stop, logN, ~0ull, cus, knobs, &f) && f.L == 0, "too few points for L >= 4");
    CHECK(eval_bits_form(5, 32, stop, logN, ~0ull, cus, knobs, &f) && f.L == 4, "L = 4");
    TreeKnobs plain;
    plain.eval_plain = true;
    CHECK(eval_bits_form(5, npts, stop, logN, fb, cus, plain, &f) && f.L == 0, "DPF_EVAL_MODE=plain");
    CHECK(eval_bits_stride(0) == 0 && eval_bits_stride(1) == 16 && eval_bits_stride(128) == 16 &&
              eval_bits_stride(129) == 32, "stride");
}

int main() {
    const uint64_t npts[] = {1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, (1ull << 20) + 1};
    const uint64_t nkeys[] = {1, 3, 64, 65, 4097};
    const uint64_t cus[] = {4, 64, 256};
    for (uint64_t n : npts)
        for (uint64_t k : nkeys)
            for (uint64_t c : cus) replay(k, n, c, 40);
    replay(3, 300, 256, 7);    // stop 0
    replay(3, 300, 256, 63);
    limits();
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("eval_bits_plan ok\n");
    return 0;
}
