// pir_any_plan_test.cpp — the launch plans for records of any width (a
// multiple of 4 bytes) over the sliced layout, as a stand-alone program:
// dpf-go_amd/csrc/pir_fold_plan.hpp and pir_scatter_plan.hpp.  A record is
// T = rec_bytes / 4 bit tiles in C = ceil(T / 8) columns, the last of which may
// be short.  The kernels give a workgroup whole columns and skip the tiles a
// record does not have (dpfh::tile_exists); this program walks every plan with
// that rule and checks, over widths x nrec x limits x CU counts, that
//   - every existing (super-group, tile) cell is covered exactly once by the
//     matrix-core fold's, the one-key fold's and the private write's plans,
//     and lies inside the buffer (sliced_bytes_any);
//   - the tiles skipped at the last super-group are exactly those that would
//     lie past the buffer (so skipping is not optional), and nothing else is;
//   - a pass reads its DB from byte S0 * 256 * rec_bytes;
//   - the first launch clears nkeys * T answer words;
//   - for multiples of 32 the plans and the arithmetic are those from before
//     records of any width.
// Built with -fsanitize=address,undefined and run directly by
// tests/test_any_plan_cpu.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pir_fold_plan.hpp"
#include "pir_scatter_plan.hpp"

using namespace dpfh;

static int g_fail = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (++g_fail <= 20) {                          \
                printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
                printf(__VA_ARGS__);                       \
                printf("\n");                              \
            }                                              \
        }                                                  \
    } while (0)

typedef unsigned long long ull;
static uint64_t g_plans = 0, g_cells = 0;

// The cells of one DB: a counter per (super-group, tile), and the buffer's end.
struct Cells {
    uint64_t rec, nsg, T, bytes;
    std::vector<uint8_t> cnt;
    Cells(uint64_t nrec, uint64_t rec_bytes)
        : rec(rec_bytes), nsg((nrec + 255) / 256), T(rec_tiles(rec_bytes)), bytes(sliced_bytes_any(nrec, rec_bytes)),
          cnt(nsg * T) {}
    // A workgroup is given column c of super-group S (S absolute; base: the
    // byte offset its launch's DB pointer starts at, S_rel: S from there).
    void column(uint64_t S, uint64_t S_rel, uint64_t base, uint32_t c) {
        CHECK(S < nsg && c < rec_cols(rec), "S=%llu c=%u", (ull)S, c);
        if (S >= nsg || c >= rec_cols(rec)) return;
        CHECK(col_tiles(rec, c) >= 1 && col_tiles(rec, c) <= 8 && col_rows(rec, c) == 32 * col_tiles(rec, c), "c=%u", c);
        for (uint32_t i = 0; i < 8; ++i) {
            const uint64_t tile = 8ull * c + i;
            const uint64_t end = base + tile_off_bytes(rec, S_rel, tile) + 1024;
            CHECK(base + tile_off_bytes(rec, S_rel, tile) == tile_off_bytes(rec, S, tile), "pass offset");
            if (tile_exists(rec, tile)) {
                CHECK(i < col_tiles(rec, c), "tile %llu of column %u", (ull)tile, c);
                CHECK(end <= bytes, "rec=%llu S=%llu tile=%llu past the buffer", (ull)rec, (ull)S, (ull)tile);
                if (cnt[S * T + tile] < 255) ++cnt[S * T + tile];
            } else {
                CHECK(i >= col_tiles(rec, c), "tile %llu of column %u", (ull)tile, c);
                // An absent tile's rows are a later super-group's, or past the end: always at the last one.
                CHECK(end > tile_off_bytes(rec, S + 1, 0), "rec=%llu S=%llu tile=%llu", (ull)rec, (ull)S, (ull)tile);
                if (S + 1 == nsg) CHECK(end > bytes, "rec=%llu S=%llu tile=%llu", (ull)rec, (ull)S, (ull)tile);
            }
        }
    }
    void once(const char* what) {
        g_cells += cnt.size();
        for (uint64_t i = 0; i < cnt.size(); ++i)
            if (cnt[i] != 1) {
                CHECK(cnt[i] == 1, "%s: rec=%llu cell (S=%llu, tile=%llu) covered %u times", what, (ull)rec, (ull)(i / T),
                      (ull)(i % T), cnt[i]);
                break;
            }
        std::fill(cnt.begin(), cnt.end(), (uint8_t)0);
    }
};

// A fold plan walked as the launchers do: cols_per_y columns per grid row.
static void walk_fold(const SlicedFoldPlan& p, Cells& cells, uint32_t cols_per_y, uint64_t clear_words, const char* what) {
    ++g_plans;
    uint64_t n_launch = 0;
    p.for_each_launch([&](const FoldLaunch& l) {
        CHECK(l.db_off == l.S0 * 256 * cells.rec, "%s: db_off=%llu S0=%llu rec=%llu", what, (ull)l.db_off, (ull)l.S0,
              (ull)cells.rec);
        CHECK(l.sel_off == 8 * l.S0, "%s: sel_off", what);
        CHECK(l.clear_words == (n_launch == 0 ? clear_words : 0), "%s: clear_words=%llu", what, (ull)l.clear_words);
        CHECK(l.blocks >= 1 && (l.blocks - 1) * l.spb < l.n && l.blocks * l.spb >= l.n, "%s: empty workgroup", what);
        for (uint64_t x = 0; x < l.blocks; ++x)
            for (uint64_t s = x * l.spb; s < l.n && s < (x + 1) * l.spb; ++s)
                for (uint64_t y = 0; y < l.gy; ++y)
                    for (uint32_t cw = 0; cw < cols_per_y; ++cw)
                        cells.column(l.S0 + s, s, l.db_off, (uint32_t)((l.g0 + y) * cols_per_y + cw));
        ++n_launch;
        return 0;
    });
    cells.once(what);
}

static bool same_launches(const SlicedFoldPlan& a, const SlicedFoldPlan& b) {
    std::vector<FoldLaunch> la, lb;
    a.for_each_launch([&](const FoldLaunch& l) { la.push_back(l); return 0; });
    b.for_each_launch([&](const FoldLaunch& l) { lb.push_back(l); return 0; });
    if (la.size() != lb.size()) return false;
    for (size_t i = 0; i < la.size(); ++i) {
        const FoldLaunch &x = la[i], &y = lb[i];
        if (x.g0 != y.g0 || x.gy != y.gy || x.S0 != y.S0 || x.n != y.n || x.blocks != y.blocks || x.spb != y.spb ||
            x.sel_off != y.sel_off || x.db_off != y.db_off || x.clear_words != y.clear_words)
            return false;
    }
    return true;
}

static void check_width(uint64_t rec, uint64_t nrec, uint32_t max_blocks, uint32_t max_sg, uint32_t cus) {
    CHECK(rec_bytes_any_ok(rec), "rec=%llu", (ull)rec);
    const uint32_t C = rec_cols(rec), T = rec_tiles(rec);
    const uint64_t nsg = (nrec + 255) / 256;
    CHECK(C == (T + 7) / 8 && T == rec / 4 && sg_stride_bytes(rec) == 1024ull * T, "rec=%llu", (ull)rec);
    uint64_t rows = 0;
    for (uint32_t c = 0; c < C; ++c) rows += col_rows(rec, c);
    CHECK(rows == 8 * rec, "rows of rec=%llu", (ull)rec);
    CHECK(sliced_bytes_any(nrec, rec) == nsg * 256 * rec, "size");
    if (nsg == 0) return;
    const FoldLimits lim = clamp_fold_limits(max_blocks, max_sg);
    Cells cells(nrec, rec);
    const uint32_t nkeys = 17;

    // The matrix-core fold: every tile shape the launcher can pick for this width.
    const int cg = fold_cg(C, FoldKnobs{}.wide_cg);
    CHECK(C % (uint32_t)cg == 0, "cg=%d C=%u", cg, C);
    for (uint32_t nk : {2u, 33u, 65u, 129u, 256u}) {
        const FoldTile& t = kFoldTiles[fold_tile_index(nk, cg)];
        CHECK(C % (uint32_t)t.CG == 0, "tile CG=%d C=%u", t.CG, C);
        for (int occ = 1; occ <= 3; occ += 2) {
            const bool ntdb = fold_ntdb_any(nsg, rec, FoldKnobs{}.nt_min);
            const uint64_t resident = cus * fold_per_cu(C, t.MT, ntdb, fold_db_bytes_any(nsg, rec), occ, 0);
            const uint64_t cw = fold_clear_words_any(nkeys, rec, 0);
            CHECK(cw == (uint64_t)nkeys * T && fold_clear_words_any(nkeys, rec, 256) == 0, "clear words");
            const SlicedFoldPlan p = plan_fold_mfma(nsg, C, t, lim, resident, cw, rec);
            walk_fold(p, cells, (uint32_t)t.CG, cw, "mfma");
            if (rec % 32 == 0) {
                CHECK(fold_db_bytes_any(nsg, rec) == fold_db_bytes(nsg, C) && cw == fold_clear_words(nkeys, C, 0) &&
                          ntdb == fold_ntdb(nsg, C, FoldKnobs{}.nt_min),
                      "rec=%llu: the arithmetic of a multiple of 32", (ull)rec);
                CHECK(same_launches(p, plan_fold_mfma(nsg, C, t, lim, resident, cw)), "rec=%llu: mfma plan changed", (ull)rec);
            }
        }
    }
    // The one-key fold: a column per grid row.
    {
        const SlicedFoldPlan p = plan_fold_sliced_direct(nsg, C, lim, cus, rec);
        walk_fold(p, cells, 1, T, "direct");
        if (rec % 32 == 0)
            CHECK(same_launches(p, plan_fold_sliced_direct(nsg, C, lim, cus)), "rec=%llu: direct plan changed", (ull)rec);
    }
    // The private write: units of (run, column group) per key tile.
    for (uint64_t nk : {3ull, 70ull}) {
        const ScatterPlan p = plan_scatter(nrec, C, nk, cus, max_blocks, max_sg);
        ++g_plans;
        CHECK(p.key_tiles() == (nk + kScatterKeyTile - 1) / kScatterKeyTile && p.cols <= kScatterMaxCols, "scatter plan");
        for (uint64_t tile = 0; tile < p.key_tiles(); ++tile) {
            for (uint64_t l = 0; l < p.launches(); ++l)
                for (uint64_t b = 0; b < p.blocks(l); ++b) {
                    const ScatterUnit u = p.unit(tile, p.first(l) + b);
                    CHECK(u.s0 < u.s1 && u.s1 <= nsg && u.c0 < u.c1 && u.c1 <= C, "scatter unit");
                    for (uint64_t S = u.s0; S < u.s1; ++S)
                        for (uint32_t c = u.c0; c < u.c1; ++c) cells.column(S, S, 0, c);
                }
            cells.once("scatter");
        }
    }
    // The update's grid: whole columns per chunk.
    {
        const UpdatePlan up = plan_update_sliced(100, nsg, C);
        CHECK(up.grid(100, C) % C == 0 && up.grid(100, C) / C >= up.chunks(100), "update grid");
    }
}

int main() {
    const uint64_t widths[] = {4, 8, 12, 16, 20, 28, 32, 36, 48, 64, 96, 100, 128, 132, 160, 260, 288, 1024, 1028, 32768};
    const uint64_t nrecs[] = {0, 1, 255, 256, 257, 1000, 5000, 70001};
    const uint32_t limits[][2] = {{0, 0}, {3, 2}, {1, 1}, {7, 5}, {1024, 4}};
    const uint32_t cus[] = {1, 8, 256};
    for (uint64_t rec : widths)
        for (uint64_t nrec : nrecs) {
            if (rec >= 1024 && nrec > 5000) continue;          // keeps the walk short
            for (const auto& lim : limits)
                for (uint32_t cu : cus) check_width(rec, nrec, lim[0], lim[1], cu);
        }
    // The width rule.
    for (uint64_t rec : {0ull, 2ull, 6ull, 33ull, 32772ull}) CHECK(!rec_bytes_any_ok(rec), "rec=%llu", (ull)rec);
    for (uint64_t rec = 0; rec <= 33000; ++rec)
        if (rec_bytes_ok(rec)) CHECK(rec_bytes_any_ok(rec) && rec_tiles(rec) == 8 * rec_cols(rec), "rec=%llu", (ull)rec);
    // One large shape by arithmetic alone: 2^24 records of 16 bytes.
    {
        const uint64_t nsg = 1ull << 16;
        const SlicedFoldPlan p = plan_fold_mfma(nsg, 1, kFoldTiles[3], clamp_fold_limits(0, 0), 256, 64 * 4, 16);
        uint64_t covered = 0;
        p.for_each_launch([&](const FoldLaunch& l) {
            CHECK(l.db_off == l.S0 * 4096, "db_off at 16 bytes");
            covered += l.n;
            return 0;
        });
        CHECK(covered == nsg, "2^24 x 16 B covered");
    }
    if (g_fail) {
        printf("pir_any_plan: %d failure(s)\n", g_fail);
        return 1;
    }
    printf("pir_any_plan ok: %llu plans, %llu cells\n", (ull)g_plans, (ull)g_cells);
    return 0;
}
