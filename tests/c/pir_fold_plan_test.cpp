// pir_fold_plan_test.cpp — the fold's launch plans
// (dpf-go_amd/csrc/pir_fold_plan.hpp) as a stand-alone program.  Over a grid of
// shapes and limits every plan covers its cells exactly once, launches no
// empty workgroup, keeps each launch inside the workgroup cap, the per-workgroup
// bound and the partials area, clears the answers in the first launch only and
// puts each pass where its super-groups are; and the tuned defaults at the
// benchmark's shape are the ones recorded below.  Built with
// -fsanitize=address,undefined and run directly by tests/test_fold_plan_cpu.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pir_fold_plan.hpp"

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
static uint64_t g_plans = 0, g_launches = 0;

// ---- the folds over the sliced DB -------------------------------------------
// sg: the plan's granule (a tile shape's SG; 2 for the one-key fold); msg_max:
// the bound on a run (UINT64_MAX: none); part: bytes of a workgroup's partial
// per column group.  Returns the number of launches that clear the answers.
static int check_sliced(const SlicedFoldPlan& p, uint64_t nsg, uint32_t C, uint64_t ncg, uint64_t cap, uint64_t sg,
                        uint64_t msg_max, uint64_t part, uint64_t clear_words) {
#define AT "nsg=%llu C=%u ncg=%llu cap=%llu sg=%llu msg=%llu res=%llu", (ull)nsg, C, (ull)ncg, (ull)cap, (ull)sg, (ull)msg_max, (ull)p.resident
    ++g_plans;
    // A counter per (super-group, column group) where that stays small; always the walk.
    const bool exhaustive = nsg * ncg <= (1u << 14);
    std::vector<uint8_t> cnt(exhaustive ? nsg * ncg : 0);
    uint64_t g_at = 0, g_end = 0, s_at = nsg, n_launch = 0;   // s_at == nsg: "column groups [g_at, g_end) finished"
    int clears = 0;
    p.for_each_launch([&](const FoldLaunch& l) {
        ++g_launches;
        if (s_at == nsg) {                                     // the next column groups start at super-group 0
            CHECK(l.g0 == g_end && l.S0 == 0, AT);
            g_at = l.g0;
            g_end = l.g0 + l.gy;
        } else {                                               // the next pass of the same column groups
            CHECK(l.g0 == g_at && l.g0 + l.gy == g_end && l.S0 == s_at, AT);
        }
        CHECK(l.gy >= 1 && l.g0 + l.gy <= ncg, AT);
        CHECK(l.n >= 1 && l.S0 + l.n <= nsg, AT);
        s_at = l.S0 + l.n;
        // Per-launch bounds.
        CHECK(l.blocks >= 1 && l.blocks * l.gy <= cap, AT);
        CHECK(l.spb >= 1 && l.spb % sg == 0 && l.spb <= msg_max, AT);
        CHECK(msg_max == UINT64_MAX || l.spb <= kFoldMaxSg, AT);
        CHECK(l.blocks * l.gy * part <= kFoldPartsBytes, AT);
        // Workgroup x folds [S0 + x spb, min(S0 + n, + spb)): the last one is
        // not empty (so none is) and reaches the end of the pass.
        CHECK((l.blocks - 1) * l.spb < l.n && l.blocks * l.spb >= l.n, AT);
        // Clearing and pass offsets.
        CHECK(l.clear_words == (n_launch == 0 ? clear_words : 0), AT);
        clears += l.clear_words != 0;
        CHECK(l.sel_off == 8 * l.S0 && l.db_off == l.S0 * 256 * 32 * C, AT);
        CHECK(l.wlim(8 * nsg) == 8 * (nsg - l.S0) && l.wlim(8 * l.S0) == 0 && l.wlim(0) == 0, AT);
        if (exhaustive)
            for (uint64_t x = 0; x < l.blocks; ++x)
                for (uint64_t S = l.S0 + x * l.spb; S < l.S0 + l.n && S < l.S0 + (x + 1) * l.spb; ++S)
                    for (uint64_t g = l.g0; g < l.g0 + l.gy; ++g)
                        if (S < nsg && g < ncg && cnt[S * ncg + g] < 255) ++cnt[S * ncg + g];
        ++n_launch;
        return 0;
    });
    CHECK(n_launch >= 1 && s_at == nsg && g_end == ncg, AT);
    for (uint64_t i = 0; i < cnt.size(); ++i)
        if (cnt[i] != 1) {
            CHECK(cnt[i] == 1, AT);
            break;
        }
#undef AT
    return clears;
}

// The launches a plan would make under these limits, from its inputs alone:
// shapes over this stay with the default limits.
static uint64_t launches_bound(uint64_t nsg, uint64_t ncg, uint64_t cap, uint64_t msg) {
    const uint64_t gy = ncg < cap ? ncg : cap, per_pass = cap / gy * msg;
    return (ncg + gy - 1) / gy * ((nsg + per_pass - 1) / per_pass);
}
constexpr uint64_t kMaxLaunches = 1u << 8;

static void check_mfma(uint64_t nsg, uint32_t C, const FoldTile& t, uint32_t max_blocks, uint32_t max_sg, uint64_t cus,
                       int occ) {
    if (C % (uint32_t)t.CG != 0) return;                       // fold_cg never pairs them
    const FoldLimits lim = clamp_fold_limits(max_blocks, max_sg);
    const uint64_t sg = (uint64_t)t.SG;
    // max_sg rounded down to a multiple of SG, or SG itself where max_sg < SG.
    const uint64_t msg = lim.max_sg >= sg ? lim.max_sg / sg * sg : sg;
    const uint64_t ncg = C / (uint32_t)t.CG;
    const bool defaults = max_blocks == 0 && max_sg == 0;
    if (!defaults && launches_bound(nsg, ncg, lim.max_blocks, msg) > kMaxLaunches) return;
    for (int knob = 0; knob <= (C == 1 ? 1 : 0); ++knob) {   // DPF_FOLD_PER_CU: read at C = 1 only
        const bool ntdb = fold_ntdb(nsg, C, FoldKnobs{}.nt_min);
        const uint64_t per_cu = fold_per_cu(C, t.MT, ntdb, fold_db_bytes(nsg, C), occ, knob);
        CHECK(per_cu >= 1 && per_cu <= (uint64_t)occ, "per_cu=%llu occ=%d", (ull)per_cu, occ);
        const uint64_t cw = fold_clear_words(17, C, 0);
        const SlicedFoldPlan p = plan_fold_mfma(nsg, C, t, lim, cus * per_cu, cw);
        CHECK(check_sliced(p, nsg, C, ncg, lim.max_blocks, sg, msg, 32ull * t.MT * 32 * t.CG, cw) == 1, "one clearing launch");
    }
}

static void check_sliced_direct(uint64_t nsg, uint32_t C, uint32_t max_blocks, uint32_t max_sg, uint64_t cus) {
    const FoldLimits lim = clamp_fold_limits(max_blocks, max_sg);
    if ((max_blocks || max_sg) && launches_bound(nsg, C, lim.max_blocks, nsg) > kMaxLaunches) return;
    const SlicedFoldPlan p = plan_fold_sliced_direct(nsg, C, lim, cus);
    CHECK(check_sliced(p, nsg, C, C, lim.max_blocks, 2, UINT64_MAX, 32, 8ull * C) == 1, "one clearing launch");
}

// A whole call: key groups of kFoldKeyGroup cover nkeys, each group's tile
// shape holds its keys and divides C, and of all the call's launches exactly
// the first clears, and clears every answer word.
static void check_call(uint32_t nkeys, uint32_t C, uint64_t nsg, int wide_cg) {
    const int cg = fold_cg(C, wide_cg);
    CHECK((cg == 1 || cg == 2 || cg == 4) && C % (uint32_t)cg == 0 && cg <= (wide_cg < 1 ? 1 : wide_cg), "cg=%d C=%u", cg, C);
    uint32_t covered = 0;
    int clears = 0, groups = 0;
    for (uint32_t k0 = 0; k0 < nkeys; k0 += kFoldKeyGroup, ++groups) {
        const uint32_t nk = nkeys - k0 < kFoldKeyGroup ? nkeys - k0 : kFoldKeyGroup;
        CHECK(k0 == covered && nk >= 1, "key groups");
        covered += nk;
        const int ti = fold_tile_index(nk, cg);
        CHECK(ti >= 0 && ti < kFoldTileCount, "tile index %d", ti);
        const FoldTile& t = kFoldTiles[ti];
        CHECK(32u * (uint32_t)t.MT >= nk && C % (uint32_t)t.CG == 0 && t.CG <= cg, "nk=%u C=%u cg=%d tile %d", nk, C, cg, ti);
        CHECK(8 % t.NT == 0 && 32ull * t.MT * 32 * t.CG <= kFoldPartBytes, "tile %d", ti);
        const uint64_t cw = fold_clear_words(nkeys, C, k0);
        CHECK(cw == (k0 == 0 ? (uint64_t)nkeys * 8 * C : 0), "clear words");
        const SlicedFoldPlan p = plan_fold_mfma(nsg, C, t, clamp_fold_limits(3, 4), 8, cw);
        bool first = true;
        p.for_each_launch([&](const FoldLaunch& l) {
            CHECK((l.clear_words != 0) == (first && k0 == 0), "nkeys=%u C=%u k0=%u", nkeys, C, k0);
            clears += l.clear_words != 0;
            first = false;
            return 0;
        });
    }
    CHECK(covered == nkeys && clears == 1 && groups == (int)((nkeys + 255) / 256), "nkeys=%u", nkeys);
}

// ---- the row-major folds -----------------------------------------------------
static void check_rows(uint64_t nchunks, uint64_t cus, uint32_t max_blocks) {
    const uint64_t cap = clamp_fold_limits(max_blocks, 0).max_blocks;
#define AT "nchunks=%llu cus=%llu cap=%llu", (ull)nchunks, (ull)cus, (ull)cap
    // k_fold_direct: workgroup b takes [b cpb, min(nchunks, + cpb)).
    const ChunkSplit d = plan_fold_direct(nchunks, cus, cap);
    CHECK(d.blocks >= 1 && d.blocks <= cap && d.blocks <= 4 * cus, AT);
    CHECK(d.cpb % kFoldDirectGran == 0 && (d.blocks - 1) * d.cpb < nchunks && d.blocks * d.cpb >= nchunks, AT);
    CHECK(d.blocks * (uint64_t)kFoldDirectMaxKeys * 32 * 8 <= kFoldPartsBytes, AT);
    // k_fold4r, with the kernel's own c0 / my.
    for (int wv : {4, 8})
        for (int skew : {-1, 0, 50, 51, 62, 75, 90, 99, 100, 1000}) {
            const Fold4rLaunch l = plan_fold4r(nchunks, wv, cus, cap, skew);
            const uint64_t gran = 2 * (uint64_t)wv;
            CHECK(l.blocks >= 1 && l.blocks <= cap && l.blocks <= fold4r_per_cu(wv) * cus, AT);
            CHECK(l.cpb >= gran && l.cpb % gran == 0 && l.cpb_first >= gran && l.cpb_first % gran == 0, AT);
            CHECK(l.nfirst == 0 || (wv == 8 && skew > 50 && skew < 100 && l.nfirst == cus && l.blocks == 2 * cus &&
                                    l.cpb_first >= l.cpb),
                  AT);
            CHECK(l.blocks * kFoldPartBytes <= kFoldPartsBytes, AT);
            uint64_t at = 0;
            for (uint64_t b = 0; b < l.blocks; ++b) {
                const uint64_t c0 = b < l.nfirst ? b * l.cpb_first : l.nfirst * l.cpb_first + (b - l.nfirst) * l.cpb;
                const uint64_t my = b < l.nfirst ? l.cpb_first : l.cpb;
                const uint64_t cend = c0 + my < nchunks ? c0 + my : nchunks;
                if (c0 < cend) {
                    CHECK(c0 == at, "wv=%d skew=%d b=%llu nchunks=%llu cus=%llu", wv, skew, (ull)b, (ull)nchunks, (ull)cus);
                    at = cend;
                } else {
                    CHECK(at == nchunks, "wv=%d skew=%d b=%llu nchunks=%llu cus=%llu", wv, skew, (ull)b, (ull)nchunks, (ull)cus);
                }
            }
            CHECK(at == nchunks, "wv=%d skew=%d nchunks=%llu cus=%llu cap=%llu", wv, skew, (ull)nchunks, (ull)cus, (ull)cap);
        }
#undef AT
}

static void check_plan_fold() {
    for (uint64_t rec : {32, 64, 96, 128, 160, 256, 1024})
        for (uint32_t nk : {1, 4, 5, 16, 17, 64, 65, 128, 129, 256, 300}) {
            const FoldPlan p = plan_fold(rec, nk);
#define AT "rec=%llu nk=%u", (ull)rec, nk
            CHECK((uint64_t)p.cols * p.col_passes == rec / 32, AT);
            CHECK(p.cols == 1 || p.cols == 2 || p.cols == 4 || p.cols == 8, AT);
            if (p.direct) {
                // Key slots of k_fold_direct<C, KB>: KB = 1, 4 or 16 holds the pass's keys.
                CHECK(p.kw == 0 && p.keys_per_pass == kFoldDirectMaxKeys, AT);
                const uint32_t pass = nk < p.keys_per_pass ? nk : p.keys_per_pass, kb = fold_direct_slots(pass);
                CHECK((kb == 1 || kb == 4 || kb == 16) && kb >= pass, AT);
                CHECK(nk <= 4 || (p.cols >= 2 && nk <= kFoldDirectMaxKeys), AT);
            } else {
                // k_fold4r<C, KW, WV>: 64 KW key lanes; KW * C <= 8 accumulator columns (the instantiated ones).
                CHECK((p.kw == 1 || p.kw == 2 || p.kw == 4) && p.keys_per_pass == 64 * p.kw, AT);
                CHECK(p.kw == 1 || 64 * (p.kw / 2) < nk, AT);              // no wider than the keys need
                CHECK(64ull * p.kw * 32 * p.cols <= kFoldPartBytes, AT);
            }
            CHECK(p.kw * p.cols <= 8, AT);
            CHECK(fold4r_waves((int)p.cols, (int)p.kw) == (p.kw == 1 && p.cols < 8 ? 8 : 4), AT);
#undef AT
        }
}

// ---- the maintenance launches ------------------------------------------------
static void check_spans() {
    for (uint64_t C : {1, 2, 3, 5, 32, 1024}) {
        CHECK(rec_bytes_ok(32 * C), "C=%llu", (ull)C);
        CHECK(slice_db_span(C) >= 1 && slice_db_span(C) * C <= (1ull << 30), "C=%llu", (ull)C);
        for (uint64_t per_rec : {2 * C, 8 * C}) {
            const uint64_t m = record_span(per_rec);
            CHECK(m >= 1 && (m * per_rec + 255) / 256 <= (1ull << 30), "per_rec=%llu", (ull)per_rec);
        }
        for (uint64_t nsg : {1ull, 3ull, 4097ull, 1ull << 16})
            for (uint64_t n : {1ull, 7ull, 64ull, 1000ull, 1ull << 20, (1ull << 31) + 5, 1ull << 36}) {
                const UpdatePlan p = plan_update_sliced(n, nsg, C);
#define AT "n=%llu nsg=%llu C=%llu K=%u", (ull)n, (ull)nsg, (ull)C, p.K
                CHECK(p.K >= 1 && p.K <= 64 && (p.K & (p.K - 1)) == 0, AT);
                CHECK(p.K == 1 || 2ull * (p.K / 2) <= n / nsg, AT);
                CHECK(p.K == 64 || 2ull * p.K > n / nsg, AT);
                uint64_t at = 0;
                for_each_span(n, p.span, [&](uint64_t i0, uint64_t m) {
                    CHECK(i0 == at && m >= 1 && i0 % p.K == 0, AT);
                    at = i0 + m;
                    const uint64_t chunks = p.chunks(m), grid = p.grid(m, C);
                    CHECK(chunks * p.K >= m && (chunks - 1) * p.K < m && chunks <= UINT32_MAX, AT);
                    CHECK(grid <= (1ull << 30) && grid % C == 0 && grid / C % 8 == 0 && grid / C >= chunks &&
                              grid / C < chunks + 8,
                          AT);
                    return 0;
                });
                CHECK(at == n, AT);
#undef AT
            }
    }
    for (uint64_t rec : {0, 16, 48, 32800, 32768 + 32}) CHECK(!rec_bytes_ok(rec), "rec=%llu", (ull)rec);
    CHECK(rec_bytes_ok(kFoldMaxRecBytes), "widest record");
    uint64_t at = 0;
    CHECK(for_each_span(10, 4, [&](uint64_t i0, uint64_t m) { return at += m, i0 == 8 ? 7 : 0; }) == 7 && at == 10, "spans");
    CHECK(for_each_span(0, 4, [&](uint64_t, uint64_t) { return 1; }) == 0, "no span of nothing");
}

// ---- the tuned defaults, as the parent of this header launched them ----------
// The benchmark's DB (2^24 records of 32 B, 256 CUs, default limits): the
// matrix-core fold's one launch.  Worked out from the launcher that preceded
// this header (its launch_mfma, split_chunks and fold_per_cu), not from the
// header.  occ is the shape's occupancy as the runtime reports it.
struct Pinned {
    uint32_t nkeys;
    int occ;
    uint64_t blocks, spb;
    bool ntdb;
    uint64_t per_cu;
};
static const Pinned kPinned[] = {
    {64, 2, 512, 128, true, 2},
    {64, 3, 763, 86, true, 3},
    {256, 2, 512, 128, true, 2},
    {256, 3, 745, 88, true, 3},
};

static void check_pinned() {
    const uint64_t nsg = (1ull << 24) / 256, cus = 256;
    const FoldKnobs knobs;
    CHECK(knobs.skew == 62 && knobs.nt_min == (256ull << 20) && knobs.per_cu == 0 && knobs.wide_cg == 4 && knobs.xor_ys == 0,
          "default knobs");
    for (const Pinned& v : kPinned) {
        const FoldTile& t = kFoldTiles[fold_tile_index(v.nkeys, fold_cg(1, knobs.wide_cg))];
        const bool ntdb = fold_ntdb(nsg, 1, knobs.nt_min);
        const uint64_t per_cu = fold_per_cu(1, t.MT, ntdb, fold_db_bytes(nsg, 1), v.occ, knobs.per_cu);
        int n = 0;
        plan_fold_mfma(nsg, 1, t, clamp_fold_limits(0, 0), cus * per_cu, 0).for_each_launch([&](const FoldLaunch& l) {
            CHECK(l.blocks == v.blocks && l.spb == v.spb && l.gy == 1 && l.n == nsg, "nkeys=%u occ=%d: blocks=%llu spb=%llu",
                  v.nkeys, v.occ, (ull)l.blocks, (ull)l.spb);
            ++n;
            return 0;
        });
        CHECK(n == 1 && ntdb == v.ntdb && per_cu == v.per_cu, "nkeys=%u occ=%d: ntdb=%d per_cu=%llu", v.nkeys, v.occ, ntdb,
              (ull)per_cu);
    }
    // The same DB through the row-major folds and the partials' reduction.
    const Fold4rLaunch l = plan_fold4r(1ull << 18, 8, cus, 1024, knobs.skew);
    CHECK(l.blocks == 512 && l.nfirst == 256 && l.cpb_first == 640 && l.cpb == 384, "k_fold4r at the benchmark's shape");
    CHECK(xor_parts_ys(512, 0) == 64 && xor_parts_ys(256, 0) == 16 && xor_parts_ys(5, 0) == 5 && xor_parts_ys(512, 8) == 8,
          "k_xor_parts slices");
    CHECK(kFoldMaxBlocks == 1024 && kFoldMaxSg == 1u << 15 && kFoldPartBytes == 16384, "limits");
    const FoldLimits a = clamp_fold_limits(0, 0), b = clamp_fold_limits(5000, 1u << 20), c = clamp_fold_limits(3, 5);
    CHECK(a.max_blocks == 1024 && a.max_sg == 1u << 15 && b.max_blocks == 1024 && b.max_sg == 1u << 15 && c.max_blocks == 3 &&
              c.max_sg == 5,
          "clamp");
}

int main() {
    const uint32_t caps[] = {1, 2, 3, 5, 7, 64, 1024};
    const uint32_t sgs[] = {0, 1, 2, 3, 4, 5, 7};
    const uint64_t cuss[] = {1, 8, 256};
    const uint32_t Cs[] = {1, 2, 3, 4, 5, 8, 12, 32, 1024};
    const uint64_t nsgs[] = {1, 2, 3, 4, 5, 7, 8, 9, 31, 33, 40, 117, 256, 1000, 4097};
    for (uint64_t nsg : nsgs)
        for (uint32_t C : Cs)
            for (uint32_t cap : caps)
                for (uint32_t sg : sgs)
                    for (uint64_t cus : cuss) {
                        for (const FoldTile& t : kFoldTiles)
                            for (int occ = 1; occ <= 4; ++occ) check_mfma(nsg, C, t, cap, sg, cus, occ);
                        check_sliced_direct(nsg, C, cap, sg, cus);
                    }
    // The default limits: the same shapes, and DBs past one pass (3 2^15 + 5
    // super-groups) and past 2^24 records per key tile row (2^20 + 2^13).
    for (uint64_t nsg : {1ull, 9ull, 4097ull, 3ull * (1u << 15) + 5, (1ull << 20) + (1ull << 13)})
        for (uint32_t C : Cs)
            for (uint64_t cus : cuss) {
                for (const FoldTile& t : kFoldTiles)
                    for (int occ = 1; occ <= 4; ++occ) check_mfma(nsg, C, t, 0, 0, cus, occ);
                check_sliced_direct(nsg, C, 0, 0, cus);
            }
    for (uint32_t nkeys : {1, 2, 32, 33, 64, 65, 128, 129, 256, 257, 300, 513})
        for (uint32_t C : Cs)
            for (int wide_cg : {1, 2, 3, 4, 8}) check_call(nkeys, C, 9, wide_cg);
    for (uint64_t nchunks : {1ull, 2ull, 7ull, 8ull, 9ull, 15ull, 16ull, 17ull, 100ull, 511ull, 512ull, 513ull, 4096ull,
                             8191ull, 1ull << 18, (1ull << 18) + 1, (1ull << 26) + 3})
        for (uint64_t cus : cuss)
            for (uint32_t cap : {1, 2, 3, 5, 7, 64, 1024, 0}) check_rows(nchunks, cus, cap);
    check_plan_fold();
    check_spans();
    check_pinned();
    if (g_fail) {
        printf("pir_fold_plan: %d failures\n", g_fail);
        return 1;
    }
    printf("pir_fold_plan ok (%llu sliced plans, %llu launches)\n", (ull)g_plans, (ull)g_launches);
    return 0;
}
