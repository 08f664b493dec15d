// pir_fold_plan.hpp — the host arithmetic behind every fold launch: how many
// workgroups a launch has, how long a workgroup's run is, how many passes a
// fold takes under dpf_set_fold_limits, where a pass starts, which launch
// clears the answers, and the grid chunking of the resident DB's maintenance
// launches.  Pure functions of (shape, CU count, limits, knobs); host-only and
// header-only (no HIP), so tests/c/pir_fold_plan_test.cpp runs them under
// ASan/UBSan without a device.  The launchers (pir_fold_rows.hip,
// pir_fold_sliced.hip, pir_db_ops.hip) walk a plan and launch.
//
// What a plan guarantees, and no kernel can check:
//   - a k_fold_mfma workgroup folds at most kFoldMaxSg super-groups (its fp32
//     counts are exact only up to 2^24);
//   - no workgroup of a sliced fold launch has an empty run (it would return
//     before writing its partial, which k_xor_parts still reads);
//   - a launch's partials fit pir_fold_parts_bytes();
//   - every (super-group, column) cell is folded exactly once.
//
// A public fold call takes one snapshot of the limits (FoldLimits) and plans
// all its launches from it; a dpf_set_fold_limits that runs concurrently with
// a call therefore applies to that call wholly or not at all, where it could
// once apply to part of it.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dpfh {

// ---- limits (dpf_set_fold_limits) and measurement knobs --------------------
constexpr uint64_t kFoldMaxBlocks = 1024;            // workgroups per launch (the partials area)
constexpr uint32_t kFoldMaxSg = 1u << 15;            // super-groups per k_fold_mfma workgroup: 2^23 records
constexpr uint64_t kFoldPartBytes = 64 * 4 * 32 * 2; // a workgroup's partial: 64*KW keys x 32C bytes, KW*C <= 8
constexpr uint64_t kFoldPartsBytes = kFoldMaxBlocks * kFoldPartBytes;
constexpr uint64_t kFoldMaxRecBytes = 32768;         // widest record of the sliced DB
constexpr uint32_t kFoldKeyGroup = 256;              // keys per matrix-core fold (8 key tiles)
constexpr uint32_t kFoldDirectMaxKeys = 16;          // key slots of k_fold_direct
constexpr uint64_t kFoldDirectGran = 8;              // chunks per k_fold_direct round: two per wave

struct FoldLimits {
    uint32_t max_blocks, max_sg;
};
// 0 = the default; larger values are cut to it.
inline FoldLimits clamp_fold_limits(uint32_t max_blocks, uint32_t max_sg) {
    return {max_blocks == 0 || max_blocks > kFoldMaxBlocks ? (uint32_t)kFoldMaxBlocks : max_blocks,
            max_sg == 0 || max_sg > kFoldMaxSg ? kFoldMaxSg : max_sg};
}

// The environment overrides (measurement only), read once per process by
// fold_knobs() in pir_kernels.hip; the values here are the defaults.
struct FoldKnobs {
    int skew = 62;                    // DPF_FOLD_SKEW: percent of a CU's chunk pair for its first k_fold4r workgroup
    uint64_t nt_min = 256ull << 20;   // DPF_FOLD_NT_MIN: DB bytes from which the matrix-core fold loads nontemporal
    int per_cu = 0;                   // DPF_FOLD_PER_CU: workgroups per CU at C = 1 (0: the tuned choice)
    int wide_cg = 4;                  // DPF_FOLD_WIDE_CG: cap of the columns per workgroup
    uint64_t xor_ys = 0;              // DPF_XOR_PARTS_YS: part slices per answer word (0: by the part count)
};

inline bool rec_bytes_ok(uint64_t rec_bytes) {
    return rec_bytes != 0 && rec_bytes % 32 == 0 && rec_bytes <= kFoldMaxRecBytes;
}

// ---- records of any width over the sliced layout ---------------------------
// The sliced kernels take every positive multiple of 4 bytes: a record is
// T = rec_bytes / 4 bit tiles of 32 rows (bit positions) in C = ceil(T / 8)
// columns, a super-group 32 T rows of 8 words with no padding after the last
// one, so the last column of a record may be short (8 * rec_bytes - 256 c
// rows) and a tile 8 c + i >= T does not exist: its rows would lie in the next
// super-group, or past the buffer.  Multiples of 32 are T = 8 C, every tile
// present.
inline bool rec_bytes_any_ok(uint64_t rec_bytes) {
    return rec_bytes != 0 && rec_bytes % 4 == 0 && rec_bytes <= kFoldMaxRecBytes;
}
inline uint32_t rec_tiles(uint64_t rec_bytes) { return (uint32_t)(rec_bytes / 4); }
inline uint32_t rec_cols(uint64_t rec_bytes) { return (uint32_t)((rec_bytes + 31) / 32); }
// Rows (bit positions) and bit tiles of column c < rec_cols().
inline uint32_t col_rows(uint64_t rec_bytes, uint32_t c) {
    const uint64_t left = 8 * rec_bytes - 256ull * c;
    return (uint32_t)(left < 256 ? left : 256);
}
inline uint32_t col_tiles(uint64_t rec_bytes, uint32_t c) { return col_rows(rec_bytes, c) / 32; }
inline bool tile_exists(uint64_t rec_bytes, uint64_t tile) { return tile < rec_bytes / 4; }
inline uint64_t sg_stride_bytes(uint64_t rec_bytes) { return 256 * rec_bytes; }
inline uint64_t sliced_bytes_any(uint64_t nrec, uint64_t rec_bytes) { return (nrec + 255) / 256 * sg_stride_bytes(rec_bytes); }
// Byte offset of tile `tile` (32 rows of 8 words: 1 KiB) of super-group S.
inline uint64_t tile_off_bytes(uint64_t rec_bytes, uint64_t S, uint64_t tile) {
    return S * sg_stride_bytes(rec_bytes) + tile * 1024;
}

// Part slices per answer word of k_xor_parts, one atomic each: 16 for <= 256
// partials (the PIR rank at N = 8: step 0.0733-0.0737 vs 0.0740-0.0745 ms with
// 64, 8 in between), 64 above (one GPU, 768 partials: 0.3799-0.3802 vs
// 0.3811-0.3817 with 16); tools/archive/r05_xys.sh, profiles/r05/xor_parts/.
inline uint32_t xor_parts_ys(uint64_t nparts, uint64_t ys_knob) {
    const uint64_t ymax = ys_knob ? ys_knob : nparts <= 256 ? 16 : 64;
    return (uint32_t)(nparts < ymax ? nparts : ymax);
}

// ---- the row-major folds ---------------------------------------------------
// How launch_pir_fold covers (rec_bytes, nkeys): `cols` 32-byte columns per
// pass (1, 2, 4 or 8 = the whole record; 1 with `col_passes` = rec_bytes/32
// for other widths), `keys_per_pass` keys per DB read, the direct kernel or
// Four-Russians with `kw` 64-key lane groups sharing each table.
struct FoldPlan {
    uint32_t cols, col_passes, keys_per_pass, kw;
    bool direct;
};
inline FoldPlan plan_fold(uint64_t rec_bytes, uint32_t nkeys) {
    FoldPlan p{};
    const uint64_t c = rec_bytes / 32;
    p.cols = (c == 1 || c == 2 || c == 4 || c == 8) ? (uint32_t)c : 1;
    p.col_passes = p.cols == c ? 1 : (uint32_t)c;
    // Measured (tools/fold_bench, 2^24 x 32 B): direct is HBM-bound to 4 keys
    // (98 -> 101 us) but slower than Four-Russians from 8 (150 vs ~140 us);
    // wider records favour it longer (64 B, 16 keys: 69 us).
    p.direct = nkeys <= 4 || (p.cols >= 2 && nkeys <= kFoldDirectMaxKeys);
    const uint32_t kw_cap = p.cols >= 8 ? 1 : p.cols == 4 ? 2 : 4;
    uint32_t kw = 1;
    if (!p.direct)
        while (kw < kw_cap && 64u * kw < nkeys) kw *= 2;
    p.keys_per_pass = p.direct ? kFoldDirectMaxKeys : 64 * kw;
    p.kw = p.direct ? 0 : kw;
    return p;
}
// The direct kernel's work is linear in its key slots: 1, 4 or 16 by batch.
inline uint32_t fold_direct_slots(uint32_t nkeys) { return nkeys <= 1 ? 1 : nkeys <= 4 ? 4 : kFoldDirectMaxKeys; }

// nchunks in `blocks` contiguous ranges of whole `gran`-chunk batches, `cpb`
// chunks each (the last one what is left), at most `cap` of them.
struct ChunkSplit {
    uint64_t blocks, cpb;
};
inline ChunkSplit split_chunks(uint64_t nchunks, uint64_t want_blocks, uint64_t gran, uint64_t cap) {
    if (want_blocks > cap) want_blocks = cap;
    uint64_t cpb = (nchunks + want_blocks - 1) / want_blocks;
    cpb = (cpb + gran - 1) / gran * gran;
    return {(nchunks + cpb - 1) / cpb, cpb};
}

inline ChunkSplit plan_fold_direct(uint64_t nchunks, uint64_t cus, uint64_t cap) {
    return split_chunks(nchunks, cus * 4, kFoldDirectGran, cap);
}

// k_fold4r<C, KW, WV>.  KW = 1, C < 8: 8 waves, 72 KiB of LDS -> 2 workgroups
// (16 waves, 128 VGPRs) per CU.  Otherwise 4 waves, 41-50 KiB -> 3 per CU (168
// VGPRs: 64 accumulators per lane).
constexpr int fold4r_waves(int C, int KW) { return KW == 1 && C < 8 ? 8 : 4; }
constexpr uint64_t fold4r_per_cu(int wv) { return wv == 8 ? 2 : 3; }

// Workgroup b < nfirst takes chunks [b * cpb_first, + cpb_first), the others
// cpb each after those (k_fold4r's c0 / my).
struct Fold4rLaunch {
    uint64_t blocks, cpb;
    uint32_t nfirst;
    uint64_t cpb_first;
};
// Two workgroups per CU: a SIMD's waves issue oldest-first, so the CU's first
// workgroup (dispatched first: one per CU) runs ahead of its second (fold
// per-wave times: 100 vs 143 us at configs[4]).  skew (percent of a CU pair's
// chunks for the first workgroup) shifts work to it.
inline Fold4rLaunch plan_fold4r(uint64_t nchunks, int wv, uint64_t cus, uint64_t cap, int skew) {
    const uint64_t per_cu = fold4r_per_cu(wv), gran = 2 * (uint64_t)wv;
    const ChunkSplit s = split_chunks(nchunks, cus * per_cu, gran, cap);
    Fold4rLaunch l{s.blocks, s.cpb, 0, s.cpb};
    if (per_cu == 2 && skew > 50 && skew < 100 && s.blocks == 2 * cus) {
        const uint64_t pair = 2 * s.cpb;
        const uint64_t first = (pair * (uint64_t)skew / 100 + gran / 2) / gran * gran;
        const uint64_t rest = pair - first;
        if (rest >= gran && nchunks <= cus * pair) l = {s.blocks, rest, (uint32_t)cus, first};
    }
    return l;
}

// ---- the folds over the sliced DB ------------------------------------------
// k_fold_mfma<MT, NT, SG, CG, NTDB, WPE>: MT key tiles x NT bit tiles per
// wave, SG super-groups per staged block, CG columns per workgroup, compiled
// for WPE waves per SIMD.  A column group of CG columns is 4 CG waves, so the
// shape has 512 / CG registers (less where two workgroups share a CU): the
// staged blocks shrink (SG) until nothing spills, and CG stops where that no
// longer works (register counts per instantiation: DESIGN §4.4).  32-byte
// records take the CG = 1 shapes.
struct FoldTile {
    int MT, NT, SG, CG, WPE;
};
constexpr FoldTile kFoldTiles[] = {
    {1, 2, 2, 4, 4}, {1, 2, 2, 2, 4}, {1, 2, 4, 1, 2},   // <= 32 keys, cg = 4, 2, 1
    {2, 2, 2, 1, 2},                                     // <= 64: CG = 2 (<2,2,4,2>, 2 waves per SIMD) measured no faster
    {4, 2, 2, 2, 2}, {4, 2, 4, 1, 1},                    // <= 128, cg >= 2, 1
    {8, 2, 4, 1, 1},                                     // <= 256
};
constexpr int kFoldTileCount = (int)(sizeof(kFoldTiles) / sizeof(kFoldTiles[0]));

// Columns per workgroup: the largest of 4, 2, 1 that divides C, capped by the
// knob and then per tile shape.
inline int fold_cg(uint32_t C, int wide_cg) {
    const int cg = C % 4 == 0 ? 4 : C % 2 == 0 ? 2 : 1;
    return cg > wide_cg ? (wide_cg >= 2 ? 2 : 1) : cg;
}
// Index into kFoldTiles of the shape for a key group of nk <= 256 keys.
inline int fold_tile_index(uint32_t nk, int cg) {
    if (nk <= 32) return cg == 4 ? 0 : cg == 2 ? 1 : 2;
    if (nk <= 64) return 3;
    if (nk <= 128) return cg >= 2 ? 4 : 5;
    return 6;
}
// The one dispatch from a run-time tile index to code compiled per shape:
// calls f(FoldTileIndex<I>{}) for I = shape (an index past the table takes the
// last shape) and returns what it returns.
template <int I>
struct FoldTileIndex {
    static constexpr int value = I;
};
template <class F>
auto with_fold_tile(int shape, F&& f) {
    static_assert(kFoldTileCount == 7, "one case per tile shape");
    switch (shape) {
        case 0: return f(FoldTileIndex<0>{});
        case 1: return f(FoldTileIndex<1>{});
        case 2: return f(FoldTileIndex<2>{});
        case 3: return f(FoldTileIndex<3>{});
        case 4: return f(FoldTileIndex<4>{});
        case 5: return f(FoldTileIndex<5>{});
        default: return f(FoldTileIndex<6>{});
    }
}

// The DB pieces of a matrix-core fold over at least nt_min DB bytes are
// loaded nontemporal.  r05 (tools/archive/r05_nt.sh, profiles/r05/fold_nt/, B = 64,
// fold us, nontemporal vs default): 2^24 x 32 B (512 MiB, twice the chip's
// last-level cache) 123-125 vs 135-138, and B = 16 95 vs 105-107; 2^23 66-69
// vs 67-74; but 2^22 39-40 vs 35-36 and 2^21 (an N = 8 rank) 25.5 vs 24.7:
// slices that stay cached between batches lose.
inline uint64_t fold_db_bytes(uint64_t nsg, uint32_t C) { return nsg * 256 * 32 * C; }
inline bool fold_ntdb(uint64_t nsg, uint32_t C, uint64_t nt_min) { return fold_db_bytes(nsg, C) >= nt_min; }
// The same for any width, by the bytes the DB really has.
inline uint64_t fold_db_bytes_any(uint64_t nsg, uint64_t rec_bytes) { return nsg * sg_stride_bytes(rec_bytes); }
inline bool fold_ntdb_any(uint64_t nsg, uint64_t rec_bytes, uint64_t nt_min) {
    return fold_db_bytes_any(nsg, rec_bytes) >= nt_min;
}

// Workgroups per CU of a matrix-core fold launch: resident workgroups only
// (one round), each a contiguous run of whole staged blocks.  (A fixed 4
// workgroups per CU left 1/4 - 3/4 of them for a second round at 3 or 1
// resident per CU.)  occ: the shape's occupancy limit; C > 1 launches that.
// 32-byte records (C = 1): two workgroups per CU instead of the occupancy
// limit (3 at 33-64 keys) for cached DB slices and for the one-key-tile
// shape: fewer partials to combine and less per-workgroup overhead (r05,
// tools/archive/r05_fpercu.sh, profiles/r05/fold_blocks/, medians of 5:
// 2^21 x 32 B 22.6 vs 24.7 us, 2^22 34.8 vs 36.0, B = 16 at 2^24 91.9 vs
// 96.6, B = 32 96.3 vs 99.8; but B = 64 at 2^23 / 2^24 67.9 / 130.7 vs
// 67.0 / 125.9).  One per CU for 33-64 keys over a slice of <= 64 MiB (the
// PIR rank at N = 8): rank step 0.0741-0.0750 vs 0.0742-0.0759 ms, lower in
// 5 of 6 interleaved pairs; at N = 4 (128 MiB) the pairs split 3 / 3 and the
// fold alone was slower (37.6 vs 33.9 us), so it keeps 2
// (tools/archive/r05_fpercu1.sh, profiles/r05/fold_blocks/per_cu1_*.txt).
// per_cu_knob > 0 (A/B runs, C = 1): this many, at most occ.
inline uint64_t fold_per_cu(uint32_t C, int MT, bool ntdb, uint64_t slice_bytes, int occ, int per_cu_knob) {
    if (C > 1) return (uint64_t)occ;
    if (per_cu_knob > 0) return (uint64_t)(per_cu_knob < occ ? per_cu_knob : occ);
    if (slice_bytes <= (64ull << 20) && MT == 2) return 1;
    return (!ntdb || MT == 1) && occ > 2 ? 2 : (uint64_t)occ;
}

// One fold launch over the sliced DB: grid (blocks, gy); workgroup (x, y)
// folds super-groups [S0 + x * spb, + spb) (cut at S0 + n) of column group
// g0 + y.  The launch reads its selection words from word sel_off of each key
// row and its DB from byte db_off, and clears clear_words answer words first
// (nonzero for the first launch of a call only).
struct FoldLaunch {
    uint64_t g0, gy, S0, n, blocks, spb;
    uint64_t sel_off, db_off, clear_words;
    uint64_t wlim(uint64_t wpk) const { return wpk > sel_off ? wpk - sel_off : 0; }   // words left of a key row
};

// The launches of one key group over nsg super-groups of ncg column groups:
// x * y <= cap workgroups each (x super-group runs, y column groups), in passes
// of at most x * msg super-groups; no workgroup folds more than msg
// super-groups or fewer than one, runs are whole multiples of gran, and a pass
// aims at `resident` workgroups.
struct SlicedFoldPlan {
    uint64_t nsg, ncg, cap, msg, gran, resident;
    uint32_t C;
    uint64_t clear_words;
    uint64_t rec_bytes = 0;   // 0: 32 C (the plans from before records of any width)
    uint64_t sg_bytes() const { return sg_stride_bytes(rec_bytes ? rec_bytes : 32ull * C); }

    // fn(const FoldLaunch&) for every launch in stream order, until one
    // returns a nonzero (error) value, which is returned.
    template <class F>
    auto for_each_launch(F fn) const -> decltype(fn(FoldLaunch{})) {
        const uint64_t gy_max = ncg < cap ? ncg : cap;
        for (uint64_t g0 = 0; g0 < ncg; g0 += gy_max) {
            const uint64_t gy = ncg - g0 < gy_max ? ncg - g0 : gy_max;
            const uint64_t xcap = cap / gy;                          // >= 1
            const uint64_t per_pass = xcap * msg;
            for (uint64_t S0 = 0; S0 < nsg; S0 += per_pass) {
                const uint64_t n = nsg - S0 < per_pass ? nsg - S0 : per_pass;
                uint64_t want = (n + msg - 1) / msg;                 // none folds more than msg super-groups
                if (want < resident / gy) want = resident / gy;
                if (want < 1) want = 1;
                const ChunkSplit s = split_chunks(n, want, gran, xcap);
                const bool first = g0 == 0 && S0 == 0;
                const FoldLaunch l{g0, gy, S0, n, s.blocks, s.cpb, S0 * 8, S0 * sg_bytes(), first ? clear_words : 0};
                if (auto e = fn(l); e != decltype(e){}) return e;
            }
        }
        return {};
    }
};

// The answer words that the first launch of key group k0 clears: all of the
// call's, in its first key group.
inline uint64_t fold_clear_words(uint32_t nkeys, uint32_t C, uint32_t k0) { return k0 == 0 ? (uint64_t)nkeys * 8 * C : 0; }
// For any width: T = rec_tiles() answer words per key, tightly packed.
inline uint64_t fold_clear_words_any(uint32_t nkeys, uint64_t rec_bytes, uint32_t k0) {
    return k0 == 0 ? (uint64_t)nkeys * rec_tiles(rec_bytes) : 0;
}

// k_fold_mfma with tile shape t for one key group; clear_words: fold_clear_words().
// resident: CUs x fold_per_cu().
// C columns (rec_cols()); rec_bytes: the record width where it is not 32 C.
inline SlicedFoldPlan plan_fold_mfma(uint64_t nsg, uint32_t C, const FoldTile& t, FoldLimits lim, uint64_t resident,
                                     uint64_t clear_words, uint64_t rec_bytes = 0) {
    const uint64_t sg = (uint64_t)t.SG, msg = lim.max_sg / sg * sg > 0 ? lim.max_sg / sg * sg : sg;
    return {nsg, C / (uint32_t)t.CG, lim.max_blocks, msg, sg, resident, C, clear_words, rec_bytes};
}
// k_fold_sliced_direct (one key): a column per grid row, runs of whole pairs
// of super-groups, 8 workgroups per CU, one pass (XOR accumulators: no bound
// on a run).
inline SlicedFoldPlan plan_fold_sliced_direct(uint64_t nsg, uint32_t C, FoldLimits lim, uint64_t cus,
                                              uint64_t rec_bytes = 0) {
    return {nsg, C, lim.max_blocks, nsg, 2, cus * 8, C, rec_bytes ? (uint64_t)rec_tiles(rec_bytes) : 8ull * C, rec_bytes};
}

// ---- grid chunking of the maintenance launches -----------------------------
// fn(first, count) over [0, n) in spans of at most `per`, until one returns a
// nonzero (error) value, which is returned.
template <class F>
auto for_each_span(uint64_t n, uint64_t per, F fn) -> decltype(fn(uint64_t{}, uint64_t{})) {
    for (uint64_t i0 = 0; i0 < n; i0 += per)
        if (auto e = fn(i0, n - i0 < per ? n - i0 : per); e != decltype(e){}) return e;
    return {};
}
// k_slice_db: one workgroup per (super-group, column), at most 2^30 per launch
// (C = rec_cols() for any width).
inline uint64_t slice_db_span(uint64_t C) { return (1ull << 30) / C; }
// Kernels of per_rec threads per record in workgroups of 256: records per
// launch, whole records and at most 2^38 threads (2^30 workgroups).
inline uint64_t record_span(uint64_t per_rec) { return (1ull << 38) / per_rec; }

// k_update_sliced: chunks of K consecutive updates, one workgroup per (chunk,
// column).  n updates over nsg super-groups: runs of n / nsg updates at least
// on average, so chunks of that many hold about one head or fewer each.  A
// launch takes `span` updates: its chunks, rounded up to a multiple of 8 (the
// kernel's slot -> chunk map), times C stay within 2^30 workgroups.
struct UpdatePlan {
    uint32_t K;
    uint64_t span;
    uint64_t chunks(uint64_t m) const { return (m + K - 1) / K; }                 // of a launch of m updates
    uint64_t grid(uint64_t m, uint64_t C) const { return (chunks(m) + 7) / 8 * 8 * C; }
};
inline UpdatePlan plan_update_sliced(uint64_t n, uint64_t nsg, uint64_t C) {
    uint32_t K = 1;
    while (K < 64 && 2ull * K <= n / nsg) K *= 2;
    return {K, ((1ull << 30) / C - 8) * K};
}

}  // namespace dpfh
