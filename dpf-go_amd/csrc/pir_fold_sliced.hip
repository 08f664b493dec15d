// pir_fold_sliced.hip — the XOR fold over the bit-sliced DB: the matrix-core
// fold (k_fold_mfma), its one-key form (k_fold_sliced_direct) and the slicing
// of a row-major DB (k_slice_db).  The launchers walk the plans of
// pir_fold_plan.hpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpf_kernels.hpp"
#include "fold_ops.hpp"
#include "pir_kernels.hpp"

namespace dpfk {

// ---------------------------------------------------------------------------
// The fold as a GF(2) matrix product on the matrix cores.
//
//   count[k][n] = sum_i sel[k][i] * dbbit[i][n],   ans bit (k, n) = count & 1
//
// is a {0,1} product of [keys x records] by [records x 256 bit positions], so
// it runs on v_mfma_scale_f32_32x32x64_f8f6f4 with e2m1 (FP4) operands: every
// product is exactly 1 or 0, the fp32 accumulators hold exact counts (far
// below 2^24 per workgroup, see below), and the parity is the answer bit.
//
// Operands.  An MFMA operand lane holds 32 K-values (records) of ONE row
// (key) or column (bit position); the K order inside the lane is ours to
// pick as long as A and B agree.  The key side is EvalFull's own layout: one
// selection word = 32 consecutive records of one key.  The DB side needs the
// transposed form -- for bit position n, one word of 32 consecutive records
// -- which the PIR server builds once when the DB is loaded (the "sliced"
// layout, k_slice_db below).  A record of rec_bytes = 32 C bytes is C 32-byte
// columns:
//   dbs[S][c][n][g] (u32), S = super-group of 256 records, c < C column,
//   n < 256 bit position of the column, g < 8 record group; bit j = bit n of
//   bytes [32c, 32c + 32) of record 256 S + 32 g + j
// (32-byte records: C = 1, dbs[S][n][g]).  A lane (n, h) loads
// dbs[S][c][n][4h .. 4h+3] and a key lane (k, h) takes selection words
// 8S + 4h .. +3 (one dwordx4 each): K-block t < 4 of super-group S is record
// groups t (h = 0) and 4 + t (h = 1).
// Word -> FP4 operand in registers, nibble i of dword d = record 4i + d:
//   one side  d0 = x & 0x1..  (0.5)  d1 = x & 0x2.. (1.0)  d2 = x & 0x4.. (2.0)
//             d3 = (x >> 1) & 0x4.. (2.0)                       5 VALU per word
//   the other d0 = (s << 2) & 0x4.. (2.0)  d1 = s & 0x2.. (1.0)
//             d2 = (s >> 2) & 0x1.. (0.5)  d3 = (s >> 3) & 0x1.. (0.5)   7 VALU
// so every nonzero product is exactly 1 with unit (E8M0 127) scales.
//
// Mapping.  A wave covers MT key tiles (32 keys) x NT bit tiles (32 bit
// positions) of one column over a contiguous run of super-groups.  To the
// fold a wide record is a record of 8 C bit tiles instead of 8, and a
// selection operand is the same for every tile, so a workgroup takes a column
// group of CG columns: CG * NS waves, NS = 8 / NT; wave wv folds bit slice
// wv % NS of column wv / NS of the group.  Then
//   - a staged block's selection rows are loaded and written to LDS once for
//     all CG columns (selection bytes per DB byte 1 / (4 CG));
//   - the workgroup's DB stream is runs of CG * 8 KiB, one per super-group.
// Column groups are the grid's y dimension: every workgroup of a launch holds
// a (super-group run, column group) pair, workgroups per launch x * y <= the
// workgroup cap.  At the end each accumulator register's parities become two
// answer words by one ballot (C/D layout: lane = column n, register e = rows
// (e&3) + 8(e>>2) + 4h), written to the workgroup's partial, and one
// k_xor_parts launch combines
//   parts[x][key][8 CG y words]
// into the answers.  32-byte records are ncols = 1, CG = 1, grid.y = 1.  CG is
// the largest of 4, 2, 1 that divides C, capped by what the tile shape's
// registers allow (dpfh::fold_cg, dpfh::kFoldTiles).
//
// Selection words reach the waves through LDS: per block of SG super-groups
// the workgroup copies each key's SG*32-byte span (coalesced) into a padded
// row, and the next block's selection words and DB pieces are in flight in
// registers while this block is folded (block-level double buffering: a
// super-group of MFMA work is ~0.2-0.4 us per wave, shorter than the HBM
// latency under load).  Loaded straight into the operand lanes, 16 B per
// lane from 32 rows 2 MiB apart, the fold fetched ~1.6x its bytes and ran at
// a third of the HBM rate (profiles/r04/fold_v1).
//
// Exactness of the fp32 counts: an accumulator gains at most 64 per MFMA
// (one per record of a K-block), and fp32 holds every integer up to 2^24.
// A workgroup's run of super-groups would grow with the DB and shrink with
// the CU count, so plan_fold_mfma never gives one more than
// dpfh::kFoldMaxSg = 2^15 super-groups (2^23 records): it adds workgroups,
// and beyond kFoldMaxBlocks of them it folds the DB in passes, each pass's
// partials XORed into the answers.  (Reducing the counts to parities inside
// the kernel moved the large-tile accumulators out of AGPRs and spilled them:
// 2.5x slower at 256 keys, r05.)  wlim: selection words per key row from
// `bits` (the row stride stays wpk), so a pass can start mid-row.  The
// operand expansions themselves (fp4_w5, fp4_w7) are in fold_ops.hpp.
//
// k_fold_mfma<MT, NT, SG, CG, NTDB, WPE>: tile shape, super-groups per staged
// block, columns per workgroup, nontemporal DB loads, and the waves per SIMD
// the shape is compiled for (its register budget).  cg0: first column group
// of the launch.
//
// Records of any width (a multiple of 4 bytes): a record is T = rec_bytes / 4
// bit tiles, a super-group 32 T rows with the next one directly behind, and
// the last column may have fewer than 8 tiles.  A wave's tile 8 col + w NT + j
// >= T does not exist (its rows would be the next super-group's, or past the
// buffer at the last one): no load, no answer word; a wave none of whose tiles
// exists only helps staging the selection rows.  Tile t, row r of super-group
// S is uint4 ((S T + t) 32 + r) 2 + h, which for T = 8 C is the form above.
// FULL: the record is whole columns (T = 8 C, a multiple of 32 bytes), every
// tile exists and the guards fold away: the kernel from before records of any
// width (with the guards in, 64-byte records measured 2 % slower at 64 keys).
//
// The loop itself -- wave decode, staging, block loop, operands, MFMA nest,
// ballots -- is fold_mfma_body.inc, shared as text with k_fold_grouped_mfma.
// What is the dense kernel's own is below, as the macros that file names: the
// answers' clearing, the column group and the run from the grid, the any-width
// tile address, and partials.
template <int MT, int NT, int SG, int CG, bool NTDB, int WPE, bool FULL>
__global__ __launch_bounds__(64 * (8 / NT) * CG, WPE) void k_fold_mfma(
    const uint32_t* __restrict__ bits, uint64_t wpk, const uint4* __restrict__ dbs, uint64_t nsg, uint32_t nkeys,
    uint64_t sg_per_block, uint32_t* __restrict__ parts, uint32_t* __restrict__ zero, uint64_t zero_words,
    uint64_t wlim, uint32_t ntiles, uint32_t cg0) {
    zero_answers(blockIdx.y == 0 ? zero : nullptr, zero_words);
#define FOLD_UNIT                                             \
    const uint64_t col0 = (uint64_t)(cg0 + blockIdx.y) * CG; \
    const uint32_t* const sel = bits;                        \
    const uint64_t stride = wpk;                             \
    const uint32_t nrows = nkeys;
#define FOLD_RUN                                                          \
    const uint64_t s0 = (uint64_t)blockIdx.x * sg_per_block;               \
    const uint64_t s1 = s0 + sg_per_block < nsg ? s0 + sg_per_block : nsg; \
    if (s0 >= s1) return; /* uniform over the workgroup */
#define FOLD_DB_AT(S, j) &dbs[((S * ntiles + tile0 + j) * 32 + r) * 2 + h]
    // Answer words: parts[x][key][8 CG y] (word = 8 * column of the launch + bit tile).
#define FOLD_EMIT_BEGIN              \
    constexpr uint32_t pkeys = 32 * MT; \
    const uint32_t pwords = 8u * CG * gridDim.y;
#define FOLD_EMIT(m, j, out)          \
    if (l < 32 && (uint32_t)j < nt) \
        parts[((uint64_t)blockIdx.x * pkeys + 32 * m + l) * pwords + (blockIdx.y * CG + cw) * 8 + w * NT + j] = out;
#include "fold_mfma_body.inc"
}

// The sliced layout (above) from a row-major DB of 32 C-byte records.
// Workgroup b = (super-group S, column c) = (b / C, b % C); its 4 waves take
// 64 records each: lane l holds the column's 8 words of record l and one
// ballot per bit position transposes 32 x 32 bits.  Any width: a record is
// ntiles words, column c has nw = min(8, ntiles - 8 c) of them, and only a
// record of whole columns (ntiles % 8 == 0: a multiple of 32 bytes) is read by
// 16-byte loads; other rows are only 4-byte aligned.
__global__ __launch_bounds__(256) void k_slice_db(const uint4* __restrict__ db, uint64_t nrec, uint32_t ncols,
                                                   uint32_t ntiles, uint32_t* __restrict__ dbs) {
    const uint64_t S = blockIdx.x / ncols;
    const uint32_t c = blockIdx.x % ncols;
    const uint32_t l = threadIdx.x & 63, wq = threadIdx.x >> 6;
    const uint64_t rec = S * 256 + wq * 64 + l;
    const uint32_t nw = ntiles - 8 * c < 8 ? ntiles - 8 * c : 8;       // uniform
    uint32_t wd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ntiles % 8 == 0) {
        uint4 a = make_uint4(0, 0, 0, 0), b = a;
        if (rec < nrec) {
            a = db[rec * 2 * ncols + 2 * c];
            b = db[rec * 2 * ncols + 2 * c + 1];
        }
        wd[0] = a.x, wd[1] = a.y, wd[2] = a.z, wd[3] = a.w, wd[4] = b.x, wd[5] = b.y, wd[6] = b.z, wd[7] = b.w;
    } else if (rec < nrec) {
        const uint32_t* row = reinterpret_cast<const uint32_t*>(db) + rec * ntiles + 8 * c;
#pragma unroll
        for (int wi = 0; wi < 8; ++wi)
            if ((uint32_t)wi < nw) wd[wi] = row[wi];
    }
    const uint32_t g = 2 * wq + (l >> 5);
#pragma unroll
    for (int wi = 0; wi < 8; ++wi) {
        if ((uint32_t)wi >= nw) break;                                  // the column's tiles end here
        uint32_t out = 0;
#pragma unroll
        for (int bb = 0; bb < 32; ++bb) {
            const uint64_t m = __builtin_amdgcn_ballot_w64(((wd[wi] >> bb) & 1u) != 0);
            out = l == (uint32_t)bb ? (uint32_t)m : out;
            out = l == (uint32_t)bb + 32 ? (uint32_t)(m >> 32) : out;
        }
        dbs[((S * ntiles + 8 * c + wi) * 32 + (l & 31)) * 8 + g] = out;
    }
}

// One key over the sliced DB: no matrix product needed (the loop is
// fold_popcount_body.inc, shared with k_fold_grouped).  Workgroup (x, y)
// folds super-group run x of column c0 + y; thread n of its 256 owns bit
// position n of that column.  Per super-group it reads its 8 words
// dbs[S][c][n][0..7] (the workgroup: 8 KiB contiguous) and XORs (selection
// word & DB word) into acc -- one v_bitop3 per word, the selection words
// wave-uniform (scalar loads).  The answer bit n is the parity of
// popcount(acc).  parts[x][8 y words].  One key only (97 us at configs[4]
// against the MFMA fold's 103): with 4 or 16 keys the per-key scalar loads
// serialise (131 / 388 us against 104 / 107, profiles/r04/fold_ab/).
// Any width: a super-group is nrows = 8 * rec_bytes rows, and thread n of
// column c has a row only if 256 c + n < nrows; the others fold nothing.
// (Nontemporal DB loads, as the matrix-core fold takes them above 256 MiB,
// measured 95.2-95.8 against 93.9-94.4 us here at 2^24 records: not used.)
__global__ __launch_bounds__(256) void k_fold_sliced_direct(const uint32_t* __restrict__ bits,
                                                            const uint4* __restrict__ dbs, uint64_t nsg,
                                                            uint64_t sg_per_block, uint32_t* __restrict__ parts,
                                                            uint32_t* __restrict__ zero, uint64_t zero_words,
                                                            uint64_t wlim, uint32_t nrows, uint32_t c0) {
    zero_answers(blockIdx.y == 0 ? zero : nullptr, zero_words);
    const uint32_t n = threadIdx.x, l = n & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t col = c0 + blockIdx.y;
    const uint64_t s0 = (uint64_t)blockIdx.x * sg_per_block;
    const uint64_t s1 = s0 + sg_per_block < nsg ? s0 + sg_per_block : nsg;
    constexpr int KP = 1;
#define FOLD_ONE_KEY
#define FOLD_SEL(j, i) bits[i]
#define FOLD_AT(S) &dbs[(S * nrows + row) * 2]
#define FOLD_EMIT_BEGIN
#define FOLD_EMIT(j, m) \
    if (l < 2) parts[(uint64_t)blockIdx.x * (8u * gridDim.y) + 8 * blockIdx.y + 2 * w + l] = l ? (uint32_t)(m >> 32) : (uint32_t)m;
#include "fold_popcount_body.inc"
}

uint64_t pir_sliced_bytes(uint64_t nrec, uint64_t rec_bytes) { return (nrec + 255) / 256 * 256 * rec_bytes; }

hipError_t launch_slice_db(const uint8_t* db, uint64_t nrec, uint64_t rec_bytes, uint8_t* dbs, hipStream_t st) {
    if (!dpfh::rec_bytes_any_ok(rec_bytes)) return hipErrorInvalidValue;
    const uint64_t nsg = (nrec + 255) / 256, C = dpfh::rec_cols(rec_bytes);
    return dpfh::for_each_span(nsg, dpfh::slice_db_span(C), [&](uint64_t S0, uint64_t n) {
        hipLaunchKernelGGL(k_slice_db, dim3((uint32_t)(n * C)), dim3(256), 0, st,
                           reinterpret_cast<const uint4*>(db + S0 * 256 * rec_bytes), nrec - S0 * 256, (uint32_t)C,
                           dpfh::rec_tiles(rec_bytes), reinterpret_cast<uint32_t*>(dbs + S0 * 256 * rec_bytes));
        return hipGetLastError();
    });
}

namespace {

// What the launches of one call share: the arguments and the one reading of
// the limits and the CU budget that all its plans are made from.
struct SlicedFold {
    const uint32_t* bits;
    uint64_t wpk;
    const uint8_t* dbs;
    uint64_t nsg;
    uint32_t C;                    // columns: rec_cols(rec_bytes)
    uint64_t rec_bytes;
    uint32_t* parts;
    dpfh::FoldLimits lim;
    uint64_t cus;
    hipStream_t st;
};

// One key group (nk <= 32 MT keys from row `bits`, answers at `ans`) with tile
// shape kFoldTiles[I]: the plan's fold launches (fp32-exact counts, see
// k_fold_mfma), each followed by a k_xor_parts launch that XORs its partials
// into ans.
template <int I>
hipError_t launch_mfma(const SlicedFold& f, const uint32_t* bits, uint32_t nk, uint32_t* ans, uint64_t clear_words) {
    constexpr dpfh::FoldTile T = dpfh::kFoldTiles[I];
    constexpr int MT = T.MT, NT = T.NT, SG = T.SG, CG = T.CG, WPE = T.WPE, NW = 8 / NT * CG;
    static_assert(32 * MT * CG * 32 <= (int)dpfh::kFoldPartBytes, "a workgroup's partial fits its 16 KiB");
    static int occ = [] {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_fold_mfma<MT, NT, SG, CG, false, WPE, false>, 64 * NW, 0) !=
                hipSuccess || n < 1)
            n = 1;
        return n;
    }();
    const dpfh::FoldKnobs& knobs = fold_knobs();
    const bool ntdb = dpfh::fold_ntdb_any(f.nsg, f.rec_bytes, knobs.nt_min);
    const uint64_t resident =
        f.cus * dpfh::fold_per_cu(f.C, MT, ntdb, dpfh::fold_db_bytes_any(f.nsg, f.rec_bytes), occ, knobs.per_cu);
    const uint32_t ntiles = dpfh::rec_tiles(f.rec_bytes);
    return dpfh::plan_fold_mfma(f.nsg, f.C, T, f.lim, resident, clear_words, f.rec_bytes)
        .for_each_launch([&](const dpfh::FoldLaunch& l) {
        const uint32_t* b = bits + l.sel_off;
        const uint4* d = reinterpret_cast<const uint4*>(f.dbs + l.db_off);
        uint32_t* z = l.clear_words ? ans : nullptr;
        const dim3 grid((uint32_t)l.blocks, (uint32_t)l.gy);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(64 * NW), 0, f.st, b, f.wpk, d, l.n, nk, l.spb, f.parts, z,
                               l.clear_words, l.wlim(f.wpk), ntiles, (uint32_t)l.g0);
        };
        if (ntiles % 8 == 0) {
            if (ntdb) launch(k_fold_mfma<MT, NT, SG, CG, true, WPE, true>);
            else launch(k_fold_mfma<MT, NT, SG, CG, false, WPE, true>);
        } else {
            if (ntdb) launch(k_fold_mfma<MT, NT, SG, CG, true, WPE, false>);
            else launch(k_fold_mfma<MT, NT, SG, CG, false, WPE, false>);
        }
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        return launch_xor_parts(f.parts, l.blocks, nk, 32u * MT, (uint32_t)(8 * CG * l.gy), ans, ntiles,
                                (uint32_t)(8 * CG * l.g0), f.st);
    });
}

// One key over the sliced DB (k_fold_sliced_direct).  parts[x][8 y words] of a
// launch: x * y * 32 bytes, far inside the partials area.
hipError_t launch_sliced_direct(const SlicedFold& f, uint32_t* ans) {
    const dpfh::SlicedFoldPlan p = dpfh::plan_fold_sliced_direct(f.nsg, f.C, f.lim, f.cus, f.rec_bytes);
    return p.for_each_launch([&](const dpfh::FoldLaunch& l) {
        hipLaunchKernelGGL(k_fold_sliced_direct, dim3((uint32_t)l.blocks, (uint32_t)l.gy), dim3(256), 0, f.st, f.bits,
                           reinterpret_cast<const uint4*>(f.dbs), f.nsg, l.spb, f.parts, l.clear_words ? ans : nullptr,
                           l.clear_words, f.wpk, (uint32_t)(8 * f.rec_bytes), (uint32_t)l.g0);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        return launch_xor_parts(f.parts, l.blocks, 1u, 1u, (uint32_t)(8 * l.gy), ans, dpfh::rec_tiles(f.rec_bytes),
                                (uint32_t)(8 * l.g0), f.st);
    });
}

}  // namespace

hipError_t launch_pir_fold_sliced(const uint32_t* bits, uint64_t words_per_key, const uint8_t* dbs, uint64_t nrec,
                                  uint64_t rec_bytes, uint32_t nkeys, uint32_t* ans, uint32_t* parts, hipStream_t st) {
    if (!dpfh::rec_bytes_any_ok(rec_bytes)) return hipErrorInvalidValue;
    if (nkeys == 0) return hipSuccess;
    if (nrec == 0) return launch_zero(ans, (uint64_t)nkeys * rec_bytes, st);
    if (words_per_key % 4 != 0 || words_per_key * 32 < nrec) return hipErrorInvalidValue;
    const uint32_t C = dpfh::rec_cols(rec_bytes), T = dpfh::rec_tiles(rec_bytes);
    const SlicedFold f{bits,  words_per_key, dbs,          (nrec + 255) / 256,   C, rec_bytes,
                       parts, fold_limits(), (uint64_t)cu_count(), st};
    if (nkeys == 1) return launch_sliced_direct(f, ans);   // popcount fold, no MFMA
    const int cg = dpfh::fold_cg(C, fold_knobs().wide_cg);
    for (uint32_t k0 = 0; k0 < nkeys; k0 += dpfh::kFoldKeyGroup) {
        const uint32_t nk = nkeys - k0 < dpfh::kFoldKeyGroup ? nkeys - k0 : dpfh::kFoldKeyGroup;
        const uint32_t* b = bits + (uint64_t)k0 * words_per_key;
        const uint64_t zw = dpfh::fold_clear_words_any(nkeys, rec_bytes, k0);
        uint32_t* a = ans + (uint64_t)k0 * T;
        const hipError_t e = dpfh::with_fold_tile(dpfh::fold_tile_index(nk, cg), [&](auto shape) {
            return launch_mfma<decltype(shape)::value>(f, b, nk, a, zw);
        });
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace dpfk

