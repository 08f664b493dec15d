// pir_fold_grouped_mfma.hip — the matrix-core grouped fold: up to 256 keys of
// every group share one pass over the group's tiles, all groups in one launch
// per key tile.  It is the fold of k_fold_mfma (pir_fold_sliced.hip: the GF(2)
// product on v_mfma_scale_f32_32x32x64_f8f6f4 with FP4 operands, the operand
// layout, the staging of selection rows through LDS, the ballot epilogue, and
// why the fp32 counts are exact) with the unit decode of the grouped kernels
// (dpfh::group_unit, pir_group_plan.hpp).  The plan is
// pir_group_fold_plan.hpp's matrix-core route; launch_pir_fold_grouped
// (pir_fold_grouped.hip) walks it.
//
// The loop is a copy of k_fold_mfma's and not a shared body.  The two differ
// in every address (a group and a run per workgroup instead of grid
// coordinates, key rows of one group, answers instead of partials), and the
// dense kernel's instantiations are tuned to the register: its tile shapes
// were picked by which of them do not spill.  A body shared through a header
// would have to be shown to compile k_fold_mfma to the same register, LDS and
// scratch figures for all its 28 instantiations; the copy leaves that kernel
// and its object code untouched.  What the two share is fold_ops.hpp (the
// operand expansions, the loads, the barrier) and the tile table
// dpfh::kFoldTiles.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dpf_kernels.hpp"
#include "fold_ops.hpp"
#include "pir_group_fold_plan.hpp"
#include "pir_kernels.hpp"

namespace dpfk {

// k_fold_grouped_mfma<MT, NT, SG, CG, WPE, FULL>: the tile shape of
// dpfh::kFoldTiles and FULL as in k_fold_mfma.  Workgroup x of the 1-D grid is
// unit u0 + x of the key tile's pass: run [s0, s1) (group-local super-groups)
// of column group un.c (CG columns) of group g, for the keys k0 .. k0 + kp - 1
// of that group, kp <= 32 MT.  Wave wv folds bit slice wv % NS of column
// wv / NS of the column group.
// Selection row j of the tile is row g * kpg + k0 + j of bits, wlim words
// long (the row stride); word 8 S + q of a row is super-group S of the GROUP.
// Rows j >= kp are not read but staged as zeros: behind the last group's keys
// there is no row.  Words at or past wlim are zeros too (a row may be shorter
// than a super-group, or end inside the last one).
// DB tile t, row r of group-local super-group S is at flat super-group
// g * gsg + S of the any-width layout (group_tile, fold_ops.hpp), half h of it.
// A bit tile the record does not have (8 col + w NT + j >= ntiles) is neither
// loaded nor answered; loads past the run are clamped inside the run and never
// folded.
// Answers: no partials.  The parities of key row 32 m + lane, bit tile
// 8 col + w NT + j go to d_ans row g * kpg + k0 + 32 m + lane, for rows < kp
// only.  atomic == 0 (one run per group and column group): this workgroup is
// the only writer of its words and stores them.  Otherwise the answers were
// cleared earlier in stream order and every nonzero word is XORed in with a
// vector atomic; XOR is order-free, so the answers are deterministic.
template <int MT, int NT, int SG, int CG, int WPE, bool FULL>
__global__ __launch_bounds__(64 * (8 / NT) * CG, WPE) void k_fold_grouped_mfma(
    const uint32_t* __restrict__ bits, uint64_t wlim, const uint4* __restrict__ dbs, uint64_t gsg, uint32_t ncg,
    uint64_t runs, uint64_t spr, uint32_t kpg, uint32_t k0, uint32_t kp, uint32_t ntiles, uint32_t* __restrict__ ans,
    uint64_t u0, uint32_t atomic) {
    constexpr int NS = 8 / NT;                                 // bit slices of a column
    constexpr int NW = NS * CG;
    constexpr bool SC = NT < MT;                               // the selection side takes the cheap expansion
    constexpr int kRows = 32 * MT;
    constexpr int kRow = SG * 8 + 4;                           // words per staged row (+4: conflict-free b128 reads)
    constexpr int kPieces = kRows * (SG * 2);                  // uint4 pieces per staged block
    constexpr int kPer = (kPieces + 64 * NW - 1) / (64 * NW);  // per thread
    __shared__ __attribute__((aligned(16))) uint32_t s_sel[kRows * kRow];
    const uint32_t l = threadIdx.x & 63, h = l >> 5, r = l & 31;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t w = wv % NS, cw = wv / NS;                   // bit slice, column of the group
    const dpfh::GroupUnit un = dpfh::group_unit(u0 + blockIdx.x, runs, spr, gsg, ncg);
    const uint64_t s0 = un.s0, s1 = un.s1;                      // never empty (the plan)
    const uint64_t key0 = un.g * kpg + k0;                      // first selection / answer row of the tile
    const uint32_t* sel = bits + key0 * wlim;
    const uint64_t col = (uint64_t)un.c * CG + cw;
    const uint64_t tile0 = 8 * col + w * NT;                    // this wave's first bit tile
    const uint32_t nt =                                         // how many of its NT tiles the record has
        FULL ? (uint32_t)NT
             : __builtin_amdgcn_readfirstlane(tile0 >= ntiles               ? 0u
                                              : ntiles - tile0 < (uint64_t)NT ? (uint32_t)(ntiles - tile0)
                                                                              : (uint32_t)NT);
    auto load_sel = [&](uint64_t sb, uint4 (&v)[kPer]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const uint32_t p = threadIdx.x + (uint32_t)i * 64 * NW;
            const uint32_t row = p / (2 * SG), q = p % (2 * SG);
            const uint64_t word = sb * 8 + 4 * q;
            const bool ok = p < (uint32_t)kPieces && row < kp && word + 4 <= wlim;
            const uint4 x = *reinterpret_cast<const uint4*>(sel + (ok ? (uint64_t)row * wlim + word : 0));
            v[i] = ok ? x : make_uint4(0, 0, 0, 0);
        }
    };
    auto store_sel = [&](const uint4 (&v)[kPer]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const uint32_t p = threadIdx.x + (uint32_t)i * 64 * NW;
            if (p < (uint32_t)kPieces) *reinterpret_cast<uint4*>(&s_sel[(p / (2 * SG)) * kRow + 4 * (p % (2 * SG))]) = v[i];
        }
    };
    // DB pieces of a whole block (clamped past the run; never folded).  A
    // tile the record does not have is not loaded: zeros.
    auto load_db = [&](uint64_t sb, uint4 (&B)[SG][NT]) __attribute__((always_inline)) {
#pragma unroll
        for (int sl = 0; sl < SG; ++sl) {
            const uint64_t S = sb + sl < s1 ? sb + sl : s1 - 1;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                B[sl][j] = make_uint4(0, 0, 0, 0);
                if ((uint32_t)j < nt)
                    B[sl][j] = fold_ld<false>(group_tile(dbs, un.g, gsg, S, 32 * ntiles, (tile0 + j) * 32 + r) + h);
            }
        }
    };
    fold_v16f acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][j][e] = 0.0f;
    // One super-group: 4 K-blocks of 64 records x MT x NT MFMAs.
    auto fold_sg = [&](int sl, const uint4 (&B)[NT]) __attribute__((always_inline)) {
        uint4 A[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
            A[m] = *reinterpret_cast<const uint4*>(&s_sel[(32 * m + r) * kRow + 8 * sl + 4 * h]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            fold_v8i bo[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) bo[j] = fp4_db<SC>(u4w(B[j], t));
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const fold_v8i ao = fp4_sel<SC>(u4w(A[m], t));
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[m][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ao, bo[j], acc[m][j], kFoldFp4, kFoldFp4,
                                                                               0, kE8M0One, 0, kE8M0One);
            }
        }
    };
    uint4 sv[kPer];
    uint4 BA[SG][NT], BB[SG][NT];
    load_sel(s0, sv);
    load_db(s0, BA);
    // One staged block: its selection rows to LDS, the next block's loads
    // issued, then its super-groups folded.
    auto block = [&](uint64_t sb, const uint4 (&Bc)[SG][NT], uint4 (&Bn)[SG][NT]) __attribute__((always_inline)) {
        lds_barrier();                                          // previous block's operand reads are done
        store_sel(sv);
        lds_barrier();
        const uint64_t nb = sb + SG < s1 ? sb + SG : sb;        // next block (clamped)
        load_sel(nb, sv);
        load_db(nb, Bn);
        const uint64_t n = s1 - sb;
#pragma unroll
        for (int sl = 0; sl < SG; ++sl)
            if ((uint64_t)sl < n && nt != 0) fold_sg(sl, Bc[sl]);
    };
    uint64_t sb = s0;
    for (; sb + SG < s1; sb += 2 * SG) {
        block(sb, BA, BB);
        block(sb + SG, BB, BA);
    }
    if (sb < s1) block(sb, BA, BB);
    // Parities -> answer words, straight into the answers (C/D layout: lane =
    // column n, register e = rows (e&3) + 8(e>>2) + 4h).
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            uint32_t out = 0;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint32_t p = ((uint32_t)acc[m][j][e]) & 1u;
                const uint64_t b = __builtin_amdgcn_ballot_w64(p != 0);
                const uint32_t row0 = (e & 3) + 8 * (e >> 2);
                out = l == row0 ? (uint32_t)b : out;
                out = l == row0 + 4 ? (uint32_t)(b >> 32) : out;
            }
            if (l < 32 && 32u * m + l < kp && (uint32_t)j < nt) {
                uint32_t* o = ans + (key0 + 32u * m + l) * ntiles + tile0 + j;
                if (!atomic) *o = out;
                else if (out) atomicXor(o, out);
            }
        }
}

namespace {

struct GroupedMfmaFold {
    const uint32_t* bits;
    uint64_t wpk;
    const uint8_t* dbs;
    uint64_t gsg;
    uint32_t kpg, ntiles;
    uint32_t* ans;
    hipStream_t st;
};

template <int I>
hipError_t launch_shape(const GroupedMfmaFold& f, const dpfh::GroupFoldLaunch& l) {
    constexpr dpfh::FoldTile T = dpfh::kFoldTiles[I];
    constexpr int MT = T.MT, NT = T.NT, SG = T.SG, CG = T.CG, WPE = T.WPE, NW = 8 / NT * CG;
    const dpfh::GroupFoldPass& p = l.pass;
    if (p.kp > 32u * MT || p.cg != (uint32_t)CG) return hipErrorInvalidValue;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((uint32_t)l.blocks), dim3(64 * NW), 0, f.st, f.bits, f.wpk,
                           reinterpret_cast<const uint4*>(f.dbs), f.gsg, p.ncg, p.runs, p.spr, f.kpg, p.k0, p.kp, f.ntiles,
                           f.ans, l.u0, (uint32_t)(p.runs > 1));
    };
    if (f.ntiles % 8 == 0) launch(k_fold_grouped_mfma<MT, NT, SG, CG, WPE, true>);
    else launch(k_fold_grouped_mfma<MT, NT, SG, CG, WPE, false>);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_fold_grouped_mfma(const dpfh::GroupFoldKeysPlan& p, const uint32_t* bits, uint64_t words_per_key,
                                    const uint8_t* dbs, uint64_t rec_bytes, uint32_t* ans, hipStream_t st) {
    const GroupedMfmaFold f{bits, words_per_key, dbs, p.gsg, p.kpg, dpfh::rec_tiles(rec_bytes), ans, st};
    if (p.atomic())
        if (hipError_t e = launch_zero(ans, p.ngroups * p.kpg * rec_bytes, st); e != hipSuccess) return e;
    return p.for_each_launch([&](const dpfh::GroupFoldLaunch& l) {
        static_assert(dpfh::kFoldTileCount == 7, "one case per tile shape");
        switch (l.pass.shape) {
            case 0: return launch_shape<0>(f, l);
            case 1: return launch_shape<1>(f, l);
            case 2: return launch_shape<2>(f, l);
            case 3: return launch_shape<3>(f, l);
            case 4: return launch_shape<4>(f, l);
            case 5: return launch_shape<5>(f, l);
            default: return launch_shape<6>(f, l);
        }
    });
}

}  // namespace dpfk
