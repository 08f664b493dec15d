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
// The fold itself is fold_mfma_body.inc, the one loop this kernel and
// k_fold_mfma share as text: the wave decode, selection staging, the
// double-buffered block loop, the operand expansion, the MFMA nest and the
// ballot epilogue.  The kernel below is what differs, as the macros that file
// names: the unit decode, where the tile's selection rows start, the address
// of a DB tile, and answers written straight to d_ans (store or atomic XOR)
// instead of partials.  Every instantiation compiles to the instructions it
// had with a loop of its own (tools/fold_isa_compare.py,
// profiles/fold_shared_body/).
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
#define FOLD_UNIT                                                                            \
    const dpfh::GroupUnit un = dpfh::group_unit(u0 + blockIdx.x, runs, spr, gsg, ncg);        \
    const uint64_t s0 = un.s0, s1 = un.s1;      /* never empty (the plan) */                  \
    const uint64_t key0 = un.g * kpg + k0;      /* first selection / answer row of the tile */ \
    const uint32_t* sel = bits + key0 * wlim;                                                 \
    const uint64_t stride = wlim;                                                             \
    const uint32_t nrows = kp;                                                                \
    constexpr bool NTDB = false;                /* not instantiated (not measured) */         \
    const uint64_t col0 = (uint64_t)un.c * CG;
#define FOLD_RUN
#define FOLD_DB_AT(S, j) group_tile(dbs, un.g, gsg, S, 32 * ntiles, (tile0 + j) * 32 + r) + h
#define FOLD_EMIT_BEGIN
#define FOLD_EMIT(m, j, out)                                        \
    if (l < 32 && 32u * m + l < kp && (uint32_t)j < nt) {           \
        uint32_t* o = ans + (key0 + 32u * m + l) * ntiles + tile0 + j; \
        if (!atomic) *o = out;                                      \
        else if (out) atomicXor(o, out);                            \
    }
#include "fold_mfma_body.inc"
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
        return dpfh::with_fold_tile((int)l.pass.shape,
                                    [&](auto shape) { return launch_shape<decltype(shape)::value>(f, l); });
    });
}

}  // namespace dpfk
