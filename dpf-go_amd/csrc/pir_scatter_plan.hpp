// pir_scatter_plan.hpp — how launch_scatter_sliced (pir_db_ops.hip) covers a
// private write: which super-groups, columns and keys each k_scatter_sliced
// workgroup takes, and how the workgroups fall into launches.  Pure functions
// of (nrec, C, nkeys, CU count, limits); host-only and header-only (no HIP), so
// tests/c/pir_scatter_plan_test.cpp runs them under ASan/UBSan without a device.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "pir_fold_plan.hpp"

namespace dpfh {

constexpr uint32_t kScatterKeyTile = 64;          // KT: keys per pass over the DB (a thread's message bits: 2 words)
constexpr uint32_t kScatterMaxCols = 4;           // 32-byte columns per workgroup (they share the staged selection words)
constexpr uint32_t kScatterPerCu = 4;             // workgroups per CU the run length aims at

// One workgroup's work: super-groups [s0, s1) of columns [c0, c1), keys [k0, k1).
struct ScatterUnit {
    uint64_t s0, s1;
    uint32_t c0, c1;
    uint64_t k0, k1;
};

// The DB's nsg super-groups are cut into runs of `run`, its C columns into ncg
// groups of `cols` (the last one may be shorter), the keys into tiles of
// kScatterKeyTile.  Workgroup u of a key tile is (run u / ncg, column group
// u % ncg), so the workgroups that read the same selection words are
// neighbours; a launch takes per_launch consecutive workgroups of one key
// tile.  Key tiles are launches of their own, in stream order: two tiles
// rewrite the same DB words.
struct ScatterPlan {
    uint64_t nsg = 0, nkeys = 0;
    uint32_t C = 0, cols = 1, ncg = 0;
    uint64_t run = 1, nruns = 0;
    uint64_t units = 0;        // workgroups per key tile = nruns * ncg
    uint64_t per_launch = 1;   // workgroups per launch (<= max_blocks)

    uint64_t key_tiles() const { return units == 0 ? 0 : (nkeys + kScatterKeyTile - 1) / kScatterKeyTile; }
    uint64_t launches() const { return (units + per_launch - 1) / per_launch; }   // per key tile
    uint64_t first(uint64_t launch) const { return launch * per_launch; }
    uint64_t blocks(uint64_t launch) const { return std::min(per_launch, units - first(launch)); }
    ScatterUnit unit(uint64_t tile, uint64_t u) const {
        const uint64_t r = u / ncg;
        const uint32_t c0 = (uint32_t)(u % ncg) * cols;
        const uint64_t k0 = tile * kScatterKeyTile;
        return {r * run, std::min(nsg, (r + 1) * run), c0, std::min(C, c0 + cols), k0,
                std::min(nkeys, k0 + kScatterKeyTile)};
    }
};

// max_blocks / max_sg: dpf_set_fold_limits' values (0 = the defaults of
// pir_fold_plan.hpp; larger ones are cut to them).  C >= 1.  Nothing to do
// (units == 0) when nrec == 0 or nkeys == 0.
inline ScatterPlan plan_scatter(uint64_t nrec, uint32_t C, uint64_t nkeys, uint32_t cus, uint32_t max_blocks,
                                uint32_t max_sg) {
    ScatterPlan p;
    p.nsg = nrec / 256 + (nrec % 256 != 0);
    p.nkeys = nkeys;
    p.C = C;
    if (p.nsg == 0 || nkeys == 0 || C == 0) return p;
    const FoldLimits lim = clamp_fold_limits(max_blocks, max_sg);
    const uint64_t cap = lim.max_blocks, msg = lim.max_sg;
    // Column groups of equal size (5 columns: 3 + 2, not 4 + 1).
    p.ncg = (C + kScatterMaxCols - 1) / kScatterMaxCols;
    p.cols = (C + p.ncg - 1) / p.ncg;
    p.ncg = (C + p.cols - 1) / p.cols;
    // Runs long enough that one launch of about kScatterPerCu workgroups per
    // CU covers the DB (a run's prologue reads the messages), never longer
    // than max_sg.
    const uint64_t want = std::min<uint64_t>(cap, (uint64_t)std::max(cus, 1u) * kScatterPerCu);
    const uint64_t xruns = std::max<uint64_t>(1, want / p.ncg);
    p.run = std::min(msg, (p.nsg + xruns - 1) / xruns);
    p.nruns = (p.nsg + p.run - 1) / p.run;
    p.units = p.nruns * p.ncg;
    p.per_launch = std::min(cap, p.units);
    return p;
}

}  // namespace dpfh
