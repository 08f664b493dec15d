// pir_export_plan.hpp — host-side planning of dpf_pir_db_export and
// dpf_pir_db_xor_records: a caller range [first, first + n) of record indices
// as an ordered list of pieces, each a run of whole super-groups of one shard
// that goes through a bounded staging buffer.  The same plan serves the
// read-out (un-slice the piece, copy rows down) and the merge (rows up into a
// zeroed piece, slice, XOR into the shard).  Host-only and header-only (no
// HIP), so tests/c/pir_export_plan_test.cpp runs it under ASan/UBSan without
// a device.
//
// What the plan guarantees, and no kernel can check:
//   - the pieces deliver the caller's records first .. first + n - 1 exactly
//     once and in order: piece k's rows go to out, out + 1, ..., and piece
//     k + 1 starts where piece k ended;
//   - a piece starts at a local multiple of 256 of its shard (a contiguous
//     sub-range of the sliced layout), un-slices whole super-groups or up to
//     the shard's end, stays inside the shard and is no larger than the chunk;
//   - the zero records behind a group's nrec (grouped handles) and the rows
//     behind a shard's last record are never delivered.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "pir_group_plan.hpp"
#include "pir_update_plan.hpp"

namespace dpfh {

enum class ExportKind { Dense, Sparse, Grouped };

struct ExportPiece {
    size_t shard;
    uint64_t local0;   // first record of the piece in the shard's flat positions, a multiple of 256
    uint64_t nrec;     // records to un-slice (or slice) from there: whole super-groups, or up to the shard's end
    uint64_t skip;     // rows of the piece in front of the first wanted one
    uint64_t take;     // wanted rows: piece rows [skip, skip + take)
    uint64_t out;      // the caller's row (record first + out) the first of them is
};

// The staging chunk in records: whole super-groups, at least one.
inline uint64_t export_chunk(uint64_t chunk_records) { return std::max<uint64_t>(256, chunk_records / 256 * 256); }

// Local records [a, b) of shard s (len flat positions long), one contiguous
// run of the caller's rows from `out` on, in pieces of at most `chunk`.
inline void export_run(size_t s, uint64_t len, uint64_t a, uint64_t b, uint64_t out, uint64_t chunk,
                       std::vector<ExportPiece>* pieces) {
    while (a < b) {
        const uint64_t l0 = a / 256 * 256;
        const uint64_t end = std::min(b, std::min(l0 + chunk, len));          // wanted rows end here
        const uint64_t upto = std::min(len, (end + 255) / 256 * 256);        // (len - l0 < 2^64 - 255: no overflow)
        pieces->push_back(ExportPiece{s, l0, upto - l0, a - l0, end - a, out});
        out += end - a;
        a = end;
    }
}

// Plans [first, first + n) of a handle's index space into *pieces (cleared
// first).  ranges: the handle's shard ranges (dense_shards, sparse_shards,
// grouped_shards) over nshards shards.  Dense and sparse: the index is the
// position in ranges' record space.  Grouped: ngroups groups of gnrec records,
// caller index g * gnrec + i at flat position g * group_stride(gnrec) + i, and
// ranges in flat positions; a piece never crosses a group's padding.  Returns
// false, *pieces empty, where the range leaves the index space (first + n
// overflowing included).  chunk_records: export_chunk() of it is used.
inline bool plan_export(ExportKind kind, uint64_t first, uint64_t n, uint64_t chunk_records, const ShardRanges& ranges,
                        size_t nshards, uint64_t ngroups, uint64_t gnrec, std::vector<ExportPiece>* pieces) {
    pieces->clear();
    const uint64_t total = kind == ExportKind::Grouped ? ngroups * gnrec : ranges.nrec;
    if (first > total || n > total - first) return false;
    if (n == 0) return true;
    const uint64_t chunk = export_chunk(chunk_records), last = first + n;
    const uint64_t gs = group_stride(gnrec);
    if (kind != ExportKind::Grouped || gs == gnrec) {
        // The index is the flat position: shard by shard.
        for (size_t s = (size_t)(first / ranges.slice); s < nshards && ranges.lo(s) < last; ++s) {
            const uint64_t lo = ranges.lo(s), hi = ranges.hi(s);
            const uint64_t a = std::max(first, lo), b = std::min(last, hi);
            if (a < b) export_run(s, hi - lo, a - lo, b - lo, a - first, chunk, pieces);
        }
        return true;
    }
    // Group by group: group g is gs flat positions of its shard, gnrec of them records.
    const uint64_t gps = ranges.slice / gs;
    for (uint64_t g = first / gnrec; g < ngroups && g * gnrec < last; ++g) {
        const size_t s = (size_t)(g / gps);
        const uint64_t base = (g - (uint64_t)s * gps) * gs;                   // the group's first local position
        const uint64_t a = std::max(first, g * gnrec), b = std::min(last, (g + 1) * gnrec);
        export_run(s, ranges.hi(s) - ranges.lo(s), base + (a - g * gnrec), base + (b - g * gnrec), a - first, chunk,
                   pieces);
    }
    return true;
}

}  // namespace dpfh
