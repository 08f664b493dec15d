// pir_export_plan_test.cpp — the piece plan of dpf_pir_db_export and
// dpf_pir_db_xor_records (dpf-go_amd/csrc/pir_export_plan.hpp) as a
// stand-alone program.  Over kinds (dense, sparse, grouped) x shard counts
// {1, 2, 3, 8} (dense: the powers of two) x record counts around super-group
// and shard boundaries x group sizes {1, 255, 256, 257, 300} x ranges (empty,
// one record, all, starting or ending one off a boundary, across a shard or
// group boundary) x chunk sizes {256, 512, 1280, ...}:
//   - every wanted record is delivered exactly once and in order, from the
//     shard and local position that the handle's own layout rule gives it
//     (restated here from ShardRanges / group_flat, not taken from the plan);
//   - every piece starts on a local multiple of 256, un-slices whole
//     super-groups or up to its shard's end, stays inside its shard, does not
//     exceed the chunk and takes at least one row;
//   - no pad record (behind a group's nrec, behind a shard's end) is delivered;
//   - a range that leaves the index space, first + n overflowing included,
//     is refused with no piece.
// Built with -fsanitize=address,undefined and run directly by
// tests/test_export_plan_cpu.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <set>
#include <vector>

#include "pir_export_plan.hpp"

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
static uint64_t g_plans = 0, g_pieces = 0, g_rows = 0, g_refused = 0;

// A handle's layout, as capi_pir_db.hip sets it up.
struct Layout {
    ExportKind kind;
    ShardRanges ranges;
    size_t nshards;
    uint64_t ngroups, gnrec, total;
    // Where the layout rule puts caller index v.
    void where(uint64_t v, size_t* shard, uint64_t* local) const {
        const uint64_t f = kind == ExportKind::Grouped ? group_flat(v, gnrec) : v;
        *shard = (size_t)(f / ranges.slice);
        *local = f - ranges.lo(*shard);
    }
};

static void check_range(const Layout& L, uint64_t first, uint64_t n, uint64_t chunk_records) {
#define AT "kind=%d shards=%zu total=%llu gnrec=%llu first=%llu n=%llu chunk=%llu", (int)L.kind, L.nshards, (ull)L.total, (ull)L.gnrec, (ull)first, (ull)n, (ull)chunk_records
    std::vector<ExportPiece> pieces(3);   // stale content must go
    const bool ok = plan_export(L.kind, first, n, chunk_records, L.ranges, L.nshards, L.ngroups, L.gnrec, &pieces);
    ++g_plans;
    const bool inside = first <= L.total && n <= L.total - first;
    CHECK(ok == inside, AT);
    if (!ok || !inside) {
        ++g_refused;
        CHECK(pieces.empty(), AT);
        return;
    }
    const uint64_t chunk = export_chunk(chunk_records);
    CHECK(chunk % 256 == 0 && chunk >= 256 && (chunk_records < 256 || chunk <= chunk_records), AT);
    uint64_t done = 0;
    for (const ExportPiece& p : pieces) {
        ++g_pieces;
        CHECK(p.shard < L.nshards, AT);
        if (p.shard >= L.nshards) return;
        const uint64_t len = L.ranges.hi(p.shard) - L.ranges.lo(p.shard);
        CHECK(p.local0 % 256 == 0, AT);
        CHECK(p.nrec >= 1 && p.nrec <= chunk, AT);
        CHECK(p.local0 + p.nrec <= len, AT);
        CHECK(p.nrec % 256 == 0 || p.local0 + p.nrec == len, AT);
        CHECK(p.take >= 1 && p.skip + p.take <= p.nrec, AT);
        CHECK(p.out == done, AT);                                   // in order, no gap, no overlap
        if (p.out != done || p.skip + p.take > p.nrec) return;
        for (uint64_t k = 0; k < p.take; ++k) {
            size_t s = 0;
            uint64_t l = 0;
            L.where(first + done + k, &s, &l);
            if (s != p.shard || l != p.local0 + p.skip + k) {
                CHECK(false, AT);
                return;
            }
            if (L.kind == ExportKind::Grouped) {
                const uint64_t gs = group_stride(L.gnrec);
                CHECK((p.local0 + p.skip + k) % gs < L.gnrec, AT);   // never a pad record
            }
        }
        done += p.take;
        g_rows += p.take;
    }
    CHECK(done == n, AT);
    if (n == 0) CHECK(pieces.empty(), AT);
#undef AT
}

// Every range the issue names, around the boundaries of the layout.
static void check_layout(const Layout& L) {
    std::set<uint64_t> bounds = {0, L.total};
    for (uint64_t b = 256; b < L.total; b += 256) bounds.insert(b);
    if (L.kind != ExportKind::Grouped)
        for (size_t s = 0; s < L.nshards; ++s) bounds.insert(L.ranges.lo(s));
    else
        for (uint64_t g = 0; g <= L.ngroups; ++g) bounds.insert(g * L.gnrec);
    const uint64_t chunks[] = {256, 512, 1280, 0, 300, 1ull << 20};
    for (uint64_t chunk : chunks) {
        check_range(L, 0, 0, chunk);
        check_range(L, L.total, 0, chunk);
        check_range(L, 0, L.total, chunk);
        check_range(L, L.total, 1, chunk);                              // outside
        check_range(L, L.total + 1, 0, chunk);
        check_range(L, 0, L.total + 1, chunk);
        check_range(L, 1, UINT64_MAX, chunk);                           // first + n overflows
        check_range(L, UINT64_MAX, 2, chunk);
        for (uint64_t b : bounds) {
            for (int d0 = -1; d0 <= 1; ++d0) {
                if ((d0 < 0 && b == 0) || b + d0 > L.total) continue;
                const uint64_t f = b + d0;
                check_range(L, f, std::min<uint64_t>(1, L.total - f), chunk);      // one record
                check_range(L, f, std::min<uint64_t>(2, L.total - f), chunk);      // across the boundary
                check_range(L, f, L.total - f, chunk);                              // to the end
                check_range(L, 0, f, chunk);                                        // from the start
                check_range(L, f, std::min<uint64_t>(258, L.total - f), chunk);
                check_range(L, f, std::min<uint64_t>(1000, L.total - f), chunk);
                const uint64_t f2 = f >= 300 ? f - 300 : 0;
                check_range(L, f2, std::min<uint64_t>(600, L.total - f2), chunk);
            }
        }
    }
}

int main() {
    const uint64_t nrecs[] = {0, 1, 2, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513, 767, 768, 769, 1000, 1023, 1024,
                              1025, 2047, 2048, 2049, 3000};
    // Dense: 2^pbits shards of 2^(logN - pbits) records, nrec <= 2^logN (the last shards may be short or empty).
    for (uint32_t pbits : {0u, 1u, 3u})
        for (uint64_t nrec : nrecs)
            for (uint32_t logN = 7 + pbits; logN <= 13; ++logN) {
                if (nrec > (1ull << logN)) continue;
                const Layout L{ExportKind::Dense, dense_shards(nrec, logN, pbits), (size_t)1 << pbits, 0, 0, nrec};
                check_layout(L);
            }
    // Sparse: an even split in whole super-groups.
    for (size_t nshards : {1, 2, 3, 8})
        for (uint64_t nrec : nrecs) {
            const Layout L{ExportKind::Sparse, sparse_shards(nrec, nshards), nshards, 0, 0, nrec};
            check_layout(L);
        }
    // Grouped: whole groups per shard, zero records behind each group's gnrec.
    for (size_t nshards : {1, 2, 3, 8})
        for (uint64_t gnrec : {1, 255, 256, 257, 300, 512, 700})
            for (uint64_t ngroups : {0, 1, 2, 3, 5, 8, 9}) {
                const Layout L{ExportKind::Grouped, grouped_shards(ngroups, gnrec, nshards), nshards, ngroups, gnrec,
                               ngroups * gnrec};
                check_layout(L);
            }
    // A grouped handle without records per group.
    {
        const Layout L{ExportKind::Grouped, grouped_shards(4, 0, 2), 2, 4, 0, 0};
        check_range(L, 0, 0, 256);
        check_range(L, 0, 1, 256);
    }
    printf("plans=%llu refused=%llu pieces=%llu rows=%llu\n", (ull)g_plans, (ull)g_refused, (ull)g_pieces, (ull)g_rows);
    if (g_fail) {
        printf("pir_export_plan FAILED: %d checks\n", g_fail);
        return 1;
    }
    printf("pir_export_plan ok\n");
    return 0;
}
