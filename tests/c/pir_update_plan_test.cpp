// Stand-alone check of the host planner of dpf_pir_db_update / _read
// (dpf-go_amd/csrc/pir_update_plan.hpp): built with -fsanitize=address,undefined
// and run directly by tests/test_pir_update_cpu.py.  No device, no library.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pir_update_plan.hpp"

using dpfh::PirUpdatePlan;
using dpfh::plan_pir_update;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                                    \
        }                                                               \
    } while (0)

template <class T>
static bool same(const std::vector<T>& a, std::initializer_list<unsigned long long> b) {
    return a == std::vector<T>(b.begin(), b.end());
}

int main() {
    // Stable sort: equal indices keep the caller's order (a read keeps them all).
    {
        const uint64_t idx[] = {7, 3, 7, 0, 3, 7};
        PirUpdatePlan p;
        CHECK(plan_pir_update(idx, 6, 8, 3, 0, false, &p));
        CHECK(same(p.local, {0, 3, 3, 7, 7, 7}));
        CHECK(same(p.src, {3, 1, 4, 0, 2, 5}));
        CHECK(same(p.shard_off, {0, 6}));
    }
    // Keep-last dedupe: of each index only its last occurrence.
    {
        const uint64_t idx[] = {7, 3, 7, 0, 3, 7};
        PirUpdatePlan p;
        CHECK(plan_pir_update(idx, 6, 8, 3, 0, true, &p));
        CHECK(same(p.local, {0, 3, 7}));
        CHECK(same(p.src, {3, 4, 5}));
        CHECK(same(p.shard_off, {0, 3}));
    }
    // One index out of range (nrec = 5 < 2^logN): rejected, the plan untouched.
    {
        const uint64_t idx[] = {1, 5, 2};
        PirUpdatePlan p;
        p.local = {42};
        p.src = {9};
        p.shard_off = {0, 1};
        CHECK(!plan_pir_update(idx, 3, 5, 3, 0, true, &p));
        CHECK(same(p.local, {42}) && same(p.src, {9}) && same(p.shard_off, {0, 1}));
        const uint64_t big[] = {0, ~0ull};
        CHECK(!plan_pir_update(big, 2, 5, 3, 1, false, &p));
        CHECK(same(p.local, {42}));
    }
    // n = 0: an empty plan with every shard empty.
    {
        PirUpdatePlan p;
        CHECK(plan_pir_update(nullptr, 0, 100, 10, 3, true, &p));
        CHECK(p.local.empty() && p.src.empty());
        CHECK(p.shard_off == std::vector<size_t>(9, 0));
    }
    // Shard split, logN = 6 (64 records): pbits 1 -> shards of 32, pbits 3 ->
    // shards of 8; indices at exact shard boundaries, empty shards, one
    // duplicate across the split.
    {
        const uint64_t idx[] = {32, 31, 0, 63, 8, 7, 32, 16};
        PirUpdatePlan p;
        CHECK(plan_pir_update(idx, 8, 64, 6, 0, true, &p));
        CHECK(same(p.local, {0, 7, 8, 16, 31, 32, 63}));
        CHECK(same(p.src, {2, 5, 4, 7, 1, 6, 3}));
        CHECK(same(p.shard_off, {0, 7}));

        CHECK(plan_pir_update(idx, 8, 64, 6, 1, true, &p));
        CHECK(same(p.local, {0, 7, 8, 16, 31, 0, 31}));
        CHECK(same(p.src, {2, 5, 4, 7, 1, 6, 3}));
        CHECK(same(p.shard_off, {0, 5, 7}));

        CHECK(plan_pir_update(idx, 8, 64, 6, 3, true, &p));
        CHECK(same(p.local, {0, 7, 0, 0, 7, 0, 7}));
        CHECK(same(p.src, {2, 5, 4, 7, 1, 6, 3}));
        //                 shard 0: 0,7 | 1: 8 | 2: 16 | 3: 31 | 4: 32 | 5, 6: none | 7: 63
        CHECK(same(p.shard_off, {0, 2, 3, 4, 5, 6, 6, 6, 7}));

        CHECK(plan_pir_update(idx, 8, 64, 6, 3, false, &p));   // a read keeps both 32s, in order
        CHECK(same(p.local, {0, 7, 0, 0, 7, 0, 0, 7}));
        CHECK(same(p.src, {2, 5, 4, 7, 1, 0, 6, 3}));
        CHECK(same(p.shard_off, {0, 2, 3, 4, 5, 7, 7, 7, 8}));
    }
    // A short DB: nrec = 20 of 2^6 over 4 shards of 16; shards 2 and 3 hold nothing.
    {
        const uint64_t idx[] = {19, 16, 15};
        PirUpdatePlan p;
        CHECK(plan_pir_update(idx, 3, 20, 6, 2, true, &p));
        CHECK(same(p.local, {15, 0, 3}));
        CHECK(same(p.shard_off, {0, 1, 3, 3, 3}));
        const uint64_t bad[] = {19, 20};
        CHECK(!plan_pir_update(bad, 2, 20, 6, 2, true, &p));
    }
    // pbits == logN (one record per shard) and logN = 63.
    {
        const uint64_t idx[] = {3, 0, 3};
        PirUpdatePlan p;
        CHECK(plan_pir_update(idx, 3, 4, 2, 2, true, &p));
        CHECK(same(p.local, {0, 0}));
        CHECK(same(p.src, {1, 2}));
        CHECK(same(p.shard_off, {0, 1, 1, 1, 2}));
        const uint64_t hi[] = {(1ull << 63) - 1, 1ull << 62};
        CHECK(plan_pir_update(hi, 2, 1ull << 63, 63, 1, true, &p));
        CHECK(same(p.local, {0, (1ull << 62) - 1}));
        CHECK(same(p.shard_off, {0, 0, 2}));
    }
    // Large batches (the radix sort) against std::stable_sort: 20000 indices
    // with many repeats over 3 shards' worth of a 2^40-record DB, both modes.
    {
        const size_t n = 20000;
        CHECK(n >= dpfh::kPlanRadixMin);
        const uint64_t nrec = (3ull << 38) - 5;
        std::vector<uint64_t> idx(n);
        uint64_t s = 88172645463325252ull;
        for (size_t i = 0; i < n; ++i) {
            s ^= s << 13, s ^= s >> 7, s ^= s << 17;                  // xorshift64
            idx[i] = i % 3 == 0 ? (s % 500) << 29 : s % nrec;         // every third from a set of 500
        }
        std::vector<size_t> ref(n);
        for (size_t i = 0; i < n; ++i) ref[i] = i;
        std::stable_sort(ref.begin(), ref.end(), [&](size_t a, size_t b) { return idx[a] < idx[b]; });
        PirUpdatePlan p;
        CHECK(plan_pir_update(idx.data(), n, nrec, 40, 2, false, &p));
        CHECK(p.src == ref);
        for (size_t k = 0; k < n; ++k) CHECK(p.local[k] == (idx[ref[k]] & ((1ull << 38) - 1)));
        CHECK(p.shard_off.size() == 5 && p.shard_off[3] == n && p.shard_off[4] == n && p.shard_off[1] > 0);
        CHECK(plan_pir_update(idx.data(), n, nrec, 40, 2, true, &p));
        std::vector<size_t> last;
        for (size_t k = 0; k < n; ++k)
            if (k + 1 == n || idx[ref[k + 1]] != idx[ref[k]]) last.push_back(ref[k]);
        CHECK(p.src == last && last.size() < n);
        // already sorted input of the same size: the no-sort path
        std::vector<uint64_t> srt(n);
        for (size_t k = 0; k < n; ++k) srt[k] = idx[ref[k]];
        CHECK(plan_pir_update(srt.data(), n, nrec, 40, 2, false, &p));
        for (size_t k = 0; k < n; ++k) CHECK(p.src[k] == k);
    }
    // The shards' record ranges (what the handle uploads) against the planners
    // (where an update lands): the ranges tile [0, nrec) in order, sparse ones
    // start on whole super-groups, and every index the planner places in
    // shard s at local l is record lo(s) + l of a shard that holds it.
    {
        const uint64_t nrecs[] = {0, 1, 255, 256, 257, 1000, (1ull << 20) + 1};
        const uint32_t logN = 21;
        auto check = [](const dpfh::ShardRanges& r, size_t nshards, bool sparse, uint32_t pbits) {
            uint64_t at = 0;
            for (size_t g = 0; g < nshards; ++g) {
                CHECK(r.lo(g) == at && r.hi(g) >= r.lo(g) && r.hi(g) <= r.nrec);
                if (sparse) CHECK(r.lo(g) % 256 == 0 || r.lo(g) == r.nrec);
                at = r.hi(g);
            }
            CHECK(at == r.nrec);
            // Both edges of every shard, and a stride through the records, out of order.
            std::vector<uint64_t> idx;
            for (size_t g = 0; g < nshards; ++g)
                if (r.hi(g) > r.lo(g)) idx.push_back(r.hi(g) - 1), idx.push_back(r.lo(g));
            for (uint64_t v = 0; v < r.nrec; v += r.nrec / 61 + 1) idx.push_back(r.nrec - 1 - v);
            PirUpdatePlan p;
            CHECK(sparse ? dpfh::plan_pir_update_ranges(idx.data(), idx.size(), r.nrec, r.slice, nshards, false, &p)
                         : plan_pir_update(idx.data(), idx.size(), r.nrec, logN, pbits, false, &p));
            CHECK(p.shard_off.size() == nshards + 1 && p.shard_off[nshards] == idx.size());
            for (size_t s = 0; s < nshards; ++s)
                for (size_t k = p.shard_off[s]; k < p.shard_off[s + 1]; ++k)
                    CHECK(r.lo(s) + p.local[k] == idx[p.src[k]] && idx[p.src[k]] < r.hi(s));
        };
        for (uint64_t nrec : nrecs) {
            for (uint32_t pbits : {0u, 1u, 3u}) check(dpfh::dense_shards(nrec, logN, pbits), (size_t)1 << pbits, false, pbits);
            for (size_t nshards : {1, 2, 3, 8}) check(dpfh::sparse_shards(nrec, nshards), nshards, true, 0);
        }
        // The sparse split is even in whole super-groups: 1000 records over 3 -> 512, 488, 0.
        const dpfh::ShardRanges r = dpfh::sparse_shards(1000, 3);
        CHECK(r.slice == 512 && r.hi(0) == 512 && r.lo(1) == 512 && r.hi(1) == 1000 && r.lo(2) == 1000 && r.hi(2) == 1000);
    }
    printf("pir_update_plan ok\n");
    return 0;
}
