// pir_update_plan.hpp — host-side planning of dpf_pir_db_update / _read: range
// check, stable sort, keep-last dedupe and the split by shard.  Host-only and
// header-only (no HIP), so tests/c/pir_update_plan_test.cpp runs it under
// ASan/UBSan without a device.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "pir_window_plan.hpp"

namespace dpfh {

constexpr size_t kPlanRadixMin = 4096;   // entries from which the planner sorts by radix

// Entries [shard_off[s], shard_off[s + 1]) belong to shard s (2^pbits shards,
// a record's shard is idx >> (logN - pbits); a sparse handle's shards are
// record ranges, plan_pir_update_ranges); within a shard `local` (the
// index inside the shard) is non-decreasing.  src[k] is the position in the
// caller's arrays that entry k came from.
struct PirUpdatePlan {
    std::vector<uint64_t> local;
    std::vector<size_t> src;
    std::vector<size_t> shard_off;
};

// Which of a handle's nrec records its shards hold: shard g has [lo(g), hi(g)),
// consecutive ranges of `slice` records cut off at nrec.  The handle uploads
// by these ranges and the planners below split by the same slice, so local
// index l of shard g is record lo(g) + l (tests/c/pir_update_plan_test.cpp).
struct ShardRanges {
    uint64_t nrec = 0, slice = 0;
    uint64_t lo(size_t g) const { return std::min<uint64_t>(nrec, (uint64_t)g * slice); }
    uint64_t hi(size_t g) const { return std::min<uint64_t>(nrec, lo(g) + slice); }
};
// Dense: shard g is the DB's part under subtree (pbits, g), 2^(logN - pbits)
// records (plan_pir_update).
inline ShardRanges dense_shards(uint64_t nrec, uint32_t logN, uint32_t pbits) {
    return ShardRanges{nrec, 1ull << (logN - pbits)};
}
// Sparse, and the ranged dense kind: the balanced split in whole super-groups
// of 256 records (pir_window_plan.hpp balanced_slice; plan_pir_update_ranges
// with cap = slice).
inline ShardRanges sparse_shards(uint64_t nrec, size_t nshards) {
    return ShardRanges{nrec, balanced_slice(nrec, (uint64_t)nshards)};
}

// The planner behind both shardings below: split(v, &shard, &local) places
// index v (shards ascending with v), nshards of them.
template <class Split>
inline bool plan_pir_update_split(const uint64_t* idx, size_t n, uint64_t nrec, size_t nshards, bool keep_last,
                                  Split split, PirUpdatePlan* plan) {
    for (size_t i = 0; i < n; ++i)
        if (idx[i] >= nrec) return false;
    // (index, position) pairs in index order, equal indices in the caller's
    // order: nothing to do for a caller that sends them sorted; a stable LSD
    // radix sort over the bits of nrec - 1 for large batches (2^20 entries:
    // ~10 ms against ~100 for a comparison sort), std::stable_sort below that.
    struct Ent {
        uint64_t v;
        size_t pos;
    };
    std::vector<Ent> e(n);
    bool sorted = true;
    for (size_t i = 0; i < n; ++i) {
        e[i] = Ent{idx[i], i};
        if (i && idx[i] < idx[i - 1]) sorted = false;
    }
    if (!sorted && n < kPlanRadixMin) {
        std::stable_sort(e.begin(), e.end(), [](const Ent& a, const Ent& b) { return a.v < b.v; });
    } else if (!sorted) {
        constexpr uint32_t kDigit = 11;
        std::vector<Ent> tmp(n);
        std::vector<size_t> cnt((size_t)1 << kDigit);
        for (uint32_t sh = 0; sh < 64 && ((nrec - 1) >> sh) != 0; sh += kDigit) {
            std::fill(cnt.begin(), cnt.end(), (size_t)0);
            for (const Ent& x : e) ++cnt[(x.v >> sh) & ((1u << kDigit) - 1)];
            size_t at = 0;
            for (size_t& c : cnt) {
                const size_t k = c;
                c = at;
                at += k;
            }
            for (const Ent& x : e) tmp[cnt[(x.v >> sh) & ((1u << kDigit) - 1)]++] = x;
            e.swap(tmp);
        }
    }
    PirUpdatePlan p;
    p.shard_off.assign(nshards + 1, 0);
    p.local.reserve(n);
    p.src.reserve(n);
    for (size_t k = 0; k < n; ++k) {
        const uint64_t v = e[k].v;
        if (keep_last && k + 1 < n && e[k + 1].v == v) continue;
        size_t shard = 0;
        uint64_t local = 0;
        split(v, &shard, &local);
        p.local.push_back(local);
        p.src.push_back(e[k].pos);
        ++p.shard_off[shard + 1];
    }
    for (size_t s = 1; s < p.shard_off.size(); ++s) p.shard_off[s] += p.shard_off[s - 1];
    *plan = std::move(p);
    return true;
}

// Plans n caller indices for a DB of nrec <= 2^logN records over 2^pbits
// shards (pbits <= logN <= 63).  Returns false, with *plan untouched, if any
// index is >= nrec.  The entries are stably sorted by index; with keep_last
// only the last occurrence of each index stays (an update: the last wins),
// without it every entry stays (a read: duplicates are answered twice).
inline bool plan_pir_update(const uint64_t* idx, size_t n, uint64_t nrec, uint32_t logN, uint32_t pbits, bool keep_last,
                            PirUpdatePlan* plan) {
    const uint32_t shift = logN - pbits;
    const uint64_t mask = (1ull << shift) - 1;
    return plan_pir_update_split(idx, n, nrec, (size_t)1 << pbits, keep_last,
                                 [=](uint64_t v, size_t* shard, uint64_t* local) {
                                     *shard = (size_t)(v >> shift);
                                     *local = v & mask;
                                 },
                                 plan);
}

// The same for a sparse handle: shard s holds the records [s * cap, (s + 1) *
// cap) of the list (cap > 0 whenever nrec > 0), nshards of them.
inline bool plan_pir_update_ranges(const uint64_t* idx, size_t n, uint64_t nrec, uint64_t cap, size_t nshards,
                                   bool keep_last, PirUpdatePlan* plan) {
    return plan_pir_update_split(idx, n, nrec, nshards, keep_last,
                                 [=](uint64_t v, size_t* shard, uint64_t* local) {
                                     *shard = (size_t)(v / cap);
                                     *local = v % cap;
                                 },
                                 plan);
}

}  // namespace dpfh
