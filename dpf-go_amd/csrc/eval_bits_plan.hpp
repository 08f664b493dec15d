// eval_bits_plan.hpp — the host arithmetic behind k_eval_bits (dpf_kernels.hip):
// every key evaluated at a list of points, the answers left as packed
// selection-bit rows bits[nkeys][bits_stride] in EvalFull's bit order (point j
// = bit j % 8 of byte j / 8).  The lists are xs[nlists][npts], tightly packed:
// key k is evaluated at list k / keys_per_list, so one shared list is the case
// keys_per_list = nkeys, and the keys of group g of a grouped call
// (keys_per_list = keys per group) meet group g's own points.
// Host-only and header-only (no HIP), so tests/c/eval_bits_plan_test.cpp and
// tests/c/eval_bits_group_plan_test.cpp replay it under ASan/UBSan without a device.
// The launcher asks this header and launches what it says; the kernel's index
// arithmetic is the functions below, called from device code as they stand.
//
// Unit-to-wave mapping: a unit is 128 consecutive points of one key and is one
// wave's work.  Wave w of the grid owns (key w / units, unit w % units), so the
// waves of a key follow one another and every wave has a uniform key at every
// npts.  Lane l takes points 128 u + l and 128 u + 64 + l (the (l, l + 64)
// pairing): the ballots of the lanes' first and second answers are the unit's
// low and high 64 bits as they stand, and lane 0 stores them as one 16-byte
// vector store at byte 16 u of the key's row.
//
// Tail rule: every point list is padded virtually to a multiple of 128.  A lane
// whose point index is >= npts reads point npts - 1 of its key's OWN list
// instead (so no load leaves that list, xs[list * npts, (list + 1) * npts))
// and is masked out of the ballot, so the bits at positions >=
// npts of the last unit's span are zero.  A row's written bytes are exactly
// [0, 16 * units); bytes past that span are never touched.
//
// What the plan guarantees, and the kernel cannot check:
//   - the waves own every (key, unit) exactly once;
//   - the grid fits 31 bits (refused otherwise, never truncated);
//   - the keys are whole lists' worth (nkeys a multiple of keys_per_list) and
//     the lists' bytes, nlists * npts * 8, fit 64 bits (refused otherwise);
//   - the frontier level is eval_frontier_level(stop, npts), or 0 (root walks)
//     exactly where eval_form falls back: logN > 63, DPF_EVAL_MODE=plain, or
//     a frontier area smaller than eval_frontier_bytes(nkeys, stop, npts).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "tree_plan.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DPF_BITS_HD __host__ __device__
#else
#define DPF_BITS_HD
#endif

namespace dpfh {

constexpr uint32_t kBitsUnitPts = 128;    // points per unit: two per lane of a wave
constexpr uint32_t kBitsUnitBytes = 16;   // their bits in the row

// Units per key: ceil(npts / 128).
DPF_BITS_HD inline uint64_t eval_bits_units(uint64_t npts) {
    return npts / kBitsUnitPts + (npts % kBitsUnitPts != 0);
}
// Bytes of a row the kernel writes: the smallest bits_stride.
DPF_BITS_HD inline uint64_t eval_bits_stride(uint64_t npts) { return eval_bits_units(npts) * kBitsUnitBytes; }
// Byte offset of a unit's 16-byte span in its key's row.
DPF_BITS_HD inline uint64_t eval_bits_unit_off(uint64_t unit) { return unit * kBitsUnitBytes; }
// Index in the (virtually padded) list of lane `lane`'s point `half` (0 or 1).
DPF_BITS_HD inline uint64_t eval_bits_point(uint64_t unit, uint32_t lane, uint32_t half) {
    return unit * kBitsUnitPts + 64u * half + lane;
}
// The index that lane loads: clamped into the list (npts > 0).
DPF_BITS_HD inline uint64_t eval_bits_clamp(uint64_t j, uint64_t npts) { return j < npts ? j : npts - 1; }
// The list of points key `key` is evaluated at, and the index in xs of that
// list's first point.  Both are wave-uniform in the kernel.
DPF_BITS_HD inline uint64_t eval_bits_list(uint64_t key, uint64_t keys_per_list) { return key / keys_per_list; }
DPF_BITS_HD inline uint64_t eval_bits_list_base(uint64_t list, uint64_t npts) { return list * npts; }
// nlists lists of npts points each: their bytes fit 64 bits.
inline bool eval_bits_lists_ok(uint64_t nlists, uint64_t npts) {
    return npts == 0 || nlists <= (~0ull >> 3) / npts;
}
// Valid lanes of half `half` of a unit: bit l set iff that lane's point exists.
// All ones except in the last unit.
inline uint64_t eval_bits_mask(uint64_t npts, uint64_t unit, uint32_t half) {
    const uint64_t first = eval_bits_point(unit, 0, half);
    if (first >= npts) return 0;
    const uint64_t n = npts - first;
    return n >= 64 ? ~0ull : (1ull << n) - 1;
}

enum EvalBitsKernel { kEvalBitsPair = 0 };   // one (key, unit) per wave, one pair of points per lane

struct EvalBitsForm {
    uint32_t L;             // frontier level (0: every walk starts at the root)
    EvalBitsKernel kernel;
    uint32_t block;         // a multiple of 64: whole waves
    uint64_t grid;
    uint64_t units;         // per key
    uint64_t nwaves;        // nkeys * units: waves with work
    uint64_t keys_per_list; // key k walks at the points of list k / keys_per_list
    uint64_t nlists;        // nkeys / keys_per_list
    uint64_t last_mask[2];  // valid lanes of the last unit's two halves
    TreeForm nodes;         // the frontier pass (L > 0)
};

// What launch_eval_bits does with nkeys keys, keys_per_list of them a list of
// npts points (all > 0) and a frontier area of frontier_bytes (0: none).  False
// when a grid would exceed kMaxGrid workgroups, when the keys are not whole
// lists' worth, or when the lists' bytes do not fit 64 bits.  The frontier is a
// key's own (its top tree levels), so its level and size do not depend on
// which list the key meets.  Short-lived waves, one unit each, as
// k_eval2: the persistent form is not taken.
inline bool eval_bits_form_lists(uint64_t nkeys, uint64_t keys_per_list, uint64_t npts, uint32_t stop, uint32_t logN,
                                 uint64_t frontier_bytes, uint64_t cus, const TreeKnobs& k, EvalBitsForm* out) {
    EvalBitsForm e{};
    e.kernel = kEvalBitsPair;
    if (keys_per_list == 0 || nkeys % keys_per_list != 0) return false;
    e.keys_per_list = keys_per_list;
    e.nlists = nkeys / keys_per_list;
    if (!eval_bits_lists_ok(e.nlists, npts)) return false;
    e.L = eval_frontier_level(stop, npts, k.eval_level_shift);
    if (logN > 63 || k.eval_plain || frontier_bytes == 0 ||
        frontier_bytes < eval_frontier_bytes(nkeys, stop, npts, k.eval_level_shift))
        e.L = 0;
    if (e.L > 0 && !tree_form(nkeys, e.L, 0, 0, true, false, cus, k.forced_depth, &e.nodes)) return false;
    e.units = eval_bits_units(npts);
    // nkeys * units * 64 threads would wrap: such a grid is refused as too large.
    if (nkeys > (~0ull >> 6) / e.units) return false;
    e.nwaves = nkeys * e.units;
    const uint64_t nthreads = e.nwaves * 64;
    e.block = pick_block(nthreads, kBlock, cus);
    e.grid = (nthreads + e.block - 1) / e.block;
    if (e.grid > kMaxGrid) return false;
    e.last_mask[0] = eval_bits_mask(npts, e.units - 1, 0);
    e.last_mask[1] = eval_bits_mask(npts, e.units - 1, 1);
    *out = e;
    return true;
}
// One list shared by all keys.
inline bool eval_bits_form(uint64_t nkeys, uint64_t npts, uint32_t stop, uint32_t logN, uint64_t frontier_bytes,
                           uint64_t cus, const TreeKnobs& k, EvalBitsForm* out) {
    return eval_bits_form_lists(nkeys, nkeys, npts, stop, logN, frontier_bytes, cus, k, out);
}

}  // namespace dpfh
