// stage_plan.hpp — how the host-buffer entry points (dpf_capi.hip) cut their
// work into chunks for the two-slot staging pipeline: which keys, which
// subtree, how many bytes and where in the caller's buffer.  Pure functions of
// the shapes; host-only and header-only (no HIP), so
// tests/c/stage_plan_test.cpp runs them under ASan/UBSan without a device.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "dpf_internal.hpp"

namespace dpfh {

constexpr size_t kStageBytes = (size_t)32 << 20;   // largest chunk of a staged output
constexpr size_t kSlabMinOut = (size_t)8 << 20;    // one key's output from which it is cut into >= 4 slabs

// Subtree (prefix_bits, prefix) lies inside a tree of `stop` levels
// (stop = stop_of(logN) <= 56, so the shift is defined).
inline bool prefix_ok(uint32_t prefix_bits, uint64_t prefix, uint32_t stop) {
    return prefix_bits <= stop && (prefix >> prefix_bits) == 0;
}

// *pb = log2(ngpus) when ngpus is a power of two and each of the 2^pb devices
// gets a subtree of the `stop` levels; false otherwise (ngpus <= 0 included).
inline bool gpus_to_pb(int ngpus, uint32_t stop, uint32_t* pb) {
    uint32_t b = 0;
    while (((int64_t)1 << b) < ngpus) ++b;
    if (((int64_t)1 << b) != ngpus || b > stop) return false;
    *pb = b;
    return true;
}

// One chunk of a staged EvalFull: subtree (prefix_bits, prefix) of keys
// [k0, k0 + n) gives `bytes` of output at byte `off` of the caller's buffer.
struct FullChunk {
    size_t k0, n;
    uint32_t prefix_bits;
    uint64_t prefix;
    size_t bytes, off;
};

// One device's EvalFull chunks.  With prefix_bits() == 0 a chunk is up to
// `per` whole keys; otherwise every key is cut into 2^slab_bits slabs, each
// one subtree (prefix_bits(), prefix0 + j).  dpf_evalfull_split confines a
// device to subtree (split_bits, lo) of its one key first.
struct FullPlan {
    size_t nk = 0, olen = 0;
    size_t per = 1;             // whole keys per chunk
    uint32_t split_bits = 0;    // the device's subtree of the key (dpf_evalfull_split)
    uint32_t slab_bits = 0;     // log2 of the chunks per key
    uint64_t prefix0 = 0;       // prefix of a key's first slab
    size_t nchunks = 0, cap = 0;        // chunks and the largest one's bytes
    size_t out_base = 0, out_bytes = 0; // the device's part of the caller's buffer
    // The distinct (nkeys, prefix_bits) launch shapes of the chunks.
    struct Shape {
        size_t nkeys;
        uint32_t prefix_bits;
    } shape[2] = {};
    size_t nshapes = 0;

    uint32_t prefix_bits() const { return split_bits + slab_bits; }
    FullChunk chunk(size_t i) const {
        if (prefix_bits() == 0) {
            const size_t k0 = i * per, n = std::min(per, nk - k0);
            return {k0, n, 0, 0, n * olen, out_base + k0 * olen};
        }
        const size_t k = i >> slab_bits, j = i & (((size_t)1 << slab_bits) - 1);
        return {k, 1, prefix_bits(), prefix0 + j, cap, out_base + k * olen + j * cap};
    }
};

// dpf_evalfull_batch's share of one device: keys [0, nk) of 2^logN points
// (nk >= 1, logN <= 63).
inline FullPlan full_plan(size_t nk, uint32_t logN) {
    FullPlan p;
    p.nk = nk;
    p.olen = full_len(logN);
    p.out_bytes = nk * p.olen;
    p.per = p.olen <= kStageBytes ? kStageBytes / p.olen : 1;
    uint32_t pb = 0;                                      // one key's output exceeds a chunk: subtree slabs
    while ((p.olen >> pb) > kStageBytes) ++pb;
    // A key whose output is >= kSlabMinOut goes in >= 4 subtree slabs even
    // when it fits one chunk, so its kernel, PCIe copy and host copy overlap
    // (BenchmarkEvalFull's logN = 28 is one 32 MiB key: as one chunk, the
    // three ran back to back).
    if (p.olen >= kSlabMinOut && pb < 2) pb = 2;
    p.slab_bits = pb;
    if (pb == 0) {
        p.nchunks = (nk + p.per - 1) / p.per;
        p.cap = std::min(p.per, nk) * p.olen;
        p.shape[p.nshapes++] = {std::min(p.per, nk), 0};
        if (nk > p.per && nk % p.per != 0) p.shape[p.nshapes++] = {nk % p.per, 0};
    } else {
        p.nchunks = nk << pb;
        p.cap = p.olen >> pb;
        p.shape[p.nshapes++] = {1, pb};
    }
    return p;
}

// dpf_evalfull_split's share of device `lo` of 2^pb (gpus_to_pb): subtree
// (pb, lo) of the one key, `slab` bytes at lo * slab, streamed out in 2^extra
// sub-slabs (pb + extra, lo * 2^extra + j) of at most kStageBytes.
inline FullPlan split_plan(uint32_t logN, uint32_t pb, size_t lo) {
    const uint32_t stop = stop_of(logN);
    FullPlan p;
    p.nk = 1;
    p.olen = full_len(logN);
    const size_t slab = p.olen >> pb;
    uint32_t extra = 0;
    while ((slab >> extra) > kStageBytes && pb + extra < stop) ++extra;
    p.split_bits = pb;
    p.slab_bits = extra;
    p.prefix0 = (uint64_t)lo << extra;
    p.nchunks = (size_t)1 << extra;
    p.cap = slab >> extra;
    p.out_base = lo * slab;
    p.out_bytes = slab;
    p.shape[p.nshapes++] = {1, pb + extra};
    return p;
}

// dpf_eval_batch's share of one device: chunks of `per` whole keys with ppk
// points each, so a chunk's points fit kStageBytes (one key when ppk alone
// exceeds it).  nk, ppk >= 1.
struct EvalPlan {
    size_t nk = 0, per = 1, nchunks = 0;
    size_t qcap = 0;   // queries (= result bytes) of the largest chunk
    size_t k0(size_t i) const { return i * per; }
    size_t n(size_t i) const { return std::min(per, nk - i * per); }
};

inline EvalPlan eval_plan(size_t nk, size_t ppk) {
    EvalPlan p;
    p.nk = nk;
    p.per = std::max<size_t>(1, std::min(nk, kStageBytes / (ppk * 8)));
    p.nchunks = (nk + p.per - 1) / p.per;
    p.qcap = p.per * ppk;
    return p;
}

}  // namespace dpfh
