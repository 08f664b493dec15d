// fold_ops.hpp — pieces of the XOR fold shared by its translation units
// (pir_fold_rows.hip, pir_fold_sliced.hip, pir_fold_grouped.hip, pir_fold_grouped_mfma.hip, pir_scatter_grouped.hip,
// pir_db_ops.hip, pir_kernels.hip)
// and the fused PIR kernel (pir_fused.hip): the answers' clearing, the bitwise
// and load helpers, the FP4 operands of the matrix-core fold (layout and
// exactness: pir_fold_sliced.hip, "The fold as a GF(2) matrix product"), the
// partials' reduction launch and the launchers' shared host state.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pir_fold_plan.hpp"

namespace dpfk {

// The first fold launch of a call clears the answers (instead of a separate
// memset launch); k_xor_parts runs after it in stream order.
__device__ __forceinline__ void zero_answers(uint32_t* zero, uint64_t words) {
    if (zero == nullptr) return;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < words; t += (uint64_t)gridDim.x * blockDim.x)
        zero[t] = 0;
}

// v_bitop3_b32 truth tables: src0 = 0xF0, src1 = 0xCC, src2 = 0xAA.
constexpr uint8_t kTT0 = 0xF0, kTT1 = 0xCC, kTT2 = 0xAA;
__device__ __forceinline__ uint32_t x3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, kTT0 ^ kTT1 ^ kTT2);
}
// a ^ (b & m)
__device__ __forceinline__ uint32_t xam(uint32_t a, uint32_t b, uint32_t m) {
    return __builtin_amdgcn_bitop3_b32(a, b, m, kTT0 ^ (kTT1 & kTT2));
}
__device__ __forceinline__ uint4 x4(uint4 a, uint4 b) { return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w); }
__device__ __forceinline__ uint4 x4am(uint4 a, uint4 b, uint32_t m) {
    return make_uint4(xam(a.x, b.x, m), xam(a.y, b.y, m), xam(a.z, b.z, m), xam(a.w, b.w, m));
}
// The grouped kernels' tile address: the two uint4 of bit row `row` (of nrows)
// in super-group S of group g, gsg super-groups a group (pir_group_plan.hpp's layout).
template <class T>
__device__ __forceinline__ T* group_tile(T* dbs, uint64_t g, uint64_t gsg, uint64_t S, uint32_t nrows, uint64_t row) {
    return &dbs[((g * gsg + S) * nrows + row) * 2];
}
// Workgroup barrier of the folds' LDS staging: the plain barrier.  The
// compiler keeps a global prefetch in flight across it; fencing the local
// address space only measured identical (r05, profiles/r05/fold_barrier).
__device__ __forceinline__ void lds_barrier() { __syncthreads(); }

// Bits of chunk cc's records below nrec, for word 0 (records 0..31) and 1;
// none when the chunk is not the caller's (live = false).  Arithmetic, not
// branches: a branch here splits the lookup block and the register
// allocator then spills the table reads around it.
__device__ __forceinline__ uint2 valid_mask(uint64_t cc, uint64_t nrec, bool live = true) {
    uint64_t v = nrec > cc * 64 ? nrec - cc * 64 : 0;
    v = live ? (v < 64 ? v : 64) : 0;
    const uint32_t lo = v < 32 ? (uint32_t)v : 32u, hi = v > 32 ? (uint32_t)v - 32u : 0u;
    return make_uint2((uint32_t)((1ull << lo) - 1), (uint32_t)((1ull << hi) - 1));
}

// A streamed 16-byte operand; NT: a nontemporal load (the `nt` cache policy),
// for DB slices too large to stay in the caches between batches (fold_ntdb).
typedef uint32_t fold_nt4 __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ uint4 fold_ld(const uint4* p) {
    if constexpr (NT) {
        const fold_nt4 v = __builtin_nontemporal_load(reinterpret_cast<const fold_nt4*>(p));
        return make_uint4(v.x, v.y, v.z, v.w);
    } else {
        return *p;
    }
}

typedef int fold_v8i __attribute__((ext_vector_type(8)));
typedef float fold_v16f __attribute__((ext_vector_type(16)));

// Which side takes the cheap 5-op expansion (ANDs + one shift; weights 0.5,
// 1, 2, 2) and which the 7-op one (weights 2, 1, 0.5, 0.5): a selection
// operand feeds NT MFMAs and a DB operand MT, so per MFMA the VALU cost is
// sel/NT + db/MT, lowest with the cheap form on the side with fewer tiles
// (SC = NT < MT in the kernel: the selection side for the 4- and 8-key-tile
// shapes, the DB side for the others).
__device__ __forceinline__ fold_v8i fp4_w5(uint32_t x) {     // weights 0.5, 1, 2, 2
    fold_v8i r;
    r[0] = (int)(x & 0x11111111u);
    r[1] = (int)(x & 0x22222222u);
    r[2] = (int)(x & 0x44444444u);
    r[3] = (int)((x >> 1) & 0x44444444u);
    r[4] = r[5] = r[6] = r[7] = 0;
    return r;
}
__device__ __forceinline__ fold_v8i fp4_w7(uint32_t s) {     // weights 2, 1, 0.5, 0.5
    fold_v8i r;
    r[0] = (int)((s << 2) & 0x44444444u);
    r[1] = (int)(s & 0x22222222u);
    r[2] = (int)((s >> 2) & 0x11111111u);
    r[3] = (int)((s >> 3) & 0x11111111u);
    r[4] = r[5] = r[6] = r[7] = 0;
    return r;
}
template <bool SC>
__device__ __forceinline__ fold_v8i fp4_db(uint32_t x) { return SC ? fp4_w7(x) : fp4_w5(x); }
template <bool SC>
__device__ __forceinline__ fold_v8i fp4_sel(uint32_t s) { return SC ? fp4_w5(s) : fp4_w7(s); }
__device__ __forceinline__ uint32_t u4w(const uint4& v, int t) { return t == 0 ? v.x : t == 1 ? v.y : t == 2 ? v.z : v.w; }

constexpr int kFoldFp4 = 4;         // cbsz / blgp format code of e2m1
constexpr int kE8M0One = 127;       // block scale 2^0

using dpfh::kFoldMaxBlocks;

// What every fold launcher plans from (pir_kernels.hip): one snapshot of
// set_fold_limits' values, taken once per public call, and the environment
// knobs, read once per process.  (The third input, the calling thread's CU
// budget, is cu_count() of dpf_kernels.hpp.)
dpfh::FoldLimits fold_limits();
const dpfh::FoldKnobs& fold_knobs();

// XOR nparts workgroup partials into the answers (stream-ordered after the fold).
hipError_t launch_xor_parts(const uint32_t* parts, uint64_t nparts, uint32_t nkeys, uint32_t pkeys,
                            uint32_t pwords, uint32_t* ans, uint64_t ans_words, uint32_t off, hipStream_t st);

}  // namespace dpfk
