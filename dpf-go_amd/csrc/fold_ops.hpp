// fold_ops.hpp — pieces of the XOR fold shared by the fold kernels
// (pir_kernels.hip) and the fused PIR kernel (pir_fused.hip): the answers'
// clearing, the FP4 operands of the matrix-core fold (layout and exactness:
// pir_kernels.hip, "The fold as a GF(2) matrix product") and the partials'
// reduction launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dpfk {

// The first fold launch of a call clears the answers (instead of a separate
// memset launch); k_xor_parts runs after it in stream order.
__device__ __forceinline__ void zero_answers(uint32_t* zero, uint64_t words) {
    if (zero == nullptr) return;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < words; t += (uint64_t)gridDim.x * blockDim.x)
        zero[t] = 0;
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

constexpr uint64_t kFoldMaxBlocks = 1024;          // workgroups per launch (partials area)

// XOR nparts workgroup partials into the answers (stream-ordered after the fold).
hipError_t launch_xor_parts(const uint32_t* parts, uint64_t nparts, uint32_t nkeys, uint32_t pkeys,
                            uint32_t pwords, uint32_t* ans, uint64_t ans_words, uint32_t off, hipStream_t st);

}  // namespace dpfk
