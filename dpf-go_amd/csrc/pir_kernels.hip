// pir_kernels.hip — what the XOR fold's translation units share: the
// reduction of the workgroups' partials into the answers (k_xor_parts), the
// limits of dpf_set_fold_limits and the environment knobs.  The folds
// themselves: pir_fold_rows.hip (LDS folds over a row-major DB),
// pir_fold_sliced.hip (matrix-core fold over the sliced DB); the resident DB's
// maintenance and the private write: pir_db_ops.hip.  Their launch arithmetic:
// pir_fold_plan.hpp.
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include <stdlib.h>

#include "fold_ops.hpp"
#include "pir_kernels.hpp"


namespace dpfk {

// ans[k * ans_words + off + i] ^= XOR over workgroups p of parts[p][k][i]
// (k < nkeys, i < pwords; pkeys keys per part).  Block (x, y): 256 words x
// parts y, y + gridDim.y, ...; one atomicXor each.  Part words at or past
// ans_words (the absent bit tiles of a record of any width) are not read.
__global__ __launch_bounds__(256) void k_xor_parts(const uint32_t* __restrict__ parts, uint64_t nparts, uint32_t nkeys,
                                                   uint32_t pkeys, uint32_t pwords, uint32_t* __restrict__ ans,
                                                   uint64_t ans_words, uint32_t off) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nkeys * pwords) return;
    const uint32_t k = t / pwords, i = t % pwords;
    if ((uint64_t)off + i >= ans_words) return;
    uint32_t v = 0;
    // Eight independent loads in flight per step (a strided loop of single
    // loads left the kernel at ~5 us, mostly dependent L2 round trips).
    const uint64_t g = gridDim.y;
    uint64_t p = blockIdx.y;
    for (; p + 7 * g < nparts; p += 8 * g) {
        uint32_t x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = parts[((p + u * g) * pkeys + k) * pwords + i];
#pragma unroll
        for (int u = 0; u < 8; ++u) v ^= x[u];
    }
    for (; p < nparts; p += g) v ^= parts[(p * pkeys + k) * pwords + i];
    if (v) atomicXor(ans + (uint64_t)k * ans_words + off + i, v);
}

// The knobs (measurement only; defaults and meaning: dpfh::FoldKnobs).  The
// one place of the fold that reads the environment.
const dpfh::FoldKnobs& fold_knobs() {
    static const dpfh::FoldKnobs k = [] {
        dpfh::FoldKnobs v;
        auto positive = [](const char* name, int dflt) {
            const char* e = getenv(name);
            return e && atoi(e) > 0 ? atoi(e) : dflt;
        };
        if (const char* e = getenv("DPF_FOLD_SKEW")) v.skew = atoi(e);
        if (const char* e = getenv("DPF_FOLD_NT_MIN"); e && *e) v.nt_min = strtoull(e, nullptr, 0);
        v.per_cu = positive("DPF_FOLD_PER_CU", v.per_cu);
        v.wide_cg = positive("DPF_FOLD_WIDE_CG", v.wide_cg);
        v.xor_ys = (uint64_t)positive("DPF_XOR_PARTS_YS", 0);
        return v;
    }();
    return k;
}

// XOR nparts workgroup partials into the answers (stream-ordered after the fold).
hipError_t launch_xor_parts(const uint32_t* parts, uint64_t nparts, uint32_t nkeys, uint32_t pkeys,
                            uint32_t pwords, uint32_t* ans, uint64_t ans_words, uint32_t off, hipStream_t st) {
    const uint32_t ys = dpfh::xor_parts_ys(nparts, fold_knobs().xor_ys);
    hipLaunchKernelGGL(k_xor_parts, dim3((nkeys * pwords + 255) / 256, ys), dim3(256), 0, st, parts, nparts, nkeys,
                       pkeys, pwords, ans, ans_words, off);
    return hipGetLastError();
}

// Answers are cleared on the caller's stream by a kernel, not by
// hipMemsetAsync: in a stream capture that is a memset node, which does not
// replay reliably ("Clearing answers"), while a kernel node
// replays like every other launch of a _dev call.
__global__ __launch_bounds__(256) void k_zero_words(uint32_t* __restrict__ p, uint64_t nwords) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nwords; i += (uint64_t)gridDim.x * 256) p[i] = 0u;
}

hipError_t launch_zero(void* p, uint64_t bytes, hipStream_t st) {
    if (bytes == 0) return hipSuccess;
    if (bytes % 4 != 0 || (uintptr_t)p % 4 != 0) return hipErrorInvalidValue;
    const uint64_t nwords = bytes / 4, blocks = (nwords + 255) / 256;
    hipLaunchKernelGGL(k_zero_words, dim3((uint32_t)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, st, (uint32_t*)p,
                       nwords);
    return hipGetLastError();
}

uint64_t pir_fold_parts_bytes() { return dpfh::kFoldPartsBytes; }

// Tuning / test limits (set_fold_limits), both in one word so that a launcher
// reads a consistent pair: workgroups per fold launch (high half) and
// super-groups per matrix-core fold workgroup.
static uint64_t pack_limits(dpfh::FoldLimits l) { return (uint64_t)l.max_blocks << 32 | l.max_sg; }
static std::atomic<uint64_t> g_fold_limits{pack_limits(dpfh::clamp_fold_limits(0, 0))};
void set_fold_limits(uint32_t max_blocks, uint32_t max_sg) {
    g_fold_limits.store(pack_limits(dpfh::clamp_fold_limits(max_blocks, max_sg)));
}
dpfh::FoldLimits fold_limits() {
    const uint64_t v = g_fold_limits.load(std::memory_order_relaxed);
    return {(uint32_t)(v >> 32), (uint32_t)v};
}

}  // namespace dpfk

