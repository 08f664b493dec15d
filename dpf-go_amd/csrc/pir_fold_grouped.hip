// pir_fold_grouped.hip — the grouped XOR fold: one launch answers many small
// DBs (groups), each with its own keys.  The layout rule and the launch plan
// are in pir_group_plan.hpp; the launcher walks the plan.  Many keys per group
// go to the matrix-core grouped fold (pir_fold_grouped_mfma.hip) by the route
// rule of pir_group_fold_plan.hpp.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "dpf_kernels.hpp"
#include "fold_ops.hpp"
#include "pir_group_fold_plan.hpp"
#include "pir_kernels.hpp"

namespace dpfk {

// The popcount fold (fold_popcount_body.inc: the loop this kernel shares
// with k_fold_sliced_direct) with a group coordinate.  Workgroup
// x of the launch is unit u0 + x of the plan (dpfh::group_unit): run
// u % runs of column (u / runs) % C of group u / (runs * C), the group-local
// super-groups [s0, s1) of that run.  Thread n of its 256 owns bit row n of the
// column; per super-group it reads its 8 words once (the workgroup: 8 KiB
// contiguous, flat super-group g * gsg + S) and folds them for each of the KP
// keys k0 .. k0 + KP - 1 of the group.  Key j's selection words are row
// g * kpg + k0 + j of bits; word 8 S + w of a row is super-group S of the
// GROUP.  A row has wlim words: fewer than a
// super-group's 8 at logN 7, and an end inside the last super-group whenever
// the row is not a multiple of 256 bits; words past it select nothing.
// Any width: thread n of column c has a row only if 256 c + n < nrows
// (= 8 * rec_bytes); the others fold nothing, and an answer word 8 c + i >=
// ntiles does not exist.
// Answer bit n of key j is the parity of popcount(acc[j]): one ballot per key,
// two words per wave.  atomic == 0 (one run per group): this workgroup is the
// only writer of its words and stores them.  Otherwise the answers were
// cleared earlier in stream order and the words are XORed in (vector atomics).
template <int KP>
__global__ __launch_bounds__(256) void k_fold_grouped(const uint32_t* __restrict__ bits, uint64_t wlim,
                                                      const uint4* __restrict__ dbs, uint64_t gsg, uint32_t C,
                                                      uint64_t runs, uint64_t spr, uint32_t kpg, uint32_t k0,
                                                      uint32_t nrows, uint32_t ntiles, uint32_t* __restrict__ ans,
                                                      uint64_t u0, uint32_t atomic) {
    const uint32_t n = threadIdx.x, l = n & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const dpfh::GroupUnit un = dpfh::group_unit(u0 + blockIdx.x, runs, spr, gsg, C);
    const uint64_t g = un.g, s0 = un.s0, s1 = un.s1;
    const uint32_t col = un.c;
    const uint64_t key0 = g * kpg + k0;                         // first answer / selection row of this pass
    const uint32_t* sel = bits + key0 * wlim;
#define FOLD_SEL(j, i) sel[j * wlim + i]
#define FOLD_AT(S) group_tile(dbs, g, gsg, S, nrows, row)
    // lanes 0 and 1 of a wave: its two answer words
#define FOLD_EMIT_BEGIN const uint32_t word = 8 * col + 2 * w + l;
#define FOLD_EMIT(j, m)                                            \
    if (l < 2 && word < ntiles) {                                  \
        const uint32_t v = l ? (uint32_t)(m >> 32) : (uint32_t)m; \
        uint32_t* out = ans + (key0 + j) * ntiles + word;          \
        if (!atomic) *out = v;                                     \
        else if (v) atomicXor(out, v);                             \
    }
#include "fold_popcount_body.inc"
}

namespace {

// DPF_GROUP_KP = 1 | 2 | 4: the widest key pass (measurement only).
uint32_t group_kp_knob() {
    static const uint32_t kp = [] {
        const char* e = getenv("DPF_GROUP_KP");
        return e && atoi(e) > 0 ? (uint32_t)atoi(e) : 0u;
    }();
    return kp;
}

// DPF_GROUP_FOLD_ROUTE = direct | mfma: the route whatever the plan's rule says,
// for every caller of the public entries and in what the form query reports
// (measurement only, named in include/dpf_hip.h; read at every call, so one
// process can time both).
int route_knob() {
    const char* e = getenv("DPF_GROUP_FOLD_ROUTE");
    return !e ? -1 : e[0] == 'd' ? (int)dpfh::kFoldRouteDirect : e[0] == 'm' ? (int)dpfh::kFoldRouteMfma : -1;
}

}  // namespace

dpfh::GroupFoldKeysPlan fold_grouped_plan(uint64_t ngroups, uint32_t keys_per_group, uint64_t nrec, uint64_t rec_bytes,
                                          uint64_t cus) {
    return dpfh::plan_fold_grouped_keys(ngroups, dpfh::group_stride(nrec) / 256, dpfh::rec_cols(rec_bytes), keys_per_group,
                                        cus ? cus : (uint64_t)cu_count(), fold_limits(), route_knob(), group_kp_knob());
}

hipError_t launch_pir_fold_grouped(const uint32_t* bits, uint64_t words_per_key, const uint8_t* dbs, uint64_t ngroups,
                                   uint32_t keys_per_group, uint64_t nrec, uint64_t rec_bytes, uint32_t* ans,
                                   uint32_t* parts, hipStream_t st) {
    (void)parts;   // the plan's launches write no scratch (dpfh::GroupedPlan::scratch_bytes)
    if (!dpfh::rec_bytes_any_ok(rec_bytes)) return hipErrorInvalidValue;
    if (ngroups == 0 || keys_per_group == 0) return hipSuccess;
    if (ngroups * keys_per_group > UINT32_MAX) return hipErrorInvalidValue;
    const uint64_t ans_bytes = ngroups * keys_per_group * rec_bytes;
    if (nrec == 0) return launch_zero(ans, ans_bytes, st);
    if (words_per_key % 4 != 0 || words_per_key * 32 < nrec) return hipErrorInvalidValue;
    const uint32_t T = dpfh::rec_tiles(rec_bytes);
    const dpfh::GroupFoldKeysPlan keys = fold_grouped_plan(ngroups, keys_per_group, nrec, rec_bytes, 0);
    if (keys.route == dpfh::kFoldRouteMfma)
        return launch_fold_grouped_mfma(keys, bits, words_per_key, dbs, rec_bytes, ans, st);
    const dpfh::GroupedPlan& p = keys.direct;
    if (p.atomic())
        if (hipError_t e = launch_zero(ans, ans_bytes, st); e != hipSuccess) return e;
    return p.for_each_launch([&](const dpfh::GroupLaunch& l) {
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3((uint32_t)l.blocks), dim3(256), 0, st, bits, words_per_key,
                               reinterpret_cast<const uint4*>(dbs), p.gsg, p.C, p.runs, p.spr, p.kpg, l.k0,
                               (uint32_t)(8 * rec_bytes), T, ans, l.u0, (uint32_t)p.atomic());
        };
        if (l.kp == 4) launch(k_fold_grouped<4>);
        else if (l.kp == 2) launch(k_fold_grouped<2>);
        else launch(k_fold_grouped<1>);
        return hipGetLastError();
    });
}

}  // namespace dpfk
