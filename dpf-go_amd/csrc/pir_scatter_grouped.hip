// pir_scatter_grouped.hip — the grouped private write: one scatter launch
// rewrites many small DBs (groups), each under its own keys.  The dual of
// pir_fold_grouped.hip; the layout rule and the launch plan are
// pir_group_plan.hpp's, the plan's builder and the route rule are in
// pir_group_scatter_plan.hpp, and the launcher walks the plan.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "dpf_kernels.hpp"
#include "fold_ops.hpp"
#include "pir_group_scatter_plan.hpp"
#include "pir_kernels.hpp"

namespace dpfk {

// The bits of selection word ww (records 32 ww .. of the group) that are records below nrec.
__device__ __forceinline__ uint32_t group_live(uint64_t ww, uint64_t nrec) {
    const uint64_t r0 = ww * 32;
    return nrec >= r0 + 32 ? ~0u : nrec <= r0 ? 0u : (1u << (uint32_t)(nrec - r0)) - 1u;
}

// The mirror of k_fold_grouped.  Workgroup x of the launch is unit u0 + x of
// the plan (dpfh::group_unit): run u % runs of column
// (u / runs) % C of group u / (runs * C), the group-local super-groups
// [s0, s1) of that run.  Thread n of its 256 owns bit row n of the column: per
// super-group it loads its 8 words (two 16-byte loads; the workgroup: 8 KiB
// contiguous, flat super-group g * gsg + S), XORs (message bit & selection
// word) of each of the KP keys k0 .. k0 + KP - 1 of the group into them -- one
// v_bitop3 per word and key -- and stores them back (two 16-byte vector
// stores).  The work per tile is KP keys' worth: nothing is staged for keys the
// group does not have.
// The selection words are wave-uniform (scalar loads) from row
// g * kpg + k0 + j of bits; word 8 S + w of a row is super-group S of the
// GROUP.  A row has wlim words (fewer than a super-group's 8 at logN 7), and
// the group has nrec records: words past either end are not read, and the bits
// of a word at records >= nrec are masked off on the scalar side, so flat
// positions [nrec, group_stride(nrec)) stay zero whatever the caller left in
// the bits.  The thread's message bit of key j (bit `row` of message
// g * kpg + k0 + j, sign-extended) is read once per run.
// Any width: thread n of column c has a row only if 256 c + n < nrows
// (= 8 * rec_bytes); the others neither load nor store.  The next
// super-group's loads are issued before the current one's arithmetic.
// Each tile of the run is read once and written once by this workgroup alone
// (the plan): no atomics, no LDS, no scratch.
template <int KP>
__global__ __launch_bounds__(256) void k_scatter_grouped(const uint32_t* __restrict__ bits, uint64_t wlim,
                                                         uint4* __restrict__ dbs, uint64_t nrec, uint64_t gsg, uint32_t C,
                                                         uint64_t runs, uint64_t spr, uint32_t kpg, uint32_t k0,
                                                         uint32_t nrows, const uint32_t* __restrict__ msgs,
                                                         uint32_t ntiles, uint64_t u0) {
    const uint32_t n = threadIdx.x;
    const dpfh::GroupUnit un = dpfh::group_unit(u0 + blockIdx.x, runs, spr, gsg, C);
    const uint64_t g = un.g, s0 = un.s0, s1 = un.s1;
    const uint32_t col = un.c;
    const uint64_t key0 = g * kpg + k0;                         // first message / selection row of this pass
    const uint32_t* sel = bits + key0 * wlim;
    const uint32_t row = col * 256 + n;
    if (row >= nrows || s0 >= s1) return;                       // a short last column lacks this row (no barrier below)
    uint32_t m[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j)
        m[j] = 0u - ((msgs[(key0 + j) * ntiles + (row >> 5)] >> (row & 31)) & 1u);
    auto at = [&](uint64_t S) { return group_tile(dbs, g, gsg, S, nrows, row); };
    auto apply = [&](uint64_t S, uint4& a, uint4& b) __attribute__((always_inline)) {
        uint32_t x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        if (8 * S + 8 <= wlim && (8 * S + 8) * 32 <= nrec) {     // uniform: whole words of live records
#pragma unroll
            for (int j = 0; j < KP; ++j)
#pragma unroll
                for (int q = 0; q < 8; ++q) x[q] = xam(x[q], m[j], sel[j * wlim + 8 * S + q]);
        } else {                                                 // the key rows or the group's records end in here
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const uint32_t live = group_live(8 * S + q, nrec);
                if (8 * S + q < wlim && live != 0) {
#pragma unroll
                    for (int j = 0; j < KP; ++j) x[q] = xam(x[q], m[j], sel[j * wlim + 8 * S + q] & live);
                }
            }
        }
        a = make_uint4(x[0], x[1], x[2], x[3]);
        b = make_uint4(x[4], x[5], x[6], x[7]);
    };
    uint4 a = at(s0)[0], b = at(s0)[1];
    for (uint64_t S = s0; S < s1; ++S) {
        uint4 na = a, nb = b;
        if (S + 1 < s1) {
            na = at(S + 1)[0];
            nb = at(S + 1)[1];
        }
        apply(S, a, b);
        at(S)[0] = a;
        at(S)[1] = b;
        a = na;
        b = nb;
    }
}

namespace {

// DPF_GROUP_SCATTER_ROUTE = grouped | loop: the route whatever the plan's rule
// says, for every caller of the public entries and in what the form query
// reports (measurement only, named in include/dpf_hip.h; read at every call,
// so one process can time both).
int route_knob() {
    const char* e = getenv("DPF_GROUP_SCATTER_ROUTE");
    return !e ? -1 : e[0] == 'g' ? (int)dpfh::kScatterRouteGrouped : e[0] == 'l' ? (int)dpfh::kScatterRouteLoop : -1;
}

}  // namespace

dpfh::GroupedPlan scatter_grouped_plan(uint64_t ngroups, uint32_t keys_per_group, uint64_t nrec, uint64_t rec_bytes,
                                       uint64_t cus) {
    dpfh::GroupedPlan p =
        dpfh::plan_scatter_grouped(ngroups, dpfh::group_stride(nrec) / 256, dpfh::rec_cols(rec_bytes), keys_per_group,
                                   cus ? cus : (uint64_t)cu_count(), fold_limits());
    if (const int knob = route_knob(); knob >= 0) p.route = (dpfh::GroupScatterRoute)knob;
    return p;
}

hipError_t launch_scatter_grouped(const uint32_t* bits, uint64_t words_per_key, uint8_t* dbs, uint64_t ngroups,
                                  uint32_t keys_per_group, uint64_t nrec, uint64_t rec_bytes, const uint8_t* msgs,
                                  hipStream_t st) {
    if (!dpfh::rec_bytes_any_ok(rec_bytes) || words_per_key % 4 != 0 || nrec > words_per_key * 32)
        return hipErrorInvalidValue;
    if (ngroups == 0 || keys_per_group == 0 || nrec == 0) return hipSuccess;
    if (ngroups * keys_per_group > UINT32_MAX) return hipErrorInvalidValue;
    const uint64_t gs = dpfh::group_stride(nrec);
    const uint32_t T = dpfh::rec_tiles(rec_bytes);
    const dpfh::GroupedPlan p = scatter_grouped_plan(ngroups, keys_per_group, nrec, rec_bytes, 0);
    if (p.route == dpfh::kScatterRouteLoop) {
        // Group g is the flat records [g * gs, g * gs + nrec): a sliced DB of its own.
        for (uint64_t g = 0; g < ngroups; ++g)
            if (hipError_t e = launch_scatter_sliced(bits + g * keys_per_group * words_per_key, words_per_key,
                                                     dbs + g * gs * rec_bytes, nrec, rec_bytes,
                                                     msgs + g * keys_per_group * rec_bytes, keys_per_group, st);
                e != hipSuccess)
                return e;
        return hipSuccess;
    }
    return p.for_each_launch([&](const dpfh::GroupLaunch& l) {
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3((uint32_t)l.blocks), dim3(256), 0, st, bits, words_per_key,
                               reinterpret_cast<uint4*>(dbs), nrec, p.gsg, p.C, p.runs, p.spr, p.kpg, l.k0,
                               (uint32_t)(8 * rec_bytes), reinterpret_cast<const uint32_t*>(msgs), T, l.u0);
        };
        if (l.kp == 4) launch(k_scatter_grouped<4>);
        else if (l.kp == 3) launch(k_scatter_grouped<3>);
        else if (l.kp == 2) launch(k_scatter_grouped<2>);
        else launch(k_scatter_grouped<1>);
        return hipGetLastError();
    });
}

}  // namespace dpfk
