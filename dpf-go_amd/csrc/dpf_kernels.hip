// dpf_kernels.hip — gfx950 kernels for DPF evaluation (EvalFull / Eval).
//
// Reference semantics: dpf/dpf.go:171-262 (Eval, evalFullRecursive, EvalFull)
// and the PRG dpf/dpf.go:59-69 over aes128MMO (dpf/aes_amd64.s:51-82); the
// AES back end is aes_ttable.hpp.
//
// Tree: a thread owns a subtree of 2^D leaves (D <= 7).  It walks from the
// root to its subtree root computing only the child on its path (one AES per
// level), then expands the subtree depth-first with the right siblings kept
// in registers (one statically-allocated slot per level), writing leaves in
// ascending order exactly like evalFullRecursive's cursor (dpf.go:213-241).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <type_traits>
#include "aes_consts.hpp"
#include "aes_ttable.hpp"
#include "dpf_kernels.hpp"
#include "wave_prio.hpp"
#include "tree_ops.hpp"

namespace dpfk {

#ifdef DPF_WAVE_TIMES
constexpr uint64_t kWaveTimesMax = 1u << 16;
__device__ uint64_t g_wave_times[5 * kWaveTimesMax];   // start, end, HW_ID, XCC_ID, walk end
#endif

struct Ctx {
    const uint8_t* tab;
    uint32_t lo;
    KeySrc ks;
    Blk fcw;
    uint8_t* outp;      // leaf mode: 16-byte leaf cursor
    uint4* nseed;       // node mode: seed cursor
    uint8_t* nt;        // node mode: t cursor
    uint32_t groups;    // 4-leaf groups finished (wave priority steps, prio_step)
    uint32_t* prog = nullptr;   // feedback form: this SIMD's 16 wave-progress slots in LDS
    uint32_t pslot = 0;         // ... and this wave's slot (hardware wave id)
};

// Issue priority by progress.  A SIMD's waves issue oldest-first, so of the
// 4 waves sharing one, the oldest finishes its subtree first and the
// youngest runs alone at the end, when the CU's LDS idles (per-wave wall
// clock, tools/wave_times.hip, configs[1]: the 4 slots of every SIMD end at
// 455 / 635 / 825 / 1015 us; waves busy 71% of the kernel's span).  Waves
// lower their priority as they pass progress thresholds (fractions of the
// thread's 4-leaf groups), so waves that are ahead yield the issue slots to
// the ones behind and a SIMD's waves finish close together (busy 95%;
// kernel 1048 -> 948 us on one box, profiles/r03/prio/).
// Thresholds 3/4, 7/8, 15/16.  Subtrees of <= 2^5 leaf blocks (8 or fewer
// groups: the PIR tree, strong-scaling ranks) step at 1/2, 3/4, 7/8: at the
// PIR shape waves are busy 0.945-0.949 of the span instead of 0.914-0.922
// and the span is 244 vs 250-256 us (profiles/r04/prio/).
// Feedback form (c.prog set: one workgroup holds every wave of its CU):
// priority from the wave's lead, in finished 4-leaf groups, over the slowest
// wave of its SIMD (wave_prio.hpp).
constexpr uint32_t kPrioFar = 3;   // prio_by_lead: a lead of 1 group is near, up to kPrioFar far
template <int DMAX>
__device__ __forceinline__ void prio_step(Ctx& c) {
    if (c.prog != nullptr) {
        prio_by_lead(c.prog, c.pslot, ++c.groups, 1, kPrioFar);
        return;
    }
    constexpr bool small = DMAX <= (int)dpfh::kPrioSmallMaxD;   // dpfh::TreeForm::prio_small
    constexpr uint32_t total = DMAX >= 2 ? 1u << (DMAX - 2) : 1u;   // 4-leaf groups per thread
    const uint32_t d = ++c.groups;
    constexpr uint32_t den = small ? 8 : 16;
    constexpr uint32_t t1 = small ? 4 : 12;
    constexpr uint32_t t2 = small ? 6 : 14;
    constexpr uint32_t t3 = small ? 7 : 15;
    const uint32_t x = d * den;
    if (x >= t3 * total) __builtin_amdgcn_s_setprio(0);
    else if (x >= t2 * total) __builtin_amdgcn_s_setprio(1);
    else if (x >= t1 * total) __builtin_amdgcn_s_setprio(2);
}

__device__ __forceinline__ void emit_node(Ctx& c, const Node& n) {
    *c.nseed++ = make_uint4(n.s.c0, n.s.c1, n.s.c2, n.s.c3);
    *c.nt++ = (uint8_t)n.t;
}

// Exchange a value with the other lane of the pair (lane ^ 1): DPP
// quad_perm [1,0,3,2], VALU only (no LDS traffic; the T-table owns the LDS).
__device__ __forceinline__ uint32_t pair_swap(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);
}
__device__ __forceinline__ Node pair_swap(const Node& n) {
    return {{pair_swap(n.s.c0), pair_swap(n.s.c1), pair_swap(n.s.c2), pair_swap(n.s.c3)}, pair_swap(n.t)};
}
__device__ __forceinline__ Node sel(bool b, const Node& x, const Node& y) {
    return {{b ? x.s.c0 : y.s.c0, b ? x.s.c1 : y.s.c1, b ? x.s.c2 : y.s.c2, b ? x.s.c3 : y.s.c3}, b ? x.t : y.t};
}

__device__ __forceinline__ Blk bsel(bool b, const Blk& x, const Blk& y) {
    return {b ? x.c0 : y.c0, b ? x.c1 : y.c1, b ? x.c2 : y.c2, b ? x.c3 : y.c3};
}

// Bottom two levels below node n: 4 leaves = 64 contiguous bytes at p
// (dpf.go:214-224 for each), stored back to back once all four are done.
// The two children are finished by one loop body (expand + leaf pair), not
// two inlined copies: the tree kernel's innermost loop must fit the
// instruction cache (64 KiB per two CUs).  Fully inlined, the PAIR path's
// loop body was ~85 KiB of code (22 AES-MMO bodies).
template <bool B, bool RAW>
__device__ __forceinline__ void leaves4(const Ctx& c, uint32_t lvl, const Node& n, uint8_t* p) {
    CW cw = key_cw<RAW>(c.ks, lvl);
    Node L, R;
    expand<B>(c.tab, c.lo, n, cw, L, R);
    CW cw1 = key_cw<RAW>(c.ks, lvl + 1);
    Blk o0 = {}, o1 = {}, o2, o3;
    // Only the pending child stays live through the first iteration (a
    // select of L or R at the top of each iteration kept both live: 5 more
    // VGPRs at every level of the expansion).
    Node m = L;
    const Node pend = R;
#pragma nounroll
    for (int h = 0; h < 2; ++h) {
        Node a, b;
        expand<B>(c.tab, c.lo, m, cw1, a, b);
        Blk oa, ob;
        mmo2<B>(c.tab, c.lo, KeyFixed<false>{}, a.s, oa, KeyFixed<false>{}, b.s, ob);
        oa = leaf_fix(oa, a.t, c.fcw);
        ob = leaf_fix(ob, b.t, c.fcw);
        o2 = oa;
        o3 = ob;
        if (h == 0) {
            o0 = oa;
            o1 = ob;
        }
        m = pend;
    }
    store16(p, o0);
    store16(p + 16, o1);
    store16(p + 32, o2);
    store16(p + 48, o3);
}

// Depth-first expansion of D more levels below node n at tree level `lvl0 +
// (DMAX - D)`; the right child of every internal node stays live in
// registers while the left subtree is expanded.  Leaf mode writes the
// converted leaves (dpf.go:214-224); node mode (NODES) writes the 2^D nodes
// D levels down instead: the frontier a batched Eval continues from.
// B: batched AES rounds (aes_ttable.hpp aes2_rounds) where the registers
// allow it: the one-key-per-wave kernels.
template <int DMAX, int D, bool NODES, bool PAIR, bool B, bool RAW = false>
__device__ __forceinline__ void dfs(Ctx& c, uint32_t lvl0, const Node& n) {
    if constexpr (PAIR && D == 3) {
        // Lane pairs write whole 128-B lines.  Lanes 2i and 2i+1 own adjacent
        // subtrees a and b of one key (same CWs), 16 << DMAX bytes apart, and
        // reach their depth-3 nodes Na, Nb in lockstep.  After expanding, the
        // even lane trades R(Na) for the odd lane's L(Nb): first the pair
        // computes Na's 8 leaves (even: 0-3, odd: 4-7) and stores the line in
        // one instruction, then Nb's.  Storing a line as two 64-B halves 8 AES
        // apart left ~4 MiB of half-written lines per XCD (its whole L2) and
        // made WRITE_SIZE 1.26x the output.  Leaves are unchanged, only which
        // lane computes them.
        CW cw = key_cw<RAW>(c.ks, lvl0 + DMAX - 3);
        Node L, R;
        expand<B>(c.tab, c.lo, n, cw, L, R);
        const bool odd = (threadIdx.x & 1u) != 0;
        const Node got = pair_swap(sel(odd, L, R));   // even gets L(Nb), odd gets R(Na)
        const int64_t sub = 16ll << DMAX;
        Node cur = sel(odd, got, L);
        const Node second = sel(odd, R, got);
#pragma nounroll
        for (int h = 0; h < 2; ++h) {   // one code copy of leaves4 (instruction cache)
            leaves4<B, RAW>(c, lvl0 + DMAX - 2, cur, c.outp + (h == 0 ? (odd ? 64 - sub : 0) : (odd ? 64 : sub)));
            prio_step<DMAX>(c);
            cur = second;
        }
        c.outp += 128;
    } else if constexpr (D == 0) {
        if constexpr (NODES) {
            emit_node(c, n);
        } else {
            Blk o = mmo1(c.tab, c.lo, KeyFixed<false>{}, n.s);
            store16(c.outp, leaf_fix(o, n.t, c.fcw));
            c.outp += 16;
        }
    } else if constexpr (D == 2 && !NODES) {
        // Bottom two levels at once: 4 leaves = 64 contiguous bytes stored back
        // to back (subtrees too shallow or lanes of different keys for PAIR).
        leaves4<B, RAW>(c, lvl0 + DMAX - 2, n, c.outp);
        prio_step<DMAX>(c);
        c.outp += 64;
    } else if constexpr (D == 2 && NODES) {
        // Bottom two levels of a frontier at once: 4 seeds = 64 contiguous
        // bytes and their 4 t bytes as one 32-bit store (one byte store per
        // node made the NODES pass write 2.2x its 17 B per node).
        CW cw = key_cw<RAW>(c.ks, lvl0 + DMAX - 2);
        Node L, R;
        expand<B>(c.tab, c.lo, n, cw, L, R);
        CW cw1 = key_cw<RAW>(c.ks, lvl0 + DMAX - 1);
        Node q[4];
        expand<B>(c.tab, c.lo, L, cw1, q[0], q[1]);
        expand<B>(c.tab, c.lo, R, cw1, q[2], q[3]);
#pragma unroll
        for (int i = 0; i < 4; ++i) c.nseed[i] = make_uint4(q[i].s.c0, q[i].s.c1, q[i].s.c2, q[i].s.c3);
        *reinterpret_cast<uint32_t*>(c.nt) = (q[0].t & 0xffu) | ((q[1].t & 0xffu) << 8) | ((q[2].t & 0xffu) << 16) |
                                             ((q[3].t & 0xffu) << 24);
        c.nseed += 4;
        c.nt += 4;
        prio_step<DMAX>(c);
    } else if constexpr (D == 1) {
        CW cw = key_cw<RAW>(c.ks, lvl0 + DMAX - 1);
        Node L, R;
        expand<B>(c.tab, c.lo, n, cw, L, R);
        if constexpr (NODES) {
            emit_node(c, L);
            emit_node(c, R);
        } else {
            Blk oL, oR;
            mmo2<B>(c.tab, c.lo, KeyFixed<false>{}, L.s, oL, KeyFixed<false>{}, R.s, oR);
            store16(c.outp, leaf_fix(oL, L.t, c.fcw));
            store16(c.outp + 16, leaf_fix(oR, R.t, c.fcw));
            c.outp += 32;
        }
    } else {
        CW cw = key_cw<RAW>(c.ks, lvl0 + DMAX - D);
        Node L, R;
        expand<B>(c.tab, c.lo, n, cw, L, R);
        // The right child is the only node live across the left subtree.
        Node ch = L;
        const Node pend = R;
#pragma nounroll
        for (int side = 0; side < 2; ++side) {
            dfs<DMAX, D - 1, NODES, PAIR, B, RAW>(c, lvl0, ch);
            ch = pend;
        }
    }
}

// Expand byte-layout DPF keys (dpf.go:89-92,111-112,137-138,165-167) into
// the aligned word records above.  One thread per (key, record).
__global__ void k_unpack(const uint8_t* __restrict__ keys, uint64_t key_len, uint64_t nkeys, uint32_t stop,
                         uint32_t* __restrict__ ek) {
    const uint64_t recs = (uint64_t)stop + 2;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nkeys * recs) return;
    const uint64_t k = i / recs, r = i % recs;
    const uint8_t* kp = keys + k * key_len;
    uint32_t* o = ek + k * (recs * 8) + r * 8;
    auto w = [](const uint8_t* p) {
        return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    };
    if (r == 0) {                         // root seed + t (dpf.go:244-246 / :175-176)
        o[0] = w(kp); o[1] = w(kp + 4); o[2] = w(kp + 8); o[3] = w(kp + 12);
        o[4] = kp[16]; o[5] = 0; o[6] = 0; o[7] = 0;
    } else if (r <= stop) {               // level r-1 CW (dpf.go:231-233)
        const uint8_t* p = kp + 17 + 18 * (r - 1);
        o[0] = w(p); o[1] = w(p + 4); o[2] = w(p + 8); o[3] = w(p + 12);
        o[4] = p[16]; o[5] = p[17]; o[6] = 0; o[7] = 0;
    } else {                              // final CW at len(k)-16 (dpf.go:206,219)
        const uint8_t* p = kp + key_len - 16;
        o[0] = w(p); o[1] = w(p + 4); o[2] = w(p + 8); o[3] = w(p + 12);
        o[4] = 0; o[5] = 0; o[6] = 0; o[7] = 0;
    }
}

// Batched / split EvalFull.  Thread u evaluates subtree `sub_base + (u mod
// 2^units_log)` at level ltop of key (u >> units_log), a block of 2^D leaves
// written at out + key*out_stride + (u mod 2^units_log) * 16 * 2^D.
// NODES: the same walk, but the 2^D nodes at level ltop + D are written to
// (uint4*)out / out_t at [key*out_stride + (u mod 2^units_log) * 2^D].
// Precondition: blockDim.x = 2^W, a power of two from 64 to kTreeBlockMax
// (dpfh::pick_block returns nothing else).  Which of its run-time forms a
// launch takes is written down in dpfh::TreeForm (tree_plan.hpp), whose rules
// for cw_lds, the walk kind and feedback are the ones this kernel applies.
template <int D, bool UNIFORM, bool NODES, bool RAW = false>
__global__ __launch_bounds__(kTreeBlockMax, kTreeWaves) void k_evalfull(const uint32_t* __restrict__ ekeys, uint32_t stop,
                                                        uint64_t nunits, uint32_t units_log, uint32_t ltop,
                                                        uint64_t sub_base, uint8_t* __restrict__ out,
                                                        uint8_t* __restrict__ out_t, uint64_t out_stride,
                                                        uint64_t klen = 0, uint64_t kboff = 0) {
    static_assert(!RAW || (UNIFORM && !NODES), "raw keys: wave-uniform leaf launches only");
#ifdef DPF_WAVE_TIMES
    const uint64_t t_start = wall_clock64();
#endif
    __shared__ __attribute__((aligned(16))) uint32_t s_tab[kTabWords];
    const uint32_t B = blockDim.x, W = 31u - (uint32_t)__builtin_clz(B);
    const uint64_t u = (uint64_t)blockIdx.x * B + threadIdx.x;
    uint64_t key = u >> units_log;
    if constexpr (UNIFORM) key = __builtin_amdgcn_readfirstlane((uint32_t)key);
    const uint64_t local = u & ((1ull << units_log) - 1);
    const uint64_t sub = sub_base + local;
    Ctx c;
    if constexpr (RAW) {
        c.ks = {nullptr, ekeys, kboff + key * klen, klen};   // ekeys: the raw key batch, 4-byte-aligned base
    } else {
        c.ks = {ekeys + key * ((uint64_t)(stop + 2) * 8), nullptr, 0, 0};
    }
    // Correction words of the walk levels 0..ltop-1 staged in LDS when the
    // whole workgroup evaluates one key (r05).  Read in the walk by scalar
    // loads, each level's CW put an s_waitcnt lgkmcnt(0) -- the counter the
    // T-table lookups also use -- into the middle of the level's dependent
    // AES rounds, exposing an L2 (or HBM) round trip per level of a walk
    // that runs while the CU is otherwise idle.  Here lane l of wave 0 loads
    // level l's CW with vector loads issued before the table fill, and the
    // walks read it from LDS (in-order returns: no wait beyond the round's own).
    // Rule: dpfh::tree_cw_lds (uniform && units_log >= W; stop <= 64 = dpfh::kCwLdsLevels always).
    __shared__ __attribute__((aligned(16))) uint32_t s_cw[8 * 64];
    const bool cw_lds = UNIFORM && stop <= 64 && units_log >= W && (uint64_t)blockIdx.x * B < nunits;   // workgroup-uniform
    const bool cw_mine = cw_lds && threadIdx.x < ltop;
    CW cw_pre{};
    if (cw_mine) cw_pre = key_cw<RAW>(c.ks, threadIdx.x);   // per-lane level: vector loads
    __shared__ __attribute__((aligned(16))) uint32_t s_prog[64];
    if (threadIdx.x < 64) s_prog[threadIdx.x] = 0xffffffffu;
    fill_table_nobar(s_tab);
    if (cw_mine) {
        *reinterpret_cast<uint4*>(s_cw + 8 * threadIdx.x) = make_uint4(cw_pre.s.c0, cw_pre.s.c1, cw_pre.s.c2, cw_pre.s.c3);
        *reinterpret_cast<uint2*>(s_cw + 8 * threadIdx.x + 4) = make_uint2(cw_pre.tl, cw_pre.tr);
    }
    __syncthreads();
    if (u >= nunits) return;
    auto lds_cw = [&](uint32_t lvl) __attribute__((always_inline)) {
        const uint4 a = *reinterpret_cast<const uint4*>(s_cw + 8 * lvl);
        const uint2 b = *reinterpret_cast<const uint2*>(s_cw + 8 * lvl + 4);
        return CW{{a.x, a.y, a.z, a.w}, b.x, b.y};
    };
    c.groups = 0;
    // Feedback priority only where the workgroup holds all 16 waves of its CU (one
    // kTreeBlockBig-thread workgroup per CU): with two workgroups per CU a
    // wave sees half of its SIMD's waves, and steering by them was 3% slower.
    // Rule: dpfh::tree_feedback.
    if (UNIFORM && !NODES && D >= (int)kFeedbackMinD && B == (uint32_t)kTreeBlockBig) {
        c.prog = prog_slots(s_prog, c.pslot);
        c.prog[c.pslot] = 0;
    }
    __builtin_amdgcn_s_setprio(3);
    c.tab = reinterpret_cast<const uint8_t*>(s_tab);
    c.lo = (threadIdx.x & 31u) * 4u;
    if constexpr (NODES) {
        c.nseed = reinterpret_cast<uint4*>(out) + key * out_stride + (local << D);
        c.nt = out_t + key * out_stride + (local << D);
    } else {
        c.fcw = key_fcw<RAW>(c.ks, stop);
        c.outp = out + key * out_stride + local * (16ull << D);
    }

    Node n;
    n.s = key_root<RAW>(c.ks, n.t);
    uint32_t lvl = 0;
    if constexpr (UNIFORM) {
        // Shared walk: when the whole workgroup evaluates consecutive
        // subtrees of one key (cw_lds), its threads' paths agree on the
        // top ltop - W levels and fan out to B nodes below.  Wave 0 walks
        // 64 paths down to level l1 = ltop - W + 6 (one per group of B/64
        // threads) and leaves them in LDS; every thread then walks only the
        // last W - 6 levels.  Wave-AES per workgroup: l1 + (B/64)(W - 6)
        // instead of (B/64) ltop (configs[4]: 33 vs 96, configs[3]: 39 vs 144).
        constexpr uint32_t F = 6, kFs = 1u << F;   // paths of the shared walk: 2^F
        __shared__ uint32_t s_front[5 * kFs];   // SoA: word k of node j at k * kFs + j
        if (W >= 7 && cw_lds) {   // uniform; which walk: dpfh::tree_walk, l1 as dpfh::TreeForm::l1
            const uint32_t l1 = ltop - W + F;
            auto put = [&](uint32_t j, const Node& m) {
                s_front[j] = m.s.c0; s_front[kFs + j] = m.s.c1; s_front[2 * kFs + j] = m.s.c2;
                s_front[3 * kFs + j] = m.s.c3; s_front[4 * kFs + j] = m.t;
            };
            auto get = [&](uint32_t j) {
                Node m;
                m.s = {s_front[j], s_front[kFs + j], s_front[2 * kFs + j], s_front[3 * kFs + j]};
                m.t = s_front[4 * kFs + j];
                return m;
            };
            if (W >= 8) {
                // 2^F paths on the first 2^(F-4) waves, one quad of lanes per
                // path (the latency form: the walk is serial, the CU nearly idle).
                if (threadIdx.x < (4u << F)) {
                    const uint32_t path = threadIdx.x >> 2, j = threadIdx.x & 3u;
                    const uint64_t subj = (sub - threadIdx.x) + ((uint64_t)path << (W - F));
                    const QuadKeys qk = quad_keys(j);
                    uint32_t col = j == 0 ? n.s.c0 : j == 1 ? n.s.c1 : j == 2 ? n.s.c2 : n.s.c3;
                    uint32_t t = n.t;
                    for (uint32_t i = 0; i < l1; ++i) {
                        const CW cw = lds_cw(i);
                        const uint32_t cwj = j == 0 ? cw.s.c0 : j == 1 ? cw.s.c1 : j == 2 ? cw.s.c2 : cw.s.c3;
                        walk_step_quad(c.tab, c.lo, qk, j, col, t, cwj, cw.tl, cw.tr,
                                       (uint32_t)(subj >> (ltop - 1 - i)) & 1u);
                    }
                    s_front[j * kFs + path] = col;
                    if (j == 0) s_front[4 * kFs + path] = t;
                }
            } else if (threadIdx.x < 64) {
                const uint64_t subj = (sub - threadIdx.x) + ((uint64_t)threadIdx.x << (W - 6));
                Node m = n;
                for (uint32_t i = 0; i < l1; ++i) {
                    CW cw = lds_cw(i);
                    walk_step<true>(c.tab, c.lo, m, cw, (uint32_t)(subj >> (ltop - 1 - i)) & 1u);
                }
                put(threadIdx.x, m);
            }
            __syncthreads();
            n = get(threadIdx.x >> (W - F));
            lvl = l1;
        }
    }
    if (cw_lds) {
        for (uint32_t i = lvl; i < ltop; ++i)
            walk_step<true>(c.tab, c.lo, n, lds_cw(i), (uint32_t)(sub >> (ltop - 1 - i)) & 1u);
    } else {
        for (uint32_t i = lvl; i < ltop; ++i)
            walk_step<true>(c.tab, c.lo, n, key_cw<RAW>(c.ks, i), (uint32_t)(sub >> (ltop - 1 - i)) & 1u);
    }
#ifdef DPF_WAVE_TIMES
    const uint64_t t_walk = wall_clock64();
#endif
    // Lane pairs share a key when a wave owns one key (UNIFORM): whole-line
    // leaf stores (dfs PAIR).
    constexpr bool kPair = UNIFORM && !NODES && D >= 3;
    dfs<D, D, NODES, kPair, UNIFORM, RAW>(c, ltop, n);
    if (c.prog != nullptr) c.prog[c.pslot] = 0xffffffffu;   // done: no longer the slowest
#ifdef DPF_WAVE_TIMES
    // Measurement build only (tools/wave_times.hip): per wave, start / end
    // (wall clock) and the hardware ids of the CU it ran on.
    if ((threadIdx.x & 63) == 0) {
        const uint64_t wv = u >> 6;
        if (wv < kWaveTimesMax) {
            g_wave_times[5 * wv] = t_start;
            g_wave_times[5 * wv + 1] = wall_clock64();
            g_wave_times[5 * wv + 2] = __builtin_amdgcn_s_getreg(0xF804);   // HW_ID
            g_wave_times[5 * wv + 3] = __builtin_amdgcn_s_getreg(0xF814);   // XCC_ID
            g_wave_times[5 * wv + 4] = t_walk;                              // root-to-subtree walk done
        }
    }
#endif
}

// Batched Eval: independent walks that compute only the child on the path
// (the reference computes both children, dpf.go:184), two queries per thread
// (q = 2u, 2u + 1): the two walks run in lockstep (same start level and
// length), so every AES round issues 32 lookups per wave instead of 16.
// Without a frontier a walk starts at the root: stop+1 AES per query.  With
// one (fseed != nullptr) it starts from the query's level-L node, written
// by the NODES pass: stop-L+1 AES.  Output: one 0/1 byte per query.
__device__ __forceinline__ Node eval_start(const uint32_t* ek, uint64_t key, uint64_t x, uint32_t logN,
                                           const uint4* fseed, const uint8_t* ft, uint32_t L) {
    Node n;
    if (fseed != nullptr) {
        const uint64_t idx = (key << L) + ((x >> (logN - L)) & ((1ull << L) - 1));
        const uint4 v = fseed[idx];
        n.s = {v.x, v.y, v.z, v.w};
        n.t = ft[idx];
    } else {
        n.s = load_blk(ek);
        n.t = ek[4];
    }
    return n;
}
struct PairIn {
    uint64_t x0, x1;
    Node n0, n1;
};
// UNI: every wave's 64 pairs (128 consecutive queries) belong to one key
// (pts_per_key a multiple of 128, launch_eval): the key index is wave-uniform,
// so its correction words come through scalar loads into SGPRs instead of
// two per-lane copies in VGPRs (12 fewer VGPRs in the walk: the kernel sits
// at the 128-VGPR limit of 4 waves per SIMD and spilled 35 without it).
template <bool UNI>
__device__ __forceinline__ uint64_t pair_key(uint64_t q, uint64_t pts_per_key) {
    const uint64_t k = q / pts_per_key;
    if constexpr (UNI) return __builtin_amdgcn_readfirstlane((uint32_t)k);
    return k;
}
// The pair's points and start nodes (frontier gathers): issued before the
// workgroup fills its table, so their HBM latency overlaps the fill.
template <bool UNI>
__device__ __forceinline__ PairIn eval_pair_in(const uint32_t* __restrict__ ekeys, uint32_t stop, uint32_t logN,
                                               const uint64_t* __restrict__ xs, uint64_t nq, uint64_t pts_per_key,
                                               const uint4* __restrict__ fseed, const uint8_t* __restrict__ ft,
                                               uint32_t L, uint64_t q0) {
    const uint64_t qa = q0 < nq ? q0 : nq - 1;
    const uint64_t q1 = qa + 1 < nq ? qa + 1 : qa;
    const uint64_t key0 = pair_key<UNI>(qa, pts_per_key), key1 = UNI ? key0 : q1 / pts_per_key;
    const uint64_t rec = (uint64_t)(stop + 2) * 8;
    PairIn p;
    p.x0 = xs[qa];
    p.x1 = xs[q1];
    p.n0 = eval_start(ekeys + key0 * rec, key0, p.x0, logN, fseed, ft, L);
    p.n1 = eval_start(ekeys + key1 * rec, key1, p.x1, logN, fseed, ft, L);
    return p;
}
// The pair's two answer bits (bit 0: query q0, bit 8: q0 + 1).
template <bool UNI>
__device__ __forceinline__ uint32_t eval_pair_bits(const uint32_t* __restrict__ ekeys, uint32_t stop, uint32_t logN,
                                                   uint64_t nq, uint64_t pts_per_key, const uint4* __restrict__ fseed,
                                                   uint32_t L, const uint32_t* s_tab, uint64_t q0, PairIn p,
                                                   const uint32_t* cwp = nullptr) {
    const uint64_t q1 = q0 + 1 < nq ? q0 + 1 : q0;
    const uint64_t key0 = pair_key<UNI>(q0, pts_per_key), key1 = UNI ? key0 : q1 / pts_per_key;
    const uint64_t rec = (uint64_t)(stop + 2) * 8;
    const uint32_t* ek0 = ekeys + key0 * rec;
    const uint32_t* ek1 = ekeys + key1 * rec;
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(s_tab);
    const uint32_t lo = (threadIdx.x & 31u) * 4u;
    const uint32_t i0 = fseed != nullptr ? L : 0;
    if (UNI && cwp != nullptr) {
        // The key's records from level i0 on, staged in LDS by the caller
        // (k_eval_persist): no scalar load -- whose lgkmcnt(0) would stall
        // the level's first AES round -- inside the walk.
        for (uint32_t i = i0; i < stop; ++i) {
            const uint4 a = *reinterpret_cast<const uint4*>(cwp + 8 * (i - i0));
            const uint2 b = *reinterpret_cast<const uint2*>(cwp + 8 * (i - i0) + 4);
            const CW cw{{a.x, a.y, a.z, a.w}, b.x, b.y};
            walk_step2<true>(tab, lo, p.n0, cw, path_bit(p.x0, logN - 1 - i), p.n1, cw,
                                       path_bit(p.x1, logN - 1 - i));
        }
    } else {
        for (uint32_t i = i0; i < stop; ++i) {
            const CW cw0 = load_cw(ek0, i), cw1 = UNI ? cw0 : load_cw(ek1, i);
            walk_step2<true>(tab, lo, p.n0, cw0, path_bit(p.x0, logN - 1 - i), p.n1, cw1,
                                       path_bit(p.x1, logN - 1 - i));
        }
    }
    Blk o0, o1;
    mmo2<true>(tab, lo, KeyFixed<false>{}, p.n0.s, o0, KeyFixed<false>{}, p.n1.s, o1);
    const Blk f0 = UNI && cwp != nullptr ? load_blk(cwp + 8 * (stop - i0)) : load_blk(ek0 + 8 + 8 * stop);
    o0 = leaf_fix(o0, p.n0.t, f0);
    o1 = leaf_fix(o1, p.n1.t, UNI ? f0 : load_blk(ek1 + 8 + 8 * stop));
    return (uint32_t)eval_bit(o0, p.x0) | ((uint32_t)eval_bit(o1, p.x1) << 8);
}
template <bool UNI>
__device__ __forceinline__ void eval_pair_walk(const uint32_t* __restrict__ ekeys, uint32_t stop, uint32_t logN,
                                               uint64_t nq, uint64_t pts_per_key, const uint4* __restrict__ fseed,
                                               uint32_t L, uint8_t* __restrict__ out, const uint32_t* s_tab,
                                               uint64_t q0, PairIn p) {
    const uint32_t b = eval_pair_bits<UNI>(ekeys, stop, logN, nq, pts_per_key, fseed, L, s_tab, q0, p);
    out[q0] = (uint8_t)b;
    if (q0 + 1 < nq) out[q0 + 1] = (uint8_t)(b >> 8);
}

template <bool UNI>
__global__ __launch_bounds__(kBlock, 4) void k_eval2(const uint32_t* __restrict__ ekeys, uint32_t stop,
                                                     uint32_t logN, const uint64_t* __restrict__ xs, uint64_t nq,
                                                     uint64_t pts_per_key, const uint4* __restrict__ fseed,
                                                     const uint8_t* __restrict__ ft, uint32_t L,
                                                     uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint32_t s_tab[kTabWords];
    // One query pair per thread (launch_eval sizes the grid so): short-lived
    // waves overlap their frontier gathers, where a grid capped at the
    // resident workgroups serialised them (3667 vs 3489 us at configs[2]).
    const uint64_t q0 = 2 * ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
    // The pair's points and frontier nodes are requested before the table
    // fill (a short-lived wave otherwise waits out their HBM latency after it).
    PairIn p{};
    if (q0 < nq) p = eval_pair_in<UNI>(ekeys, stop, logN, xs, nq, pts_per_key, fseed, ft, L, q0);
    fill_table(s_tab);
    __builtin_amdgcn_s_setprio(3);
    if (q0 < nq) eval_pair_walk<UNI>(ekeys, stop, logN, nq, pts_per_key, fseed, L, out, s_tab, q0, p);
}

// Eval of every key at a list of points, the answers as packed selection
// bits: key k meets list k / keys_per_list of xs[][npts] (one shared list:
// keys_per_list = nkeys; a grouped call: the keys of group g at group g's own
// points), and bit j % 8 of byte j / 8 of row `key` of bits[][bits_stride]
// is Eval(key, list[j]), EvalFull's bit order, so the rows feed the folds and
// the scatter as EvalFull output does.  The mapping, the tail rule and what
// the launch guarantees are written down in eval_bits_plan.hpp: wave w owns
// unit w % units (128 points) of key w / units; lane l walks points 128 u + l
// and 128 u + 64 + l in lockstep (the pair walk of k_eval2<true>: the key is
// wave-uniform at every npts, its records come by scalar loads); a lane past
// npts reads point npts - 1 and is masked out of the ballot; the two ballots
// are the unit's 16 bytes, stored by lane 0 as one vector store.  No per-key
// copy of the points, no byte per query, no atomics.
// (A batch would need 2^32 keys before the 32-bit readfirstlane of the key
// index, here and in pair_key, could truncate: their records alone are 256 GiB.)
__global__ __launch_bounds__(kBlock, 4) void k_eval_bits(const uint32_t* __restrict__ ekeys, uint32_t stop,
                                                         uint32_t logN, const uint64_t* __restrict__ xs, uint64_t npts,
                                                         uint64_t keys_per_list, uint64_t units, uint64_t nwaves,
                                                         const uint4* __restrict__ fseed,
                                                         const uint8_t* __restrict__ ft, uint32_t L,
                                                         uint8_t* __restrict__ bits, uint64_t bits_stride) {
    __shared__ __attribute__((aligned(16))) uint32_t s_tab[kTabWords];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t w = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wib;   // wave-uniform
    const bool live = w < nwaves;
    uint64_t key = 0, unit = 0, j0 = 0, j1 = 0;
    // The points and frontier nodes are requested before the table fill, as in k_eval2.
    PairIn p{};
    if (live) {
        key = w / units;
        unit = w - key * units;
        j0 = dpfh::eval_bits_point(unit, lane, 0);
        j1 = dpfh::eval_bits_point(unit, lane, 1);
        const uint32_t* ek = ekeys + key * ((uint64_t)(stop + 2) * 8);
        // The key's own list: its index (below 2^32 as the key's is) and its
        // base are wave-uniform and stay in scalar registers; the clamp is
        // within the list, so a tail lane never reads the next list's points.
        const uint32_t list = __builtin_amdgcn_readfirstlane((uint32_t)dpfh::eval_bits_list(key, keys_per_list));
        const uint64_t* lx = xs + dpfh::eval_bits_list_base(list, npts);
        p.x0 = lx[dpfh::eval_bits_clamp(j0, npts)];
        p.x1 = lx[dpfh::eval_bits_clamp(j1, npts)];
        p.n0 = eval_start(ek, key, p.x0, logN, fseed, ft, L);
        p.n1 = eval_start(ek, key, p.x1, logN, fseed, ft, L);
    }
    fill_table(s_tab);
    __builtin_amdgcn_s_setprio(3);
    if (!live) return;
    // eval_pair_bits<true> names its key as query / pts_per_key: query `key`
    // of a batch with one point per key.
    const uint32_t b = eval_pair_bits<true>(ekeys, stop, logN, key + 1, 1, fseed, L, s_tab, key, p);
    const uint64_t m0 = __builtin_amdgcn_ballot_w64((b & 1u) != 0 && j0 < npts);
    const uint64_t m1 = __builtin_amdgcn_ballot_w64(((b >> 8) & 1u) != 0 && j1 < npts);
    if (lane == 0)
        *reinterpret_cast<uint4*>(bits + key * bits_stride + dpfh::eval_bits_unit_off(unit)) =
            make_uint4((uint32_t)m0, (uint32_t)(m0 >> 32), (uint32_t)m1, (uint32_t)(m1 >> 32));
}

// Persistent batched Eval (r05): one 1024-thread workgroup per CU fills its
// T-table once and strides over the query pairs; the next pair's points and
// frontier nodes move into per-wave LDS slots by LDS-DMA
// (global_load_lds_dwordx4 / _dword) while the current pair walks, so they
// cost no VGPRs (k_eval2 sits at the 128-VGPR limit; a register prefetch of
// the next pair spilled and ran slower) and no
// workgroup waits out a fresh table fill or its first gathers.
// Pipeline per thread, iteration i: read x(i) and node(i) from LDS; read
// x(i+1), issue node(i+1)'s gathers; issue x(i+2); walk pair i.  The slots are
// this wave's own, so no barrier: the compiler waits vmcnt(0) before the first
// slot read of an iteration (the DMAs issued one walk earlier), and T-table
// reads (a different LDS object) never wait on them.
// UNI only: a wave's 64 pairs are 128 consecutive queries of one key, and nq
// is even (pts_per_key % 128 == 0), so a pair's points are one 16-byte load.
// (kEvalPBlock threads: tree_plan.hpp, with the grid that launch_eval gives it.)
constexpr uint32_t kEvalPrioFar = 3;   // prio_by_lead every 4 pairs: a lead of 4 is near, up to 4 * kEvalPrioFar far
struct EvalSlots {
    uint4 x[2][64];      // x(i), x(i+1): {x0, x1} as two uint64
    uint4 n0[64], n1[64]; // frontier seeds of pair i's two queries
    uint32_t t0[64], t1[64];   // aligned dwords holding their t bytes
    uint32_t cw[2][64];  // pair i's key records, levels L..stop-1 and the final CW (parity of i)
};
// s_waitcnt vmcnt(0) as a compiler memory barrier: the slot DMAs have
// landed and no slot read is hoisted above the wait (hipcc's own waits did
// not cover every slot read once the loop was rotated).
__device__ __forceinline__ void eval_vm0() {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
}
// s_waitcnt lgkmcnt(0) that is also a compiler memory barrier: this wave's
// LDS reads of a slot stay above it (and complete before it ends), and the
// LDS-DMA that overwrites the slot stays below it.
__device__ __forceinline__ void eval_lgkm0() {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
}
__device__ __forceinline__ void glds(const void* g, void* l, int size) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (size == 16)
        __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)l, 16, 0, 0);
    else
        __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)l, 4, 0, 0);
#else
    (void)g;
    (void)l;
    (void)size;
#endif
}
__global__ __launch_bounds__(kEvalPBlock, 1) void k_eval_persist(const uint32_t* __restrict__ ekeys, uint32_t stop,
                                                                 uint32_t logN, const uint64_t* __restrict__ xs,
                                                                 uint64_t nq, uint64_t pts_per_key,
                                                                 const uint4* __restrict__ fseed,
                                                                 const uint8_t* __restrict__ ft, uint32_t L,
                                                                 uint8_t* __restrict__ out) {
    // The table must sit at LDS address 0, where every lookup's address is
    // its byte index (the ds_read offset field is 16 bits): the stricter
    // alignment places it first.  Behind the 72 KiB of slots it cost one
    // v_add_u32 per lookup, 320 per walk level.
    __shared__ __attribute__((aligned(256))) uint32_t s_tab[kTabWords];
    __shared__ __attribute__((aligned(16))) EvalSlots s_sl[kEvalPBlock / 64];
    const uint32_t lane = threadIdx.x & 63;
    EvalSlots& sl = s_sl[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)];
    const uint64_t npairs = nq / 2;
    const uint64_t nthr = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t gt = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // every wave runs the same number of iterations (tail pairs clamped, not stored)
    const uint64_t iters = (npairs + nthr - 1) / nthr;
    auto pair_of = [&](uint64_t i) __attribute__((always_inline)) {
        const uint64_t p = i * nthr + gt;
        return p < npairs ? p : npairs - 1;
    };
    const uint64_t rec = (uint64_t)(stop + 2) * 8;
    const uint32_t ncw = (stop - L) * 8 + 4;
    const bool cw_slots = ncw <= 64;      // uniform; rule: dpfh::eval_cw_staged
    auto issue_x = [&](uint64_t i, int slot) __attribute__((always_inline)) {
        glds(xs + 2 * pair_of(i), &sl.x[slot][0], 16);
    };
    auto issue_nodes = [&](uint64_t i, int slot) __attribute__((always_inline)) {
        const uint4 xv = sl.x[slot][lane];
        const uint64_t x0 = ((uint64_t)xv.y << 32) | xv.x, x1 = ((uint64_t)xv.w << 32) | xv.z;
        const uint64_t key = pair_key<true>(2 * pair_of(i), pts_per_key);
        const uint64_t m = (1ull << L) - 1;
        const uint64_t i0 = (key << L) + ((x0 >> (logN - L)) & m), i1 = (key << L) + ((x1 >> (logN - L)) & m);
        eval_lgkm0();                                    // this wave's reads of the node slots are done
        glds(fseed + i0, &sl.n0[0], 16);
        glds(fseed + i1, &sl.n1[0], 16);
        glds(ft + (i0 & ~3ull), &sl.t0[0], 4);
        glds(ft + (i1 & ~3ull), &sl.t1[0], 4);
        // The key's records from level L: 8 words per level, then the final
        // CW (dpf.go:186-188, :206), one word per lane.  Slot parity i & 1:
        // walk i - 2 (the slot's last reader) is done, by the wait above.
        if (cw_slots && lane < ncw) glds(ekeys + key * rec + 8 + 8 * L + lane, &sl.cw[slot][0], 4);
    };
    // Pair i's points and nodes into registers, after vmcnt(0): the slot
    // DMAs, issued one walk earlier, and the previous pair's output stores,
    // issued after the previous wait -- so a walk's stores are never waited
    // on right after they issue.
    auto read_pair = [&](uint64_t i) __attribute__((always_inline)) {
        eval_vm0();
        PairIn p;
        const uint4 xv = sl.x[i & 1][lane];
        p.x0 = ((uint64_t)xv.y << 32) | xv.x;
        p.x1 = ((uint64_t)xv.w << 32) | xv.z;
        const uint4 a = sl.n0[lane], b = sl.n1[lane];
        const uint64_t key = pair_key<true>(2 * pair_of(i), pts_per_key);
        const uint64_t m = (1ull << L) - 1;
        const uint32_t i0 = (uint32_t)((key << L) + ((p.x0 >> (logN - L)) & m)) & 3u;
        const uint32_t i1 = (uint32_t)((key << L) + ((p.x1 >> (logN - L)) & m)) & 3u;
        p.n0.s = {a.x, a.y, a.z, a.w};
        p.n1.s = {b.x, b.y, b.z, b.w};
        p.n0.t = (sl.t0[lane] >> (8 * i0)) & 0xffu;
        p.n1.t = (sl.t1[lane] >> (8 * i1)) & 0xffu;
        return p;
    };
    if (iters == 0) return;                               // uniform over the grid
    // Wave-progress slots per SIMD, as the tree kernel's prio_step feedback form.
    __shared__ __attribute__((aligned(16))) uint32_t s_prog[64];
    if (threadIdx.x < 64) s_prog[threadIdx.x] = 0xffffffffu;
    issue_x(0, 0);
    if (iters > 1) issue_x(1, 1);
    fill_table(s_tab);
    __builtin_amdgcn_s_setprio(3);
    uint32_t pslot;
    uint32_t* prog = prog_slots(s_prog, pslot);
    prog[pslot] = 0;
    issue_nodes(0, 0);
    PairIn p = read_pair(0);
    if (iters > 1) issue_nodes(1, 1);
    if (iters > 2) {
        eval_lgkm0();
        issue_x(2, 0);
    }
    for (uint64_t it = 0; it < iters; ++it) {
        if ((it & 3) == 0) prio_by_lead(prog, pslot, (uint32_t)it, 4, 4 * kEvalPrioFar);   // progress: pairs walked
        const uint64_t pr = it * nthr + gt;
        const uint32_t* cwp = cw_slots ? &sl.cw[it & 1][0] : nullptr;
        const uint32_t b = eval_pair_bits<true>(ekeys, stop, logN, nq, pts_per_key, fseed, L, s_tab, 2 * pair_of(it), p,
                                                cwp);
        // unconditional (the last iteration rereads its own slots): a
        // conditional read leaves the DMAs possibly pending at the join, and
        // the compiler then waits on this pair's stores before issue_nodes
        p = read_pair(it + 1 < iters ? it + 1 : it);
        if (pr < npairs) {
            out[2 * pr] = (uint8_t)b;
            out[2 * pr + 1] = (uint8_t)(b >> 8);
        }
        if (it + 2 < iters) issue_nodes(it + 2, (int)(it & 1));
        if (it + 3 < iters) {
            eval_lgkm0();
            issue_x(it + 3, (int)((it + 1) & 1));
        }
    }
    prog[pslot] = 0xffffffffu;
}

// aes128MMO microbenchmark / self-test on the T-table back end: two
// independent blocks per thread (the PRG's own ILP), iterated `reps` times.
template <bool RIGHT>
__global__ __launch_bounds__(kBlock, 4) void k_mmo_tt(const uint4* __restrict__ in, uint4* __restrict__ out,
                                                      uint64_t npairs, uint32_t reps) {
    __shared__ __attribute__((aligned(16))) uint32_t s_tab[kTabWords];
    fill_table(s_tab);
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= npairs) return;
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(s_tab);
    const uint32_t lo = (threadIdx.x & 31u) * 4u;
    const uint4 va = in[2 * u], vb = in[2 * u + 1];
    Blk a = {va.x, va.y, va.z, va.w}, b = {vb.x, vb.y, vb.z, vb.w};
    for (uint32_t r = 0; r < reps; ++r) mmo2<true>(tab, lo, KeyFixed<RIGHT>{}, a, a, KeyFixed<RIGHT>{}, b, b);
    out[2 * u] = make_uint4(a.c0, a.c1, a.c2, a.c3);
    out[2 * u + 1] = make_uint4(b.c0, b.c1, b.c2, b.c3);
}

// ------------------------------------------------------------ launchers ---

hipError_t launch_mmo_tt(const uint8_t* in, uint8_t* out, uint64_t nblocks, uint32_t right, uint32_t reps,
                         hipStream_t st) {
    const uint64_t pairs = nblocks / 2;
    if (pairs == 0) return hipSuccess;
    const dim3 grid((uint32_t)((pairs + kBlock - 1) / kBlock));
    if (right)
        hipLaunchKernelGGL(k_mmo_tt<true>, grid, dim3(kBlock), 0, st, reinterpret_cast<const uint4*>(in),
                           reinterpret_cast<uint4*>(out), pairs, reps);
    else
        hipLaunchKernelGGL(k_mmo_tt<false>, grid, dim3(kBlock), 0, st, reinterpret_cast<const uint4*>(in),
                           reinterpret_cast<uint4*>(out), pairs, reps);
    return hipGetLastError();
}

hipError_t launch_unpack(const uint8_t* keys, uint64_t key_len, uint64_t nkeys, uint32_t stop, uint32_t* ek,
                         hipStream_t st) {
    const uint64_t n = nkeys * ((uint64_t)stop + 2);
    if (n == 0) return hipSuccess;
    const uint32_t blocks = (uint32_t)((n + 255) / 256);
    hipLaunchKernelGGL(k_unpack, dim3(blocks), dim3(256), 0, st, keys, key_len, nkeys, stop, ek);
    return hipGetLastError();
}

// CUs a launch may occupy: the calling thread's budget when the C ABI set
// one (a stream created with a CU mask, dpf_stream_create_cu_masked), else
// the device's.  Grid shapes (one round of resident waves, the depth model)
// are sized to it, so a kernel on a 64-CU stream does not queue 4 rounds.
static thread_local int t_cu_budget = 0;
void set_cu_budget(int cus) { t_cu_budget = cus; }
int cu_budget() { return t_cu_budget; }
int cu_count() {
    if (t_cu_budget > 0) return t_cu_budget;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        cus = 256;
    return cus;
}

// The measurement switches of the launch plans (tree_plan.hpp), read from the
// environment once per process.
const dpfh::TreeKnobs& tree_knobs() {
    static const dpfh::TreeKnobs knobs = [] {
        dpfh::TreeKnobs k;
        if (const char* e = getenv("DPF_SUBTREE_DEPTH")) k.forced_depth = atoi(e);
        if (const char* e = getenv("DPF_RAW_KEYS")) k.raw_keys = e[0] != '0';
        if (const char* e = getenv("DPF_EVAL_PERSIST"); e && *e) k.eval_persist = atoi(e);
        if (const char* e = getenv("DPF_EVAL_UNIFORM")) k.eval_uniform = e[0] != '0';
        if (const char* e = getenv("DPF_EVAL_LEVEL_SHIFT"); e && *e) k.eval_level_shift = atoi(e);
        if (const char* e = getenv("DPF_EVAL_MODE")) k.eval_plain = e[0] == 'p';
        return k;
    }();
    return knobs;
}

// The plan of a tree launch (dpfh::tree_form: depth, workgroup, grid and the
// kernel form) for the calling thread's CU budget; false when it is refused.
static bool tree_launch(uint64_t nkeys, uint32_t depth, uint32_t prefix_bits, uint64_t prefix, bool nodes, bool raw,
                        dpfh::TreeForm* t) {
    return dpfh::tree_form(nkeys, depth, prefix_bits, prefix, nodes, raw, (uint64_t)cu_count(),
                           tree_knobs().forced_depth, t);
}
// f(std::integral_constant<int, D>) for the run-time depth d <= kMaxD.
template <class F>
static void with_depth(uint32_t d, F&& f) {
    switch (d) {
        case 0: return f(std::integral_constant<int, 0>{});
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        default: return f(std::integral_constant<int, 7>{});
    }
}

// Tree pass over every key: leaves of the subtree (prefix_bits, prefix) when
// NODES is false, the 2^depth nodes at level `depth` (prefix 0) when true.
template <bool NODES>
static hipError_t launch_tree(const uint32_t* ek, uint64_t nkeys, uint32_t stop, uint32_t depth,
                              uint32_t prefix_bits, uint64_t prefix, uint8_t* out, uint8_t* out_t,
                              uint64_t out_stride, hipStream_t st) {
    dpfh::TreeForm t;
    if (!tree_launch(nkeys, depth, prefix_bits, prefix, NODES, false, &t)) return hipErrorInvalidValue;
    if (t.nunits == 0) return hipSuccess;
    const dim3 grid((uint32_t)t.grid), block(t.block);
    with_depth(t.d, [&](auto dd) {
        constexpr int D = decltype(dd)::value;
        if (t.uniform)
            hipLaunchKernelGGL((k_evalfull<D, true, NODES>), grid, block, 0, st, ek, stop, t.nunits, t.units_log,
                               t.ltop, t.sub_base, out, out_t, out_stride);
        else
            hipLaunchKernelGGL((k_evalfull<D, false, NODES>), grid, block, 0, st, ek, stop, t.nunits, t.units_log,
                               t.ltop, t.sub_base, out, out_t, out_stride);
    });
    return hipGetLastError();
}

// One-shot EvalFull straight from the key bytes (RAW): where
// dpfh::evalfull_raw_ok (every wave owns one key, DPF_RAW_KEYS not 0).  Any
// key alignment: the kernel reads from the 4-byte-aligned base below `keys`.
bool evalfull_raw_ok(uint64_t nkeys, uint32_t stop, uint32_t prefix_bits) {
    return dpfh::evalfull_raw_ok(nkeys, stop, prefix_bits, (uint64_t)cu_count(), tree_knobs());
}

hipError_t launch_evalfull_raw(const uint8_t* keys, uint64_t klen, uint64_t nkeys, uint32_t stop, uint32_t prefix_bits,
                               uint64_t prefix, uint8_t* out, uint64_t out_stride, hipStream_t st) {
    dpfh::TreeForm t;
    if (!tree_launch(nkeys, stop, prefix_bits, prefix, false, true, &t) || !t.uniform) return hipErrorInvalidValue;
    // Aligned base below the batch, the batch's offset from it in kboff.
    const uint64_t kboff = (uintptr_t)keys & 3;
    const uint32_t* kw = reinterpret_cast<const uint32_t*>(keys - kboff);
    const dim3 grid((uint32_t)t.grid), block(t.block);
    with_depth(t.d, [&](auto dd) {
        hipLaunchKernelGGL((k_evalfull<decltype(dd)::value, true, false, true>), grid, block, 0, st, kw, stop,
                           t.nunits, t.units_log, t.ltop, t.sub_base, out, nullptr, out_stride, klen, kboff);
    });
    return hipGetLastError();
}

hipError_t launch_nodes(const uint32_t* ek, uint64_t nkeys, uint32_t stop, uint32_t depth, uint32_t prefix_bits,
                        uint64_t prefix, uint8_t* seeds, uint8_t* ts, uint64_t stride, hipStream_t st) {
    return launch_tree<true>(ek, nkeys, stop, depth, prefix_bits, prefix, seeds, ts, stride, st);
}

hipError_t launch_evalfull(const uint32_t* ek, uint64_t nkeys, uint32_t stop, uint32_t prefix_bits,
                           uint64_t prefix, uint8_t* out, uint64_t out_stride, hipStream_t st) {
    return launch_tree<false>(ek, nkeys, stop, stop, prefix_bits, prefix, out, nullptr, out_stride, st);
}

// The frontier's level and size (tree_plan.hpp) under DPF_EVAL_LEVEL_SHIFT.
uint32_t eval_frontier_level(uint32_t stop, uint64_t pts_per_key) {
    return dpfh::eval_frontier_level(stop, pts_per_key, tree_knobs().eval_level_shift);
}

uint64_t eval_frontier_bytes(uint64_t nkeys, uint32_t stop, uint64_t pts_per_key) {
    return dpfh::eval_frontier_bytes(nkeys, stop, pts_per_key, tree_knobs().eval_level_shift);
}

// Batched Eval kernel (dpf_set_eval_kernel): 0 = frontier + per-query walks,
// 1 = the trie kernel (eval_trie.hip, the experimental library only) where
// eval_trie_ok holds.  Env DPF_EVAL_TRIE=0|1 sets the initial value.
static std::atomic<int> g_eval_trie{[] {
    const char* e = getenv("DPF_EVAL_TRIE");
    return eval_trie_built() && e && e[0] == '1' ? 1 : 0;
}()};
static bool trie_on() { return g_eval_trie.load(std::memory_order_relaxed) != 0; }
int set_eval_trie(int on) { return g_eval_trie.exchange(on ? 1 : 0); }
int get_eval_trie() { return g_eval_trie.load(); }

hipError_t launch_eval(const uint32_t* ek, uint32_t stop, uint32_t logN, const uint64_t* xs, uint64_t nq,
                       uint64_t pts_per_key, uint8_t* out, void* frontier, uint64_t frontier_bytes,
                       hipStream_t st) {
    if (nq == 0) return hipSuccess;
    // The whole choice (frontier level, kernel, grid) is dpfh::eval_form's.
    const uint64_t nkeys = nq / pts_per_key;
    const bool xs16 = (reinterpret_cast<uintptr_t>(xs) & 15u) == 0;
    dpfh::EvalForm f;
    if (!dpfh::eval_form(nq, pts_per_key, stop, logN, frontier == nullptr ? 0 : frontier_bytes, xs16,
                         (uint64_t)cu_count(), tree_knobs(), &f))
        return hipErrorInvalidValue;
    const uint32_t L = f.L;
    const uint4* fseed = nullptr;
    const uint8_t* ft = nullptr;
    if (L > 0) {
        uint8_t* fs = static_cast<uint8_t*>(frontier);
        uint8_t* fts = fs + (nkeys << L) * 16;
        hipError_t e = launch_tree<true>(ek, nkeys, stop, L, 0, 0, fs, fts, 1ull << L, st);
        if (e != hipSuccess) return e;
        fseed = reinterpret_cast<const uint4*>(fs);
        ft = fts;
    }
    if (L > 0 && trie_on() && nq == nkeys * pts_per_key && eval_trie_ok(stop, logN, pts_per_key, L))
        return launch_eval_trie(ek, stop, logN, xs, nkeys, pts_per_key, fseed, ft, L, out, st);
    const dim3 grid((uint32_t)f.grid), block(f.block);
    if (f.kernel == dpfh::kEvalPersist)
        hipLaunchKernelGGL(k_eval_persist, grid, block, 0, st, ek, stop, logN, xs, nq, pts_per_key, fseed, ft, L, out);
    else if (f.kernel == dpfh::kEvalPairUniform)
        hipLaunchKernelGGL(k_eval2<true>, grid, block, 0, st, ek, stop, logN, xs, nq, pts_per_key, fseed, ft, L, out);
    else
        hipLaunchKernelGGL(k_eval2<false>, grid, block, 0, st, ek, stop, logN, xs, nq, pts_per_key, fseed, ft, L, out);
    return hipGetLastError();
}

hipError_t launch_eval_bits(const uint32_t* ek, uint32_t stop, uint32_t logN, const uint64_t* xs, uint64_t nkeys,
                            uint64_t keys_per_list, uint64_t npts, uint8_t* bits, uint64_t bits_stride, void* frontier,
                            uint64_t frontier_bytes, hipStream_t st) {
    if (nkeys == 0 || npts == 0) return hipSuccess;
    // The whole choice (frontier level, block, grid, units, lists) is dpfh::eval_bits_form_lists'.
    dpfh::EvalBitsForm f;
    if (!dpfh::eval_bits_form_lists(nkeys, keys_per_list, npts, stop, logN, frontier == nullptr ? 0 : frontier_bytes,
                                    (uint64_t)cu_count(), tree_knobs(), &f))
        return hipErrorInvalidValue;
    if (bits_stride % 16 != 0 || bits_stride < dpfh::eval_bits_stride(npts)) return hipErrorInvalidValue;
    const uint4* fseed = nullptr;
    const uint8_t* ft = nullptr;
    if (f.L > 0) {
        uint8_t* fs = static_cast<uint8_t*>(frontier);
        uint8_t* fts = fs + (nkeys << f.L) * 16;
        hipError_t e = launch_tree<true>(ek, nkeys, stop, f.L, 0, 0, fs, fts, 1ull << f.L, st);
        if (e != hipSuccess) return e;
        fseed = reinterpret_cast<const uint4*>(fs);
        ft = fts;
    }
    hipLaunchKernelGGL(k_eval_bits, dim3((uint32_t)f.grid), dim3(f.block), 0, st, ek, stop, logN, xs, (uint64_t)npts,
                       f.keys_per_list, f.units, f.nwaves, fseed, ft, f.L, bits, bits_stride);
    return hipGetLastError();
}

}  // namespace dpfk
