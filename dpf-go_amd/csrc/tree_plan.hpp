// tree_plan.hpp — the host arithmetic behind every tree launch (k_evalfull:
// leaves, nodes, raw keys) and every batched-Eval launch (k_eval_persist,
// k_eval2): per-thread subtree depth, workgroup size, grid, and which of the
// kernel's run-time forms a launch takes.  Pure functions of (shape, CU count,
// measurement switches); host-only and header-only (no HIP), so
// tests/c/tree_plan_test.cpp runs them under ASan/UBSan without a device.
// The launchers (dpf_kernels.hip) read the environment and the CU count, ask
// this header, and launch what it says.
//
// What a plan guarantees, and no kernel can check:
//   - the threads' output ranges tile every key's output exactly once;
//   - a workgroup that takes the shared walk (cw_lds) has no thread past
//     nunits: the walk's barrier comes after the kernel's `u >= nunits` exit;
//   - s_cw (64 levels) holds every level such a workgroup walks;
//   - the grid fits 31 bits (refused otherwise, never truncated).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

namespace dpfh {

// ---- geometry --------------------------------------------------------------
constexpr int kBlock = 512;    // threads per workgroup (8 waves); 2 workgroups per CU (64 KiB LDS table each)
// Tree kernel geometry: 2 workgroups of kTreeBlock threads per CU (LDS-bound),
// kTreeWaves waves per SIMD (VGPR budget).  Leaf launches with deep
// per-thread subtrees (D >= kBigMinD: configs[1], configs[3]) use one
// kTreeBlockBig-thread workgroup per CU instead, so that all 16 waves of a CU
// share one LDS and can balance their progress (prio_step feedback form).
constexpr int kTreeBlock = 512;
constexpr int kTreeBlockBig = 1024;
constexpr int kTreeBlockMax = 1024;
constexpr uint32_t kBigMinD = 6;
constexpr uint32_t kFeedbackMinD = 6;   // progress feedback needs enough groups per thread
constexpr int kTreeWaves = 4;
constexpr uint32_t kMaxD = 7;  // per-thread DFS subtree depth: 128 leaves = 2 KiB of output per thread
constexpr uint32_t kMaxFrontierHbm = 16;  // batched Eval, HBM frontier: deepest shared level
constexpr int kEvalPBlock = 1024;         // k_eval_persist: one workgroup per CU
constexpr uint32_t kPrioSmallMaxD = 5;    // prio_step: subtrees of <= 2^5 leaf blocks step at 1/2, 3/4, 7/8
constexpr uint32_t kWalkFanLog = 6;       // shared walk: 2^6 paths, left in LDS at level l1
constexpr uint32_t kCwLdsLevels = 64;     // s_cw: correction words of the walk levels a workgroup stages
constexpr uint32_t kEvalCwSlotWords = 64; // EvalSlots::cw: one word per lane
constexpr uint64_t kMaxGrid = 0x7fffffffull;
// The feedback form needs every wave of a CU (16 = 4 SIMDs x kTreeWaves) in one workgroup.
static_assert(kTreeBlockBig == 64 * 16, "feedback priority: one workgroup holds all 16 waves of its CU");
static_assert(kTreeBlockBig <= kTreeBlockMax && kTreeBlock <= kTreeBlockMax, "k_evalfull's launch bounds");

// ---- measurement switches (read from the environment by dpf_kernels.hip) ----
struct TreeKnobs {
    int forced_depth = -1;       // DPF_SUBTREE_DEPTH: per-thread subtree depth (< 0: the model's choice)
    bool raw_keys = true;        // DPF_RAW_KEYS=0: no launch straight from the key bytes
    int eval_persist = 1;        // DPF_EVAL_PERSIST=0: never k_eval_persist
    bool eval_uniform = true;    // DPF_EVAL_UNIFORM=0: never k_eval2<true>
    int eval_level_shift = 0;    // DPF_EVAL_LEVEL_SHIFT=n: the frontier n levels deeper
    bool eval_plain = false;     // DPF_EVAL_MODE=plain: root walks
};

inline uint32_t log2u(uint32_t pow2) {
    uint32_t w = 0;
    while ((1u << w) < pow2) ++w;
    return w;
}

// Workgroup size for a grid of n threads: full maxb-thread groups (maxb a
// power of two) once the grid covers every CU, otherwise the smallest power
// of two (>= one wave) that spreads it over all CUs, so that a small batch is
// not packed onto a few CUs whose LDS pipe then serialises it.
inline uint32_t pick_block(uint64_t n, uint32_t maxb, uint64_t cus) {
    uint32_t b = 64;
    while (b < maxb && n > cus * b) b <<= 1;
    return b;
}

// Per-thread subtree depth D and workgroup size.  A thread walks span - D
// levels (one AES each) and expands 3 * 2^D - 2 AES depth-first: deeper
// subtrees amortise the walk, shallower ones give more, shorter threads.
// Time model fitted to tools/archive/exp_latency.sh on MI355X (all batch shapes
// within ~8%): a thread's AES take max(kLat, w * kPerWave) each, w = waves
// per CU (<= 16; more threads run in further rounds).  The throughput regime
// (4096 keys x logN=20) takes D = 7; one key at logN=20 takes D = 0, 14 AES
// deep per thread instead of 197 at D = 7.
// forced >= 0 (DPF_SUBTREE_DEPTH) overrides the choice (measurement only).
struct TreeShape {
    uint32_t d, block;
};
inline TreeShape pick_shape(uint32_t span, uint64_t nkeys, bool nodes, uint32_t prefix_bits, uint64_t cus,
                            int forced) {
    const uint32_t dmax = span < kMaxD ? span : kMaxD;
    auto threads = [&](uint32_t dd) { return span - dd >= 40 ? ~0ull : nkeys << (span - dd); };
    auto block = [&](uint32_t dd) {
        return pick_block(threads(dd), !nodes && dd >= kBigMinD ? (uint32_t)kTreeBlockBig : (uint32_t)kTreeBlock,
                          cus);
    };
    if (forced >= 0) {
        const uint32_t d = dmax < (uint32_t)forced ? dmax : (uint32_t)forced;
        return {d, block(d)};
    }
    constexpr double kLat = 1.9e-6;       // one AES-MMO of a thread on a lightly loaded CU
    constexpr double kPerWave = 0.2e-6;   // ... per resident wave when the CU's LDS pipe is shared
    const double wave_slots = 64.0 * (double)(int)cus;
    uint32_t best = dmax;
    double best_t = 1e30;
    for (int dd = (int)dmax; dd >= 0; --dd) {
        const uint32_t d = (uint32_t)dd;
        double walk = (double)(span - d), lat = 0.0;
        const double w = (double)threads(d) / wave_slots;                 // waves per CU
        const double rounds = w > 16.0 ? std::ceil(w / 16.0) : 1.0;
        const double per = w > 16.0 ? 16.0 * kPerWave : std::max(kLat, w * kPerWave);
        // The shared workgroup walk (k_evalfull): one wave walks the top
        // ltop - W + 6 levels alone (latency, once per round of workgroups),
        // every thread the last W - 6.
        const uint32_t W = log2u(block(d));
        if (W >= 7 && span - d >= W) {
            walk = (double)(W - 6);
            lat = (double)(span + prefix_bits - d - W + 6) * kLat;
        }
        const double work = walk + (nodes ? 2.0 : 3.0) * (double)(1u << d) - 2.0;   // NODES: no leaf AES
        const double t = rounds * (lat + work * std::max(kLat, per));
        if (t < best_t * 0.98) {          // prefer the deeper subtree on near-ties (less total work)
            best_t = t;
            best = d;
        }
    }
    return {best, block(best)};
}

// ---- the form of a tree launch ----------------------------------------------
// Everything k_evalfull<D, UNIFORM, NODES, RAW> branches on, template
// arguments and run-time conditions alike.  The kernel derives cw_lds, the
// walk kind and feedback itself; the rules are stated once, here, and its
// comments cite them.
enum TreeWalk { kWalkNone = 0, kWalkLane = 1, kWalkQuad = 2 };

// UNIFORM: every wave owns one key.
inline bool tree_uniform(uint32_t units_log) { return units_log >= 6; }
// A whole workgroup evaluates consecutive subtrees of one key: its correction
// words sit in LDS (stop <= 56 < kCwLdsLevels always holds).
inline bool tree_cw_lds(bool uniform, uint32_t units_log, uint32_t W) { return uniform && units_log >= W; }
// Shared walk of such a workgroup: none at one wave, one lane per path at
// two waves, a quad of lanes per path from four waves on.
inline TreeWalk tree_walk(bool cw_lds, uint32_t W) {
    return !cw_lds || W < 7 ? kWalkNone : W >= 8 ? kWalkQuad : kWalkLane;
}
// Progress-feedback priority: leaf launches whose workgroup holds all 16 waves of its CU.
inline bool tree_feedback(bool uniform, bool nodes, uint32_t d, uint32_t block) {
    return uniform && !nodes && d >= kFeedbackMinD && block == (uint32_t)kTreeBlockBig;
}

struct TreeForm {
    uint32_t d;           // per-thread subtree depth
    uint32_t block, W;    // workgroup size 2^W
    uint32_t ltop;        // levels walked per thread
    uint32_t units_log;   // threads per key = 2^units_log
    uint64_t nunits, grid, sub_base;
    bool uniform, nodes, raw, cw_lds;
    TreeWalk walk;
    uint32_t l1;          // level the shared walk leaves its 64 paths at (0 without one)
    bool feedback, prio_small;
};

// What a tree launch over the subtrees (prefix_bits, prefix) down to level
// `depth` of every key derives from pick_shape; shared by the leaf, node and
// raw-key launches.  `raw`: the launch reads the key bytes themselves.  False
// when the grid would exceed kMaxGrid workgroups (f is then not to be used).
// Needs prefix_bits <= depth <= 56.
inline bool tree_form(uint64_t nkeys, uint32_t depth, uint32_t prefix_bits, uint64_t prefix, bool nodes, bool raw,
                      uint64_t cus, int forced, TreeForm* f) {
    const TreeShape sh = pick_shape(depth - prefix_bits, nkeys, nodes, prefix_bits, cus, forced);
    TreeForm t{};
    t.d = sh.d;
    t.block = sh.block;
    t.W = log2u(sh.block);
    t.ltop = depth - sh.d;
    t.units_log = t.ltop - prefix_bits;
    // nkeys << units_log would wrap: such a grid is refused as too large.
    if (nkeys > (~0ull >> t.units_log)) return false;
    t.nunits = nkeys << t.units_log;
    t.sub_base = prefix << t.units_log;
    t.grid = t.nunits / sh.block + (t.nunits % sh.block != 0);
    if (t.grid > kMaxGrid) return false;
    t.uniform = tree_uniform(t.units_log);
    t.nodes = nodes;
    t.raw = raw;
    t.cw_lds = tree_cw_lds(t.uniform, t.units_log, t.W);
    t.walk = tree_walk(t.cw_lds, t.W);
    t.l1 = t.walk == kWalkNone ? 0 : t.ltop - t.W + kWalkFanLog;
    t.feedback = tree_feedback(t.uniform, nodes, t.d, t.block);
    t.prio_small = t.d <= kPrioSmallMaxD;
    *f = t;
    return true;
}

// One-shot EvalFull straight from the key bytes (RAW): only where every wave
// owns one key (the shape the leaf launch would pick has >= 64 threads per
// key) and DPF_RAW_KEYS is not 0 (measurement switch).
inline bool evalfull_raw_ok(uint64_t nkeys, uint32_t stop, uint32_t prefix_bits, uint64_t cus, const TreeKnobs& k) {
    if (!k.raw_keys || nkeys == 0 || prefix_bits > stop) return false;
    TreeForm f;
    return tree_form(nkeys, stop, prefix_bits, 0, false, true, cus, k.forced_depth, &f) && f.uniform;
}

// ---- batched Eval -------------------------------------------------------------
// Shared frontier at the deepest level L whose nodes a key's points cover
// twice over on average: 2^(L+1) <= ppk, i.e. >= 2 points per frontier
// node (L = 9 at 1024 points per key), used when L >= 4.
// shift (DPF_EVAL_LEVEL_SHIFT, measurement only): the frontier that many levels deeper.
inline uint32_t eval_frontier_level(uint32_t stop, uint64_t pts_per_key, int shift = 0) {
    uint32_t L = 0;
    while (L < kMaxFrontierHbm && L < stop && (2ull << (L + 1)) <= pts_per_key) ++L;
    if (L >= 4 && shift > 0 && L + (uint32_t)shift < stop && L + (uint32_t)shift <= kMaxFrontierHbm) L += shift;
    return L >= 4 ? L : 0;
}

// Seeds (16 B) then t bytes of the 2^L frontier nodes of every key, padded to 256 B.
inline uint64_t eval_frontier_bytes(uint64_t nkeys, uint32_t stop, uint64_t pts_per_key, int shift = 0) {
    const uint32_t L = eval_frontier_level(stop, pts_per_key, shift);
    if (L == 0) return 0;
    return ((nkeys << L) * 16 + (nkeys << L) + 255) & ~255ull;
}

// k_eval_persist keeps a pair's key records (levels L..stop-1, 8 words each,
// and the 4-word final CW) in a per-wave LDS slot of one word per lane when
// they fit; otherwise its walks read them by scalar loads.
inline bool eval_cw_staged(uint32_t stop, uint32_t L) { return (stop - L) * 8 + 4 <= kEvalCwSlotWords; }

enum EvalKernel { kEvalPersist = 0, kEvalPairUniform = 1, kEvalPair = 2, kEvalTrie = 3 };

struct EvalForm {
    uint32_t L;           // frontier level (0: every walk starts at the root)
    EvalKernel kernel;
    uint32_t block;
    uint64_t grid;
    bool cw_staged;       // k_eval_persist only: key records in LDS slots
    bool ragged;          // the last workgroup has threads without a pair
    TreeForm nodes;       // the frontier pass (L > 0)
};

// What launch_eval does with nq = nkeys * pts_per_key queries (nq > 0) and a
// frontier area of frontier_bytes (0: none), the trie kernel aside: where
// that one is selected and takes the shape (eval_trie_ok; the experimental
// library only), it replaces the query kernel chosen here and keeps L and
// the frontier pass.  False when a grid would exceed kMaxGrid.
inline bool eval_form(uint64_t nq, uint64_t pts_per_key, uint32_t stop, uint32_t logN, uint64_t frontier_bytes,
                      bool xs_aligned16, uint64_t cus, const TreeKnobs& k, EvalForm* out) {
    EvalForm e{};
    const uint64_t nkeys = nq / pts_per_key;
    e.L = eval_frontier_level(stop, pts_per_key, k.eval_level_shift);
    if (logN > 63 || k.eval_plain || frontier_bytes == 0 ||
        frontier_bytes < eval_frontier_bytes(nkeys, stop, pts_per_key, k.eval_level_shift))
        e.L = 0;
    if (e.L > 0 && !tree_form(nkeys, e.L, 0, 0, true, false, cus, k.forced_depth, &e.nodes)) return false;
    const bool whole = nq == nkeys * pts_per_key;
    // Persistent form (k_eval_persist): needs the frontier and wave-uniform
    // keys.  Its LDS-DMA stages a pair's two points with one 16-byte load
    // from xs + 2*pair, so it needs a 16-byte-aligned xs; an 8-byte-aligned
    // one (a torch slice xs[1:]) takes k_eval2, whose loads are 8 bytes wide.
    if (k.eval_persist && xs_aligned16 && e.L > 0 && pts_per_key % 128 == 0 && whole &&
        nq >= 2 * (uint64_t)kEvalPBlock) {
        const uint64_t want = (nq / 2 + kEvalPBlock - 1) / kEvalPBlock;
        e.kernel = kEvalPersist;
        e.block = kEvalPBlock;
        e.grid = want < cus ? want : cus;
        e.cw_staged = eval_cw_staged(stop, e.L);
        e.ragged = (nq / 2) % ((uint64_t)e.grid * kEvalPBlock) != 0;
        *out = e;
        return true;
    }
    // One pair per thread: no grid-stride loop to fall back on.
    const uint64_t nthreads = (nq + 1) / 2;
    e.block = pick_block(nthreads, kBlock, cus);
    e.grid = (nthreads + e.block - 1) / e.block;
    if (e.grid > kMaxGrid) return false;
    // Wave-uniform keys when every wave's 128 queries share one key.
    e.kernel = k.eval_uniform && pts_per_key % 128 == 0 && e.block % 64 == 0 ? kEvalPairUniform : kEvalPair;
    e.ragged = nthreads % e.block != 0;
    *out = e;
    return true;
}

}  // namespace dpfh
