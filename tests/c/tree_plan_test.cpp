// Stand-alone check of the tree and batched-Eval launch plans
// (dpf-go_amd/csrc/tree_plan.hpp): built with -fsanitize=address,undefined
// and run directly by tests/test_tree_plan_cpu.py.  No device, no library.
//
// 1. A sweep over (nkeys, stop, prefix_bits, leaf / node, CU count, forced
//    depth) checks what every plan must guarantee: minimal power-of-two
//    workgroups, output ranges that tile each key once, exact grids, refusal
//    of exactly the grids above 2^31 - 1, and the form rules the kernel
//    applies on its own (uniform, raw, cw_lds, walk kind, l1, feedback).
// 2. The same for the batched-Eval plan.
// 3. Recorded plans on 256 CUs: the benchmark shapes and the shapes of
//    tests/test_gpu_parity.py::test_every_subtree_depth per forced depth.
// 4. With the argument "forms": the distinct kernel forms that the universe
//    of tests/test_gpu_tree_forms.py reaches on 256, 64, 16 and 4 CUs, each
//    with its cheapest representative call, for the Python test to assert on.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <tuple>
#include <vector>

#include "tree_plan.hpp"

using namespace dpfh;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #c, g_ctx); \
            exit(1);                                                    \
        }                                                               \
    } while (0)
static char g_ctx[256] = "";

typedef unsigned __int128 u128;

static std::vector<uint64_t> nkeys_list(uint64_t upto) {
    std::vector<uint64_t> v;
    for (uint64_t n = 1; n <= 70; ++n) v.push_back(n);
    for (uint64_t n : {96, 128, 130, 256, 300, 512, 513, 1024, 2048, 2056, 4096, 4100, 65536})
        if (n <= upto) v.push_back(n);
    return v;
}
static bool pow2(uint32_t x) { return x != 0 && (x & (x - 1)) == 0; }

// ---- 1. every tree plan of the sweep ----------------------------------------
static void check_tree(uint64_t nkeys, uint32_t stop, uint32_t pb, bool nodes, uint64_t cus, int forced, size_t* nok,
                       size_t* nrefused) {
    snprintf(g_ctx, sizeof g_ctx, "nkeys %llu stop %u pb %u nodes %d cus %llu forced %d", (unsigned long long)nkeys, stop,
             pb, (int)nodes, (unsigned long long)cus, forced);
    const uint32_t span = stop - pb;
    const TreeShape sh = pick_shape(span, nkeys, nodes, pb, cus, forced);
    // depth and workgroup
    CHECK(sh.d <= std::min(span, kMaxD));
    if (forced >= 0) CHECK(sh.d == std::min<uint32_t>((uint32_t)forced, std::min(span, kMaxD)));
    const uint32_t maxb = !nodes && sh.d >= kBigMinD ? kTreeBlockBig : kTreeBlock;
    CHECK(pow2(sh.block) && sh.block >= 64 && sh.block <= maxb);
    const u128 threads = (u128)nkeys << (span - sh.d);
    CHECK(sh.block == 64 || threads > (u128)cus * sh.block / 2);
    CHECK(sh.block == maxb || threads <= (u128)cus * sh.block);
    // refusal: exactly the grids above 2^31 - 1
    const u128 grid = (threads + sh.block - 1) / sh.block;
    const uint64_t prefix = pb ? ((uint64_t)1 << pb) - 1 : 0;   // the last subtree
    const bool raw = !nodes && evalfull_raw_ok(nkeys, stop, pb, cus, TreeKnobs{forced});
    TreeForm f;
    const bool ok = tree_form(nkeys, stop, pb, prefix, nodes, raw, cus, forced, &f);
    CHECK(ok == (grid <= (u128)kMaxGrid));
    if (!ok) {
        ++*nrefused;
        CHECK(!raw);
        return;
    }
    ++*nok;
    CHECK(f.d == sh.d && f.block == sh.block && (1u << f.W) == f.block);
    CHECK(f.ltop == stop - f.d && f.ltop >= pb && f.units_log == f.ltop - pb);
    // the threads' output ranges tile each key's output exactly once
    const u128 per_thread = nodes ? (u128)1 << f.d : (u128)16 << f.d;
    const u128 per_key = nodes ? (u128)1 << span : (u128)16 << span;
    CHECK(((u128)1 << f.units_log) * per_thread == per_key);
    CHECK(f.nunits == nkeys << f.units_log && (u128)f.nunits == threads);
    CHECK(f.sub_base == prefix << f.units_log);
    CHECK(f.sub_base + (((uint64_t)1 << f.units_log) - 1) < ((u128)1 << f.ltop));   // the last subtree is in the tree
    CHECK(f.grid == (f.nunits + f.block - 1) / f.block && (u128)f.grid == grid);
    CHECK(f.nunits == 0 || (f.grid - 1) * f.block < f.nunits);
    // the forms
    CHECK(f.uniform == (f.units_log >= 6));
    CHECK(f.nodes == nodes && f.raw == raw);
    if (f.raw) CHECK(f.uniform && !f.nodes);
    if (!nodes && nkeys > 0) CHECK(f.raw == f.uniform);   // DPF_RAW_KEYS unset: raw wherever a wave owns one key
    CHECK(f.cw_lds == (f.uniform && f.units_log >= f.W));
    if (f.cw_lds) {
        CHECK(f.nunits % f.block == 0);   // no thread leaves before the shared walk's barrier
        CHECK(f.ltop <= kCwLdsLevels);
    }
    CHECK(f.walk == (!f.cw_lds || f.W < 7 ? kWalkNone : f.W == 7 ? kWalkLane : kWalkQuad));
    if (f.walk != kWalkNone) {
        CHECK(f.ltop + 6 >= f.W && f.l1 == f.ltop - f.W + 6 && f.l1 <= f.ltop);
        CHECK(f.ltop - f.l1 == f.W - 6);   // every thread walks the last W - 6 levels itself
    } else {
        CHECK(f.l1 == 0);
    }
    CHECK(f.feedback == (f.uniform && !nodes && f.d >= kFeedbackMinD && f.block == (uint32_t)kTreeBlockBig));
    CHECK(f.prio_small == (f.d <= 5));
}

static void tree_sweep() {
    const uint64_t cuss[] = {1, 2, 3, 4, 16, 32, 64, 80, 240, 256, 304};
    size_t nok = 0, nrefused = 0;
    for (uint64_t nkeys : nkeys_list(65536))
        for (uint32_t stop = 0; stop <= 56; ++stop)
            for (uint32_t pb = 0; pb <= std::min(stop, 24u); ++pb)
                for (int nodes = 0; nodes < 2; ++nodes)
                    for (uint64_t cus : cuss)
                        for (int forced = -1; forced <= 7; ++forced)
                            check_tree(nkeys, stop, pb, nodes != 0, cus, forced, &nok, &nrefused);
    CHECK(nok > 1000000 && nrefused > 1000);   // both sides of the refusal were met
    // DPF_RAW_KEYS=0: never raw; nothing else moves
    TreeKnobs off;
    off.raw_keys = false;
    CHECK(!evalfull_raw_ok(1, 17, 0, 256, off) && evalfull_raw_ok(1, 17, 0, 256, TreeKnobs{}));
    CHECK(!evalfull_raw_ok(0, 17, 0, 256, TreeKnobs{}) && !evalfull_raw_ok(1, 5, 6, 256, TreeKnobs{}));
    printf("tree sweep: %zu plans, %zu refused\n", nok, nrefused);
}

// ---- 2. every Eval plan of the sweep ----------------------------------------
static void eval_sweep() {
    const uint64_t cuss[] = {1, 4, 16, 64, 256, 304};
    const uint64_t ppks[] = {1, 2, 7, 31, 32, 33, 64, 96, 128, 255, 256, 257, 384, 512, 1000, 1024, 3000,
                             4096, 65536, 131072, 262144, 1u << 20};
    const uint32_t logNs[] = {7, 8, 9, 11, 12, 13, 16, 20, 21, 22, 24, 32, 40, 63, 64};
    size_t n = 0, persist = 0, staged = 0, refused = 0;
    for (uint64_t nkeys : nkeys_list(65536))
        for (uint64_t ppk : ppks)
            for (uint32_t logN : logNs)
                for (uint64_t cus : cuss)
                    for (int variant = 0; variant < 6; ++variant) {
                        snprintf(g_ctx, sizeof g_ctx, "eval nkeys %llu ppk %llu logN %u cus %llu variant %d",
                                 (unsigned long long)nkeys, (unsigned long long)ppk, logN, (unsigned long long)cus, variant);
                        const uint32_t stop = logN - 7;
                        const uint64_t nq = nkeys * ppk, need = eval_frontier_bytes(nkeys, stop, ppk);
                        TreeKnobs k;
                        bool a16 = true;
                        uint64_t fbytes = need;
                        if (variant == 1) a16 = false;
                        if (variant == 2) fbytes = need ? need - 1 : 0;   // one byte short: root walks
                        if (variant == 3) k.eval_persist = 0;
                        if (variant == 4) k.eval_uniform = false;
                        if (variant == 5) fbytes = 0;
                        EvalForm e;
                        if (!eval_form(nq, ppk, stop, logN, fbytes, a16, cus, k, &e)) {
                            ++refused;
                            continue;
                        }
                        ++n;
                        // the frontier level: the deepest L with two points per node on average,
                        // below the leaves, at most kMaxFrontierHbm; none below 4
                        const uint32_t L = eval_frontier_level(stop, ppk);
                        CHECK(L == 0 || L >= 4);
                        CHECK(L <= std::min(stop, kMaxFrontierHbm));
                        if (L > 0) {
                            CHECK(((uint64_t)2 << L) <= ppk);
                            CHECK(L == stop || L == kMaxFrontierHbm || ((uint64_t)2 << (L + 1)) > ppk);   // the deepest
                            CHECK(need >= (nkeys << L) * 17 && need % 256 == 0 && need < (nkeys << L) * 17 + 256);
                        } else {
                            CHECK(need == 0);
                            CHECK(stop < 4 || ppk < 32);
                        }
                        CHECK(e.L == (logN <= 63 && fbytes >= need && fbytes > 0 ? L : 0));
                        if (e.L > 0) {
                            CHECK(e.nodes.nodes && e.nodes.ltop + e.nodes.d == e.L && e.nodes.sub_base == 0);
                            CHECK(e.nodes.nunits == nkeys << e.nodes.units_log);
                        }
                        const bool can_persist = e.L > 0 && ppk % 128 == 0 && a16 && nq >= 2048 && k.eval_persist;
                        CHECK((e.kernel == kEvalPersist) == can_persist);
                        if (e.kernel == kEvalPersist) {
                            ++persist;
                            CHECK(e.block == 1024 && e.grid >= 1 && e.grid <= cus);
                            CHECK(e.grid == cus || e.grid * 1024 >= nq / 2);
                            CHECK(e.cw_staged == ((stop - e.L) * 8 + 4 <= 64));
                            staged += e.cw_staged;
                            CHECK(nq % 2 == 0);   // a pair's two points are one 16-byte load
                            CHECK(e.ragged == ((nq / 2) % (e.grid * 1024) != 0));
                        } else {
                            CHECK(e.kernel == kEvalPairUniform || e.kernel == kEvalPair);
                            CHECK((e.kernel == kEvalPairUniform) == (ppk % 128 == 0 && k.eval_uniform));
                            CHECK(pow2(e.block) && e.block >= 64 && e.block <= (uint32_t)kBlock);
                            const uint64_t thr = (nq + 1) / 2;
                            CHECK(e.block == 64 || thr > cus * e.block / 2);
                            CHECK(e.block == (uint32_t)kBlock || thr <= cus * e.block);
                            CHECK(e.grid == (thr + e.block - 1) / e.block && e.grid <= kMaxGrid);
                            CHECK(e.ragged == (thr % e.block != 0));
                            CHECK(!e.cw_staged);
                        }
                    }
    CHECK(n > 100000 && persist > 1000 && staged > 100 && staged < persist);
    // the pair kernel's grid: 2^39 queries on one CU are 2^38 threads in 2^29 workgroups of 512;
    // 2^41 queries would need 2^31 and are refused
    EvalForm e;
    snprintf(g_ctx, sizeof g_ctx, "eval grid limit");
    CHECK(eval_form((uint64_t)1 << 39, 1, 13, 20, 0, true, 1, TreeKnobs{}, &e) && e.grid == (uint64_t)1 << 29);
    CHECK(!eval_form((uint64_t)1 << 41, 1, 13, 20, 0, true, 1, TreeKnobs{}, &e));
    // the 64-word limit of the persistent kernel's key-record slots, at L = 7 (256 points per key):
    // logN 20 stages 6 * 8 + 4 = 52 words, 21 stages 60, 22 needs 68 and walks by scalar loads
    CHECK(eval_frontier_level(13, 256) == 7 && eval_frontier_level(13, 1024) == 9);
    CHECK(eval_cw_staged(13, 7) && eval_cw_staged(14, 7) && !eval_cw_staged(15, 7) && !eval_cw_staged(25, 8));
    printf("eval sweep: %zu plans (%zu persistent, %zu staged), %zu refused\n", n, persist, staged, refused);
}

// ---- 3. recorded plans on 256 CUs ---------------------------------------------
struct Rec {
    uint64_t nkeys;
    uint32_t stop, pb;
    bool nodes;
    int forced;
    uint32_t d, block;
    uint64_t nunits, grid;
    TreeWalk walk;
    bool uniform, feedback;
};
static void recorded() {
    const TreeWalk N = kWalkNone, Ln = kWalkLane, Q = kWalkQuad;
    const Rec recs[] = {
        // the benchmark's shapes
        {4096, 13, 0, false, -1, 7, 1024, 262144, 256, N, true, true},     // configs[1]: 4096 keys, logN 20
        {1, 25, 0, false, -1, 7, 1024, 262144, 256, Q, true, true},        // configs[3]: 1 key, logN 32, one device
        {1, 25, 3, false, -1, 4, 512, 262144, 512, Q, true, false},        // ... an eighth of it per device
        {64, 17, 0, false, -1, 5, 512, 262144, 512, Q, true, false},       // configs[4]: PIR tree, 64 keys, logN 24
        {64, 17, 3, false, -1, 2, 512, 262144, 512, Q, true, false},       // ... an eighth of it per device
        // test_every_subtree_depth: EvalFull, 1 key, logN 24 (stop 17): one-key workgroups, CWs from LDS
        {1, 17, 0, false, 0, 0, 512, 131072, 256, Q, true, false},
        {1, 17, 0, false, 1, 1, 256, 65536, 256, Q, true, false},
        {1, 17, 0, false, 2, 2, 128, 32768, 256, Ln, true, false},
        {1, 17, 0, false, 3, 3, 64, 16384, 256, N, true, false},
        {1, 17, 0, false, 4, 4, 64, 8192, 128, N, true, false},
        {1, 17, 0, false, 5, 5, 64, 4096, 64, N, true, false},
        {1, 17, 0, false, 6, 6, 64, 2048, 32, N, true, false},
        {1, 17, 0, false, 7, 7, 64, 1024, 16, N, true, false},
        // ... EvalFull, 70 keys, logN 16 (stop 9)
        {70, 9, 0, false, 0, 0, 256, 35840, 140, Q, true, false},          // two workgroups per key
        {70, 9, 0, false, 1, 1, 128, 17920, 140, Ln, true, false},
        {70, 9, 0, false, 2, 2, 64, 8960, 140, N, true, false},            // wave-uniform keys, one wave per workgroup
        {70, 9, 0, false, 3, 3, 64, 4480, 70, N, true, false},
        {70, 9, 0, false, 4, 4, 64, 2240, 35, N, false, false},            // 32 .. 4 threads per key: per-lane keys
        {70, 9, 0, false, 5, 5, 64, 1120, 18, N, false, false},
        {70, 9, 0, false, 6, 6, 64, 560, 9, N, false, false},
        {70, 9, 0, false, 7, 7, 64, 280, 5, N, false, false},
        // ... Eval, 70 keys x 256 points, logN 16: node pass to level 7, 128 .. 1 threads per key
        {70, 7, 0, true, 0, 0, 64, 8960, 140, N, true, false},
        {70, 7, 0, true, 1, 1, 64, 4480, 70, N, true, false},
        {70, 7, 0, true, 2, 2, 64, 2240, 35, N, false, false},
        {70, 7, 0, true, 3, 3, 64, 1120, 18, N, false, false},
        {70, 7, 0, true, 4, 4, 64, 560, 9, N, false, false},
        {70, 7, 0, true, 5, 5, 64, 280, 5, N, false, false},
        {70, 7, 0, true, 6, 6, 64, 140, 3, N, false, false},
        {70, 7, 0, true, 7, 7, 64, 70, 2, N, false, false},
    };
    for (const Rec& r : recs) {
        snprintf(g_ctx, sizeof g_ctx, "recorded nkeys %llu stop %u pb %u nodes %d forced %d", (unsigned long long)r.nkeys,
                 r.stop, r.pb, (int)r.nodes, r.forced);
        TreeForm f;
        CHECK(tree_form(r.nkeys, r.stop, r.pb, 0, r.nodes, false, 256, r.forced, &f));
        if (f.d != r.d || f.block != r.block || f.nunits != r.nunits || f.grid != r.grid || f.walk != r.walk ||
            f.uniform != r.uniform || f.feedback != r.feedback)
            fprintf(stderr, "got d %u block %u nunits %llu grid %llu walk %d uniform %d feedback %d\n", f.d, f.block,
                    (unsigned long long)f.nunits, (unsigned long long)f.grid, (int)f.walk, (int)f.uniform, (int)f.feedback);
        CHECK(f.d == r.d && f.block == r.block && f.nunits == r.nunits && f.grid == r.grid);
        CHECK(f.walk == r.walk && f.uniform == r.uniform && f.feedback == r.feedback);
    }
    // raw key bytes are read where stop - D >= 6: all of the 1-key case, D <= 3 of the 70-key case
    for (int d = 0; d <= 7; ++d) {
        TreeKnobs k;
        k.forced_depth = d;
        CHECK(evalfull_raw_ok(1, 17, 0, 256, k));
        CHECK(evalfull_raw_ok(70, 9, 0, 256, k) == (d <= 3));
    }
    // the persistent Eval kernel of that test: 70 * 256 queries, L = 7, 9 workgroups
    EvalForm e;
    CHECK(eval_form(70 * 256, 256, 9, 16, eval_frontier_bytes(70, 9, 256), true, 256, TreeKnobs{}, &e));
    CHECK(e.L == 7 && e.kernel == kEvalPersist && e.grid == 9 && e.cw_staged && e.ragged);
    printf("recorded plans ok\n");
}

// ---- 4. the forms the GPU matrix reaches ---------------------------------------
// Universe (the same in tests/test_gpu_tree_forms.py): cus in {256, 64, 16, 4};
// nkeys the list above up to 4100; prefix_bits 0..12;
//   leaf launches: logN 7..32 (stop 0..25), prefix_bits <= stop;
//   node launches: to level `depth` in 3..22 with depth - prefix_bits >= 3.
//     depth 4..16 at prefix 0 is the batched-Eval frontier of 2^(depth+1)
//     points per key (cost: its queries, one result byte each); the others
//     are the byte-sliced back end's frontier pass at stop = depth + 3 (cost:
//     the leaves it feeds, 16 << (depth + 3 - prefix_bits) bytes per key).
// Form: what k_evalfull branches on; for leaf launches also whether the
// prefix is non-zero.  A node launch with a prefix runs the code of the same
// form without one (the prefix only moves sub_base), and only the
// byte-sliced route has one, at 128 bytes of leaves per node: a node form
// ("node") counts whatever the prefix, and the node forms of launches with a
// prefix are listed again ("nodepfx"): the GPU matrix runs all of them too,
// under a cap of their own (40 MiB).
typedef std::tuple<int, uint32_t, uint32_t, int, int, int, int, int, int> FormKey;   // nodes d block uniform raw cw_lds walk feedback prefixed
struct Rep {
    uint64_t cost, nkeys;
    uint32_t stop, pb, cus;
};
static void forms() {
    std::map<FormKey, Rep> best[3];
    std::map<FormKey, bool> at256[3];
    const char* kinds[3] = {"leaf", "node", "nodepfx"};
    const uint32_t cuss[] = {256, 64, 16, 4};
    for (int ci = 0; ci < 4; ++ci)
        for (uint64_t nkeys : nkeys_list(4100))
            for (uint32_t pb = 0; pb <= 12; ++pb)
                for (int nodes = 0; nodes < 2; ++nodes)
                    for (uint32_t depth = nodes ? 3 : 0; depth <= (nodes ? 22u : 25u); ++depth) {
                        if (depth < pb || (nodes && depth - pb < 3)) continue;
                        const bool raw = !nodes && evalfull_raw_ok(nkeys, depth, pb, cuss[ci], TreeKnobs{});
                        TreeForm f;
                        if (!tree_form(nkeys, depth, pb, 0, nodes != 0, raw, cuss[ci], -1, &f)) continue;
                        uint64_t cost;
                        if (!nodes) cost = nkeys * ((uint64_t)16 << (depth - pb));
                        else if (pb == 0 && depth >= 4 && depth <= 16) cost = nkeys * ((uint64_t)2 << depth);
                        else cost = nkeys * ((uint64_t)16 << (depth + 3 - pb));
                        // leaf launches: with and without a prefix; node launches: the form, whatever
                        // the prefix, and again those that have one
                        for (int kind = nodes; kind <= (nodes && pb != 0 ? 2 : nodes); ++kind) {
                            const FormKey key{nodes, f.d, f.block, f.uniform, f.raw, f.cw_lds, (int)f.walk, f.feedback,
                                              kind == 1 ? 0 : pb != 0};
                            if (ci == 0) at256[kind][key] = true;
                            auto it = best[kind].find(key);
                            if (it == best[kind].end() || cost < it->second.cost)
                                best[kind][key] = Rep{cost, nkeys, depth, pb, cuss[ci]};
                        }
                    }
    for (int nodes = 0; nodes < 3; ++nodes) {
        printf("FORMS %s total %zu at256 %zu\n", kinds[nodes], best[nodes].size(), at256[nodes].size());
        for (const auto& kv : best[nodes]) {
            const FormKey& k = kv.first;
            const Rep& r = kv.second;
            printf("FORM %s d %u block %u uniform %d raw %d cw_lds %d walk %d feedback %d prefixed %d rep nkeys %llu "
                   "depth %u pb %u cus %u cost %llu\n",
                   kinds[nodes], std::get<1>(k), std::get<2>(k), std::get<3>(k), std::get<4>(k), std::get<5>(k),
                   std::get<6>(k), std::get<7>(k), std::get<8>(k), (unsigned long long)r.nkeys, r.stop, r.pb, r.cus,
                   (unsigned long long)r.cost);
        }
    }
}

int main(int argc, char** argv) {
    if (argc > 1 && strcmp(argv[1], "forms") == 0) {
        forms();
        return 0;
    }
    tree_sweep();
    eval_sweep();
    recorded();
    printf("tree_plan ok\n");
    return 0;
}
