// Stand-alone check of the chunk plans of the host-buffer entry points
// (dpf-go_amd/csrc/stage_plan.hpp): built with -fsanitize=address,undefined
// and run directly by tests/test_stage_host_cpu.py.  No device, no library.
// The pinned values are worked out by hand from the rules the plans state.
#include <stdio.h>
#include <stdlib.h>

#include "stage_plan.hpp"

using dpfh::EvalPlan;
using dpfh::FullChunk;
using dpfh::FullPlan;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                                    \
        }                                                               \
    } while (0)

static const size_t MiB = (size_t)1 << 20;

// The chunks of `p` cover [at, at + p.out_bytes) of the caller's buffer once,
// in increasing order, each within the capacity, the capacity within a stage.
// Returns the end of the covered range.
static size_t check_tiling(const FullPlan& p, size_t at) {
    CHECK(p.cap <= dpfh::kStageBytes && p.nchunks >= 1);
    CHECK(p.out_base == at);
    for (size_t i = 0; i < p.nchunks; ++i) {
        const FullChunk c = p.chunk(i);
        CHECK(c.off == at && c.bytes >= 1 && c.bytes <= p.cap);
        CHECK(c.n >= 1 && c.k0 + c.n <= p.nk);
        CHECK(c.bytes == c.n * (p.olen >> c.prefix_bits));          // n subtrees' worth of leaves
        CHECK(c.prefix_bits == p.prefix_bits() && (c.prefix >> c.prefix_bits) == 0);
        // where those leaves belong in the caller's buffer: key k0, subtree `prefix`
        CHECK(c.off == c.k0 * p.olen + c.prefix * (p.olen >> c.prefix_bits));
        bool listed = false;                                         // its launch shape is one the plan names
        for (size_t s = 0; s < p.nshapes; ++s)
            listed = listed || (p.shape[s].nkeys == c.n && p.shape[s].prefix_bits == c.prefix_bits);
        CHECK(listed);
        at += c.bytes;
    }
    CHECK(at == p.out_base + p.out_bytes);
    return at;
}

static void tiling_sweep() {
    const size_t nks[] = {1, 2, 7, 255, 256, 257, 300, 4096};
    const uint32_t logNs[] = {0, 3, 7, 12, 20, 25, 26, 27, 28, 29, 30, 32};
    const size_t ppks[] = {1, 37, 256, 1024, 1400001, 1500032, 5000000};
    size_t done = 0, skipped = 0;   // nothing is skipped: the check walks chunks, not bytes
    for (size_t nk : nks) {
        for (uint32_t logN : logNs) {
            const FullPlan p = dpfh::full_plan(nk, logN);
            CHECK(p.nk == nk && p.olen == dpfh::full_len(logN) && p.out_bytes == nk * p.olen);
            CHECK(check_tiling(p, 0) == nk * p.olen);
            ++done;
        }
        for (size_t ppk : ppks) {
            const EvalPlan e = dpfh::eval_plan(nk, ppk);
            CHECK(e.per >= 1 && e.qcap == e.per * ppk && e.qcap <= dpfh::kStageBytes);
            CHECK(e.per == 1 || e.qcap * 8 <= dpfh::kStageBytes);   // the points fit a stage, or one key alone
            size_t at = 0;
            for (size_t i = 0; i < e.nchunks; ++i) {
                CHECK(e.k0(i) == at && e.n(i) >= 1 && e.n(i) <= e.per);
                at += e.n(i);
            }
            CHECK(at == nk && e.nchunks >= 1);
            ++done;
        }
    }
    // dpf_evalfull_split: the devices' shares, in device order, tile the one key's output.
    for (uint32_t logN : logNs)
        for (int ngpus : {1, 2, 4, 8}) {
            uint32_t pb = 0;
            if (!dpfh::gpus_to_pb(ngpus, dpfh::stop_of(logN), &pb)) {
                CHECK(((size_t)ngpus >> dpfh::stop_of(logN)) > 1);   // only: more devices than subtrees
                continue;
            }
            size_t at = 0;
            for (size_t lo = 0; lo < (size_t)ngpus; ++lo) at = check_tiling(dpfh::split_plan(logN, pb, lo), at);
            CHECK(at == dpfh::full_len(logN));
            ++done;
        }
    printf("tiling: %zu plans checked, %zu skipped\n", done, skipped);
    CHECK(skipped == 0);
}

static void pinned_full() {
    {
        const FullPlan p = dpfh::full_plan(4096, 20);
        CHECK(p.prefix_bits() == 0 && p.per == 256 && p.nchunks == 16 && p.cap == 32 * MiB);
    }
    {
        const FullPlan p = dpfh::full_plan(300, 20);
        CHECK(p.prefix_bits() == 0 && p.per == 256 && p.nchunks == 2);
        const FullChunk c = p.chunk(1);
        CHECK(c.k0 == 256 && c.n == 44 && c.off == 33554432 && c.bytes == 5767168 && c.prefix_bits == 0);
        CHECK(p.nshapes == 2 && p.shape[0].nkeys == 256 && p.shape[0].prefix_bits == 0);
        CHECK(p.shape[1].nkeys == 44 && p.shape[1].prefix_bits == 0);
    }
    {
        const FullPlan p = dpfh::full_plan(100, 20);
        CHECK(p.prefix_bits() == 0 && p.per == 256 && p.nchunks == 1 && p.cap == 13107200);
        CHECK(p.nshapes == 1 && p.shape[0].nkeys == 100);
    }
    {
        const FullPlan p = dpfh::full_plan(5, 3);
        CHECK(p.prefix_bits() == 0 && p.nchunks == 1 && p.cap == 80);
    }
    {
        const FullPlan p = dpfh::full_plan(3, 25);   // 4 MiB a key: below kSlabMinOut, whole keys
        CHECK(p.prefix_bits() == 0 && p.per == 8 && p.nchunks == 1);
    }
    {
        // 8 MiB a key = kSlabMinOut: every key of the batch goes in 4 slabs of
        // 2 MiB, although 4 whole keys would fit one chunk.  ADVICE.md
        // questions this rule for multi-key batches (it was meant for a single
        // key's overlap); a fix changes this row to whole-key chunks.
        const FullPlan p = dpfh::full_plan(3, 26);
        CHECK(p.prefix_bits() == 2 && p.nchunks == 12 && p.cap == 2 * MiB);
        for (size_t i = 0; i < 12; ++i) {
            const FullChunk c = p.chunk(i);
            CHECK(c.k0 == i / 4 && c.n == 1 && c.prefix_bits == 2 && c.prefix == i % 4);
            CHECK(c.bytes == 2 * MiB && c.off == (i / 4) * 8 * MiB + (i % 4) * 2 * MiB);
        }
        CHECK(p.nshapes == 1 && p.shape[0].nkeys == 1 && p.shape[0].prefix_bits == 2);
    }
    {
        const FullPlan p = dpfh::full_plan(1, 28);
        CHECK(p.prefix_bits() == 2 && p.nchunks == 4 && p.cap == 8 * MiB);
    }
    {
        const FullPlan p = dpfh::full_plan(2, 29);
        CHECK(p.prefix_bits() == 2 && p.nchunks == 8 && p.cap == 16 * MiB);
    }
    {
        const FullPlan p = dpfh::full_plan(1, 30);
        CHECK(p.prefix_bits() == 2 && p.nchunks == 4 && p.cap == 32 * MiB);
    }
    {
        const FullPlan p = dpfh::full_plan(1, 32);
        CHECK(p.prefix_bits() == 4 && p.nchunks == 16 && p.cap == 32 * MiB);
    }
}

static void pinned_eval() {
    {
        const EvalPlan e = dpfh::eval_plan(16384, 1024);
        CHECK(e.per == 4096 && e.nchunks == 4 && e.qcap == 4194304);
    }
    {
        const EvalPlan e = dpfh::eval_plan(5, 1500032);
        CHECK(e.per == 2 && e.nchunks == 3 && e.qcap == 3000064);
        CHECK(e.n(0) == 2 && e.n(1) == 2 && e.n(2) == 1 && e.k0(2) == 4);
    }
    {
        const EvalPlan e = dpfh::eval_plan(3, 5000000);
        CHECK(e.per == 1 && e.nchunks == 3);
    }
    {
        const EvalPlan e = dpfh::eval_plan(8, 256);
        CHECK(e.per == 8 && e.nchunks == 1);
    }
}

static void pinned_split() {
    uint32_t pb = 99;
    {
        CHECK(dpfh::gpus_to_pb(8, dpfh::stop_of(32), &pb) && pb == 3);
        for (size_t lo = 0; lo < 8; ++lo) {
            const FullPlan p = dpfh::split_plan(32, pb, lo);
            CHECK(p.split_bits == 3 && p.out_bytes == 64 * MiB && p.slab_bits == 1 && p.cap == 32 * MiB);
            CHECK(p.nchunks == 2 && p.out_base == lo * 64 * MiB);
            for (size_t j = 0; j < 2; ++j) {
                const FullChunk c = p.chunk(j);
                CHECK(c.k0 == 0 && c.n == 1 && c.prefix_bits == 4 && c.prefix == 2 * lo + j);
                CHECK(c.bytes == 32 * MiB && c.off == lo * 64 * MiB + j * 32 * MiB);
            }
        }
    }
    {
        CHECK(dpfh::gpus_to_pb(1, dpfh::stop_of(32), &pb) && pb == 0);
        const FullPlan p = dpfh::split_plan(32, pb, 0);
        CHECK(p.split_bits == 0 && p.slab_bits == 4 && p.nchunks == 16 && p.cap == 32 * MiB);
    }
    {
        CHECK(dpfh::gpus_to_pb(1, dpfh::stop_of(18), &pb) && pb == 0);
        const FullPlan p = dpfh::split_plan(18, pb, 0);
        CHECK(p.nchunks == 1 && p.cap == 32 * 1024 && p.prefix_bits() == 0);
        const FullChunk c = p.chunk(0);
        CHECK(c.k0 == 0 && c.n == 1 && c.bytes == 32 * 1024 && c.off == 0);
    }
    {
        CHECK(dpfh::gpus_to_pb(8, dpfh::stop_of(10), &pb) && pb == 3);
        const FullPlan p = dpfh::split_plan(10, pb, 5);
        CHECK(p.split_bits == 3 && p.slab_bits == 0 && p.out_bytes == 16 && p.cap == 16 && p.nchunks == 1);
        const FullChunk c = p.chunk(0);
        CHECK(c.prefix_bits == 3 && c.prefix == 5 && c.off == 80 && c.bytes == 16);
    }
    // Rejected, *pb untouched: more devices than subtrees, no power of two, no device.
    pb = 99;
    CHECK(!dpfh::gpus_to_pb(16, dpfh::stop_of(10), &pb));
    CHECK(!dpfh::gpus_to_pb(3, dpfh::stop_of(20), &pb));
    CHECK(!dpfh::gpus_to_pb(0, dpfh::stop_of(20), &pb));
    CHECK(!dpfh::gpus_to_pb(-4, dpfh::stop_of(20), &pb));
    CHECK(pb == 99);
}

static void prefix_range() {
    CHECK(dpfh::prefix_ok(0, 0, 0) && !dpfh::prefix_ok(0, 1, 0) && !dpfh::prefix_ok(1, 0, 0));
    CHECK(dpfh::prefix_ok(2, 3, 5) && !dpfh::prefix_ok(2, 4, 5));
    CHECK(dpfh::prefix_ok(5, 31, 5) && !dpfh::prefix_ok(6, 0, 5));
    CHECK(dpfh::prefix_ok(56, (1ull << 56) - 1, 56) && !dpfh::prefix_ok(56, 1ull << 56, 56));
    CHECK(!dpfh::prefix_ok(2, ~0ull, 5));
}

int main() {
    tiling_sweep();
    pinned_full();
    pinned_eval();
    pinned_split();
    prefix_range();
    printf("stage_plan ok\n");
    return 0;
}
