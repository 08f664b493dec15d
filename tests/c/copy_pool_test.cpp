// Stand-alone check of the copy pool of the host-buffer paths
// (dpf-go_amd/csrc/copy_pool.hpp): several caller threads share the pool's
// workers at once, as concurrent dpf_evalfull_batch / dpf_eval_batch calls on
// different devices do.  Built with -fsanitize=address,undefined and again
// with -fsanitize=thread, and run directly by tests/test_stage_host_cpu.py.
// No device, no library.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <thread>
#include <vector>

#include "copy_pool.hpp"

using dpfh::CopyPool;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                                    \
        }                                                               \
    } while (0)

static const size_t MiB = (size_t)1 << 20;
// One byte, exactly one piece, one piece and a byte, several pieces and a ragged end.
static const size_t kSizes[] = {1, 2 * MiB, 2 * MiB + 1, 9 * MiB + 3};

static void caller(unsigned id) {
    const size_t cap = 9 * MiB + 3;
    std::vector<uint8_t> src(cap), dst(cap);
    uint64_t s = 88172645463325252ull + id;
    for (size_t i = 0; i < cap; ++i) {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;   // xorshift64
        src[i] = (uint8_t)s;
    }
    for (int round = 0; round < 20; ++round)
        for (size_t n : kSizes) {
            memset(dst.data(), 0xA5, n);
            if (n < cap) dst[n] = 0x5C;                                          // the byte after the copy stays
            CopyPool::get().memcpy_par(dst.data(), src.data() + (cap - n), n);   // odd source offsets too
            CHECK(memcmp(dst.data(), src.data() + (cap - n), n) == 0);
            CHECK(n == cap || dst[n] == 0x5C);
        }
    // First touch: one zero per 4 KiB page, nothing else written.
    std::vector<uint8_t> fresh(5 * MiB + 4097, 0xFF);
    CopyPool::get().prefault_par(fresh.data(), fresh.size());
    for (size_t o = 0; o < fresh.size(); ++o) CHECK(fresh[o] == (o % 4096 == 0 ? 0 : 0xFF));
    // Nothing to copy: no memcpy on the null pointers.
    CopyPool::get().memcpy_par(nullptr, nullptr, 0);
}

int main() {
    std::vector<std::thread> th;
    for (unsigned i = 0; i < 4; ++i) th.emplace_back(caller, i);
    for (auto& t : th) t.join();
    printf("copy_pool ok\n");
    return 0;
}
