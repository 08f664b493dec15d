// subkeys.hip — k_subkeys: the device form of oracle.reroot_key for runs of
// consecutive prefixes.  A node (s, t) of the GGM tree with the remaining
// correction words is a DPF key of the smaller domain; unit (key k, piece p)
// walks key k from its root down prefix_bits levels along first_prefix + p and
// writes that key, wire format, at d_sub[k * nprefix + p][sub_len].  The walk
// is the tree kernel's own (tree_ops.hpp key_root / key_cw / walk_step: t a
// byte tested != 0, the t correction bytes XORed in as bytes), so a malformed
// key re-roots as evalFullRecursive would walk it (dpf.go:213-241).
//
// One thread per unit, the units of a launch in (key, piece) order, a
// workgroup of four waves taking 256 units at a time in a grid-stride loop: the
// pieces of a key share their upper levels, and a unit redoes them -- at most
// prefix_bits dependent AES-MMO a unit, latency-bound, where a shared walk
// would need an exchange per level.  A workgroup fills the 64 KiB T-table of
// aes_ttable.hpp once for all its units (32 lane copies, every lookup
// conflict-free; a single-copy table would serialise a wave's lookups 32-fold
// on one bank per row), and the grid is capped at one workgroup for each CU
// the launch may use.  A unit's thread also copies its key's tail: aligned
// words in, a few in flight at a time, bytes out (a sub-key starts at any
// address).  A copy spread byte by byte over the workgroup, one dependent
// load after another, took 70 us at 64 keys x 32 pieces
// (profiles/pir_window/ab_bytewise_copy.jsonl; this form: ab.jsonl).  No scratch, no allocation, no memset, no
// synchronisation: asynchronous on the caller's stream, and capturable.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "aes_ttable.hpp"
#include "dpf_kernels.hpp"
#include "tree_ops.hpp"

namespace dpfk {

namespace {

constexpr uint32_t kSubBlock = 256;

// n bytes from byte `so` of the batch (counted from the aligned base kw) to
// o: whole words through the funnel, each load inside a word that holds one
// of the bytes wanted, then the last n % 4 bytes one by one.
__device__ __forceinline__ void copy_bytes(const uint32_t* __restrict__ kw, uint64_t so, uint64_t n, uint8_t* __restrict__ o) {
    const uint32_t* p = kw + (so >> 2);
    const uint32_t sh = (uint32_t)(so & 3) * 8;
    const uint64_t words = n / 4;
#pragma unroll 8
    for (uint64_t i = 0; i < words; ++i) {
        const uint32_t v = sh ? funnel(p[i], p[i + 1], sh) : p[i];
        o[4 * i] = (uint8_t)v;
        o[4 * i + 1] = (uint8_t)(v >> 8);
        o[4 * i + 2] = (uint8_t)(v >> 16);
        o[4 * i + 3] = (uint8_t)(v >> 24);
    }
    const uint8_t* b = reinterpret_cast<const uint8_t*>(kw) + so;
    for (uint64_t j = 4 * words; j < n; ++j) o[j] = b[j];
}

// Sub-key bytes [17, sub_len - 16) are the key's from 17 + 18 * prefix_bits
// on, and its last 16 bytes are the key's last 16 (the final CW is always
// k[len-16:], dpf.go:206,219).  With sub_len = klen - 18 * prefix_bits the two
// runs meet: the tail is copied unchanged, a long key's trailing bytes with it.
__global__ __launch_bounds__(kSubBlock) void k_subkeys(const uint32_t* __restrict__ kw, uint64_t kboff, uint64_t klen,
                                                       uint64_t nunits, uint32_t prefix_bits, uint64_t first_prefix,
                                                       uint64_t nprefix, uint8_t* __restrict__ sub, uint64_t sub_len) {
    __shared__ __attribute__((aligned(16))) uint32_t s_tab[kTabWords];
    fill_table(s_tab);
    const uint8_t* tab = reinterpret_cast<const uint8_t*>(s_tab);
    const uint32_t lo = (threadIdx.x & 31u) * 4u;
    for (uint64_t u = (uint64_t)blockIdx.x * kSubBlock + threadIdx.x; u < nunits; u += (uint64_t)gridDim.x * kSubBlock) {
        const uint64_t k = u / nprefix, prefix = first_prefix + u % nprefix;
        const KeySrc ks{nullptr, kw, kboff + k * klen, klen};
        uint8_t* o = sub + u * sub_len;   // any alignment: byte stores
        copy_bytes(kw, ks.kb + 17 + 18ull * prefix_bits, sub_len - 33, o + 17);
        copy_bytes(kw, ks.kb + klen - 16, 16, o + sub_len - 16);
        Node n;
        n.s = key_root<true>(ks, n.t);
        for (uint32_t lvl = 0; lvl < prefix_bits; ++lvl)
            walk_step(tab, lo, n, key_cw<true>(ks, lvl), (uint32_t)(prefix >> (prefix_bits - 1 - lvl)) & 1u);
        const uint32_t c[4] = {n.s.c0, n.s.c1, n.s.c2, n.s.c3};
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = (uint8_t)(c[i >> 2] >> (8 * (i & 3)));
        o[16] = (uint8_t)n.t;
    }
}

}  // namespace

// Preconditions (the C ABI checks them): prefix_bits <= stop of the keys'
// domain, first_prefix + nprefix <= 2^prefix_bits, klen >= 17 + 18 * stop,
// 33 <= sub_len <= klen - 18 * prefix_bits + (what a canonical key adds: see
// window_canonical_sub_key_len), nkeys * nprefix units.
hipError_t launch_subkeys(const uint8_t* keys, uint64_t klen, uint64_t nkeys, uint32_t prefix_bits, uint64_t first_prefix,
                          uint64_t nprefix, uint8_t* sub, uint64_t sub_len, hipStream_t st) {
    const uint64_t nunits = nkeys * nprefix;
    if (nunits == 0) return hipSuccess;
    const uint64_t want = (nunits + kSubBlock - 1) / kSubBlock, cap = (uint64_t)std::max(cu_count(), 1);
    const uint64_t kboff = (uintptr_t)keys & 3;   // the 4-byte-aligned base below the batch (launch_evalfull_raw)
    hipLaunchKernelGGL(k_subkeys, dim3((uint32_t)(want < cap ? want : cap)), dim3(kSubBlock), 0, st,
                       reinterpret_cast<const uint32_t*>(keys - kboff), kboff, klen, nunits, prefix_bits, first_prefix, nprefix,
                       sub, sub_len);
    return hipGetLastError();
}

}  // namespace dpfk
