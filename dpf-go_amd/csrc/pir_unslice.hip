// pir_unslice.hip — the whole-DB read-out of a resident PIR DB: the inverse of
// k_slice_db (k_unslice_db: bit-sliced layout -> row-major records) and the
// merge of two sliced buffers of one shape (k_xor_words).  Grid chunking:
// dpfh::slice_db_span (pir_fold_plan.hpp), as for the forward kernel.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>

#include "dpf_kernels.hpp"
#include "pir_kernels.hpp"

namespace dpfk {

// Row-major records from the sliced layout dbs[S][p][g] (pir_fold_sliced.hip):
// the inverse of k_slice_db.  A workgroup takes one super-group S and a group
// of CG consecutive 32-byte columns from c0 on: nt = min(8 CG, ntiles - 8 c0)
// bit tiles, nt KiB contiguous.  Its 4 waves take 64 records each.  For tile wi
// lane l holds the word dbs[S][8 c0 + wi][n = l & 31][g = 2 wq + (l >> 5)],
// whose bit j is bit n of word 8 c0 + wi of record 256 S + 32 g + j: each
// 32-lane half holds a 32 x 32 bit matrix, and its transpose gives lane l that
// word of record 64 wq + l.  The transposition is five block-swap steps
// (transpose32: one exchange with lane n ^ d and one masked merge each, ~30
// VALU and 5 cross-lane moves per tile).  The mirror image of k_slice_db, 32
// ballots and 64 selects per tile, was the first form and was VALU-bound at the
// forward kernel's own rate (0.68 ms against 0.19 at 2^24 x 32 B).
//
// Loads: the tiles are read as the fold, update and scatter kernels read them:
// thread t takes uint4 t, t + 256, ..., a wave 1 KiB contiguous per
// instruction, all of them issued before the first is used.  The words go
// through LDS to the lanes that transpose them.  A lane reads one word per
// tile, (n, g) -> word 8 n + g of the tile: left as it is, a 32-lane half
// would hit 4 banks 8 ways (ds_read_b32 banks are words mod 32).  So uint4 slot
// s = 2 n + h of a tile is stored at slot s ^ ((n >> 2) & 1) with its
// components rotated up by n >> 3: the 32 lanes of a half, g fixed, then read
// 8 slots x 4 components = 32 different banks.  (The other load form, each lane
// fetching its word from HBM by a 4-byte load at a stride of 32 bytes, measured
// 0.32 against 0.19 ms at 2^24 x 32 B and 0.16 against 0.11 at 2^24 x 16 B:
// deleted.)
//
// Stores: a lane holds the nt words of its record.  One column (CG = 1, records
// up to 32 bytes): it writes them itself, 16-byte stores where rows are
// multiples of 16 bytes (a wave: 2 KiB contiguous for 32-byte records), word
// stores otherwise (rows then are only 4-byte aligned).  Wider records: with a
// store per lane every instruction would touch 64 rows, 16 bytes in each (256-
// byte records: 1.14 ms for 2^22; with 4 columns per workgroup and the same
// stores 0.81).  So the wave's 64 rows of nt / 4 uint4 go back through its
// quarter of the LDS and consecutive lanes store consecutive 16 bytes of a
// row, whole 128-byte lines with 4 columns (0.62 ms).  Rows that are not
// multiples of 16 bytes take the same way word by word.  Rows >= nrec of the
// last super-group are not written, so the output is exactly nrec rows and the
// pad bits of the input never reach one.  No scratch, no atomics.
// Measurements: profiles/pir_export.
__device__ __forceinline__ uint32_t pick4(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t i) {
    return i == 0 ? a0 : i == 1 ? a1 : i == 2 ? a2 : a3;
}

// The 32 x 32 bit matrix held by a 32-lane half of the wave (lane n: row n,
// bit j: column j) transposed in place: five block-swap steps, each one
// exchange with lane n ^ d and one masked merge.
__device__ __forceinline__ uint32_t transpose32(uint32_t x, uint32_t l) {
    constexpr uint32_t kLow[5] = {0x0000FFFFu, 0x00FF00FFu, 0x0F0F0F0Fu, 0x33333333u, 0x55555555u};
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const int d = 16 >> s;
        const uint32_t y = (uint32_t)__shfl_xor((int)x, d);
        const bool hi = (l & (uint32_t)d) != 0;                          // the lower row of its pair of blocks
        const uint32_t keep = hi ? ~kLow[s] : kLow[s];
        x = (x & keep) | ((hi ? y >> d : y << d) & ~keep);
    }
    return x;
}

constexpr int kUnsliceCols = 4;   // columns of a wide record per workgroup: 128 contiguous bytes of every row
// (LDS: 8 KiB a column.  Two-column records get their own instantiation: 16 KiB, twice the workgroups per CU.)
template <int CG>
__global__ __launch_bounds__(256) void k_unslice_db(const uint4* __restrict__ dbs, uint64_t nrec, uint32_t ncols,
                                                     uint32_t ntiles, uint32_t* __restrict__ db) {
    __shared__ uint4 tiles[CG * 512];                                   // the column group: up to 8 CG tiles of 64 uint4
    const uint32_t ncg = (ncols + CG - 1) / CG;
    const uint64_t S = blockIdx.x / ncg;
    const uint32_t c0 = (blockIdx.x % ncg) * CG;
    const uint32_t t = threadIdx.x, l = t & 63, wq = t >> 6;
    const uint32_t nt = ntiles - 8 * c0 < 8 * CG ? ntiles - 8 * c0 : 8 * CG;   // the group's tiles (uniform)
    const uint4* src = dbs + (S * ntiles + 8 * c0) * 64;
    uint4 v[2 * CG];
#pragma unroll
    for (int i = 0; i < 2 * CG; ++i)
        if (256u * i + t < 64 * nt) v[i] = src[256u * i + t];
#pragma unroll
    for (int i = 0; i < 2 * CG; ++i) {
        const uint32_t q = 256u * i + t;
        if (q >= 64 * nt) break;                                        // the group's tiles end here
        const uint32_t s = q & 63, n = s >> 1, r = n >> 3;              // position p holds component (p - r) & 3
        tiles[(q & ~63u) + (s ^ ((n >> 2) & 1))] =
            make_uint4(pick4(v[i].x, v[i].w, v[i].z, v[i].y, r), pick4(v[i].y, v[i].x, v[i].w, v[i].z, r),
                       pick4(v[i].z, v[i].y, v[i].x, v[i].w, r), pick4(v[i].w, v[i].z, v[i].y, v[i].x, r));
    }
    __syncthreads();
    const uint32_t n = l & 31, g = 2 * wq + (l >> 5);
    const uint32_t* tw = reinterpret_cast<const uint32_t*>(tiles) +
                         ((2 * n + (g >> 2)) ^ ((n >> 2) & 1)) * 4 + (((g & 3) + (n >> 3)) & 3);
    uint32_t wd[8 * CG];
#pragma unroll
    for (int wi = 0; wi < 8 * CG; ++wi) wd[wi] = (uint32_t)wi < nt ? transpose32(tw[wi * 256], l) : 0u;
    const uint64_t rec0 = S * 256 + wq * 64;                            // the wave's first record
    if (CG > 1 && ntiles % 4 == 0) {
        // Rows of whole uint4 (and so is nt): the wave's 64 rows of npr uint4 back through its own quarter of
        // the LDS, so that consecutive lanes store consecutive 16 bytes of a row.  Row r keeps its uint4 k at
        // slot (k + r) % npr: a lane's writes and 8 lanes' reads both spread over the banks.
        const uint32_t npr = nt / 4;
        __syncthreads();                                                // every wave has read its words of the tiles
        uint4* o4 = tiles + wq * (64 * 2 * CG);
        const uint32_t lm = l % npr;
#pragma unroll
        for (int k = 0; k < 2 * CG; ++k) {
            if ((uint32_t)k >= npr) break;
            const uint32_t kk = k + lm >= npr ? k + lm - npr : k + lm;
            o4[l * npr + kk] = make_uint4(wd[4 * k], wd[4 * k + 1], wd[4 * k + 2], wd[4 * k + 3]);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 2 * CG; ++j) {
            if ((uint32_t)j >= npr) break;
            const uint32_t i = 64u * j + l, r = i / npr, k = i - r * npr, rm = r % npr;
            const uint32_t kk = k + rm >= npr ? k + rm - npr : k + rm;
            if (rec0 + r < nrec) reinterpret_cast<uint4*>(db + (rec0 + r) * ntiles + 8 * c0)[k] = o4[r * npr + kk];
        }
        return;
    }
    if (CG > 1) {
        // Rows that are only 4-byte aligned: the same word by word.  Row r keeps word w at (w + r) % nt.
        // i / nt for i < 2^11, nt <= 32 by one multiplication: (i * ceil(2^16 / nt)) >> 16 is exact there.
        __syncthreads();
        uint32_t* o1 = reinterpret_cast<uint32_t*>(tiles + wq * (64 * 2 * CG));
        const uint32_t magic = (65536u + nt - 1) / nt;
        const uint32_t lm = l - ((l * magic) >> 16) * nt;
#pragma unroll
        for (int w = 0; w < 8 * CG; ++w) {
            if ((uint32_t)w >= nt) break;
            o1[l * nt + (w + lm >= nt ? w + lm - nt : w + lm)] = wd[w];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8 * CG; ++j) {
            if ((uint32_t)j >= nt) break;
            const uint32_t i = 64u * j + l, r = (i * magic) >> 16, w = i - r * nt, rm = r - ((r * magic) >> 16) * nt;
            if (rec0 + r < nrec) db[(rec0 + r) * ntiles + 8 * c0 + w] = o1[r * nt + (w + rm >= nt ? w + rm - nt : w + rm)];
        }
        return;
    }
    const uint64_t rec = rec0 + l;
    if (rec >= nrec) return;
    uint32_t* row = db + rec * ntiles + 8 * c0;
    if (ntiles % 4 == 0) {                                              // rows of whole uint4, and so is nt
#pragma unroll
        for (int k = 0; k < 2 * CG; ++k)
            if (4u * k < nt)
                reinterpret_cast<uint4*>(row)[k] = make_uint4(wd[4 * k], wd[4 * k + 1], wd[4 * k + 2], wd[4 * k + 3]);
    } else {
#pragma unroll
        for (int wi = 0; wi < 8 * CG; ++wi)
            if ((uint32_t)wi < nt) row[wi] = wd[wi];
    }
}

// dst[i] ^= src[i] over n uint4, grid-stride: two sliced buffers of one shape
// merged in place (zero padding stays zero).
__global__ __launch_bounds__(256) void k_xor_words(uint4* __restrict__ dst, const uint4* __restrict__ src, uint64_t n) {
    const uint64_t step = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
        const uint4 a = dst[i], b = src[i];
        dst[i] = make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w);
    }
}

hipError_t launch_unslice_db(const uint8_t* dbs, uint64_t nrec, uint64_t rec_bytes, uint8_t* db, hipStream_t st) {
    if (!dpfh::rec_bytes_any_ok(rec_bytes)) return hipErrorInvalidValue;
    const uint64_t nsg = (nrec + 255) / 256, C = dpfh::rec_cols(rec_bytes);
    const uint64_t cg = C == 1 ? 1 : C == 2 ? 2 : kUnsliceCols, ncg = (C + cg - 1) / cg;
    const auto kernel = cg == 1 ? k_unslice_db<1> : cg == 2 ? k_unslice_db<2> : k_unslice_db<kUnsliceCols>;
    return dpfh::for_each_span(nsg, dpfh::slice_db_span(C), [&](uint64_t S0, uint64_t n) {
        hipLaunchKernelGGL(kernel, dim3((uint32_t)(n * ncg)), dim3(256), 0, st,
                           reinterpret_cast<const uint4*>(dbs + S0 * 256 * rec_bytes), nrec - S0 * 256, (uint32_t)C,
                           dpfh::rec_tiles(rec_bytes), reinterpret_cast<uint32_t*>(db + S0 * 256 * rec_bytes));
        return hipGetLastError();
    });
}

hipError_t launch_xor_words(uint8_t* dst, const uint8_t* src, uint64_t bytes, hipStream_t st) {
    if (bytes % 16 != 0) return hipErrorInvalidValue;
    const uint64_t n = bytes / 16;
    if (n == 0) return hipSuccess;
    const uint64_t blocks = std::min<uint64_t>((n + 255) / 256, kXorWordsMaxBlocks);
    hipLaunchKernelGGL(k_xor_words, dim3((uint32_t)blocks), dim3(256), 0, st, reinterpret_cast<uint4*>(dst),
                       reinterpret_cast<const uint4*>(src), n);
    return hipGetLastError();
}

}  // namespace dpfk
