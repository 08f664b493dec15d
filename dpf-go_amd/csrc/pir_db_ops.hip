// pir_db_ops.hip — a resident PIR DB changed in place: records updated and
// read back (k_update_sliced, k_gather_sliced; k_scatter_rows, k_gather_rows
// on a row-major DB) and the private write, the fold's dual (k_scatter_sliced,
// k_xor_scatter_rows).  Grid chunking: pir_fold_plan.hpp; the private write's
// plan: pir_scatter_plan.hpp.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>

#include "dpf_kernels.hpp"
#include "fold_ops.hpp"
#include "pir_kernels.hpp"
#include "pir_scatter_plan.hpp"

namespace dpfk {

// ---- records of a resident DB changed and read back in place --------------
// A record's 256 C bits lie in 256 C different words of the sliced layout, one
// bit in each, so an update is a read-modify-write of whole tiles: tile
// (S, c) = dbs[S][c][0..255][0..7], 8 KiB contiguous.  Owner form, no atomics:
// the updates come sorted by record index, so those of one super-group are a
// contiguous run idx[h .. e), and the workgroup of the run's head h rewrites
// tile (S, c) alone.  Thread n of its 256 loads its row dbs[S][c][n][0..7]
// (two uint4, the access pattern of k_fold_sliced_direct), walks the run --
// for update i it replaces bit j = idx & 31 of word g = (idx & 255) >> 5 with
// bit n of column c of recs[i] (g, j wave-uniform; bit n of a column is bit
// n & 31 of its little-endian word n >> 5, so a wave needs two words per
// update) -- and stores the row back.  Later updates overwrite earlier ones
// in the registers: of equal indices the last wins.
//
// Grid: workgroup b = (slot, column c) = (b / C, b % C) takes a chunk of K
// consecutive updates.  For K > 1, slot -> chunk deals each eighth of the
// chunks to one residue of slot % 8: workgroups go round-robin over the 8
// XCDs, and the heads of a dense run come at a fixed stride (every 256 / K
// chunks), a multiple of 8 for 32-byte records, so chunk = slot would run
// every tile of such a run on one XCD.  Lane l < K tests update i = i0 + l for being a head (i == 0 or
// idx[i-1] >> 8 != idx[i] >> 8, and idx[i] < nrec: entries past nrec are
// skipped, so the padding of the last super-group stays zero) and the
// workgroup takes the chunk's heads one after the other; a run may extend
// past the chunk, it belongs to its head.  K = 1 is one workgroup per (update,
// column), which exits unless the update is a head; the launcher raises K
// with the least possible mean run length n / ceil(nrec / 256), so that dense
// updates do not launch 255 idle workgroups per tile.  The run is walked 64
// entries at a time: lane l of every wave loads idx[i + l] (a ballot finds
// the run's end) and its wave's two words of recs[i + l], and the walk takes
// (g, j) and the two words of each update by v_readlane, so a run costs one
// round of loads per 64 updates, not one per update.  Where the entries of
// such a batch are consecutive records (a dense run), 64 ballots transpose
// the batch as k_slice_db does -- thread n gets the 64 new bits of its bit
// position at once -- and two shifts per word deposit them: ~5 VALU per
// update instead of ~27.  With unsorted input two workgroups may rewrite one
// tile (content unspecified), but S comes from an idx < nrec and record loads
// from i < n: no access leaves the buffers.  Sparse updates are bound by the
// three dependent round trips of a tile (index, tile and record loads), so
// the kernel is held to 8 waves per SIMD (measurements: profiles/pir_update).
//
// Records of any width (ntiles = rec_bytes / 4 words): a super-group is
// 32 ntiles rows, thread t of column c has a row only if 256 c + t is below
// that, and a wave's two record words are read as one uint2 only where the
// record is an even number of words (then rows of recs are 8-byte aligned and
// word 8 c + 2 w + 1 exists whenever 8 c + 2 w does).  Threads without a row
// still take part in the ballots; they load and store nothing.
constexpr uint32_t kUpdSeqMin = 16;   // consecutive updates of a batch from which the ballot form is cheaper
__global__ __launch_bounds__(256, 8) void k_update_sliced(uint4* __restrict__ dbs, uint64_t nrec, uint32_t ncols,
                                                        uint32_t ntiles, const uint64_t* __restrict__ idx,
                                                        const uint32_t* __restrict__ recs, uint64_t n, uint64_t i_base,
                                                        uint32_t K, uint32_t nchunks) {
    const uint32_t c = blockIdx.x % ncols;
    const uint32_t slot = blockIdx.x / ncols, per8 = (nchunks + 7) / 8;
    const uint32_t chunk = K > 1 ? (slot % 8) * per8 + slot / 8 : slot;
    if (chunk >= nchunks) return;
    const uint64_t i0 = i_base + (uint64_t)chunk * K;
    const uint32_t t = threadIdx.x, l = t & 63;
    uint64_t heads;
    {
        const uint64_t i = i0 + l;
        bool head = false;
        if (l < K && i < n) {
            const uint64_t v = idx[i];
            head = v < nrec && (i == 0 || (idx[i - 1] >> 8) != (v >> 8));
        }
        heads = __builtin_amdgcn_ballot_w64(head);
    }
    const uint32_t w = t >> 6;                  // bit positions 64 w .. 64 w + 63: words 2 w, 2 w + 1 of the column
    const uint32_t w0i = 8 * c + 2 * w;          // this wave's first word of a record
    const uint32_t nwv = w0i >= ntiles ? 0u : ntiles - w0i < 2 ? 1u : 2u;
    const bool pair = (ntiles & 1) == 0;
    const bool live = 256u * c + t < 32u * ntiles;
    while (heads) {
        const uint32_t u = (uint32_t)__builtin_ctzll(heads);
        heads &= heads - 1;
        uint64_t i = i0 + u;
        const uint64_t S = idx[i] >> 8;
        uint4* row = &dbs[(S * 32 * ntiles + 256u * c + t) * 2];
        uint4 a = make_uint4(0, 0, 0, 0), b = a;
        if (live) a = row[0], b = row[1];
        uint32_t x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        for (;;) {
            // Entries i .. i + 63, one per lane: how many continue the run,
            // and this wave's two words of each of their records.
            const uint64_t il = i + l;
            uint64_t v = ~0ull;
            if (il < n) v = idx[il];
            const bool in = v < nrec && (v >> 8) == S;
            uint2 wv = make_uint2(0, 0);
            if (in && nwv) {
                const uint32_t* rw = recs + il * ntiles + w0i;
                if (pair) {
                    wv = *reinterpret_cast<const uint2*>(rw);
                } else {
                    wv.x = rw[0];
                    if (nwv > 1) wv.y = rw[1];
                }
            }
            const uint64_t m = __builtin_amdgcn_ballot_w64(in);
            const uint32_t cnt = ~m ? (uint32_t)__builtin_ctzll(~m) : 64u;
            const uint32_t lo = (uint32_t)v & 255u;
            const uint32_t off = (uint32_t)__builtin_amdgcn_readlane((int)lo, 0);
            // (entries of one run share S: consecutive records <=> consecutive low bytes)
            const bool seq = cnt >= kUpdSeqMin && __builtin_amdgcn_ballot_w64(l < cnt && lo != off + l) == 0;
            if (seq) {
                uint64_t M = 0;              // bit q: bit t of the column of update q's record
#pragma unroll
                for (uint32_t bb = 0; bb < 32; ++bb) {
                    const uint64_t m0 = __builtin_amdgcn_ballot_w64(((wv.x >> bb) & 1u) != 0);
                    const uint64_t m1 = __builtin_amdgcn_ballot_w64(((wv.y >> bb) & 1u) != 0);
                    M = l == bb ? m0 : M;
                    M = l == bb + 32 ? m1 : M;
                }
                const uint64_t V = cnt == 64 ? ~0ull : (1ull << cnt) - 1;       // updates of the batch
                // Update q is bit off + q of the row's 256: word gg takes bits [sh, sh + 32) of M.
                auto win = [](uint64_t mm, int sh) -> uint32_t {
                    return sh >= 64 || sh <= -32 ? 0u : sh >= 0 ? (uint32_t)(mm >> sh) : (uint32_t)mm << -sh;
                };
#pragma unroll
                for (int gg = 0; gg < 8; ++gg) {
                    const int sh = 32 * gg - (int)off;
                    const uint32_t mk = win(V, sh);                                    // scalar
                    x[gg] = (x[gg] & ~mk) | (win(M, sh) & mk);
                }
            }
            for (uint32_t q = 0; !seq && q < cnt; ++q) {
                const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)lo, (int)q);
                const uint32_t w0 = (uint32_t)__builtin_amdgcn_readlane((int)wv.x, (int)q);
                const uint32_t w1 = (uint32_t)__builtin_amdgcn_readlane((int)wv.y, (int)q);
                const uint32_t g = r >> 5, j = r & 31;
                const uint32_t nb = 0u - (((l < 32 ? w0 : w1) >> (l & 31)) & 1u);     // all ones / all zeros
#pragma unroll
                for (uint32_t gg = 0; gg < 8; ++gg) {
                    const uint32_t mk = g == gg ? 1u << j : 0u;                        // scalar
                    x[gg] = (x[gg] & ~mk) | (nb & mk);
                }
            }
            if (cnt < 64) break;
            i += 64;
        }
        if (live) {
            row[0] = make_uint4(x[0], x[1], x[2], x[3]);
            row[1] = make_uint4(x[4], x[5], x[6], x[7]);
        }
    }
}

// Record idx[i] of the sliced DB in row-major form (zeros for idx[i] >= nrec):
// one thread per output word (i, wd) of the record's ntiles words (any width:
// one word per bit tile), bit b of it = bit j of row 32 wd + b, group g of
// super-group S.  Not a hot path: 32 loads of 4 bytes per word.
__global__ __launch_bounds__(256) void k_gather_sliced(const uint32_t* __restrict__ dbs, uint64_t nrec, uint32_t ntiles,
                                                        const uint64_t* __restrict__ idx, uint64_t nwords,
                                                        uint32_t* __restrict__ out) {
    const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (tid >= nwords) return;
    const uint32_t wd = (uint32_t)(tid % ntiles);
    const uint64_t r = idx[tid / ntiles];
    uint32_t o = 0;
    if (r < nrec) {
        const uint64_t S = r >> 8;
        const uint32_t g = ((uint32_t)r & 255u) >> 5, j = (uint32_t)r & 31u;
        const uint32_t* p = dbs + ((S * ntiles + wd) * 32) * 8 + g;
#pragma unroll 8
        for (uint32_t b = 0; b < 32; ++b) o |= ((p[8 * b] >> j) & 1u) << b;
    }
    out[tid] = o;
}

// The same two operations on a row-major DB [nrec][rec_bytes] (a handle kept
// row-major): one thread per 16 bytes.  The scatter takes sorted indices and
// writes only the last update of equal ones; indices >= nrec are skipped
// (gather: read as zeros).
__global__ __launch_bounds__(256) void k_scatter_rows(uint4* __restrict__ db, uint64_t nrec, uint32_t q16,
                                                       const uint64_t* __restrict__ idx, const uint4* __restrict__ recs,
                                                       uint64_t n, uint64_t npieces) {
    const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (tid >= npieces) return;
    const uint64_t i = tid / q16;
    const uint64_t r = idx[i];
    if (r >= nrec || (i + 1 < n && idx[i + 1] == r)) return;
    db[r * q16 + tid % q16] = recs[tid];
}

__global__ __launch_bounds__(256) void k_gather_rows(const uint4* __restrict__ db, uint64_t nrec, uint32_t q16,
                                                      const uint64_t* __restrict__ idx, uint64_t npieces,
                                                      uint4* __restrict__ out) {
    const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (tid >= npieces) return;
    const uint64_t r = idx[tid / q16];
    out[tid] = r < nrec ? db[r * q16 + tid % q16] : make_uint4(0, 0, 0, 0);
}

using dpfh::rec_bytes_ok;

hipError_t launch_update_sliced(uint8_t* dbs, uint64_t nrec, uint64_t rec_bytes, const uint64_t* idx,
                                const uint8_t* recs, uint64_t n, hipStream_t st) {
    if (!dpfh::rec_bytes_any_ok(rec_bytes)) return hipErrorInvalidValue;
    if (n == 0 || nrec == 0) return hipSuccess;
    const uint64_t C = dpfh::rec_cols(rec_bytes);
    const dpfh::UpdatePlan p = dpfh::plan_update_sliced(n, (nrec + 255) / 256, C);
    return dpfh::for_each_span(n, p.span, [&](uint64_t i0, uint64_t m) {
        hipLaunchKernelGGL(k_update_sliced, dim3((uint32_t)p.grid(m, C)), dim3(256), 0, st,
                           reinterpret_cast<uint4*>(dbs), nrec, (uint32_t)C, dpfh::rec_tiles(rec_bytes), idx,
                           reinterpret_cast<const uint32_t*>(recs), n, i0, p.K, (uint32_t)p.chunks(m));
        return hipGetLastError();
    });
}

// n records of per_rec threads each, in launches over whole records
// (dpfh::record_span): fn(first record, records, threads).
template <class F>
static hipError_t for_record_chunks(uint64_t n, uint64_t per_rec, F fn) {
    return dpfh::for_each_span(n, dpfh::record_span(per_rec), [&](uint64_t i0, uint64_t m) {
        fn(i0, m, m * per_rec);
        return hipGetLastError();
    });
}

hipError_t launch_gather_sliced(const uint8_t* dbs, uint64_t nrec, uint64_t rec_bytes, const uint64_t* idx, uint64_t n,
                                uint8_t* out, hipStream_t st) {
    if (!dpfh::rec_bytes_any_ok(rec_bytes)) return hipErrorInvalidValue;
    const uint64_t T = dpfh::rec_tiles(rec_bytes);
    return for_record_chunks(n, T, [&](uint64_t i0, uint64_t, uint64_t threads) {
        hipLaunchKernelGGL(k_gather_sliced, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, st,
                           reinterpret_cast<const uint32_t*>(dbs), nrec, (uint32_t)T, idx + i0, threads,
                           reinterpret_cast<uint32_t*>(out + i0 * rec_bytes));
    });
}

hipError_t launch_update_rows(uint8_t* db, uint64_t nrec, uint64_t rec_bytes, const uint64_t* idx, const uint8_t* recs,
                              uint64_t n, hipStream_t st) {
    if (!rec_bytes_ok(rec_bytes)) return hipErrorInvalidValue;
    const uint64_t q16 = rec_bytes / 16;
    return for_record_chunks(n, q16, [&](uint64_t i0, uint64_t, uint64_t threads) {
        // n - i0: the look-ahead idx[i + 1] of a chunk's last record reads the next chunk's first index.
        hipLaunchKernelGGL(k_scatter_rows, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, st,
                           reinterpret_cast<uint4*>(db), nrec, (uint32_t)q16, idx + i0,
                           reinterpret_cast<const uint4*>(recs + i0 * rec_bytes), n - i0, threads);
    });
}

hipError_t launch_gather_rows(const uint8_t* db, uint64_t nrec, uint64_t rec_bytes, const uint64_t* idx, uint64_t n,
                              uint8_t* out, hipStream_t st) {
    if (!rec_bytes_ok(rec_bytes)) return hipErrorInvalidValue;
    const uint64_t q16 = rec_bytes / 16;
    return for_record_chunks(n, q16, [&](uint64_t i0, uint64_t, uint64_t threads) {
        hipLaunchKernelGGL(k_gather_rows, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, st,
                           reinterpret_cast<const uint4*>(db), nrec, (uint32_t)q16, idx + i0, threads,
                           reinterpret_cast<uint4*>(out + i0 * rec_bytes));
    });
}

// ---- private writes: messages XORed into the records the bits select ------
// The dual of the fold: db[i] ^= XOR over keys k with bit i of bits[k] set of
// msgs[k].  In the sliced layout the 32 records of a word dbs[S][c][n][g] are
// the 32 selection bits of word 8 S + g of a key's row, so
//   dbs[S][c][n][g] ^= XOR over k with bit 256 c + n of msgs[k] set of bits[k][8 S + g]
// with no bit transposition anywhere: one v_bitop3 (acc ^ (mask & sel)) per
// (key, word), the mask a sign-extended message bit (one v_bfe_i32 per four
// words).
//
// k_scatter_sliced<CG>: a workgroup takes a run of super-groups [s0, s1) of a
// group of up to CG columns and one tile of kt <= 64 keys (the plan:
// pir_scatter_plan.hpp).  Tile (S, c) is 512 uint4; thread t owns uint4 t and
// t + 256 of it: words g = 4 h .. 4 h + 3 (h = t & 1) of bit positions
// n = t >> 1 and 128 + (t >> 1), so a wave's loads and stores are contiguous
// KiBs and a thread needs only half of a key's 8 selection words per
// super-group: one broadcast ds_read_b128 per key (two per key, with a thread
// per bit position, put the LDS pipe level with the VALU at one column).  Its
// message bits -- bit k of mb[ci][slot] = bit 256 (c0 + ci) + n of key k's
// message -- are read once per run, from the messages staged in LDS.  The
// selection words of kScatterSB super-groups at a time are staged in LDS by
// coalesced 16-byte loads (a key's 128 contiguous bytes by 8 lanes), masked
// there to the records below nrec: whatever the caller left in the bits past
// nrec, the padding of the last super-group stays zero.  Words past the end of
// a key's row (wpk) are not read.  The next tile's loads are issued before the
// current one's arithmetic.  Each tile is read once and written once by one
// workgroup: no atomics, no scratch.
//
// Records of any width (ntiles = rec_bytes / 4 words): a super-group is
// 64 ntiles uint4, a thread's uint4 (c0 + ci) 512 + t + 256 sl exists only
// below that (no load, no store, zero message bits otherwise), and the
// messages, whose rows are then only 4-byte aligned, are staged word by word.
// FULL: the record is whole columns (a multiple of 32 bytes); the row guards
// become the column test and the kernel is the one from before records of any
// width (with the guards in, 32- and 64-byte records measured 1.5-2.5 % slower).
constexpr int kScatterSB = 4;                        // super-groups per staging round
constexpr int kScatterKT = (int)dpfh::kScatterKeyTile;
static_assert(dpfh::kScatterMaxCols == 4, "k_scatter_sliced is instantiated for 1 .. 4 columns");

// The bits of selection word ww (records 32 ww ..) that are records below nrec.
__device__ __forceinline__ uint32_t scatter_live(uint64_t ww, uint64_t nrec) {
    const uint64_t r0 = ww * 32;
    return nrec >= r0 + 32 ? ~0u : nrec <= r0 ? 0u : (1u << (uint32_t)(nrec - r0)) - 1u;
}

// (Held to the waves per SIMD that each CG had before the row guards: 5, 4, 5, 4.)
template <int CG, bool FULL>
__global__ __launch_bounds__(256, CG == 2 || CG == 4 ? 4 : 5) void k_scatter_sliced(
                                                        const uint32_t* __restrict__ bits, uint64_t wpk,
                                                        uint4* __restrict__ dbs, uint64_t nrec, uint64_t nsg,
                                                        uint32_t ncols, const uint4* __restrict__ msgs, uint32_t ntiles,
                                                        uint32_t kt, uint64_t run, uint32_t ncg, uint64_t u0) {
    __shared__ uint4 sel[kScatterKT][kScatterSB][2];            // 8 KiB; first the messages [kt][2 CG]
    static_assert(sizeof(sel) >= (size_t)kScatterKT * 2 * CG * sizeof(uint4), "the staged messages fit");
    const uint32_t t = threadIdx.x, h = t & 1, n = t >> 1;
    const uint64_t u = u0 + blockIdx.x;
    const uint64_t r = u / ncg;
    const uint32_t c0 = (uint32_t)(u % ncg) * CG;
    const uint64_t s0 = r * run, s1 = s0 + run < nsg ? s0 + run : nsg;
    if (s0 >= s1) return;                                      // (uniform; the plan launches no such workgroup)

    // Message bits of this thread's two bit positions, per column.
    uint32_t mb[CG][2][2];                                     // [column][slot][key word]
    {
        uint4* mst = &sel[0][0][0];
        if (FULL) {
            for (uint32_t i = t; i < kt * 2 * CG; i += 256) {
                const uint32_t k = i / (2 * CG), q = 2 * c0 + i % (2 * CG);
                mst[i] = q < 2 * ncols ? msgs[(uint64_t)k * (ntiles / 4) + q] : make_uint4(0, 0, 0, 0);
            }
        } else {
            uint32_t* mw = reinterpret_cast<uint32_t*>(mst);
            const uint32_t* msgw = reinterpret_cast<const uint32_t*>(msgs);
            for (uint32_t i = t; i < kt * 8 * CG; i += 256) {
                const uint32_t k = i / (8 * CG), q = 8 * c0 + i % (8 * CG);
                mw[i] = q < ntiles ? msgw[(uint64_t)k * ntiles + q] : 0u;
            }
        }
        __syncthreads();
        const uint8_t* mbytes = reinterpret_cast<const uint8_t*>(mst);
#pragma unroll
        for (int ci = 0; ci < CG; ++ci)
#pragma unroll
            for (int sl = 0; sl < 2; ++sl) {
                const uint32_t nn = n + 128 * sl;
                uint32_t lo = 0, hi = 0;
                for (uint32_t k = 0; k < kt; ++k) {
                    const uint32_t b = (mbytes[k * 32 * CG + 32 * ci + (nn >> 3)] >> (nn & 7)) & 1u;
                    lo |= k < 32 ? b << k : 0u;
                    hi |= k >= 32 ? b << (k - 32) : 0u;
                }
                mb[ci][sl][0] = lo;
                mb[ci][sl][1] = hi;
            }
    }

    const uint32_t sg_u4 = 64 * ntiles;                        // uint4 per super-group
    auto tile = [&](uint64_t S, int ci) { return &dbs[S * sg_u4 + (c0 + ci) * 512 + t]; };
    const uint32_t left = sg_u4 > c0 * 512 + t ? sg_u4 - (c0 * 512 + t) : 0;   // uint4 from this thread's first to the end
    auto have = [&](int ci, int sl) { return FULL ? c0 + ci < ncols : (uint32_t)(ci * 512 + 256 * sl) < left; };
    auto load = [&](uint64_t S, uint4 (&x)[CG][2]) __attribute__((always_inline)) {
#pragma unroll
        for (int ci = 0; ci < CG; ++ci) {
            if (have(ci, 0)) x[ci][0] = tile(S, ci)[0];
            if (have(ci, 1)) x[ci][1] = tile(S, ci)[256];
        }
    };
    uint4 cur[CG][2] = {}, nxt[CG][2] = {};
    load(s0, cur);
    for (uint64_t S0 = s0; S0 < s1; S0 += kScatterSB) {
        __syncthreads();                                       // the previous round's (or the messages') reads are done
#pragma unroll
        for (uint32_t i = t; i < (uint32_t)kScatterKT * kScatterSB * 2; i += 256) {
            const uint32_t k = i / (2 * kScatterSB), s = (i / 2) % kScatterSB, hh = i & 1;
            const uint64_t ww = 8 * (S0 + s) + 4 * hh;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (k < kt && S0 + s < s1 && ww < wpk) {           // wpk is a multiple of 4: the whole uint4 is in the row
                v = *reinterpret_cast<const uint4*>(bits + (uint64_t)k * wpk + ww);
                v.x &= scatter_live(ww, nrec);
                v.y &= scatter_live(ww + 1, nrec);
                v.z &= scatter_live(ww + 2, nrec);
                v.w &= scatter_live(ww + 3, nrec);
            }
            sel[k][s][hh] = v;
        }
        __syncthreads();
        for (uint32_t s = 0; s < (uint32_t)kScatterSB && S0 + s < s1; ++s) {
            const uint64_t S = S0 + s;
            if (S + 1 < s1) load(S + 1, nxt);
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                if (kt <= 32u * w) break;
                const uint32_t kend = kt - 32u * w < 32u ? kt - 32u * w : 32u;
                for (uint32_t kk = 0; kk < kend; kk += 8) {    // keys past kt: zero message bits, zero words
#pragma unroll
                    for (uint32_t j = 0; j < 8; ++j) {
                        const uint4 sv = sel[32 * w + kk + j][s][h];
#pragma unroll
                        for (int ci = 0; ci < CG; ++ci)
#pragma unroll
                            for (int sl = 0; sl < 2; ++sl) {
                                const uint32_t m = (uint32_t)__builtin_amdgcn_sbfe((int)mb[ci][sl][w], kk + j, 1);
                                uint4& x = cur[ci][sl];
                                x = make_uint4(xam(x.x, m, sv.x), xam(x.y, m, sv.y), xam(x.z, m, sv.z), xam(x.w, m, sv.w));
                            }
                    }
                }
            }
#pragma unroll
            for (int ci = 0; ci < CG; ++ci) {
                if (have(ci, 0)) tile(S, ci)[0] = cur[ci][0];
                if (have(ci, 1)) tile(S, ci)[256] = cur[ci][1];
            }
#pragma unroll
            for (int ci = 0; ci < CG; ++ci) {
                cur[ci][0] = nxt[ci][0];
                cur[ci][1] = nxt[ci][1];
            }
        }
    }
}

// The same on a row-major DB [nrec][16 q16 bytes]: a thread per 16 bytes of a
// record.  Workgroup (x, y) takes pieces [16 y, 16 y + P) of rpb consecutive
// records (P = min(q16, 16) pieces per row of the workgroup, rpb = 256 / P),
// stages those pieces of the kt <= 64 messages in LDS and walks the keys,
// testing the record's bit.  Row-major handles and the plain device entry
// point; untuned.
__global__ __launch_bounds__(256) void k_xor_scatter_rows(const uint32_t* __restrict__ bits, uint64_t wpk,
                                                           uint4* __restrict__ db, uint64_t nrec, uint32_t q16,
                                                           const uint4* __restrict__ msgs, uint32_t kt, uint32_t P,
                                                           uint32_t rpb) {
    __shared__ uint4 m[kScatterKT][16];
    const uint32_t t = threadIdx.x, p0 = 16 * blockIdx.y;
    for (uint32_t i = t; i < kt * P; i += 256) {
        const uint32_t k = i / P, p = i % P;
        m[k][p] = p0 + p < q16 ? msgs[(uint64_t)k * q16 + p0 + p] : make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    const uint32_t pc = t % P, rl = t / P;
    const uint64_t rec = (uint64_t)blockIdx.x * rpb + rl;
    if (rl >= rpb || rec >= nrec || p0 + pc >= q16) return;
    uint4 acc = db[rec * q16 + p0 + pc];
    for (uint32_t k = 0; k < kt; ++k) {
        const uint32_t bit = (bits[(uint64_t)k * wpk + (rec >> 5)] >> (rec & 31)) & 1u;
        acc = x4am(acc, m[k][pc], 0u - bit);
    }
    db[rec * q16 + p0 + pc] = acc;
}

template <int CG>
static hipError_t scatter_sliced_cg(const dpfh::ScatterPlan& p, const uint32_t* bits, uint64_t wpk, uint8_t* dbs,
                                    uint64_t nrec, uint64_t rec_bytes, const uint8_t* msgs, hipStream_t st) {
    const auto kernel = rec_bytes % 32 == 0 ? k_scatter_sliced<CG, true> : k_scatter_sliced<CG, false>;
    for (uint64_t tile = 0; tile < p.key_tiles(); ++tile) {
        const dpfh::ScatterUnit k = p.unit(tile, 0);
        for (uint64_t l = 0; l < p.launches(); ++l) {
            hipLaunchKernelGGL(kernel, dim3((uint32_t)p.blocks(l)), dim3(256), 0, st, bits + k.k0 * wpk, wpk,
                               reinterpret_cast<uint4*>(dbs), nrec, p.nsg, p.C,
                               reinterpret_cast<const uint4*>(msgs + k.k0 * rec_bytes), dpfh::rec_tiles(rec_bytes),
                               (uint32_t)(k.k1 - k.k0), p.run, p.ncg, p.first(l));
            if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

hipError_t launch_scatter_sliced(const uint32_t* bits, uint64_t words_per_key, uint8_t* dbs, uint64_t nrec,
                                 uint64_t rec_bytes, const uint8_t* msgs, uint64_t nkeys, hipStream_t st) {
    if (!dpfh::rec_bytes_any_ok(rec_bytes) || words_per_key % 4 != 0 || nrec > words_per_key * 32)
        return hipErrorInvalidValue;
    if (nkeys == 0 || nrec == 0) return hipSuccess;
    const dpfh::FoldLimits lim = fold_limits();
    const dpfh::ScatterPlan p = dpfh::plan_scatter(nrec, dpfh::rec_cols(rec_bytes), nkeys, (uint32_t)cu_count(),
                                                   lim.max_blocks, lim.max_sg);
    switch (p.cols) {
        case 1: return scatter_sliced_cg<1>(p, bits, words_per_key, dbs, nrec, rec_bytes, msgs, st);
        case 2: return scatter_sliced_cg<2>(p, bits, words_per_key, dbs, nrec, rec_bytes, msgs, st);
        case 3: return scatter_sliced_cg<3>(p, bits, words_per_key, dbs, nrec, rec_bytes, msgs, st);
        default: return scatter_sliced_cg<4>(p, bits, words_per_key, dbs, nrec, rec_bytes, msgs, st);
    }
}

hipError_t launch_scatter_rows(const uint32_t* bits, uint64_t words_per_key, uint8_t* db, uint64_t nrec,
                               uint64_t rec_bytes, const uint8_t* msgs, uint64_t nkeys, hipStream_t st) {
    if (!rec_bytes_ok(rec_bytes) || words_per_key % 4 != 0 || nrec > words_per_key * 32) return hipErrorInvalidValue;
    if (nkeys == 0 || nrec == 0) return hipSuccess;
    const uint32_t q16 = (uint32_t)(rec_bytes / 16), P = q16 < 16 ? q16 : 16, rpb = 256 / P;
    const uint64_t per = (uint64_t)rpb << 30;                  // records per launch: <= 2^30 workgroups in x
    for (uint64_t k0 = 0; k0 < nkeys; k0 += dpfh::kScatterKeyTile) {
        const uint32_t kt = (uint32_t)std::min<uint64_t>(dpfh::kScatterKeyTile, nkeys - k0);
        for (uint64_t r0 = 0; r0 < nrec; r0 += per) {
            // (r0 is a multiple of 32: the launch's selection words start at word r0 / 32 of each row.)
            const uint64_t n = std::min(per, nrec - r0);
            hipLaunchKernelGGL(k_xor_scatter_rows, dim3((uint32_t)((n + rpb - 1) / rpb), (q16 + 15) / 16), dim3(256), 0,
                               st, bits + k0 * words_per_key + r0 / 32, words_per_key,
                               reinterpret_cast<uint4*>(db + r0 * rec_bytes), n, q16,
                               reinterpret_cast<const uint4*>(msgs + k0 * rec_bytes), kt, P, rpb);
            if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

}  // namespace dpfk
