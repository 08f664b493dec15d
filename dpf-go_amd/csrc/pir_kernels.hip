// pir_kernels.hip — XOR-fold of records selected by EvalFull bits on gfx950:
// the 2-server PIR answer (last row: a build-only operator with
// no reference counterpart) and its general-payload form.
//
//   ans_k = XOR over records i with bit_i(EvalFull(key_k)) = 1 of DB[i]
//
// Phase 1 (dpf_kernels.hip, subtree EvalFull) writes each key's selection
// bits into HBM: bits[k][i/32] bit (i%32), which is exactly EvalFull's packed
// LSB-first byte layout (dpf/dpf.go:248-261) read as little-endian u32.
// Phase 2 (here) reads every record once from HBM per launch and folds it
// into all of the launch's answers.  The fold is a GF(2) product and stays
// bitwise (VALU XOR + LDS table lookups); it is not reshaped into an int8
// MFMA GEMM (8x data expansion for the same HBM-bound stream).
//
// Work unit.  A "chunk" is 64 records (one 64-bit word pair of every key's
// selection bits); a record is C 32-byte columns (C = rec_bytes / 32).  A
// chunk is processed as C "sub-steps" of 2 KiB of contiguous DB bytes (64/C
// records x all C columns), loaded by one wave as two coalesced 1 KiB loads:
// lane l holds 16-byte pieces p = l and p = 64 + l.  Records of any other
// multiple of 32 B run as C = 1 over one 32-byte column at a time (rec_u4 /
// col below), one launch per column.
//
// Two kernels, chosen by batch size (launch_pir_fold):
//   k_fold_direct  B <= 16 keys: each lane XORs its pieces into per-key
//                  accumulators under the key's selection bit (selection
//                  words come through scalar loads, uniform per wave).
//                  ~10 VALU per key per 2 KiB: HBM-bound up to 16 keys.
//   k_fold4r       B > 16: Four-Russians.  Per 4-record group and 32-byte
//                  column a 16-entry table (entry e = XOR of the records
//                  whose bit is set in e) is built in LDS once per wave and
//                  looked up by up to 4 x 64 keys (lane = key): 2
//                  ds_read_b128 per key per group instead of 32 masked XORs.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <stdint.h>
#include <stdlib.h>

#include "dpf_kernels.hpp"
#include "fold_ops.hpp"
#include "pir_kernels.hpp"
#include "pir_scatter_plan.hpp"

namespace dpfk {

#ifdef DPF_FOLD_TIMES
constexpr uint64_t kFoldTimesMax = 1u << 14;
__device__ uint64_t g_fold_times[4 * kFoldTimesMax];
#endif

// v_bitop3_b32 truth tables: src0 = 0xF0, src1 = 0xCC, src2 = 0xAA.
constexpr uint8_t kTT0 = 0xF0, kTT1 = 0xCC, kTT2 = 0xAA;
__device__ __forceinline__ uint32_t x3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, kTT0 ^ kTT1 ^ kTT2);
}
// a ^ (b & m)
__device__ __forceinline__ uint32_t xam(uint32_t a, uint32_t b, uint32_t m) {
    return __builtin_amdgcn_bitop3_b32(a, b, m, kTT0 ^ (kTT1 & kTT2));
}
__device__ __forceinline__ uint4 x4(uint4 a, uint4 b) { return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w); }
__device__ __forceinline__ uint4 x4am(uint4 a, uint4 b, uint32_t m) {
    return make_uint4(xam(a.x, b.x, m), xam(a.y, b.y, m), xam(a.z, b.z, m), xam(a.w, b.w, m));
}
// Workgroup barrier of the folds' LDS staging: the plain barrier.  The
// compiler keeps a global prefetch in flight across it; fencing the local
// address space only measured identical (r05, profiles/r05/fold_barrier).
__device__ __forceinline__ void lds_barrier() { __syncthreads(); }
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Piece p (0..127) of sub-step q of chunk cc, as a 16-byte index into the DB.
// C > 1: contiguous records; C == 1: record stride rec_u4, column col (any
// record width that is a multiple of 32 B).  Indices past the end are
// clamped to the last record (its selection bit is masked off).
template <int C>
__device__ __forceinline__ uint64_t piece_index(uint64_t cc, uint32_t q, uint32_t p, uint64_t nrec, uint64_t rec_u4,
                                                uint32_t col) {
    if constexpr (C == 1) {
        uint64_t r = cc * 64 + (p >> 1);
        if (r >= nrec) r = nrec - 1;
        return r * rec_u4 + 2 * col + (p & 1);
    } else {
        const uint64_t last = nrec * 2 * C - 1;
        const uint64_t i = (cc * C + q) * 128 + p;
        return i < last ? i : last;
    }
}

// Bits of chunk cc's records below nrec, for word 0 (records 0..31) and 1;
// none when the chunk is not the caller's (live = false).  Arithmetic, not
// branches: a branch here splits the lookup block and the register
// allocator then spills the table reads around it.
__device__ __forceinline__ uint2 valid_mask(uint64_t cc, uint64_t nrec, bool live = true) {
    uint64_t v = nrec > cc * 64 ? nrec - cc * 64 : 0;
    v = live ? (v < 64 ? v : 64) : 0;
    const uint32_t lo = v < 32 ? (uint32_t)v : 32u, hi = v > 32 ? (uint32_t)v - 32u : 0u;
    return make_uint2((uint32_t)((1ull << lo) - 1), (uint32_t)((1ull << hi) - 1));
}

// ---------------------------------------------------------------------------
// k_fold_direct<C, KB>: up to KB keys per launch, 4 waves per workgroup, each
// wave takes every 4th chunk of the workgroup's contiguous range.  Lane l
// always holds the same 16-byte position u = l mod 2C of its records, so its
// accumulators are 4 words per key, XOR-reduced across lanes at the end.
// A streamed 16-byte operand; NT: a nontemporal load (the `nt` cache policy),
// for DB slices too large to stay in the caches between batches (launch_mfma).
typedef uint32_t fold_nt4 __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ uint4 fold_ld(const uint4* p) {
    if constexpr (NT) {
        const fold_nt4 v = __builtin_nontemporal_load(reinterpret_cast<const fold_nt4*>(p));
        return make_uint4(v.x, v.y, v.z, v.w);
    } else {
        return *p;
    }
}
constexpr int kFoldSkewDefault = 62;   // percent of a CU's chunk pair for its first k_fold4r workgroup (launch_4r)
constexpr int kDWaves = 4;
constexpr int kDirectMaxKeys = 16;

template <int C, int KB>
__global__ __launch_bounds__(64 * kDWaves) void k_fold_direct(const uint32_t* __restrict__ bits, uint64_t wpk,
                                                             const uint4* __restrict__ db, uint64_t nrec,
                                                             uint64_t rec_u4, uint32_t col, uint32_t nkeys,
                                                             uint64_t chunks_per_block, uint32_t* __restrict__ parts,
                                                             uint32_t* __restrict__ zero, uint64_t zero_words) {
    zero_answers(zero, zero_words);
    __shared__ uint32_t s_comb[kDWaves][KB][2 * C][4];
    const uint32_t l = threadIdx.x & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t nchunks = (nrec + 63) / 64;
    const uint64_t c0 = (uint64_t)blockIdx.x * chunks_per_block;
    const uint64_t cend = c0 + chunks_per_block < nchunks ? c0 + chunks_per_block : nchunks;
    uint32_t acc[KB][4];
#pragma unroll
    for (int k = 0; k < KB; ++k) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0;
    // Record (within the chunk) of sub-step q's pieces l (A) and 64 + l (B).
    const uint32_t rA0 = l / (2 * C);
    // Selection words travel like the pieces: lane l loads key (l mod KB)'s
    // word pair of a chunk together with the chunk's first sub-step (vector
    // loads, one chunk ahead), and v_readlane hands each key's pair to the
    // wave as scalars.  (Per-key scalar loads were each waited on where used.)
    const uint32_t skey = (l % KB) < nkeys ? (l % KB) : 0;
    auto load = [&](uint64_t cc, uint32_t q, uint4& A, uint4& B, uint2& S) __attribute__((always_inline)) {
        A = db[piece_index<C>(cc, q, l, nrec, rec_u4, col)];
        B = db[piece_index<C>(cc, q, 64 + l, nrec, rec_u4, col)];
        if (q == 0) {
            const uint64_t cs = cc < nchunks ? cc : nchunks - 1;
            S = *reinterpret_cast<const uint2*>(bits + skey * wpk + 2 * cs);
        }
    };
    // Items (chunk, sub-step) in pairs of chunks: 2C items, so the two load
    // buffers alternate by item parity and the next item's pieces are in
    // flight while this one is folded.  Every step issues its loads and XORs
    // unconditionally (indices clamped, selection bits masked): a branch
    // around a prefetch makes the compiler drain every load (s_waitcnt
    // vmcnt(0)) at the join.
    uint4 A0, B0, A1, B1;
    uint2 S0 = make_uint2(0, 0), S1 = make_uint2(0, 0);
    load(c0 + w, 0, A0, B0, S0);
    uint2 sel[KB];
    auto step = [&](uint64_t cp, int i, const uint4& A, const uint4& B, const uint2& S, uint4& NA, uint4& NB,
                    uint2& NS) __attribute__((always_inline)) {
        const uint64_t cc = cp + (uint64_t)(i / C) * kDWaves;
        const uint32_t q = (uint32_t)(i % C);
        const uint64_t nc = i + 1 < 2 * C ? cp + (uint64_t)((i + 1) / C) * kDWaves : cp + 2 * kDWaves;
        const uint32_t nq = i + 1 < 2 * C ? (uint32_t)((i + 1) % C) : 0;
        if (q == 0) {
            const uint2 vm = valid_mask(cc, nrec, cc < cend);
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                const bool live = (uint32_t)k < nkeys;
                const uint32_t sx = __builtin_amdgcn_readlane(S.x, k), sy = __builtin_amdgcn_readlane(S.y, k);
                sel[k] = make_uint2(live ? sx & vm.x : 0u, live ? sy & vm.y : 0u);
            }
        }
        load(nc, nq, NA, NB, NS);
        // Records of A and B: 64q/C + rA0 and that + 32/C.  For C = 1 they are
        // in words 0 and 1; for C >= 2 both are in word 2q/C.
        const uint32_t rA = (64 * q) / C + rA0, rB = rA + 32 / C;
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            const uint32_t wA = C == 1 ? sel[k].x : ((2 * q) / C ? sel[k].y : sel[k].x);
            const uint32_t wB = C == 1 ? sel[k].y : wA;
            const uint32_t mA = 0u - ((wA >> (rA & 31)) & 1u);
            const uint32_t mB = 0u - ((wB >> (rB & 31)) & 1u);
            acc[k][0] = xam(xam(acc[k][0], A.x, mA), B.x, mB);
            acc[k][1] = xam(xam(acc[k][1], A.y, mA), B.y, mB);
            acc[k][2] = xam(xam(acc[k][2], A.z, mA), B.z, mB);
            acc[k][3] = xam(xam(acc[k][3], A.w, mA), B.w, mB);
        }
    };
    for (uint64_t cp = c0 + w; cp < cend; cp += 2 * kDWaves) {
#pragma unroll
        for (int i = 0; i < 2 * C; i += 2) {
            step(cp, i, A0, B0, S0, A1, B1, S1);
            step(cp, i + 1, A1, B1, S1, A0, B0, S0);
        }
    }
    // Lanes with the same position u = l mod 2C hold partial XORs of the same words.
#pragma unroll
    for (int k = 0; k < KB; ++k) {
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            uint32_t v = acc[k][d];
#pragma unroll
            for (int off = 2 * C; off < 64; off *= 2) v ^= (uint32_t)__shfl_xor((int)v, off, 64);
            acc[k][d] = v;
        }
    }
    if (l < 2 * C) {
#pragma unroll
        for (int k = 0; k < KB; ++k)
#pragma unroll
            for (int d = 0; d < 4; ++d) s_comb[w][k][l][d] = acc[k][d];
    }
    __syncthreads();
    // parts[block][key][8C words]; word 4u + d of a key's answer is position u, dword d.
    constexpr uint32_t words = (uint32_t)KB * 8 * C;
    for (uint32_t t = threadIdx.x; t < words; t += blockDim.x) {
        const uint32_t k = t / (8 * C), u = (t / 4) % (2 * C), d = t % 4;
        uint32_t v = 0;
#pragma unroll
        for (int ww = 0; ww < kDWaves; ++ww) v ^= s_comb[ww][k][u][d];
        parts[(uint64_t)blockIdx.x * words + t] = v;
    }
}

// ---------------------------------------------------------------------------
// k_fold4r<C, KW, WV>: Four-Russians over 64*KW keys (lane l = keys l, 64+l,
// ...), WV waves per workgroup.  Per sub-step the wave owns 16 tables (4-record
// group gs x column cl, t = gs*C + cl), each two 256-byte rows (half h of the
// 32-byte column) of 16 slots:
//   stage : the loaded pieces go straight to their single-record slots
//           (entries 1, 2, 4, 8); entry 0 is a zero written once;
//   build : lanes 4t .. 4t+3 (h = l&1, a = (l>>1)&1) read the row's 4 records
//           and write the other 11 entries, 6 stores per lane;
//   lookup: each key-lane takes the group's 4 selection bits -- a nibble of
//           EvalFull's LSB-first layout -- as the entry index and XORs the
//           32-byte entry (2 ds_read_b128) into column cl's accumulator.
// Slot of entry e in row (t, h): f(e) ^ sw(t, h), f linear with f(8) = 11,
// sw = 2[t&1] ^ 1[t&2] ^ 4h (searched exhaustively): every staging store,
// build read and build store is conflict-free in its lane groups (8-lane
// groups over 32 banks for ds_write_b128, the 16-lane groups of ds_read_b128
// over 64 banks), lookups read one row and f is a bijection.
// The build is amortised over all 64*KW keys, so a B = 256 batch reads the DB
// once with 1/4 of the per-key table work of B = 64.

__host__ __device__ constexpr uint32_t f_slot(uint32_t e) { return e ^ (((e >> 3) & 1u) * 3u); }
__host__ __device__ constexpr uint32_t sw_row(uint32_t t, uint32_t h) {
    return ((t & 1u) ? 2u : 0u) ^ ((t & 2u) ? 1u : 0u) ^ (h ? 4u : 0u);
}

template <int WV>
struct Fold4rCfg {
    static constexpr int batch = 2 * WV;          // chunks per selection batch: 16*WV bytes of a key's bits
    static constexpr int sel_row = 4 * WV + 2;    // words per staged row (+2 pad: conflict-free ds_read_b64)
};

template <int C, int KW, int WV>
__global__ __launch_bounds__(64 * WV, WV == 8 ? 4 : 3) void k_fold4r(const uint32_t* __restrict__ bits, uint64_t wpk,
                                                                    const uint4* __restrict__ db, uint64_t nrec,
                                                                    uint64_t rec_u4, uint32_t col, uint32_t nkeys,
                                                                    uint64_t chunks_per_block,
                                                                    uint32_t* __restrict__ parts,
                                                                    uint32_t* __restrict__ zero, uint64_t zero_words,
                                                                    uint32_t nfirst, uint64_t cpb_first) {
    zero_answers(zero, zero_words);
    using Cfg = Fold4rCfg<WV>;
    __shared__ uint4 s_tab[WV][32 * 16];                                   // 8 KiB per wave
    __shared__ __attribute__((aligned(16))) uint32_t s_sel[KW * 64 * Cfg::sel_row];
    const uint32_t l = threadIdx.x & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t nchunks = (nrec + 63) / 64;
    // The first nfirst workgroups (dispatched first: one per CU) take
    // cpb_first chunks, the rest chunks_per_block (fold_split below).
    const uint64_t b = blockIdx.x;
    const uint64_t c0 = b < nfirst ? b * cpb_first : nfirst * cpb_first + (b - nfirst) * chunks_per_block;
    const uint64_t my = b < nfirst ? cpb_first : chunks_per_block;
    const uint64_t cend = c0 + my < nchunks ? c0 + my : nchunks;
    uint4* tab = s_tab[w];
#ifdef DPF_FOLD_TIMES
    const uint64_t t_start = wall_clock64();
#endif

    // Entry 0 of every row: a zero slot, written once.
    if (l < 32) tab[l * 16 + sw_row(l >> 1, l & 1)] = make_uint4(0, 0, 0, 0);
    // Staging slots of this lane's pieces p = l (A) and 64 + l (B, table + 8).
    const uint32_t pr = l / (2 * C), pcl = (l / 2) % C, ph = l & 1;
    const uint32_t pt = (pr >> 2) * C + pcl, pi = pr & 3;
    const uint32_t stA = (2 * pt + ph) * 16 + (f_slot(1u << pi) ^ sw_row(pt, ph));
    const uint32_t stB = stA + 16 * 16;
    // Build role: row (bt, bh), lane pair a.
    const uint32_t bt = l >> 2, bh = l & 1, ba = (l >> 1) & 1;
    uint4* brow = tab + (2 * bt + bh) * 16;
    const uint32_t bsw = sw_row(bt, bh);
    const uint32_t m0 = ba ? 0u : ~0u;

    // Selection staging: thread t copies 16 B of key (kg*64 + t/WV)'s line.
    const uint32_t sk = threadIdx.x / WV, sp = threadIdx.x % WV;
    auto load_sel = [&](int kg, uint64_t cb) __attribute__((always_inline)) {
        const uint32_t key = (uint32_t)kg * 64 + sk;
        const uint32_t* srow = bits + (uint64_t)(key < nkeys ? key : 0) * wpk;
        const uint64_t wo = cb * 2 + 4 * sp;                         // clamped, then zeroed: no branch
        const uint4 v = *reinterpret_cast<const uint4*>(srow + (wo + 4 <= wpk ? wo : wpk - 4));
        return wo + 4 <= wpk ? v : make_uint4(0, 0, 0, 0);
    };
    uint32_t keymask[KW];
#pragma unroll
    for (int kg = 0; kg < KW; ++kg) keymask[kg] = (uint32_t)kg * 64 + l < nkeys ? ~0u : 0u;

    uint32_t acc[KW][C][8];
#pragma unroll
    for (int kg = 0; kg < KW; ++kg)
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[kg][c][i] = 0;

    auto fold = [&](uint64_t cc, uint32_t q, uint64_t cb, const uint4& A, const uint4& B) __attribute__((always_inline)) {
        // stage
        tab[stA] = A;
        tab[stB] = B;
        wave_sync();
        // build: R_i = record i of this row's group
        const uint4 R0 = brow[f_slot(1) ^ bsw], R1 = brow[f_slot(2) ^ bsw];
        const uint4 R2 = brow[f_slot(4) ^ bsw], R3 = brow[f_slot(8) ^ bsw];
        const uint4 R12 = x4(R1, R2), R13 = x4(R1, R3), R23 = x4(R2, R3), R123 = x4(R12, R3);
        // a = 0 writes 7, 11, 13, 15, 3, 5; a = 1 writes 6, 10, 12, 14, 9.
        brow[f_slot(7 ^ ba) ^ bsw] = x4am(R12, R0, m0);
        brow[f_slot(11 ^ ba) ^ bsw] = x4am(R13, R0, m0);
        brow[f_slot(13 ^ ba) ^ bsw] = x4am(R23, R0, m0);
        brow[f_slot(15 ^ ba) ^ bsw] = x4am(R123, R0, m0);
        const uint4 S = ba ? R3 : R1;
        brow[f_slot(ba ? 9 : 3) ^ bsw] = x4(R0, S);
        if (!ba) brow[f_slot(5) ^ bsw] = x4(R0, R2);
        wave_sync();
        // lookups
        const uint32_t j = (uint32_t)(cc - cb);
        const uint2 vm = valid_mask(cc, nrec);
#pragma unroll
        for (int kg = 0; kg < KW; ++kg) {
            // One lane group at a time: interleaving their reads only spills.
            if (kg) __builtin_amdgcn_sched_barrier(0);
            uint2 sel = *reinterpret_cast<const uint2*>(&s_sel[(kg * 64 + l) * Cfg::sel_row + 2 * j]);
            sel.x &= vm.x & keymask[kg];
            sel.y &= vm.y & keymask[kg];
            // Nibbles n of this sub-step: n = q*16/C + gs, gs < 16/C (word n >> 3).
            // Pre-swizzle: f applied to every nibble.
            auto fz = [](uint32_t z) __attribute__((always_inline)) {
                const uint32_t m = (z >> 3) & 0x11111111u;
                return z ^ m ^ (m << 1);
            };
            const uint32_t z0 = fz(sel.x), z1 = fz(sel.y);
            // Tables t and t + C share column cl: one 3-input XOR per word for
            // both (the bitop3 builtin also keeps the compiler from
            // re-associating the chain).  The 8 pairs are software-pipelined:
            // pair p + 1's 4 reads are issued before pair p's XORs, with
            // scheduling fences so the compiler keeps that order (left alone,
            // it reads one pair, waits, XORs: 4 reads in flight per wave).
            // A second pair in flight gave no gain (fold_bench r03).
            auto slot = [&](uint32_t t) __attribute__((always_inline)) {
                const uint32_t n = q * (16 / C) + t / C;
                const uint32_t z = (n >> 3) ? z1 : z0;
                return (z >> (4 * (n & 7))) & 15u;
            };
            constexpr int kPairs = 8;
            uint4 rd[kPairs][4];
            auto pair_t0 = [](int pi) { return (pi / C) * 2 * C + pi % C; };   // pair pi = tables (t0, t0 + C)
            auto issue = [&](int pi) __attribute__((always_inline)) {
                const uint32_t t0 = pair_t0(pi), t1 = t0 + C;
                const uint32_t e0 = slot(t0), e1 = slot(t1);
                rd[pi][0] = tab[(2 * t0) * 16 + (e0 ^ sw_row(t0, 0))];
                rd[pi][1] = tab[(2 * t0 + 1) * 16 + (e0 ^ sw_row(t0, 1))];
                rd[pi][2] = tab[(2 * t1) * 16 + (e1 ^ sw_row(t1, 0))];
                rd[pi][3] = tab[(2 * t1 + 1) * 16 + (e1 ^ sw_row(t1, 1))];
            };
            issue(0);
#pragma unroll
            for (int pi = 0; pi < kPairs; ++pi) {
                if (pi + 1 < kPairs) issue(pi + 1);
                __builtin_amdgcn_sched_barrier(0);
                const uint4 lo0 = rd[pi][0], hi0 = rd[pi][1], lo1 = rd[pi][2], hi1 = rd[pi][3];
                uint32_t* a = acc[kg][pair_t0(pi) % C];
                a[0] = x3(a[0], lo0.x, lo1.x); a[1] = x3(a[1], lo0.y, lo1.y);
                a[2] = x3(a[2], lo0.z, lo1.z); a[3] = x3(a[3], lo0.w, lo1.w);
                a[4] = x3(a[4], hi0.x, hi1.x); a[5] = x3(a[5], hi0.y, hi1.y);
                a[6] = x3(a[6], hi0.z, hi1.z); a[7] = x3(a[7], hi0.w, hi1.w);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        wave_sync();
    };

    // Batches of Cfg::batch chunks (one 16*WV-byte piece of every key's bits);
    // each wave takes chunks cb + w and cb + WV + w of a batch, C sub-steps
    // each.  Loads ping-pong between two buffers (2C items per batch, even),
    // so the next sub-step's records are in flight during a fold.
    auto load = [&](uint64_t cc, uint32_t q, uint4& A, uint4& B) __attribute__((always_inline)) {
        A = db[piece_index<C>(cc, q, l, nrec, rec_u4, col)];
        B = db[piece_index<C>(cc, q, 64 + l, nrec, rec_u4, col)];
    };
    uint4 A0, B0, A1, B1;
    load(c0 + w, 0, A0, B0);
    uint4 snext[KW];
#pragma unroll
    for (int kg = 0; kg < KW; ++kg) snext[kg] = load_sel(kg, c0);
    auto step = [&](uint64_t cb, int i, const uint4& A, const uint4& B, uint4& NA, uint4& NB) __attribute__((always_inline)) {
        const uint64_t cc = cb + w + (uint64_t)(i / C) * WV;
        const uint32_t q = (uint32_t)(i % C);
        const uint64_t nc = i + 1 < 2 * C ? cb + w + (uint64_t)((i + 1) / C) * WV : cb + Cfg::batch + w;
        const uint32_t nq = i + 1 < 2 * C ? (uint32_t)((i + 1) % C) : 0;
        load(nc, nq, NA, NB);            // unconditional (clamped): see k_fold_direct
        if (cc < cend) fold(cc, q, cb, A, B);
    };
    for (uint64_t cb = c0; cb < cend; cb += Cfg::batch) {
        lds_barrier();                                     // previous batch's selection reads are done
#pragma unroll
        for (int kg = 0; kg < KW; ++kg) {
            uint32_t* row = &s_sel[(kg * 64 + sk) * Cfg::sel_row + 4 * sp];
            *reinterpret_cast<uint2*>(row) = make_uint2(snext[kg].x, snext[kg].y);
            *reinterpret_cast<uint2*>(row + 2) = make_uint2(snext[kg].z, snext[kg].w);
        }
        lds_barrier();
#pragma unroll
        for (int kg = 0; kg < KW; ++kg) snext[kg] = load_sel(kg, cb + Cfg::batch);
#pragma unroll
        for (int i = 0; i < 2 * C; i += 2) {
            step(cb, i, A0, B0, A1, B1);
            step(cb, i + 1, A1, B1, A0, B0);
        }
    }
#ifdef DPF_FOLD_TIMES
    // Measurement build only (tools/fold_bench.hip -DDPF_FOLD_TIMES): per
    // wave, start / end of its chunk loop and the CU it ran on.
    if (l == 0) {
        const uint64_t wv = (uint64_t)blockIdx.x * WV + w;
        if (wv < kFoldTimesMax) {
            g_fold_times[4 * wv] = t_start;
            g_fold_times[4 * wv + 1] = wall_clock64();
            g_fold_times[4 * wv + 2] = __builtin_amdgcn_s_getreg(0xF804);   // HW_ID
            g_fold_times[4 * wv + 3] = __builtin_amdgcn_s_getreg(0xF814);   // XCC_ID
        }
    }
#endif
    // Combine the workgroup's waves in LDS (reusing the tables), one
    // 8-word slice (key group, column) at a time: parts[block][key][8C words].
    constexpr uint32_t pkeys = 64 * KW, pwords = 8 * C;
    uint32_t* comb = reinterpret_cast<uint32_t*>(&s_tab[0][0]);     // [wave][lane][8]
#pragma unroll
    for (int kg = 0; kg < KW; ++kg)
#pragma unroll
        for (int c = 0; c < C; ++c) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 8; ++i) comb[(w * 64 + l) * 8 + i] = acc[kg][c][i];
            __syncthreads();
            for (uint32_t t = threadIdx.x; t < 64 * 8; t += blockDim.x) {
                uint32_t v = 0;
#pragma unroll
                for (int ww = 0; ww < WV; ++ww) v ^= comb[ww * 64 * 8 + t];
                const uint32_t key = kg * 64 + t / 8;
                parts[((uint64_t)blockIdx.x * pkeys + key) * pwords + c * 8 + (t % 8)] = v;
            }
        }
}

// ans[k * ans_words + off + i] ^= XOR over workgroups p of parts[p][k][i]
// (k < nkeys, i < pwords; pkeys keys per part).  Block (x, y): 256 words x
// parts y, y + gridDim.y, ...; one atomicXor each.
__global__ __launch_bounds__(256) void k_xor_parts(const uint32_t* __restrict__ parts, uint64_t nparts, uint32_t nkeys,
                                                   uint32_t pkeys, uint32_t pwords, uint32_t* __restrict__ ans,
                                                   uint64_t ans_words, uint32_t off) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nkeys * pwords) return;
    const uint32_t k = t / pwords, i = t % pwords;
    uint32_t v = 0;
    // Eight independent loads in flight per step (a strided loop of single
    // loads left the kernel at ~5 us, mostly dependent L2 round trips).
    const uint64_t g = gridDim.y;
    uint64_t p = blockIdx.y;
    for (; p + 7 * g < nparts; p += 8 * g) {
        uint32_t x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = parts[((p + u * g) * pkeys + k) * pwords + i];
#pragma unroll
        for (int u = 0; u < 8; ++u) v ^= x[u];
    }
    for (; p < nparts; p += g) v ^= parts[(p * pkeys + k) * pwords + i];
    if (v) atomicXor(ans + (uint64_t)k * ans_words + off + i, v);
}

// XOR nparts workgroup partials into the answers (stream-ordered after the fold).
hipError_t launch_xor_parts(const uint32_t* parts, uint64_t nparts, uint32_t nkeys, uint32_t pkeys,
                            uint32_t pwords, uint32_t* ans, uint64_t ans_words, uint32_t off, hipStream_t st) {
    // Part slices per answer word, one atomic each: 16 for <= 256 partials
    // (the PIR rank at N = 8: step 0.0733-0.0737 vs 0.0740-0.0745 ms with 64,
    // 8 in between), 64 above (one GPU, 768 partials: 0.3799-0.3802 vs
    // 0.3811-0.3817 with 16); tools/archive/r05_xys.sh, profiles/r05/xor_parts/.
    // DPF_XOR_PARTS_YS=<n> (measurement only) fixes it.
    static const uint64_t yenv = [] {
        const char* e = getenv("DPF_XOR_PARTS_YS");
        return e && atoi(e) > 0 ? (uint64_t)atoi(e) : 0ull;
    }();
    const uint64_t ymax = yenv ? yenv : nparts <= 256 ? 16 : 64;
    const uint32_t ys = (uint32_t)(nparts < ymax ? nparts : ymax);
    hipLaunchKernelGGL(k_xor_parts, dim3((nkeys * pwords + 255) / 256, ys), dim3(256), 0, st, parts, nparts, nkeys,
                       pkeys, pwords, ans, ans_words, off);
    return hipGetLastError();
}

static int cu_count_fold() { return cu_count(); }   // the calling thread's CU budget (dpf_kernels.hip)

constexpr uint64_t kFoldPartBytes = 64 * 4 * 32 * 2;   // largest part: 64*KW keys x 32C bytes, KW*C <= 8
constexpr uint32_t kFoldMaxSgPerBlock = 1u << 15; // k_fold_mfma: super-groups per workgroup (fp32-exact counts)

uint64_t pir_fold_parts_bytes() { return kFoldMaxBlocks * kFoldPartBytes; }

// Tuning / test limits (set_fold_limits): workgroups per fold launch and
// super-groups per matrix-core fold workgroup.
static std::atomic<uint32_t> g_fold_blocks{(uint32_t)kFoldMaxBlocks};
static std::atomic<uint32_t> g_fold_max_sg{kFoldMaxSgPerBlock};
static uint32_t fold_max_sg() { return g_fold_max_sg.load(std::memory_order_relaxed); }
void set_fold_limits(uint32_t max_blocks, uint32_t max_sg) {
    g_fold_blocks.store(max_blocks == 0 || max_blocks > kFoldMaxBlocks ? (uint32_t)kFoldMaxBlocks : max_blocks);
    g_fold_max_sg.store(max_sg == 0 || max_sg > kFoldMaxSgPerBlock ? kFoldMaxSgPerBlock : max_sg);
}

namespace {

// Split nchunks into `blocks` contiguous ranges of whole `gran`-chunk batches.
// cap_in: the workgroup cap the caller sized its passes with (0: read it
// here); a launcher that derives a per-workgroup bound from the cap must pass
// the value it read, so a concurrent dpf_set_fold_limits cannot change it
// between the two reads.
void split_chunks(uint64_t nchunks, uint64_t want_blocks, uint64_t gran, uint64_t& blocks, uint64_t& cpb,
                  uint64_t cap_in = 0) {
    const uint64_t cap = cap_in ? cap_in : g_fold_blocks.load(std::memory_order_relaxed);
    if (want_blocks > cap) want_blocks = cap;
    cpb = (nchunks + want_blocks - 1) / want_blocks;
    cpb = (cpb + gran - 1) / gran * gran;
    blocks = (nchunks + cpb - 1) / cpb;
}

struct FoldArgs {
    const uint32_t* bits;
    uint64_t wpk;
    const uint4* db;
    uint64_t nrec, rec_u4;
    uint32_t col, nkeys;
    uint32_t* parts;
    uint32_t* zero;          // first pass: the answers, cleared before k_xor_parts XORs into them
    uint64_t zero_words;
};

template <int C, int KB>
hipError_t launch_direct_kb(const FoldArgs& a, uint64_t nchunks, uint64_t& blocks, hipStream_t st) {
    uint64_t cpb;
    split_chunks(nchunks, (uint64_t)cu_count_fold() * 4, 2 * kDWaves, blocks, cpb);
    hipLaunchKernelGGL((k_fold_direct<C, KB>), dim3((uint32_t)blocks), dim3(64 * kDWaves), 0, st, a.bits, a.wpk, a.db,
                       a.nrec, a.rec_u4, a.col, a.nkeys, cpb, a.parts, a.zero, a.zero_words);
    return hipGetLastError();
}

// The direct kernel's work is linear in its key slots: 1, 4 or 16 by batch.
template <int C>
hipError_t launch_direct(const FoldArgs& a, uint64_t nchunks, uint64_t& blocks, uint32_t& pkeys, hipStream_t st) {
    if (a.nkeys <= 1) return pkeys = 1, launch_direct_kb<C, 1>(a, nchunks, blocks, st);
    if (a.nkeys <= 4) return pkeys = 4, launch_direct_kb<C, 4>(a, nchunks, blocks, st);
    return pkeys = kDirectMaxKeys, launch_direct_kb<C, kDirectMaxKeys>(a, nchunks, blocks, st);
}

template <int C, int KW>
hipError_t launch_4r(const FoldArgs& a, uint64_t nchunks, uint64_t& blocks, hipStream_t st) {
    // KW = 1, C < 8: 8 waves, 72 KiB of LDS -> 2 workgroups (16 waves, 128
    // VGPRs) per CU.  Otherwise 4 waves, 41-50 KiB -> 3 per CU (168 VGPRs:
    // 64 accumulators per lane).
    constexpr int WV = KW == 1 && C < 8 ? 8 : 4;
    const uint64_t cus = (uint64_t)cu_count_fold();
    const uint64_t per_cu = WV == 8 ? 2 : 3;
    uint64_t cpb;
    split_chunks(nchunks, cus * per_cu, 2 * WV, blocks, cpb);
    // Two workgroups per CU: a SIMD's waves issue oldest-first, so the CU's
    // first workgroup runs ahead of its second (fold per-wave times: 100 vs
    // 143 us at configs[4]).  DPF_FOLD_SKEW (percent of a CU pair's chunks
    // for the first workgroup) shifts work to it.
    static const int skew = [] {
        const char* e = getenv("DPF_FOLD_SKEW");
        return e ? atoi(e) : kFoldSkewDefault;
    }();
    uint32_t nfirst = 0;
    uint64_t cpb_first = cpb;
    const uint64_t gran = 2 * WV;
    if (per_cu == 2 && skew > 50 && skew < 100 && blocks == 2 * cus) {
        const uint64_t pair = 2 * cpb;
        cpb_first = (pair * (uint64_t)skew / 100 + gran / 2) / gran * gran;
        const uint64_t rest = pair - cpb_first;
        if (rest >= gran && nchunks <= cus * pair) {
            nfirst = (uint32_t)cus;
            cpb = rest;
        } else {
            cpb_first = cpb;
        }
    }
    hipLaunchKernelGGL((k_fold4r<C, KW, WV>), dim3((uint32_t)blocks), dim3(64 * WV), 0, st, a.bits, a.wpk, a.db,
                       a.nrec, a.rec_u4, a.col, a.nkeys, cpb, a.parts, a.zero, a.zero_words, nfirst, cpb_first);
    return hipGetLastError();
}

// One pass over the DB for `a.nkeys` keys (<= 64*KW or <= 16 direct) with C
// columns per record: fold kernel, then k_xor_parts into ans.
template <int C>
hipError_t fold_pass(const FoldArgs& a, bool direct, int kw, uint32_t* ans, uint64_t ans_words, uint32_t off,
                     hipStream_t st) {
    const uint64_t nchunks = (a.nrec + 63) / 64;
    uint64_t blocks = 0;
    uint32_t pkeys;
    hipError_t e;
    if (direct) {
        e = launch_direct<C>(a, nchunks, blocks, pkeys, st);
    } else if (kw >= 4) {
        if constexpr (C <= 2) e = launch_4r<C, 4>(a, nchunks, blocks, st);
        else return hipErrorInvalidValue;
        pkeys = 256;
    } else if (kw == 2) {
        if constexpr (C <= 4) e = launch_4r<C, 2>(a, nchunks, blocks, st);
        else return hipErrorInvalidValue;
        pkeys = 128;
    } else {
        e = launch_4r<C, 1>(a, nchunks, blocks, st);
        pkeys = 64;
    }
    if (e != hipSuccess) return e;
    return launch_xor_parts(a.parts, blocks, a.nkeys, pkeys, 8 * C, ans, ans_words, off, st);
}

}  // namespace

// ---------------------------------------------------------------------------
// The fold as a GF(2) matrix product on the matrix cores.
//
//   count[k][n] = sum_i sel[k][i] * dbbit[i][n],   ans bit (k, n) = count & 1
//
// is a {0,1} product of [keys x records] by [records x 256 bit positions], so
// it runs on v_mfma_scale_f32_32x32x64_f8f6f4 with e2m1 (FP4) operands: every
// product is exactly 1 or 0, the fp32 accumulators hold exact counts (far
// below 2^24 per workgroup, see below), and the parity is the answer bit.
//
// Operands.  An MFMA operand lane holds 32 K-values (records) of ONE row
// (key) or column (bit position); the K order inside the lane is ours to
// pick as long as A and B agree.  The key side is EvalFull's own layout: one
// selection word = 32 consecutive records of one key.  The DB side needs the
// transposed form -- for bit position n, one word of 32 consecutive records
// -- which the PIR server builds once when the DB is loaded (the "sliced"
// layout, k_slice_db below).  A record of rec_bytes = 32 C bytes is C 32-byte
// columns:
//   dbs[S][c][n][g] (u32), S = super-group of 256 records, c < C column,
//   n < 256 bit position of the column, g < 8 record group; bit j = bit n of
//   bytes [32c, 32c + 32) of record 256 S + 32 g + j
// (32-byte records: C = 1, dbs[S][n][g]).  A lane (n, h) loads
// dbs[S][c][n][4h .. 4h+3] and a key lane (k, h) takes selection words
// 8S + 4h .. +3 (one dwordx4 each): K-block t < 4 of super-group S is record
// groups t (h = 0) and 4 + t (h = 1).
// Word -> FP4 operand in registers, nibble i of dword d = record 4i + d:
//   one side  d0 = x & 0x1..  (0.5)  d1 = x & 0x2.. (1.0)  d2 = x & 0x4.. (2.0)
//             d3 = (x >> 1) & 0x4.. (2.0)                       5 VALU per word
//   the other d0 = (s << 2) & 0x4.. (2.0)  d1 = s & 0x2.. (1.0)
//             d2 = (s >> 2) & 0x1.. (0.5)  d3 = (s >> 3) & 0x1.. (0.5)   7 VALU
// so every nonzero product is exactly 1 with unit (E8M0 127) scales.
//
// Mapping.  A wave covers MT key tiles (32 keys) x NT bit tiles (32 bit
// positions) of one column over a contiguous run of super-groups.  To the
// fold a wide record is a record of 8 C bit tiles instead of 8, and a
// selection operand is the same for every tile, so a workgroup takes a column
// group of CG columns: CG * NS waves, NS = 8 / NT; wave wv folds bit slice
// wv % NS of column wv / NS of the group.  Then
//   - a staged block's selection rows are loaded and written to LDS once for
//     all CG columns (selection bytes per DB byte 1 / (4 CG));
//   - the workgroup's DB stream is runs of CG * 8 KiB, one per super-group.
// Column groups are the grid's y dimension: every workgroup of a launch holds
// a (super-group run, column group) pair, workgroups per launch x * y <= the
// workgroup cap.  At the end each accumulator register's parities become two
// answer words by one ballot (C/D layout: lane = column n, register e = rows
// (e&3) + 8(e>>2) + 4h), written to the workgroup's partial, and one
// k_xor_parts launch combines
//   parts[x][key][8 CG y words]
// into the answers.  32-byte records are ncols = 1, CG = 1, grid.y = 1.  CG is
// the largest of 4, 2, 1 that divides C, capped by what the tile shape's
// registers allow (launch_pir_fold_sliced).
//
// Selection words reach the waves through LDS: per block of SG super-groups
// the workgroup copies each key's SG*32-byte span (coalesced) into a padded
// row, and the next block's selection words and DB pieces are in flight in
// registers while this block is folded (block-level double buffering: a
// super-group of MFMA work is ~0.2-0.4 us per wave, shorter than the HBM
// latency under load).  Loaded straight into the operand lanes, 16 B per
// lane from 32 rows 2 MiB apart, the fold fetched ~1.6x its bytes and ran at
// a third of the HBM rate (profiles/r04/fold_v1).
//
// Exactness of the fp32 counts: an accumulator gains at most 64 per MFMA
// (one per record of a K-block), and fp32 holds every integer up to 2^24.
// A workgroup's run of super-groups would grow with the DB and shrink with
// the CU count, so launch_mfma never gives one more than
// kFoldMaxSgPerBlock = 2^15 super-groups (2^23 records): it adds workgroups,
// and beyond kFoldMaxBlocks of them it folds the DB in passes, each pass's
// partials XORed into the answers.  (Reducing the counts to parities inside
// the kernel moved the large-tile accumulators out of AGPRs and spilled them:
// 2.5x slower at 256 keys, r05.)  wlim: selection words per key row from
// `bits` (the row stride stays wpk), so a pass can start mid-row.  The
// operand expansions themselves (fp4_w5, fp4_w7) are in fold_ops.hpp.
//
// k_fold_mfma<MT, NT, SG, CG, NTDB, WPE>: tile shape, super-groups per staged
// block, columns per workgroup, nontemporal DB loads, and the waves per SIMD
// the shape is compiled for (its register budget).  cg0: first column group
// of the launch.
template <int MT, int NT, int SG, int CG, bool NTDB, int WPE>
__global__ __launch_bounds__(64 * (8 / NT) * CG, WPE) void k_fold_mfma(
    const uint32_t* __restrict__ bits, uint64_t wpk, const uint4* __restrict__ dbs, uint64_t nsg, uint32_t nkeys,
    uint64_t sg_per_block, uint32_t* __restrict__ parts, uint32_t* __restrict__ zero, uint64_t zero_words,
    uint64_t wlim, uint32_t ncols, uint32_t cg0) {
    constexpr int NS = 8 / NT;                                 // bit slices of a column
    constexpr int NW = NS * CG;
    constexpr bool SC = NT < MT;                               // the selection side takes the cheap expansion
    constexpr int kRows = 32 * MT;
    constexpr int kRow = SG * 8 + 4;                           // words per staged row (+4: conflict-free b128 reads)
    constexpr int kPieces = kRows * (SG * 2);                  // uint4 pieces per staged block
    constexpr int kPer = (kPieces + 64 * NW - 1) / (64 * NW);  // per thread
    __shared__ __attribute__((aligned(16))) uint32_t s_sel[kRows * kRow];
    zero_answers(blockIdx.y == 0 ? zero : nullptr, zero_words);
    const uint32_t l = threadIdx.x & 63, h = l >> 5, r = l & 31;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t w = wv % NS, cw = wv / NS;                   // bit slice, column of the group
    const uint64_t col = (uint64_t)(cg0 + blockIdx.y) * CG + cw;
    const uint64_t s0 = (uint64_t)blockIdx.x * sg_per_block;
    const uint64_t s1 = s0 + sg_per_block < nsg ? s0 + sg_per_block : nsg;
    if (s0 >= s1) return;                                       // uniform over the workgroup
    auto load_sel = [&](uint64_t sb, uint4 (&v)[kPer]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const uint32_t p = threadIdx.x + (uint32_t)i * 64 * NW;
            const uint32_t row = p / (2 * SG), q = p % (2 * SG);
            const uint64_t word = sb * 8 + 4 * q;
            const bool ok = p < (uint32_t)kPieces && row < nkeys && word + 4 <= wlim;
            const uint4 x = *reinterpret_cast<const uint4*>(bits + (ok ? (uint64_t)row * wpk + word : 0));
            v[i] = ok ? x : make_uint4(0, 0, 0, 0);
        }
    };
    auto store_sel = [&](const uint4 (&v)[kPer]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < kPer; ++i) {
            const uint32_t p = threadIdx.x + (uint32_t)i * 64 * NW;
            if (p < (uint32_t)kPieces) *reinterpret_cast<uint4*>(&s_sel[(p / (2 * SG)) * kRow + 4 * (p % (2 * SG))]) = v[i];
        }
    };
    // DB pieces of a whole block (clamped past the range; never folded).
    auto load_db = [&](uint64_t sb, uint4 (&B)[SG][NT]) __attribute__((always_inline)) {
#pragma unroll
        for (int sl = 0; sl < SG; ++sl) {
            const uint64_t S = sb + sl < s1 ? sb + sl : s1 - 1;
#pragma unroll
            for (int j = 0; j < NT; ++j)
                B[sl][j] = fold_ld<NTDB>(&dbs[((S * ncols + col) * 256 + 32u * (w * NT + j) + r) * 2 + h]);
        }
    };
    fold_v16f acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][j][e] = 0.0f;
    // One super-group: 4 K-blocks of 64 records x MT x NT MFMAs.
    auto fold_sg = [&](int sl, const uint4 (&B)[NT]) __attribute__((always_inline)) {
        uint4 A[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
            A[m] = *reinterpret_cast<const uint4*>(&s_sel[(32 * m + r) * kRow + 8 * sl + 4 * h]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            fold_v8i bo[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) bo[j] = fp4_db<SC>(u4w(B[j], t));
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const fold_v8i ao = fp4_sel<SC>(u4w(A[m], t));
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[m][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(ao, bo[j], acc[m][j], kFoldFp4, kFoldFp4,
                                                                               0, kE8M0One, 0, kE8M0One);
            }
        }
    };
    uint4 sv[kPer];
    uint4 BA[SG][NT], BB[SG][NT];
    load_sel(s0, sv);
    load_db(s0, BA);
    // One staged block: its selection rows to LDS, the next block's loads
    // issued, then its super-groups folded.
    auto block = [&](uint64_t sb, const uint4 (&Bc)[SG][NT], uint4 (&Bn)[SG][NT]) __attribute__((always_inline)) {
        lds_barrier();                                          // previous block's operand reads are done
        store_sel(sv);
        lds_barrier();
        const uint64_t nb = sb + SG < s1 ? sb + SG : sb;        // next block (clamped)
        load_sel(nb, sv);
        load_db(nb, Bn);
        const uint64_t n = s1 - sb;
#pragma unroll
        for (int sl = 0; sl < SG; ++sl)
            if ((uint64_t)sl < n) fold_sg(sl, Bc[sl]);
    };
    uint64_t sb = s0;
    for (; sb + SG < s1; sb += 2 * SG) {
        block(sb, BA, BB);
        block(sb + SG, BB, BA);
    }
    if (sb < s1) block(sb, BA, BB);
    // Parities -> answer words: parts[x][key][8 CG y] (word = 8 * column of the launch + bit tile).
    constexpr uint32_t pkeys = 32 * MT;
    const uint32_t pwords = 8u * CG * gridDim.y;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            uint32_t out = 0;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint32_t p = ((uint32_t)acc[m][j][e]) & 1u;
                const uint64_t b = __builtin_amdgcn_ballot_w64(p != 0);
                const uint32_t row0 = (e & 3) + 8 * (e >> 2);
                out = l == row0 ? (uint32_t)b : out;
                out = l == row0 + 4 ? (uint32_t)(b >> 32) : out;
            }
            if (l < 32)
                parts[((uint64_t)blockIdx.x * pkeys + 32 * m + l) * pwords + (blockIdx.y * CG + cw) * 8 + w * NT + j] = out;
        }
}

// The sliced layout (above) from a row-major DB of 32 C-byte records.
// Workgroup b = (super-group S, column c) = (b / C, b % C); its 4 waves take
// 64 records each: lane l holds the column's 8 words of record l and one
// ballot per bit position transposes 32 x 32 bits.
__global__ __launch_bounds__(256) void k_slice_db(const uint4* __restrict__ db, uint64_t nrec, uint32_t ncols,
                                                   uint32_t* __restrict__ dbs) {
    const uint64_t S = blockIdx.x / ncols;
    const uint32_t c = blockIdx.x % ncols;
    const uint32_t l = threadIdx.x & 63, wq = threadIdx.x >> 6;
    const uint64_t rec = S * 256 + wq * 64 + l;
    uint4 a = make_uint4(0, 0, 0, 0), b = a;
    if (rec < nrec) {
        a = db[rec * 2 * ncols + 2 * c];
        b = db[rec * 2 * ncols + 2 * c + 1];
    }
    const uint32_t wd[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const uint32_t g = 2 * wq + (l >> 5);
#pragma unroll
    for (int wi = 0; wi < 8; ++wi) {
        uint32_t out = 0;
#pragma unroll
        for (int bb = 0; bb < 32; ++bb) {
            const uint64_t m = __builtin_amdgcn_ballot_w64(((wd[wi] >> bb) & 1u) != 0);
            out = l == (uint32_t)bb ? (uint32_t)m : out;
            out = l == (uint32_t)bb + 32 ? (uint32_t)(m >> 32) : out;
        }
        dbs[((S * ncols + c) * 256 + 32 * wi + (l & 31)) * 8 + g] = out;
    }
}

// One key over the sliced DB: no matrix product needed.  Workgroup (x, y)
// folds super-group run x of column c0 + y; thread n of its 256 owns bit
// position n of that column.  Per super-group it reads its 8 words
// dbs[S][c][n][0..7] (the workgroup: 8 KiB contiguous) and XORs (selection
// word & DB word) into acc -- one v_bitop3 per word, the selection words
// wave-uniform (scalar loads).  The answer bit n is the parity of
// popcount(acc).  parts[x][8 y words].  One key only (97 us at configs[4]
// against the MFMA fold's 103): with 4 or 16 keys the per-key scalar loads
// serialise (131 / 388 us against 104 / 107, profiles/r04/fold_ab/).
// (Nontemporal DB loads, as the matrix-core fold takes them above 256 MiB,
// measured 95.2-95.8 against 93.9-94.4 us here at 2^24 records: not used.)
__global__ __launch_bounds__(256) void k_fold_sliced_direct(const uint32_t* __restrict__ bits,
                                                            const uint4* __restrict__ dbs, uint64_t nsg,
                                                            uint64_t sg_per_block, uint32_t* __restrict__ parts,
                                                            uint32_t* __restrict__ zero, uint64_t zero_words,
                                                            uint64_t wlim, uint32_t ncols, uint32_t c0) {
    zero_answers(blockIdx.y == 0 ? zero : nullptr, zero_words);
    const uint32_t n = threadIdx.x, l = n & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t col = c0 + blockIdx.y;
    const uint64_t s0 = (uint64_t)blockIdx.x * sg_per_block;
    const uint64_t s1 = s0 + sg_per_block < nsg ? s0 + sg_per_block : nsg;
    uint32_t acc = 0;
    auto fold = [&](uint64_t S, const uint4& a, const uint4& b) __attribute__((always_inline)) {
        const uint32_t x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        if (8 * S + 8 <= wlim) {                               // uniform
#pragma unroll
            for (int g = 0; g < 8; ++g) acc = xam(acc, x[g], bits[8 * S + g]);
        } else {                                               // the key row ends inside this super-group
#pragma unroll
            for (int g = 0; g < 8; ++g)
                if (8 * S + g < wlim) acc = xam(acc, x[g], bits[8 * S + g]);
        }
    };
    auto at = [&](uint64_t S) { return &dbs[((S * ncols + col) * 256 + n) * 2]; };
    uint64_t S = s0;
    for (; S + 1 < s1; S += 2) {
        const uint4 a0 = at(S)[0], b0 = at(S)[1];
        const uint4 a1 = at(S + 1)[0], b1 = at(S + 1)[1];
        fold(S, a0, b0);
        fold(S + 1, a1, b1);
    }
    if (S < s1) fold(S, at(S)[0], at(S)[1]);
    const uint64_t m = __builtin_amdgcn_ballot_w64((__builtin_popcount(acc) & 1) != 0);
    if (l < 2)
        parts[(uint64_t)blockIdx.x * (8u * gridDim.y) + 8 * blockIdx.y + 2 * w + l] = l ? (uint32_t)(m >> 32) : (uint32_t)m;
}

uint64_t pir_sliced_bytes(uint64_t nrec, uint64_t rec_bytes) { return (nrec + 255) / 256 * 256 * rec_bytes; }

hipError_t launch_slice_db(const uint8_t* db, uint64_t nrec, uint64_t rec_bytes, uint8_t* dbs, hipStream_t st) {
    if (rec_bytes == 0 || rec_bytes % 32 != 0 || rec_bytes > kFoldMaxRecBytes) return hipErrorInvalidValue;
    const uint64_t nsg = (nrec + 255) / 256, C = rec_bytes / 32;
    if (nsg == 0) return hipSuccess;
    // One workgroup per (super-group, column), in launches of at most 2^30.
    const uint64_t per = (1ull << 30) / C;
    for (uint64_t S0 = 0; S0 < nsg; S0 += per) {
        const uint64_t n = nsg - S0 < per ? nsg - S0 : per;
        hipLaunchKernelGGL(k_slice_db, dim3((uint32_t)(n * C)), dim3(256), 0, st,
                           reinterpret_cast<const uint4*>(db + S0 * 256 * rec_bytes), nrec - S0 * 256, (uint32_t)C,
                           reinterpret_cast<uint32_t*>(dbs + S0 * 256 * rec_bytes));
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

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
constexpr uint32_t kUpdSeqMin = 16;   // consecutive updates of a batch from which the ballot form is cheaper
__global__ __launch_bounds__(256, 8) void k_update_sliced(uint4* __restrict__ dbs, uint64_t nrec, uint32_t ncols,
                                                        const uint64_t* __restrict__ idx,
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
    const uint2* recs2 = reinterpret_cast<const uint2*>(recs);
    while (heads) {
        const uint32_t u = (uint32_t)__builtin_ctzll(heads);
        heads &= heads - 1;
        uint64_t i = i0 + u;
        const uint64_t S = idx[i] >> 8;
        uint4* row = &dbs[((S * ncols + c) * 256 + t) * 2];
        const uint4 a = row[0], b = row[1];
        uint32_t x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        for (;;) {
            // Entries i .. i + 63, one per lane: how many continue the run,
            // and this wave's two words of each of their records.
            const uint64_t il = i + l;
            uint64_t v = ~0ull;
            if (il < n) v = idx[il];
            const bool in = v < nrec && (v >> 8) == S;
            uint2 wv = make_uint2(0, 0);
            if (in) wv = recs2[(il * ncols + c) * 4 + w];
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
        row[0] = make_uint4(x[0], x[1], x[2], x[3]);
        row[1] = make_uint4(x[4], x[5], x[6], x[7]);
    }
}

// Record idx[i] of the sliced DB in row-major form (zeros for idx[i] >= nrec):
// one thread per output word (i, c, wd), bit b of it = bit j of
// dbs[S][c][32 wd + b][g].  Not a hot path: 32 loads of 4 bytes per word.
__global__ __launch_bounds__(256) void k_gather_sliced(const uint32_t* __restrict__ dbs, uint64_t nrec, uint32_t ncols,
                                                        const uint64_t* __restrict__ idx, uint64_t nwords,
                                                        uint32_t* __restrict__ out) {
    const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (tid >= nwords) return;
    const uint32_t wd = (uint32_t)(tid & 7);
    const uint64_t ic = tid >> 3;
    const uint32_t c = (uint32_t)(ic % ncols);
    const uint64_t r = idx[ic / ncols];
    uint32_t o = 0;
    if (r < nrec) {
        const uint64_t S = r >> 8;
        const uint32_t g = ((uint32_t)r & 255u) >> 5, j = (uint32_t)r & 31u;
        const uint32_t* p = dbs + ((S * ncols + c) * 256 + 32 * wd) * 8 + g;
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

static bool rec_bytes_ok(uint64_t rec_bytes) {
    return rec_bytes != 0 && rec_bytes % 32 == 0 && rec_bytes <= kFoldMaxRecBytes;
}

hipError_t launch_update_sliced(uint8_t* dbs, uint64_t nrec, uint64_t rec_bytes, const uint64_t* idx,
                                const uint8_t* recs, uint64_t n, hipStream_t st) {
    if (!rec_bytes_ok(rec_bytes)) return hipErrorInvalidValue;
    if (n == 0 || nrec == 0) return hipSuccess;
    const uint64_t C = rec_bytes / 32, nsg = (nrec + 255) / 256;
    // n updates over nsg super-groups: runs of n / nsg updates at least on
    // average, so chunks of that many hold about one head or fewer each.
    uint32_t K = 1;
    while (K < 64 && 2ull * K <= n / nsg) K *= 2;
    // One workgroup per (chunk, column), in launches of at most 2^30
    // (chunks rounded up to a multiple of 8: the kernel's slot -> chunk map).
    const uint64_t per = ((1ull << 30) / C - 8) * K;    // updates per launch
    for (uint64_t i0 = 0; i0 < n; i0 += per) {
        const uint64_t m = n - i0 < per ? n - i0 : per;
        const uint64_t nchunks = (m + K - 1) / K;
        hipLaunchKernelGGL(k_update_sliced, dim3((uint32_t)((nchunks + 7) / 8 * 8 * C)), dim3(256), 0, st,
                           reinterpret_cast<uint4*>(dbs), nrec, (uint32_t)C, idx,
                           reinterpret_cast<const uint32_t*>(recs), n, i0, K, (uint32_t)nchunks);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

// n records of per_rec threads each, in launches of at most 2^30 workgroups
// of 256 threads over whole records: fn(first record, records, threads).
template <class F>
static hipError_t for_record_chunks(uint64_t n, uint64_t per_rec, F fn) {
    const uint64_t per = (1ull << 38) / per_rec;         // records per launch: <= 2^38 threads
    for (uint64_t i0 = 0; i0 < n; i0 += per) {
        const uint64_t m = n - i0 < per ? n - i0 : per;
        fn(i0, m, m * per_rec);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_gather_sliced(const uint8_t* dbs, uint64_t nrec, uint64_t rec_bytes, const uint64_t* idx, uint64_t n,
                                uint8_t* out, hipStream_t st) {
    if (!rec_bytes_ok(rec_bytes)) return hipErrorInvalidValue;
    const uint64_t C = rec_bytes / 32;
    return for_record_chunks(n, 8 * C, [&](uint64_t i0, uint64_t, uint64_t threads) {
        hipLaunchKernelGGL(k_gather_sliced, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, st,
                           reinterpret_cast<const uint32_t*>(dbs), nrec, (uint32_t)C, idx + i0, threads,
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
constexpr int kScatterSB = 4;                        // super-groups per staging round
constexpr int kScatterKT = (int)dpfh::kScatterKeyTile;
static_assert(dpfh::kScatterMaxCols == 4, "k_scatter_sliced is instantiated for 1 .. 4 columns");
static_assert(dpfh::kScatterMaxBlocks == kFoldMaxBlocks && dpfh::kScatterMaxSg == kFoldMaxSgPerBlock,
              "the scatter plan's defaults are set_fold_limits' defaults");

// The bits of selection word ww (records 32 ww ..) that are records below nrec.
__device__ __forceinline__ uint32_t scatter_live(uint64_t ww, uint64_t nrec) {
    const uint64_t r0 = ww * 32;
    return nrec >= r0 + 32 ? ~0u : nrec <= r0 ? 0u : (1u << (uint32_t)(nrec - r0)) - 1u;
}

template <int CG>
__global__ __launch_bounds__(256) void k_scatter_sliced(const uint32_t* __restrict__ bits, uint64_t wpk,
                                                        uint4* __restrict__ dbs, uint64_t nrec, uint64_t nsg,
                                                        uint32_t ncols, const uint4* __restrict__ msgs, uint32_t rec_u4,
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
        for (uint32_t i = t; i < kt * 2 * CG; i += 256) {
            const uint32_t k = i / (2 * CG), q = 2 * c0 + i % (2 * CG);
            mst[i] = q < 2 * ncols ? msgs[(uint64_t)k * rec_u4 + q] : make_uint4(0, 0, 0, 0);
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

    auto tile = [&](uint64_t S, int ci) { return &dbs[((S * ncols + c0 + ci) * 256) * 2 + t]; };
    auto load = [&](uint64_t S, uint4 (&x)[CG][2]) __attribute__((always_inline)) {
#pragma unroll
        for (int ci = 0; ci < CG; ++ci)
            if (c0 + ci < ncols) {
                x[ci][0] = tile(S, ci)[0];
                x[ci][1] = tile(S, ci)[256];
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
            for (int ci = 0; ci < CG; ++ci)
                if (c0 + ci < ncols) {
                    tile(S, ci)[0] = cur[ci][0];
                    tile(S, ci)[256] = cur[ci][1];
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
    for (uint64_t tile = 0; tile < p.key_tiles(); ++tile) {
        const dpfh::ScatterUnit k = p.unit(tile, 0);
        for (uint64_t l = 0; l < p.launches(); ++l) {
            hipLaunchKernelGGL(k_scatter_sliced<CG>, dim3((uint32_t)p.blocks(l)), dim3(256), 0, st, bits + k.k0 * wpk,
                               wpk, reinterpret_cast<uint4*>(dbs), nrec, p.nsg, p.C,
                               reinterpret_cast<const uint4*>(msgs + k.k0 * rec_bytes), (uint32_t)(rec_bytes / 16),
                               (uint32_t)(k.k1 - k.k0), p.run, p.ncg, p.first(l));
            if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

hipError_t launch_scatter_sliced(const uint32_t* bits, uint64_t words_per_key, uint8_t* dbs, uint64_t nrec,
                                 uint64_t rec_bytes, const uint8_t* msgs, uint64_t nkeys, hipStream_t st) {
    if (!rec_bytes_ok(rec_bytes) || words_per_key % 4 != 0 || nrec > words_per_key * 32) return hipErrorInvalidValue;
    if (nkeys == 0 || nrec == 0) return hipSuccess;
    const dpfh::ScatterPlan p =
        dpfh::plan_scatter(nrec, (uint32_t)(rec_bytes / 32), nkeys, (uint32_t)cu_count_fold(),
                           g_fold_blocks.load(std::memory_order_relaxed), fold_max_sg());
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

namespace {
// The DB pieces of a matrix-core fold over at least this many DB bytes are
// loaded nontemporal.  r05 (tools/archive/r05_nt.sh, profiles/r05/fold_nt/, B = 64,
// fold us, nontemporal vs default): 2^24 x 32 B (512 MiB, twice the chip's
// last-level cache) 123-125 vs 135-138, and B = 16 95 vs 105-107; 2^23 66-69
// vs 67-74; but 2^22 39-40 vs 35-36 and 2^21 (an N = 8 rank) 25.5 vs 24.7:
// slices that stay cached between batches lose.  DPF_FOLD_NT_MIN overrides.
constexpr uint64_t kFoldNtMinBytes = 256ull << 20;
uint64_t fold_nt_min_bytes() {
    static const uint64_t v = [] {
        const char* e = getenv("DPF_FOLD_NT_MIN");
        return e && *e ? strtoull(e, nullptr, 0) : kFoldNtMinBytes;
    }();
    return v;
}

// Workgroups per CU of a matrix-core fold launch: resident workgroups only
// (one round), each a contiguous run of whole staged blocks.  (A fixed 4
// workgroups per CU left 1/4 - 3/4 of them for a second round at 3 or 1
// resident per CU.)  occ: the shape's occupancy limit; C > 1 launches that.
// 32-byte records (C = 1): two workgroups per CU instead of the occupancy
// limit (3 at 33-64 keys) for cached DB slices and for the one-key-tile
// shape: fewer partials to combine and less per-workgroup overhead (r05,
// tools/archive/r05_fpercu.sh, profiles/r05/fold_blocks/, medians of 5:
// 2^21 x 32 B 22.6 vs 24.7 us, 2^22 34.8 vs 36.0, B = 16 at 2^24 91.9 vs
// 96.6, B = 32 96.3 vs 99.8; but B = 64 at 2^23 / 2^24 67.9 / 130.7 vs
// 67.0 / 125.9).  One per CU for 33-64 keys over a slice of <= 64 MiB (the
// PIR rank at N = 8): rank step 0.0741-0.0750 vs 0.0742-0.0759 ms, lower in
// 5 of 6 interleaved pairs; at N = 4 (128 MiB) the pairs split 3 / 3 and the
// fold alone was slower (37.6 vs 33.9 us), so it keeps 2
// (tools/archive/r05_fpercu1.sh, profiles/r05/fold_blocks/per_cu1_*.txt).
// DPF_FOLD_PER_CU=<n> (A/B runs, C = 1): this many, at most occ.
uint64_t fold_per_cu(uint32_t C, int MT, bool ntdb, uint64_t slice_bytes, int occ) {
    if (C > 1) return (uint64_t)occ;
    static const int env_pcu = [] {
        const char* e = getenv("DPF_FOLD_PER_CU");
        return e && atoi(e) > 0 ? atoi(e) : 0;
    }();
    if (env_pcu > 0) return (uint64_t)(env_pcu < occ ? env_pcu : occ);
    if (slice_bytes <= (64ull << 20) && MT == 2) return 1;
    return (!ntdb || MT == 1) && occ > 2 ? 2 : (uint64_t)occ;
}

// One key group (<= 32 MT keys) over the sliced DB of C columns: launches of
// x * y <= cap workgroups (x super-group runs, y column groups), in passes of
// at most x * msg super-groups; each workgroup folds <= msg super-groups
// (fp32-exact counts, see k_fold_mfma) and each fold launch is followed by a
// k_xor_parts launch that XORs its partials into ans.
template <int MT, int NT, int SG, int CG, int WPE>
hipError_t launch_mfma(const uint32_t* bits, uint64_t wpk, const uint8_t* dbs, uint64_t nsg, uint32_t C, uint32_t nk,
                       uint32_t* parts, uint32_t* ans, uint32_t* zero, uint64_t zero_words, hipStream_t st) {
    constexpr int NW = 8 / NT * CG;
    static_assert(32 * MT * CG * 32 <= (int)kFoldPartBytes, "a workgroup's partial fits its 16 KiB");
    static int occ = [] {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_fold_mfma<MT, NT, SG, CG, false, WPE>, 64 * NW, 0) !=
                hipSuccess || n < 1)
            n = 1;
        return n;
    }();
    const uint64_t cap = g_fold_blocks.load(std::memory_order_relaxed);
    const uint64_t msg = (uint64_t)fold_max_sg() / SG * SG > 0 ? (uint64_t)fold_max_sg() / SG * SG : SG;
    const uint64_t db_bytes = nsg * 256 * 32 * C;
    const bool ntdb = db_bytes >= fold_nt_min_bytes();
    const uint64_t ncg = C / CG;
    const uint64_t gy_max = ncg < cap ? ncg : cap;
    const uint64_t resident = (uint64_t)cu_count_fold() * fold_per_cu(C, MT, ntdb, db_bytes, occ);
    for (uint64_t g0 = 0; g0 < ncg; g0 += gy_max) {
        const uint64_t gy = ncg - g0 < gy_max ? ncg - g0 : gy_max;
        const uint64_t xcap = cap / gy;                          // >= 1
        const uint64_t per_pass = xcap * msg;
        for (uint64_t S0 = 0; S0 < nsg; S0 += per_pass) {
            const uint64_t n = nsg - S0 < per_pass ? nsg - S0 : per_pass;
            uint64_t want = (n + msg - 1) / msg;                 // none folds more than msg super-groups
            if (want < resident / gy) want = resident / gy;
            if (want < 1) want = 1;
            uint64_t blocks, spb;
            split_chunks(n, want, SG, blocks, spb, xcap);
            if (spb > msg || blocks * gy > cap) return hipErrorInvalidValue;
            const uint32_t* b = bits + S0 * 8;
            const uint64_t wlim = wpk > S0 * 8 ? wpk - S0 * 8 : 0;
            const uint4* d = reinterpret_cast<const uint4*>(dbs + S0 * 256 * 32 * C);
            const bool first = g0 == 0 && S0 == 0;
            uint32_t* z = first ? zero : nullptr;
            const uint64_t zw = first ? zero_words : 0;
            const dim3 grid((uint32_t)blocks, (uint32_t)gy);
            if (ntdb)
                hipLaunchKernelGGL((k_fold_mfma<MT, NT, SG, CG, true, WPE>), grid, dim3(64 * NW), 0, st, b, wpk, d, n,
                                   nk, spb, parts, z, zw, wlim, C, (uint32_t)g0);
            else
                hipLaunchKernelGGL((k_fold_mfma<MT, NT, SG, CG, false, WPE>), grid, dim3(64 * NW), 0, st, b, wpk, d, n,
                                   nk, spb, parts, z, zw, wlim, C, (uint32_t)g0);
            if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
            if (hipError_t e = launch_xor_parts(parts, blocks, nk, 32u * MT, (uint32_t)(8 * CG * gy), ans, 8ull * C,
                                                (uint32_t)(8 * CG * g0), st);
                e != hipSuccess)
                return e;
        }
    }
    return hipSuccess;
}

// One key over the sliced DB (k_fold_sliced_direct): x * y <= cap.
hipError_t launch_sliced_direct(const uint32_t* bits, uint64_t wpk, const uint8_t* dbs, uint64_t nsg, uint32_t C,
                                uint32_t* parts, uint32_t* ans, hipStream_t st) {
    const uint64_t cap = g_fold_blocks.load(std::memory_order_relaxed);
    // parts[x][8 y words] of a launch: x * y * 32 bytes, far inside the partials area.
    const uint64_t gy_max = C < cap ? C : cap;
    for (uint64_t c0 = 0; c0 < C; c0 += gy_max) {
        const uint64_t gy = C - c0 < gy_max ? C - c0 : gy_max;
        uint64_t want = (uint64_t)cu_count_fold() * 8 / gy;
        if (want < 1) want = 1;
        uint64_t blocks, spb;
        split_chunks(nsg, want, 2, blocks, spb, cap / gy);
        if (blocks * gy > cap) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_fold_sliced_direct, dim3((uint32_t)blocks, (uint32_t)gy), dim3(256), 0, st, bits,
                           reinterpret_cast<const uint4*>(dbs), nsg, spb, parts, c0 == 0 ? ans : nullptr,
                           c0 == 0 ? 8ull * C : 0ull, wpk, C, (uint32_t)c0);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        if (hipError_t e = launch_xor_parts(parts, blocks, 1u, 1u, (uint32_t)(8 * gy), ans, 8ull * C, (uint32_t)(8 * c0), st);
            e != hipSuccess)
            return e;
    }
    return hipSuccess;
}
}  // namespace

hipError_t launch_pir_fold_sliced(const uint32_t* bits, uint64_t words_per_key, const uint8_t* dbs, uint64_t nrec,
                                  uint64_t rec_bytes, uint32_t nkeys, uint32_t* ans, uint32_t* parts, hipStream_t st) {
    if (rec_bytes == 0 || rec_bytes % 32 != 0 || rec_bytes > kFoldMaxRecBytes) return hipErrorInvalidValue;
    if (nkeys == 0) return hipSuccess;
    if (nrec == 0) return hipMemsetAsync(ans, 0, (size_t)nkeys * rec_bytes, st);
    if (words_per_key % 4 != 0 || words_per_key * 32 < nrec) return hipErrorInvalidValue;
    const uint64_t nsg = (nrec + 255) / 256;
    const uint32_t C = (uint32_t)(rec_bytes / 32);
    if (nkeys == 1) return launch_sliced_direct(bits, words_per_key, dbs, nsg, C, parts, ans, st);   // popcount fold, no MFMA
    // Columns per workgroup: the largest of 4, 2, 1 that divides C, capped
    // per tile shape below.  DPF_FOLD_WIDE_CG=<1|2|4> (measurement) caps it.
    static const int cg_env = [] {
        const char* e = getenv("DPF_FOLD_WIDE_CG");
        return e && atoi(e) > 0 ? atoi(e) : 4;
    }();
    int cg = C % 4 == 0 ? 4 : C % 2 == 0 ? 2 : 1;
    if (cg > cg_env) cg = cg_env >= 2 ? 2 : 1;
    for (uint32_t k0 = 0; k0 < nkeys; k0 += 256) {
        const uint32_t nk = nkeys - k0 < 256 ? nkeys - k0 : 256;
        const uint32_t* b = bits + (uint64_t)k0 * words_per_key;
        uint32_t* zero = k0 == 0 ? ans : nullptr;
        const uint64_t zw = k0 == 0 ? (uint64_t)nkeys * 8 * C : 0;
        uint32_t* a = ans + (uint64_t)k0 * 8 * C;
        hipError_t e;
#define DPF_MW(MT_, NT_, SG_, CG_, WPE_) \
    launch_mfma<MT_, NT_, SG_, CG_, WPE_>(b, words_per_key, dbs, nsg, C, nk, parts, a, zero, zw, st)
        // Tile shape per key count (32 keys per tile): MT key tiles x NT bit
        // tiles per wave.  A column group of CG columns is 4 CG waves, so
        // the shape has 512 / CG registers (less where two workgroups share
        // a CU): the staged blocks shrink (SG) until nothing spills, and CG
        // stops where that no longer works (register counts per
        // instantiation: DESIGN §4.4).  32-byte records take the CG = 1 shapes.
        if (nk <= 32) e = cg == 4 ? DPF_MW(1, 2, 2, 4, 4) : cg == 2 ? DPF_MW(1, 2, 2, 2, 4) : DPF_MW(1, 2, 4, 1, 2);
        else if (nk <= 64) e = DPF_MW(2, 2, 2, 1, 2);   // CG = 2 (<2,2,4,2>, 2 waves per SIMD) measured no faster
        else if (nk <= 128) e = cg >= 2 ? DPF_MW(4, 2, 2, 2, 2) : DPF_MW(4, 2, 4, 1, 1);
        else e = DPF_MW(8, 2, 4, 1, 1);
#undef DPF_MW
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

FoldPlan plan_fold(uint64_t rec_bytes, uint32_t nkeys) {
    FoldPlan p{};
    const uint64_t c = rec_bytes / 32;
    p.cols = (c == 1 || c == 2 || c == 4 || c == 8) ? (uint32_t)c : 1;
    p.col_passes = p.cols == c ? 1 : (uint32_t)c;
    // Measured (tools/fold_bench, 2^24 x 32 B): direct is HBM-bound to 4 keys
    // (98 -> 101 us) but slower than Four-Russians from 8 (150 vs ~140 us);
    // wider records favour it longer (64 B, 16 keys: 69 us).
    p.direct = nkeys <= 4 || (p.cols >= 2 && nkeys <= (uint32_t)kDirectMaxKeys);
    const uint32_t kw_cap = p.cols >= 8 ? 1 : p.cols == 4 ? 2 : 4;
    uint32_t kw = 1;
    if (!p.direct)
        while (kw < kw_cap && 64u * kw < nkeys) kw *= 2;
    p.keys_per_pass = p.direct ? (uint32_t)kDirectMaxKeys : 64 * kw;
    p.kw = p.direct ? 0 : kw;
    return p;
}

hipError_t launch_pir_fold(const uint32_t* bits, uint64_t words_per_key, const uint8_t* db, uint64_t nrec,
                           uint64_t rec_bytes, uint32_t nkeys, uint32_t* ans, uint32_t* parts, hipStream_t st) {
    if (nkeys == 0) return hipSuccess;
    if (rec_bytes == 0 || rec_bytes % 32 != 0) return hipErrorInvalidValue;
    if (nrec == 0) return hipMemsetAsync(ans, 0, (size_t)nkeys * rec_bytes, st);
    const FoldPlan p = plan_fold(rec_bytes, nkeys);
    const uint64_t rec_u4 = rec_bytes / 16, ans_words = rec_bytes / 4;
    for (uint32_t col = 0; col < p.col_passes; ++col)
        for (uint32_t k0 = 0; k0 < nkeys; k0 += p.keys_per_pass) {
            const uint32_t nk = nkeys - k0 < p.keys_per_pass ? nkeys - k0 : p.keys_per_pass;
            FoldArgs a{bits + (uint64_t)k0 * words_per_key, words_per_key, reinterpret_cast<const uint4*>(db),
                       nrec,  rec_u4, col, nk, parts, nullptr, 0};
            if (col == 0 && k0 == 0) {
                a.zero = ans;
                a.zero_words = (uint64_t)nkeys * ans_words;
            }
            uint32_t* an = ans + (uint64_t)k0 * ans_words;
            hipError_t e;
            switch (p.cols) {
                case 2: e = fold_pass<2>(a, p.direct, (int)p.kw, an, ans_words, 0, st); break;
                case 4: e = fold_pass<4>(a, p.direct, (int)p.kw, an, ans_words, 0, st); break;
                case 8: e = fold_pass<8>(a, p.direct, (int)p.kw, an, ans_words, 0, st); break;
                default: e = fold_pass<1>(a, p.direct, (int)p.kw, an, ans_words, 8 * col, st); break;
            }
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

}  // namespace dpfk
