// pir_window_plan.hpp — a window of the domain as a batch of equal sub-keys
// (host-only, no HIP; tests/c/pir_window_plan_test.cpp).
//
// A node (s, t) of the GGM tree with the remaining correction words is a DPF
// key of the smaller domain (oracle.reroot_key).  So any run of leaf blocks
//   points [128 * first_block, 128 * (first_block + nblocks))
// of a 2^logN domain is covered by P consecutive aligned pieces of 2^s points,
// each the whole domain of one re-rooted key: k_subkeys (subkeys.hip) makes the
// P sub-keys of every key, and one tree launch over nkeys * P keys at logN' = s
// writes a key's pieces side by side, a row of P * 2^s / 8 bytes in which the
// window starts at byte row_offset.
//
// s = clamp(floor(log2(128 * nblocks)) - 4, 7, logN): between 16 and 32 pieces
// of window, so P <= 33, and what is evaluated outside the window is less than
// two pieces, at most 1/8 of the window (s unclamped).  Clamped at 7 (fewer
// than 16 blocks) a piece is one leaf block and nothing is evaluated outside.
//
//
// Route: where the smallest aligned subtree that holds the window has at most
// twice the window's points, the window is evaluated as that one subtree (the
// prefixed tree launch the dense forms run, no sub-keys; the window starts at
// row_offset of the subtree's bytes, and the fold ignores the rest).  Measured
// on one MI355X (profiles/pir_window/ab.jsonl): at 1.0, 1.6 and
// 2.0 times the window's points the one subtree beat the pieces at 1, 16 and
// 64 keys (the sub-key launch costs 15-30 us, and the tree kernel is slower a
// point over many keys of 2^16..2^20 points than over few of 2^21..2^24).  At
// 6.4 times the pieces won at 64 keys (104 against 154 us), tied at 16 and
// lost at one key (56 against 33 us); between 2 and 6.4 times nothing is
// measured.  The subtree's rows are nkeys * 2^(s-3) bytes, which has no bound
// in the window's size once the window straddles a high bit of the domain, so
// the rule keeps the factor at two for every key count.
//
// Also here: the balanced split of nrec records over n shards, which the
// sparse and the ranged PIR handles share (pir_update_plan.hpp).
#pragma once
#include <stdint.h>

namespace dpfh {

constexpr uint32_t kWindowSubtree = 0;   // the enclosing aligned subtree: the existing prefix path, no sub-keys
constexpr uint32_t kWindowPieces = 1;    // P re-rooted sub-keys per key

struct WindowPlan {
    uint32_t route = kWindowSubtree;
    uint32_t s = 0;              // log2 of a piece's points (>= 7 where logN >= 7)
    uint32_t prefix_bits = 0;    // logN - s: levels walked to a piece's root
    uint64_t first_prefix = 0;   // index of the first piece among the 2^prefix_bits
    uint64_t npieces = 0;        // P
    uint64_t piece_bytes = 0;    // 2^s / 8 (16 for logN < 7)
    uint64_t row_bytes = 0;      // P * piece_bytes
    uint64_t row_offset = 0;     // byte of the row at which the window starts, a multiple of 16
};

// Leaf blocks of a 2^logN domain (one below logN 7), logN <= 63.
inline uint64_t window_domain_blocks(uint32_t logN) { return logN <= 7 ? 1 : 1ull << (logN - 7); }

// A window the plan takes: logN <= 63, at least one block, inside the domain.
inline bool window_ok(uint32_t logN, uint64_t first_block, uint64_t nblocks) {
    if (logN > 63 || nblocks == 0) return false;
    const uint64_t dom = window_domain_blocks(logN);
    return first_block < dom && nblocks <= dom - first_block;
}

inline uint32_t floor_log2(uint64_t x) {   // x > 0
    uint32_t r = 0;
    while (x >>= 1) ++r;
    return r;
}

// log2 of the blocks of the smallest aligned subtree that holds blocks
// [first_block, first_block + nblocks), nblocks > 0.
inline uint32_t window_enclosing_log(uint64_t first_block, uint64_t nblocks) {
    const uint64_t diff = first_block ^ (first_block + nblocks - 1);
    return diff == 0 ? 0 : floor_log2(diff) + 1;
}

// Precondition: window_ok.  128 * (first_block + nblocks) <= 2^63: nothing overflows.
inline WindowPlan window_plan(uint32_t logN, uint64_t first_block, uint64_t nblocks) {
    WindowPlan w;
    if (logN < 7) {   // the domain is one leaf block
        w.piece_bytes = w.row_bytes = 16;
        w.npieces = 1;
        w.s = logN;
        return w;
    }
    const uint32_t m = floor_log2(nblocks) + 7;   // floor(log2(128 * nblocks))
    const uint32_t eb = window_enclosing_log(first_block, nblocks);
    if (eb <= 56 && ((uint64_t)1 << eb) <= 2 * nblocks) {   // (nblocks <= 2^56: no overflow)
        w.s = eb + 7;
        w.prefix_bits = logN - w.s;
        w.first_prefix = first_block >> eb;
        w.npieces = 1;
        w.piece_bytes = w.row_bytes = (uint64_t)16 << eb;
        w.row_offset = 16 * (first_block - (w.first_prefix << eb));
        return w;
    }
    w.route = kWindowPieces;
    w.s = m < 11 ? 7 : m - 4;   // (m - 4 < logN: the window fits the domain)
    w.prefix_bits = logN - w.s;
    const uint32_t bs = w.s - 7;   // log2 of a piece's blocks
    w.first_prefix = first_block >> bs;
    w.npieces = ((first_block + nblocks - 1) >> bs) - w.first_prefix + 1;
    w.piece_bytes = (uint64_t)16 << bs;
    w.row_bytes = w.npieces * w.piece_bytes;
    w.row_offset = 16 * (first_block - (w.first_prefix << bs));
    return w;
}

// Length of a piece's key: the deep key without the records of the levels
// walked (oracle.reroot_key); a long key's trailing bytes travel with it.
inline uint64_t window_sub_key_len(uint64_t key_len, uint32_t prefix_bits) { return key_len - 18ull * prefix_bits; }
// The same for a key of exactly 33 + 18 * (logN - 7) bytes, whatever the
// caller's key length: the composites' sub-keys (their workspace is sized
// without a key length) hold the records below the piece's root and the final
// CW, the caller's last 16 bytes.
inline uint64_t window_canonical_sub_key_len(const WindowPlan& w) { return 33 + 18ull * (w.s >= 7 ? w.s - 7 : 0); }

// Records [first_rec, first_rec + nrec) of the domain as a window of leaf
// blocks: first_rec a multiple of 128, nrec > 0, first_rec + nrec <= 2^logN.
inline bool window_records_ok(uint32_t logN, uint64_t first_rec, uint64_t nrec) {
    if (logN > 63 || first_rec % 128 != 0) return false;
    const uint64_t dom = 1ull << logN;
    return first_rec <= dom && nrec <= dom - first_rec;
}
inline uint64_t window_blocks_of(uint64_t nrec) { return nrec / 128 + (nrec % 128 != 0); }

// The balanced split of nrec records over nshards (> 0) shards: shard g holds
// the records from g * balanced_slice up, whole super-groups of 256 records,
// so every shard's sliced layout starts on one.
inline uint64_t balanced_slice(uint64_t nrec, uint64_t nshards) {
    const uint64_t sg = nrec / 256 + (nrec % 256 != 0);
    return (sg / nshards + (sg % nshards != 0)) * 256;
}

}  // namespace dpfh
