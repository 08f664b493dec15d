// pir_kernels.hpp — launchers for the XOR fold (pir_fold_rows.hip,
// pir_fold_sliced.hip; shared parts in pir_kernels.hip): the PIR answer and
// the general-payload streaming consumer of EvalFull output; for the resident
// DB's in-place updates; and for the fold's dual, the private write (messages
// XORed into the selected records), both in pir_db_ops.hip.  How each launcher
// sizes its launches: pir_fold_plan.hpp; the grouped ones: pir_group_plan.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pir_fold_plan.hpp"
#include "pir_group_fold_plan.hpp"
#include "pir_group_scatter_plan.hpp"

namespace dpfk {

// How launch_pir_fold covers (rec_bytes, nkeys).
using dpfh::FoldPlan;
using dpfh::plan_fold;

// ans[k][0 .. rec_bytes) = XOR of the records db[i] (rec_bytes each, a
// multiple of 32; i < nrec) whose bit i is set in bits[k * words_per_key
// ...] (EvalFull's LSB-first layout); zero when nrec == 0.  The first fold
// launch clears ans itself (no separate memset).  `parts` is scratch of
// pir_fold_parts_bytes() (per-workgroup partial answers).  bits, db 16-byte
// aligned; words_per_key a multiple of 4 covering nrec bits.
uint64_t pir_fold_parts_bytes();
// `bytes` (a multiple of 4, p 4-byte aligned) of zeros on st: how every
// launcher and _dev entry clears answers (a kernel, so that a stream capture
// records no memset node; pir_kernels.hip, DESIGN.md §4.4 "Clearing answers").
hipError_t launch_zero(void* p, uint64_t bytes, hipStream_t st);
hipError_t launch_pir_fold(const uint32_t* bits, uint64_t words_per_key, const uint8_t* db, uint64_t nrec,
                           uint64_t rec_bytes, uint32_t nkeys, uint32_t* ans, uint32_t* parts, hipStream_t st);

// The matrix-core fold (k_fold_mfma; k_fold_sliced_direct for one key): the
// same answers from the DB in its bit-sliced layout, for records of
// rec_bytes = 32 C bytes (a positive multiple of 32, at most
// kFoldMaxRecBytes):
//   dbs[S][c][n][g] (u32), S = super-group of 256 records, c < C 32-byte
//   column, n < 256 bit position of the column, g < 8 group of 32 records
// (32-byte records: dbs[S][n][g]), pir_sliced_bytes(nrec, rec_bytes) bytes,
// built once by launch_slice_db from the row-major DB.  launch_slice_db of
// records [256 S0, ...) into dbs + S0 * 256 * rec_bytes writes what slicing
// the whole DB writes there.  Same bits / parts / ans contract as
// launch_pir_fold; ans is [nkeys][rec_bytes].
// The sliced launchers here and below take every rec_bytes that is a positive
// multiple of 4 (dpfh::rec_bytes_any_ok): as rows, dbs[S][p][g] with
// p < 8 * rec_bytes the record's bit position, a super-group 8 * rec_bytes
// rows with no padding behind it; a record is rec_bytes / 4 bit tiles of 32
// rows in ceil(rec_bytes / 32) columns, the last one possibly short
// (pir_fold_plan.hpp).  For multiples of 32 that is the layout above, and
// the kernels run their whole-column instantiations.  Row-major records,
// messages and answers are [n][rec_bytes], tightly packed: only their base
// pointers are 16-byte aligned.  The C ABI's _wide entry points keep the
// multiple-of-32 rule in front of these launchers; the _any ones do not.
using dpfh::kFoldMaxRecBytes;   // 32768
uint64_t pir_sliced_bytes(uint64_t nrec, uint64_t rec_bytes);
hipError_t launch_slice_db(const uint8_t* db, uint64_t nrec, uint64_t rec_bytes, uint8_t* dbs, hipStream_t st);
hipError_t launch_pir_fold_sliced(const uint32_t* bits, uint64_t words_per_key, const uint8_t* dbs, uint64_t nrec,
                                  uint64_t rec_bytes, uint32_t nkeys, uint32_t* ans, uint32_t* parts, hipStream_t st);

// The grouped fold (k_fold_grouped, pir_fold_grouped.hip): dbs is the sliced
// layout (any width) of ngroups groups of nrec records, group g at flat record
// g * dpfh::group_stride(nrec) with zero records behind its nrec
// (pir_group_plan.hpp); bits is [ngroups * keys_per_group][words_per_key], row
// g * keys_per_group + j selecting within group g (bit i = record i of the
// group), and ans [ngroups * keys_per_group][rec_bytes] in the same order,
// overwritten; zeros when nrec == 0.  The keys of a group share each read of
// its tiles, up to 4 per pass; from dpfh::kGroupFoldMfmaMinKeys keys per group
// (the route rule of pir_group_fold_plan.hpp) up to 256 per pass on the matrix
// cores (k_fold_grouped_mfma, pir_fold_grouped_mfma.hip).  words_per_key a
// multiple of 4 covering nrec bits; ngroups * keys_per_group fits 32 bits.
// `parts` is not written on either route: runs of one group combine by atomic
// XOR into answers cleared earlier in stream order.  bits, dbs 16-byte, ans
// 4-byte aligned.
hipError_t launch_pir_fold_grouped(const uint32_t* bits, uint64_t words_per_key, const uint8_t* dbs, uint64_t ngroups,
                                   uint32_t keys_per_group, uint64_t nrec, uint64_t rec_bytes, uint32_t* ans,
                                   uint32_t* parts, hipStream_t st);
// The plan that call walks: under the current limits, on `cus` CUs (0: the
// calling thread's budget), its route after the DPF_GROUP_FOLD_ROUTE knob.
dpfh::GroupFoldKeysPlan fold_grouped_plan(uint64_t ngroups, uint32_t keys_per_group, uint64_t nrec, uint64_t rec_bytes,
                                          uint64_t cus);
// The launches of p's matrix-core route (p.gsg > 0, p.kpg > 0): the clear where
// p.atomic(), then every key tile's.  Same buffers as launch_pir_fold_grouped.
hipError_t launch_fold_grouped_mfma(const dpfh::GroupFoldKeysPlan& p, const uint32_t* bits, uint64_t words_per_key,
                                    const uint8_t* dbs, uint64_t rec_bytes, uint32_t* ans, hipStream_t st);

// Records of a resident DB changed and read back in place (k_update_sliced,
// k_gather_sliced).  Update: record idx[i] := recs[i * rec_bytes ..) for
// i < n, idx non-decreasing (of equal indices the last wins; unsorted input
// leaves the touched super-groups unspecified but stays inside the buffers),
// idx[i] >= nrec skipped; afterwards dbs is what launch_slice_db writes from
// the modified row-major DB.  Gather: out[i] = record idx[i] in row-major
// form, any order, zeros for idx[i] >= nrec.  No workspace, asynchronous on
// st.  idx 8-byte, dbs / recs / out 16-byte aligned.  The _rows forms do the
// same on a row-major DB [nrec][rec_bytes].
hipError_t launch_update_sliced(uint8_t* dbs, uint64_t nrec, uint64_t rec_bytes, const uint64_t* idx,
                                const uint8_t* recs, uint64_t n, hipStream_t st);
hipError_t launch_gather_sliced(const uint8_t* dbs, uint64_t nrec, uint64_t rec_bytes, const uint64_t* idx, uint64_t n,
                                uint8_t* out, hipStream_t st);
hipError_t launch_update_rows(uint8_t* db, uint64_t nrec, uint64_t rec_bytes, const uint64_t* idx, const uint8_t* recs,
                              uint64_t n, hipStream_t st);
hipError_t launch_gather_rows(const uint8_t* db, uint64_t nrec, uint64_t rec_bytes, const uint64_t* idx, uint64_t n,
                              uint8_t* out, hipStream_t st);

// The whole-DB read-out (pir_unslice.hip).  launch_unslice_db is the inverse
// of launch_slice_db: db [nrec][rec_bytes] row-major from the sliced layout of
// any width; exactly nrec rows are written, whatever the rows past nrec of the
// last super-group hold.  As for slicing, records [256 S0, ...) come from
// dbs + S0 * 256 * rec_bytes.  launch_xor_words: dst ^= src over `bytes` (a
// multiple of 16), the merge of two sliced buffers of one shape (or of plain
// rows).  No workspace, asynchronous on st; all pointers 16-byte aligned.
constexpr uint64_t kXorWordsMaxBlocks = 8192;   // grid-stride beyond: 8 workgroups for each of 4 SIMDs of 256 CUs
hipError_t launch_unslice_db(const uint8_t* dbs, uint64_t nrec, uint64_t rec_bytes, uint8_t* db, hipStream_t st);
hipError_t launch_xor_words(uint8_t* dst, const uint8_t* src, uint64_t bytes, hipStream_t st);

// Private writes, the dual of the fold (k_scatter_sliced; k_xor_scatter_rows
// on a row-major DB): record i ^= XOR over keys k < nkeys with bit i of
// bits[k * words_per_key ...] set of msgs[k * rec_bytes ..), for i < nrec.
// Selection bits at positions >= nrec are ignored, so the sliced layout's
// padding stays zero.  Keys go in tiles of dpfh::kScatterKeyTile, one pass
// over the DB each, planned by pir_scatter_plan.hpp under set_fold_limits'
// max_blocks (workgroups per launch) and max_sg (super-groups per workgroup).
// No workspace, no atomics, asynchronous on st.  bits, dbs / db and msgs
// 16-byte aligned; words_per_key a multiple of 4 covering nrec bits.
hipError_t launch_scatter_sliced(const uint32_t* bits, uint64_t words_per_key, uint8_t* dbs, uint64_t nrec,
                                 uint64_t rec_bytes, const uint8_t* msgs, uint64_t nkeys, hipStream_t st);
hipError_t launch_scatter_rows(const uint32_t* bits, uint64_t words_per_key, uint8_t* db, uint64_t nrec,
                               uint64_t rec_bytes, const uint8_t* msgs, uint64_t nkeys, hipStream_t st);

// The grouped private write, the dual of the grouped fold (k_scatter_grouped,
// pir_scatter_grouped.hip): dbs is the grouped layout above, bits and msgs are
// [ngroups * keys_per_group] rows in group order, and for i < nrec
//   group g, record i ^= XOR over k < keys_per_group with bit i of
//   bits[(g * keys_per_group + k) * words_per_key ...] set of
//   msgs[(g * keys_per_group + k) * rec_bytes ..).
// Bits at positions >= nrec are ignored, so the zero records behind every
// group's nrec stay zero; words past a row's end are not read.  Planned by
// plan_scatter_grouped (pir_group_scatter_plan.hpp; the fold's plan type,
// dpfh::GroupedPlan) under set_fold_limits' max_blocks and max_sg: key passes
// of 4 and a last one of 1 to 3 over one grid of all groups, or (the plan's route
// rule; few large groups with many keys) a loop of launch_scatter_sliced over
// each group's flat range.  No workspace, no atomics, asynchronous on st.
// bits, dbs and msgs 16-byte aligned; words_per_key a multiple of 4 covering
// nrec bits; ngroups * keys_per_group fits 32 bits.
hipError_t launch_scatter_grouped(const uint32_t* bits, uint64_t words_per_key, uint8_t* dbs, uint64_t ngroups,
                                  uint32_t keys_per_group, uint64_t nrec, uint64_t rec_bytes, const uint8_t* msgs,
                                  hipStream_t st);
// The plan that call walks: under the current limits, on `cus` CUs (0: the
// calling thread's budget), its route after the DPF_GROUP_SCATTER_ROUTE knob.
dpfh::GroupedPlan scatter_grouped_plan(uint64_t ngroups, uint32_t keys_per_group, uint64_t nrec, uint64_t rec_bytes,
                                       uint64_t cus);

// Tuning / test limits of the fold launches: at most max_blocks workgroups
// per launch (0 = the default, 1024), and at most max_sg super-groups per
// matrix-core fold workgroup (0 = the default and maximum, 2^15 = 2^23
// records, so its fp32 counts stay below 2^24); larger DBs fold in passes.
void set_fold_limits(uint32_t max_blocks, uint32_t max_sg);

// Fused PIR answer (k_pir_fused): the subtree EvalFull of keys [0, nkeys)
// from their expanded records (launch_unpack) and the matrix-core fold over
// the sliced DB in one launch; where pir_fused_ok() (<= 64 keys, 2^8 .. 2^10
// blocks of 256 leaf pairs in the subtree; any_size: from one block, for
// tests).  Same ans / parts contract.  Defined in pir_fused.hip, which only
// the experimental library links (make experimental): measured slower than
// the two launches.  The product library links
// experimental_none.cpp instead: pir_fused_ok() is false and the launcher
// refuses.
bool pir_fused_ok(uint64_t nkeys, uint32_t stop, uint32_t prefix_bits, bool any_size = false);
// Whether k_pir_fused is compiled into this library (the experimental build only).
bool pir_fused_built();
hipError_t launch_pir_fused(const uint32_t* ek, uint32_t nkeys, uint32_t stop, uint32_t prefix_bits, uint64_t prefix,
                            const uint8_t* dbs, uint64_t nrec, uint32_t* ans, uint32_t* parts, hipStream_t st);

}  // namespace dpfk
