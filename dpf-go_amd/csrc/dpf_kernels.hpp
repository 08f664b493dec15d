// dpf_kernels.hpp — launchers for the gfx950 DPF kernels (dpf_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eval_bits_plan.hpp"
#include "tree_plan.hpp"

namespace dpfk {

// Workgroup sizes, subtree depths and the frontier limit: tree_plan.hpp,
// with the launch plans that use them.
using dpfh::kBlock;
using dpfh::kTreeBlock;
using dpfh::kTreeBlockBig;
using dpfh::kTreeBlockMax;
using dpfh::kBigMinD;
using dpfh::kFeedbackMinD;
using dpfh::kTreeWaves;
using dpfh::kMaxD;
using dpfh::kMaxFrontierHbm;
using dpfh::kEvalPBlock;

// CU budget of the calling thread's launches (0: the whole device); see
// cu_count() in dpf_kernels.hip.
void set_cu_budget(int cus);
int cu_budget();
int cu_count();
// The process's measurement switches (DPF_SUBTREE_DEPTH, DPF_RAW_KEYS,
// DPF_EVAL_*) as the launch plans of tree_plan.hpp take them.
const dpfh::TreeKnobs& tree_knobs();

// Expanded-key words per key: (stop + 2) records of 8 u32.
inline uint64_t ek_words(uint32_t stop) { return ((uint64_t)stop + 2) * 8; }

// aes128MMO iterated `reps` times over nblocks (even) blocks, T-table back end.
hipError_t launch_mmo_tt(const uint8_t* in, uint8_t* out, uint64_t nblocks, uint32_t right, uint32_t reps,
                         hipStream_t st);

hipError_t launch_unpack(const uint8_t* keys, uint64_t key_len, uint64_t nkeys, uint32_t stop, uint32_t* ek,
                         hipStream_t st);

// EvalFull of the subtree rooted at depth `prefix_bits`, index `prefix`, of
// every key (prefix_bits = 0 -> whole domain).  Output per key: 2^(stop -
// prefix_bits) leaves of 16 B at out + key * out_stride.
hipError_t launch_evalfull(const uint32_t* ek, uint64_t nkeys, uint32_t stop, uint32_t prefix_bits,
                           uint64_t prefix, uint8_t* out, uint64_t out_stride, hipStream_t st);

// The same from the key bytes themselves ([nkeys][klen], the reference's
// layout, any alignment), no unpack launch: only where evalfull_raw_ok()
// (every wave owns one key).
bool evalfull_raw_ok(uint64_t nkeys, uint32_t stop, uint32_t prefix_bits);
hipError_t launch_evalfull_raw(const uint8_t* keys, uint64_t klen, uint64_t nkeys, uint32_t stop, uint32_t prefix_bits,
                               uint64_t prefix, uint8_t* out, uint64_t out_stride, hipStream_t st);

// Re-rooted keys (k_subkeys, subkeys.hip): key k walked prefix_bits levels
// along first_prefix + p, as a key of the subtree's domain, sub_len bytes at
// sub + (k * nprefix + p) * sub_len, for p < nprefix.  sub_len = klen - 18 *
// prefix_bits copies the key's tail unchanged (oracle.reroot_key); the
// canonical 33 + 18 * (stop - prefix_bits) takes the records below the node
// and the key's last 16 bytes.  Any alignment of keys and sub.
hipError_t launch_subkeys(const uint8_t* keys, uint64_t klen, uint64_t nkeys, uint32_t prefix_bits, uint64_t first_prefix,
                          uint64_t nprefix, uint8_t* sub, uint64_t sub_len, hipStream_t st);

// The 2^(depth - prefix_bits) nodes at level `depth` below prefix node
// (prefix_bits, prefix) of every key: seeds (16 B) at seeds + (key * stride
// + j) * 16 and t bytes at ts + key * stride + j.
hipError_t launch_nodes(const uint32_t* ek, uint64_t nkeys, uint32_t stop, uint32_t depth, uint32_t prefix_bits,
                        uint64_t prefix, uint8_t* seeds, uint8_t* ts, uint64_t stride, hipStream_t st);

// Batched Eval.  When a key has enough points to share the top of its tree
// (L = the deepest level with 2^(L+1) <= pts_per_key, used when L >= 4), the
// 2^L nodes at level L of every key are first
// computed into `frontier` (eval_frontier_bytes of it) and each query starts
// there; with frontier == nullptr (or too small) every walk starts at the root.
uint32_t eval_frontier_level(uint32_t stop, uint64_t pts_per_key);
// Batched Eval kernel choice: 1 = visited-node trie below the frontier.
int set_eval_trie(int on);   // returns the previous choice
int get_eval_trie();
// The trie kernel itself (k_eval_trie) is in eval_trie.hip, which only the
// experimental library links; the product library links
// experimental_none.cpp instead: not built, never ok, the launcher refuses.
// launch_eval takes it where eval_trie_ok() (one key per workgroup, <= 1024
// points per key, frontier level L): the queries of nkeys keys from the
// frontier (fseed, ft) computed by launch_eval.
bool eval_trie_built();
bool eval_trie_ok(uint32_t stop, uint32_t logN, uint64_t pts_per_key, uint32_t L);
hipError_t launch_eval_trie(const uint32_t* ek, uint32_t stop, uint32_t logN, const uint64_t* xs, uint64_t nkeys,
                            uint64_t pts_per_key, const uint4* fseed, const uint8_t* ft, uint32_t L, uint8_t* out,
                            hipStream_t st);
uint64_t eval_frontier_bytes(uint64_t nkeys, uint32_t stop, uint64_t pts_per_key);
hipError_t launch_eval(const uint32_t* ek, uint32_t stop, uint32_t logN, const uint64_t* xs, uint64_t nq,
                       uint64_t pts_per_key, uint8_t* out, void* frontier, uint64_t frontier_bytes,
                       hipStream_t st);
// Key k at the npts points of list k / keys_per_list of xs[][npts] (nkeys a
// multiple of keys_per_list; keys_per_list = nkeys: one shared list), as
// selection-bit rows bits[nkeys][bits_stride] (k_eval_bits; plan and layout:
// eval_bits_plan.hpp).
// bits_stride: a multiple of 16, at least dpfh::eval_bits_stride(npts).  The
// frontier is launch_eval's, sized eval_frontier_bytes(nkeys, stop, npts).
hipError_t launch_eval_bits(const uint32_t* ek, uint32_t stop, uint32_t logN, const uint64_t* xs, uint64_t nkeys,
                            uint64_t keys_per_list, uint64_t npts, uint8_t* bits, uint64_t bits_stride,
                            void* frontier, uint64_t frontier_bytes, hipStream_t st);

}  // namespace dpfk
