// capi_pir.hip — the device-resident PIR forms of the C ABI (include/dpf_hip.h):
// slicing a DB and un-slicing it again, the XOR fold and its dual the XOR scatter over caller-made
// selection bits, the composites that make the bits themselves (a subtree
// EvalFull, or for a sparse key set an Eval at the records' points), and the
// in-place update / gather of records.  All enqueue on the caller's stream.
//
// Every argument is checked before any device call, so a bad buffer is
// DPF_ERR_PARAM and not a GPU fault: each entry is a list of capi_common.hpp's
// rules in its own order of reports.  The launchers and their plans are in
// pir_kernels.hpp; no kernel is defined here.
#include <stdlib.h>
#include <string.h>

#include <atomic>

#include "capi_common.hpp"

using namespace dpfc;

namespace {

// PIR kernel over the sliced DB: the tree launch then the fold launch
// (DPF_PIR_SPLIT, the default: measured faster), or both in one launch
// where it applies (DPF_PIR_FUSED, k_pir_fused).  DPF_PIR_KERNEL=split|
// fused|fused-any sets the start value; in a build without k_pir_fused the
// environment value falls back to split, as dpf_set_pir_kernel refuses it.
std::atomic<int> g_pir_kernel{[] {
    const char* e = getenv("DPF_PIR_KERNEL");
    if (!dpfk::pir_fused_built()) return DPF_PIR_SPLIT;
    if (e && strcmp(e, "fused-any") == 0) return DPF_PIR_FUSED_ANY;
    if (e && e[0] == 'f') return DPF_PIR_FUSED;
    return DPF_PIR_SPLIT;
}()};

// The launcher of each operation by the DB's layout -- sliced: the bit-sliced
// layout (the matrix-core fold), else row-major records (the LDS fold).
auto fold_launcher(bool sliced) { return sliced ? dpfk::launch_pir_fold_sliced : dpfk::launch_pir_fold; }
auto scatter_launcher(bool sliced) { return sliced ? dpfk::launch_scatter_sliced : dpfk::launch_scatter_rows; }

// Device buffers of the PIR answer entry points: present when there is work
// for them, and aligned as the kernels access them (DB 16 B, answers and
// workspace as u32 words).
int check_answer_bufs(const void* d_keys, size_t nkeys, const void* d_db, uint64_t nrec, const void* d_ans,
                      const void* d_work) {
    if (nkeys > 0 && !(present(d_keys, d_ans, d_work) && (nrec == 0 || present(d_db)))) return null_buffer();
    if (!aligned(16, d_db, d_work) || !aligned(4, d_ans)) return misaligned_buffer();
    return DPF_OK;
}
// The same with the records' points, which the call reads where it reads the
// DB: every null buffer is reported before any misaligned one.
int check_answer_bufs(const void* d_keys, size_t nkeys, const void* d_db, const void* d_points, uint64_t nrec,
                      const void* d_ans, const void* d_work) {
    if (nkeys > 0 && nrec > 0 && !present(d_points)) return null_buffer();
    if (int rc = check_answer_bufs(d_keys, nkeys, d_db, nrec, d_ans, d_work)) return rc;
    return aligned(8, d_points) ? DPF_OK : misaligned_buffer();
}

// The PIR answer of the five *_dev entries below: the subtree EvalFull into
// the workspace (tree launch), then the fold over the DB of rec_bytes-wide
// records.  In front of that, 32-byte sliced records take both in one launch
// (k_pir_fused) where g_pir_kernel selects it.
int pir_answer(RecRule rule, bool sliced, int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
               uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_db, uint64_t nrec, size_t rec_bytes,
               uint8_t* d_ans, void* d_work, void* stream) {
    if (int rc = check_rec_bytes(rule, rec_bytes)) return rc;
    if (int rc = check_subtree(klen, logN, prefix_bits, prefix, nrec)) return rc;
    if (int rc = check_answer_bufs(d_keys, nkeys, d_db, nrec, d_ans, d_work)) return rc;
    DeviceGuard g(device);
    CuScope cus(stream);
    hipStream_t st = (hipStream_t)stream;
    if (nkeys == 0) return DPF_OK;
    if (nrec == 0) {
        HIP_TRY(dpfk::launch_zero(d_ans, nkeys * rec_bytes, st));
        return DPF_OK;
    }
    const uint32_t stop = stop_of(logN);
    const PirWs w = pir_ws(d_work, nkeys, stop, prefix_bits);
    const bool bs = want_bs();
    const int fz = g_pir_kernel.load(std::memory_order_relaxed);
    if (sliced && rec_bytes == 32 && !bs && fz != DPF_PIR_SPLIT &&
        dpfk::pir_fused_ok(nkeys, stop, prefix_bits, fz == DPF_PIR_FUSED_ANY)) {
        // One launch: tree + matrix-core fold (k_pir_fused) from the expanded records.
        forget_expanded(d_work);
        HIP_TRY(dpfk::launch_unpack(d_keys, klen, nkeys, stop, w.tree.ek, st));
        note_expanded(d_work, nkeys, stop, false);
        HIP_TRY(dpfk::launch_pir_fused(w.tree.ek, (uint32_t)nkeys, stop, prefix_bits, prefix, d_db, nrec,
                                       (uint32_t*)d_ans, w.parts, st));
        return DPF_OK;
    }
    HIP_TRY(tree_from_keys(d_keys, klen, nkeys, stop, prefix_bits, prefix, w.bits, w.per_key, d_work, st, bs));
    HIP_TRY(fold_launcher(sliced)((const uint32_t*)w.bits, w.per_key / 4, d_db, nrec, rec_bytes, (uint32_t)nkeys,
                                  (uint32_t*)d_ans, w.parts, st));
    return DPF_OK;
}

// The four fold entries behind their rec_bytes check: the shape and buffer
// checks in the order they report (bits_stride, nrec, alignment, null), then
// the fold on the caller's stream.  d_work's alignment is checked only for
// the sliced forms above 32 bytes (work16).
int xor_fold(bool sliced, bool work16, int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys,
             const uint8_t* d_db, uint64_t nrec, size_t rec_bytes, uint8_t* d_ans, void* d_work, void* stream) {
    if (int rc = check_sel_bits(bits_stride, nrec)) return rc;
    if (!aligned(16, d_bits, d_db) || !aligned(4, d_ans) || (work16 && !aligned(16, d_work))) return misaligned_buffer();
    if (nkeys > 0 && !(present(d_ans, d_work) && (nrec == 0 || present(d_bits, d_db)))) return null_buffer();
    DeviceGuard g(device);
    CuScope cus(stream);
    if (nkeys == 0) return DPF_OK;
    HIP_TRY(fold_launcher(sliced)((const uint32_t*)d_bits, bits_stride / 4, d_db, nrec, rec_bytes, (uint32_t)nkeys,
                                  (uint32_t*)d_ans, (uint32_t*)d_work, (hipStream_t)stream));
    return DPF_OK;
}

int pir_db_slice(RecRule rule, int device, const uint8_t* d_db, uint64_t nrec, size_t rec_bytes, uint8_t* d_dbs,
                 void* stream) {
    if (int rc = check_rec_bytes(rule, rec_bytes)) return rc;
    if (nrec > 0 && !present(d_db, d_dbs)) return null_buffer();
    if (!aligned(16, d_db, d_dbs)) return misaligned_buffer();
    DeviceGuard g(device);
    HIP_TRY(dpfk::launch_slice_db(d_db, nrec, rec_bytes, d_dbs, (hipStream_t)stream));
    return DPF_OK;
}

size_t sliced_size(RecRule rule, uint64_t nrec, size_t rec_bytes) {
    return rec_bytes_ok(rule, rec_bytes) ? std::max<size_t>(16, dpfk::pir_sliced_bytes(nrec, rec_bytes)) : 0;
}

// Records of the sliced DB changed (d_recs in) or read back (d_out) in place:
// every argument is checked before any device call.
int update_or_gather(RecRule rule, int device, uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes, const uint64_t* d_idx,
                     const uint8_t* d_recs, uint8_t* d_out, size_t n, void* stream) {
    const uint8_t* d_rows = d_recs ? d_recs : d_out;
    if (int rc = check_rec_bytes(rule, rec_bytes)) return rc;
    if (!present(d_dbs, d_idx, d_rows)) return null_buffer();
    if (!aligned(16, d_dbs, d_rows) || !aligned(8, d_idx)) return misaligned_buffer();
    if (n == 0) return DPF_OK;
    DeviceGuard g(device);
    if (d_recs)
        HIP_TRY(dpfk::launch_update_sliced(d_dbs, nrec, rec_bytes, d_idx, d_recs, n, (hipStream_t)stream));
    else
        HIP_TRY(dpfk::launch_gather_sliced(d_dbs, nrec, rec_bytes, d_idx, n, d_out, (hipStream_t)stream));
    return DPF_OK;
}

// Private writes (the dual of the fold): every argument is checked before
// any device call, in the order rec_bytes, bits_stride, nrec, null, alignment.
int xor_scatter(RecRule rule, bool sliced, int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys,
                const uint8_t* d_msgs, uint8_t* d_db, uint64_t nrec, size_t rec_bytes, void* stream) {
    if (int rc = check_rec_bytes(rule, rec_bytes)) return rc;
    if (int rc = check_sel_bits(bits_stride, nrec)) return rc;
    if (!present(d_bits, d_msgs, d_db)) return null_buffer();
    if (!aligned(16, d_bits, d_msgs, d_db)) return misaligned_buffer();
    if (nkeys == 0 || nrec == 0) return DPF_OK;
    DeviceGuard g(device);
    CuScope cus(stream);
    HIP_TRY(scatter_launcher(sliced)((const uint32_t*)d_bits, bits_stride / 4, d_db, nrec, rec_bytes, d_msgs, nkeys,
                                     (hipStream_t)stream));
    return DPF_OK;
}

// The private write of the three *_dev entries below: the subtree EvalFull
// into the workspace (pir_answer's layout, always the split path; the fold's
// partials stay unused), then the scatter of the messages over the DB.
int pir_write(RecRule rule, bool sliced, int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
              uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_msgs, uint8_t* d_db, uint64_t nrec,
              size_t rec_bytes, void* d_work, void* stream) {
    if (int rc = check_rec_bytes(rule, rec_bytes)) return rc;
    if (int rc = check_subtree(klen, logN, prefix_bits, prefix, nrec)) return rc;
    if (!present(d_keys, d_msgs, d_db, d_work)) return null_buffer();
    if (!aligned(16, d_msgs, d_db, d_work)) return misaligned_buffer();
    if (nkeys == 0 || nrec == 0) return DPF_OK;
    DeviceGuard g(device);
    CuScope cus(stream);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t stop = stop_of(logN);
    const PirWs w = pir_ws(d_work, nkeys, stop, prefix_bits);
    HIP_TRY(tree_from_keys(d_keys, klen, nkeys, stop, prefix_bits, prefix, w.bits, w.per_key, d_work, st, want_bs()));
    HIP_TRY(scatter_launcher(sliced)((const uint32_t*)w.bits, w.per_key / 4, d_db, nrec, rec_bytes, d_msgs, nkeys, st));
    return DPF_OK;
}

// The grouped slice (to_flat) / un-slice entries: width, the products, null,
// alignment, empty; then `launch` once where the groups have no padding (the
// row-major DB is the flat one), else per group at its row-major and flat
// strides (the zero records behind its nrec: zero-filled / not written).
template <class Launch>
int grouped_reslice(Launch launch, bool to_flat, const char* too_large, int device, const uint8_t* d_src, uint64_t ngroups,
                    uint64_t nrec, size_t rec_bytes, uint8_t* d_dst, void* stream) {
    if (int rc = check_rec_bytes(RecRule::Mul4, rec_bytes)) return rc;
    uint64_t bytes = 0;
    if (!dpfh::grouped_bytes(ngroups, nrec, rec_bytes, &bytes)) return fail(DPF_ERR_PARAM, too_large);
    if (bytes > 0 && !present(d_src, d_dst)) return null_buffer();
    if (!aligned(16, d_src, d_dst)) return misaligned_buffer();
    if (bytes == 0) return DPF_OK;
    DeviceGuard g(device);
    hipStream_t st = (hipStream_t)stream;
    const uint64_t gs = dpfh::group_stride(nrec);
    if (gs == nrec) {
        HIP_TRY(launch(d_src, ngroups * nrec, rec_bytes, d_dst, st));
        return DPF_OK;
    }
    const uint64_t from = (to_flat ? nrec : gs) * rec_bytes, to = (to_flat ? gs : nrec) * rec_bytes;
    for (uint64_t i = 0; i < ngroups; ++i) HIP_TRY(launch(d_src + i * from, nrec, rec_bytes, d_dst + i * to, st));
    return DPF_OK;
}

// The two grouped composites' front: group_ws (the write leaves the fold's
// scratch unused) and the tree pass of all keys into its selection rows.
int group_tree(const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN, void* d_work, hipStream_t st, GroupWs* w) {
    const uint32_t stop = stop_of(logN);
    *w = group_ws(d_work, nkeys, stop);
    HIP_TRY(tree_from_keys(d_keys, klen, nkeys, stop, 0, 0, w->bits, w->per_key, d_work, st, want_bs()));
    return DPF_OK;
}

}  // namespace

extern "C" {

size_t dpf_pir_workspace_size(size_t nkeys, uint32_t logN, uint32_t prefix_bits) {
    const uint32_t stop = stop_of(logN);
    return pir_ws(nullptr, nkeys, stop, std::min(prefix_bits, stop)).total;
}

size_t dpf_xor_fold_workspace_size(void) { return dpfk::pir_fold_parts_bytes(); }

int dpf_set_pir_kernel(int kernel) {
    if (kernel != DPF_PIR_SPLIT && kernel != DPF_PIR_FUSED && kernel != DPF_PIR_FUSED_ANY)
        return fail(DPF_ERR_PARAM, "dpf: unknown PIR kernel");
    if (kernel != DPF_PIR_SPLIT && !dpfk::pir_fused_built())
        return fail(DPF_ERR_PARAM, "dpf: the fused PIR kernel is not in this build (make -C dpf-go_amd experimental)");
    return g_pir_kernel.exchange(kernel);
}
int dpf_get_pir_kernel(void) { return g_pir_kernel.load(); }

int dpf_pir_kernel_for(size_t nkeys, uint32_t logN, uint32_t prefix_bits) {
    const uint32_t stop = stop_of(logN);
    const int k = g_pir_kernel.load(std::memory_order_relaxed);
    return !want_bs() && k != DPF_PIR_SPLIT && prefix_bits <= stop &&
                   dpfk::pir_fused_ok(nkeys, stop, prefix_bits, k == DPF_PIR_FUSED_ANY)
               ? DPF_PIR_FUSED
               : DPF_PIR_SPLIT;
}

int dpf_set_fold_limits(uint32_t max_blocks, uint32_t max_sg_per_block) {
    dpfk::set_fold_limits(max_blocks, max_sg_per_block);
    return DPF_OK;
}

// ---- the bit-sliced layout: 32-byte records, multiples of 32 (_wide), of 4 (_any) ----
size_t dpf_pir_db_sliced_size(uint64_t nrec) { return sliced_size(RecRule::Mul32, nrec, 32); }
size_t dpf_pir_db_sliced_size_wide(uint64_t nrec, size_t rec_bytes) { return sliced_size(RecRule::Mul32, nrec, rec_bytes); }
size_t dpf_pir_db_sliced_size_any(uint64_t nrec, size_t rec_bytes) { return sliced_size(RecRule::Mul4, nrec, rec_bytes); }

int dpf_pir_db_slice_dev(int device, const uint8_t* d_db, uint64_t nrec, uint8_t* d_dbs, void* stream) {
    return pir_db_slice(RecRule::Mul32, device, d_db, nrec, 32, d_dbs, stream);
}
int dpf_pir_db_slice_wide_dev(int device, const uint8_t* d_db, uint64_t nrec, size_t rec_bytes, uint8_t* d_dbs,
                              void* stream) {
    return pir_db_slice(RecRule::Mul32, device, d_db, nrec, rec_bytes, d_dbs, stream);
}
int dpf_pir_db_slice_any_dev(int device, const uint8_t* d_db, uint64_t nrec, size_t rec_bytes, uint8_t* d_dbs,
                             void* stream) {
    return pir_db_slice(RecRule::Mul4, device, d_db, nrec, rec_bytes, d_dbs, stream);
}

// ---- answers: subtree EvalFull + fold ----
int dpf_pir_answer_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                       uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_db, uint64_t nrec, uint8_t* d_ans,
                       void* d_work, void* stream) {
    return pir_answer(RecRule::Mul32, false, device, d_keys, klen, nkeys, logN, prefix_bits, prefix, d_db, nrec, 32, d_ans,
                      d_work, stream);
}
int dpf_pir_answer_sliced_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                              uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_dbs, uint64_t nrec,
                              uint8_t* d_ans, void* d_work, void* stream) {
    return pir_answer(RecRule::Mul32, true, device, d_keys, klen, nkeys, logN, prefix_bits, prefix, d_dbs, nrec, 32, d_ans,
                      d_work, stream);
}
int dpf_pir_answer_wide_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                            uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_db, uint64_t nrec, size_t rec_bytes,
                            uint8_t* d_ans, void* d_work, void* stream) {
    return pir_answer(RecRule::Mul32, false, device, d_keys, klen, nkeys, logN, prefix_bits, prefix, d_db, nrec, rec_bytes,
                      d_ans, d_work, stream);
}
int dpf_pir_answer_sliced_wide_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                                   uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_dbs, uint64_t nrec,
                                   size_t rec_bytes, uint8_t* d_ans, void* d_work, void* stream) {
    return pir_answer(RecRule::Mul32, true, device, d_keys, klen, nkeys, logN, prefix_bits, prefix, d_dbs, nrec, rec_bytes,
                      d_ans, d_work, stream);
}
int dpf_pir_answer_sliced_any_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                                  uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_dbs, uint64_t nrec,
                                  size_t rec_bytes, uint8_t* d_ans, void* d_work, void* stream) {
    return pir_answer(RecRule::Mul4, true, device, d_keys, klen, nkeys, logN, prefix_bits, prefix, d_dbs, nrec, rec_bytes,
                      d_ans, d_work, stream);
}

// ---- folds over caller-made selection bits ----
int dpf_xor_fold_dev(int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys, const uint8_t* d_payload,
                     uint64_t nrec, size_t rec_bytes, uint8_t* d_ans, void* d_work, void* stream) {
    if (int rc = check_rec_bytes(RecRule::Mul32Uncapped, rec_bytes)) return rc;
    return xor_fold(false, false, device, d_bits, bits_stride, nkeys, d_payload, nrec, rec_bytes, d_ans, d_work, stream);
}
int dpf_xor_fold_sliced_dev(int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys, const uint8_t* d_dbs,
                            uint64_t nrec, uint8_t* d_ans, void* d_work, void* stream) {
    return xor_fold(true, false, device, d_bits, bits_stride, nkeys, d_dbs, nrec, 32, d_ans, d_work, stream);
}
int dpf_xor_fold_sliced_wide_dev(int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys,
                                 const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes, uint8_t* d_ans, void* d_work,
                                 void* stream) {
    if (int rc = check_rec_bytes(RecRule::Mul32, rec_bytes)) return rc;
    return xor_fold(true, rec_bytes > 32, device, d_bits, bits_stride, nkeys, d_dbs, nrec, rec_bytes, d_ans, d_work,
                    stream);
}
int dpf_xor_fold_sliced_any_dev(int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys,
                                const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes, uint8_t* d_ans, void* d_work,
                                void* stream) {
    if (int rc = check_rec_bytes(RecRule::Mul4, rec_bytes)) return rc;
    return xor_fold(true, rec_bytes > 32, device, d_bits, bits_stride, nkeys, d_dbs, nrec, rec_bytes, d_ans, d_work,
                    stream);
}

// ---- records changed / read back in place ----
int dpf_pir_db_update_sliced_wide_dev(int device, uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes, const uint64_t* d_idx,
                                      const uint8_t* d_recs, size_t n, void* stream) {
    return update_or_gather(RecRule::Mul32, device, d_dbs, nrec, rec_bytes, d_idx, d_recs, nullptr, n, stream);
}
int dpf_pir_db_gather_sliced_wide_dev(int device, const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                                      const uint64_t* d_idx, size_t n, uint8_t* d_out, void* stream) {
    return update_or_gather(RecRule::Mul32, device, const_cast<uint8_t*>(d_dbs), nrec, rec_bytes, d_idx, nullptr, d_out, n,
                            stream);
}
int dpf_pir_db_update_sliced_any_dev(int device, uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes, const uint64_t* d_idx,
                                     const uint8_t* d_recs, size_t n, void* stream) {
    return update_or_gather(RecRule::Mul4, device, d_dbs, nrec, rec_bytes, d_idx, d_recs, nullptr, n, stream);
}
int dpf_pir_db_gather_sliced_any_dev(int device, const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                                     const uint64_t* d_idx, size_t n, uint8_t* d_out, void* stream) {
    return update_or_gather(RecRule::Mul4, device, const_cast<uint8_t*>(d_dbs), nrec, rec_bytes, d_idx, nullptr, d_out, n,
                            stream);
}

// ---- private writes: scatters over caller-made bits, and subtree EvalFull + scatter ----
int dpf_xor_scatter_dev(int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys, const uint8_t* d_msgs,
                        uint8_t* d_db, uint64_t nrec, size_t rec_bytes, void* stream) {
    return xor_scatter(RecRule::Mul32, false, device, d_bits, bits_stride, nkeys, d_msgs, d_db, nrec, rec_bytes, stream);
}
int dpf_xor_scatter_sliced_wide_dev(int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys,
                                    const uint8_t* d_msgs, uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                                    void* stream) {
    return xor_scatter(RecRule::Mul32, true, device, d_bits, bits_stride, nkeys, d_msgs, d_dbs, nrec, rec_bytes, stream);
}
int dpf_xor_scatter_sliced_any_dev(int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys,
                                   const uint8_t* d_msgs, uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                                   void* stream) {
    return xor_scatter(RecRule::Mul4, true, device, d_bits, bits_stride, nkeys, d_msgs, d_dbs, nrec, rec_bytes, stream);
}
int dpf_pir_write_wide_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                           uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_msgs, uint8_t* d_db, uint64_t nrec,
                           size_t rec_bytes, void* d_work, void* stream) {
    return pir_write(RecRule::Mul32, false, device, d_keys, klen, nkeys, logN, prefix_bits, prefix, d_msgs, d_db, nrec,
                     rec_bytes, d_work, stream);
}
int dpf_pir_write_sliced_wide_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                                  uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_msgs, uint8_t* d_dbs,
                                  uint64_t nrec, size_t rec_bytes, void* d_work, void* stream) {
    return pir_write(RecRule::Mul32, true, device, d_keys, klen, nkeys, logN, prefix_bits, prefix, d_msgs, d_dbs, nrec,
                     rec_bytes, d_work, stream);
}
int dpf_pir_write_sliced_any_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                                 uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_msgs, uint8_t* d_dbs,
                                 uint64_t nrec, size_t rec_bytes, void* d_work, void* stream) {
    return pir_write(RecRule::Mul4, true, device, d_keys, klen, nkeys, logN, prefix_bits, prefix, d_msgs, d_dbs, nrec,
                     rec_bytes, d_work, stream);
}

// ---- PIR over any record range: records [first_rec, first_rec + nrec) of the domain ----
// The selection bits come from the window EvalFull (window_evalfull: sub-keys
// and one tree launch over them, or the prefixed launch of the forms above
// where the window is one subtree) into rows inside d_work; the fold and the
// scatter read them at row_offset, stride row_bytes.
size_t dpf_pir_window_workspace_size(size_t nkeys, uint32_t logN, uint64_t first_rec, uint64_t nrec, size_t rec_bytes) {
    if (!rec_bytes_ok(RecRule::Mul4, rec_bytes) || !dpfh::window_records_ok(logN, first_rec, nrec)) return 0;
    if (nrec == 0) return 16;
    return window_ws(nullptr, nkeys, logN, first_rec / 128, dpfh::window_blocks_of(nrec)).total;
}

int dpf_pir_answer_window_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN, uint64_t first_rec,
                              const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes, uint8_t* d_ans, void* d_work,
                              void* stream) {
    if (int rc = check_rec_bytes(RecRule::Mul4, rec_bytes)) return rc;
    if (int rc = check_window_records(klen, logN, first_rec, nrec)) return rc;
    if (int rc = check_answer_bufs(d_keys, nkeys, d_dbs, nrec, d_ans, d_work)) return rc;
    DeviceGuard g(device);
    CuScope cus(stream);
    hipStream_t st = (hipStream_t)stream;
    if (nkeys == 0) return DPF_OK;
    if (nrec == 0) {
        HIP_TRY(dpfk::launch_zero(d_ans, nkeys * rec_bytes, st));
        return DPF_OK;
    }
    const WindowWs w = window_ws(d_work, nkeys, logN, first_rec / 128, dpfh::window_blocks_of(nrec));
    HIP_TRY(window_evalfull(d_keys, klen, nkeys, logN, w, w.rows, w.plan.row_bytes, st));
    HIP_TRY(fold_launcher(true)((const uint32_t*)(w.rows + w.plan.row_offset), w.plan.row_bytes / 4, d_dbs, nrec, rec_bytes,
                                (uint32_t)nkeys, (uint32_t*)d_ans, w.parts, st));
    return DPF_OK;
}

int dpf_pir_write_window_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN, uint64_t first_rec,
                             const uint8_t* d_msgs, uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes, void* d_work,
                             void* stream) {
    if (int rc = check_rec_bytes(RecRule::Mul4, rec_bytes)) return rc;
    if (int rc = check_window_records(klen, logN, first_rec, nrec)) return rc;
    if (!present(d_keys, d_msgs, d_dbs, d_work)) return null_buffer();
    if (!aligned(16, d_msgs, d_dbs, d_work)) return misaligned_buffer();
    if (nkeys == 0 || nrec == 0) return DPF_OK;
    DeviceGuard g(device);
    CuScope cus(stream);
    hipStream_t st = (hipStream_t)stream;
    const WindowWs w = window_ws(d_work, nkeys, logN, first_rec / 128, dpfh::window_blocks_of(nrec));
    HIP_TRY(window_evalfull(d_keys, klen, nkeys, logN, w, w.rows, w.plan.row_bytes, st));
    HIP_TRY(scatter_launcher(true)((const uint32_t*)(w.rows + w.plan.row_offset), w.plan.row_bytes / 4, d_dbs, nrec, rec_bytes,
                                   d_msgs, nkeys, st));
    return DPF_OK;
}

// ---- PIR over a sparse key set: record j lives at domain point d_points[j] ----
// The selection bits come from the Eval-bits launches at the records' points,
// not from an EvalFull of a subtree; the fold and the scatter are the dense ones.
size_t dpf_pir_sparse_workspace_size(size_t nkeys, uint64_t nrec, uint32_t logN) {
    return sparse_ws(nullptr, nkeys, nrec, logN).total;
}

int dpf_pir_answer_sparse_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                              const uint64_t* d_points, const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                              uint8_t* d_ans, void* d_work, void* stream) {
    if (int rc = check_rec_bytes(RecRule::Mul4, rec_bytes)) return rc;
    if (int rc = check_key(klen, logN, false)) return rc;
    if (int rc = check_answer_bufs(d_keys, nkeys, d_dbs, nrec, d_ans, d_work)) return rc;
    if (nkeys > 0 && nrec > 0 && !present(d_points)) return null_buffer();
    if (!aligned(8, d_points)) return misaligned_buffer();
    if (nkeys == 0) return DPF_OK;
    DeviceGuard g(device);
    CuScope cus(stream);
    hipStream_t st = (hipStream_t)stream;
    if (nrec == 0) {
        HIP_TRY(dpfk::launch_zero(d_ans, nkeys * rec_bytes, st));
        return DPF_OK;
    }
    const SparseWs w = sparse_ws(d_work, nkeys, nrec, logN);
    HIP_TRY(eval_bits_launch(d_keys, klen, nkeys, nkeys, d_points, nrec, logN, w.bits, w.stride, d_work, w.eval_bytes, st));
    HIP_TRY(fold_launcher(true)((const uint32_t*)w.bits, w.stride / 4, d_dbs, nrec, rec_bytes, (uint32_t)nkeys,
                                (uint32_t*)d_ans, w.parts, st));
    return DPF_OK;
}

int dpf_pir_write_sparse_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                             const uint64_t* d_points, const uint8_t* d_msgs, uint8_t* d_dbs, uint64_t nrec,
                             size_t rec_bytes, void* d_work, void* stream) {
    if (int rc = check_rec_bytes(RecRule::Mul4, rec_bytes)) return rc;
    if (int rc = check_key(klen, logN, false)) return rc;
    if (!present(d_keys, d_points, d_msgs, d_dbs, d_work)) return null_buffer();
    if (!aligned(16, d_msgs, d_dbs, d_work) || !aligned(8, d_points)) return misaligned_buffer();
    if (nkeys == 0 || nrec == 0) return DPF_OK;
    DeviceGuard g(device);
    CuScope cus(stream);
    hipStream_t st = (hipStream_t)stream;
    const SparseWs w = sparse_ws(d_work, nkeys, nrec, logN);
    HIP_TRY(eval_bits_launch(d_keys, klen, nkeys, nkeys, d_points, nrec, logN, w.bits, w.stride, d_work, w.eval_bytes, st));
    HIP_TRY(scatter_launcher(true)((const uint32_t*)w.bits, w.stride / 4, d_dbs, nrec, rec_bytes, d_msgs, nkeys, st));
    return DPF_OK;
}

// ---- grouped PIR: ngroups small DBs of one shape, each with its own keys ----
// The layout is the any-width sliced layout of one flat DB (pir_group_plan.hpp);
// the fold has a group coordinate (launch_pir_fold_grouped).
uint64_t dpf_pir_group_stride(uint64_t nrec) { return dpfh::group_stride(nrec); }

size_t dpf_pir_db_grouped_size(uint64_t ngroups, uint64_t nrec, size_t rec_bytes) {
    uint64_t bytes = 0;
    if (!rec_bytes_ok(RecRule::Mul4, rec_bytes) || !dpfh::grouped_bytes(ngroups, nrec, rec_bytes, &bytes)) return 0;
    return std::max<size_t>(16, bytes);
}

int dpf_pir_db_slice_grouped_dev(int device, const uint8_t* d_db, uint64_t ngroups, uint64_t nrec, size_t rec_bytes,
                                 uint8_t* d_dbs, void* stream) {
    return grouped_reslice(dpfk::launch_slice_db, true, "dpf: grouped DB too large", device, d_db, ngroups, nrec, rec_bytes,
                           d_dbs, stream);
}

// ---- the whole-DB read-out: un-slice, and the merge of two sliced buffers ----
// The inverse of the two slice entries above, with their rules in their order
// (grouped_reslice); a DB of any width is one group.
int dpf_pir_db_unslice_any_dev(int device, const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes, uint8_t* d_db,
                               void* stream) {
    return grouped_reslice(dpfk::launch_unslice_db, false, "dpf: DB too large", device, d_dbs, 1, nrec, rec_bytes, d_db,
                           stream);
}

int dpf_pir_db_unslice_grouped_dev(int device, const uint8_t* d_dbs, uint64_t ngroups, uint64_t nrec, size_t rec_bytes,
                                   uint8_t* d_db, void* stream) {
    return grouped_reslice(dpfk::launch_unslice_db, false, "dpf: grouped DB too large", device, d_dbs, ngroups, nrec,
                           rec_bytes, d_db, stream);
}

int dpf_pir_db_xor_sliced_dev(int device, uint8_t* d_dbs, const uint8_t* d_other, size_t bytes, void* stream) {
    if (bytes % 16 != 0) return fail(DPF_ERR_PARAM, "dpf: bytes must be a multiple of 16");
    if (bytes > 0 && !present(d_dbs, d_other)) return null_buffer();
    if (!aligned(16, d_dbs, d_other)) return misaligned_buffer();
    if (bytes == 0) return DPF_OK;
    DeviceGuard g(device);
    HIP_TRY(dpfk::launch_xor_words(d_dbs, d_other, bytes, (hipStream_t)stream));
    return DPF_OK;
}

size_t dpf_xor_fold_grouped_workspace_size(uint64_t ngroups, uint64_t keys_per_group, size_t rec_bytes) {
    if (!rec_bytes_ok(RecRule::Mul4, rec_bytes) || check_group_keys(ngroups, keys_per_group) != DPF_OK) return 0;
    return group_fold_ws_bytes();
}

int dpf_xor_fold_grouped_dev(int device, const uint8_t* d_bits, size_t bits_stride, uint64_t ngroups,
                             uint64_t keys_per_group, const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                             uint8_t* d_ans, void* d_work, void* stream) {
    if (int rc = check_rec_bytes(RecRule::Mul4, rec_bytes)) return rc;
    if (int rc = check_sel_bits(bits_stride, nrec)) return rc;
    if (int rc = check_group_keys(ngroups, keys_per_group)) return rc;
    const uint64_t nkeys = ngroups * keys_per_group;
    if (nkeys > 0 && !(present(d_ans, d_work) && (nrec == 0 || present(d_bits, d_dbs)))) return null_buffer();
    if (!aligned(16, d_bits, d_dbs, d_work) || !aligned(4, d_ans)) return misaligned_buffer();
    if (nkeys == 0) return DPF_OK;
    DeviceGuard g(device);
    CuScope cus(stream);
    HIP_TRY(dpfk::launch_pir_fold_grouped((const uint32_t*)d_bits, bits_stride / 4, d_dbs, ngroups,
                                          (uint32_t)keys_per_group, nrec, rec_bytes, (uint32_t*)d_ans, (uint32_t*)d_work,
                                          (hipStream_t)stream));
    return DPF_OK;
}

size_t dpf_pir_grouped_workspace_size(uint64_t ngroups, uint64_t keys_per_group, uint32_t logN, size_t rec_bytes) {
    if (!rec_bytes_ok(RecRule::Mul4, rec_bytes) || check_group_keys(ngroups, keys_per_group) != DPF_OK) return 0;
    return group_ws(nullptr, ngroups * keys_per_group, stop_of(logN)).total;
}

int dpf_pir_answer_grouped_dev(int device, const uint8_t* d_keys, size_t klen, uint64_t ngroups, uint64_t keys_per_group,
                               uint32_t logN, const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes, uint8_t* d_ans,
                               void* d_work, void* stream) {
    if (int rc = check_rec_bytes(RecRule::Mul4, rec_bytes)) return rc;
    if (int rc = check_subtree(klen, logN, 0, 0, nrec)) return rc;   // the key, then nrec <= 2^logN
    if (int rc = check_group_keys(ngroups, keys_per_group)) return rc;
    const size_t nkeys = ngroups * keys_per_group;
    if (int rc = check_answer_bufs(d_keys, nkeys, d_dbs, nrec, d_ans, d_work)) return rc;
    if (nkeys == 0) return DPF_OK;
    DeviceGuard g(device);
    CuScope cus(stream);
    hipStream_t st = (hipStream_t)stream;
    if (nrec == 0) {
        HIP_TRY(dpfk::launch_zero(d_ans, nkeys * rec_bytes, st));
        return DPF_OK;
    }
    GroupWs w;
    if (int rc = group_tree(d_keys, klen, nkeys, logN, d_work, st, &w)) return rc;
    HIP_TRY(dpfk::launch_pir_fold_grouped((const uint32_t*)w.bits, w.per_key / 4, d_dbs, ngroups, (uint32_t)keys_per_group,
                                          nrec, rec_bytes, (uint32_t*)d_ans, w.scratch, st));
    return DPF_OK;
}

int dpf_fold_grouped_form_for(uint64_t ngroups, uint64_t keys_per_group, uint64_t nrec, size_t rec_bytes, int cus,
                              dpf_fold_grouped_form* form) {
    if (form == nullptr || !rec_bytes_ok(RecRule::Mul4, rec_bytes) || check_group_keys(ngroups, keys_per_group) != DPF_OK ||
        nrec > UINT64_MAX - 255)
        return fail(DPF_ERR_PARAM, "dpf: form query out of range");
    const dpfh::GroupFoldKeysPlan p =
        dpfk::fold_grouped_plan(ngroups, (uint32_t)keys_per_group, nrec, rec_bytes, (uint64_t)(cus > 0 ? cus : 0));
    memset(form, 0, sizeof *form);
    form->route = (uint32_t)p.route;
    form->atomic = p.atomic();
    form->max_blocks = p.cap;
    uint64_t launches = 0;
    if (p.route == dpfh::kFoldRouteMfma) {
        const dpfh::GroupFoldPass t = p.tile(0);
        form->columns_per_wg = t.cg;
        form->keys_per_tile = 32u * (uint32_t)dpfh::kFoldTiles[t.shape].MT;
        form->runs = t.runs;
        form->sg_per_run = t.spr;
        form->units = p.units(t);
        form->passes = form->units ? p.tiles() : 0;
        p.for_each_launch([&](const dpfh::GroupFoldLaunch&) { return ++launches, 0; });
    } else {
        form->columns_per_wg = 1;
        form->keys_per_tile = p.direct.kp_max;
        form->runs = p.direct.runs;
        form->sg_per_run = p.direct.spr;
        form->units = p.direct.units();
        form->passes = p.direct.passes();
        p.direct.for_each_launch([&](const dpfh::GroupLaunch&) { return ++launches, 0; });
    }
    form->launches = launches;
    return DPF_OK;
}

// ---- grouped private writes: the dual of the grouped fold ----
// The scatter has a group coordinate (launch_scatter_grouped), or loops the
// dense scatter over the groups where its plan says so; no workspace.
int dpf_xor_scatter_grouped_dev(int device, const uint8_t* d_bits, size_t bits_stride, uint64_t ngroups,
                                uint64_t keys_per_group, const uint8_t* d_msgs, uint8_t* d_dbs, uint64_t nrec,
                                size_t rec_bytes, void* stream) {
    if (int rc = check_rec_bytes(RecRule::Mul4, rec_bytes)) return rc;
    if (int rc = check_sel_bits(bits_stride, nrec)) return rc;
    if (int rc = check_group_keys(ngroups, keys_per_group)) return rc;
    if (!present(d_bits, d_msgs, d_dbs)) return null_buffer();
    if (!aligned(16, d_bits, d_msgs, d_dbs)) return misaligned_buffer();
    if (ngroups == 0 || keys_per_group == 0 || nrec == 0) return DPF_OK;
    DeviceGuard g(device);
    CuScope cus(stream);
    HIP_TRY(dpfk::launch_scatter_grouped((const uint32_t*)d_bits, bits_stride / 4, d_dbs, ngroups,
                                         (uint32_t)keys_per_group, nrec, rec_bytes, d_msgs, (hipStream_t)stream));
    return DPF_OK;
}

int dpf_pir_write_grouped_dev(int device, const uint8_t* d_keys, size_t klen, uint64_t ngroups, uint64_t keys_per_group,
                              uint32_t logN, const uint8_t* d_msgs, uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                              void* d_work, void* stream) {
    if (int rc = check_rec_bytes(RecRule::Mul4, rec_bytes)) return rc;
    if (int rc = check_subtree(klen, logN, 0, 0, nrec)) return rc;   // the key, then nrec <= 2^logN
    if (int rc = check_group_keys(ngroups, keys_per_group)) return rc;
    if (!present(d_keys, d_msgs, d_dbs, d_work)) return null_buffer();
    if (!aligned(16, d_msgs, d_dbs, d_work)) return misaligned_buffer();
    const size_t nkeys = ngroups * keys_per_group;
    if (nkeys == 0 || nrec == 0) return DPF_OK;
    DeviceGuard g(device);
    CuScope cus(stream);
    hipStream_t st = (hipStream_t)stream;
    GroupWs w;
    if (int rc = group_tree(d_keys, klen, nkeys, logN, d_work, st, &w)) return rc;
    HIP_TRY(dpfk::launch_scatter_grouped((const uint32_t*)w.bits, w.per_key / 4, d_dbs, ngroups, (uint32_t)keys_per_group,
                                         nrec, rec_bytes, d_msgs, st));
    return DPF_OK;
}

int dpf_scatter_grouped_form_for(uint64_t ngroups, uint64_t keys_per_group, uint64_t nrec, size_t rec_bytes, int cus,
                                 dpf_scatter_grouped_form* form) {
    if (form == nullptr || !rec_bytes_ok(RecRule::Mul4, rec_bytes) || check_group_keys(ngroups, keys_per_group) != DPF_OK ||
        nrec > UINT64_MAX - 255)
        return fail(DPF_ERR_PARAM, "dpf: form query out of range");
    const dpfh::GroupedPlan p =
        dpfk::scatter_grouped_plan(ngroups, (uint32_t)keys_per_group, nrec, rec_bytes, (uint64_t)(cus > 0 ? cus : 0));
    memset(form, 0, sizeof *form);
    form->route = (uint32_t)p.route;
    form->columns = p.C;
    form->runs = p.runs;
    form->sg_per_run = p.spr;
    form->units = p.units();
    form->max_blocks = p.cap;
    form->passes = p.passes();
    uint64_t launches = 0;
    uint32_t widths = 0;
    p.for_each_launch([&](const dpfh::GroupLaunch& l) {
        ++launches;
        if (l.u0 == 0) widths |= 1u << (l.kp - 1);
        return 0;
    });
    form->launches = launches;
    form->pass_widths = widths;
    return DPF_OK;
}

// ---- grouped keyword PIR: every group's records at its own points ----
// The selection rows come from the Eval-bits launch with a list coordinate
// (group g's keys at d_points[g][0 .. nrec)), not from a whole-domain tree
// pass; the fold and the scatter are the grouped ones.
size_t dpf_pir_grouped_sparse_workspace_size(uint64_t ngroups, uint64_t keys_per_group, uint64_t nrec, uint32_t logN,
                                             size_t rec_bytes) {
    if (!rec_bytes_ok(RecRule::Mul4, rec_bytes) || check_group_keys(ngroups, keys_per_group) != DPF_OK) return 0;
    return group_sparse_ws(nullptr, ngroups * keys_per_group, nrec, logN).total;
}

int dpf_pir_answer_grouped_sparse_dev(int device, const uint8_t* d_keys, size_t klen, uint64_t ngroups,
                                      uint64_t keys_per_group, uint32_t logN, const uint64_t* d_points,
                                      const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes, uint8_t* d_ans, void* d_work,
                                      void* stream) {
    if (int rc = check_rec_bytes(RecRule::Mul4, rec_bytes)) return rc;
    if (int rc = check_key(klen, logN)) return rc;
    if (int rc = check_group_keys(ngroups, keys_per_group)) return rc;
    if (int rc = check_group_points(ngroups, nrec)) return rc;
    const size_t nkeys = ngroups * keys_per_group;
    if (int rc = check_answer_bufs(d_keys, nkeys, d_dbs, d_points, nrec, d_ans, d_work)) return rc;
    if (nkeys == 0) return DPF_OK;
    DeviceGuard g(device);
    CuScope cus(stream);
    hipStream_t st = (hipStream_t)stream;
    if (nrec == 0) {
        HIP_TRY(dpfk::launch_zero(d_ans, nkeys * rec_bytes, st));
        return DPF_OK;
    }
    const GroupSparseWs w = group_sparse_ws(d_work, nkeys, nrec, logN);
    HIP_TRY(eval_bits_launch(d_keys, klen, nkeys, keys_per_group, d_points, nrec, logN, w.bits, w.stride, d_work,
                             w.eval_bytes, st));
    HIP_TRY(dpfk::launch_pir_fold_grouped((const uint32_t*)w.bits, w.stride / 4, d_dbs, ngroups, (uint32_t)keys_per_group,
                                          nrec, rec_bytes, (uint32_t*)d_ans, w.scratch, st));
    return DPF_OK;
}

int dpf_pir_write_grouped_sparse_dev(int device, const uint8_t* d_keys, size_t klen, uint64_t ngroups,
                                     uint64_t keys_per_group, uint32_t logN, const uint64_t* d_points,
                                     const uint8_t* d_msgs, uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes, void* d_work,
                                     void* stream) {
    if (int rc = check_rec_bytes(RecRule::Mul4, rec_bytes)) return rc;
    if (int rc = check_key(klen, logN)) return rc;
    if (int rc = check_group_keys(ngroups, keys_per_group)) return rc;
    if (int rc = check_group_points(ngroups, nrec)) return rc;
    if (!present(d_keys, d_points, d_msgs, d_dbs, d_work)) return null_buffer();
    if (!aligned(16, d_msgs, d_dbs, d_work) || !aligned(8, d_points)) return misaligned_buffer();
    const size_t nkeys = ngroups * keys_per_group;
    if (nkeys == 0 || nrec == 0) return DPF_OK;
    DeviceGuard g(device);
    CuScope cus(stream);
    hipStream_t st = (hipStream_t)stream;
    const GroupSparseWs w = group_sparse_ws(d_work, nkeys, nrec, logN);
    HIP_TRY(eval_bits_launch(d_keys, klen, nkeys, keys_per_group, d_points, nrec, logN, w.bits, w.stride, d_work,
                             w.eval_bytes, st));
    HIP_TRY(dpfk::launch_scatter_grouped((const uint32_t*)w.bits, w.stride / 4, d_dbs, ngroups, (uint32_t)keys_per_group,
                                         nrec, rec_bytes, d_msgs, st));
    return DPF_OK;
}

}  // extern "C"
