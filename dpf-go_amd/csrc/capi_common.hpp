// capi_common.hpp — what the translation units of the C ABI share (internal).
//   dpf_capi.hip     the device registry and the knobs, the staging pipeline,
//                    the tree, Eval and Eval-bits entries, the form queries
//   capi_pir.hip     every device-resident PIR form (slice and un-slice, fold, scatter,
//                    answer, write, update / gather, the sparse composites,
//                    the grouped forms, the grouped-sparse composites)
//   capi_pir_db.hip  the resident-DB handle (create, answer, update / read, write,
//                    the grouped write, export / merge / clear)
// Here: the error slot, the device objects, and one definition of each
// workspace layout and of each argument rule.  An entry point is a short list
// of these rules in its own order of reports (the folds check alignment before
// null, the scatters and the answers null before alignment): the order decides
// which message a doubly-bad call gets, so it is part of the contract
// (tests/test_capi_contract_cpu.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dpf_hip.h"
#include "dpf_internal.hpp"
#include "bs_kernels.hpp"
#include "dpf_kernels.hpp"
#include "eval_bits_plan.hpp"
#include "pir_group_plan.hpp"
#include "pir_kernels.hpp"
#include "pir_window_plan.hpp"
#include "stage_plan.hpp"

namespace dpfc {

using dpfh::stop_of;

extern thread_local std::string t_err;   // dpf_last_error's text (dpf_capi.hip)

inline int fail(int code, const std::string& msg) {
    t_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                                         \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) return dpfc::fail(DPF_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
    } while (0)

// A buffer grown on demand: device memory (hipMalloc), or with Pinned a
// pinned host staging buffer (hipHostMalloc).
template <bool Pinned>
struct Buf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        release();
        hipError_t e = Pinned ? hipHostMalloc(&p, n, hipHostMallocDefault) : hipMalloc(&p, n);
        if (e == hipSuccess) cap = n;
        return e;
    }
    void release() {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
};
using DevBuf = Buf<false>;
using HostBuf = Buf<true>;

struct Dev {
    int id = 0;
    hipStream_t st = nullptr;    // kernels
    hipStream_t cst = nullptr;   // device -> host copies of the pipelined host-buffer paths
    hipStream_t hst = nullptr;   // host -> device copies (batched Eval's points)
    hipEvent_t ev_k[2] = {nullptr, nullptr}, ev_c[2] = {nullptr, nullptr}, ev_h[2] = {nullptr, nullptr};
    std::mutex mu;
    DevBuf keys, work, out, xs;
    HostBuf pin[2];
    ~Dev();
};
using DevList = std::vector<std::shared_ptr<Dev>>;

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        (void)hipSetDevice(d);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// A _dev entry point launching on a stream of dpf_stream_create_cu_masked
// sizes its grids to that stream's CUs; any other stream gets the whole device.
struct CuScope {
    int prev;
    explicit CuScope(void* stream);
    ~CuScope() { dpfk::set_cu_budget(prev); }
};

// The opened devices, opening every visible one on first use; pick_devs: the
// first min(ngpus, opened) of them (ngpus <= 0: all).  Empty + error set on failure.
DevList devices(int* rc);
DevList pick_devs(int ngpus, int* rc);

// Run fn(device_index, lo, hi) over `n` items split evenly across g devices.
template <class F>
int shard(size_t n, int g, F fn) {
    if (g <= 1 || n <= 1) return fn(0, (size_t)0, n);
    std::vector<int> rc((size_t)g, DPF_OK);
    std::vector<std::string> errs((size_t)g);
    std::vector<std::thread> th;
    for (int i = 0; i < g; ++i) {
        const size_t lo = n * (size_t)i / (size_t)g, hi = n * (size_t)(i + 1) / (size_t)g;
        th.emplace_back([&, i, lo, hi] {
            rc[(size_t)i] = lo < hi ? fn(i, lo, hi) : DPF_OK;
            errs[(size_t)i] = t_err;
        });
    }
    for (auto& t : th) t.join();
    for (int i = 0; i < g; ++i)
        if (rc[(size_t)i]) return fail(rc[(size_t)i], errs[(size_t)i]);
    return DPF_OK;
}

// The back end a call uses, decided once per call (expansion and launches agree).
bool want_bs();

// ---- workspace layouts ------------------------------------------------------
inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
// base + off; base is null where only a layout's size is asked for.
inline uint8_t* at(const void* base, size_t off) { return reinterpret_cast<uint8_t*>((uintptr_t)base + off); }

// Tree workspace for nk expanded keys: [T-table records | byte-sliced CW
// words | byte-sliced frontier for up to `chunk` keys per launch].
inline size_t tree_ws_bytes(size_t nk, uint32_t stop, uint32_t prefix_bits, size_t chunk) {
    return align256(nk * dpfk::ek_words(stop) * 4) + align256(nk * dpfk::bs_key_words(stop) * 4) +
           dpfk::bs_frontier_bytes(chunk, stop, prefix_bits);
}
struct TreeWs {
    uint32_t* ek;
    uint32_t* ekb;
    void* frontier;
};
inline TreeWs tree_ws(void* work, size_t nk, uint32_t stop) {
    const size_t ek = align256(nk * dpfk::ek_words(stop) * 4);
    return {(uint32_t*)work, (uint32_t*)at(work, ek), at(work, ek + align256(nk * dpfk::bs_key_words(stop) * 4))};
}

// d_work of the dense PIR composites: [tree workspace | selection bits = the
// subtree's EvalFull bytes, per_key of them a key | the fold's partials], the
// first two parts padded to 256 B.  prefix_bits <= stop.
struct PirWs {
    TreeWs tree;
    uint8_t* bits;
    uint64_t per_key;
    uint32_t* parts;
    size_t total;
};
inline PirWs pir_ws(void* d_work, size_t nkeys, uint32_t stop, uint32_t prefix_bits) {
    PirWs w;
    w.tree = tree_ws(d_work, nkeys, stop);
    w.per_key = (uint64_t)16 << (stop - prefix_bits);
    const size_t tree = align256(tree_ws_bytes(nkeys, stop, prefix_bits, nkeys)), bits = align256(nkeys * w.per_key);
    w.bits = at(d_work, tree);
    w.parts = (uint32_t*)at(d_work, tree + bits);
    w.total = tree + bits + dpfk::pir_fold_parts_bytes();
    return w;
}

// Batched-Eval and Eval-bits workspace: [expanded keys, padded to 256 B | the
// frontier].  A caller may pass less than eval_ws_bytes: what is left past the
// records is the frontier's (launch_eval walks from the root if it is too
// small), and a workspace that does not hold the records is refused.
inline size_t eval_ws_bytes(size_t nkeys, size_t ppk, uint32_t logN) {
    return std::max<size_t>(16, align256(nkeys * dpfk::ek_words(stop_of(logN)) * 4) +
                                    dpfk::eval_frontier_bytes(nkeys, stop_of(logN), ppk));
}
struct EvalWs {
    size_t ek_bytes;         // the records, padded
    void* frontier;          // null: none
    size_t frontier_bytes;
    bool fits;               // the records fit
};
inline EvalWs eval_ws(void* d_work, size_t work_bytes, size_t nkeys, uint32_t logN) {
    const size_t rec = nkeys * dpfk::ek_words(stop_of(logN)) * 4, ekb = align256(rec);
    const bool rest = work_bytes > ekb;
    return {ekb, rest ? at(d_work, ekb) : nullptr, rest ? work_bytes - ekb : 0, work_bytes >= rec};
}
inline int check_eval_ws(const EvalWs& w) {
    return w.fits ? DPF_OK : fail(DPF_ERR_PARAM, "dpf: Eval workspace too small");
}

// d_work of the two sparse composites: [Eval-bits workspace | bit rows
// [nkeys][dpf_eval_bits_stride(nrec)] | the fold's partials], each part
// rounded up to 16 bytes.
struct SparseWs {
    size_t eval_bytes, stride;
    uint8_t* bits;
    uint32_t* parts;
    size_t total;
};
inline SparseWs sparse_ws(void* d_work, size_t nkeys, uint64_t nrec, uint32_t logN) {
    SparseWs w;
    w.eval_bytes = align16(eval_ws_bytes(nkeys, nrec, logN));
    w.stride = dpfh::eval_bits_stride(nrec);
    const size_t rows = align16(nkeys * w.stride);
    w.bits = at(d_work, w.eval_bytes);
    w.parts = (uint32_t*)at(d_work, w.eval_bytes + rows);
    w.total = w.eval_bytes + rows + align16(dpfk::pir_fold_parts_bytes());
    return w;
}

// d_work of the grouped PIR composite: [tree workspace of all ngroups * kpg
// keys | selection bits, a whole-domain EvalFull row of per_key bytes a key |
// the grouped fold's scratch], the first two parts padded to 256 B.  The
// grouped fold writes no scratch (dpfh::GroupedPlan::scratch_bytes); its
// size function keeps the ABI's 16-byte minimum.
inline size_t group_fold_ws_bytes() { return std::max<size_t>(16, dpfh::GroupedPlan{}.scratch_bytes()); }
struct GroupWs {
    uint8_t* bits;
    uint64_t per_key;
    uint32_t* scratch;
    size_t total;
};
inline GroupWs group_ws(void* d_work, size_t nkeys, uint32_t stop) {
    GroupWs w;
    w.per_key = (uint64_t)16 << stop;
    const size_t tree = align256(tree_ws_bytes(nkeys, stop, 0, nkeys)), bits = align256(nkeys * w.per_key);
    w.bits = at(d_work, tree);
    w.scratch = (uint32_t*)at(d_work, tree + bits);
    w.total = tree + bits + group_fold_ws_bytes();
    return w;
}

// d_work of the two grouped-sparse composites: [Eval-bits workspace of all
// nkeys = ngroups * kpg keys at nrec points each | bit rows
// [nkeys][dpf_eval_bits_stride(nrec)] in group order | the grouped fold's
// scratch], the first two parts rounded up to 16 bytes.  The rows keep the
// Eval-bits stride: the grouped fold and scatter read no word past a row's end
// (their wlim), so a 16-byte row (nrec <= 128) needs no rounding up to the
// 32 bytes of a super-group's selection words.
struct GroupSparseWs {
    size_t eval_bytes, stride;
    uint8_t* bits;
    uint32_t* scratch;
    size_t total;
};
inline GroupSparseWs group_sparse_ws(void* d_work, size_t nkeys, uint64_t nrec, uint32_t logN) {
    GroupSparseWs w;
    w.eval_bytes = align16(eval_ws_bytes(nkeys, nrec, logN));
    w.stride = dpfh::eval_bits_stride(nrec);
    const size_t rows = align16(nkeys * w.stride);
    w.bits = at(d_work, w.eval_bytes);
    w.scratch = (uint32_t*)at(d_work, w.eval_bytes + rows);
    w.total = w.eval_bytes + rows + group_fold_ws_bytes();
    return w;
}

// d_work of the window forms (pir_window_plan.hpp): [sub-keys, nkeys * P of
// the canonical length | tree workspace of nkeys * P keys at logN' = s | rows
// [nkeys][row_bytes] | the fold's partials], each of the first three padded
// to 256 B.  dpf_evalfull_window_dev uses the first two parts (its rows are
// the caller's), the PIR composites all four.  On the subtree route there are
// no sub-keys: the tree workspace is that of nkeys keys at logN below the
// window's prefix, at the front.
struct WindowWs {
    dpfh::WindowPlan plan;
    size_t nsub, sub_len;    // sub-keys (0 on the subtree route) and their length
    uint8_t* sub;
    void* tree;
    uint8_t* rows;
    uint32_t* parts;
    size_t evalfull_total, total;
};
inline WindowWs window_ws(void* d_work, size_t nkeys, uint32_t logN, uint64_t first_block, uint64_t nblocks) {
    WindowWs w;
    w.plan = dpfh::window_plan(logN, first_block, nblocks);
    const bool pieces = w.plan.route == dpfh::kWindowPieces;
    w.nsub = pieces ? nkeys * (size_t)w.plan.npieces : 0;
    w.sub_len = (size_t)dpfh::window_canonical_sub_key_len(w.plan);
    const size_t sub = align256(w.nsub * w.sub_len);
    const size_t tree = align256(pieces ? tree_ws_bytes(w.nsub, stop_of(w.plan.s), 0, w.nsub)
                                        : tree_ws_bytes(nkeys, stop_of(logN), w.plan.prefix_bits, nkeys));
    // (+16: the fold reads whole super-groups' words, 32 bytes, of a window of 16-byte blocks.)
    const size_t rows = align256(nkeys * (size_t)w.plan.row_bytes + 16);
    w.sub = at(d_work, 0);
    w.tree = at(d_work, sub);
    w.rows = at(d_work, sub + tree);
    w.parts = (uint32_t*)at(d_work, sub + tree + rows);
    w.evalfull_total = std::max<size_t>(16, sub + tree);
    w.total = sub + tree + rows + dpfk::pir_fold_parts_bytes();
    return w;
}

// The window EvalFull of the three window entries, arguments checked: the
// sub-keys and one tree launch over all of them where a key's pieces land
// side by side (row_stride == row_bytes), else a launch per key; on the
// subtree route the one prefixed tree launch of the dense forms.
hipError_t window_evalfull(const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN, const WindowWs& w,
                           uint8_t* d_rows, size_t row_stride, hipStream_t st);

// ---- expanded keys in a caller's d_work (dpf_capi.hip) -----------------------
// Every entry point that expands keys into a caller's d_work records what it
// left there (the tree_ws layout), so a later dpf_evalfull_expanded_dev never
// reads planes built from other keys; a workspace of another layout is dropped.
void note_expanded(const void* d_work, size_t nkeys, uint32_t stop, bool bs);
void forget_expanded(const void* d_work);

// One-shot tree pass from the key bytes in HBM into `out`, with a caller's d_work.
hipError_t tree_from_keys(const uint8_t* d_keys, size_t klen, size_t nk, uint32_t stop, uint32_t prefix_bits,
                          uint64_t prefix, uint8_t* out, uint64_t stride, void* d_work, hipStream_t st, bool bs);

// The keys' T-table records into the front of an Eval workspace, whose other
// layout a later dpf_evalfull_expanded_dev must not take for a tree's.
inline hipError_t eval_unpack(const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN, void* d_work,
                              hipStream_t st) {
    forget_expanded(d_work);
    return dpfk::launch_unpack(d_keys, klen, nkeys, stop_of(logN), (uint32_t*)d_work, st);
}

// The launches of dpf_eval_bits_dev and dpf_eval_bits_grouped_dev, arguments
// checked (dpf_capi.hip): key k at list k / keys_per_list of d_xs[][npts]
// (keys_per_list = nkeys: one shared list).
hipError_t eval_bits_launch(const uint8_t* d_keys, size_t klen, size_t nkeys, size_t keys_per_list, const uint64_t* d_xs,
                            size_t npts, uint32_t logN, uint8_t* d_bits, size_t bits_stride, void* d_work,
                            size_t work_bytes, hipStream_t st);

// ---- argument rules ----------------------------------------------------------
// The reference reads k[0:17], the level records k[17+18i : 17+18i+18] for
// i < stop and the final CW at k[len-16 : len] (dpf.go:175-176,186-188,206,
// 219,231-233): any key of at least 17 + 18*stop bytes evaluates without an
// index panic, including keys whose final CW overlaps the last record.
// EvalFull (full) with logN > 63 cannot allocate its 2^(logN-3)-byte output
// (dpf.go:251 panics in makeslice): DPF_ERR_PARAM.  Eval validates no logN
// (dpf.go:171-211): any logN with a long enough key evaluates, its path bits
// above bit 63 read as 0 (path_bit).
inline int check_key(size_t klen, uint32_t logN, bool full = true) {
    if (full && logN > 63) return fail(DPF_ERR_PARAM, "dpf: logN > 63");
    if (klen < 17 + 18 * (size_t)stop_of(logN)) return fail(DPF_ERR_KEYLEN, "dpf: key shorter than 17+18*(logN-7) bytes");
    return DPF_OK;
}

// Which record widths an entry point takes: a multiple of 32 bytes (the row-
// major fold: any such width; the _wide forms: up to DPF_PIR_MAX_REC_BYTES),
// a multiple of 4 (the _any forms), or any from 1 byte (the handle, which
// pads to 4 on the device).
enum class RecRule { Mul32Uncapped, Mul32, Mul4, Bytes1 };
inline bool rec_bytes_ok(RecRule r, size_t n) {
    const size_t unit = r == RecRule::Bytes1 ? 1 : r == RecRule::Mul4 ? 4 : 32;
    return n != 0 && n % unit == 0 && (r == RecRule::Mul32Uncapped || n <= DPF_PIR_MAX_REC_BYTES);
}
inline int check_rec_bytes(RecRule r, size_t n) {
    if (rec_bytes_ok(r, n)) return DPF_OK;
    switch (r) {
        case RecRule::Mul32Uncapped: return fail(DPF_ERR_PARAM, "dpf: rec_bytes must be a positive multiple of 32");
        case RecRule::Mul32:
            return fail(DPF_ERR_PARAM, "dpf: rec_bytes must be a positive multiple of 32, at most DPF_PIR_MAX_REC_BYTES");
        case RecRule::Mul4:
            return fail(DPF_ERR_PARAM, "dpf: rec_bytes must be a positive multiple of 4, at most DPF_PIR_MAX_REC_BYTES");
        default: return fail(DPF_ERR_PARAM, "dpf: rec_bytes must be 1 .. DPF_PIR_MAX_REC_BYTES");
    }
}

// A DB slice under subtree (prefix_bits, prefix) of the keys' domain: the key,
// the prefix, and no more records than the subtree has points.
inline int check_subtree(size_t klen, uint32_t logN, uint32_t prefix_bits, uint64_t prefix, uint64_t nrec) {
    if (int rc = check_key(klen, logN)) return rc;
    if (!dpfh::prefix_ok(prefix_bits, prefix, stop_of(logN))) return fail(DPF_ERR_PARAM, "dpf: subtree prefix out of range");
    const uint64_t slice = logN - prefix_bits >= 64 ? ~0ull : (1ull << (logN - prefix_bits));
    if (nrec > slice) return fail(DPF_ERR_PARAM, "dpf: more DB records than the subtree's domain");
    return DPF_OK;
}

// A window of leaf blocks of the keys' domain: the key, at least one block,
// inside the domain.
inline int check_window(size_t klen, uint32_t logN, uint64_t first_block, uint64_t nblocks) {
    if (int rc = check_key(klen, logN)) return rc;
    if (!dpfh::window_ok(logN, first_block, nblocks)) return fail(DPF_ERR_PARAM, "dpf: window outside the 2^logN domain");
    return DPF_OK;
}
// Records [first_rec, first_rec + nrec) of the keys' domain behind a window.
inline int check_window_records(size_t klen, uint32_t logN, uint64_t first_rec, uint64_t nrec) {
    if (int rc = check_key(klen, logN)) return rc;
    if (first_rec % 128 != 0) return fail(DPF_ERR_PARAM, "dpf: first_rec must be a multiple of 128");
    if (!dpfh::window_records_ok(logN, first_rec, nrec)) return fail(DPF_ERR_PARAM, "dpf: records outside the 2^logN domain");
    return DPF_OK;
}
// Consecutive prefixes [first_prefix, first_prefix + nprefix) at depth
// prefix_bits of the keys' tree.
inline int check_prefix_run(size_t klen, uint32_t logN, uint32_t prefix_bits, uint64_t first_prefix, uint64_t nprefix) {
    if (int rc = check_key(klen, logN)) return rc;
    if (prefix_bits > stop_of(logN)) return fail(DPF_ERR_PARAM, "dpf: prefix_bits > logN - 7");
    const uint64_t all = 1ull << prefix_bits;   // (prefix_bits <= 56)
    if (first_prefix > all || nprefix > all - first_prefix) return fail(DPF_ERR_PARAM, "dpf: subtree prefix out of range");
    return DPF_OK;
}
// Rows a window EvalFull writes, row_stride bytes a key.
inline int check_window_rows(size_t row_stride, uint64_t row_bytes) {
    if (row_stride % 16 != 0 || row_stride < row_bytes)
        return fail(DPF_ERR_PARAM, "dpf: row_stride must be a multiple of 16, at least the window form's row_bytes");
    return DPF_OK;
}

// Caller-made selection bits, bits_stride bytes a key: rows of whole 16-byte
// words with a bit for every record.
inline int check_sel_bits(size_t bits_stride, uint64_t nrec) {
    if (bits_stride % 16 != 0) return fail(DPF_ERR_PARAM, "dpf: bits_stride must be a multiple of 16");
    if (nrec > (uint64_t)bits_stride * 8) return fail(DPF_ERR_PARAM, "dpf: more records than selection bits per key");
    return DPF_OK;
}

// Bit rows an Eval-bits launch writes, bits_stride bytes a key: whole 16-byte
// words that hold the span of npts points.
inline int check_bits_rows(size_t bits_stride, size_t npts) {
    if (bits_stride % 16 != 0 || bits_stride < dpfh::eval_bits_stride(npts))
        return fail(DPF_ERR_PARAM, "dpf: bits_stride must be a multiple of 16, at least dpf_eval_bits_stride(npts)");
    return DPF_OK;
}

// A grouped call's key rows: ngroups * keys_per_group of them, counted in 32 bits.
inline int check_group_keys(uint64_t ngroups, uint64_t keys_per_group) {
    if (ngroups != 0 && keys_per_group > (uint64_t)UINT32_MAX / ngroups)
        return fail(DPF_ERR_PARAM, "dpf: ngroups * keys_per_group does not fit 32 bits");
    return DPF_OK;
}

// A grouped call's point lists [ngroups][npts]: their bytes fit 64 bits.
inline int check_group_points(uint64_t ngroups, uint64_t npts) {
    if (!dpfh::eval_bits_lists_ok(ngroups, npts)) return fail(DPF_ERR_PARAM, "dpf: ngroups * npts points do not fit 64 bits");
    return DPF_OK;
}

// Device pointers: all present; all aligned to n bytes (a null one is).
template <class... P>
bool present(P... p) {
    return (... && (p != nullptr));
}
template <class... P>
bool aligned(size_t n, P... p) {
    return (... | (uintptr_t)p) % n == 0;
}
inline int null_buffer() { return fail(DPF_ERR_PARAM, "dpf: null device buffer"); }
inline int misaligned_buffer() { return fail(DPF_ERR_PARAM, "dpf: misaligned device buffer"); }

}  // namespace dpfc
