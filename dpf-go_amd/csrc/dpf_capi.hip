// dpf_capi.hip — the C ABI (include/dpf_hip.h) over the gfx950 kernels.
//
// Host-buffer entry points stage keys into HBM, run the kernels on a
// per-device stream under a per-device mutex and copy results back;
// device-resident (_dev) entry points only enqueue on the caller's stream.
// There is no CPU evaluation path: without a usable gfx950 device every
// evaluation call fails with DPF_ERR_NODEV.
//
// What needs no device lives in host-only headers with CPU tests of their
// own: stage_plan.hpp cuts a host-buffer call into the chunks of the staging
// pipeline (chunk sizes, subtree slabs, output offsets), copy_pool.hpp is the
// thread pool of the pinned <-> caller-buffer copies, pir_update_plan.hpp
// plans dpf_pir_db_update / _read, eval_bits_plan.hpp (with tree_plan.hpp, by
// way of the launchers) the Eval into selection bits.  This file keeps the HIP calls: buffers,
// streams, events and launches, and the argument checks of the entry points.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dpf_hip.h"
#include "dpf_internal.hpp"
#include "bs_kernels.hpp"
#include "copy_pool.hpp"
#include "dpf_kernels.hpp"
#include "pir_kernels.hpp"
#include "pir_update_plan.hpp"
#include "stage_plan.hpp"

using dpfh::CopyPool;
using dpfh::full_len;
using dpfh::key_len;
using dpfh::kStageBytes;
using dpfh::stop_of;

namespace {

thread_local std::string t_err;

int fail(int code, const std::string& msg) {
    t_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(DPF_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
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

// Open devices.  Entry points take a snapshot (shared_ptr copies) under
// g_mu, so dpf_gpu_shutdown only drops the registry's references: a call in
// flight, or a PIR handle, keeps its devices alive until it is done with
// them, and the last reference releases the device's buffers and streams.
// The registry is a never-destroyed heap object: a process that exits
// without dpf_gpu_shutdown runs no Dev destructor (so no HIP call) during
// static teardown, whatever the order against the HIP runtime and torch.
std::mutex g_mu;
std::vector<std::shared_ptr<Dev>>& g_devs = *new std::vector<std::shared_ptr<Dev>>();
std::atomic<int> g_ndevs{0};   // g_devs.size(), readable without g_mu (small-call routing)

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

// Streams created by dpf_stream_create_cu_masked and the CUs each may use.
// A _dev entry point launching on one of them sizes its grids to those CUs
// (CuScope); any other stream gets the whole device.
std::mutex g_cus_mu;
std::unordered_map<hipStream_t, int> g_stream_cus;

struct CuScope {
    int prev;
    explicit CuScope(void* stream) : prev(dpfk::cu_budget()) {
        int c = 0;
        if (stream) {
            std::lock_guard<std::mutex> lk(g_cus_mu);
            auto it = g_stream_cus.find((hipStream_t)stream);
            if (it != g_stream_cus.end()) c = it->second;
        }
        dpfk::set_cu_budget(c);
    }
    ~CuScope() { dpfk::set_cu_budget(prev); }
};

Dev::~Dev() {
    std::lock_guard<std::mutex> dl(mu);
    DeviceGuard g(id);
    for (hipStream_t t : {st, cst, hst})
        if (t) (void)hipStreamSynchronize(t);
    keys.release();
    work.release();
    out.release();
    xs.release();
    for (int i = 0; i < 2; ++i) {
        pin[i].release();
        for (hipEvent_t e : {ev_k[i], ev_c[i], ev_h[i]})
            if (e) (void)hipEventDestroy(e);
    }
    for (hipStream_t t : {st, cst, hst})
        if (t) (void)hipStreamDestroy(t);
}

using DevList = std::vector<std::shared_ptr<Dev>>;

int check_gfx950(int ordinal) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, ordinal) != hipSuccess) return fail(DPF_ERR_NODEV, "dpf: device query failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(DPF_ERR_NODEV, std::string("dpf: device is ") + prop.gcnArchName + ", need gfx950");
    return DPF_OK;
}

// Open exactly the HIP ordinals `ids`, or with no ids the first `ngpus`
// visible devices (all if ngpus <= 0).  Caller holds g_mu, registry empty.
int open_list(std::vector<int> ids, int ngpus = 0) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(DPF_ERR_NODEV, "dpf: no HIP device visible (gfx950 required)");
    if (ids.empty())
        for (int i = 0; i < (ngpus > 0 ? std::min(n, ngpus) : n); ++i) ids.push_back(i);
    for (int id : ids) {
        if (id < 0 || id >= n) return fail(DPF_ERR_PARAM, "dpf: device ordinal out of range");
        if (int rc = check_gfx950(id)) return rc;
    }
    DevList devs;
    for (int id : ids) {
        auto d = std::make_shared<Dev>();
        d->id = id;
        DeviceGuard g(id);
        if (hipStreamCreateWithFlags(&d->st, hipStreamNonBlocking) != hipSuccess)
            return fail(DPF_ERR_HIP, "dpf: hipStreamCreate failed");
        devs.push_back(std::move(d));
    }
    g_devs = std::move(devs);
    g_ndevs.store((int)g_devs.size());
    return (int)g_devs.size();
}

int open_devices(int ngpus) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_devs.empty()) return (int)g_devs.size();
    return open_list({}, ngpus);
}

// The opened devices, opening every visible one on first use.  Returns an
// empty list (and sets the error) when none can be opened.
DevList devices(int* rc) {
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if (!g_devs.empty()) {
            *rc = (int)g_devs.size();
            return g_devs;
        }
    }
    *rc = open_devices(0);
    std::lock_guard<std::mutex> lk(g_mu);
    return *rc > 0 ? g_devs : DevList{};
}

// The reference reads k[0:17], the level records k[17+18i : 17+18i+18] for
// i < stop and the final CW at k[len-16 : len] (dpf.go:175-176,186-188,206,
// 219,231-233): any key of at least 17 + 18*stop bytes evaluates without an
// index panic, including keys whose final CW overlaps the last record.
// EvalFull (full) with logN > 63 cannot allocate its 2^(logN-3)-byte output
// (dpf.go:251 panics in makeslice): DPF_ERR_PARAM.  Eval validates no logN
// (dpf.go:171-211): any logN with a long enough key evaluates, its path bits
// above bit 63 read as 0 (path_bit).
int check_key(size_t klen, uint32_t logN, bool full = true) {
    if (full && logN > 63) return fail(DPF_ERR_PARAM, "dpf: logN > 63");
    if (klen < 17 + 18 * (size_t)stop_of(logN)) return fail(DPF_ERR_KEYLEN, "dpf: key shorter than 17+18*(logN-7) bytes");
    return DPF_OK;
}

// ---- AES back end of the tree kernels (configs[1]: bitsliced vs T-table) --
// DPF_AES_IMPL=bitsliced|ttable sets the default; dpf_set_aes_impl switches
// at run time.  Both give bit-identical outputs.
std::atomic<int> g_aes_impl{[] {
    const char* e = getenv("DPF_AES_IMPL");
    return e && (e[0] == 'b' || e[0] == 'B') ? DPF_AES_BITSLICED : DPF_AES_TTABLE;
}()};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Tree workspace for nk expanded keys: [T-table records | byte-sliced CW
// words | byte-sliced frontier for up to `chunk` keys per launch].
size_t tree_ws_bytes(size_t nk, uint32_t stop, uint32_t prefix_bits, size_t chunk) {
    return align256(nk * dpfk::ek_words(stop) * 4) + align256(nk * dpfk::bs_key_words(stop) * 4) +
           dpfk::bs_frontier_bytes(chunk, stop, prefix_bits);
}

struct TreeWs {
    uint32_t* ek;
    uint32_t* ekb;
    void* frontier;
};

TreeWs tree_ws(void* work, size_t nk, uint32_t stop) {
    uint8_t* p = static_cast<uint8_t*>(work);
    TreeWs w;
    w.ek = reinterpret_cast<uint32_t*>(p);
    p += align256(nk * dpfk::ek_words(stop) * 4);
    w.ekb = reinterpret_cast<uint32_t*>(p);
    p += align256(nk * dpfk::bs_key_words(stop) * 4);
    w.frontier = p;
    return w;
}

// Expanded keys at the start of a PIR or batched-Eval workspace, padded to 256 B.
size_t pir_ek_bytes(size_t nkeys, uint32_t logN) { return align256(nkeys * dpfk::ek_words(stop_of(logN)) * 4); }

// Batched-Eval workspace: expanded keys (256-B padded), then the frontier.
size_t eval_work_bytes(size_t nkeys, size_t ppk, uint32_t logN) {
    return pir_ek_bytes(nkeys, logN) + dpfk::eval_frontier_bytes(nkeys, stop_of(logN), ppk);
}

// The back end a call uses, decided once per call (expansion and launches agree).
bool want_bs() { return g_aes_impl.load(std::memory_order_relaxed) == DPF_AES_BITSLICED; }

// Key records: the T-table's 8-word records always; the byte-sliced planes
// (7.6 MB at configs[1], 2/3 of the unpack time) only for the byte-sliced back end.
hipError_t expand_keys(const uint8_t* d_keys, size_t klen, size_t nk, uint32_t stop, const TreeWs& w, hipStream_t st,
                       bool bs) {
    if (bs) return dpfk::launch_unpack_both(d_keys, klen, nk, stop, w.ek, w.ekb, st);
    return dpfk::launch_unpack(d_keys, klen, nk, stop, w.ek, st);
}

// Leaves of subtree (prefix_bits, prefix) of keys [k0, k0 + n): byte-sliced
// when bs (its records expanded) and the subtree is deep enough, else T-table.
hipError_t run_tree(const TreeWs& w, size_t k0, size_t n, uint32_t stop, uint32_t prefix_bits, uint64_t prefix,
                    uint8_t* out, uint64_t stride, hipStream_t st, bool bs) {
    if (bs && dpfk::bs_applicable(stop, prefix_bits))
        return dpfk::launch_evalfull_bs(w.ek + k0 * dpfk::ek_words(stop), w.ekb + k0 * dpfk::bs_key_words(stop), n, stop,
                                        prefix_bits, prefix, out, stride, w.frontier, st);
    return dpfk::launch_evalfull(w.ek + k0 * dpfk::ek_words(stop), n, stop, prefix_bits, prefix, out, stride, st);
}

// The expanded form's layout depends on (nkeys, stop) (tree_ws), so each
// expanded workspace is recorded here and dpf_evalfull_expanded_dev refuses
// one expanded for another shape instead of reading misplaced records.
std::mutex g_exp_mu;
// Also records whether the byte-sliced planes were built: the T-table back
// end expands only its own records, and switching to the byte-sliced one
// later derives them from those (launch_bs_from_ek) on first use.
struct Expanded {
    size_t nkeys;
    uint32_t stop;
    bool bs;
};
std::unordered_map<const void*, Expanded>& g_expanded = *new std::unordered_map<const void*, Expanded>();

// Every entry point that expands keys into a caller's d_work records what it
// left there (the same tree_ws layout), so a later dpf_evalfull_expanded_dev
// never reads planes built from other keys; dpf_eval_batch_dev's workspace
// has another layout past the records and is dropped.
void note_expanded(const void* d_work, size_t nkeys, uint32_t stop, bool bs) {
    std::lock_guard<std::mutex> lk(g_exp_mu);
    g_expanded[d_work] = {nkeys, stop, bs};
}
void forget_expanded(const void* d_work) {
    std::lock_guard<std::mutex> lk(g_exp_mu);
    g_expanded.erase(d_work);
}

// One-shot tree pass from the key bytes in HBM, with a caller's d_work:
// straight from the bytes when the T-table back end runs a wave-uniform shape
// (dpfk::evalfull_raw_ok: no unpack launch, d_work untouched and its record
// dropped), else expand into d_work, run, and record what d_work now holds.
hipError_t tree_from_keys(const uint8_t* d_keys, size_t klen, size_t nk, uint32_t stop, uint32_t prefix_bits,
                          uint64_t prefix, uint8_t* out, uint64_t stride, void* d_work, hipStream_t st, bool bs) {
    forget_expanded(d_work);
    if (!bs && dpfk::evalfull_raw_ok(nk, stop, prefix_bits))
        return dpfk::launch_evalfull_raw(d_keys, klen, nk, stop, prefix_bits, prefix, out, stride, st);
    const TreeWs w = tree_ws(d_work, nk, stop);
    hipError_t e = expand_keys(d_keys, klen, nk, stop, w, st, bs);
    if (e == hipSuccess) e = run_tree(w, 0, nk, stop, prefix_bits, prefix, out, stride, st, bs);
    if (e == hipSuccess) note_expanded(d_work, nk, stop, bs);
    return e;
}

// Staging of the pipelined host-buffer paths: two device slots of chunk_cap
// bytes in d.out, two pinned slots of pin_off + chunk_cap bytes.
int ensure_staging(Dev& d, size_t chunk_cap, size_t pin_off) {
    if (!d.cst) {
        HIP_TRY(hipStreamCreateWithFlags(&d.cst, hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) {
            HIP_TRY(hipEventCreateWithFlags(&d.ev_k[i], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&d.ev_c[i], hipEventDisableTiming));
        }
    }
    HIP_TRY(d.out.ensure(2 * chunk_cap));
    for (int i = 0; i < 2; ++i) HIP_TRY(d.pin[i].ensure(pin_off + chunk_cap));
    return DPF_OK;
}

// Opt-in (DPF_PREFAULT_OUTPUT=1): for large caller buffers (a fresh Go
// slice / numpy array), ask for transparent huge pages and pre-touch the
// pages in parallel while the GPU works, so first touch costs one fault per
// 2 MiB instead of per 4 KiB inside the copy.  Off by default: it changes
// the memory policy of caller-owned memory (a Go heap manages THP itself)
// and zero-writes the buffer before data arrives.
bool prefault_output() {
    static const bool on = [] {
        const char* e = getenv("DPF_PREFAULT_OUTPUT");
        return e && e[0] == '1';
    }();
    return on;
}

void hint_hugepages(uint8_t* p, size_t n) {
    if (n < ((size_t)64 << 20) || !prefault_output()) return;
    const uintptr_t a = ((uintptr_t)p + ((1u << 21) - 1)) & ~(uintptr_t)((1u << 21) - 1);
    const uintptr_t e = ((uintptr_t)p + n) & ~(uintptr_t)((1u << 21) - 1);
    if (e > a) (void)madvise((void*)a, e - a, MADV_HUGEPAGE);
}

// Pipelined device -> host output of `nchunks` chunks (<= chunk_cap bytes
// each; the plans of stage_plan.hpp).  produce(i, dbuf, bytes, host_off)
// enqueues the kernels writing chunk i into device slot dbuf on d.st.  Kernel
// i, the PCIe copy of chunk i-1 (d.cst, into a pinned slot) and the host copy
// of chunk i-2 (pinned -> caller buffer, CopyPool) overlap; two device and two
// pinned slots.  Chunk i lands at out + off_i - out_base; [out, out +
// out_bytes) is the whole destination.  Results sit pin_off bytes into a
// pinned slot: the bytes before them are produce's (batched Eval's points).
template <class Produce>
int pipeline_d2h(Dev& d, size_t nchunks, size_t chunk_cap, Produce produce, uint8_t* out, size_t out_bytes,
                 size_t out_base = 0, size_t pin_off = 0) {
    if (nchunks == 0) return DPF_OK;
    hint_hugepages(out, out_bytes);
    if (int rc = ensure_staging(d, chunk_cap, pin_off)) return rc;
    size_t bytes[2] = {0, 0}, off[2] = {0, 0};
    auto drain = [&](size_t i) -> int {              // chunk i: wait for its PCIe copy, then host copy
        const int s = (int)(i & 1);
        HIP_TRY(hipEventSynchronize(d.ev_c[s]));
        CopyPool::get().memcpy_par(out + (off[s] - out_base), (uint8_t*)d.pin[s].p + pin_off, bytes[s]);
        return DPF_OK;
    };
    for (size_t i = 0; i < nchunks; ++i) {
        const int s = (int)(i & 1);
        uint8_t* dbuf = (uint8_t*)d.out.p + (size_t)s * chunk_cap;
        if (i >= 2) HIP_TRY(hipStreamWaitEvent(d.st, d.ev_c[s], 0));   // slot's previous PCIe copy done
        if (int rc = produce(i, dbuf, bytes[s], off[s])) return rc;
        HIP_TRY(hipEventRecord(d.ev_k[s], d.st));
        HIP_TRY(hipStreamWaitEvent(d.cst, d.ev_k[s], 0));
        HIP_TRY(hipMemcpyAsync((uint8_t*)d.pin[s].p + pin_off, dbuf, bytes[s], hipMemcpyDeviceToHost, d.cst));
        HIP_TRY(hipEventRecord(d.ev_c[s], d.cst));
        if (i == std::min<size_t>(1, nchunks - 1) && out_bytes >= ((size_t)64 << 20) && prefault_output())
            CopyPool::get().prefault_par(out, out_bytes);   // while the GPU works on chunks 0-1
        if (i >= 1)
            if (int rc = drain(i - 1)) return rc;          // frees pinned slot (i-1)&1 for chunk i+1
    }
    return drain(nchunks - 1);
}

// Host-buffer EvalFull of one device's plan (dpfh::full_plan: groups of whole
// keys or subtree slabs; dpfh::split_plan: this device's subtree of one key)
// into the caller's whole buffer `out`.  Every chunk runs straight from the
// key bytes when each launch shape of the plan allows it (dpfk::
// evalfull_raw_ok), else the keys are expanded once for all chunks.
int full_on_device(Dev& d, const uint8_t* keys, size_t klen, uint32_t logN, const dpfh::FullPlan& plan, uint8_t* out) {
    std::lock_guard<std::mutex> lk(d.mu);
    DeviceGuard g(d.id);
    const uint32_t stop = stop_of(logN);
    const size_t nk = plan.nk;
    HIP_TRY(d.keys.ensure(nk * klen));
    HIP_TRY(d.work.ensure(tree_ws_bytes(nk, stop, plan.split_bits, std::min(plan.per, nk))));
    HIP_TRY(hipMemcpyAsync(d.keys.p, keys, nk * klen, hipMemcpyHostToDevice, d.st));
    const TreeWs w = tree_ws(d.work.p, nk, stop);
    const bool bs = want_bs();
    const uint8_t* dk = (const uint8_t*)d.keys.p;
    bool raw = !bs;
    for (size_t i = 0; raw && i < plan.nshapes; ++i)
        raw = dpfk::evalfull_raw_ok(plan.shape[i].nkeys, stop, plan.shape[i].prefix_bits);
    if (!raw) HIP_TRY(expand_keys(dk, klen, nk, stop, w, d.st, bs));
    return pipeline_d2h(d, plan.nchunks, plan.cap, [&](size_t i, uint8_t* dbuf, size_t& bytes, size_t& off) {
        const dpfh::FullChunk c = plan.chunk(i);
        const uint64_t stride = plan.olen >> c.prefix_bits;   // one key's bytes of this subtree
        if (raw)
            HIP_TRY(dpfk::launch_evalfull_raw(dk + c.k0 * klen, klen, c.n, stop, c.prefix_bits, c.prefix, dbuf, stride,
                                              d.st));
        else
            HIP_TRY(run_tree(w, c.k0, c.n, stop, c.prefix_bits, c.prefix, dbuf, stride, d.st, bs));
        bytes = c.bytes;
        off = c.off;
        return DPF_OK;
    }, out + plan.out_base, plan.out_bytes, plan.out_base);
}

// Host-buffer batched Eval on one device, pipelined over chunks of keys
// (dpfh::eval_plan): caller xs -> pinned (CopyPool) -> HBM (d.hst) -> the Eval
// kernels (d.st) -> pinned (d.cst) -> caller out, two slots per stage, so
// chunk i's kernel overlaps the PCIe copies of its neighbours.  A pinned slot
// holds [xs qcap*8][results qcap].
int eval_on_device(Dev& d, const uint8_t* keys, size_t klen, size_t nk, const uint64_t* xs, size_t ppk,
                   uint32_t logN, uint8_t* out) {
    std::lock_guard<std::mutex> lk(d.mu);
    DeviceGuard g(d.id);
    const uint32_t stop = stop_of(logN);
    const size_t ekw = dpfk::ek_words(stop);
    const dpfh::EvalPlan plan = dpfh::eval_plan(nk, ppk);
    const size_t qcap = plan.qcap, ekb = pir_ek_bytes(nk, logN);
    const size_t fbytes = dpfk::eval_frontier_bytes(plan.per, stop, ppk);
    HIP_TRY(d.keys.ensure(std::max<size_t>(1, nk * klen)));
    HIP_TRY(d.work.ensure(std::max<size_t>(16, ekb + fbytes)));
    HIP_TRY(d.xs.ensure(2 * qcap * 8));
    if (!d.hst) {
        HIP_TRY(hipStreamCreateWithFlags(&d.hst, hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) HIP_TRY(hipEventCreateWithFlags(&d.ev_h[i], hipEventDisableTiming));
    }
    HIP_TRY(hipMemcpyAsync(d.keys.p, keys, nk * klen, hipMemcpyHostToDevice, d.st));
    HIP_TRY(dpfk::launch_unpack((const uint8_t*)d.keys.p, klen, nk, stop, (uint32_t*)d.work.p, d.st));
    const uint32_t* ek = (const uint32_t*)d.work.p;
    void* frontier = (uint8_t*)d.work.p + ekb;
    return pipeline_d2h(d, plan.nchunks, qcap, [&](size_t i, uint8_t* dout, size_t& bytes, size_t& off) {
        const int s = (int)(i & 1);
        const size_t k0 = plan.k0(i), q = plan.n(i) * ppk;
        uint64_t* dxs = (uint64_t*)d.xs.p + (size_t)s * qcap;
        CopyPool::get().memcpy_par(d.pin[s].p, xs + k0 * ppk, q * 8);
        if (i >= 2) HIP_TRY(hipStreamWaitEvent(d.hst, d.ev_k[s], 0));   // slot's previous kernel read its xs
        HIP_TRY(hipMemcpyAsync(dxs, d.pin[s].p, q * 8, hipMemcpyHostToDevice, d.hst));
        HIP_TRY(hipEventRecord(d.ev_h[s], d.hst));
        HIP_TRY(hipStreamWaitEvent(d.st, d.ev_h[s], 0));
        HIP_TRY(dpfk::launch_eval(ek + k0 * ekw, stop, logN, dxs, q, ppk, dout, frontier, fbytes, d.st));
        bytes = q;
        off = k0 * ppk;
        return DPF_OK;
    }, out, nk * ppk, 0, qcap * 8);
}

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

// The first min(ngpus, opened) devices (ngpus <= 0: all); empty + error set on failure.
DevList pick_devs(int ngpus, int* rc) {
    DevList devs = devices(rc);
    if (*rc <= 0) return {};
    if (ngpus > 0 && (size_t)ngpus < devs.size()) devs.resize((size_t)ngpus);
    *rc = (int)devs.size();
    return devs;
}

}  // namespace

extern "C" {

const char* dpf_last_error(void) { return t_err.c_str(); }

size_t dpf_key_len(uint32_t logN) { return key_len(logN); }
size_t dpf_evalfull_len(uint32_t logN) { return full_len(logN); }
size_t dpf_workspace_size(size_t nkeys, uint32_t logN) {
    return std::max<size_t>(16, tree_ws_bytes(nkeys, stop_of(logN), 0, nkeys));
}

int dpf_set_aes_impl(int impl) {
    if (impl != DPF_AES_TTABLE && impl != DPF_AES_BITSLICED) return fail(DPF_ERR_PARAM, "dpf: unknown AES back end");
    return g_aes_impl.exchange(impl);
}

int dpf_get_aes_impl(void) { return g_aes_impl.load(); }

int dpf_set_eval_kernel(int kernel) {
    if (kernel != DPF_EVAL_WALK && kernel != DPF_EVAL_TRIE) return fail(DPF_ERR_PARAM, "dpf: unknown Eval kernel");
    if (kernel == DPF_EVAL_TRIE && !dpfk::eval_trie_built())
        return fail(DPF_ERR_PARAM, "dpf: the trie Eval kernel is not in this build (make -C dpf-go_amd experimental)");
    return dpfk::set_eval_trie(kernel == DPF_EVAL_TRIE) ? DPF_EVAL_TRIE : DPF_EVAL_WALK;
}

int dpf_get_eval_kernel(void) { return dpfk::get_eval_trie() ? DPF_EVAL_TRIE : DPF_EVAL_WALK; }

int dpf_aes_mmo_dev(int device, int impl, int right, const uint8_t* d_in, uint8_t* d_out, size_t nblocks,
                    uint32_t reps, void* stream) {
    if (impl != DPF_AES_TTABLE && impl != DPF_AES_BITSLICED) return fail(DPF_ERR_PARAM, "dpf: unknown AES back end");
    if (nblocks % 8) return fail(DPF_ERR_PARAM, "dpf: nblocks must be a multiple of 8");
    DeviceGuard g(device);
    if (impl == DPF_AES_BITSLICED)
        HIP_TRY(dpfk::launch_mmo_bs(d_in, d_out, nblocks, right ? 1u : 0u, reps, (hipStream_t)stream));
    else
        HIP_TRY(dpfk::launch_mmo_tt(d_in, d_out, nblocks, right ? 1u : 0u, reps, (hipStream_t)stream));
    return DPF_OK;
}

int dpf_gpu_init(int ngpus) { return open_devices(ngpus); }

int dpf_gpu_init_devices(const int* ordinals, int n) {
    if (n <= 0 || ordinals == nullptr) return fail(DPF_ERR_PARAM, "dpf: empty device list");
    std::vector<int> ids(ordinals, ordinals + n);
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_devs.empty()) {
        bool same = g_devs.size() == ids.size();
        for (size_t i = 0; same && i < ids.size(); ++i) same = g_devs[i]->id == ids[i];
        if (!same) return fail(DPF_ERR_PARAM, "dpf: already initialised with other devices (dpf_gpu_shutdown first)");
        return (int)g_devs.size();
    }
    return open_list(ids);
}

void dpf_gpu_shutdown(void) {
    DevList old;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        old.swap(g_devs);
        g_ndevs.store(0);
    }
    // Dropping the registry's references; a device still used by an
    // in-flight call or a PIR handle is released when that lets go.
}

int dpf_gpu_count(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    return (int)g_devs.size();
}

int dpf_gen_seeded(uint64_t alpha, uint32_t logN, const uint8_t s0[16], const uint8_t s1[16], uint8_t* ka,
                   uint8_t* kb) {
    int rc = dpfh::gen_seeded(alpha, logN, s0, s1, ka, kb);
    return rc ? fail(rc, "dpf: invalid parameters") : DPF_OK;
}

int dpf_gen(uint64_t alpha, uint32_t logN, uint8_t* ka, uint8_t* kb) {
    int rc = dpfh::gen_random(alpha, logN, ka, kb);
    return rc ? fail(rc, "dpf: invalid parameters") : DPF_OK;
}

int dpf_gen_batch_seeded(const uint64_t* alphas, uint32_t logN, const uint8_t* s0s, const uint8_t* s1s, size_t n,
                         uint8_t* kas, uint8_t* kbs, int nthreads) {
    int rc = dpfh::gen_batch_seeded(alphas, logN, s0s, s1s, n, kas, kbs, nthreads);
    return rc ? fail(rc, "dpf: invalid parameters") : DPF_OK;
}

int dpf_keys_pack(const uint8_t* const* keys, const size_t* lens, size_t n, size_t key_len, uint8_t* out) {
    int rc = dpfh::keys_pack(keys, lens, n, key_len, out);
    return rc == DPF_ERR_KEYLEN ? fail(rc, "dpf: key length differs from the batch's key_len")
           : rc                ? fail(rc, "dpf: invalid parameters")
                               : DPF_OK;
}

int dpf_keys_unpack(const uint8_t* packed, size_t key_len, size_t n, uint8_t* const* keys) {
    int rc = dpfh::keys_unpack(packed, key_len, n, keys);
    return rc ? fail(rc, "dpf: invalid parameters") : DPF_OK;
}

int dpf_evalfull_batch(const uint8_t* keys, size_t klen, size_t nkeys, uint32_t logN, uint8_t* out, int ngpus) {
    if (int rc = check_key(klen, logN)) return rc;
    if (nkeys == 0) return DPF_OK;
    int g = 0;
    const DevList devs = pick_devs(ngpus, &g);
    if (g <= 0) return g;
    const size_t olen = full_len(logN);
    return shard(nkeys, g, [&](int dev, size_t lo, size_t hi) {
        return full_on_device(*devs[(size_t)dev], keys + lo * klen, klen, logN, dpfh::full_plan(hi - lo, logN),
                              out + lo * olen);
    });
}

// ---- small-call path (host_eval.cpp) ------------------------
std::atomic<int> g_small_mode{[] {
    const char* e = getenv("DPF_SMALL_CALLS");
    if (!e) return DPF_SMALL_AUTO;
    if (e[0] == 'g' || e[0] == 'G') return DPF_SMALL_GPU;
    if (e[0] == 'h' || e[0] == 'H') return DPF_SMALL_HOST;
    return DPF_SMALL_AUTO;
}()};

// Largest logN whose single-key EvalFull goes to the host in AUTO mode: up
// to it, one key's host EvalFull (3*2^(logN-7) AES on VAES) is faster than
// the GPU round trip (key H2D, launch, output D2H, sync) -- measured on the
// GPU box's EPYC (profiles/r03/small_calls; r05: host 69 us vs GPU 89 us at
// 21, 137 vs 105 at 22, profiles/r05/small_calls/small_vaes.json).
constexpr uint32_t kSmallFullMaxLogN = 21;
// Without VAES (DPF_HOST_ISA=aesni: two 128-bit AES-NI chains per node) the
// host path is ~2x slower at these sizes; measured crossover logN = 20: host
// 72 us vs GPU 83 us at 20, 138 vs 100 at 21
// (profiles/r05/small_calls/small_aesni.json; r04's 19 was an estimate).
constexpr uint32_t kSmallFullMaxLogNNoVaes = 20;
// DPF_SMALL_HOST's ceiling: two host-side levels of the full width (~2.1x the
// output) and one core; above it the call goes to the GPU.
constexpr uint32_t kHostFullMaxLogN = 28;
uint32_t small_full_max() { return dpfh::host_eval_vaes() ? kSmallFullMaxLogN : kSmallFullMaxLogNNoVaes; }

int dpf_set_small_call_path(int mode) {
    if (mode != DPF_SMALL_AUTO && mode != DPF_SMALL_GPU && mode != DPF_SMALL_HOST)
        return fail(DPF_ERR_PARAM, "dpf: unknown small-call mode");
    return g_small_mode.exchange(mode);
}
int dpf_get_small_call_path(void) { return g_small_mode.load(); }
uint32_t dpf_small_call_max_logN(void) { return small_full_max(); }

// Route a single call to the host?  Only with a gfx950 device open (so the
// host path is never a stand-in for a missing GPU) and AES-NI present.
// Returns 1 = host, 0 = GPU, < 0 = error (no device).
int route_host(bool full, uint32_t logN) {
    const int mode = g_small_mode.load(std::memory_order_relaxed);
    if (mode == DPF_SMALL_GPU || !dpfh::host_eval_available()) return 0;
    if (g_ndevs.load(std::memory_order_acquire) <= 0) {   // open on first use, as the GPU path would
        int g = 0;
        (void)pick_devs(1, &g);
        if (g <= 0) return g;
    }
    if (mode == DPF_SMALL_HOST) return !full || logN <= kHostFullMaxLogN ? 1 : 0;
    return !full || logN <= small_full_max() ? 1 : 0;
}

int dpf_evalfull(const uint8_t* key, size_t klen, uint32_t logN, uint8_t* out) {
    if (int rc = check_key(klen, logN)) return rc;
    const int h = route_host(true, logN);
    if (h < 0) return h;
    if (h) {
        try {
            dpfh::evalfull_host(key, klen, logN, out);
        } catch (const std::bad_alloc&) {
            return fail(DPF_ERR_NOMEM, "dpf: host EvalFull allocation failed");
        }
        return DPF_OK;
    }
    return dpf_evalfull_batch(key, klen, 1, logN, out, 1);
}

int dpf_eval_batch(const uint8_t* keys, size_t klen, size_t nkeys, const uint64_t* xs, size_t ppk, uint32_t logN,
                   uint8_t* out, int ngpus) {
    if (int rc = check_key(klen, logN, false)) return rc;
    if (nkeys == 0 || ppk == 0) return DPF_OK;
    int g = 0;
    const DevList devs = pick_devs(ngpus, &g);
    if (g <= 0) return g;
    return shard(nkeys, g, [&](int dev, size_t lo, size_t hi) {
        return eval_on_device(*devs[(size_t)dev], keys + lo * klen, klen, hi - lo, xs + lo * ppk, ppk, logN,
                              out + lo * ppk);
    });
}

int dpf_eval(const uint8_t* key, size_t klen, uint64_t x, uint32_t logN, uint8_t* out_bit) {
    if (int rc = check_key(klen, logN, false)) return rc;
    const int h = route_host(false, logN);
    if (h < 0) return h;
    if (h) {
        dpfh::eval_batch_host(key, klen, 1, &x, 1, logN, out_bit);
        return DPF_OK;
    }
    return dpf_eval_batch(key, klen, 1, &x, 1, logN, out_bit, 1);
}

int dpf_evalfull_split(const uint8_t* key, size_t klen, uint32_t logN, uint8_t* out, int ngpus) {
    if (int rc = check_key(klen, logN)) return rc;
    int have = 0;
    const DevList devs = pick_devs(0, &have);
    if (have <= 0) return have;
    const int want = ngpus <= 0 ? have : ngpus;
    if (want > have) return fail(DPF_ERR_PARAM, "dpf: more GPUs requested than opened");
    uint32_t pb = 0;
    if (!dpfh::gpus_to_pb(want, stop_of(logN), &pb))
        return fail(DPF_ERR_PARAM, "dpf: ngpus must be a power of two <= 2^(logN-7)");
    return shard((size_t)want, want, [&](int dev, size_t lo, size_t hi) {
        (void)hi;
        return full_on_device(*devs[(size_t)dev], key, klen, logN, dpfh::split_plan(logN, pb, lo), out);
    });
}

int dpf_evalfull_subtree_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                             uint32_t prefix_bits, uint64_t prefix, uint8_t* d_out, void* d_work, void* stream) {
    if (int rc = check_key(klen, logN)) return rc;
    const uint32_t stop = stop_of(logN);
    if (!dpfh::prefix_ok(prefix_bits, prefix, stop)) return fail(DPF_ERR_PARAM, "dpf: subtree prefix out of range");
    if (nkeys == 0) return DPF_OK;
    DeviceGuard g(device);
    CuScope cus(stream);
    HIP_TRY(tree_from_keys(d_keys, klen, nkeys, stop, prefix_bits, prefix, d_out, (uint64_t)16 << (stop - prefix_bits),
                           d_work, (hipStream_t)stream, want_bs()));
    return DPF_OK;
}

int dpf_evalfull_batch_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                           uint8_t* d_out, void* d_work, void* stream) {
    return dpf_evalfull_subtree_dev(device, d_keys, klen, nkeys, logN, 0, 0, d_out, d_work, stream);
}

size_t dpf_eval_workspace_size(size_t nkeys, size_t pts_per_key, uint32_t logN) {
    return std::max<size_t>(16, eval_work_bytes(nkeys, pts_per_key, logN));
}

uint32_t dpf_eval_frontier_level(uint32_t logN, size_t pts_per_key) {
    return logN > 63 ? 0 : dpfk::eval_frontier_level(stop_of(logN), pts_per_key);   // launch_eval: no frontier above 63
}

int dpf_eval_batch_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, const uint64_t* d_xs,
                       size_t ppk, uint32_t logN, uint8_t* d_out, void* d_work, size_t work_bytes, void* stream) {
    if (int rc = check_key(klen, logN, false)) return rc;
    if (nkeys == 0 || ppk == 0) return DPF_OK;
    const uint32_t stop = stop_of(logN);
    const size_t ekb = pir_ek_bytes(nkeys, logN);
    if (work_bytes < nkeys * dpfk::ek_words(stop) * 4) return fail(DPF_ERR_PARAM, "dpf: Eval workspace too small");
    if (d_xs == nullptr || d_out == nullptr || d_keys == nullptr || (reinterpret_cast<uintptr_t>(d_xs) & 7u) != 0)
        return fail(DPF_ERR_PARAM, "dpf: d_keys/d_xs/d_out must be device pointers, d_xs 8-byte aligned");
    DeviceGuard g(device);
    CuScope cus(stream);
    forget_expanded(d_work);
    HIP_TRY(dpfk::launch_unpack(d_keys, klen, nkeys, stop, (uint32_t*)d_work, (hipStream_t)stream));
    // The frontier (if it fits in the rest of the workspace) lets queries share the tree's top levels.
    void* frontier = work_bytes > ekb ? (uint8_t*)d_work + ekb : nullptr;
    HIP_TRY(dpfk::launch_eval((const uint32_t*)d_work, stop, logN, d_xs, nkeys * ppk, ppk, d_out, frontier,
                              work_bytes > ekb ? work_bytes - ekb : 0, (hipStream_t)stream));
    return DPF_OK;
}

size_t dpf_eval_bits_stride(size_t npts) { return dpfh::eval_bits_stride(npts); }

size_t dpf_eval_bits_workspace_size(size_t nkeys, size_t npts, uint32_t logN) {
    return dpf_eval_workspace_size(nkeys, npts, logN);
}

// Every argument check of dpf_eval_bits_dev, in the order it reports; no
// device call.
static int check_eval_bits(const void* d_keys, size_t klen, size_t nkeys, const void* d_xs, size_t npts, uint32_t logN,
                           const void* d_bits, size_t bits_stride, const void* d_work, size_t work_bytes) {
    if (int rc = check_key(klen, logN, false)) return rc;
    if (bits_stride % 16 != 0 || bits_stride < dpfh::eval_bits_stride(npts))
        return fail(DPF_ERR_PARAM, "dpf: bits_stride must be a multiple of 16, at least dpf_eval_bits_stride(npts)");
    if ((uintptr_t)d_xs % 8 != 0 || ((uintptr_t)d_bits | (uintptr_t)d_work) % 16 != 0)
        return fail(DPF_ERR_PARAM, "dpf: misaligned device buffer");
    if (nkeys == 0 || npts == 0) return DPF_OK;
    if (!d_keys || !d_xs || !d_bits || !d_work) return fail(DPF_ERR_PARAM, "dpf: null device buffer");
    if (work_bytes < nkeys * dpfk::ek_words(stop_of(logN)) * 4)
        return fail(DPF_ERR_PARAM, "dpf: Eval workspace too small");
    return DPF_OK;
}

// The launches of dpf_eval_bits_dev, arguments checked: the caller holds the
// device and CU scopes.
static hipError_t eval_bits_launch(const uint8_t* d_keys, size_t klen, size_t nkeys, const uint64_t* d_xs, size_t npts,
                                   uint32_t logN, uint8_t* d_bits, size_t bits_stride, void* d_work, size_t work_bytes,
                                   hipStream_t st) {
    const uint32_t stop = stop_of(logN);
    const size_t ekb = pir_ek_bytes(nkeys, logN);
    forget_expanded(d_work);
    hipError_t e = dpfk::launch_unpack(d_keys, klen, nkeys, stop, (uint32_t*)d_work, st);
    if (e != hipSuccess) return e;
    void* frontier = work_bytes > ekb ? (uint8_t*)d_work + ekb : nullptr;
    return dpfk::launch_eval_bits((const uint32_t*)d_work, stop, logN, d_xs, nkeys, npts, d_bits, bits_stride, frontier,
                                  work_bytes > ekb ? work_bytes - ekb : 0, st);
}

int dpf_eval_bits_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, const uint64_t* d_xs, size_t npts,
                      uint32_t logN, uint8_t* d_bits, size_t bits_stride, void* d_work, size_t work_bytes,
                      void* stream) {
    if (int rc = check_eval_bits(d_keys, klen, nkeys, d_xs, npts, logN, d_bits, bits_stride, d_work, work_bytes))
        return rc;
    if (nkeys == 0 || npts == 0) return DPF_OK;
    DeviceGuard g(device);
    CuScope cus(stream);
    HIP_TRY(eval_bits_launch(d_keys, klen, nkeys, d_xs, npts, logN, d_bits, bits_stride, d_work, work_bytes,
                             (hipStream_t)stream));
    return DPF_OK;
}

// Introspection: the launchers' own plans (tree_plan.hpp) as plain C structs.
static dpf_tree_form c_form(const dpfh::TreeForm& t) {
    dpf_tree_form f;
    memset(&f, 0, sizeof f);
    f.d = t.d;
    f.block = t.block;
    f.w = t.W;
    f.ltop = t.ltop;
    f.units_log = t.units_log;
    f.walk = (uint32_t)t.walk;
    f.l1 = t.l1;
    f.uniform = t.uniform;
    f.nodes = t.nodes;
    f.raw = t.raw;
    f.cw_lds = t.cw_lds;
    f.feedback = t.feedback;
    f.prio_small = t.prio_small;
    f.nunits = t.nunits;
    f.grid = t.grid;
    f.sub_base = t.sub_base;
    return f;
}
static uint64_t form_cus(int cus) { return (uint64_t)(cus > 0 ? cus : dpfk::cu_count()); }

int dpf_tree_form_for(size_t nkeys, uint32_t logN, uint32_t prefix_bits, uint32_t node_level, int cus,
                      dpf_tree_form* form) {
    if (form == nullptr || logN > 63) return fail(DPF_ERR_PARAM, "dpf: form query out of range");
    const uint32_t stop = stop_of(logN);
    const bool nodes = node_level != 0;
    const uint32_t depth = nodes ? node_level : stop;
    if (depth > stop || prefix_bits > depth) return fail(DPF_ERR_PARAM, "dpf: form query out of range");
    const dpfh::TreeKnobs& k = dpfk::tree_knobs();
    const uint64_t c = form_cus(cus);
    const bool raw = !nodes && dpfh::evalfull_raw_ok(nkeys, stop, prefix_bits, c, k);
    dpfh::TreeForm t;
    if (!dpfh::tree_form(nkeys, depth, prefix_bits, 0, nodes, raw, c, k.forced_depth, &t))
        return fail(DPF_ERR_PARAM, "dpf: tree launch refused: more than 2^31 - 1 workgroups");
    *form = c_form(t);
    return DPF_OK;
}

int dpf_eval_form_for(size_t nkeys, size_t ppk, uint32_t logN, size_t work_bytes, int xs_aligned16, int cus,
                      dpf_eval_form* form) {
    if (form == nullptr || logN > 4096 || nkeys == 0 || ppk == 0)
        return fail(DPF_ERR_PARAM, "dpf: form query out of range");
    const uint32_t stop = stop_of(logN);
    const size_t ekb = pir_ek_bytes(nkeys, logN);
    if (work_bytes < nkeys * dpfk::ek_words(stop) * 4) return fail(DPF_ERR_PARAM, "dpf: Eval workspace too small");
    dpfh::EvalForm e;
    if (!dpfh::eval_form((uint64_t)nkeys * ppk, ppk, stop, logN, work_bytes > ekb ? work_bytes - ekb : 0,
                         xs_aligned16 != 0, form_cus(cus), dpfk::tree_knobs(), &e))
        return fail(DPF_ERR_PARAM, "dpf: Eval launch refused: more than 2^31 - 1 workgroups");
    memset(form, 0, sizeof *form);
    form->level = e.L;
    form->kernel = (uint32_t)e.kernel;
    form->block = e.block;
    form->grid = e.grid;
    form->cw_staged = e.cw_staged;
    form->ragged = e.ragged;
    if (e.L > 0) form->nodes = c_form(e.nodes);
    if (e.L > 0 && dpfk::get_eval_trie() && dpfk::eval_trie_ok(stop, logN, ppk, e.L)) {
        form->kernel = DPF_EVAL_TRIE_KERNEL;   // launch_eval: the trie kernel takes the queries
        form->block = 0;
        form->grid = 0;
        form->cw_staged = form->ragged = 0;
    }
    return DPF_OK;
}

int dpf_expand_keys_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN, void* d_work,
                        void* stream) {
    if (int rc = check_key(klen, logN)) return rc;
    DeviceGuard g(device);
    CuScope cus(stream);
    const bool bs = want_bs();
    forget_expanded(d_work);
    HIP_TRY(expand_keys(d_keys, klen, nkeys, stop_of(logN), tree_ws(d_work, nkeys, stop_of(logN)), (hipStream_t)stream,
                        bs));
    note_expanded(d_work, nkeys, stop_of(logN), bs);
    return DPF_OK;
}

int dpf_forget_workspace(const void* d_work) {
    forget_expanded(d_work);
    return DPF_OK;
}

int dpf_evalfull_expanded_dev(int device, void* d_work, size_t nkeys, uint32_t logN, uint32_t prefix_bits,
                              uint64_t prefix, uint8_t* d_out, void* stream) {
    if (logN > 63) return fail(DPF_ERR_PARAM, "dpf: logN > 63");
    const uint32_t stop = stop_of(logN);
    if (!dpfh::prefix_ok(prefix_bits, prefix, stop)) return fail(DPF_ERR_PARAM, "dpf: subtree prefix out of range");
    if (nkeys == 0) return DPF_OK;
    const bool bs = want_bs();
    bool build_bs = false;
    {
        std::lock_guard<std::mutex> lk(g_exp_mu);
        const auto it = g_expanded.find(d_work);
        if (it == g_expanded.end() || it->second.nkeys != nkeys || it->second.stop != stop)
            return fail(DPF_ERR_PARAM, "dpf: d_work was not expanded by dpf_expand_keys_dev for this nkeys and logN");
        build_bs = bs && !it->second.bs;
    }
    DeviceGuard g(device);
    CuScope cus(stream);
    const TreeWs w = tree_ws(d_work, nkeys, stop);
    if (build_bs) {
        HIP_TRY(dpfk::launch_bs_from_ek(w.ek, nkeys, stop, w.ekb, (hipStream_t)stream));
        note_expanded(d_work, nkeys, stop, true);   // only once the planes' launch is enqueued
    }
    const uint64_t stride = (uint64_t)16 << (stop - prefix_bits);
    HIP_TRY(run_tree(w, 0, nkeys, stop, prefix_bits, prefix, d_out, stride, (hipStream_t)stream, bs));
    return DPF_OK;
}

// ------------------------------------------------------------------ PIR ---

// Device buffers of the PIR answer entry points: present when there is work
// for them, and aligned as the kernels access them (DB 16 B, answers and
// workspace as u32 words), so a bad buffer is DPF_ERR_PARAM, not a GPU fault.
static int check_pir_bufs(const void* d_keys, size_t nkeys, const void* d_db, uint64_t nrec, const void* d_ans,
                          const void* d_work) {
    if (nkeys > 0 && (!d_keys || !d_ans || !d_work || (nrec > 0 && !d_db)))
        return fail(DPF_ERR_PARAM, "dpf: null device buffer");
    if ((uintptr_t)d_db % 16 != 0 || (uintptr_t)d_ans % 4 != 0 || (uintptr_t)d_work % 16 != 0)
        return fail(DPF_ERR_PARAM, "dpf: misaligned device buffer");
    return DPF_OK;
}

size_t dpf_pir_workspace_size(size_t nkeys, uint32_t logN, uint32_t prefix_bits) {
    const uint32_t stop = stop_of(logN);
    const uint32_t pb = prefix_bits > stop ? stop : prefix_bits;
    return align256(tree_ws_bytes(nkeys, stop, pb, nkeys)) + align256(nkeys * ((size_t)16 << (stop - pb))) +
           dpfk::pir_fold_parts_bytes();
}

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

// The 32-byte record forms are the _wide forms at rec_bytes = 32.
size_t dpf_pir_db_sliced_size(uint64_t nrec) { return dpf_pir_db_sliced_size_wide(nrec, 32); }

int dpf_pir_db_slice_dev(int device, const uint8_t* d_db, uint64_t nrec, uint8_t* d_dbs, void* stream) {
    return dpf_pir_db_slice_wide_dev(device, d_db, nrec, 32, d_dbs, stream);
}

// any: the _any entry points (a multiple of 4); else the _wide rule (of 32).
static int check_rec_bytes(size_t rec_bytes, bool any = false) {
    if (any) {
        if (rec_bytes == 0 || rec_bytes % 4 != 0 || rec_bytes > DPF_PIR_MAX_REC_BYTES)
            return fail(DPF_ERR_PARAM, "dpf: rec_bytes must be a positive multiple of 4, at most DPF_PIR_MAX_REC_BYTES");
        return DPF_OK;
    }
    if (rec_bytes == 0 || rec_bytes % 32 != 0 || rec_bytes > DPF_PIR_MAX_REC_BYTES)
        return fail(DPF_ERR_PARAM, "dpf: rec_bytes must be a positive multiple of 32, at most DPF_PIR_MAX_REC_BYTES");
    return DPF_OK;
}

// The PIR answer of the four *_dev entries below: the subtree EvalFull into
// the workspace (tree launch), then the fold over the DB of rec_bytes-wide
// records -- sliced: the matrix-core fold over the bit-sliced layout, else
// the LDS fold over the row-major DB.  In front of that, 32-byte sliced
// records take both in one launch (k_pir_fused) where g_pir_kernel selects it.
static int pir_answer(bool sliced, int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                      uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_db, uint64_t nrec, size_t rec_bytes,
                      uint8_t* d_ans, void* d_work, void* stream, bool any = false) {
    if (int rc = check_rec_bytes(rec_bytes, any)) return rc;
    if (int rc = check_key(klen, logN)) return rc;
    const uint32_t stop = stop_of(logN);
    if (!dpfh::prefix_ok(prefix_bits, prefix, stop)) return fail(DPF_ERR_PARAM, "dpf: subtree prefix out of range");
    const uint64_t slice = logN - prefix_bits >= 64 ? ~0ull : (1ull << (logN - prefix_bits));
    if (nrec > slice) return fail(DPF_ERR_PARAM, "dpf: more DB records than the subtree's domain");
    if (int rc = check_pir_bufs(d_keys, nkeys, d_db, nrec, d_ans, d_work)) return rc;
    DeviceGuard g(device);
    CuScope cus(stream);
    hipStream_t st = (hipStream_t)stream;
    if (nkeys == 0) return DPF_OK;
    if (nrec == 0) {
        HIP_TRY(hipMemsetAsync(d_ans, 0, nkeys * rec_bytes, st));
        return DPF_OK;
    }
    // [tree workspace | selection bits = EvalFull bytes of the subtree | fold partials]
    uint8_t* bits = (uint8_t*)d_work + align256(tree_ws_bytes(nkeys, stop, prefix_bits, nkeys));
    const uint64_t per_key = (uint64_t)16 << (stop - prefix_bits);
    uint32_t* parts = (uint32_t*)(bits + align256(nkeys * per_key));
    const bool bs = want_bs();
    const int fz = g_pir_kernel.load(std::memory_order_relaxed);
    if (sliced && rec_bytes == 32 && !bs && fz != DPF_PIR_SPLIT &&
        dpfk::pir_fused_ok(nkeys, stop, prefix_bits, fz == DPF_PIR_FUSED_ANY)) {
        // One launch: tree + matrix-core fold (k_pir_fused) from the expanded records.
        const TreeWs w = tree_ws(d_work, nkeys, stop);
        forget_expanded(d_work);
        HIP_TRY(dpfk::launch_unpack(d_keys, klen, nkeys, stop, w.ek, st));
        note_expanded(d_work, nkeys, stop, false);
        HIP_TRY(dpfk::launch_pir_fused(w.ek, (uint32_t)nkeys, stop, prefix_bits, prefix, d_db, nrec, (uint32_t*)d_ans,
                                       parts, st));
        return DPF_OK;
    }
    HIP_TRY(tree_from_keys(d_keys, klen, nkeys, stop, prefix_bits, prefix, bits, per_key, d_work, st, bs));
    HIP_TRY((sliced ? dpfk::launch_pir_fold_sliced : dpfk::launch_pir_fold)(
        (const uint32_t*)bits, per_key / 4, d_db, nrec, rec_bytes, (uint32_t)nkeys, (uint32_t*)d_ans, parts, st));
    return DPF_OK;
}

int dpf_pir_answer_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                       uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_db, uint64_t nrec, uint8_t* d_ans,
                       void* d_work, void* stream) {
    return pir_answer(false, device, d_keys, klen, nkeys, logN, prefix_bits, prefix, d_db, nrec, 32, d_ans, d_work, stream);
}

int dpf_pir_answer_sliced_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                              uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_dbs, uint64_t nrec,
                              uint8_t* d_ans, void* d_work, void* stream) {
    return pir_answer(true, device, d_keys, klen, nkeys, logN, prefix_bits, prefix, d_dbs, nrec, 32, d_ans, d_work, stream);
}

int dpf_pir_answer_wide_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                            uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_db, uint64_t nrec, size_t rec_bytes,
                            uint8_t* d_ans, void* d_work, void* stream) {
    return pir_answer(false, device, d_keys, klen, nkeys, logN, prefix_bits, prefix, d_db, nrec, rec_bytes, d_ans, d_work,
                      stream);
}

int dpf_pir_answer_sliced_wide_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                                   uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_dbs, uint64_t nrec,
                                   size_t rec_bytes, uint8_t* d_ans, void* d_work, void* stream) {
    return pir_answer(true, device, d_keys, klen, nkeys, logN, prefix_bits, prefix, d_dbs, nrec, rec_bytes, d_ans, d_work,
                      stream);
}

int dpf_pir_answer_sliced_any_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                                  uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_dbs, uint64_t nrec,
                                  size_t rec_bytes, uint8_t* d_ans, void* d_work, void* stream) {
    return pir_answer(true, device, d_keys, klen, nkeys, logN, prefix_bits, prefix, d_dbs, nrec, rec_bytes, d_ans, d_work,
                      stream, true);
}

// The three fold entries behind their rec_bytes check: the shape and buffer
// checks in the order they report (bits_stride, nrec, alignment, null), then
// the fold on the caller's stream -- sliced: the matrix-core fold over the
// bit-sliced layout, else the LDS fold over the row-major payload.  d_work's
// alignment is checked only for the wide sliced form above 32 bytes (work16).
static int xor_fold(bool sliced, bool work16, int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys,
                    const uint8_t* d_db, uint64_t nrec, size_t rec_bytes, uint8_t* d_ans, void* d_work, void* stream) {
    if (bits_stride % 16 != 0) return fail(DPF_ERR_PARAM, "dpf: bits_stride must be a multiple of 16");
    if (nrec > (uint64_t)bits_stride * 8) return fail(DPF_ERR_PARAM, "dpf: more records than selection bits per key");
    if (((uintptr_t)d_bits | (uintptr_t)d_db) % 16 != 0 || (uintptr_t)d_ans % 4 != 0 ||
        (work16 && (uintptr_t)d_work % 16 != 0))
        return fail(DPF_ERR_PARAM, "dpf: misaligned device buffer");
    if (nkeys > 0 && (!d_ans || !d_work || (nrec > 0 && (!d_bits || !d_db))))
        return fail(DPF_ERR_PARAM, "dpf: null device buffer");
    DeviceGuard g(device);
    CuScope cus(stream);
    if (nkeys == 0) return DPF_OK;
    HIP_TRY((sliced ? dpfk::launch_pir_fold_sliced : dpfk::launch_pir_fold)(
        (const uint32_t*)d_bits, bits_stride / 4, d_db, nrec, rec_bytes, (uint32_t)nkeys, (uint32_t*)d_ans,
        (uint32_t*)d_work, (hipStream_t)stream));
    return DPF_OK;
}

int dpf_xor_fold_dev(int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys, const uint8_t* d_payload,
                     uint64_t nrec, size_t rec_bytes, uint8_t* d_ans, void* d_work, void* stream) {
    // Unlike check_rec_bytes, no DPF_PIR_MAX_REC_BYTES cap.
    if (rec_bytes == 0 || rec_bytes % 32 != 0) return fail(DPF_ERR_PARAM, "dpf: rec_bytes must be a positive multiple of 32");
    return xor_fold(false, false, device, d_bits, bits_stride, nkeys, d_payload, nrec, rec_bytes, d_ans, d_work, stream);
}

int dpf_xor_fold_sliced_dev(int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys, const uint8_t* d_dbs,
                            uint64_t nrec, uint8_t* d_ans, void* d_work, void* stream) {
    return xor_fold(true, false, device, d_bits, bits_stride, nkeys, d_dbs, nrec, 32, d_ans, d_work, stream);
}

int dpf_xor_fold_sliced_wide_dev(int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys,
                                 const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes, uint8_t* d_ans, void* d_work,
                                 void* stream) {
    if (int rc = check_rec_bytes(rec_bytes)) return rc;
    return xor_fold(true, rec_bytes > 32, device, d_bits, bits_stride, nkeys, d_dbs, nrec, rec_bytes, d_ans, d_work,
                    stream);
}

int dpf_xor_fold_sliced_any_dev(int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys,
                                const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes, uint8_t* d_ans, void* d_work,
                                void* stream) {
    if (int rc = check_rec_bytes(rec_bytes, true)) return rc;
    return xor_fold(true, rec_bytes > 32, device, d_bits, bits_stride, nkeys, d_dbs, nrec, rec_bytes, d_ans, d_work,
                    stream);
}

// ---- records of rec_bytes = 32 C bytes over the sliced layout -------------
// (and, by the _any entries, of any multiple of 4 bytes: the same launchers)
size_t dpf_pir_db_sliced_size_wide(uint64_t nrec, size_t rec_bytes) {
    if (rec_bytes == 0 || rec_bytes % 32 != 0 || rec_bytes > DPF_PIR_MAX_REC_BYTES) return 0;
    return std::max<size_t>(16, dpfk::pir_sliced_bytes(nrec, rec_bytes));
}

size_t dpf_pir_db_sliced_size_any(uint64_t nrec, size_t rec_bytes) {
    if (rec_bytes == 0 || rec_bytes % 4 != 0 || rec_bytes > DPF_PIR_MAX_REC_BYTES) return 0;
    return std::max<size_t>(16, dpfk::pir_sliced_bytes(nrec, rec_bytes));
}

static int pir_db_slice(int device, const uint8_t* d_db, uint64_t nrec, size_t rec_bytes, uint8_t* d_dbs, void* stream,
                        bool any) {
    if (int rc = check_rec_bytes(rec_bytes, any)) return rc;
    if (nrec > 0 && (!d_db || !d_dbs)) return fail(DPF_ERR_PARAM, "dpf: null device buffer");
    if (((uintptr_t)d_db | (uintptr_t)d_dbs) % 16 != 0) return fail(DPF_ERR_PARAM, "dpf: misaligned device buffer");
    DeviceGuard g(device);
    HIP_TRY(dpfk::launch_slice_db(d_db, nrec, rec_bytes, d_dbs, (hipStream_t)stream));
    return DPF_OK;
}

int dpf_pir_db_slice_wide_dev(int device, const uint8_t* d_db, uint64_t nrec, size_t rec_bytes, uint8_t* d_dbs,
                              void* stream) {
    return pir_db_slice(device, d_db, nrec, rec_bytes, d_dbs, stream, false);
}

int dpf_pir_db_slice_any_dev(int device, const uint8_t* d_db, uint64_t nrec, size_t rec_bytes, uint8_t* d_dbs,
                             void* stream) {
    return pir_db_slice(device, d_db, nrec, rec_bytes, d_dbs, stream, true);
}

// Records of the sliced DB changed / read back in place: every argument is
// checked before any device call.
static int check_update_bufs(size_t rec_bytes, const void* d_dbs, const void* d_idx, const void* d_recs,
                             bool any = false) {
    if (int rc = check_rec_bytes(rec_bytes, any)) return rc;
    if (!d_dbs || !d_idx || !d_recs) return fail(DPF_ERR_PARAM, "dpf: null device buffer");
    if (((uintptr_t)d_dbs | (uintptr_t)d_recs) % 16 != 0 || (uintptr_t)d_idx % 8 != 0)
        return fail(DPF_ERR_PARAM, "dpf: misaligned device buffer");
    return DPF_OK;
}

int dpf_pir_db_update_sliced_wide_dev(int device, uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes, const uint64_t* d_idx,
                                      const uint8_t* d_recs, size_t n, void* stream) {
    if (int rc = check_update_bufs(rec_bytes, d_dbs, d_idx, d_recs)) return rc;
    if (n == 0) return DPF_OK;
    DeviceGuard g(device);
    HIP_TRY(dpfk::launch_update_sliced(d_dbs, nrec, rec_bytes, d_idx, d_recs, n, (hipStream_t)stream));
    return DPF_OK;
}

int dpf_pir_db_gather_sliced_wide_dev(int device, const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                                      const uint64_t* d_idx, size_t n, uint8_t* d_out, void* stream) {
    if (int rc = check_update_bufs(rec_bytes, d_dbs, d_idx, d_out)) return rc;
    if (n == 0) return DPF_OK;
    DeviceGuard g(device);
    HIP_TRY(dpfk::launch_gather_sliced(d_dbs, nrec, rec_bytes, d_idx, n, d_out, (hipStream_t)stream));
    return DPF_OK;
}

int dpf_pir_db_update_sliced_any_dev(int device, uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes, const uint64_t* d_idx,
                                     const uint8_t* d_recs, size_t n, void* stream) {
    if (int rc = check_update_bufs(rec_bytes, d_dbs, d_idx, d_recs, true)) return rc;
    if (n == 0) return DPF_OK;
    DeviceGuard g(device);
    HIP_TRY(dpfk::launch_update_sliced(d_dbs, nrec, rec_bytes, d_idx, d_recs, n, (hipStream_t)stream));
    return DPF_OK;
}

int dpf_pir_db_gather_sliced_any_dev(int device, const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                                     const uint64_t* d_idx, size_t n, uint8_t* d_out, void* stream) {
    if (int rc = check_update_bufs(rec_bytes, d_dbs, d_idx, d_out, true)) return rc;
    if (n == 0) return DPF_OK;
    DeviceGuard g(device);
    HIP_TRY(dpfk::launch_gather_sliced(d_dbs, nrec, rec_bytes, d_idx, n, d_out, (hipStream_t)stream));
    return DPF_OK;
}

// Private writes (the dual of the fold): every argument is checked before
// any device call, in the order rec_bytes, bits_stride, nrec, null, alignment.
static int check_scatter_bufs(size_t rec_bytes, const void* d_bits, size_t bits_stride, uint64_t nrec,
                              const void* d_msgs, const void* d_db, bool any = false) {
    if (int rc = check_rec_bytes(rec_bytes, any)) return rc;
    if (bits_stride % 16 != 0) return fail(DPF_ERR_PARAM, "dpf: bits_stride must be a multiple of 16");
    if (nrec > (uint64_t)bits_stride * 8) return fail(DPF_ERR_PARAM, "dpf: more records than selection bits per key");
    if (!d_bits || !d_msgs || !d_db) return fail(DPF_ERR_PARAM, "dpf: null device buffer");
    if (((uintptr_t)d_bits | (uintptr_t)d_msgs | (uintptr_t)d_db) % 16 != 0)
        return fail(DPF_ERR_PARAM, "dpf: misaligned device buffer");
    return DPF_OK;
}

static int xor_scatter(bool sliced, int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys,
                       const uint8_t* d_msgs, uint8_t* d_db, uint64_t nrec, size_t rec_bytes, void* stream,
                       bool any = false) {
    if (int rc = check_scatter_bufs(rec_bytes, d_bits, bits_stride, nrec, d_msgs, d_db, any)) return rc;
    if (nkeys == 0 || nrec == 0) return DPF_OK;
    DeviceGuard g(device);
    CuScope cus(stream);
    HIP_TRY((sliced ? dpfk::launch_scatter_sliced : dpfk::launch_scatter_rows)(
        (const uint32_t*)d_bits, bits_stride / 4, d_db, nrec, rec_bytes, d_msgs, nkeys, (hipStream_t)stream));
    return DPF_OK;
}

int dpf_xor_scatter_dev(int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys, const uint8_t* d_msgs,
                        uint8_t* d_db, uint64_t nrec, size_t rec_bytes, void* stream) {
    return xor_scatter(false, device, d_bits, bits_stride, nkeys, d_msgs, d_db, nrec, rec_bytes, stream);
}

int dpf_xor_scatter_sliced_wide_dev(int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys,
                                    const uint8_t* d_msgs, uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                                    void* stream) {
    return xor_scatter(true, device, d_bits, bits_stride, nkeys, d_msgs, d_dbs, nrec, rec_bytes, stream);
}

int dpf_xor_scatter_sliced_any_dev(int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys,
                                   const uint8_t* d_msgs, uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                                   void* stream) {
    return xor_scatter(true, device, d_bits, bits_stride, nkeys, d_msgs, d_dbs, nrec, rec_bytes, stream, true);
}

// The private write of the two *_dev entries below: the subtree EvalFull into
// the workspace (pir_answer's layout, always the split path), then the
// scatter of the messages over the DB.
static int pir_write(bool sliced, int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                     uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_msgs, uint8_t* d_db, uint64_t nrec,
                     size_t rec_bytes, void* d_work, void* stream, bool any = false) {
    if (int rc = check_rec_bytes(rec_bytes, any)) return rc;
    if (int rc = check_key(klen, logN)) return rc;
    const uint32_t stop = stop_of(logN);
    if (!dpfh::prefix_ok(prefix_bits, prefix, stop)) return fail(DPF_ERR_PARAM, "dpf: subtree prefix out of range");
    const uint64_t slice = logN - prefix_bits >= 64 ? ~0ull : (1ull << (logN - prefix_bits));
    if (nrec > slice) return fail(DPF_ERR_PARAM, "dpf: more DB records than the subtree's domain");
    if (!d_keys || !d_msgs || !d_db || !d_work) return fail(DPF_ERR_PARAM, "dpf: null device buffer");
    if (((uintptr_t)d_msgs | (uintptr_t)d_db | (uintptr_t)d_work) % 16 != 0)
        return fail(DPF_ERR_PARAM, "dpf: misaligned device buffer");
    if (nkeys == 0 || nrec == 0) return DPF_OK;
    DeviceGuard g(device);
    CuScope cus(stream);
    hipStream_t st = (hipStream_t)stream;
    // [tree workspace | selection bits = EvalFull bytes of the subtree | (the fold's partials: unused)]
    uint8_t* bits = (uint8_t*)d_work + align256(tree_ws_bytes(nkeys, stop, prefix_bits, nkeys));
    const uint64_t per_key = (uint64_t)16 << (stop - prefix_bits);
    HIP_TRY(tree_from_keys(d_keys, klen, nkeys, stop, prefix_bits, prefix, bits, per_key, d_work, st, want_bs()));
    HIP_TRY((sliced ? dpfk::launch_scatter_sliced : dpfk::launch_scatter_rows)(
        (const uint32_t*)bits, per_key / 4, d_db, nrec, rec_bytes, d_msgs, nkeys, st));
    return DPF_OK;
}

int dpf_pir_write_wide_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                           uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_msgs, uint8_t* d_db, uint64_t nrec,
                           size_t rec_bytes, void* d_work, void* stream) {
    return pir_write(false, device, d_keys, klen, nkeys, logN, prefix_bits, prefix, d_msgs, d_db, nrec, rec_bytes, d_work,
                     stream);
}

int dpf_pir_write_sliced_wide_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                                  uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_msgs, uint8_t* d_dbs,
                                  uint64_t nrec, size_t rec_bytes, void* d_work, void* stream) {
    return pir_write(true, device, d_keys, klen, nkeys, logN, prefix_bits, prefix, d_msgs, d_dbs, nrec, rec_bytes, d_work,
                     stream);
}

int dpf_pir_write_sliced_any_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                                 uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_msgs, uint8_t* d_dbs,
                                 uint64_t nrec, size_t rec_bytes, void* d_work, void* stream) {
    return pir_write(true, device, d_keys, klen, nkeys, logN, prefix_bits, prefix, d_msgs, d_dbs, nrec, rec_bytes, d_work,
                     stream, true);
}

size_t dpf_xor_fold_workspace_size(void) { return dpfk::pir_fold_parts_bytes(); }

// ---- PIR over a sparse key set: record j lives at domain point d_points[j] ----
// The selection bits come from dpf_eval_bits_dev at the records' points, not
// from an EvalFull of a subtree; the fold and the scatter are the dense ones.
static size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// d_work of the two sparse composites: [Eval-bits workspace | bit rows
// [nkeys][dpf_eval_bits_stride(nrec)] | the fold's partials], each part
// rounded up to 16 bytes.
struct SparseWs {
    size_t eval_bytes, stride;
    uint8_t* bits;
    uint32_t* parts;
};
static SparseWs sparse_ws(void* d_work, size_t nkeys, uint64_t nrec, uint32_t logN) {
    SparseWs w;
    w.eval_bytes = align16(dpf_eval_bits_workspace_size(nkeys, nrec, logN));
    w.stride = dpf_eval_bits_stride(nrec);
    w.bits = (uint8_t*)d_work + w.eval_bytes;
    w.parts = (uint32_t*)(w.bits + align16(nkeys * w.stride));
    return w;
}

size_t dpf_pir_sparse_workspace_size(size_t nkeys, uint64_t nrec, uint32_t logN) {
    return align16(dpf_eval_bits_workspace_size(nkeys, nrec, logN)) + align16(nkeys * dpf_eval_bits_stride(nrec)) +
           align16(dpf_xor_fold_workspace_size());
}

int dpf_pir_answer_sparse_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                              const uint64_t* d_points, const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                              uint8_t* d_ans, void* d_work, void* stream) {
    if (int rc = check_rec_bytes(rec_bytes, true)) return rc;
    if (int rc = check_key(klen, logN, false)) return rc;
    if (int rc = check_pir_bufs(d_keys, nkeys, d_dbs, nrec, d_ans, d_work)) return rc;
    if (nkeys > 0 && nrec > 0 && !d_points) return fail(DPF_ERR_PARAM, "dpf: null device buffer");
    if ((uintptr_t)d_points % 8 != 0) return fail(DPF_ERR_PARAM, "dpf: misaligned device buffer");
    if (nkeys == 0) return DPF_OK;
    DeviceGuard g(device);
    CuScope cus(stream);
    hipStream_t st = (hipStream_t)stream;
    if (nrec == 0) {
        HIP_TRY(hipMemsetAsync(d_ans, 0, nkeys * rec_bytes, st));
        return DPF_OK;
    }
    const SparseWs w = sparse_ws(d_work, nkeys, nrec, logN);
    HIP_TRY(eval_bits_launch(d_keys, klen, nkeys, d_points, nrec, logN, w.bits, w.stride, d_work, w.eval_bytes, st));
    HIP_TRY(dpfk::launch_pir_fold_sliced((const uint32_t*)w.bits, w.stride / 4, d_dbs, nrec, rec_bytes, (uint32_t)nkeys,
                                         (uint32_t*)d_ans, w.parts, st));
    return DPF_OK;
}

int dpf_pir_write_sparse_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN,
                             const uint64_t* d_points, const uint8_t* d_msgs, uint8_t* d_dbs, uint64_t nrec,
                             size_t rec_bytes, void* d_work, void* stream) {
    if (int rc = check_rec_bytes(rec_bytes, true)) return rc;
    if (int rc = check_key(klen, logN, false)) return rc;
    if (!d_keys || !d_points || !d_msgs || !d_dbs || !d_work) return fail(DPF_ERR_PARAM, "dpf: null device buffer");
    if (((uintptr_t)d_msgs | (uintptr_t)d_dbs | (uintptr_t)d_work) % 16 != 0 || (uintptr_t)d_points % 8 != 0)
        return fail(DPF_ERR_PARAM, "dpf: misaligned device buffer");
    if (nkeys == 0 || nrec == 0) return DPF_OK;
    DeviceGuard g(device);
    CuScope cus(stream);
    hipStream_t st = (hipStream_t)stream;
    const SparseWs w = sparse_ws(d_work, nkeys, nrec, logN);
    HIP_TRY(eval_bits_launch(d_keys, klen, nkeys, d_points, nrec, logN, w.bits, w.stride, d_work, w.eval_bytes, st));
    HIP_TRY(dpfk::launch_scatter_sliced((const uint32_t*)w.bits, w.stride / 4, d_dbs, nrec, rec_bytes, d_msgs, nkeys, st));
    return DPF_OK;
}

int dpf_set_fold_limits(uint32_t max_blocks, uint32_t max_sg_per_block) {
    dpfk::set_fold_limits(max_blocks, max_sg_per_block);
    return DPF_OK;
}

// A PIR handle owns references to the devices its shards live on, so it
// stays usable (and freeable) after dpf_gpu_shutdown.
struct PirDb {
    uint32_t logN = 0, pbits = 0;
    uint64_t nrec = 0;
    size_t rec_bytes = 32;         // the caller's record width
    size_t w4 = 32;                // bytes per record on the device: rec_bytes rounded up to a multiple of 4, pad zero
    bool sliced = true;            // shards in the bit-sliced layout (the matrix-core fold)
    DevList devs;                  // per shard: its device
    std::vector<void*> shard;      // per device: its DB slice
    std::vector<uint64_t> shard_n; // records in that slice
    // The sparse kind (dpf_pir_db_create_sparse): record j lives at domain
    // point points[j]; shard g holds records [g * shard_cap, ...), a range of
    // whole super-groups and not a subtree (pbits = 0), with its slice of the
    // points beside it in HBM.
    bool sparse = false;
    uint64_t shard_cap = 0;
    std::vector<void*> shard_pts;  // per device: uint64 points of its records
    ~PirDb() {
        for (size_t i = 0; i < shard.size(); ++i) {
            DeviceGuard gd(devs[i]->id);
            (void)hipFree(shard[i]);
            if (i < shard_pts.size()) (void)hipFree(shard_pts[i]);
        }
    }
};

int dpf_pir_db_create(const uint8_t* db, uint64_t nrec, uint32_t logN, int ngpus, void** handle) {
    return dpf_pir_db_create_wide(db, nrec, 32, logN, ngpus, handle);
}

size_t dpf_pir_db_rec_bytes(void* handle) { return handle ? ((PirDb*)handle)->rec_bytes : 0; }

// Upload chunk of a sliced shard: whole super-groups, at most this many bytes.
constexpr uint64_t kPirUploadChunk = 256ull << 20;

// Rows of `w` bytes between a tight host array [n][w] and device rows of
// `pitch` >= w bytes (the handle's padded records), in either direction.
static hipError_t copy_rows_up(void* dev, size_t pitch, const uint8_t* host, size_t w, size_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (w == pitch) return hipMemcpyAsync(dev, host, n * w, hipMemcpyHostToDevice, st);
    if (hipError_t e = hipMemsetAsync(dev, 0, n * pitch, st); e != hipSuccess) return e;   // the pad bytes are zero
    return hipMemcpy2DAsync(dev, pitch, host, w, w, n, hipMemcpyHostToDevice, st);
}
static hipError_t copy_rows_down(uint8_t* host, const void* dev, size_t pitch, size_t w, size_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (w == pitch) return hipMemcpyAsync(host, dev, n * w, hipMemcpyDeviceToHost, st);
    return hipMemcpy2DAsync(host, w, dev, pitch, w, n, hipMemcpyDeviceToHost, st);
}

// any: dpf_pir_db_create_any (every width from 1 byte; shards at w4 bytes per
// record); else dpf_pir_db_create_wide's rule.  sparse: dpf_pir_db_create_sparse
// (record j at domain point points[j]; shards are record ranges of whole
// super-groups, any device count, each with its points beside it).
static int pir_db_create(const uint8_t* db, uint64_t nrec, size_t caller_bytes, uint32_t logN, int ngpus, void** handle,
                         bool any, bool sparse = false, const uint64_t* points = nullptr) {
    if (!handle) return fail(DPF_ERR_PARAM, "dpf: null handle");
    *handle = nullptr;
    if (any) {
        if (caller_bytes == 0 || caller_bytes > DPF_PIR_MAX_REC_BYTES)
            return fail(DPF_ERR_PARAM, "dpf: rec_bytes must be 1 .. DPF_PIR_MAX_REC_BYTES");
    } else if (int rc = check_rec_bytes(caller_bytes)) {
        return rc;
    }
    const size_t rec_bytes = (caller_bytes + 3) & ~(size_t)3;   // on the device
    if (logN > 63 || (!sparse && nrec > (1ull << logN))) return fail(DPF_ERR_PARAM, "dpf: DB larger than 2^logN");
    if (sparse) {
        if (nrec > 0 && (!points || !db)) return fail(DPF_ERR_PARAM, "dpf: null buffer");
        for (uint64_t j = 0; j < nrec; ++j)
            if ((points[j] >> logN) != 0) return fail(DPF_ERR_PARAM, "dpf: point outside the 2^logN domain");
    }
    int have = 0;
    const DevList devs = pick_devs(0, &have);
    if (have <= 0) return have;
    const int want = ngpus <= 0 ? have : ngpus;
    uint32_t pb = 0;
    if (sparse) {
        if (want > have) return fail(DPF_ERR_PARAM, "dpf: ngpus must be <= opened devices");
    } else if (want > have || !dpfh::gpus_to_pb(want, stop_of(logN), &pb)) {
        return fail(DPF_ERR_PARAM, "dpf: ngpus must be a power of two <= opened devices and 2^(logN-7)");
    }
    auto h = std::make_unique<PirDb>();
    h->logN = logN;
    h->pbits = pb;
    h->nrec = nrec;
    h->rec_bytes = caller_bytes;
    h->w4 = rec_bytes;
    // DPF_PIR_FOLD=lds keeps the row-major shards and the LDS fold (A/B runs).
    static const bool lds = [] {
        const char* e = getenv("DPF_PIR_FOLD");
        return e && e[0] == 'l';
    }();
    h->sliced = !lds;
    if (lds && caller_bytes % 32 != 0)
        return fail(DPF_ERR_PARAM, "dpf: row-major shards (DPF_PIR_FOLD=lds) take multiples of 32 bytes only");
    if (lds && sparse) return fail(DPF_ERR_PARAM, "dpf: sparse handles keep sliced shards only (DPF_PIR_FOLD=lds set)");
    h->sparse = sparse;
    h->shard_cap = sparse ? ((nrec + 255) / 256 + (uint64_t)want - 1) / (uint64_t)want * 256 : 0;
    const uint64_t slice = sparse ? h->shard_cap : 1ull << (logN - pb);
    for (int g = 0; g < want; ++g) {
        const uint64_t lo = std::min<uint64_t>(nrec, (uint64_t)g * slice);
        const uint64_t hi = std::min<uint64_t>(nrec, lo + slice);
        DeviceGuard gd(devs[(size_t)g]->id);
        void* p = nullptr;
        const size_t bytes = h->sliced ? dpf_pir_db_sliced_size_any(hi - lo, rec_bytes)
                                       : std::max<uint64_t>(hi - lo, 1) * rec_bytes;
        if (hipMalloc(&p, bytes) != hipSuccess) return fail(DPF_ERR_NOMEM, "dpf: DB shard allocation failed");
        h->devs.push_back(devs[(size_t)g]);     // ~PirDb frees what was allocated so far
        h->shard.push_back(p);
        h->shard_n.push_back(hi - lo);
        if (sparse) {
            void* q = nullptr;
            if (hipMalloc(&q, std::max<uint64_t>(hi - lo, 2) * 8) != hipSuccess)
                return fail(DPF_ERR_NOMEM, "dpf: DB shard allocation failed");
            h->shard_pts.push_back(q);
            if (hi > lo && hipMemcpy(q, points + lo, (hi - lo) * 8, hipMemcpyHostToDevice) != hipSuccess)
                return fail(DPF_ERR_HIP, "dpf: DB upload failed");
        }
        if (hi <= lo) continue;
        if (!h->sliced) {
            if (hipMemcpy(p, db + lo * rec_bytes, (hi - lo) * rec_bytes, hipMemcpyHostToDevice) != hipSuccess)
                return fail(DPF_ERR_HIP, "dpf: DB upload failed");
            continue;
        }
        // Row-major records up through a bounded staging buffer, in chunks of
        // whole super-groups, each sliced into its place in the shard (a
        // chunk that starts at a multiple of 256 records is a contiguous
        // sub-range of the sliced layout).
        const uint64_t chunk = std::max<uint64_t>(256, kPirUploadChunk / rec_bytes / 256 * 256);
        void* tmp = nullptr;
        if (hipMalloc(&tmp, std::min<uint64_t>(hi - lo, chunk) * rec_bytes) != hipSuccess)
            return fail(DPF_ERR_NOMEM, "dpf: DB staging allocation failed");
        bool ok = true;
        for (uint64_t r0 = lo; ok && r0 < hi; r0 += chunk) {
            const uint64_t n = std::min<uint64_t>(chunk, hi - r0);
            ok = copy_rows_up(tmp, rec_bytes, db + r0 * caller_bytes, caller_bytes, n, nullptr) == hipSuccess &&
                 dpfk::launch_slice_db((const uint8_t*)tmp, n, rec_bytes, (uint8_t*)p + (r0 - lo) * rec_bytes,
                                       nullptr) == hipSuccess &&
                 hipDeviceSynchronize() == hipSuccess;   // tmp is reused by the next chunk
        }
        (void)hipFree(tmp);
        if (!ok) return fail(DPF_ERR_HIP, "dpf: DB upload failed");
    }
    *handle = h.release();
    return DPF_OK;
}

int dpf_pir_db_create_wide(const uint8_t* db, uint64_t nrec, size_t rec_bytes, uint32_t logN, int ngpus,
                           void** handle) {
    return pir_db_create(db, nrec, rec_bytes, logN, ngpus, handle, false);
}

int dpf_pir_db_create_any(const uint8_t* db, uint64_t nrec, size_t rec_bytes, uint32_t logN, int ngpus, void** handle) {
    return pir_db_create(db, nrec, rec_bytes, logN, ngpus, handle, true);
}

int dpf_pir_db_create_sparse(const uint64_t* points, const uint8_t* db, uint64_t nrec, size_t rec_bytes, uint32_t logN,
                             int ngpus, void** handle) {
    return pir_db_create(db, nrec, rec_bytes, logN, ngpus, handle, true, true, points);
}

int dpf_pir_answer(void* handle, const uint8_t* keys, size_t klen, size_t nkeys, uint8_t* ans) {
    PirDb* h = (PirDb*)handle;
    if (!h) return fail(DPF_ERR_PARAM, "dpf: null PIR handle");
    if (int rc = check_key(klen, h->logN)) return rc;
    const int g = (int)h->shard.size();
    const size_t rb = h->rec_bytes, w4 = h->w4;
    std::vector<std::vector<uint8_t>> part((size_t)g, std::vector<uint8_t>(nkeys * rb));
    int rc = shard((size_t)g, g, [&](int dev, size_t lo, size_t hi) {
        (void)hi;
        Dev& d = *h->devs[(size_t)dev];
        std::lock_guard<std::mutex> lk(d.mu);
        DeviceGuard gd(d.id);
        HIP_TRY(d.keys.ensure(std::max<size_t>(1, nkeys * klen)));
        HIP_TRY(d.work.ensure(h->sparse ? dpf_pir_sparse_workspace_size(nkeys, h->shard_n[lo], h->logN)
                                        : dpf_pir_workspace_size(nkeys, h->logN, h->pbits)));
        HIP_TRY(d.out.ensure(std::max<size_t>(32, nkeys * w4)));
        HIP_TRY(hipMemcpyAsync(d.keys.p, keys, nkeys * klen, hipMemcpyHostToDevice, d.st));
        // (Row-major shards are multiples of 32 bytes; sliced ones any multiple of 4.)
        int r = h->sparse
                    ? dpf_pir_answer_sparse_dev(d.id, (const uint8_t*)d.keys.p, klen, nkeys, h->logN,
                                                (const uint64_t*)h->shard_pts[lo], (const uint8_t*)h->shard[lo],
                                                h->shard_n[lo], w4, (uint8_t*)d.out.p, d.work.p, d.st)
                    : (h->sliced ? dpf_pir_answer_sliced_any_dev : dpf_pir_answer_wide_dev)(
                          d.id, (const uint8_t*)d.keys.p, klen, nkeys, h->logN, h->pbits, lo,
                          (const uint8_t*)h->shard[lo], h->shard_n[lo], w4, (uint8_t*)d.out.p, d.work.p, d.st);
        if (r) return r;
        HIP_TRY(copy_rows_down(part[lo].data(), d.out.p, w4, rb, nkeys, d.st));
        HIP_TRY(hipStreamSynchronize(d.st));
        return DPF_OK;
    });
    if (rc) return rc;
    memset(ans, 0, nkeys * rb);
    for (int i = 0; i < g; ++i)
        for (size_t b = 0; b < nkeys * rb; ++b) ans[b] ^= part[(size_t)i][b];
    return DPF_OK;
}

uint64_t dpf_pir_db_nrec(void* handle) { return handle ? ((PirDb*)handle)->nrec : 0; }

// One chunk of a shard's planned entries [a, b): the local indices and (for
// an update) the records go up through the device's staging buffers, the
// device form runs on the device's stream under its mutex, and the call
// returns when the stream is idle: a concurrent dpf_pir_answer sees the shard
// before or after the chunk, never in between.
static int pir_update_chunk(PirDb* h, size_t s, const dpfh::PirUpdatePlan& plan, size_t a, size_t b,
                            const uint8_t* recs, uint8_t* out, std::vector<uint8_t>& host) {
    const size_t rb = h->rec_bytes, w4 = h->w4, m = b - a;
    Dev& d = *h->devs[s];
    uint8_t* db = (uint8_t*)h->shard[s];
    const uint64_t nrec = h->shard_n[s];
    // Entries that are consecutive in the caller's arrays (sorted input) go
    // up / come back straight from / to them; otherwise through `host`.
    bool direct = true;
    for (size_t k = 1; direct && k < m; ++k) direct = plan.src[a + k] == plan.src[a] + k;
    uint8_t* stage = nullptr;
    if (direct) {
        stage = recs ? const_cast<uint8_t*>(recs) + plan.src[a] * rb : out + plan.src[a] * rb;
    } else {
        host.resize(m * rb);
        stage = host.data();
        if (recs)
            for (size_t k = 0; k < m; ++k) memcpy(stage + k * rb, recs + plan.src[a + k] * rb, rb);
    }
    std::lock_guard<std::mutex> lk(d.mu);
    DeviceGuard gd(d.id);
    HIP_TRY(d.xs.ensure(m * 8));
    HIP_TRY(d.out.ensure(m * w4));
    const uint64_t* d_idx = (const uint64_t*)d.xs.p;
    HIP_TRY(hipMemcpyAsync(d.xs.p, plan.local.data() + a, m * 8, hipMemcpyHostToDevice, d.st));
    if (recs) {
        HIP_TRY(copy_rows_up(d.out.p, w4, stage, rb, m, d.st));
        HIP_TRY((h->sliced ? dpfk::launch_update_sliced : dpfk::launch_update_rows)(db, nrec, w4, d_idx,
                                                                                    (const uint8_t*)d.out.p, m, d.st));
    } else {
        HIP_TRY((h->sliced ? dpfk::launch_gather_sliced : dpfk::launch_gather_rows)(db, nrec, w4, d_idx, m,
                                                                                    (uint8_t*)d.out.p, d.st));
        HIP_TRY(copy_rows_down(stage, d.out.p, w4, rb, m, d.st));
    }
    HIP_TRY(hipStreamSynchronize(d.st));
    if (d.out.cap > 2 * kStageBytes) d.out.release();   // a large chunk's staging is not kept
    if (d.xs.cap > kStageBytes) d.xs.release();
    if (out && !direct)
        for (size_t k = 0; k < m; ++k) memcpy(out + plan.src[a + k] * rb, stage + k * rb, rb);
    return DPF_OK;
}

// dpf_pir_db_update (recs) and dpf_pir_db_read (out): plan on the host, then
// shard by shard in chunks of at most kPirUploadChunk bytes of records.
static int pir_update_or_read(void* handle, const uint64_t* idx, size_t n, const uint8_t* recs, uint8_t* out) {
    PirDb* h = (PirDb*)handle;
    if (!h) return fail(DPF_ERR_PARAM, "dpf: null PIR handle");
    if (n == 0) return DPF_OK;
    if (!idx || (!recs && !out)) return fail(DPF_ERR_PARAM, "dpf: null buffer");
    dpfh::PirUpdatePlan plan;
    if (!(h->sparse ? dpfh::plan_pir_update_ranges(idx, n, h->nrec, h->shard_cap, h->shard.size(), recs != nullptr, &plan)
                    : dpfh::plan_pir_update(idx, n, h->nrec, h->logN, h->pbits, recs != nullptr, &plan)))
        return fail(DPF_ERR_PARAM, "dpf: record index outside the DB");
    const size_t chunk = std::max<size_t>(1, kPirUploadChunk / h->w4);
    std::vector<uint8_t> host;
    for (size_t s = 0; s + 1 < plan.shard_off.size(); ++s)
        for (size_t a = plan.shard_off[s]; a < plan.shard_off[s + 1]; a += chunk)
            if (int rc = pir_update_chunk(h, s, plan, a, std::min(a + chunk, plan.shard_off[s + 1]), recs, out, host))
                return rc;
    return DPF_OK;
}

int dpf_pir_db_update(void* handle, const uint64_t* idx, const uint8_t* recs, size_t n) {
    return pir_update_or_read(handle, idx, n, recs, nullptr);
}

int dpf_pir_db_read(void* handle, const uint64_t* idx, size_t n, uint8_t* out) {
    return pir_update_or_read(handle, idx, n, nullptr, out);
}

// Every shard applies the batch to its slice: keys and messages up through
// the device's staging buffers, tree and scatter on the device's stream under
// its mutex, and the call returns when the stream is idle, so a concurrent
// dpf_pir_answer sees a shard before or after the whole batch.
int dpf_pir_db_write(void* handle, const uint8_t* keys, size_t klen, size_t nkeys, const uint8_t* msgs) {
    PirDb* h = (PirDb*)handle;
    if (!h) return fail(DPF_ERR_PARAM, "dpf: null PIR handle");
    if (int rc = check_key(klen, h->logN)) return rc;
    if (nkeys == 0) return DPF_OK;
    if (!keys || !msgs) return fail(DPF_ERR_PARAM, "dpf: null buffer");
    const int g = (int)h->shard.size();
    const size_t rb = h->rec_bytes, w4 = h->w4;
    return shard((size_t)g, g, [&](int dev, size_t lo, size_t hi) {
        (void)hi;
        if (h->shard_n[lo] == 0) return (int)DPF_OK;
        Dev& d = *h->devs[(size_t)dev];
        std::lock_guard<std::mutex> lk(d.mu);
        DeviceGuard gd(d.id);
        HIP_TRY(d.keys.ensure(nkeys * klen));
        HIP_TRY(d.work.ensure(h->sparse ? dpf_pir_sparse_workspace_size(nkeys, h->shard_n[lo], h->logN)
                                        : dpf_pir_workspace_size(nkeys, h->logN, h->pbits)));
        HIP_TRY(d.out.ensure(nkeys * w4));
        HIP_TRY(hipMemcpyAsync(d.keys.p, keys, nkeys * klen, hipMemcpyHostToDevice, d.st));
        HIP_TRY(copy_rows_up(d.out.p, w4, msgs, rb, nkeys, d.st));   // zero pad bytes: the DB's stay zero
        int r = h->sparse
                    ? dpf_pir_write_sparse_dev(d.id, (const uint8_t*)d.keys.p, klen, nkeys, h->logN,
                                               (const uint64_t*)h->shard_pts[lo], (const uint8_t*)d.out.p,
                                               (uint8_t*)h->shard[lo], h->shard_n[lo], w4, d.work.p, d.st)
                    : (h->sliced ? dpf_pir_write_sliced_any_dev : dpf_pir_write_wide_dev)(
                          d.id, (const uint8_t*)d.keys.p, klen, nkeys, h->logN, h->pbits, lo, (const uint8_t*)d.out.p,
                          (uint8_t*)h->shard[lo], h->shard_n[lo], w4, d.work.p, d.st);
        if (r) return r;
        HIP_TRY(hipStreamSynchronize(d.st));
        return (int)DPF_OK;
    });
}

void dpf_pir_db_free(void* handle) { delete (PirDb*)handle; }

int dpf_stream_create_cu_masked(int device, uint32_t cu_first, uint32_t cu_count, void** stream) {
    if (!stream) return fail(DPF_ERR_PARAM, "dpf: null stream out-pointer");
    *stream = nullptr;
    DeviceGuard g(device);
    int ncu = 0;
    HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device));
    if (cu_count == 0 || (uint64_t)cu_first + cu_count > (uint64_t)ncu)
        return fail(DPF_ERR_PARAM, "dpf: CU range outside the device");
    std::vector<uint32_t> mask(((size_t)ncu + 31) / 32, 0u);
    for (uint32_t b = cu_first; b < cu_first + cu_count; ++b) mask[b / 32] |= 1u << (b % 32);
    hipStream_t st = nullptr;
    HIP_TRY(hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()));
    {
        std::lock_guard<std::mutex> lk(g_cus_mu);
        g_stream_cus[st] = (int)cu_count;
    }
    *stream = st;
    return DPF_OK;
}

int dpf_stream_destroy(void* stream) {
    if (!stream) return DPF_OK;
    {
        std::lock_guard<std::mutex> lk(g_cus_mu);
        g_stream_cus.erase((hipStream_t)stream);
    }
    HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    return DPF_OK;
}

}  // extern "C"
