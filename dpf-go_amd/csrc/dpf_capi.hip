// dpf_capi.hip — the C ABI (include/dpf_hip.h) over the gfx950 kernels: the
// device registry and the knobs, the staging pipeline of the host-buffer entry
// points, and the tree, Eval and Eval-bits entries with their form queries
// (the PIR forms and the file map: capi_common.hpp).
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
// thread pool of the pinned <-> caller-buffer copies, eval_bits_plan.hpp (with
// tree_plan.hpp, by way of the launchers) the Eval into selection bits.
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>

#include <atomic>
#include <unordered_map>

#include "capi_common.hpp"
#include "copy_pool.hpp"

using namespace dpfc;
using dpfh::CopyPool;
using dpfh::full_len;
using dpfh::key_len;

thread_local std::string dpfc::t_err;

namespace {

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

// Streams created by dpf_stream_create_cu_masked and the CUs each may use.
// A _dev entry point launching on one of them sizes its grids to those CUs
// (CuScope); any other stream gets the whole device.
std::mutex g_cus_mu;
std::unordered_map<hipStream_t, int> g_stream_cus;

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

}  // namespace

CuScope::CuScope(void* stream) : prev(dpfk::cu_budget()) {
    int c = 0;
    if (stream) {
        std::lock_guard<std::mutex> lk(g_cus_mu);
        auto it = g_stream_cus.find((hipStream_t)stream);
        if (it != g_stream_cus.end()) c = it->second;
    }
    dpfk::set_cu_budget(c);
}

dpfc::Dev::~Dev() {
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

// The opened devices, opening every visible one on first use.  Returns an
// empty list (and sets the error) when none can be opened.
DevList dpfc::devices(int* rc) {
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

// The first min(ngpus, opened) devices (ngpus <= 0: all); empty + error set on failure.
DevList dpfc::pick_devs(int ngpus, int* rc) {
    DevList devs = devices(rc);
    if (*rc <= 0) return {};
    if (ngpus > 0 && (size_t)ngpus < devs.size()) devs.resize((size_t)ngpus);
    *rc = (int)devs.size();
    return devs;
}

namespace {

// ---- AES back end of the tree kernels (configs[1]: bitsliced vs T-table) --
// DPF_AES_IMPL=bitsliced|ttable sets the default; dpf_set_aes_impl switches
// at run time.  Both give bit-identical outputs.
std::atomic<int> g_aes_impl{[] {
    const char* e = getenv("DPF_AES_IMPL");
    return e && (e[0] == 'b' || e[0] == 'B') ? DPF_AES_BITSLICED : DPF_AES_TTABLE;
}()};

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

}  // namespace

bool dpfc::want_bs() { return g_aes_impl.load(std::memory_order_relaxed) == DPF_AES_BITSLICED; }

void dpfc::note_expanded(const void* d_work, size_t nkeys, uint32_t stop, bool bs) {
    std::lock_guard<std::mutex> lk(g_exp_mu);
    g_expanded[d_work] = {nkeys, stop, bs};
}
void dpfc::forget_expanded(const void* d_work) {
    std::lock_guard<std::mutex> lk(g_exp_mu);
    g_expanded.erase(d_work);
}

// One-shot tree pass from the key bytes in HBM, with a caller's d_work:
// straight from the bytes when the T-table back end runs a wave-uniform shape
// (dpfk::evalfull_raw_ok: no unpack launch, d_work untouched and its record
// dropped), else expand into d_work, run, and record what d_work now holds.
hipError_t dpfc::tree_from_keys(const uint8_t* d_keys, size_t klen, size_t nk, uint32_t stop, uint32_t prefix_bits,
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

hipError_t dpfc::window_evalfull(const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN, const WindowWs& w,
                                 uint8_t* d_rows, size_t row_stride, hipStream_t st) {
    const dpfh::WindowPlan& p = w.plan;
    const bool bs = want_bs();
    if (p.route == dpfh::kWindowSubtree)
        return tree_from_keys(d_keys, klen, nkeys, stop_of(logN), p.prefix_bits, p.first_prefix, d_rows, row_stride, w.tree, st,
                              bs);
    forget_expanded(w.sub);   // d_work itself: the sub-keys overwrite what a dense call expanded there
    hipError_t e = dpfk::launch_subkeys(d_keys, klen, nkeys, p.prefix_bits, p.first_prefix, p.npieces, w.sub, w.sub_len, st);
    if (e != hipSuccess) return e;
    const uint32_t stop = stop_of(p.s);
    if (row_stride == p.row_bytes)
        e = tree_from_keys(w.sub, w.sub_len, w.nsub, stop, 0, 0, d_rows, p.piece_bytes, w.tree, st, bs);
    else
        for (size_t k = 0; k < nkeys && e == hipSuccess; ++k)
            e = tree_from_keys(w.sub + k * p.npieces * w.sub_len, w.sub_len, p.npieces, stop, 0, 0, d_rows + k * row_stride,
                               p.piece_bytes, w.tree, st, bs);
    forget_expanded(w.tree);   // the sub-keys' records are no caller's: nothing for dpf_evalfull_expanded_dev
    return e;
}

hipError_t dpfc::eval_bits_launch(const uint8_t* d_keys, size_t klen, size_t nkeys, size_t keys_per_list,
                                  const uint64_t* d_xs, size_t npts, uint32_t logN, uint8_t* d_bits, size_t bits_stride,
                                  void* d_work, size_t work_bytes, hipStream_t st) {
    const EvalWs w = eval_ws(d_work, work_bytes, nkeys, logN);
    hipError_t e = eval_unpack(d_keys, klen, nkeys, logN, d_work, st);
    if (e != hipSuccess) return e;
    return dpfk::launch_eval_bits((const uint32_t*)d_work, stop_of(logN), logN, d_xs, nkeys, keys_per_list, npts, d_bits,
                                  bits_stride, w.frontier, w.frontier_bytes, st);
}

namespace {

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
    const size_t qcap = plan.qcap;
    // The records of every key, then the frontier of one chunk's keys.
    const size_t work = eval_ws(nullptr, 0, nk, logN).ek_bytes + dpfk::eval_frontier_bytes(plan.per, stop, ppk);
    HIP_TRY(d.keys.ensure(std::max<size_t>(1, nk * klen)));
    HIP_TRY(d.work.ensure(std::max<size_t>(16, work)));
    HIP_TRY(d.xs.ensure(2 * qcap * 8));
    if (!d.hst) {
        HIP_TRY(hipStreamCreateWithFlags(&d.hst, hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) HIP_TRY(hipEventCreateWithFlags(&d.ev_h[i], hipEventDisableTiming));
    }
    HIP_TRY(hipMemcpyAsync(d.keys.p, keys, nk * klen, hipMemcpyHostToDevice, d.st));
    HIP_TRY(dpfk::launch_unpack((const uint8_t*)d.keys.p, klen, nk, stop, (uint32_t*)d.work.p, d.st));
    const uint32_t* ek = (const uint32_t*)d.work.p;
    const EvalWs w = eval_ws(d.work.p, work, nk, logN);
    return pipeline_d2h(d, plan.nchunks, qcap, [&](size_t i, uint8_t* dout, size_t& bytes, size_t& off) {
        const int s = (int)(i & 1);
        const size_t k0 = plan.k0(i), q = plan.n(i) * ppk;
        uint64_t* dxs = (uint64_t*)d.xs.p + (size_t)s * qcap;
        CopyPool::get().memcpy_par(d.pin[s].p, xs + k0 * ppk, q * 8);
        if (i >= 2) HIP_TRY(hipStreamWaitEvent(d.hst, d.ev_k[s], 0));   // slot's previous kernel read its xs
        HIP_TRY(hipMemcpyAsync(dxs, d.pin[s].p, q * 8, hipMemcpyHostToDevice, d.hst));
        HIP_TRY(hipEventRecord(d.ev_h[s], d.hst));
        HIP_TRY(hipStreamWaitEvent(d.st, d.ev_h[s], 0));
        HIP_TRY(dpfk::launch_eval(ek + k0 * ekw, stop, logN, dxs, q, ppk, dout, w.frontier, w.frontier_bytes, d.st));
        bytes = q;
        off = k0 * ppk;
        return DPF_OK;
    }, out, nk * ppk, 0, qcap * 8);
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

static int host_rc(int rc) { return rc ? fail(rc, "dpf: invalid parameters") : DPF_OK; }

int dpf_gen_seeded(uint64_t alpha, uint32_t logN, const uint8_t s0[16], const uint8_t s1[16], uint8_t* ka,
                   uint8_t* kb) {
    return host_rc(dpfh::gen_seeded(alpha, logN, s0, s1, ka, kb));
}

int dpf_gen(uint64_t alpha, uint32_t logN, uint8_t* ka, uint8_t* kb) { return host_rc(dpfh::gen_random(alpha, logN, ka, kb)); }

int dpf_gen_batch_seeded(const uint64_t* alphas, uint32_t logN, const uint8_t* s0s, const uint8_t* s1s, size_t n,
                         uint8_t* kas, uint8_t* kbs, int nthreads) {
    return host_rc(dpfh::gen_batch_seeded(alphas, logN, s0s, s1s, n, kas, kbs, nthreads));
}

int dpf_keys_pack(const uint8_t* const* keys, const size_t* lens, size_t n, size_t key_len, uint8_t* out) {
    const int rc = dpfh::keys_pack(keys, lens, n, key_len, out);
    return rc == DPF_ERR_KEYLEN ? fail(rc, "dpf: key length differs from the batch's key_len") : host_rc(rc);
}

int dpf_keys_unpack(const uint8_t* packed, size_t key_len, size_t n, uint8_t* const* keys) {
    return host_rc(dpfh::keys_unpack(packed, key_len, n, keys));
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

// ---- windows of the domain: re-rooted sub-keys (pir_window_plan.hpp) ----
int dpf_window_form_for(uint32_t logN, uint64_t first_block, uint64_t nblocks, size_t klen, dpf_window_form* form) {
    if (form == nullptr) return fail(DPF_ERR_PARAM, "dpf: null form pointer");
    if (int rc = check_window(klen, logN, first_block, nblocks)) return rc;
    const dpfh::WindowPlan p = dpfh::window_plan(logN, first_block, nblocks);
    memset(form, 0, sizeof *form);
    form->route = p.route;
    form->prefix_bits = p.prefix_bits;
    form->first_prefix = p.first_prefix;
    form->npieces = p.npieces;
    form->piece_bytes = p.piece_bytes;
    form->row_bytes = p.row_bytes;
    form->row_offset = p.row_offset;
    form->sub_key_len = p.route == dpfh::kWindowPieces ? dpfh::window_sub_key_len(klen, p.prefix_bits) : klen;
    return DPF_OK;
}

int dpf_subkeys_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN, uint32_t prefix_bits,
                    uint64_t first_prefix, uint64_t nprefix, uint8_t* d_sub, void* stream) {
    if (int rc = check_prefix_run(klen, logN, prefix_bits, first_prefix, nprefix)) return rc;
    // A key's last 16 bytes are its final CW: they lie behind the records of the levels walked.
    if (klen < 17 + 18 * (size_t)prefix_bits + 16)
        return fail(DPF_ERR_KEYLEN, "dpf: key shorter than 33+18*prefix_bits bytes");
    if (nkeys == 0 || nprefix == 0) return DPF_OK;
    if (!present(d_keys, d_sub)) return null_buffer();
    DeviceGuard g(device);
    CuScope cus(stream);
    HIP_TRY(dpfk::launch_subkeys(d_keys, klen, nkeys, prefix_bits, first_prefix, nprefix, d_sub,
                                 dpfh::window_sub_key_len(klen, prefix_bits), (hipStream_t)stream));
    return DPF_OK;
}

size_t dpf_evalfull_window_workspace_size(size_t nkeys, uint32_t logN, uint64_t first_block, uint64_t nblocks) {
    if (!dpfh::window_ok(logN, first_block, nblocks)) return 0;
    return window_ws(nullptr, nkeys, logN, first_block, nblocks).evalfull_total;
}

int dpf_evalfull_window_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, uint32_t logN, uint64_t first_block,
                            uint64_t nblocks, uint8_t* d_rows, size_t row_stride, void* d_work, void* stream) {
    if (int rc = check_window(klen, logN, first_block, nblocks)) return rc;
    const WindowWs w = window_ws(d_work, nkeys, logN, first_block, nblocks);
    if (int rc = check_window_rows(row_stride, w.plan.row_bytes)) return rc;
    if (nkeys > 0 && !present(d_keys, d_rows, d_work)) return null_buffer();
    if (!aligned(16, d_rows, d_work)) return misaligned_buffer();
    if (nkeys == 0) return DPF_OK;
    DeviceGuard g(device);
    CuScope cus(stream);
    HIP_TRY(window_evalfull(d_keys, klen, nkeys, logN, w, d_rows, row_stride, (hipStream_t)stream));
    return DPF_OK;
}

size_t dpf_eval_workspace_size(size_t nkeys, size_t ppk, uint32_t logN) { return eval_ws_bytes(nkeys, ppk, logN); }

uint32_t dpf_eval_frontier_level(uint32_t logN, size_t pts_per_key) {
    return logN > 63 ? 0 : dpfk::eval_frontier_level(stop_of(logN), pts_per_key);   // launch_eval: no frontier above 63
}

int dpf_eval_batch_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, const uint64_t* d_xs,
                       size_t ppk, uint32_t logN, uint8_t* d_out, void* d_work, size_t work_bytes, void* stream) {
    if (int rc = check_key(klen, logN, false)) return rc;
    if (nkeys == 0 || ppk == 0) return DPF_OK;
    const EvalWs w = eval_ws(d_work, work_bytes, nkeys, logN);
    if (int rc = check_eval_ws(w)) return rc;
    if (d_xs == nullptr || d_out == nullptr || d_keys == nullptr || (reinterpret_cast<uintptr_t>(d_xs) & 7u) != 0)
        return fail(DPF_ERR_PARAM, "dpf: d_keys/d_xs/d_out must be device pointers, d_xs 8-byte aligned");
    DeviceGuard g(device);
    CuScope cus(stream);
    HIP_TRY(eval_unpack(d_keys, klen, nkeys, logN, d_work, (hipStream_t)stream));
    // The frontier (if it fits in the rest of the workspace) lets queries share the tree's top levels.
    HIP_TRY(dpfk::launch_eval((const uint32_t*)d_work, stop_of(logN), logN, d_xs, nkeys * ppk, ppk, d_out, w.frontier,
                              w.frontier_bytes, (hipStream_t)stream));
    return DPF_OK;
}

size_t dpf_eval_bits_stride(size_t npts) { return dpfh::eval_bits_stride(npts); }

size_t dpf_eval_bits_workspace_size(size_t nkeys, size_t npts, uint32_t logN) { return eval_ws_bytes(nkeys, npts, logN); }

int dpf_eval_bits_dev(int device, const uint8_t* d_keys, size_t klen, size_t nkeys, const uint64_t* d_xs, size_t npts,
                      uint32_t logN, uint8_t* d_bits, size_t bits_stride, void* d_work, size_t work_bytes,
                      void* stream) {
    if (int rc = check_key(klen, logN, false)) return rc;
    if (int rc = check_bits_rows(bits_stride, npts)) return rc;
    if (!aligned(8, d_xs) || !aligned(16, d_bits, d_work)) return misaligned_buffer();
    if (nkeys == 0 || npts == 0) return DPF_OK;
    if (!present(d_keys, d_xs, d_bits, d_work)) return null_buffer();
    if (int rc = check_eval_ws(eval_ws(d_work, work_bytes, nkeys, logN))) return rc;
    DeviceGuard g(device);
    CuScope cus(stream);
    HIP_TRY(eval_bits_launch(d_keys, klen, nkeys, nkeys, d_xs, npts, logN, d_bits, bits_stride, d_work, work_bytes,
                             (hipStream_t)stream));
    return DPF_OK;
}

// The keys of group g at group g's own list of d_xs [ngroups][npts]: the same
// kernel with a list coordinate (eval_bits_plan.hpp).  The checks come in the
// grouped entries' order (capi_pir.hip).
int dpf_eval_bits_grouped_dev(int device, const uint8_t* d_keys, size_t klen, uint64_t ngroups, uint64_t keys_per_group,
                              const uint64_t* d_xs, size_t npts, uint32_t logN, uint8_t* d_bits, size_t bits_stride,
                              void* d_work, size_t work_bytes, void* stream) {
    if (int rc = check_bits_rows(bits_stride, npts)) return rc;
    if (int rc = check_key(klen, logN)) return rc;
    if (int rc = check_group_keys(ngroups, keys_per_group)) return rc;
    if (int rc = check_group_points(ngroups, npts)) return rc;
    const size_t nkeys = ngroups * keys_per_group;
    if (nkeys > 0 && npts > 0 && !present(d_keys, d_xs, d_bits, d_work)) return null_buffer();
    if (!aligned(8, d_xs) || !aligned(16, d_bits, d_work)) return misaligned_buffer();
    if (nkeys == 0 || npts == 0) return DPF_OK;
    if (int rc = check_eval_ws(eval_ws(d_work, work_bytes, nkeys, logN))) return rc;
    DeviceGuard g(device);
    CuScope cus(stream);
    HIP_TRY(eval_bits_launch(d_keys, klen, nkeys, keys_per_group, d_xs, npts, logN, d_bits, bits_stride, d_work,
                             work_bytes, (hipStream_t)stream));
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
    const EvalWs w = eval_ws(nullptr, work_bytes, nkeys, logN);   // dpf_eval_batch_dev's own split
    if (int rc = check_eval_ws(w)) return rc;
    dpfh::EvalForm e;
    if (!dpfh::eval_form((uint64_t)nkeys * ppk, ppk, stop, logN, w.frontier_bytes,
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
