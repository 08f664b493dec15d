// capi_pir_db.hip — the resident PIR database of the C ABI (include/dpf_hip.h):
// a handle that keeps a DB sharded over the opened devices and answers,
// updates, reads, privately writes, exports, merges and clears it from host
// buffers.  Every shard runs
// the device-resident forms of capi_pir.hip on its device's stream under the
// device's mutex; pir_update_plan.hpp has the shards' record ranges and the
// planners of update / read that must agree with them.  No kernel is defined here.
#include <stdlib.h>
#include <string.h>

#include <atomic>

#include "capi_common.hpp"
#include "pir_export_plan.hpp"
#include "pir_update_plan.hpp"

using namespace dpfc;
using dpfh::kStageBytes;

namespace {

// A PIR handle owns references to the devices its shards live on, so it
// stays usable (and freeable) after dpf_gpu_shutdown.
struct PirDb {
    uint32_t logN = 0, pbits = 0;
    uint64_t nrec = 0;
    size_t rec_bytes = 32;         // the caller's record width
    size_t w4 = 32;                // bytes per record on the device: rec_bytes rounded up to a multiple of 4, pad zero
    bool sliced = true;            // shards in the bit-sliced layout (the matrix-core fold)
    // Shard g holds the records ranges.lo(g) .. ranges.hi(g) -- dense: the
    // slice of subtree (pbits, g); sparse (dpf_pir_db_create_sparse: record j
    // lives at domain point points[j]): a range of whole super-groups and not
    // a subtree (pbits = 0), with its slice of the points beside it in HBM.
    bool sparse = false;
    // Ranged (dpf_pir_db_create_ranged): dense, record j at domain point j, but
    // sharded by the sparse kind's record ranges (pbits = 0); a shard answers
    // and writes through the window forms with first_rec = ranges.lo(g).
    bool ranged = false;
    bool by_ranges() const { return sparse || ranged; }   // the range bookkeeping of update / read / export
    // Grouped (dpf_pir_db_create_grouped): ngroups
    // groups of gnrec records, nrec = ngroups * gnrec the caller's index space.
    // Shard s holds the whole groups [group_lo(s), group_hi(s)), gps of them,
    // and `ranges` is in flat positions of the grouped layout (pir_group_plan.hpp).
    // Grouped and sparse (dpf_pir_db_create_grouped_sparse): record i of group g
    // lives at points[g][i]; a shard's groups' points [groups][gnrec], tight,
    // sit beside it in HBM.
    bool grouped = false;
    uint64_t ngroups = 0, gnrec = 0, gps = 0;
    uint64_t group_lo(size_t s) const { return std::min<uint64_t>(ngroups, (uint64_t)s * gps); }
    uint64_t group_hi(size_t s) const { return std::min<uint64_t>(ngroups, group_lo(s) + gps); }
    dpfh::ShardRanges ranges;
    DevList devs;                  // per shard: its device
    std::vector<void*> shard;      // per device: its DB slice
    std::vector<uint64_t> shard_n; // records in that slice
    std::vector<void*> shard_pts;  // per device: uint64 points of its records (sparse)
    ~PirDb() {
        for (size_t i = 0; i < shard.size(); ++i) {
            DeviceGuard gd(devs[i]->id);
            (void)hipFree(shard[i]);
            if (i < shard_pts.size()) (void)hipFree(shard_pts[i]);
        }
    }
};

// Upload chunk of a sliced shard: whole super-groups, at most this many bytes.
constexpr uint64_t kPirUploadChunk = 256ull << 20;

// Rows of `w` bytes between a tight host array [n][w] and device rows of
// `pitch` >= w bytes (the handle's padded records), in either direction.
hipError_t copy_rows_up(void* dev, size_t pitch, const uint8_t* host, size_t w, size_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (w == pitch) return hipMemcpyAsync(dev, host, n * w, hipMemcpyHostToDevice, st);
    if (hipError_t e = hipMemsetAsync(dev, 0, n * pitch, st); e != hipSuccess) return e;   // the pad bytes are zero
    return hipMemcpy2DAsync(dev, pitch, host, w, w, n, hipMemcpyHostToDevice, st);
}
hipError_t copy_rows_down(uint8_t* host, const void* dev, size_t pitch, size_t w, size_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    if (w == pitch) return hipMemcpyAsync(host, dev, n * w, hipMemcpyDeviceToHost, st);
    return hipMemcpy2DAsync(host, w, dev, pitch, w, n, hipMemcpyDeviceToHost, st);
}

// DPF_PIR_FOLD=lds keeps the row-major shards and the LDS fold (A/B runs).
bool lds_shards() {
    static const bool lds = [] {
        const char* e = getenv("DPF_PIR_FOLD");
        return e && e[0] == 'l';
    }();
    return lds;
}

// Shard g of a handle under construction, on its device: the allocation(s),
// the points, and the records [lo, hi) of db.  The handle owns each buffer
// from the moment it exists, so ~PirDb frees a half-built handle.
int upload_shard(PirDb* h, const std::shared_ptr<Dev>& dev, size_t g, const uint8_t* db, const uint64_t* points) {
    const uint64_t lo = h->ranges.lo(g), hi = h->ranges.hi(g);
    const size_t rec_bytes = h->w4, caller_bytes = h->rec_bytes;
    DeviceGuard gd(dev->id);
    void* p = nullptr;
    const size_t bytes = h->sliced ? dpf_pir_db_sliced_size_any(hi - lo, rec_bytes)
                                   : std::max<uint64_t>(hi - lo, 1) * rec_bytes;
    if (hipMalloc(&p, bytes) != hipSuccess) return fail(DPF_ERR_NOMEM, "dpf: DB shard allocation failed");
    h->devs.push_back(dev);
    h->shard.push_back(p);
    h->shard_n.push_back(hi - lo);
    if (h->sparse) {
        void* q = nullptr;
        if (hipMalloc(&q, std::max<uint64_t>(hi - lo, 2) * 8) != hipSuccess)
            return fail(DPF_ERR_NOMEM, "dpf: DB shard allocation failed");
        h->shard_pts.push_back(q);
        if (hi > lo && hipMemcpy(q, points + lo, (hi - lo) * 8, hipMemcpyHostToDevice) != hipSuccess)
            return fail(DPF_ERR_HIP, "dpf: DB upload failed");
    }
    if (hi <= lo) return DPF_OK;
    if (!h->sliced) {
        if (hipMemcpy(p, db + lo * rec_bytes, (hi - lo) * rec_bytes, hipMemcpyHostToDevice) != hipSuccess)
            return fail(DPF_ERR_HIP, "dpf: DB upload failed");
        return DPF_OK;
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
             dpfk::launch_slice_db((const uint8_t*)tmp, n, rec_bytes, (uint8_t*)p + (r0 - lo) * rec_bytes, nullptr) ==
                 hipSuccess &&
             hipDeviceSynchronize() == hipSuccess;   // tmp is reused by the next chunk
    }
    (void)hipFree(tmp);
    return ok ? DPF_OK : fail(DPF_ERR_HIP, "dpf: DB upload failed");
}

// Shard s of a grouped handle under construction: its groups of db
// [ngroups][gnrec][rec_bytes] go up through a staging buffer of whole groups
// (at least one, however large) laid out as the flat DB, zero records behind
// each group's gnrec, and are sliced into their place in the shard.  points
// (the grouped keyword kind): the shard's groups' lists go up as they are.
int upload_grouped_shard(PirDb* h, const std::shared_ptr<Dev>& dev, size_t s, const uint8_t* db, const uint64_t* points) {
    const uint64_t g0 = h->group_lo(s), g1 = h->group_hi(s), n = h->gnrec, gs = dpfh::group_stride(n);
    const size_t w4 = h->w4, rb = h->rec_bytes;
    DeviceGuard gd(dev->id);
    void* p = nullptr;
    if (hipMalloc(&p, dpf_pir_db_grouped_size(g1 - g0, n, w4)) != hipSuccess)
        return fail(DPF_ERR_NOMEM, "dpf: DB shard allocation failed");
    h->devs.push_back(dev);
    h->shard.push_back(p);
    h->shard_n.push_back((g1 - g0) * gs);
    if (h->sparse) {
        void* q = nullptr;
        if (hipMalloc(&q, std::max<uint64_t>((g1 - g0) * n, 2) * 8) != hipSuccess)
            return fail(DPF_ERR_NOMEM, "dpf: DB shard allocation failed");
        h->shard_pts.push_back(q);
        if (g1 > g0 && n > 0 && hipMemcpy(q, points + g0 * n, (g1 - g0) * n * 8, hipMemcpyHostToDevice) != hipSuccess)
            return fail(DPF_ERR_HIP, "dpf: DB upload failed");
    }
    if (g1 <= g0 || n == 0) return DPF_OK;
    const uint64_t per = std::max<uint64_t>(1, kPirUploadChunk / (gs * w4));   // groups per staging chunk
    uint8_t* tmp = nullptr;
    if (hipMalloc((void**)&tmp, std::min<uint64_t>(per, g1 - g0) * gs * w4) != hipSuccess)
        return fail(DPF_ERR_NOMEM, "dpf: DB staging allocation failed");
    bool ok = true;
    for (uint64_t g = g0; ok && g < g1; g += per) {
        const uint64_t m = std::min<uint64_t>(per, g1 - g);
        if (gs == n) {
            ok = copy_rows_up(tmp, w4, db + g * n * rb, rb, m * n, nullptr) == hipSuccess;
        } else {
            ok = hipMemsetAsync(tmp, 0, m * gs * w4, nullptr) == hipSuccess;
            for (uint64_t j = 0; ok && j < m; ++j)
                ok = copy_rows_up(tmp + j * gs * w4, w4, db + (g + j) * n * rb, rb, n, nullptr) == hipSuccess;
        }
        ok = ok && dpfk::launch_slice_db(tmp, m * gs, w4, (uint8_t*)p + (g - g0) * gs * w4, nullptr) == hipSuccess &&
             hipDeviceSynchronize() == hipSuccess;   // tmp is reused by the next chunk
    }
    (void)hipFree(tmp);
    return ok ? DPF_OK : fail(DPF_ERR_HIP, "dpf: DB upload failed");
}

// dpf_pir_db_create_grouped and, with sparse (every group's records at its own
// points [ngroups][nrec]), dpf_pir_db_create_grouped_sparse: what needs no
// device, the devices, the uploads.
int pir_db_create_grouped(const uint64_t* points, bool sparse, const uint8_t* db, uint64_t ngroups, uint64_t nrec,
                          size_t caller_bytes, uint32_t logN, int ngpus, void** handle) {
    if (!handle) return fail(DPF_ERR_PARAM, "dpf: null handle");
    *handle = nullptr;
    if (int rc = check_rec_bytes(RecRule::Bytes1, caller_bytes)) return rc;
    if (logN > 63 || (!sparse && nrec > (1ull << logN))) return fail(DPF_ERR_PARAM, "dpf: group larger than 2^logN");
    const size_t w4 = (caller_bytes + 3) & ~(size_t)3;
    uint64_t bytes = 0;
    if (!dpfh::grouped_bytes(ngroups, nrec, w4, &bytes)) return fail(DPF_ERR_PARAM, "dpf: grouped DB too large");
    if (ngroups > 0 && nrec > 0 && (!db || (sparse && !points))) return fail(DPF_ERR_PARAM, "dpf: null buffer");
    if (sparse) {
        if (int rc = check_group_points(ngroups, nrec)) return rc;
        for (uint64_t j = 0; j < ngroups * nrec; ++j)
            if ((points[j] >> logN) != 0) return fail(DPF_ERR_PARAM, "dpf: point outside the 2^logN domain");
    }
    int have = 0;
    const DevList devs = pick_devs(0, &have);
    if (have <= 0) return have;
    const int want = ngpus <= 0 ? have : ngpus;
    if (want > have) return fail(DPF_ERR_PARAM, "dpf: ngpus must be <= opened devices");
    if (lds_shards()) return fail(DPF_ERR_PARAM, "dpf: grouped handles keep sliced shards only (DPF_PIR_FOLD=lds set)");
    auto h = std::make_unique<PirDb>();
    h->logN = logN;
    h->nrec = ngroups * nrec;
    h->rec_bytes = caller_bytes;
    h->w4 = w4;
    h->grouped = true;
    h->sparse = sparse;
    h->ngroups = ngroups;
    h->gnrec = nrec;
    h->gps = dpfh::groups_per_shard(ngroups, (size_t)want);
    h->ranges = dpfh::grouped_shards(ngroups, nrec, (size_t)want);
    for (int g = 0; g < want; ++g)
        if (int rc = upload_grouped_shard(h.get(), devs[(size_t)g], (size_t)g, db, points)) return rc;
    *handle = h.release();
    return DPF_OK;
}

// rule: RecRule::Mul32 (dpf_pir_db_create, _wide) or Bytes1 (_any and _sparse:
// every width from 1 byte, shards at w4 bytes per record).  points: the
// sparse kind (any device count; each shard with its points beside it).
// Ranged: the dense kind over the sparse kind's record ranges.
enum class DbKind { Dense, Sparse, Ranged };
int pir_db_create(RecRule rule, const uint64_t* points, DbKind kind, const uint8_t* db, uint64_t nrec,
                  size_t caller_bytes, uint32_t logN, int ngpus, void** handle) {
    const bool sparse = kind == DbKind::Sparse, ranged = kind == DbKind::Ranged;
    // What needs no device.
    if (!handle) return fail(DPF_ERR_PARAM, "dpf: null handle");
    *handle = nullptr;
    if (int rc = check_rec_bytes(rule, caller_bytes)) return rc;
    if (logN > 63 || (!sparse && nrec > (1ull << logN))) return fail(DPF_ERR_PARAM, "dpf: DB larger than 2^logN");
    if (sparse) {
        if (nrec > 0 && (!points || !db)) return fail(DPF_ERR_PARAM, "dpf: null buffer");
        for (uint64_t j = 0; j < nrec; ++j)
            if ((points[j] >> logN) != 0) return fail(DPF_ERR_PARAM, "dpf: point outside the 2^logN domain");
    }
    // The devices and the shards' ranges.
    int have = 0;
    const DevList devs = pick_devs(0, &have);
    if (have <= 0) return have;
    const int want = ngpus <= 0 ? have : ngpus;
    uint32_t pb = 0;
    if (sparse || ranged) {
        if (want > have) return fail(DPF_ERR_PARAM, "dpf: ngpus must be <= opened devices");
    } else if (want > have || !dpfh::gpus_to_pb(want, stop_of(logN), &pb)) {
        return fail(DPF_ERR_PARAM, "dpf: ngpus must be a power of two <= opened devices and 2^(logN-7)");
    }
    auto h = std::make_unique<PirDb>();
    h->logN = logN;
    h->pbits = pb;
    h->nrec = nrec;
    h->rec_bytes = caller_bytes;
    h->w4 = (caller_bytes + 3) & ~(size_t)3;
    h->sliced = !lds_shards();
    if (!h->sliced && !rec_bytes_ok(RecRule::Mul32Uncapped, caller_bytes))
        return fail(DPF_ERR_PARAM, "dpf: row-major shards (DPF_PIR_FOLD=lds) take multiples of 32 bytes only");
    if (!h->sliced && sparse)
        return fail(DPF_ERR_PARAM, "dpf: sparse handles keep sliced shards only (DPF_PIR_FOLD=lds set)");
    if (!h->sliced && ranged)
        return fail(DPF_ERR_PARAM, "dpf: ranged handles keep sliced shards only (DPF_PIR_FOLD=lds set)");
    h->sparse = sparse;
    h->ranged = ranged;
    h->ranges = sparse || ranged ? dpfh::sparse_shards(nrec, (size_t)want) : dpfh::dense_shards(nrec, logN, pb);
    // The uploads.
    for (int g = 0; g < want; ++g)
        if (int rc = upload_shard(h.get(), devs[(size_t)g], (size_t)g, db, points)) return rc;
    *handle = h.release();
    return DPF_OK;
}

// One shard's turn in dpf_pir_answer / dpf_pir_db_write(_grouped): under its device's
// mutex and on its device, staging of at least keys_bytes / out_bytes and the
// workspace of the shard's device form, the keys up, then body(d) and the
// stream drained, so a concurrent call sees the shard before or after.
template <class Body>
int on_shard(PirDb* h, size_t s, const uint8_t* keys, size_t klen, size_t nkeys, size_t keys_bytes, size_t out_bytes,
             Body body) {
    Dev& d = *h->devs[s];
    std::lock_guard<std::mutex> lk(d.mu);
    DeviceGuard gd(d.id);
    HIP_TRY(d.keys.ensure(keys_bytes));
    // (The grouped workspace is a function of the key rows, groups x keys per group, alone.)
    HIP_TRY(d.work.ensure(h->grouped && h->sparse ? dpf_pir_grouped_sparse_workspace_size(1, nkeys, h->gnrec, h->logN, h->w4)
                          : h->grouped            ? dpf_pir_grouped_workspace_size(1, nkeys, h->logN, h->w4)
                          : h->sparse             ? dpf_pir_sparse_workspace_size(nkeys, h->shard_n[s], h->logN)
                          : h->ranged
                              ? dpf_pir_window_workspace_size(nkeys, h->logN, h->shard_n[s] ? h->ranges.lo(s) : 0,
                                                              h->shard_n[s], h->w4)
                                                  : dpf_pir_workspace_size(nkeys, h->logN, h->pbits)));
    HIP_TRY(d.out.ensure(out_bytes));
    HIP_TRY(hipMemcpyAsync(d.keys.p, keys, nkeys * klen, hipMemcpyHostToDevice, d.st));
    if (int rc = body(d)) return rc;
    HIP_TRY(hipStreamSynchronize(d.st));
    return DPF_OK;
}

int check_grouped_nkeys(const PirDb* h, size_t nkeys) {
    if (h->ngroups == 0 ? nkeys != 0 : nkeys % h->ngroups != 0)
        return fail(DPF_ERR_PARAM, "dpf: nkeys must be a multiple of the handle's groups");
    return DPF_OK;
}

// The key rows [ngroups][kpg] split over the shards' group ranges: shard s takes
// its turn (on_shard) with the rows of its groups [g0, g0 + ng) and body(d, s,
// g0, ng, kpg); one without groups, or with skip_empty without records, does not.
template <class Body>
int on_group_shards(PirDb* h, const uint8_t* keys, size_t klen, size_t nkeys, bool skip_empty, Body body) {
    const int g = (int)h->shard.size();
    const size_t kpg = nkeys / h->ngroups;
    return shard((size_t)g, g, [&](int, size_t s, size_t) {
        const uint64_t g0 = h->group_lo(s), ng = h->group_hi(s) - g0;
        if (ng == 0 || (skip_empty && h->gnrec == 0)) return (int)DPF_OK;
        const size_t nk = ng * kpg;
        return on_shard(h, s, keys + g0 * kpg * klen, klen, nk, nk * klen, std::max<size_t>(32, nk * h->w4),
                        [&](Dev& d) { return body(d, s, g0, ng, kpg); });
    });
}

// The device form of shard s by its kind (sparse, sliced, row-major; the last
// takes multiples of 32 bytes, the others any multiple of 4): the answers
// into, or with `write` the messages from, d.out.
int shard_dev(PirDb* h, size_t s, Dev& d, size_t klen, size_t nkeys, bool write) {
    const uint8_t* k = (const uint8_t*)d.keys.p;
    uint8_t *db = (uint8_t*)h->shard[s], *io = (uint8_t*)d.out.p;
    const uint64_t n = h->shard_n[s];
    if (h->sparse) {
        const uint64_t* pts = (const uint64_t*)h->shard_pts[s];
        return write ? dpf_pir_write_sparse_dev(d.id, k, klen, nkeys, h->logN, pts, io, db, n, h->w4, d.work.p, d.st)
                     : dpf_pir_answer_sparse_dev(d.id, k, klen, nkeys, h->logN, pts, db, n, h->w4, io, d.work.p, d.st);
    }
    if (h->ranged) {
        const uint64_t first = n ? h->ranges.lo(s) : 0;   // (a shard the split left empty starts at nrec)
        return write ? dpf_pir_write_window_dev(d.id, k, klen, nkeys, h->logN, first, io, db, n, h->w4, d.work.p, d.st)
                     : dpf_pir_answer_window_dev(d.id, k, klen, nkeys, h->logN, first, db, n, h->w4, io, d.work.p, d.st);
    }
    if (write)
        return (h->sliced ? dpf_pir_write_sliced_any_dev : dpf_pir_write_wide_dev)(
            d.id, k, klen, nkeys, h->logN, h->pbits, s, io, db, n, h->w4, d.work.p, d.st);
    return (h->sliced ? dpf_pir_answer_sliced_any_dev : dpf_pir_answer_wide_dev)(
        d.id, k, klen, nkeys, h->logN, h->pbits, s, db, n, h->w4, io, d.work.p, d.st);
}

// One chunk of a shard's planned entries [a, b): the local indices and (for
// an update) the records go up through the device's staging buffers, the
// device form runs on the device's stream under its mutex, and the call
// returns when the stream is idle: a concurrent dpf_pir_answer sees the shard
// before or after the chunk, never in between.
int pir_update_chunk(PirDb* h, size_t s, const dpfh::PirUpdatePlan& plan, size_t a, size_t b, const uint8_t* recs,
                     uint8_t* out, std::vector<uint8_t>& host) {
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
int pir_update_or_read(void* handle, const uint64_t* idx, size_t n, const uint8_t* recs, uint8_t* out) {
    PirDb* h = (PirDb*)handle;
    if (!h) return fail(DPF_ERR_PARAM, "dpf: null PIR handle");
    if (n == 0) return DPF_OK;
    if (!idx || (!recs && !out)) return fail(DPF_ERR_PARAM, "dpf: null buffer");
    dpfh::PirUpdatePlan plan;
    if (!(h->grouped  ? dpfh::plan_pir_update_grouped(idx, n, h->ngroups, h->gnrec, h->shard.size(), recs != nullptr, &plan)
          : h->by_ranges()
              ? dpfh::plan_pir_update_ranges(idx, n, h->nrec, h->ranges.slice, h->shard.size(), recs != nullptr, &plan)
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

// ---- whole-DB read-out, merge and clear ---------------------------------------
// dpf_set_export_limits: bytes of a piece's staging buffer (0: kPirUploadChunk).
std::atomic<size_t> g_export_chunk{0};

// The pieces of [first, first + n) (pir_export_plan.hpp), planned before
// anything runs: a range outside the DB changes nothing.
int plan_range(PirDb* h, uint64_t first, uint64_t n, std::vector<dpfh::ExportPiece>* pieces) {
    const size_t lim = g_export_chunk.load(std::memory_order_relaxed);
    const dpfh::ExportKind kind = h->grouped  ? dpfh::ExportKind::Grouped
                                  : h->by_ranges() ? dpfh::ExportKind::Sparse
                                                   : dpfh::ExportKind::Dense;
    if (!dpfh::plan_export(kind, first, n, (lim ? lim : kPirUploadChunk) / h->w4, h->ranges, h->shard.size(), h->ngroups,
                           h->gnrec, pieces))
        return fail(DPF_ERR_PARAM, "dpf: record range outside the DB");
    return DPF_OK;
}

// One piece under its device's mutex, on its stream, drained before the next:
// a concurrent call sees the shard before or after the piece.  Export: the
// piece un-sliced into staging, its wanted rows copied down.  Merge: the
// wanted rows up into a zeroed piece (zero rows around them, zero pad bytes),
// sliced into a second staging buffer and XORed into the shard, whose padding
// therefore stays zero.  Row-major shards take plain copies and a plain XOR.
int export_piece(PirDb* h, const dpfh::ExportPiece& p, uint8_t* out, const uint8_t* recs) {
    const size_t rb = h->rec_bytes, w4 = h->w4;
    Dev& d = *h->devs[p.shard];
    uint8_t* db = (uint8_t*)h->shard[p.shard];
    std::lock_guard<std::mutex> lk(d.mu);
    DeviceGuard gd(d.id);
    if (!h->sliced) {   // (w4 == rb, a multiple of 32)
        uint8_t* rows = db + (p.local0 + p.skip) * rb;
        if (out) {
            HIP_TRY(hipMemcpyAsync(out + p.out * rb, rows, p.take * rb, hipMemcpyDeviceToHost, d.st));
        } else {
            HIP_TRY(d.out.ensure(p.take * rb));
            HIP_TRY(hipMemcpyAsync(d.out.p, recs + p.out * rb, p.take * rb, hipMemcpyHostToDevice, d.st));
            HIP_TRY(dpfk::launch_xor_words(rows, (const uint8_t*)d.out.p, p.take * rb, d.st));
        }
    } else {
        uint8_t* part = db + p.local0 * w4;
        HIP_TRY(d.out.ensure(p.nrec * w4));
        uint8_t* stage = (uint8_t*)d.out.p;
        if (out) {
            HIP_TRY(dpfk::launch_unslice_db(part, p.nrec, w4, stage, d.st));
            HIP_TRY(copy_rows_down(out + p.out * rb, stage + p.skip * w4, w4, rb, p.take, d.st));
        } else {
            const size_t sliced = dpfk::pir_sliced_bytes(p.nrec, w4);
            HIP_TRY(d.work.ensure(sliced));
            HIP_TRY(hipMemsetAsync(stage, 0, p.nrec * w4, d.st));
            HIP_TRY(copy_rows_up(stage + p.skip * w4, w4, recs + p.out * rb, rb, p.take, d.st));
            HIP_TRY(dpfk::launch_slice_db(stage, p.nrec, w4, (uint8_t*)d.work.p, d.st));
            HIP_TRY(dpfk::launch_xor_words(part, (const uint8_t*)d.work.p, sliced, d.st));
        }
    }
    HIP_TRY(hipStreamSynchronize(d.st));
    if (d.out.cap > 2 * kStageBytes) d.out.release();   // a large piece's staging is not kept
    if (!out && d.work.cap > 2 * kStageBytes) d.work.release();
    return DPF_OK;
}

int pir_export_or_xor(void* handle, uint64_t first, uint64_t n, uint8_t* out, const uint8_t* recs) {
    PirDb* h = (PirDb*)handle;
    if (!h) return fail(DPF_ERR_PARAM, "dpf: null PIR handle");
    std::vector<dpfh::ExportPiece> pieces;
    if (int rc = plan_range(h, first, n, &pieces)) return rc;
    if (n == 0) return DPF_OK;
    if (!out && !recs) return fail(DPF_ERR_PARAM, "dpf: null buffer");
    for (const dpfh::ExportPiece& p : pieces)
        if (int rc = export_piece(h, p, out, recs)) return rc;
    return DPF_OK;
}

}  // namespace

extern "C" {

int dpf_pir_db_create(const uint8_t* db, uint64_t nrec, uint32_t logN, int ngpus, void** handle) {
    return pir_db_create(RecRule::Mul32, nullptr, DbKind::Dense, db, nrec, 32, logN, ngpus, handle);
}
int dpf_pir_db_create_wide(const uint8_t* db, uint64_t nrec, size_t rec_bytes, uint32_t logN, int ngpus,
                           void** handle) {
    return pir_db_create(RecRule::Mul32, nullptr, DbKind::Dense, db, nrec, rec_bytes, logN, ngpus, handle);
}
int dpf_pir_db_create_any(const uint8_t* db, uint64_t nrec, size_t rec_bytes, uint32_t logN, int ngpus, void** handle) {
    return pir_db_create(RecRule::Bytes1, nullptr, DbKind::Dense, db, nrec, rec_bytes, logN, ngpus, handle);
}
int dpf_pir_db_create_sparse(const uint64_t* points, const uint8_t* db, uint64_t nrec, size_t rec_bytes, uint32_t logN,
                             int ngpus, void** handle) {
    return pir_db_create(RecRule::Bytes1, points, DbKind::Sparse, db, nrec, rec_bytes, logN, ngpus, handle);
}
int dpf_pir_db_create_ranged(const uint8_t* db, uint64_t nrec, size_t rec_bytes, uint32_t logN, int ngpus, void** handle) {
    return pir_db_create(RecRule::Bytes1, nullptr, DbKind::Ranged, db, nrec, rec_bytes, logN, ngpus, handle);
}
int dpf_pir_db_create_grouped(const uint8_t* db, uint64_t ngroups, uint64_t nrec, size_t rec_bytes, uint32_t logN,
                              int ngpus, void** handle) {
    return pir_db_create_grouped(nullptr, false, db, ngroups, nrec, rec_bytes, logN, ngpus, handle);
}
int dpf_pir_db_create_grouped_sparse(const uint64_t* points, const uint8_t* db, uint64_t ngroups, uint64_t nrec,
                                     size_t rec_bytes, uint32_t logN, int ngpus, void** handle) {
    return pir_db_create_grouped(points, true, db, ngroups, nrec, rec_bytes, logN, ngpus, handle);
}

size_t dpf_pir_db_rec_bytes(void* handle) { return handle ? ((PirDb*)handle)->rec_bytes : 0; }
uint64_t dpf_pir_db_nrec(void* handle) { return handle ? ((PirDb*)handle)->nrec : 0; }
uint64_t dpf_pir_db_ngroups(void* handle) {
    PirDb* h = (PirDb*)handle;
    return !h ? 0 : h->grouped ? h->ngroups : 1;
}
void dpf_pir_db_free(void* handle) { delete (PirDb*)handle; }

int dpf_pir_answer(void* handle, const uint8_t* keys, size_t klen, size_t nkeys, uint8_t* ans) {
    PirDb* h = (PirDb*)handle;
    if (!h) return fail(DPF_ERR_PARAM, "dpf: null PIR handle");
    if (int rc = check_key(klen, h->logN)) return rc;
    const int g = (int)h->shard.size();
    const size_t rb = h->rec_bytes, w4 = h->w4;
    if (h->grouped) {
        // keys [ngroups][kpg]: every shard gets its groups' key rows and
        // writes its groups' answers into their place; nothing to XOR.
        if (int rc = check_grouped_nkeys(h, nkeys)) return rc;
        if (nkeys == 0) return DPF_OK;
        if (!keys || !ans) return fail(DPF_ERR_PARAM, "dpf: null buffer");
        return on_group_shards(h, keys, klen, nkeys, false, [&](Dev& d, size_t s, uint64_t g0, uint64_t ng, size_t kpg) {
            const uint8_t *k = (const uint8_t*)d.keys.p, *db = (const uint8_t*)h->shard[s];
            if (int r = h->sparse ? dpf_pir_answer_grouped_sparse_dev(d.id, k, klen, ng, kpg, h->logN,
                                                                      (const uint64_t*)h->shard_pts[s], db, h->gnrec, w4,
                                                                      (uint8_t*)d.out.p, d.work.p, d.st)
                                  : dpf_pir_answer_grouped_dev(d.id, k, klen, ng, kpg, h->logN, db, h->gnrec, w4,
                                                               (uint8_t*)d.out.p, d.work.p, d.st))
                return r;
            HIP_TRY(copy_rows_down(ans + g0 * kpg * rb, d.out.p, w4, rb, ng * kpg, d.st));
            return (int)DPF_OK;
        });
    }
    std::vector<std::vector<uint8_t>> part((size_t)g, std::vector<uint8_t>(nkeys * rb));
    int rc = shard((size_t)g, g, [&](int, size_t s, size_t) {
        return on_shard(h, s, keys, klen, nkeys, std::max<size_t>(1, nkeys * klen), std::max<size_t>(32, nkeys * w4),
                        [&](Dev& d) {
                            if (int r = shard_dev(h, s, d, klen, nkeys, false)) return r;
                            HIP_TRY(copy_rows_down(part[s].data(), d.out.p, w4, rb, nkeys, d.st));
                            return (int)DPF_OK;
                        });
    });
    if (rc) return rc;
    memset(ans, 0, nkeys * rb);
    for (int i = 0; i < g; ++i)
        for (size_t b = 0; b < nkeys * rb; ++b) ans[b] ^= part[(size_t)i][b];
    return DPF_OK;
}

int dpf_pir_db_update(void* handle, const uint64_t* idx, const uint8_t* recs, size_t n) {
    return pir_update_or_read(handle, idx, n, recs, nullptr);
}
int dpf_pir_db_read(void* handle, const uint64_t* idx, size_t n, uint8_t* out) {
    return pir_update_or_read(handle, idx, n, nullptr, out);
}

int dpf_pir_db_export(void* handle, uint64_t first, uint64_t n, uint8_t* out) {
    return pir_export_or_xor(handle, first, n, out, nullptr);
}
int dpf_pir_db_xor_records(void* handle, uint64_t first, uint64_t n, const uint8_t* recs) {
    return pir_export_or_xor(handle, first, n, nullptr, recs);
}

// Every shard zeroed on its stream under its device's mutex; a sparse or grouped keyword handle keeps its points.
int dpf_pir_db_clear(void* handle) {
    PirDb* h = (PirDb*)handle;
    if (!h) return fail(DPF_ERR_PARAM, "dpf: null PIR handle");
    for (size_t s = 0; s < h->shard.size(); ++s) {
        Dev& d = *h->devs[s];
        std::lock_guard<std::mutex> lk(d.mu);
        DeviceGuard gd(d.id);
        const size_t bytes = h->sliced ? (size_t)dpfk::pir_sliced_bytes(h->shard_n[s], h->w4) : h->shard_n[s] * h->w4;
        if (bytes == 0) continue;
        HIP_TRY(hipMemsetAsync(h->shard[s], 0, bytes, d.st));
        HIP_TRY(hipStreamSynchronize(d.st));
    }
    return DPF_OK;
}

int dpf_set_export_limits(size_t chunk_bytes) {
    g_export_chunk.store(chunk_bytes);
    return DPF_OK;
}

// Every shard applies the batch to its slice: keys and messages up through
// the device's staging buffers, tree and scatter on the device's stream.
int dpf_pir_db_write(void* handle, const uint8_t* keys, size_t klen, size_t nkeys, const uint8_t* msgs) {
    PirDb* h = (PirDb*)handle;
    if (!h) return fail(DPF_ERR_PARAM, "dpf: null PIR handle");
    if (h->grouped)
        return fail(DPF_ERR_PARAM, "dpf: dpf_pir_db_write does not take a grouped handle (use dpf_pir_db_write_grouped)");
    if (int rc = check_key(klen, h->logN)) return rc;
    if (nkeys == 0) return DPF_OK;
    if (!keys || !msgs) return fail(DPF_ERR_PARAM, "dpf: null buffer");
    const int g = (int)h->shard.size();
    const size_t rb = h->rec_bytes, w4 = h->w4;
    return shard((size_t)g, g, [&](int, size_t s, size_t) {
        if (h->shard_n[s] == 0) return (int)DPF_OK;
        return on_shard(h, s, keys, klen, nkeys, nkeys * klen, nkeys * w4, [&](Dev& d) {
            HIP_TRY(copy_rows_up(d.out.p, w4, msgs, rb, nkeys, d.st));   // zero pad bytes: the DB's stay zero
            return shard_dev(h, s, d, klen, nkeys, true);
        });
    });
}

// The grouped private write: keys and msgs [ngroups][kpg]; shard s gets its
// groups' key and message rows and applies them to its groups.
int dpf_pir_db_write_grouped(void* handle, const uint8_t* keys, size_t klen, size_t nkeys, const uint8_t* msgs) {
    PirDb* h = (PirDb*)handle;
    if (!h) return fail(DPF_ERR_PARAM, "dpf: null PIR handle");
    if (!h->grouped) return fail(DPF_ERR_PARAM, "dpf: dpf_pir_db_write_grouped takes a grouped handle only");
    if (int rc = check_key(klen, h->logN)) return rc;
    if (int rc = check_grouped_nkeys(h, nkeys)) return rc;
    if (nkeys == 0) return DPF_OK;
    if (!keys || !msgs) return fail(DPF_ERR_PARAM, "dpf: null buffer");
    const size_t rb = h->rec_bytes, w4 = h->w4;
    return on_group_shards(h, keys, klen, nkeys, true, [&](Dev& d, size_t s, uint64_t g0, uint64_t ng, size_t kpg) {
        HIP_TRY(copy_rows_up(d.out.p, w4, msgs + g0 * kpg * rb, rb, ng * kpg, d.st));   // zero pad bytes: the DB's stay zero
        const uint8_t *k = (const uint8_t*)d.keys.p, *m = (const uint8_t*)d.out.p;
        uint8_t* db = (uint8_t*)h->shard[s];
        return h->sparse ? dpf_pir_write_grouped_sparse_dev(d.id, k, klen, ng, kpg, h->logN, (const uint64_t*)h->shard_pts[s],
                                                            m, db, h->gnrec, w4, d.work.p, d.st)
                         : dpf_pir_write_grouped_dev(d.id, k, klen, ng, kpg, h->logN, m, db, h->gnrec, w4, d.work.p, d.st);
    });
}

}  // extern "C"
