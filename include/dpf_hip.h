/*
 * dpf_hip.h — C ABI of the MI355X DPF evaluation engine (libdpf_hip.so).
 *
 * Drop-in boundary for dkales/dpf-go's evaluation path.  The reference's Go
 * API is (dpf/dpf.go):
 *     type DPFkey []byte                                  :7
 *     func Gen(alpha, logN uint64) (DPFkey, DPFkey)       :71
 *     func Eval(k DPFkey, x, logN uint64) byte            :171
 *     func EvalFull(key DPFkey, logN uint64) []byte       :243
 * A cgo file in package dpf keeps those signatures and calls the functions
 * below.  Byte layouts are the reference's, unchanged:
 *   key   = seed[16] | t[1] | stop x (sCW[16] | tLCW[1] | tRCW[1]) | finalCW[16]
 *           stop = max(logN-7, 0), length 33 + 18*stop      (dpf.go:89-167)
 *   EvalFull output = 2^(logN-3) bytes (16 if logN < 7), point x is bit
 *           (x % 8) of byte (x / 8)                          (dpf.go:248-251, dpf_test.go:52)
 *
 * Conventions: every buffer is caller-owned; calls are synchronous unless
 * the name ends in _dev; nothing is retained after return (cgo pointer
 * rules).  Return value 0 = success, negative = error (DPF_ERR_*); the Go
 * wrapper turns a nonzero code into panic(), as the reference panics.
 * All functions are thread-safe (per-device mutex + stream).
 */
#ifndef DPF_HIP_H
#define DPF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPF_OK 0
#define DPF_ERR_PARAM (-1)   /* invalid alpha/logN: where Gen panics (dpf.go:72-74) */
#define DPF_ERR_KEYLEN (-2)  /* key shorter than 17+18*stop: where Eval/EvalFull index out of range */
#define DPF_ERR_NODEV (-3)   /* no usable gfx950 device / dpf_gpu_init not possible */
#define DPF_ERR_HIP (-4)     /* HIP runtime error (message in dpf_last_error) */
#define DPF_ERR_NOMEM (-5)   /* device or host allocation failed */

/* Last error message of the calling thread ("" if none). */
const char* dpf_last_error(void);

/* ---- sizes ------------------------------------------------------------ */
/* len(DPFkey) produced by Gen for this logN (dpf.go:89-167). */
size_t dpf_key_len(uint32_t logN);
/* len(EvalFull(k, logN)) (dpf.go:248-251); 0 for logN > 63 (no such output). */
size_t dpf_evalfull_len(uint32_t logN);
/* Device scratch bytes the _dev entry points need for nkeys keys. */
size_t dpf_workspace_size(size_t nkeys, uint32_t logN);

/* ---- device management (no reference counterpart: the reference has no
 *      device; dpf.go:22-44 init() is the nearest analogue) --------------- */
/* Open ngpus devices (<= 0: every visible device).  Idempotent.  Returns the
 * number of devices opened (> 0) or a negative error.  Host-buffer entry
 * points open every visible device on first use when nothing is open. */
int dpf_gpu_init(int ngpus);
/* Open exactly the HIP ordinals ordinals[0..n) (e.g. one process per GPU:
 * its LOCAL_RANK only), so no context is created on any other device.
 * Idempotent for the same list; DPF_ERR_PARAM if other devices are open. */
int dpf_gpu_init_devices(const int* ordinals, int n);
/* Drops the library's references to the opened devices.  Calls already in
 * flight and live PIR handles keep the devices they use until they finish
 * (or are freed); later host-buffer calls re-open devices on demand. */
void dpf_gpu_shutdown(void);
int dpf_gpu_count(void);

/* ---- host-side key generation (Gen stays on the host, north star) ------ */
/* Replaces Gen (dpf.go:71-169) with the two crypto/rand seeds (:80-81)
 * passed in.  ka/kb: dpf_key_len(logN) bytes each. */
int dpf_gen_seeded(uint64_t alpha, uint32_t logN, const uint8_t s0[16], const uint8_t s1[16], uint8_t* ka,
                   uint8_t* kb);
/* Gen (dpf.go:71) itself: seeds from getrandom(2), like crypto/rand. */
int dpf_gen(uint64_t alpha, uint32_t logN, uint8_t* ka, uint8_t* kb);
/* n keys pairs at once over nthreads host threads (<= 0: all cores).
 * alphas[n], s0s/s1s [n][16], kas/kbs [n][dpf_key_len]. */
int dpf_gen_batch_seeded(const uint64_t* alphas, uint32_t logN, const uint8_t* s0s, const uint8_t* s1s, size_t n,
                         uint8_t* kas, uint8_t* kbs, int nthreads);

/* ---- key wire format ------------------------------------ */
/* A key is the reference's DPFkey bytes (type DPFkey []byte, dpf.go:7; layout
 * dpf.go:89-92,111-112,137-138,165-167), so a key made by the Go Gen is a
 * valid input here and vice versa.  A batch is [n][key_len] contiguous (what
 * dpf_gen_batch_seeded writes and every batched entry reads).
 * dpf_keys_pack gathers n keys (pointers; lens[i] must equal key_len, or
 * lens = NULL) into out[n][key_len]: DPF_ERR_KEYLEN on a length mismatch.
 * dpf_keys_unpack scatters a batch back to n key buffers of key_len bytes.
 * Host-only; large batches are copied on several threads. */
int dpf_keys_pack(const uint8_t* const* keys, const size_t* lens, size_t n, size_t key_len, uint8_t* out);
int dpf_keys_unpack(const uint8_t* packed, size_t key_len, size_t n, uint8_t* const* keys);

/* ---- evaluation, host buffers (synchronous; PCIe-inclusive) ------------ */
/* Keys: at least 17 + 18*stop bytes (the reference's own index bound,
 * dpf.go:175-176,186-188); the final CW is always k[len-16 : len]
 * (dpf.go:206,219), longer keys are accepted.  Shorter: DPF_ERR_KEYLEN. */
/* Eval (dpf.go:171-211): *out_bit = 0/1.  Like the reference, Eval accepts
 * any logN (Gen never makes a key above 63): path bits above bit 63 of x read
 * as 0 (Go's `uint64(1) << s` is 0 for s >= 64, dpf.go:194), so such a key
 * takes the left child on its top logN-64 levels.  The EvalFull entry points
 * return DPF_ERR_PARAM for logN > 63, where the reference panics allocating
 * its 2^(logN-3)-byte output (dpf.go:251). */
int dpf_eval(const uint8_t* key, size_t key_len, uint64_t x, uint32_t logN, uint8_t* out_bit);
/* Host output buffers are written by parallel copies from pinned staging;
 * with DPF_PREFAULT_OUTPUT=1 in the environment, buffers >= 64 MiB also get
 * a MADV_HUGEPAGE hint and are pre-touched (zeroed) while the GPU works.
 * Off by default: it changes the caller's memory policy. */
/* EvalFull (dpf.go:243-262): out = dpf_evalfull_len(logN) bytes. */
int dpf_evalfull(const uint8_t* key, size_t key_len, uint32_t logN, uint8_t* out);
/* nkeys x EvalFull; keys packed [nkeys][key_len], out [nkeys][evalfull_len].
 * Keys are sharded over ngpus devices (<= 0: all opened devices). */
int dpf_evalfull_batch(const uint8_t* keys, size_t key_len, size_t nkeys, uint32_t logN, uint8_t* out, int ngpus);
/* nkeys x pts_per_key Eval; xs [nkeys][pts_per_key], out one 0/1 byte per
 * query in the same order. */
int dpf_eval_batch(const uint8_t* keys, size_t key_len, size_t nkeys, const uint64_t* xs, size_t pts_per_key,
                   uint32_t logN, uint8_t* out, int ngpus);
/* One EvalFull split by top-level subtree over ngpus devices (ngpus must be
 * a power of two <= 2^stop); out = dpf_evalfull_len(logN) bytes. */
int dpf_evalfull_split(const uint8_t* key, size_t key_len, uint32_t logN, uint8_t* out, int ngpus);

/* ---- evaluation, device-resident buffers (asynchronous on `stream`) ----
 * Pointers are device pointers on `device`; `work` holds
 * dpf_workspace_size(nkeys, logN) bytes; stream is a hipStream_t (NULL =
 * the default stream).  Nothing is synchronised.  After one eager call of
 * the same shape, a _dev call may be recorded in a stream capture and
 * replayed over new buffer contents (tests/test_gpu_stream_capture.py). */
int dpf_evalfull_batch_dev(int device, const uint8_t* d_keys, size_t key_len, size_t nkeys, uint32_t logN,
                           uint8_t* d_out, void* d_work, void* stream);
/* The subtree at depth prefix_bits, index prefix of every key: 2^(logN-3-
 * prefix_bits) bytes per key at d_out + k*that (logN-7 >= prefix_bits).
 * dpf_workspace_size counts scratch for the whole tree and outgrows any
 * device at deep logN; a subtree call (this one, dpf_expand_keys_dev and
 * dpf_evalfull_expanded_dev) uses at most dpf_pir_workspace_size(nkeys,
 * logN, prefix_bits) bytes of d_work. */
int dpf_evalfull_subtree_dev(int device, const uint8_t* d_keys, size_t key_len, size_t nkeys, uint32_t logN,
                             uint32_t prefix_bits, uint64_t prefix, uint8_t* d_out, void* d_work, void* stream);
/* Batched Eval on HBM buffers.  d_work holds work_bytes; with
 * dpf_eval_workspace_size(nkeys, pts_per_key, logN) bytes the queries of a
 * key share its top tree levels (a frontier of 2^L nodes per key computed
 * once); with only dpf_workspace_size(nkeys, logN) bytes each query walks
 * from the root.  Results are identical either way.  d_xs must be 8-byte
 * aligned (DPF_ERR_PARAM otherwise); a 16-byte-aligned d_xs lets the
 * persistent kernel stage query pairs by LDS-DMA, an 8-byte-aligned one
 * (e.g. a tensor slice xs[1:]) runs the per-pair kernel, same results. */
size_t dpf_eval_workspace_size(size_t nkeys, size_t pts_per_key, uint32_t logN);
/* Depth L of that shared frontier (0: none).  Work with the frontier:
 * 2^(L+1)-2 AES per key for the frontier nodes, then logN-7-L+1 per query
 * (against the reference's 2*(logN-7)+1, dpf.go:183-209). */
uint32_t dpf_eval_frontier_level(uint32_t logN, size_t pts_per_key);
int dpf_eval_batch_dev(int device, const uint8_t* d_keys, size_t key_len, size_t nkeys, const uint64_t* d_xs,
                       size_t pts_per_key, uint32_t logN, uint8_t* d_out, void* d_work, size_t work_bytes,
                       void* stream);
/* Eval of every key at ONE list of points, the answers as packed selection
 * bits: d_xs [npts] is shared by all nkeys keys (unsorted, repeated and
 * bit-63 points are fine; no per-key copy is made), and bit j%8 of byte j/8 of
 * row k of d_bits [nkeys][bits_stride] is Eval(key_k, d_xs[j], logN): the bit
 * dpf_eval_batch_dev returns for (key_k, d_xs[j]), for every logN it accepts,
 * in EvalFull's bit order.  The kernel writes the first
 * dpf_eval_bits_stride(npts) = 16*ceil(npts/128) bytes of every row, with
 * zeros at bit positions >= npts of that span, and touches no byte of a row
 * past it.  So the rows are valid d_bits input, with nrec = npts, of
 * dpf_xor_fold_dev, dpf_xor_fold_sliced_any_dev, dpf_xor_scatter_dev and
 * dpf_xor_scatter_sliced_any_dev: PIR over records that sit at arbitrary
 * points of a large domain (keyword PIR) instead of a dense prefix of a
 * subtree.  A wave evaluates 128 consecutive points of one key and turns its
 * answers into the row's 16 bytes by wave ballots: 1/8 byte of output per
 * query, no byte-per-query intermediate, no atomics.
 * dpf_eval_bits_workspace_size is dpf_eval_workspace_size(nkeys, npts, logN):
 * the expanded keys and the frontier, nothing that grows as nkeys*npts.  With
 * that many work_bytes the points share each key's top tree levels; with no
 * more than the expanded keys (dpf_eval_workspace_size(nkeys, 1, logN)) every
 * walk starts at the root, as for dpf_eval_batch_dev; the bits are identical.
 * DPF_ERR_KEYLEN for a short key; DPF_ERR_PARAM, each checked before any
 * device call, when bits_stride is not a multiple of 16 or is below
 * dpf_eval_bits_stride(npts), d_xs is not 8-byte aligned, d_bits or d_work is
 * not 16-byte aligned, a pointer is null while nkeys and npts are nonzero, or
 * work_bytes does not hold the expanded keys (nkeys * (logN-7+2) * 32 bytes;
 * dpf_workspace_size(nkeys, logN) always does, but outgrows any device at
 * deep logN).  nkeys == 0 or npts == 0 returns DPF_OK without a launch.
 * Asynchronous on `stream`. */
size_t dpf_eval_bits_stride(size_t npts);
size_t dpf_eval_bits_workspace_size(size_t nkeys, size_t npts, uint32_t logN);
int dpf_eval_bits_dev(int device, const uint8_t* d_keys, size_t key_len, size_t nkeys, const uint64_t* d_xs,
                      size_t npts, uint32_t logN, uint8_t* d_bits, size_t bits_stride, void* d_work, size_t work_bytes,
                      void* stream);
/* The same launch with a point list per group: d_keys is
 * [ngroups * keys_per_group][key_len] in group order, d_xs is [ngroups][npts]
 * uint64, tightly packed, and the keys of group g are evaluated at group g's
 * own npts points: bit j of row g * keys_per_group + k of d_bits
 * [ngroups * keys_per_group][bits_stride] is Eval(that key, d_xs[g][j], logN).
 * The row contract is dpf_eval_bits_dev's: the first
 * dpf_eval_bits_stride(npts) bytes of every row are written, bits at positions
 * >= npts are zero, nothing past that span is touched; so the rows are valid
 * d_bits input of dpf_xor_fold_grouped_dev and dpf_xor_scatter_grouped_dev
 * with nrec = npts.  One kernel serves both entries (dpf_eval_bits_dev is the
 * case of one list for all keys); a lane of a list's last, partial unit reads
 * that list's last point and never the next list's.  The workspace is
 * dpf_eval_bits_workspace_size(ngroups * keys_per_group, npts, logN), and with
 * no more than the expanded keys every walk starts at the root; the bits are
 * identical.  Checked before any device call, in the grouped entries' order:
 * bits_stride (DPF_ERR_PARAM); logN > 63 (DPF_ERR_PARAM); the key length
 * (DPF_ERR_KEYLEN); ngroups * keys_per_group not fitting 32 bits, or
 * ngroups * npts * 8 bytes of points not fitting 64 (DPF_ERR_PARAM); a null
 * buffer while there is work; a misaligned buffer (d_xs 8-byte, d_bits and
 * d_work 16-byte); then ngroups, keys_per_group or npts == 0 returns DPF_OK
 * without a launch, and a work_bytes that does not hold the expanded keys is
 * DPF_ERR_PARAM.  Asynchronous on `stream`, capturable. */
int dpf_eval_bits_grouped_dev(int device, const uint8_t* d_keys, size_t key_len, uint64_t ngroups,
                              uint64_t keys_per_group, const uint64_t* d_xs, size_t npts, uint32_t logN,
                              uint8_t* d_bits, size_t bits_stride, void* d_work, size_t work_bytes, void* stream);

/* ---- Introspection: which form of a kernel a call runs -------------------
 * The tree kernel is one source but many kernels at run time; these say which
 * one a call takes, from the same plan (csrc/tree_plan.hpp) the launchers
 * follow, under the process's environment switches.  They change no state and
 * need no open device when cus > 0 (cus <= 0: the current device's CU count,
 * or the calling thread's CU-masked stream budget).  The fields describe the
 * current kernels for tests and tools; they are not a stable contract and may
 * change with any release. */
#define DPF_WALK_NONE 0 /* every thread walks from the root */
#define DPF_WALK_LANE 1 /* shared walk, one lane per path (128-thread workgroups) */
#define DPF_WALK_QUAD 2 /* shared walk, a quad of lanes per path (>= 256 threads) */
typedef struct dpf_tree_form {
    uint32_t d;         /* per-thread subtree depth */
    uint32_t block;     /* workgroup size = 2^w */
    uint32_t w;
    uint32_t ltop;      /* levels walked per thread */
    uint32_t units_log; /* threads per key = 2^units_log */
    uint32_t walk;      /* DPF_WALK_* */
    uint32_t l1;        /* level the shared walk ends at (0 without one) */
    uint8_t uniform, nodes, raw, cw_lds, feedback, prio_small;
    uint8_t pad_[2];
    uint64_t nunits;    /* threads with work */
    uint64_t grid;      /* workgroups */
    uint64_t sub_base;  /* first subtree of a key, for prefix 0 */
} dpf_tree_form;
/* The leaf launch of dpf_evalfull_subtree_dev(nkeys, logN, prefix_bits) under
 * the T-table back end (node_level == 0; `raw` says whether it reads the key
 * bytes or needs expanded records), or the node pass down to level
 * node_level below the root (prefix_bits <= node_level <= logN - 7) that the
 * batched Eval frontier (prefix_bits = 0, node_level = L) and the byte-sliced
 * back end run.  DPF_ERR_PARAM for a shape out of range or a grid the
 * launcher would refuse. */
int dpf_tree_form_for(size_t nkeys, uint32_t logN, uint32_t prefix_bits, uint32_t node_level, int cus,
                      dpf_tree_form* form);
#define DPF_EVAL_PERSIST 0      /* k_eval_persist: one 1024-thread workgroup per CU strides over the pairs */
#define DPF_EVAL_PAIR_UNIFORM 1 /* k_eval2<true>: one pair per thread, a wave's queries share a key */
#define DPF_EVAL_PAIR 2         /* k_eval2<false>: one pair per thread, per-lane keys */
#define DPF_EVAL_TRIE_KERNEL 3  /* k_eval_trie (the experimental library, dpf_set_eval_kernel) */
typedef struct dpf_eval_form {
    uint32_t level;     /* frontier level L (0: root walks) */
    uint32_t kernel;    /* DPF_EVAL_* above */
    uint32_t block;
    uint8_t cw_staged;  /* DPF_EVAL_PERSIST: a pair's key records sit in LDS slots */
    uint8_t ragged;     /* the last workgroup (or stride) has threads without a pair */
    uint8_t pad_[2];
    uint64_t grid;
    dpf_tree_form nodes; /* the frontier pass, when level > 0 */
} dpf_eval_form;
/* What dpf_eval_batch_dev runs for nkeys x pts_per_key queries with a
 * workspace of work_bytes and a d_xs that is (or is not) 16-byte aligned. */
int dpf_eval_form_for(size_t nkeys, size_t pts_per_key, uint32_t logN, size_t work_bytes, int xs_aligned16, int cus,
                      dpf_eval_form* form);

/* ---- CU-partitioned streams (no reference counterpart: engine plumbing) -
 * A stream whose kernels may run only on CUs [cu_first, cu_first+cu_count)
 * of `device` (hipExtStreamCreateWithCUMask).  Bit i of the mask is spread
 * across the XCDs (consecutive bits land on different XCDs), so any
 * contiguous range is balanced over the chip.  The _dev entry points size
 * their grids to the stream's CUs.  Two such streams over disjoint ranges let
 * an LDS-bound kernel (the tree) and an HBM-bound one (the PIR fold) run side
 * by side without sharing a CU.  Destroy with dpf_stream_destroy. */
int dpf_stream_create_cu_masked(int device, uint32_t cu_first, uint32_t cu_count, void** stream);
int dpf_stream_destroy(void* stream);

/* ---- AES back end of the tree kernels (BASELINE configs[1]) ------------
 * DPF_AES_TTABLE: T-tables staged in LDS (aes_ttable.hpp).
 * DPF_AES_BITSLICED: table-free byte-sliced AES, 8 blocks per lane in VALU
 * registers (aes_bytesliced.hpp); used for EvalFull subtrees of >= 2^7 leaf
 * blocks per key, the T-table elsewhere.  Outputs are bit-identical.
 * Process-wide; the default comes from env DPF_AES_IMPL=ttable|bitsliced. */
#define DPF_AES_TTABLE 0
#define DPF_AES_BITSLICED 1
int dpf_set_aes_impl(int impl);   /* returns the previous back end */
int dpf_get_aes_impl(void);
/* ---- batched Eval kernel (dpf_eval_batch*, BASELINE configs[2]) ---------
 * DPF_EVAL_WALK (default): the level-L frontier, then one walk per query.
 * DPF_EVAL_TRIE: the same frontier, then only the visited nodes of each
 * key's query trie below it (5,307 instead of 6,142 AES per
 * key at configs[2]), where logN <= 20 and pts_per_key <= 1024; the walk
 * kernel elsewhere.  Outputs are bit-identical.  The trie kernel was
 * measured slower and is built only in the experimental library (make
 * -C dpf-go_amd experimental); the product library returns DPF_ERR_PARAM
 * for DPF_EVAL_TRIE.  Process-wide; env DPF_EVAL_TRIE=1 sets the initial
 * value (experimental build). */
#define DPF_EVAL_WALK 0
#define DPF_EVAL_TRIE 1
int dpf_set_eval_kernel(int kernel);   /* returns the previous kernel */
int dpf_get_eval_kernel(void);
/* ---- small-call path of the single-key API ---------------
 * dpf_eval and dpf_evalfull are the reference's latency-bound single calls
 * (dpf.go:171, :243).  DPF_SMALL_AUTO (default) evaluates them on the host's
 * AES units (host_eval.cpp: AES-NI/VAES, bit-exact with the kernels) when
 * that beats a GPU round trip: every dpf_eval, and dpf_evalfull up to
 * logN = dpf_small_call_max_logN(), which depends on the host (21 with
 * VAES, 20 with AES-NI only); DPF_SMALL_GPU always uses the GPU,
 * DPF_SMALL_HOST the host whenever it has AES-NI, except dpf_evalfull above
 * logN = 28 (outputs of 32 MiB and more), which stays on the GPU.  Either
 * way a gfx950
 * device must be open (DPF_ERR_NODEV otherwise): this is a latency path,
 * not a fallback.  The batched and _dev entry points always run on the GPU.
 * Process-wide; default from env DPF_SMALL_CALLS=auto|gpu|host. */
#define DPF_SMALL_AUTO 0
#define DPF_SMALL_GPU 1
#define DPF_SMALL_HOST 2
int dpf_set_small_call_path(int mode);   /* returns the previous mode */
int dpf_get_small_call_path(void);
uint32_t dpf_small_call_max_logN(void);
/* aes128MMO (aes_amd64.s:51-82) of nblocks (multiple of 8) 16-byte blocks,
 * iterated `reps` times (out = MMO^reps(in)), under the fixed left (right=0)
 * or right key (dpf.go:23-24): the AES blocks/s microbenchmark + self-test. */
int dpf_aes_mmo_dev(int device, int impl, int right, const uint8_t* d_in, uint8_t* d_out, size_t nblocks,
                    uint32_t reps, void* stream);

/* Two-phase form of the above: expand keys once into d_work (the aligned
 * per-level records the kernels read), then evaluate any number of
 * subtrees of all nkeys keys from the expanded form.  Lets a caller time the
 * tree kernel alone and reuse expanded keys across calls.  The layout
 * depends on (nkeys, logN): dpf_evalfull_expanded_dev must pass the nkeys
 * and logN that dpf_expand_keys_dev used for this d_work, else
 * DPF_ERR_PARAM.  d_work is also the byte-sliced back end's frontier
 * scratch, so evaluations from one d_work must not overlap in time (use
 * one d_work per stream). */
int dpf_expand_keys_dev(int device, const uint8_t* d_keys, size_t key_len, size_t nkeys, uint32_t logN, void* d_work,
                        void* stream);
int dpf_evalfull_expanded_dev(int device, void* d_work, size_t nkeys, uint32_t logN, uint32_t prefix_bits,
                              uint64_t prefix, uint8_t* d_out, void* stream);
/* The library remembers, per d_work address, what dpf_expand_keys_dev (and
 * the other _dev entry points that expand into a caller's workspace) left
 * there.  Call this before freeing a workspace: a new buffer later allocated
 * at the same address would otherwise pass dpf_evalfull_expanded_dev's
 * shape check with stale records.  Always returns 0. */
int dpf_forget_workspace(const void* d_work);

/* ---- 2-server PIR over a DPF (BASELINE configs[4]; no reference
 *      counterpart: a consumer of EvalFull, SURVEY 8a last row) -----------
 * Server answer for key k: XOR of the 32-byte records DB[i] with
 * bit i of EvalFull(key_k, logN) set.  The DB holds nrec <= 2^logN records
 * of 32 bytes; the two servers' answers XOR to DB[alpha]. */

/* Device form on one GPU: DB slice = records of subtree (prefix_bits,
 * prefix), i.e. global records [prefix*2^(logN-prefix_bits), ...), d_db
 * holding nrec <= 2^(logN-prefix_bits) of them.  d_ans = nkeys*32 bytes
 * (overwritten); d_work = dpf_pir_workspace_size(nkeys, logN, prefix_bits). */
size_t dpf_pir_workspace_size(size_t nkeys, uint32_t logN, uint32_t prefix_bits);
int dpf_pir_answer_dev(int device, const uint8_t* d_keys, size_t key_len, size_t nkeys, uint32_t logN,
                       uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_db, uint64_t nrec, uint8_t* d_ans,
                       void* d_work, void* stream);

/* Streaming consumer of EvalFull output, the PIR fold
 * generalised to any payload: for each key k,
 *   ans[k] = XOR over i < nrec with bit i of bits[k] set of payload[i]
 * (bit i = bit i%8 of byte i/8, EvalFull's layout, dpf.go:251-261), computed
 * where the EvalFull output already lives, so it never leaves HBM.
 * d_bits [nkeys][bits_stride] (e.g. dpf_evalfull_batch_dev's output;
 * bits_stride a multiple of 16, nrec <= 8*bits_stride), d_payload
 * [nrec][rec_bytes] (rec_bytes a positive multiple of 32), d_ans
 * [nkeys][rec_bytes] (overwritten), d_work dpf_xor_fold_workspace_size()
 * bytes; 16-byte-aligned device pointers.  Asynchronous on `stream`. */
size_t dpf_xor_fold_workspace_size(void);
int dpf_xor_fold_dev(int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys, const uint8_t* d_payload,
                     uint64_t nrec, size_t rec_bytes, uint8_t* d_ans, void* d_work, void* stream);

/* The fold on the matrix cores (v_mfma_scale_f32_32x32x64_f8f6f4, FP4 {0,1}
 * operands, exact counts whose parity is the answer bit) reads the DB in a
 * bit-sliced layout that a PIR server builds once when it loads the DB:
 * dbs[S][n][g] (u32) for super-group S of 256 records, bit position n < 256
 * and record group g < 8, bit j = bit n of record 256*S + 32*g + j (records
 * past nrec read as 0).  dpf_pir_db_slice_dev writes it from the row-major
 * DB (nrec x 32 B) into dpf_pir_db_sliced_size(nrec) bytes.  The _sliced
 * entry points take that layout and give the same answers as their row-major
 * forms (same workspace sizes); 32-byte records (wider ones: the _wide
 * entry points below).  dpf_pir_answer_sliced_dev can be recorded in a stream
 * capture only under DPF_PIR_SPLIT, the default: where dpf_set_pir_kernel
 * (below) selected the fused kernel, its launcher synchronises first. */
size_t dpf_pir_db_sliced_size(uint64_t nrec);
int dpf_pir_db_slice_dev(int device, const uint8_t* d_db, uint64_t nrec, uint8_t* d_dbs, void* stream);
int dpf_pir_answer_sliced_dev(int device, const uint8_t* d_keys, size_t key_len, size_t nkeys, uint32_t logN,
                              uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_dbs, uint64_t nrec,
                              uint8_t* d_ans, void* d_work, void* stream);
int dpf_xor_fold_sliced_dev(int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys, const uint8_t* d_dbs,
                            uint64_t nrec, uint8_t* d_ans, void* d_work, void* stream);
/* Records wider than 32 bytes on the matrix cores.  rec_bytes = 32*C, a
 * positive multiple of 32 up to DPF_PIR_MAX_REC_BYTES (else DPF_ERR_PARAM;
 * the size function returns 0).  The wide sliced layout is ABI:
 *   dbs[S][c][n][g] (u32): super-group S of 256 records, column c < C, bit
 *   position n < 256, record group g < 8; bit j of the word = bit n of bytes
 *   [32c, 32c+32) of record 256*S + 32*g + j, bit n of a column being bit n%8
 *   of its byte n/8.  Records past nrec read as 0.
 * It takes ceil(nrec/256) * 256 * rec_bytes bytes (minimum 16), and for C = 1
 * it is the 32-byte layout above, byte for byte.  Super-groups follow one
 * another, so a shard or an upload chunk that starts at a multiple of 256
 * records is a contiguous sub-range: slicing records [256*S0, ...) into
 * d_dbs + S0*256*rec_bytes writes the bytes that slicing the whole DB writes
 * there (how a DB larger than a staging buffer is loaded).
 * The _wide entry points keep the contracts, workspace sizes and answers of
 * their 32-byte forms with d_ans = [nkeys][rec_bytes] (overwritten), and at
 * rec_bytes == 32 they are those forms.  dpf_xor_fold_sliced_wide_dev is
 * dpf_xor_fold_dev over the sliced DB; dpf_pir_answer_sliced_wide_dev is the
 * tree pass of dpf_pir_answer_sliced_dev followed by the wide fold (always
 * the split path); dpf_pir_answer_wide_dev is dpf_pir_answer_dev for a
 * row-major DB of rec_bytes-byte records (the LDS fold of dpf_xor_fold_dev).
 * The fold gives a workgroup up to 4 columns of its super-groups, so the
 * selection bits it reads per DB byte fall from 1/4 towards 1/16.  Over
 * 512 MiB of 64-byte to 1-KiB records the sliced form measured faster than
 * the row-major one (dpf_xor_fold_dev, dpf_pir_answer_wide_dev) at every
 * batch size tried, 1 to 256 keys (no crossover
 * found), so the handle below keeps its shards sliced. */
#define DPF_PIR_MAX_REC_BYTES 32768
size_t dpf_pir_db_sliced_size_wide(uint64_t nrec, size_t rec_bytes);
int dpf_pir_db_slice_wide_dev(int device, const uint8_t* d_db, uint64_t nrec, size_t rec_bytes, uint8_t* d_dbs,
                              void* stream);
int dpf_xor_fold_sliced_wide_dev(int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys,
                                 const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes, uint8_t* d_ans, void* d_work,
                                 void* stream);
int dpf_pir_answer_sliced_wide_dev(int device, const uint8_t* d_keys, size_t key_len, size_t nkeys, uint32_t logN,
                                   uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_dbs, uint64_t nrec,
                                   size_t rec_bytes, uint8_t* d_ans, void* d_work, void* stream);
int dpf_pir_answer_wide_dev(int device, const uint8_t* d_keys, size_t key_len, size_t nkeys, uint32_t logN,
                            uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_db, uint64_t nrec, size_t rec_bytes,
                            uint8_t* d_ans, void* d_work, void* stream);
/* Records of a sliced DB changed and read back in place, without re-slicing
 * it.  Both are asynchronous on `stream`, need no workspace and synchronise
 * nothing; rec_bytes as above (32 is the C = 1 case of the same kernels);
 * d_dbs, d_recs and d_out 16-byte and d_idx 8-byte aligned, none of them
 * null (else DPF_ERR_PARAM, checked before any device call); n == 0 returns
 * DPF_OK without a launch.
 * dpf_pir_db_update_sliced_wide_dev sets record d_idx[i] of d_dbs to
 * d_recs[i * rec_bytes ..) for every i < n.  d_idx must be non-decreasing; of
 * equal indices the last one wins; entries with d_idx[i] >= nrec are skipped
 * (so the padding of the last super-group stays zero: "records past nrec
 * read as 0").  Afterwards d_dbs holds, byte for byte, what
 * dpf_pir_db_slice_wide_dev writes from the modified row-major DB.  With
 * indices that are not sorted the content of the touched super-groups is
 * unspecified, but no access leaves the buffers.  One workgroup rewrites
 * each touched 8-KiB tile (super-group, column) alone: no atomics, and
 * untouched tiles are neither read nor written.
 * dpf_pir_db_gather_sliced_wide_dev writes d_out[i * rec_bytes ..) = record
 * d_idx[i] in row-major form, indices in any order, zeros for
 * d_idx[i] >= nrec. */
int dpf_pir_db_update_sliced_wide_dev(int device, uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                                      const uint64_t* d_idx, const uint8_t* d_recs, size_t n, void* stream);
int dpf_pir_db_gather_sliced_wide_dev(int device, const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                                      const uint64_t* d_idx, size_t n, uint8_t* d_out, void* stream);
/* Private writes, the dual of the fold and the server step of a two-server
 * private write: for every key k with a message m_k,
 *   d_db / d_dbs record i ^= XOR over k < nkeys with bit i of d_bits[k] set
 *                            of d_msgs[k],   for i < nrec
 * (bit i = bit i%8 of byte i/8, EvalFull's layout).  Two servers that apply
 * the same messages under their shares of the keys change the XOR of their
 * DBs by m_k at alpha_k only.  The messages themselves are not hidden.
 * d_bits [nkeys][bits_stride] (bits_stride a multiple of 16, nrec <=
 * 8*bits_stride), d_msgs [nkeys][rec_bytes], rec_bytes a positive multiple of
 * 32 up to DPF_PIR_MAX_REC_BYTES; d_bits, d_msgs and the DB 16-byte aligned
 * and not null (else DPF_ERR_PARAM, checked before any device call);
 * nkeys == 0 or nrec == 0 returns DPF_OK without a launch.  Asynchronous on
 * `stream`, no workspace, no atomics.  dpf_xor_scatter_dev takes the
 * row-major DB [nrec][rec_bytes], dpf_xor_scatter_sliced_wide_dev the wide
 * sliced layout (32 is its C = 1 case).  Selection bits at positions >= nrec
 * are ignored whatever the caller left there, so the padding of the last
 * super-group stays zero ("records past nrec read as 0").  In the sliced
 * layout the 32 records of a word are the 32 selection bits of one u32 of a
 * key's row, so the kernel transposes nothing: each 8-KiB tile (super-group,
 * column) is read once and written once per tile of 64 keys, and more keys
 * are further passes over the DB.  dpf_set_fold_limits bounds its launches
 * too (workgroups per launch; super-groups per workgroup). */
int dpf_xor_scatter_dev(int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys, const uint8_t* d_msgs,
                        uint8_t* d_db, uint64_t nrec, size_t rec_bytes, void* stream);
int dpf_xor_scatter_sliced_wide_dev(int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys,
                                    const uint8_t* d_msgs, uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                                    void* stream);
/* The subtree EvalFull of the keys into d_work, then the scatter: the dual
 * of dpf_pir_answer_wide_dev / dpf_pir_answer_sliced_wide_dev, with their
 * slice contract (d_db holds nrec <= 2^(logN-prefix_bits) records of subtree
 * (prefix_bits, prefix), more is DPF_ERR_PARAM) and workspace
 * (dpf_pir_workspace_size(nkeys, logN, prefix_bits) bytes, 16-byte aligned).
 * Always a tree launch followed by the scatter; DPF_PIR_FUSED has no part in
 * it.  d_keys, d_msgs, the DB and d_work not null, the last three 16-byte
 * aligned (else DPF_ERR_PARAM before any device call). */
int dpf_pir_write_wide_dev(int device, const uint8_t* d_keys, size_t key_len, size_t nkeys, uint32_t logN,
                           uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_msgs, uint8_t* d_db, uint64_t nrec,
                           size_t rec_bytes, void* d_work, void* stream);
int dpf_pir_write_sliced_wide_dev(int device, const uint8_t* d_keys, size_t key_len, size_t nkeys, uint32_t logN,
                                  uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_msgs, uint8_t* d_dbs,
                                  uint64_t nrec, size_t rec_bytes, void* d_work, void* stream);
/* Records of any width over the sliced layout.  The layout is defined for
 * every rec_bytes that is a positive multiple of 4 up to
 * DPF_PIR_MAX_REC_BYTES, and is ABI.  As a u32 array:
 *   dbs[S][p][g]: super-group S of 256 records, p < 8*rec_bytes the bit
 *   position of the record (bit p%8 of its byte p/8), record group g < 8;
 *   bit j of the word = bit p of record 256*S + 32*g + j.  Records past nrec
 *   read as 0.
 * A super-group is 8*rec_bytes rows of 8 words and the next one follows
 * directly: rows past a record's last bit do not exist.  The size is
 * ceil(nrec/256) * 256 * rec_bytes bytes (minimum 16), a chunk that starts at
 * a multiple of 256 records is still a contiguous sub-range (at byte
 * S0*256*rec_bytes), and for rec_bytes = 32*C the layout is the wide layout
 * above, byte for byte (p = 256*c + n).  Stored this way a table of 16-byte
 * records takes half the memory, and the fold half the DB traffic, of the
 * same table padded to 32 bytes.
 * A multiple of 4 because a tile of 32 rows is the unit of the fold, of an
 * answer word and of a selection word; other widths go through
 * dpf_pir_db_create_any below, which pads records to the next multiple of 4 on
 * the device.  The record is rec_bytes/4 such tiles in ceil(rec_bytes/32)
 * columns of up to 8, the last column possibly short; the kernels are those of
 * the _wide entry points, which skip the tiles a record does not have (no
 * load, no answer word).
 * Each _any entry point below is its _wide counterpart with that width rule:
 * rec_bytes that is 0, not a multiple of 4 or above DPF_PIR_MAX_REC_BYTES is
 * DPF_ERR_PARAM (the size function returns 0), checked before any device call
 * and before the other arguments; alignment (of the base pointers: rows of
 * d_db, d_recs, d_out, d_msgs and d_ans are [n][rec_bytes], tightly packed,
 * and need not be 16-byte aligned themselves), null, nrec, bits_stride and
 * prefix rules, workspace sizes and asynchrony are those of the _wide form.
 * The _wide entry points keep rejecting widths that are not multiples of 32. */
size_t dpf_pir_db_sliced_size_any(uint64_t nrec, size_t rec_bytes);
int dpf_pir_db_slice_any_dev(int device, const uint8_t* d_db, uint64_t nrec, size_t rec_bytes, uint8_t* d_dbs,
                             void* stream);
int dpf_xor_fold_sliced_any_dev(int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys,
                                const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes, uint8_t* d_ans, void* d_work,
                                void* stream);
int dpf_pir_answer_sliced_any_dev(int device, const uint8_t* d_keys, size_t key_len, size_t nkeys, uint32_t logN,
                                  uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_dbs, uint64_t nrec,
                                  size_t rec_bytes, uint8_t* d_ans, void* d_work, void* stream);
int dpf_pir_db_update_sliced_any_dev(int device, uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                                     const uint64_t* d_idx, const uint8_t* d_recs, size_t n, void* stream);
int dpf_pir_db_gather_sliced_any_dev(int device, const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                                     const uint64_t* d_idx, size_t n, uint8_t* d_out, void* stream);
int dpf_xor_scatter_sliced_any_dev(int device, const uint8_t* d_bits, size_t bits_stride, size_t nkeys,
                                   const uint8_t* d_msgs, uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                                   void* stream);
int dpf_pir_write_sliced_any_dev(int device, const uint8_t* d_keys, size_t key_len, size_t nkeys, uint32_t logN,
                                 uint32_t prefix_bits, uint64_t prefix, const uint8_t* d_msgs, uint8_t* d_dbs,
                                 uint64_t nrec, size_t rec_bytes, void* d_work, void* stream);
/* Tuning / test limits of the XOR fold launches (process-wide; 0 = default):
 * at most max_blocks workgroups per fold launch (default and maximum 1024),
 * and at most max_sg_per_block super-groups of 256 records per matrix-core
 * fold workgroup (default and maximum 2^15).  The matrix-core fold's answer
 * bits are parities of fp32 counts, exact up to 2^24; with at most 2^23
 * records per workgroup no count gets there, and a DB with more super-groups
 * than max_blocks x max_sg_per_block is folded in passes.  Answers do not
 * depend on either; tests use them to force multi-pass folds.  Returns 0. */
int dpf_set_fold_limits(uint32_t max_blocks, uint32_t max_sg_per_block);
/* Kernel shape of dpf_pir_answer_sliced_dev (and of a sliced PIR handle):
 * DPF_PIR_SPLIT (default): a tree launch writes the selection bits to HBM
 * and a fold launch reads them back.  DPF_PIR_FUSED: where nkeys <= 64 and
 * the slice holds 2^8..2^10 blocks of 256 leaf pairs (logN - prefix_bits =
 * 24..26), one launch runs the subtree EvalFull and the matrix-core fold
 * together (k_pir_fused: per CU, 12 waves expand the tree with one key per
 * lane and 4 waves fold each leaf pair from LDS), so the selection bits
 * never reach HBM; measured slower on MI355X, the split
 * path elsewhere.  DPF_PIR_FUSED_ANY fuses any slice from logN -
 * prefix_bits = 16 (test mode).  Answers are identical.  The fused kernel is
 * linked only into the experimental library (make -C dpf-go_amd
 * experimental: the product library's objects plus csrc/pir_fused.hip and
 * csrc/eval_trie.hip): the product library returns DPF_ERR_PARAM for DPF_PIR_FUSED and
 * DPF_PIR_FUSED_ANY.  The fused launcher reads a device symbol synchronously
 * before it launches, so a call that takes the fused choice cannot be recorded
 * in a stream capture; the split path can.  Process-wide; env
 * DPF_PIR_KERNEL=split|fused|fused-any. */
#define DPF_PIR_SPLIT 0
#define DPF_PIR_FUSED 1
#define DPF_PIR_FUSED_ANY 2
int dpf_set_pir_kernel(int kernel);   /* returns the previous kernel */
int dpf_get_pir_kernel(void);
/* What dpf_pir_answer_sliced_dev runs for this shape under the current
 * setting and AES back end: DPF_PIR_FUSED or DPF_PIR_SPLIT. */
int dpf_pir_kernel_for(size_t nkeys, uint32_t logN, uint32_t prefix_bits);

/* Host form: the DB is uploaded once, sharded by top-level subtree over
 * ngpus devices (a power of two), each GPU folds its slice and the host
 * XORs the per-GPU partial answers (RCCL has no XOR reduction). */
int dpf_pir_db_create(const uint8_t* db, uint64_t nrec, uint32_t logN, int ngpus, void** handle);
int dpf_pir_answer(void* handle, const uint8_t* keys, size_t key_len, size_t nkeys, uint8_t* ans);
/* The same for records of rec_bytes bytes (a positive multiple of 32 up to
 * DPF_PIR_MAX_REC_BYTES, else DPF_ERR_PARAM with *handle = NULL);
 * dpf_pir_db_create is the rec_bytes = 32 case.  The shards are kept in the
 * wide sliced layout (row-major with env DPF_PIR_FOLD=lds), uploaded through
 * a staging buffer of at most 256 MiB in chunks of whole super-groups.
 * dpf_pir_answer on the handle writes nkeys * dpf_pir_db_rec_bytes(handle)
 * bytes. */
int dpf_pir_db_create_wide(const uint8_t* db, uint64_t nrec, size_t rec_bytes, uint32_t logN, int ngpus,
                           void** handle);
/* The same for records of every width, 1 .. DPF_PIR_MAX_REC_BYTES bytes (else
 * DPF_ERR_PARAM with *handle = NULL).  db is [nrec][rec_bytes], tightly
 * packed.  The shards hold each record in (rec_bytes+3)&~3 bytes of the
 * any-width sliced layout above; the pad bytes are zero and stay zero.
 * Upload, answers, updates, reads and writes convert between the caller's
 * tight rows and the device's padded ones by pitched copies, so
 * dpf_pir_answer, dpf_pir_db_update, dpf_pir_db_read and dpf_pir_db_write take
 * and return rows of dpf_pir_db_rec_bytes(handle) bytes, the caller's width,
 * under their contracts below.  With env DPF_PIR_FOLD=lds (row-major shards) a
 * width that is not a multiple of 32 is DPF_ERR_PARAM with *handle = NULL.
 * For a multiple of 32 the handle is what dpf_pir_db_create_wide makes. */
int dpf_pir_db_create_any(const uint8_t* db, uint64_t nrec, size_t rec_bytes, uint32_t logN, int ngpus, void** handle);
size_t dpf_pir_db_rec_bytes(void* handle);
/* Records the handle was created with (0 for NULL). */
uint64_t dpf_pir_db_nrec(void* handle);
/* Change / read back n records of a resident DB in place: record idx[i] :=
 * recs[i * rec_bytes ..), resp. out[i * rec_bytes ..) := record idx[i].  idx
 * may be in any order and may repeat; of repeated indices the last update
 * wins, and a read returns the records in the caller's order.  Every index
 * is checked against dpf_pir_db_nrec first: one index >= nrec returns
 * DPF_ERR_PARAM and nothing is changed (a DB does not grow).  The host sorts
 * the updates (stably), splits them by shard and sends each shard's part
 * through a staging buffer in chunks of at most 256 MiB of records; a chunk
 * runs on its device's stream under that device's mutex, so a concurrent
 * dpf_pir_answer sees the DB wholly before or wholly after each chunk.
 * Sliced shards take dpf_pir_db_update_sliced_wide_dev, row-major ones
 * (DPF_PIR_FOLD=lds) a plain scatter.  Synchronous. */
int dpf_pir_db_update(void* handle, const uint64_t* idx, const uint8_t* recs, size_t n);
int dpf_pir_db_read(void* handle, const uint64_t* idx, size_t n, uint8_t* out);
/* Private write to a resident DB: every shard applies the batch to its slice
 * (dpf_pir_write_sliced_wide_dev; row-major shards dpf_pir_write_wide_dev).
 * keys [nkeys][key_len], msgs [nkeys][dpf_pir_db_rec_bytes(handle)].  A short
 * key is DPF_ERR_KEYLEN and nothing is changed.  Per shard the batch runs on
 * the device's stream under that device's mutex, so a concurrent
 * dpf_pir_answer sees a shard wholly before or wholly after the batch; writes
 * to different shards are not atomic with respect to each other, as for
 * dpf_pir_db_update.  Synchronous. */
int dpf_pir_db_write(void* handle, const uint8_t* keys, size_t key_len, size_t nkeys, const uint8_t* msgs);
void dpf_pir_db_free(void* handle);

/* ---- windows of the domain: sub-keys, window EvalFull, PIR over any range --
 * A node (s, t) of the GGM tree with the remaining correction words is a DPF
 * key of the smaller domain.  dpf_subkeys_dev is that re-rooting on the
 * device: key k walked prefix_bits levels (<= logN - 7) along first_prefix + p
 * becomes the key of subtree (prefix_bits, first_prefix + p), key_len - 18 *
 * prefix_bits bytes (seed, t, then key bytes [17 + 18 * prefix_bits, key_len)
 * unchanged) at d_sub[k * nprefix + p], for p < nprefix, first_prefix + nprefix
 * <= 2^prefix_bits.  Its EvalFull at logN - prefix_bits is that subtree's slice
 * of the deep key's EvalFull, byte for byte, for malformed keys too; every
 * entry point that takes keys takes it.  key_len >= 33 + 18 * prefix_bits, no
 * alignment of d_keys or d_sub.  prefix_bits = 0 copies the keys.
 *
 * A window is points [128 * first_block, 128 * (first_block + nblocks)) of the
 * 2^logN domain (logN <= 63, nblocks >= 1, inside the domain, else
 * DPF_ERR_PARAM).  dpf_window_form_for says, without a device, how the window
 * forms evaluate it: DPF_WINDOW_SUBTREE where an aligned subtree of at most
 * twice the window's points holds it (the window itself, where it is one; any
 * window at logN < 7) -- the prefixed tree launch of dpf_evalfull_subtree_dev,
 * one piece, the window at row_offset of the subtree's bytes -- else
 * DPF_WINDOW_PIECES: npieces <= 33 consecutive aligned pieces of 2^s points, s
 * = max(floor(log2(128 * nblocks)) - 4, 7), each the whole domain of one
 * sub-key, so that at most two pieces' worth of points, under 1/8 of the
 * window, is evaluated outside it.  (Measured on one MI355X, DESIGN.md 4.4: up
 * to twice the points the one subtree is as fast or faster than the pieces.)
 * dpf_evalfull_window_dev writes row k, the pieces of key k side by side
 * (row_bytes = npieces * piece_bytes), at d_rows + k * row_stride; the
 * window's 16 * nblocks bytes begin at byte row_offset of a row.  row_stride:
 * a multiple of 16, at least row_bytes; with row_stride == row_bytes all
 * nkeys * npieces sub-keys go through one tree launch, a larger stride takes
 * one launch per key.  d_rows and d_work 16-byte aligned; d_work holds
 * dpf_evalfull_window_workspace_size bytes (0 for a refused window).
 *
 * The PIR forms: d_dbs is the any-width sliced layout (rec_bytes a positive
 * multiple of 4 up to DPF_PIR_MAX_REC_BYTES) of records [first_rec, first_rec
 * + nrec) of the domain, first_rec a multiple of 128, first_rec + nrec <=
 * 2^logN.  The answer for key k is the XOR of the records first_rec + j whose
 * bit of EvalFull(key_k) is set (d_ans [nkeys][rec_bytes], overwritten; zeros
 * for nrec == 0); the write is the dual.  Each is the window EvalFull of blocks
 * [first_rec / 128, ... + ceil(nrec / 128)) into rows inside d_work, then
 * dpf_xor_fold_sliced_any_dev / dpf_xor_scatter_sliced_any_dev from row_offset
 * at stride row_bytes; DPF_PIR_FUSED has no part in either.  d_work holds
 * dpf_pir_window_workspace_size bytes (0 for refused arguments).  Checked
 * before any device call, in this order: rec_bytes, the key length
 * (DPF_ERR_KEYLEN), first_rec, the range, then null and misaligned buffers as
 * for the dense forms above.  All asynchronous on `stream`, with no
 * allocation, memset or synchronisation: the stream-capture contract of the
 * _dev calls above holds. */
#define DPF_WINDOW_SUBTREE 0
#define DPF_WINDOW_PIECES 1
typedef struct dpf_window_form {
    uint32_t route;         /* DPF_WINDOW_SUBTREE / DPF_WINDOW_PIECES */
    uint32_t prefix_bits;   /* levels from the root to a piece's root */
    uint64_t first_prefix;  /* the first piece among the 2^prefix_bits */
    uint64_t npieces;
    uint64_t piece_bytes;   /* EvalFull bytes of a piece */
    uint64_t row_bytes;     /* npieces * piece_bytes */
    uint64_t row_offset;    /* byte of a row at which the window starts, a multiple of 16 */
    uint64_t sub_key_len;   /* key_len - 18 * prefix_bits (key_len on the subtree route) */
} dpf_window_form;
int dpf_window_form_for(uint32_t logN, uint64_t first_block, uint64_t nblocks, size_t key_len, dpf_window_form* form);
int dpf_subkeys_dev(int device, const uint8_t* d_keys, size_t key_len, size_t nkeys, uint32_t logN, uint32_t prefix_bits,
                    uint64_t first_prefix, uint64_t nprefix, uint8_t* d_sub, void* stream);
size_t dpf_evalfull_window_workspace_size(size_t nkeys, uint32_t logN, uint64_t first_block, uint64_t nblocks);
int dpf_evalfull_window_dev(int device, const uint8_t* d_keys, size_t key_len, size_t nkeys, uint32_t logN,
                            uint64_t first_block, uint64_t nblocks, uint8_t* d_rows, size_t row_stride, void* d_work,
                            void* stream);
size_t dpf_pir_window_workspace_size(size_t nkeys, uint32_t logN, uint64_t first_rec, uint64_t nrec, size_t rec_bytes);
int dpf_pir_answer_window_dev(int device, const uint8_t* d_keys, size_t key_len, size_t nkeys, uint32_t logN,
                              uint64_t first_rec, const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes, uint8_t* d_ans,
                              void* d_work, void* stream);
int dpf_pir_write_window_dev(int device, const uint8_t* d_keys, size_t key_len, size_t nkeys, uint32_t logN,
                             uint64_t first_rec, const uint8_t* d_msgs, uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                             void* d_work, void* stream);
/* A resident DB of the ranged dense kind: record j lives at domain point j, as
 * for dpf_pir_db_create_any, but the shards are balanced record ranges, not
 * subtrees: ngpus is any count up to the opened devices (<= 0: all of them),
 * shard g holds the ceil(ceil(nrec/256) / ngpus) * 256 records starting at g
 * times that many (the sparse kind's split) and answers and writes through the
 * window forms with that first_rec.  Every other handle call keeps its
 * contract.  With env DPF_PIR_FOLD=lds (row-major shards) creation is
 * DPF_ERR_PARAM. */
int dpf_pir_db_create_ranged(const uint8_t* db, uint64_t nrec, size_t rec_bytes, uint32_t logN, int ngpus, void** handle);

/* ---- PIR over a sparse key set (keyword PIR) ----------------------------
 * Record j of the DB lives at domain point d_points[j], any point of the
 * 2^logN domain, instead of at position j of a subtree: the client hashes its
 * keyword to a point, runs Gen(point, logN) and sends one key to each server.
 * The selection bits come from dpf_eval_bits_dev at the records' points; the
 * fold and the scatter are those of the dense entry points.
 * Device forms: d_dbs is the any-width sliced layout of nrec records
 * (rec_bytes a positive multiple of 4 up to DPF_PIR_MAX_REC_BYTES), d_points
 * [nrec] uint64.  The answer for key k is the XOR of the records j with
 * Eval(key_k, d_points[j]) = 1 (d_ans [nkeys][rec_bytes], overwritten; zeros
 * for nrec == 0); the write is the dual, record j ^= XOR of d_msgs[k] over the
 * same keys.  Points may repeat: such records are selected together.  Each is
 * dpf_eval_bits_dev into a bit area inside d_work, then the fold
 * (dpf_xor_fold_sliced_any_dev) or the scatter
 * (dpf_xor_scatter_sliced_any_dev); DPF_PIR_FUSED has no part in either.
 * d_work holds dpf_pir_sparse_workspace_size(nkeys, nrec, logN) bytes: the
 * Eval-bits workspace, nkeys * dpf_eval_bits_stride(nrec) bytes of bit rows
 * and dpf_xor_fold_workspace_size(), each rounded up to 16 bytes.  Checked
 * before any device call, in this order: rec_bytes (DPF_ERR_PARAM), the key
 * length (DPF_ERR_KEYLEN), then null and misaligned buffers (DPF_ERR_PARAM;
 * d_dbs, d_msgs and d_work 16-byte, d_points 8-byte, d_ans 4-byte aligned;
 * the answer form allows null buffers it has no work for, the write form
 * none).  nkeys == 0, and for the write nrec == 0, return DPF_OK without a
 * launch.  Asynchronous on `stream`. */
size_t dpf_pir_sparse_workspace_size(size_t nkeys, uint64_t nrec, uint32_t logN);
int dpf_pir_answer_sparse_dev(int device, const uint8_t* d_keys, size_t key_len, size_t nkeys, uint32_t logN,
                              const uint64_t* d_points, const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                              uint8_t* d_ans, void* d_work, void* stream);
int dpf_pir_write_sparse_dev(int device, const uint8_t* d_keys, size_t key_len, size_t nkeys, uint32_t logN,
                             const uint64_t* d_points, const uint8_t* d_msgs, uint8_t* d_dbs, uint64_t nrec,
                             size_t rec_bytes, void* d_work, void* stream);
/* A resident DB of the sparse kind: points [nrec] and db [nrec][rec_bytes]
 * (tightly packed, every width 1 .. DPF_PIR_MAX_REC_BYTES, padded to a
 * multiple of 4 on the device as dpf_pir_db_create_any does).  logN <= 63,
 * and a point >= 2^logN is DPF_ERR_PARAM (*handle = NULL).  Repeated points
 * are allowed: both records are selected together, so a client reads their
 * XOR.  ngpus is any count up to the opened devices (<= 0: all of them):
 * shard g holds the ceil(ceil(nrec/256) / ngpus) * 256 records starting at g
 * times that many, a range of whole super-groups and not a subtree, with its
 * slice of the points beside it in HBM.  The points are fixed at creation.
 * dpf_pir_answer and dpf_pir_db_write on the handle run the sparse device
 * forms per shard and XOR the partial answers on the host;
 * dpf_pir_db_update, dpf_pir_db_read, dpf_pir_db_nrec and
 * dpf_pir_db_rec_bytes keep their contracts, idx being a record's position
 * in the list.  With env DPF_PIR_FOLD=lds (row-major shards) creation is
 * DPF_ERR_PARAM. */
int dpf_pir_db_create_sparse(const uint64_t* points, const uint8_t* db, uint64_t nrec, size_t rec_bytes,
                             uint32_t logN, int ngpus, void** handle);

/* ---- Grouped PIR: many small DBs, each with its own keys -----------------
 * Every form above answers all keys of a batch against one DB.  A grouped DB
 * is ngroups groups of nrec records of rec_bytes each, all of one shape (the
 * owner pads a short group with zero records, which select nothing), and
 * every group has its own keys_per_group keys over its own 2^logN domain: the
 * buckets of a batch code (multi-query PIR: one key per bucket instead of one
 * whole-domain key per wanted record), or many independent tables behind one
 * server.  One fold launch has a group coordinate, so a batch costs launches
 * by the batch and not by the group.
 * Layout: no new format.  d_dbs is the any-width sliced layout of ONE flat DB
 * in which group g, record i sits at flat position g * gs + i, with group
 * stride gs = dpf_pir_group_stride(nrec) = nrec rounded up to a multiple of
 * 256; flat positions [nrec, gs) of every group are zero records.
 * dpf_pir_db_grouped_size is ngroups * gs * rec_bytes (at least 16; 0 for a
 * width that is not a positive multiple of 4 up to DPF_PIR_MAX_REC_BYTES or a
 * product that overflows).  dpf_pir_db_slice_grouped_dev builds it from the
 * tightly packed d_db [ngroups][nrec][rec_bytes] (one slicing launch when
 * nrec is a multiple of 256, else one per group: build time, not the hot
 * path); dpf_pir_db_update_sliced_any_dev, _gather_ and the scatter work on it
 * by flat position, with ngroups * gs as their nrec.
 * dpf_xor_fold_grouped_dev: d_bits is [ngroups * keys_per_group][bits_stride]
 * and row g * keys_per_group + j selects within group g (bit i = record i of
 * the group; bits at positions >= nrec meet zero records only); d_ans
 * [ngroups * keys_per_group][rec_bytes] in the same order, overwritten, zeros
 * for nrec == 0.  bits_stride is a multiple of 16 with a bit for each of the
 * nrec records.  d_work holds dpf_xor_fold_grouped_workspace_size(ngroups,
 * keys_per_group, rec_bytes) bytes.  dpf_set_fold_limits' max_blocks, where
 * below its default, caps the workgroups of each of its launches.
 * Keys per group: up to 4 keys of a group share one pass over its tiles (one
 * launch per pass for all groups).  Many keys per group (from 5: the route
 * rule of csrc/pir_group_fold_plan.hpp), the clients of a batched server for
 * instance, take the matrix-core grouped fold instead: one pass and one
 * launch per 256 keys of every group, with dpf_set_fold_limits'
 * max_sg_per_block bounding a workgroup's run as in the dense matrix-core
 * fold; the workspace is the same and is not written.  Env
 * DPF_GROUP_FOLD_ROUTE=direct|mfma, read at every call, forces the route for
 * every caller of the grouped fold, the grouped answers and the grouped
 * handles (measurement only; leave it unset).  dpf_fold_grouped_form_for below
 * tells which route a shape takes.
 * dpf_pir_answer_grouped_dev: d_keys is [ngroups * keys_per_group][key_len] in
 * that order; one tree pass of all the keys over the whole 2^logN domain into
 * a bit area inside d_work, then the grouped fold.  DPF_PIR_FUSED has no part
 * in it.  d_work holds dpf_pir_grouped_workspace_size(ngroups,
 * keys_per_group, logN, rec_bytes) bytes: the tree workspace of all the keys
 * (dpf_workspace_size) and their EvalFull rows (dpf_evalfull_len each), both
 * rounded up to 256 bytes, and the grouped fold's workspace.  Both size
 * functions are 0 for a bad width or a key count that does not fit 32 bits.
 * Checked before any device call, in this order: rec_bytes (DPF_ERR_PARAM);
 * for the answer the key (logN > 63 DPF_ERR_PARAM, then DPF_ERR_KEYLEN) and
 * nrec > 2^logN, for the fold bits_stride (DPF_ERR_PARAM); ngroups *
 * keys_per_group not fitting 32 bits (DPF_ERR_PARAM); null buffers the call
 * has work for; misaligned buffers (d_dbs, d_bits and d_work 16-byte, d_ans
 * 4-byte).  ngroups == 0 or keys_per_group == 0 returns DPF_OK without a
 * launch.  Asynchronous on `stream`. */
uint64_t dpf_pir_group_stride(uint64_t nrec);
size_t dpf_pir_db_grouped_size(uint64_t ngroups, uint64_t nrec, size_t rec_bytes);
int dpf_pir_db_slice_grouped_dev(int device, const uint8_t* d_db, uint64_t ngroups, uint64_t nrec, size_t rec_bytes,
                                 uint8_t* d_dbs, void* stream);
size_t dpf_xor_fold_grouped_workspace_size(uint64_t ngroups, uint64_t keys_per_group, size_t rec_bytes);
int dpf_xor_fold_grouped_dev(int device, const uint8_t* d_bits, size_t bits_stride, uint64_t ngroups,
                             uint64_t keys_per_group, const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                             uint8_t* d_ans, void* d_work, void* stream);
size_t dpf_pir_grouped_workspace_size(uint64_t ngroups, uint64_t keys_per_group, uint32_t logN, size_t rec_bytes);
int dpf_pir_answer_grouped_dev(int device, const uint8_t* d_keys, size_t key_len, uint64_t ngroups,
                               uint64_t keys_per_group, uint32_t logN, const uint8_t* d_dbs, uint64_t nrec,
                               size_t rec_bytes, uint8_t* d_ans, void* d_work, void* stream);
/* What dpf_xor_fold_grouped_dev launches for a shape under the current
 * dpf_set_fold_limits, on `cus` CUs (<= 0: the current device's / the calling
 * thread's stream budget; needs no device when cus > 0) and, like the call
 * itself, under env DPF_GROUP_FOLD_ROUTE where set.  DPF_ERR_PARAM for a bad
 * width, a key count that does not fit 32 bits or a null form; ngroups == 0,
 * keys_per_group == 0 or nrec == 0 has launches == 0 (the clear of nrec == 0
 * is not counted).  Where the keys of a group take several key tiles of
 * different shapes, columns_per_wg, keys_per_tile, runs, sg_per_run and units
 * are those of the first (the widest) tile. */
#define DPF_FOLD_GROUPED_DIRECT 0 /* up to 4 keys of a group per pass over the DB */
#define DPF_FOLD_GROUPED_MFMA 1   /* the matrix-core grouped fold: up to 256 keys per pass */
typedef struct dpf_fold_grouped_form {
    uint32_t route;          /* DPF_FOLD_GROUPED_* above */
    uint32_t columns_per_wg; /* 32-byte columns a workgroup folds (1 on the direct route) */
    uint32_t keys_per_tile;  /* keys of a group per pass at the most: 4 (direct), 32 .. 256 (the tile shape) */
    uint32_t atomic;         /* 1: the answers are cleared first and the runs' words XORed in atomically */
    uint64_t runs;           /* workgroups per (group, column group) */
    uint64_t sg_per_run;     /* super-groups per run (the last run: what is left) */
    uint64_t units;          /* workgroups per pass */
    uint64_t passes;         /* passes over the DB: key passes (direct) or key tiles */
    uint64_t launches;       /* fold launches of all passes (the clear is not counted) */
    uint64_t max_blocks;     /* workgroups per launch at the most */
} dpf_fold_grouped_form;
int dpf_fold_grouped_form_for(uint64_t ngroups, uint64_t keys_per_group, uint64_t nrec, size_t rec_bytes, int cus,
                              dpf_fold_grouped_form* form);
/* A resident DB of the grouped kind: db [ngroups][nrec][rec_bytes], tightly
 * packed, every width 1 .. DPF_PIR_MAX_REC_BYTES (padded to a multiple of 4
 * on the device as dpf_pir_db_create_any does); logN <= 63 and nrec <= 2^logN
 * (the domain of ONE group).  ngpus is any count up to the opened devices
 * (<= 0: all of them): shard s holds the ceil(ngroups / ngpus) whole groups
 * starting at s times that many.  dpf_pir_answer on the handle requires nkeys
 * to be a multiple of ngroups (else DPF_ERR_PARAM): keys is [ngroups][kpg]
 * and ans has the same order; each shard receives its groups' key rows and
 * writes its groups' answers, with no host XOR.  dpf_pir_db_update and
 * dpf_pir_db_read take idx = g * nrec + i, < ngroups * nrec, and keep their
 * contracts; dpf_pir_db_nrec is ngroups * nrec.  dpf_pir_db_ngroups is the
 * group count (1 for the other kinds of handle, 0 for NULL).
 * dpf_pir_db_write on a grouped handle is DPF_ERR_PARAM (its keys are one
 * batch over one DB): the grouped private write is dpf_pir_db_write_grouped
 * below.  With env DPF_PIR_FOLD=lds creation is DPF_ERR_PARAM. */
int dpf_pir_db_create_grouped(const uint8_t* db, uint64_t ngroups, uint64_t nrec, size_t rec_bytes, uint32_t logN,
                              int ngpus, void** handle);
uint64_t dpf_pir_db_ngroups(void* handle);

/* ---- Grouped private writes: the dual of the grouped fold ----------------
 * d_bits and d_msgs are [ngroups * keys_per_group] rows in group order, and
 * for i < nrec
 *   group g, record i ^= XOR over k < keys_per_group, with bit i of
 *                        d_bits row g * keys_per_group + k set,
 *                        of d_msgs row g * keys_per_group + k.
 * Bit i of a row is bit i of the GROUP's domain, as in the grouped fold.  Flat
 * positions [nrec, dpf_pir_group_stride(nrec)) of every group stay zero
 * whatever the caller left in the bits past nrec, and a row's words past its
 * end are not read.  A key with an all-zero message is a dummy and changes
 * nothing.  Two servers that apply the same messages under their shares of the
 * keys change the XOR of their DBs by message k at (g, alpha_k) only.
 * dpf_xor_scatter_grouped_dev: caller-made bits, bits_stride a multiple of 16
 * with a bit for each of the nrec records; no workspace.  One 1-D launch per
 * key pass (4 keys of every group, the last pass the 1 to 3 left: kpg keys are
 * ceil(kpg / 4) passes over the DB) covers all groups; few large groups
 * with many keys each go through one dense scatter per group instead (the
 * plan's route rule, csrc/pir_group_scatter_plan.hpp).  dpf_set_fold_limits'
 * max_blocks, where below its default, caps the workgroups of each launch, and
 * max_sg_per_block the super-groups a workgroup rewrites.  Env
 * DPF_GROUP_SCATTER_ROUTE=grouped|loop, read at every call, forces the route
 * for every caller of these entries (measurement only; leave it unset).
 * dpf_pir_write_grouped_dev: d_keys is [ngroups * keys_per_group][key_len] in
 * that order; one tree pass of all the keys over the whole 2^logN domain into
 * the bit area inside d_work, then the grouped scatter.  d_work holds
 * dpf_pir_grouped_workspace_size(ngroups, keys_per_group, logN, rec_bytes)
 * bytes, the answer's workspace.  Both AES back ends; DPF_PIR_FUSED has no
 * part in it.
 * Checked before any device call, in this order: rec_bytes (DPF_ERR_PARAM);
 * for the scatter bits_stride, for the write the key (logN > 63 DPF_ERR_PARAM,
 * then DPF_ERR_KEYLEN) and nrec > 2^logN (DPF_ERR_PARAM); ngroups *
 * keys_per_group not fitting 32 bits; a null buffer (every buffer must be
 * given, as for the other scatters); a buffer that is not 16-byte aligned
 * (d_bits, d_msgs, d_dbs, d_work).  ngroups == 0, keys_per_group == 0 or
 * nrec == 0 then returns DPF_OK without a launch.  Both are asynchronous on
 * `stream` and can be captured: no synchronisation, no allocation, no memset. */
int dpf_xor_scatter_grouped_dev(int device, const uint8_t* d_bits, size_t bits_stride, uint64_t ngroups,
                                uint64_t keys_per_group, const uint8_t* d_msgs, uint8_t* d_dbs, uint64_t nrec,
                                size_t rec_bytes, void* stream);
int dpf_pir_write_grouped_dev(int device, const uint8_t* d_keys, size_t key_len, uint64_t ngroups,
                              uint64_t keys_per_group, uint32_t logN, const uint8_t* d_msgs, uint8_t* d_dbs,
                              uint64_t nrec, size_t rec_bytes, void* d_work, void* stream);
/* The private write of a grouped handle: keys [nkeys][key_len] and msgs
 * [nkeys][dpf_pir_db_rec_bytes(handle)], nkeys = ngroups * kpg in group order
 * (row g * kpg + j writes into group g); nkeys not a multiple of the handle's
 * groups is DPF_ERR_PARAM, a handle that is not grouped is DPF_ERR_PARAM, a
 * short key is DPF_ERR_KEYLEN, and nothing is changed.  Shard s receives only
 * its groups' key and message rows and runs dpf_pir_write_grouped_dev on its
 * device's stream under that device's mutex, with dpf_pir_db_write's
 * guarantees towards concurrent calls.  Synchronous. */
int dpf_pir_db_write_grouped(void* handle, const uint8_t* keys, size_t key_len, size_t nkeys, const uint8_t* msgs);
/* What dpf_xor_scatter_grouped_dev launches for a shape under the current
 * dpf_set_fold_limits, on `cus` CUs (<= 0: the current device's / the calling
 * thread's stream budget; needs no device when cus > 0) and, like the call
 * itself, under env DPF_GROUP_SCATTER_ROUTE where set.  DPF_ERR_PARAM for a
 * bad width or a key count that does not fit 32 bits. */
#define DPF_SCATTER_GROUPED 0 /* the grouped kernel, one launch per key pass */
#define DPF_SCATTER_LOOP 1    /* one dense scatter per group */
typedef struct dpf_scatter_grouped_form {
    uint32_t route;       /* DPF_SCATTER_* above; the fields below describe the grouped kernel's launches */
    uint32_t columns;     /* 32-byte columns of a record, the last one possibly short */
    uint32_t pass_widths; /* bit w - 1 set: a key pass of width w (1 .. 4) is used */
    uint32_t pad_;
    uint64_t runs;        /* workgroups per (group, column) */
    uint64_t sg_per_run;  /* super-groups per run (the last run: what is left) */
    uint64_t units;       /* workgroups per key pass */
    uint64_t max_blocks;  /* workgroups per launch at the most */
    uint64_t passes;      /* key passes */
    uint64_t launches;    /* launches of all passes */
} dpf_scatter_grouped_form;
int dpf_scatter_grouped_form_for(uint64_t ngroups, uint64_t keys_per_group, uint64_t nrec, size_t rec_bytes, int cus,
                                 dpf_scatter_grouped_form* form);

/* ---- Grouped keyword PIR: every group's records at its own points ---------
 * The grouped and the sparse kinds composed: ngroups groups of nrec records,
 * and record i of group g lives at domain point d_points[g][i], any point of a
 * 2^logN domain with logN <= 63 (keywords hashed to points, cuckoo-hashed into
 * buckets; or many keyword tables behind one server).  d_points is
 * [ngroups][nrec] uint64, tightly packed: it is NOT padded to the group
 * stride.  d_dbs is the grouped layout of dpf_pir_db_slice_grouped_dev (group
 * stride dpf_pir_group_stride(nrec)); d_keys, d_ans and d_msgs are
 * [ngroups * keys_per_group] rows in group order.  Points may repeat within a
 * group (such records are selected together), and nrec > 2^logN is not an
 * error, as for the sparse forms.
 * Each composite is dpf_eval_bits_grouped_dev into a bit area inside d_work,
 * then the grouped fold (dpf_xor_fold_grouped_dev) or the grouped scatter
 * (dpf_xor_scatter_grouped_dev): launches by the batch, not by the group.  The
 * bit rows keep the stride dpf_eval_bits_stride(nrec), also where that is 16
 * bytes (nrec <= 128) and a super-group of 256 records would have 32: the
 * grouped fold, like the scatter, reads no word past a row's end, so the rows
 * are not rounded up and no gap is zeroed.
 * d_work holds dpf_pir_grouped_sparse_workspace_size bytes: the Eval-bits
 * workspace dpf_eval_bits_workspace_size(ngroups * keys_per_group, nrec, logN)
 * rounded up to 16 bytes, ngroups * keys_per_group * dpf_eval_bits_stride(nrec)
 * bytes of rows, and dpf_xor_fold_grouped_workspace_size(); 0 for a bad width
 * or a key count that does not fit 32 bits.
 * Checked before any device call, in this order: rec_bytes (DPF_ERR_PARAM);
 * logN > 63 (DPF_ERR_PARAM); the key length (DPF_ERR_KEYLEN); ngroups *
 * keys_per_group not fitting 32 bits, or the points' bytes not fitting 64
 * (DPF_ERR_PARAM); null buffers (the answer allows those it has no work for,
 * the write none, as the grouped write); misaligned buffers (d_dbs, d_msgs and
 * d_work 16-byte, d_points 8-byte, d_ans 4-byte).  ngroups == 0 or
 * keys_per_group == 0 returns DPF_OK without a launch; nrec == 0 makes the
 * answer zero d_ans and the write a no-op.  Asynchronous on `stream` and
 * capturable: no synchronisation, no allocation. */
size_t dpf_pir_grouped_sparse_workspace_size(uint64_t ngroups, uint64_t keys_per_group, uint64_t nrec, uint32_t logN,
                                             size_t rec_bytes);
int dpf_pir_answer_grouped_sparse_dev(int device, const uint8_t* d_keys, size_t key_len, uint64_t ngroups,
                                      uint64_t keys_per_group, uint32_t logN, const uint64_t* d_points,
                                      const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes, uint8_t* d_ans,
                                      void* d_work, void* stream);
int dpf_pir_write_grouped_sparse_dev(int device, const uint8_t* d_keys, size_t key_len, uint64_t ngroups,
                                     uint64_t keys_per_group, uint32_t logN, const uint64_t* d_points,
                                     const uint8_t* d_msgs, uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes,
                                     void* d_work, void* stream);
/* A resident DB of the grouped keyword kind: points [ngroups][nrec] and db
 * [ngroups][nrec][rec_bytes], both tightly packed, every width 1 ..
 * DPF_PIR_MAX_REC_BYTES (padded to a multiple of 4 on the device as
 * dpf_pir_db_create_any does).  logN <= 63, and a point >= 2^logN is
 * DPF_ERR_PARAM (*handle = NULL); nrec may exceed 2^logN and points may
 * repeat.  Shards are ranges of whole groups exactly as
 * dpf_pir_db_create_grouped cuts them, each with its groups' points beside it
 * in HBM.  The handle is a grouped handle in every other respect:
 * dpf_pir_answer and dpf_pir_db_write_grouped need nkeys to be a multiple of
 * the groups, give each shard its groups' rows, do no host XOR, and run the
 * two composites above; dpf_pir_db_write is DPF_ERR_PARAM; update, read,
 * export, xor_records, clear, nrec, ngroups and rec_bytes keep the grouped
 * handle's contracts with idx = g * nrec + i.  The points are fixed at
 * creation and survive dpf_pir_db_clear.  With env DPF_PIR_FOLD=lds creation
 * is DPF_ERR_PARAM. */
int dpf_pir_db_create_grouped_sparse(const uint64_t* points, const uint8_t* db, uint64_t ngroups, uint64_t nrec,
                                     size_t rec_bytes, uint32_t logN, int ngpus, void** handle);

/* ---- Whole-DB read-out of a resident DB: un-slice, XOR-merge, clear -------
 * A DB that accumulates private writes (a mailbox, a bulletin board) is read
 * out whole at the end of an epoch: each server exports its share, the shares
 * are XORed, and the table is cleared for the next epoch.
 * dpf_pir_db_unslice_any_dev is the inverse of dpf_pir_db_slice_any_dev: d_db
 * [nrec][rec_bytes], row-major and tightly packed, from the any-width sliced
 * layout d_dbs (k_unslice_db: the tiles of up to 4 columns by coalesced 16-byte
 * loads through LDS, a five-step 32 x 32 bit transposition per tile, rows of
 * more than 32 bytes stored through LDS so that consecutive lanes write
 * consecutive bytes).  Exactly nrec * rec_bytes bytes are written: rows
 * past nrec of the last super-group are neither written nor, whatever d_dbs
 * holds there, read into a written row.  As for slicing, a range of whole
 * super-groups is un-sliced by offsetting both pointers: records
 * [256*S0, 256*S0 + n) come from d_dbs + S0*256*rec_bytes into
 * d_db + S0*256*rec_bytes (pass n as nrec).
 * dpf_pir_db_unslice_grouped_dev is the inverse of dpf_pir_db_slice_grouped_dev:
 * d_db [ngroups][nrec][rec_bytes], tight; the zero records behind each group's
 * nrec are not written (one launch per group where groups have padding).
 * dpf_pir_db_xor_sliced_dev: d_dbs ^= d_other over `bytes` bytes, the merge of
 * two sliced (or grouped, or row-major) buffers of one shape; zero padding
 * stays zero.
 * Checked before any device call, in this order: rec_bytes (a positive
 * multiple of 4, at most DPF_PIR_MAX_REC_BYTES) resp. bytes (a multiple of
 * 16); the products of the sizes not fitting 64 bits; a null buffer where
 * there is work; a buffer that is not 16-byte aligned.  All DPF_ERR_PARAM.
 * Nothing to do (nrec == 0, ngroups == 0, bytes == 0) then returns DPF_OK
 * without a launch.  All three are asynchronous on `stream` and can be
 * captured: no synchronisation, no allocation, no memset, no workspace. */
int dpf_pir_db_unslice_any_dev(int device, const uint8_t* d_dbs, uint64_t nrec, size_t rec_bytes, uint8_t* d_db,
                               void* stream);
int dpf_pir_db_unslice_grouped_dev(int device, const uint8_t* d_dbs, uint64_t ngroups, uint64_t nrec,
                                   size_t rec_bytes, uint8_t* d_db, void* stream);
int dpf_pir_db_xor_sliced_dev(int device, uint8_t* d_dbs, const uint8_t* d_other, size_t bytes, void* stream);
/* The same on a handle of any kind (dense, sparse, grouped; any shard count;
 * sliced or, with DPF_PIR_FOLD=lds, row-major shards), over the records
 * [first, first + n) of the handle's index space (a sparse handle: positions
 * in its list; a grouped one: g * nrec + i, the padding behind a group is
 * never delivered).  A range that leaves [0, dpf_pir_db_nrec) -- first + n
 * overflowing included -- is DPF_ERR_PARAM and nothing is changed; n == 0 is
 * DPF_OK; a NULL handle or, with n > 0, a NULL buffer is DPF_ERR_PARAM.
 * dpf_pir_db_export: out [n][dpf_pir_db_rec_bytes(handle)], tight := the
 * records.  dpf_pir_db_xor_records: record first + i ^= recs[i], rows of the
 * same width; the pad bytes and pad records of every shard and group stay
 * zero.  Both walk the range in pieces of whole super-groups of one shard, at
 * most dpf_set_export_limits' bytes each (csrc/pir_export_plan.hpp): a piece
 * is un-sliced into a staging buffer and copied down, resp. staged, sliced and
 * XORed into the shard, on its device's stream under that device's mutex, so a
 * concurrent dpf_pir_answer sees a shard wholly before or wholly after each
 * piece.  dpf_pir_db_clear: every record := 0 (one memset per shard, under the
 * same mutex); a sparse handle keeps its points.  All synchronous.
 * dpf_set_export_limits: tuning / test limit of a piece's staging bytes
 * (process-wide; 0 = the default, 256 MiB; a piece is at least one
 * super-group).  Results do not depend on it.  Returns 0. */
int dpf_pir_db_export(void* handle, uint64_t first, uint64_t n, uint8_t* out);
int dpf_pir_db_xor_records(void* handle, uint64_t first, uint64_t n, const uint8_t* recs);
int dpf_pir_db_clear(void* handle);
int dpf_set_export_limits(size_t chunk_bytes);

#ifdef __cplusplus
}
#endif

#endif /* DPF_HIP_H */
