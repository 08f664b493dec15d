"""Size function and argument checks of the grouped keyword PIR entry points
(include/dpf_hip.h: dpf_eval_bits_grouped_dev, the two grouped-sparse
composites and dpf_pir_db_create_grouped_sparse).  No device is needed: the
sizes are arithmetic, and every DPF_ERR_PARAM / DPF_ERR_KEYLEN case returns
before any device call (with no device a call that got that far would return
DPF_ERR_HIP or fault on the fake pointers, which are never dereferenced)."""
import ctypes

import dpf

P = 1 << 20      # an aligned fake device address
LOGN = 40
KL = 33 + 18 * (LOGN - 7)
SHORT = 17 + 18 * (LOGN - 7) - 1


def test_workspace_size_is_the_sum_of_the_public_parts():
    r16 = lambda x: (x + 15) // 16 * 16
    for rec in (0, 6, 32768 + 4):
        assert dpf.pir_grouped_sparse_workspace_size(3, 2, 100, LOGN, rec) == 0, rec
    assert dpf.pir_grouped_sparse_workspace_size(1 << 31, 2, 100, LOGN, 32) == 0        # 2^32 key rows
    assert dpf.pir_grouped_sparse_workspace_size(1 << 16, 1 << 16, 100, LOGN, 32) == 0
    for ng, kpg, nrec, logN, rec in ((1, 1, 1, 7, 4), (3, 5, 129, 30, 20), (384, 1, 4096, 40, 32), (65, 2, 600, 63, 100),
                                     (96, 1, 1 << 14, 40, 32), (5, 5, 0, 30, 4)):
        nk = ng * kpg
        fold = dpf.xor_fold_grouped_workspace_size(ng, kpg, rec)
        assert fold >= 16 and fold % 16 == 0
        want = r16(dpf.eval_bits_workspace_size(nk, nrec, logN)) + r16(nk * dpf.eval_bits_stride(nrec)) + fold
        assert dpf.pir_grouped_sparse_workspace_size(ng, kpg, nrec, logN, rec) == want, (ng, kpg, nrec, logN, rec)
        assert dpf.pir_grouped_sparse_workspace_size(1, nk, nrec, logN, rec) == want    # a function of the key rows and nrec
    # The rows keep the Eval-bits stride: 16 bytes up to 128 records, not a super-group's 32.
    a = dpf.pir_grouped_sparse_workspace_size(4, 1, 128, 30, 32)
    b = dpf.pir_grouped_sparse_workspace_size(4, 1, 129, 30, 32)
    assert b - a == 4 * 16 + (r16(dpf.eval_bits_workspace_size(4, 129, 30)) - r16(dpf.eval_bits_workspace_size(4, 128, 30)))


def test_eval_bits_grouped_validates_before_touching_a_device():
    L = dpf.lib()

    def bits(keys=P, kl=KL, ng=3, kpg=2, xs=P, npts=300, logN=LOGN, out=P, stride=48, work=P, wb=1 << 20):
        return L.dpf_eval_bits_grouped_dev(0, keys, kl, ng, kpg, xs, npts, logN, out, stride, work, wb, None)

    assert bits(stride=40) == dpf.DPF_ERR_PARAM and b"bits_stride" in L.dpf_last_error()
    assert bits(stride=32) == dpf.DPF_ERR_PARAM                       # 256 bits for 300 points
    assert bits(logN=64, kl=4096) == dpf.DPF_ERR_PARAM and b"logN > 63" in L.dpf_last_error()
    assert bits(kl=SHORT) == dpf.DPF_ERR_KEYLEN and b"key shorter" in L.dpf_last_error()
    assert bits(ng=1 << 31) == dpf.DPF_ERR_PARAM and b"32 bits" in L.dpf_last_error()
    assert bits(ng=1 << 31, kpg=1, npts=1 << 30, stride=1 << 27) == dpf.DPF_ERR_PARAM
    assert b"64 bits" in L.dpf_last_error()
    for name in ("keys", "xs", "out", "work"):
        assert bits(**{name: None}) == dpf.DPF_ERR_PARAM, name
        assert b"null" in L.dpf_last_error()
    for name in ("out", "work"):
        assert bits(**{name: P + 8}) == dpf.DPF_ERR_PARAM, name
        assert b"misaligned" in L.dpf_last_error()
    assert bits(xs=P + 4) == dpf.DPF_ERR_PARAM and b"misaligned" in L.dpf_last_error()
    assert bits(wb=16) == dpf.DPF_ERR_PARAM and b"workspace" in L.dpf_last_error()
    # The order of reports: stride, logN, key, key rows, null, misaligned, workspace.
    assert bits(stride=40, logN=64) == dpf.DPF_ERR_PARAM and b"bits_stride" in L.dpf_last_error()
    assert bits(logN=64, kl=10) == dpf.DPF_ERR_PARAM and b"logN > 63" in L.dpf_last_error()
    assert bits(kl=SHORT, ng=1 << 31) == dpf.DPF_ERR_KEYLEN
    assert bits(ng=1 << 31, keys=None) == dpf.DPF_ERR_PARAM and b"32 bits" in L.dpf_last_error()
    assert bits(keys=None, out=P + 8) == dpf.DPF_ERR_PARAM and b"null" in L.dpf_last_error()
    assert bits(out=P + 8, wb=16) == dpf.DPF_ERR_PARAM and b"misaligned" in L.dpf_last_error()
    # Nothing to do: DPF_OK without a launch, whatever the pointers; the shape rules still hold.
    assert bits(ng=0) == dpf.DPF_OK and bits(kpg=0) == dpf.DPF_OK and bits(npts=0, stride=0) == dpf.DPF_OK
    assert bits(ng=0, keys=None, xs=None, out=None, work=None, wb=0) == dpf.DPF_OK
    assert bits(ng=0, stride=40) == dpf.DPF_ERR_PARAM
    assert bits(ng=0, kl=10) == dpf.DPF_ERR_KEYLEN


def _order(L, call, nullable, aligned16, aligned4=()):
    """The rules the two composites share, in the documented order."""
    for rec in (0, 6, 32768 + 4):
        assert call(rec=rec) == dpf.DPF_ERR_PARAM, rec
        assert b"rec_bytes" in L.dpf_last_error()
    assert call(logN=64, kl=4096) == dpf.DPF_ERR_PARAM and b"logN > 63" in L.dpf_last_error()
    assert call(kl=SHORT) == dpf.DPF_ERR_KEYLEN and b"key shorter" in L.dpf_last_error()
    assert call(ng=1 << 16, kpg=1 << 16) == dpf.DPF_ERR_PARAM and b"32 bits" in L.dpf_last_error()
    for name in nullable:
        assert call(**{name: None}) == dpf.DPF_ERR_PARAM, name
        assert b"null" in L.dpf_last_error()
    for name in aligned16:
        assert call(**{name: P + 8}) == dpf.DPF_ERR_PARAM, name
        assert b"misaligned" in L.dpf_last_error()
    for name in aligned4:
        assert call(**{name: P + 2}) == dpf.DPF_ERR_PARAM, name
        assert b"misaligned" in L.dpf_last_error()
    assert call(points=P + 4) == dpf.DPF_ERR_PARAM and b"misaligned" in L.dpf_last_error()
    # 1 before 2 before 3 before 4 before 5 before 6.
    assert call(rec=6, logN=64) == dpf.DPF_ERR_PARAM and b"rec_bytes" in L.dpf_last_error()
    assert call(logN=64, kl=10) == dpf.DPF_ERR_PARAM and b"logN > 63" in L.dpf_last_error()
    assert call(kl=SHORT, ng=1 << 31) == dpf.DPF_ERR_KEYLEN
    assert call(ng=1 << 31, keys=None) == dpf.DPF_ERR_PARAM and b"32 bits" in L.dpf_last_error()
    assert call(keys=None, dbs=P + 8) == dpf.DPF_ERR_PARAM and b"null" in L.dpf_last_error()
    assert call(points=None, work=P + 8) == dpf.DPF_ERR_PARAM and b"null" in L.dpf_last_error()
    assert call(ng=0, kl=10) == dpf.DPF_ERR_KEYLEN              # the shape rules hold for an empty call too
    assert call(ng=0, rec=6) == dpf.DPF_ERR_PARAM


def test_grouped_sparse_answer_validates_before_touching_a_device():
    L = dpf.lib()

    def answer(keys=P, kl=KL, ng=3, kpg=2, logN=LOGN, points=P, dbs=P, nrec=300, rec=20, ans=P, work=P):
        return L.dpf_pir_answer_grouped_sparse_dev(0, keys, kl, ng, kpg, logN, points, dbs, nrec, rec, ans, work, None)

    _order(L, answer, ("keys", "points", "dbs", "ans", "work"), ("dbs", "work"), ("ans",))
    # nrec > 2^logN is not an error: the call gets as far as the null-buffer rule.
    kl7 = 33
    assert answer(logN=7, kl=kl7, nrec=129, ans=None) == dpf.DPF_ERR_PARAM and b"null" in L.dpf_last_error()
    assert answer(logN=7, kl=kl7, nrec=1 << 20, points=None) == dpf.DPF_ERR_PARAM and b"null" in L.dpf_last_error()
    # Buffers the call has no work for may be null.
    assert answer(ng=0) == dpf.DPF_OK and answer(kpg=0) == dpf.DPF_OK
    assert answer(ng=0, keys=None, points=None, dbs=None, ans=None, work=None) == dpf.DPF_OK
    assert answer(kpg=0, keys=None, points=None, dbs=None, ans=None, work=None) == dpf.DPF_OK
    assert answer(nrec=0, points=None, dbs=None, ans=None) == dpf.DPF_ERR_PARAM      # the answers are still zeroed


def test_grouped_sparse_write_validates_before_touching_a_device():
    L = dpf.lib()

    def write(keys=P, kl=KL, ng=3, kpg=2, logN=LOGN, points=P, msgs=P, dbs=P, nrec=300, rec=20, work=P):
        return L.dpf_pir_write_grouped_sparse_dev(0, keys, kl, ng, kpg, logN, points, msgs, dbs, nrec, rec, work, None)

    _order(L, write, ("keys", "points", "msgs", "dbs", "work"), ("msgs", "dbs", "work"))
    assert write(logN=7, kl=33, nrec=129, msgs=None) == dpf.DPF_ERR_PARAM and b"null" in L.dpf_last_error()
    # Nothing to do: DPF_OK without a launch.
    assert write(ng=0) == dpf.DPF_OK and write(kpg=0) == dpf.DPF_OK and write(nrec=0) == dpf.DPF_OK
    # ... but, as for the other scatters, every buffer must be given.
    assert write(ng=0, msgs=None) == dpf.DPF_ERR_PARAM and b"null" in L.dpf_last_error()


def test_grouped_sparse_handle_validates_before_opening_a_device():
    L = dpf.lib()
    h = ctypes.c_void_p(1)
    db = (ctypes.c_uint8 * 128)()
    u8 = ctypes.cast(db, ctypes.POINTER(ctypes.c_uint8))
    pts = (ctypes.c_uint64 * 4)(1, 2, 3, 4)
    u64 = ctypes.cast(pts, ctypes.POINTER(ctypes.c_uint64))
    create = L.dpf_pir_db_create_grouped_sparse
    assert create(u64, u8, 2, 2, 32, 10, 1, None) == dpf.DPF_ERR_PARAM                     # null handle pointer
    assert create(u64, u8, 2, 2, 0, 10, 1, ctypes.byref(h)) == dpf.DPF_ERR_PARAM           # bad widths
    assert h.value is None
    assert create(u64, u8, 2, 2, 32768 + 1, 10, 1, ctypes.byref(h)) == dpf.DPF_ERR_PARAM
    h = ctypes.c_void_p(1)
    assert create(u64, u8, 2, 2, 32, 64, 1, ctypes.byref(h)) == dpf.DPF_ERR_PARAM          # logN = 64
    assert h.value is None
    assert create(u64, u8, 1 << 40, 1 << 30, 32, 40, 1, ctypes.byref(h)) == dpf.DPF_ERR_PARAM   # the product overflows
    assert create(None, u8, 2, 2, 32, 10, 1, ctypes.byref(h)) == dpf.DPF_ERR_PARAM
    assert b"null" in L.dpf_last_error()
    assert create(u64, None, 2, 2, 32, 10, 1, ctypes.byref(h)) == dpf.DPF_ERR_PARAM
    assert b"null" in L.dpf_last_error()
    for bad in (1 << 10, 1 << 63):
        h = ctypes.c_void_p(1)
        pts[3] = bad
        assert create(u64, u8, 2, 2, 32, 10, 1, ctypes.byref(h)) == dpf.DPF_ERR_PARAM       # a point outside 2^10
        assert b"outside" in L.dpf_last_error() and h.value is None
