"""Size functions and argument checks of the grouped PIR entry points
(include/dpf_hip.h).  No device is needed: the sizes are arithmetic, and every
DPF_ERR_PARAM / DPF_ERR_KEYLEN case returns before any device call (with no
device a call that got that far would return DPF_ERR_HIP or fault on the fake
pointers, which are never dereferenced)."""
import ctypes

import dpf

P = 1 << 20      # an aligned fake device address
LOGN = 12
KL = 33 + 18 * (LOGN - 7)


def test_group_stride_and_db_size():
    assert dpf.pir_group_stride(0) == 0
    assert all(dpf.pir_group_stride(n) == 256 for n in range(1, 257))
    assert dpf.pir_group_stride(257) == 512
    assert dpf.pir_db_grouped_size(3, 257, 20) == 3 * 512 * 20
    assert dpf.pir_db_grouped_size(7, 256, 32) == 7 * 256 * 32 == dpf.pir_db_sliced_size_any(7 * 256, 32)
    assert dpf.pir_db_grouped_size(0, 100, 32) == 16 and dpf.pir_db_grouped_size(5, 0, 32) == 16   # the minimum
    for rec in (0, 6, 32768 + 4):
        assert dpf.pir_db_grouped_size(3, 100, rec) == 0, rec
    assert dpf.pir_db_grouped_size(1 << 40, 1 << 30, 4) == 0                                      # overflows
    assert dpf.pir_db_grouped_size(2, (1 << 64) - 1, 4) == 0


def test_workspace_sizes():
    r256 = lambda x: (x + 255) // 256 * 256
    for rec in (0, 6, 32768 + 4):
        assert dpf.xor_fold_grouped_workspace_size(3, 2, rec) == 0, rec
        assert dpf.pir_grouped_workspace_size(3, 2, LOGN, rec) == 0, rec
    assert dpf.xor_fold_grouped_workspace_size(1 << 31, 2, 32) == 0        # 2^32 key rows
    assert dpf.pir_grouped_workspace_size(1 << 31, 2, LOGN, 32) == 0
    # The composite's workspace is the sum of the parts of its layout.
    for ng, kpg, logN, rec in ((1, 1, 7, 4), (3, 5, 13, 20), (384, 1, 19, 32), (65, 2, 10, 100), (100000, 1, 8, 32)):
        nk = ng * kpg
        fold = dpf.xor_fold_grouped_workspace_size(ng, kpg, rec)
        assert fold >= 16 and fold % 16 == 0
        want = r256(dpf.workspace_size(nk, logN)) + r256(nk * dpf.evalfull_len(logN)) + fold
        assert dpf.pir_grouped_workspace_size(ng, kpg, logN, rec) == want
        assert dpf.pir_grouped_workspace_size(1, nk, logN, rec) == want    # a function of the key rows only


def test_grouped_fold_validates_before_touching_a_device():
    L = dpf.lib()

    def fold(bits=P, stride=48, ng=3, kpg=2, dbs=P, nrec=300, rec=20, ans=P, work=P):
        return L.dpf_xor_fold_grouped_dev(0, bits, stride, ng, kpg, dbs, nrec, rec, ans, work, None)

    for rec in (0, 6, 32768 + 4):
        assert fold(rec=rec) == dpf.DPF_ERR_PARAM, rec
    assert b"rec_bytes" in L.dpf_last_error()
    assert fold(stride=40) == dpf.DPF_ERR_PARAM             # not a multiple of 16
    assert fold(stride=32) == dpf.DPF_ERR_PARAM             # 256 bits for 300 records
    assert fold(nrec=385) == dpf.DPF_ERR_PARAM              # the rule is against nrec, not the stride of a group
    assert fold(ng=1 << 31, kpg=2) == dpf.DPF_ERR_PARAM     # 2^32 key rows
    assert b"32 bits" in L.dpf_last_error()
    assert fold(ng=(1 << 32) - 1, kpg=1, ans=None) == dpf.DPF_ERR_PARAM    # fits: the next rule reports
    assert b"null" in L.dpf_last_error()
    for name in ("bits", "dbs", "ans", "work"):
        assert fold(**{name: None}) == dpf.DPF_ERR_PARAM, name
        assert b"null" in L.dpf_last_error()
    for name in ("bits", "dbs", "work"):
        assert fold(**{name: P + 8}) == dpf.DPF_ERR_PARAM, name
        assert b"misaligned" in L.dpf_last_error()
    assert fold(ans=P + 2) == dpf.DPF_ERR_PARAM
    # The order of reports: the width before the stride, null before misaligned.
    assert fold(rec=6, stride=40) == dpf.DPF_ERR_PARAM and b"rec_bytes" in L.dpf_last_error()
    assert fold(bits=None, dbs=P + 8) == dpf.DPF_ERR_PARAM and b"null" in L.dpf_last_error()
    # Nothing to do: DPF_OK without a launch, whatever the pointers.
    assert fold(ng=0) == dpf.DPF_OK
    assert fold(kpg=0) == dpf.DPF_OK
    assert fold(ng=0, bits=None, dbs=None, ans=None, work=None) == dpf.DPF_OK
    # ... but the shape rules hold for an empty call too.
    assert fold(ng=0, stride=40) == dpf.DPF_ERR_PARAM


def test_grouped_answer_validates_before_touching_a_device():
    L = dpf.lib()

    def answer(keys=P, kl=KL, ng=3, kpg=2, logN=LOGN, dbs=P, nrec=300, rec=20, ans=P, work=P):
        return L.dpf_pir_answer_grouped_dev(0, keys, kl, ng, kpg, logN, dbs, nrec, rec, ans, work, None)

    for rec in (0, 6, 32768 + 4):
        assert answer(rec=rec) == dpf.DPF_ERR_PARAM, rec
    assert answer(logN=64, kl=4096) == dpf.DPF_ERR_PARAM
    assert b"logN > 63" in L.dpf_last_error()
    assert answer(kl=17 + 18 * (LOGN - 7) - 1) == dpf.DPF_ERR_KEYLEN
    assert b"key shorter" in L.dpf_last_error()
    assert answer(nrec=(1 << LOGN) + 1) == dpf.DPF_ERR_PARAM
    assert b"domain" in L.dpf_last_error()
    assert answer(nrec=1 << LOGN, ans=None) == dpf.DPF_ERR_PARAM and b"null" in L.dpf_last_error()
    assert answer(ng=1 << 16, kpg=1 << 16) == dpf.DPF_ERR_PARAM
    assert b"32 bits" in L.dpf_last_error()
    for name in ("keys", "dbs", "ans", "work"):
        assert answer(**{name: None}) == dpf.DPF_ERR_PARAM, name
        assert b"null" in L.dpf_last_error()
    for name in ("dbs", "work"):
        assert answer(**{name: P + 8}) == dpf.DPF_ERR_PARAM, name
        assert b"misaligned" in L.dpf_last_error()
    assert answer(ans=P + 2) == dpf.DPF_ERR_PARAM
    # The order of reports: width, key, nrec, key rows, null, misaligned.
    assert answer(rec=6, kl=10) == dpf.DPF_ERR_PARAM
    assert answer(kl=10, nrec=1 << 20) == dpf.DPF_ERR_KEYLEN
    assert answer(nrec=1 << 20, ng=1 << 31) == dpf.DPF_ERR_PARAM and b"domain" in L.dpf_last_error()
    assert answer(ng=1 << 31, keys=None) == dpf.DPF_ERR_PARAM and b"32 bits" in L.dpf_last_error()
    assert answer(keys=None, dbs=P + 8) == dpf.DPF_ERR_PARAM and b"null" in L.dpf_last_error()
    assert answer(ng=0) == dpf.DPF_OK
    assert answer(kpg=0) == dpf.DPF_OK
    assert answer(ng=0, keys=None, dbs=None, ans=None, work=None) == dpf.DPF_OK
    assert answer(ng=0, kl=10) == dpf.DPF_ERR_KEYLEN


def test_grouped_slice_validates_before_touching_a_device():
    L = dpf.lib()

    def slice_(db=P, ng=3, nrec=300, rec=20, dbs=P):
        return L.dpf_pir_db_slice_grouped_dev(0, db, ng, nrec, rec, dbs, None)

    for rec in (0, 6, 32768 + 4):
        assert slice_(rec=rec) == dpf.DPF_ERR_PARAM, rec
    assert slice_(ng=1 << 40, nrec=1 << 30) == dpf.DPF_ERR_PARAM
    assert slice_(db=None) == dpf.DPF_ERR_PARAM and slice_(dbs=None) == dpf.DPF_ERR_PARAM
    assert slice_(db=P + 8) == dpf.DPF_ERR_PARAM and slice_(dbs=P + 8) == dpf.DPF_ERR_PARAM
    assert slice_(ng=0) == dpf.DPF_OK and slice_(nrec=0, db=None, dbs=None) == dpf.DPF_OK


def test_grouped_handle_validates_before_opening_a_device():
    L = dpf.lib()
    h = ctypes.c_void_p(1)
    db = (ctypes.c_uint8 * 64)()
    u8 = ctypes.cast(db, ctypes.POINTER(ctypes.c_uint8))
    create = L.dpf_pir_db_create_grouped
    assert create(u8, 2, 1, 32, 10, 1, None) == dpf.DPF_ERR_PARAM                      # null handle pointer
    assert create(u8, 2, 1, 0, 10, 1, ctypes.byref(h)) == dpf.DPF_ERR_PARAM            # bad widths
    assert h.value is None
    assert create(u8, 2, 1, 32768 + 1, 10, 1, ctypes.byref(h)) == dpf.DPF_ERR_PARAM
    assert create(u8, 2, 1, 32, 64, 1, ctypes.byref(h)) == dpf.DPF_ERR_PARAM           # logN > 63
    assert create(u8, 2, 1025, 32, 10, 1, ctypes.byref(h)) == dpf.DPF_ERR_PARAM        # a group larger than 2^logN
    assert b"2^logN" in L.dpf_last_error()
    assert create(u8, 1 << 40, 1 << 30, 32, 40, 1, ctypes.byref(h)) == dpf.DPF_ERR_PARAM   # the product overflows
    assert create(None, 2, 1, 32, 10, 1, ctypes.byref(h)) == dpf.DPF_ERR_PARAM
    assert L.dpf_pir_db_ngroups(None) == 0
