"""Size functions and argument checks of the Eval-bits and sparse-PIR entry
points (include/dpf_hip.h).  No device is needed: the sizes are arithmetic,
and every DPF_ERR_PARAM / DPF_ERR_KEYLEN case returns before any device call
(with no device a call that got that far would return DPF_ERR_HIP or fault on
the fake pointers, which are never dereferenced)."""
import ctypes

import dpf

P = 1 << 20      # an aligned fake device address
LOGN = 40
KL = 33 + 18 * (LOGN - 7)


def test_eval_bits_sizes():
    assert dpf.eval_bits_stride(0) == 0
    assert all(dpf.eval_bits_stride(n) == 16 for n in range(1, 129))
    assert dpf.eval_bits_stride(129) == 32
    assert dpf.eval_bits_stride(256) == 32 and dpf.eval_bits_stride(257) == 48
    assert dpf.eval_bits_stride((1 << 20) + 1) == (1 << 17) + 16
    for nk, npts, logN in ((1, 1, 7), (3, 300, 20), (64, 1 << 22, 40), (16, 1 << 20, 63), (5, 1000, 70)):
        assert dpf.eval_bits_workspace_size(nk, npts, logN) == dpf.eval_workspace_size(nk, npts, logN)
    # Expanded keys and the frontier only: nothing that grows as nkeys * npts.
    nk, npts = 64, 1 << 22
    ws = dpf.eval_bits_workspace_size(nk, npts, LOGN)
    assert 3 * ws < nk * npts                                       # 68 MiB, against 2 GiB of tiled points
    assert ws == dpf.eval_bits_workspace_size(nk, npts * 4, LOGN)   # the frontier is capped at level 16


def test_sparse_workspace_is_the_sum_of_its_three_parts():
    r16 = lambda x: (x + 15) // 16 * 16
    for nk, nrec, logN in ((1, 1, 30), (5, 1000, 63), (64, 1 << 22, 40), (65, 257, 30)):
        want = (r16(dpf.eval_bits_workspace_size(nk, nrec, logN)) + r16(nk * dpf.eval_bits_stride(nrec)) +
                r16(dpf.xor_fold_workspace_size()))
        assert dpf.pir_sparse_workspace_size(nk, nrec, logN) == want


def test_eval_bits_validates_before_touching_a_device():
    L = dpf.lib()
    ws = dpf.eval_bits_workspace_size(2, 300, LOGN)
    ok = dict(keys=P, kl=KL, nk=2, xs=P, npts=300, bits=P, stride=48, work=P, wb=ws)

    def call(**kw):
        a = dict(ok, **kw)
        return L.dpf_eval_bits_dev(0, a["keys"], a["kl"], a["nk"], a["xs"], a["npts"], LOGN, a["bits"], a["stride"],
                                   a["work"], a["wb"], None)

    assert call(stride=40) == dpf.DPF_ERR_PARAM          # not a multiple of 16
    assert call(stride=32) == dpf.DPF_ERR_PARAM          # below dpf_eval_bits_stride(300) = 48
    assert call(stride=0) == dpf.DPF_ERR_PARAM
    assert call(xs=P + 4) == dpf.DPF_ERR_PARAM           # d_xs not 8-byte aligned
    assert call(bits=P + 8) == dpf.DPF_ERR_PARAM         # d_bits not 16-byte aligned
    assert call(work=P + 8) == dpf.DPF_ERR_PARAM         # d_work not 16-byte aligned
    for name in ("keys", "xs", "bits", "work"):
        assert call(**{name: None}) == dpf.DPF_ERR_PARAM, name
    records = 2 * (LOGN - 7 + 2) * 32
    assert records <= dpf.workspace_size(2, LOGN)
    assert call(wb=records - 1) == dpf.DPF_ERR_PARAM     # does not hold the expanded keys
    assert call(wb=0) == dpf.DPF_ERR_PARAM
    assert call(kl=17 + 18 * (LOGN - 7) - 1) == dpf.DPF_ERR_KEYLEN
    assert b"key shorter" in L.dpf_last_error()
    # Nothing to do: DPF_OK without a launch, whatever the pointers.
    assert call(nk=0) == dpf.DPF_OK
    assert call(npts=0, stride=0, xs=None, bits=None) == dpf.DPF_OK
    # ... but the shape rules hold for an empty call too.
    assert call(nk=0, stride=40) == dpf.DPF_ERR_PARAM


def test_sparse_composites_validate_before_touching_a_device():
    L = dpf.lib()

    def answer(keys=P, kl=KL, nk=2, pts=P, dbs=P, nrec=300, rec=20, ans=P, work=P):
        return L.dpf_pir_answer_sparse_dev(0, keys, kl, nk, LOGN, pts, dbs, nrec, rec, ans, work, None)

    def write(keys=P, kl=KL, nk=2, pts=P, msgs=P, dbs=P, nrec=300, rec=20, work=P):
        return L.dpf_pir_write_sparse_dev(0, keys, kl, nk, LOGN, pts, msgs, dbs, nrec, rec, work, None)

    for f in (answer, write):
        for rec in (0, 6, 32768 + 4):
            assert f(rec=rec) == dpf.DPF_ERR_PARAM, rec
        assert f(kl=100) == dpf.DPF_ERR_KEYLEN
        for name in ("keys", "pts", "dbs", "work"):
            assert f(**{name: None}) == dpf.DPF_ERR_PARAM, name
        assert f(pts=P + 4) == dpf.DPF_ERR_PARAM
        assert f(dbs=P + 8) == dpf.DPF_ERR_PARAM
        assert f(work=P + 8) == dpf.DPF_ERR_PARAM
        assert f(nk=0) == dpf.DPF_OK
    assert answer(ans=None) == dpf.DPF_ERR_PARAM
    assert answer(ans=P + 2) == dpf.DPF_ERR_PARAM
    assert write(msgs=None) == dpf.DPF_ERR_PARAM
    assert write(msgs=P + 8) == dpf.DPF_ERR_PARAM
    assert write(nrec=0) == dpf.DPF_OK


def test_sparse_handle_validates_before_opening_a_device():
    L = dpf.lib()
    h = ctypes.c_void_p(1)
    pts = (ctypes.c_uint64 * 2)(5, 1 << 30)
    db = (ctypes.c_uint8 * 64)()
    cast = lambda a, t: ctypes.cast(a, ctypes.POINTER(t))
    u64, u8 = cast(pts, ctypes.c_uint64), cast(db, ctypes.c_uint8)
    assert L.dpf_pir_db_create_sparse(u64, u8, 2, 32, 30, 1, ctypes.byref(h)) == dpf.DPF_ERR_PARAM   # 2^30 >= 2^logN
    assert h.value is None
    assert L.dpf_pir_db_create_sparse(u64, u8, 2, 32, 64, 1, ctypes.byref(h)) == dpf.DPF_ERR_PARAM   # logN > 63
    assert L.dpf_pir_db_create_sparse(u64, u8, 2, 0, 40, 1, ctypes.byref(h)) == dpf.DPF_ERR_PARAM
    assert L.dpf_pir_db_create_sparse(None, u8, 2, 32, 40, 1, ctypes.byref(h)) == dpf.DPF_ERR_PARAM
    assert L.dpf_pir_db_create_sparse(u64, u8, 2, 32, 40, 1, None) == dpf.DPF_ERR_PARAM
