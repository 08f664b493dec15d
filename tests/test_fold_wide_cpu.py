"""Argument checks of the wide-record (rec_bytes = 32*C) sliced fold and PIR
entry points, without a device: validation precedes any device call, so fake
aligned addresses are never dereferenced (as
test_capi.py::test_xor_fold_validates_before_touching_a_device)."""
import ctypes

import pytest

import dpf

P = 4096   # aligned fake device address, never used


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 4000])
def test_sliced_size_wide(n):
    assert dpf.pir_db_sliced_size_wide(n, 32) == dpf.pir_db_sliced_size(n)
    for rec in (64, 96, 1024):
        assert dpf.pir_db_sliced_size_wide(n, rec) == max(16, (n + 255) // 256 * 256 * rec)


def _fold(bits=P, stride=16, nrec=128, rec=64, dbs=P, ans=P):
    return dpf.lib().dpf_xor_fold_sliced_wide_dev(0, bits, stride, 1, dbs, nrec, rec, ans, P, None)


def _pir(f, rec=64, dbs=P, ans=P, prefix_bits=0, prefix=0, nrec=100, logN=12):
    return getattr(dpf.lib(), f)(0, P, dpf.key_len(logN), 1, logN, prefix_bits, prefix, dbs, nrec, rec, ans, P, None)


PIR = ("dpf_pir_answer_sliced_wide_dev", "dpf_pir_answer_wide_dev")


@pytest.mark.parametrize("rec", [0, 48, 33])
def test_wide_entries_reject_bad_rec_bytes(rec):
    assert _fold(rec=rec) == dpf.DPF_ERR_PARAM
    for f in PIR:
        assert _pir(f, rec=rec) == dpf.DPF_ERR_PARAM
    assert dpf.lib().dpf_pir_db_slice_wide_dev(0, P, 100, rec, P, None) == dpf.DPF_ERR_PARAM


@pytest.mark.parametrize("rec", [32, 64, 1024])
def test_wide_fold_rejects_bad_shapes(rec):
    assert _fold(rec=rec, bits=P + 4) == dpf.DPF_ERR_PARAM      # misaligned d_bits
    assert _fold(rec=rec, dbs=P + 8) == dpf.DPF_ERR_PARAM       # misaligned d_dbs
    assert _fold(rec=rec, ans=P + 2) == dpf.DPF_ERR_PARAM       # misaligned d_ans
    assert _fold(rec=rec, stride=24, nrec=8) == dpf.DPF_ERR_PARAM    # bits_stride % 16
    assert _fold(rec=rec, stride=16, nrec=129) == dpf.DPF_ERR_PARAM  # nrec > 8 * bits_stride


@pytest.mark.parametrize("rec", [32, 64, 1024])
@pytest.mark.parametrize("f", PIR)
def test_wide_pir_rejects_bad_shapes(f, rec):
    assert _pir(f, rec=rec, dbs=P + 8) == dpf.DPF_ERR_PARAM     # misaligned DB
    assert _pir(f, rec=rec, ans=P + 2) == dpf.DPF_ERR_PARAM     # misaligned d_ans
    assert _pir(f, rec=rec, prefix_bits=2, prefix=4) == dpf.DPF_ERR_PARAM    # prefix >= 2^prefix_bits
    assert _pir(f, rec=rec, prefix_bits=9) == dpf.DPF_ERR_PARAM              # prefix_bits > logN - 7
    assert _pir(f, rec=rec, prefix_bits=2, prefix=3, nrec=1025) == dpf.DPF_ERR_PARAM   # more than the subtree


def test_create_wide_rejects_bad_rec_bytes_and_clears_the_handle():
    h = ctypes.c_void_p(1234)
    db = (ctypes.c_uint8 * 96)()
    rc = dpf.lib().dpf_pir_db_create_wide(db, 2, 48, 12, 1, ctypes.byref(h))
    assert rc == dpf.DPF_ERR_PARAM
    assert not h.value
    assert dpf.lib().dpf_pir_db_rec_bytes(None) == 0
