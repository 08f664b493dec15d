"""Argument checks of the any-width (rec_bytes a multiple of 4) sliced entry
points, without a device: validation precedes any device call, so the fake
aligned addresses are never dereferenced (as tests/test_fold_wide_cpu.py)."""
import ctypes

import pytest

import dpf

P = 4096   # aligned fake device address, never used
MAX_REC = 32768   # DPF_PIR_MAX_REC_BYTES (include/dpf_hip.h)
BAD = (0, 2, 6, 33, 32772)
E_ANY = "dpf: rec_bytes must be a positive multiple of 4, at most DPF_PIR_MAX_REC_BYTES"
E_ALIGN = "dpf: misaligned device buffer"
E_NULL = "dpf: null device buffer"


def _err():
    return dpf.lib().dpf_last_error().decode()


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 4000])
def test_sliced_size_any(n):
    for rec in (4, 12, 20, 36, 100, 32768):
        assert dpf.pir_db_sliced_size_any(n, rec) == max(16, (n + 255) // 256 * 256 * rec)
    for rec in (32, 64, 96, 1024, 32768):
        assert dpf.pir_db_sliced_size_any(n, rec) == dpf.pir_db_sliced_size_wide(n, rec)
    for rec in BAD:
        assert dpf.pir_db_sliced_size_any(n, rec) == 0


# Every _any device entry as a call with one faulty argument set; a valid call
# is never made (it would reach a device).
def _slice(rec, db=P, dbs=P):
    return dpf.lib().dpf_pir_db_slice_any_dev(0, db, 100, rec, dbs, None)


def _fold(rec, bits=P, stride=16, nrec=128, dbs=P, ans=P, work=P):
    return dpf.lib().dpf_xor_fold_sliced_any_dev(0, bits, stride, 1, dbs, nrec, rec, ans, work, None)


def _pir(rec, keys=P, dbs=P, ans=P, work=P, prefix_bits=0, prefix=0, nrec=100, logN=12, klen=None):
    kl = dpf.key_len(logN) if klen is None else klen
    return dpf.lib().dpf_pir_answer_sliced_any_dev(0, keys, kl, 1, logN, prefix_bits, prefix, dbs, nrec, rec, ans, work,
                                                   None)


def _update(rec, dbs=P, idx=P, recs=P):
    return dpf.lib().dpf_pir_db_update_sliced_any_dev(0, dbs, 100, rec, idx, recs, 1, None)


def _gather(rec, dbs=P, idx=P, out=P):
    return dpf.lib().dpf_pir_db_gather_sliced_any_dev(0, dbs, 100, rec, idx, 1, out, None)


def _scatter(rec, bits=P, stride=16, nrec=128, msgs=P, dbs=P):
    return dpf.lib().dpf_xor_scatter_sliced_any_dev(0, bits, stride, 1, msgs, dbs, nrec, rec, None)


def _write(rec, keys=P, msgs=P, dbs=P, work=P, prefix_bits=0, prefix=0, nrec=100, logN=12, klen=None):
    kl = dpf.key_len(logN) if klen is None else klen
    return dpf.lib().dpf_pir_write_sliced_any_dev(0, keys, kl, 1, logN, prefix_bits, prefix, msgs, dbs, nrec, rec, work,
                                                  None)


@pytest.mark.parametrize("rec", BAD)
def test_any_entries_reject_bad_widths_ahead_of_other_errors(rec):
    bad = dpf.DPF_ERR_PARAM
    calls = [
        lambda: _slice(rec), lambda: _slice(rec, db=None, dbs=P + 8),
        lambda: _fold(rec), lambda: _fold(rec, stride=24, nrec=8), lambda: _fold(rec, bits=None, dbs=P + 8, ans=None),
        lambda: _pir(rec), lambda: _pir(rec, klen=3), lambda: _pir(rec, prefix_bits=2, prefix=4, dbs=None),
        lambda: _update(rec), lambda: _update(rec, dbs=None, idx=P + 4),
        lambda: _gather(rec), lambda: _gather(rec, out=None, idx=P + 4),
        lambda: _scatter(rec), lambda: _scatter(rec, stride=24, nrec=8, msgs=None),
        lambda: _write(rec), lambda: _write(rec, klen=3, keys=None, prefix_bits=9),
    ]
    for c in calls:
        assert c() == bad
        assert _err() == E_ANY


@pytest.mark.parametrize("rec", [4, 20, 48])
def test_any_entries_pass_the_width_check_then_check_buffers_as_wide(rec):
    bad = dpf.DPF_ERR_PARAM
    rows = [
        (lambda: _slice(rec, db=P + 8), E_ALIGN), (lambda: _slice(rec, dbs=P + 8), E_ALIGN),
        (lambda: _slice(rec, db=None), E_NULL), (lambda: _slice(rec, dbs=None), E_NULL),
        (lambda: _fold(rec, bits=P + 4), E_ALIGN), (lambda: _fold(rec, dbs=P + 8), E_ALIGN),
        (lambda: _fold(rec, ans=P + 2), E_ALIGN), (lambda: _fold(rec, bits=None), E_NULL),
        (lambda: _fold(rec, dbs=None), E_NULL), (lambda: _fold(rec, ans=None), E_NULL),
        (lambda: _fold(rec, work=None), E_NULL),
        (lambda: _fold(rec, stride=24, nrec=8), "dpf: bits_stride must be a multiple of 16"),
        (lambda: _fold(rec, nrec=129), "dpf: more records than selection bits per key"),
        (lambda: _pir(rec, dbs=P + 8), E_ALIGN), (lambda: _pir(rec, ans=P + 2), E_ALIGN),
        (lambda: _pir(rec, dbs=None), E_NULL), (lambda: _pir(rec, ans=None), E_NULL),
        (lambda: _pir(rec, prefix_bits=2, prefix=4), "dpf: subtree prefix out of range"),
        (lambda: _pir(rec, prefix_bits=2, prefix=3, nrec=1025), "dpf: more DB records than the subtree's domain"),
        (lambda: _update(rec, dbs=P + 8), E_ALIGN), (lambda: _update(rec, recs=P + 4), E_ALIGN),
        (lambda: _update(rec, idx=P + 4), E_ALIGN), (lambda: _update(rec, recs=None), E_NULL),
        (lambda: _gather(rec, dbs=P + 8), E_ALIGN), (lambda: _gather(rec, out=P + 4), E_ALIGN),
        (lambda: _gather(rec, idx=None), E_NULL),
        (lambda: _scatter(rec, bits=P + 8), E_ALIGN), (lambda: _scatter(rec, msgs=P + 4), E_ALIGN),
        (lambda: _scatter(rec, dbs=None), E_NULL),
        (lambda: _scatter(rec, stride=24, nrec=8), "dpf: bits_stride must be a multiple of 16"),
        (lambda: _write(rec, msgs=P + 4), E_ALIGN), (lambda: _write(rec, dbs=P + 8), E_ALIGN),
        (lambda: _write(rec, work=P + 8), E_ALIGN), (lambda: _write(rec, keys=None), E_NULL),
        (lambda: _write(rec, prefix_bits=9), "dpf: subtree prefix out of range"),
    ]
    for c, text in rows:
        assert c() == bad
        assert _err() == text
    # the work buffer's alignment: only above 32 bytes, as for _wide
    assert (_fold(rec, work=P + 8, bits=None) == bad) and _err() == (E_ALIGN if rec > 32 else E_NULL)


@pytest.mark.parametrize("rec", [0, 32769])
def test_create_any_rejects_bad_widths_and_clears_the_handle(rec):
    h = ctypes.c_void_p(1234)
    db = (ctypes.c_uint8 * 96)()
    assert dpf.lib().dpf_pir_db_create_any(db, 2, rec, 12, 1, ctypes.byref(h)) == dpf.DPF_ERR_PARAM
    assert not h.value


def test_wide_entries_still_reject_48():
    L = dpf.lib()
    bad = dpf.DPF_ERR_PARAM
    assert L.dpf_pir_db_sliced_size_wide(100, 48) == 0
    assert L.dpf_pir_db_slice_wide_dev(0, P, 100, 48, P, None) == bad
    assert L.dpf_xor_fold_sliced_wide_dev(0, P, 16, 1, P, 128, 48, P, P, None) == bad
    kl = dpf.key_len(12)
    assert L.dpf_pir_answer_sliced_wide_dev(0, P, kl, 1, 12, 0, 0, P, 100, 48, P, P, None) == bad
    assert L.dpf_pir_db_update_sliced_wide_dev(0, P, 100, 48, P, P, 1, None) == bad
    assert L.dpf_pir_db_gather_sliced_wide_dev(0, P, 100, 48, P, 1, P, None) == bad
    assert L.dpf_xor_scatter_sliced_wide_dev(0, P, 16, 1, P, P, 128, 48, None) == bad
    assert L.dpf_pir_write_sliced_wide_dev(0, P, kl, 1, 12, 0, 0, P, P, 100, 48, P, None) == bad
    h = ctypes.c_void_p(1234)
    db = (ctypes.c_uint8 * 96)()
    assert L.dpf_pir_db_create_wide(db, 2, 48, 12, 1, ctypes.byref(h)) == bad
    assert not h.value
