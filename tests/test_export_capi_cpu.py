"""The whole-DB read-out (dpf_pir_db_unslice_any_dev, _unslice_grouped_dev,
dpf_pir_db_xor_sliced_dev, dpf_pir_db_export, _xor_records, _clear,
dpf_set_export_limits), the parts that need no device: the header declares the
entries, the library exports them and the Python table has them; every
argument check returns before any device call (with no device a call that got
that far would return DPF_ERR_HIP or fault on the fake pointers, which are
never dereferenced), in the order the header states; nothing-to-do calls are
DPF_OK; a null handle is refused."""
import ctypes
import os
import re

import numpy as np
import pytest

import dpf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 20      # an aligned fake device address
ENTRIES = ("dpf_pir_db_unslice_any_dev", "dpf_pir_db_unslice_grouped_dev", "dpf_pir_db_xor_sliced_dev",
           "dpf_pir_db_export", "dpf_pir_db_xor_records", "dpf_pir_db_clear", "dpf_set_export_limits")


def _unslice(dbs=P, nrec=300, rec=20, db=P):
    return dpf.lib().dpf_pir_db_unslice_any_dev(0, dbs, nrec, rec, db, None)


def _unslice_g(dbs=P, ng=3, nrec=300, rec=20, db=P):
    return dpf.lib().dpf_pir_db_unslice_grouped_dev(0, dbs, ng, nrec, rec, db, None)


def _xor(dbs=P, other=P, nbytes=4096):
    return dpf.lib().dpf_pir_db_xor_sliced_dev(0, dbs, other, nbytes, None)


def test_header_declares_and_library_exports_the_entry_points():
    with open(os.path.join(ROOT, "include", "dpf_hip.h")) as f:
        header = f.read()
    for name in ENTRIES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in dpf.SIGNATURES
        assert getattr(dpf.lib(), name) is not None
    assert "offsetting both pointers" in header


def test_unslice_validates_before_touching_a_device():
    L = dpf.lib()
    for call in (_unslice, _unslice_g):
        for rec in (0, 6, 32768 + 4):
            assert call(rec=rec) == dpf.DPF_ERR_PARAM, rec
            assert b"rec_bytes" in L.dpf_last_error()
            assert call(rec=rec, nrec=0) == dpf.DPF_ERR_PARAM      # also with nothing to do
        assert call(nrec=(1 << 64) - 100) == dpf.DPF_ERR_PARAM      # nrec rounded up to 256 overflows
        assert b"too large" in L.dpf_last_error()
        assert call(nrec=1 << 60, rec=32) == dpf.DPF_ERR_PARAM      # the byte count overflows
        assert b"too large" in L.dpf_last_error()
        for name in ("dbs", "db"):
            assert call(**{name: None}) == dpf.DPF_ERR_PARAM, name
            assert b"null" in L.dpf_last_error()
            assert call(**{name: P + 8}) == dpf.DPF_ERR_PARAM, name
            assert b"misaligned" in L.dpf_last_error()
        # The order of reports: width, products, null, misaligned.
        assert call(rec=6, nrec=1 << 62) == dpf.DPF_ERR_PARAM and b"rec_bytes" in L.dpf_last_error()
        assert call(nrec=1 << 62, dbs=None) == dpf.DPF_ERR_PARAM and b"too large" in L.dpf_last_error()
        assert call(dbs=None, db=P + 8) == dpf.DPF_ERR_PARAM and b"null" in L.dpf_last_error()
        # Nothing to do: DPF_OK without a launch (there is no device here), null buffers included.
        assert call(nrec=0) == dpf.DPF_OK
        assert call(nrec=0, dbs=None, db=None) == dpf.DPF_OK
        assert call(nrec=0, db=P + 4) == dpf.DPF_ERR_PARAM         # ... but alignment holds for an empty call
    assert _unslice_g(ng=1 << 40, nrec=1 << 30) == dpf.DPF_ERR_PARAM and b"too large" in L.dpf_last_error()
    assert _unslice_g(ng=0) == dpf.DPF_OK
    assert _unslice_g(ng=0, dbs=None, db=None) == dpf.DPF_OK


def test_xor_sliced_validates_before_touching_a_device():
    L = dpf.lib()
    for nbytes in (8, 4100, 17):
        assert _xor(nbytes=nbytes) == dpf.DPF_ERR_PARAM
        assert b"multiple of 16" in L.dpf_last_error()
    for name in ("dbs", "other"):
        assert _xor(**{name: None}) == dpf.DPF_ERR_PARAM, name
        assert b"null" in L.dpf_last_error()
        assert _xor(**{name: P + 8}) == dpf.DPF_ERR_PARAM, name
        assert b"misaligned" in L.dpf_last_error()
    assert _xor(nbytes=8, dbs=None) == dpf.DPF_ERR_PARAM and b"multiple of 16" in L.dpf_last_error()
    assert _xor(dbs=None, other=P + 8) == dpf.DPF_ERR_PARAM and b"null" in L.dpf_last_error()
    assert _xor(nbytes=0) == dpf.DPF_OK
    assert _xor(nbytes=0, dbs=None, other=None) == dpf.DPF_OK


def test_handle_entries_reject_a_null_handle():
    buf = (ctypes.c_uint8 * 256)()
    L = dpf.lib()
    for n in (1, 0):
        assert L.dpf_pir_db_export(None, 0, n, buf) == dpf.DPF_ERR_PARAM
        assert b"null PIR handle" in L.dpf_last_error()
        assert L.dpf_pir_db_xor_records(None, 0, n, buf) == dpf.DPF_ERR_PARAM
        assert b"null PIR handle" in L.dpf_last_error()
    assert L.dpf_pir_db_clear(None) == dpf.DPF_ERR_PARAM
    assert b"null PIR handle" in L.dpf_last_error()


def test_export_limits_and_python_wrappers():
    assert dpf.lib().dpf_set_export_limits(8192) == dpf.DPF_OK
    assert dpf.lib().dpf_set_export_limits(0) == dpf.DPF_OK
    for name in ("pir_db_unslice_any_dev", "pir_db_unslice_grouped_dev", "pir_db_xor_sliced_dev", "set_export_limits"):
        assert callable(getattr(dpf, name))
    for name in ("export", "xor_records", "clear"):
        assert callable(getattr(dpf.PirDB, name))
    # Shape errors are ValueError before the C call (no handle is needed to get there).
    db = dpf.PirDB.__new__(dpf.PirDB)
    db.rec_bytes, db._h = 20, ctypes.c_void_p()
    with pytest.raises(ValueError):
        db.xor_records(np.zeros(30, np.uint8))
    with pytest.raises(ValueError):
        db.xor_records(np.zeros(40, np.uint8), first=-1)
    with pytest.raises(ValueError):
        db.export(first=-1)
    with pytest.raises(ValueError):
        db.export(0, -2)
