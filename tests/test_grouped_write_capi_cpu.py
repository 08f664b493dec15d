"""Grouped private writes (dpf_xor_scatter_grouped_dev,
dpf_pir_write_grouped_dev, dpf_pir_db_write_grouped), the parts that need no
device: the header declares the entries, the library exports them and the
Python table has them; every argument check returns before any device call
(with no device a call that got that far would return DPF_ERR_HIP or fault on
the fake pointers, which are never dereferenced), in the order the header
states; nothing-to-do calls are DPF_OK; and the form query is arithmetic."""
import ctypes
import os
import re

import dpf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 20      # an aligned fake device address
LOGN = 12
KL = 33 + 18 * (LOGN - 7)
ENTRIES = ("dpf_xor_scatter_grouped_dev", "dpf_pir_write_grouped_dev", "dpf_pir_db_write_grouped")


def _scatter(bits=P, stride=48, ng=3, kpg=2, msgs=P, dbs=P, nrec=300, rec=20):
    return dpf.lib().dpf_xor_scatter_grouped_dev(0, bits, stride, ng, kpg, msgs, dbs, nrec, rec, None)


def _write(keys=P, kl=KL, ng=3, kpg=2, logN=LOGN, msgs=P, dbs=P, nrec=300, rec=20, work=P):
    return dpf.lib().dpf_pir_write_grouped_dev(0, keys, kl, ng, kpg, logN, msgs, dbs, nrec, rec, work, None)


def test_header_declares_and_library_exports_the_entry_points():
    with open(os.path.join(ROOT, "include", "dpf_hip.h")) as f:
        header = f.read()
    for name in ENTRIES + ("dpf_scatter_grouped_form_for",):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in dpf.SIGNATURES
        assert getattr(dpf.lib(), name) is not None
    # The dense write still refuses a grouped handle, and now says where to go.
    assert "dpf_pir_db_write on a grouped handle is DPF_ERR_PARAM" in header
    assert "a grouped private\n * write is not built" not in header


def test_grouped_scatter_validates_before_touching_a_device():
    L = dpf.lib()
    for rec in (0, 6, 32768 + 4):
        assert _scatter(rec=rec) == dpf.DPF_ERR_PARAM, rec
        assert _scatter(rec=rec, ng=0) == dpf.DPF_ERR_PARAM        # also with nothing to do
    assert b"rec_bytes" in L.dpf_last_error()
    assert _scatter(stride=40) == dpf.DPF_ERR_PARAM                # not a multiple of 16
    assert b"multiple of 16" in L.dpf_last_error()
    assert _scatter(stride=32) == dpf.DPF_ERR_PARAM                # 256 bits for 300 records
    assert _scatter(nrec=385) == dpf.DPF_ERR_PARAM                 # the rule is against nrec, not the group's stride
    assert b"selection bits" in L.dpf_last_error()
    assert _scatter(ng=1 << 31, kpg=2) == dpf.DPF_ERR_PARAM        # 2^32 key rows
    assert b"32 bits" in L.dpf_last_error()
    assert _scatter(ng=(1 << 32) - 1, kpg=1, msgs=None) == dpf.DPF_ERR_PARAM    # fits: the next rule reports
    assert b"null" in L.dpf_last_error()
    for name in ("bits", "msgs", "dbs"):
        assert _scatter(**{name: None}) == dpf.DPF_ERR_PARAM, name
        assert b"null" in L.dpf_last_error()
        assert _scatter(**{name: None, "ng": 0}) == dpf.DPF_ERR_PARAM, name     # every buffer, as the other scatters
        assert _scatter(**{name: P + 8}) == dpf.DPF_ERR_PARAM, name
        assert b"misaligned" in L.dpf_last_error()
    # The order of reports: width, stride, key rows, null, misaligned.
    assert _scatter(rec=6, stride=40) == dpf.DPF_ERR_PARAM and b"rec_bytes" in L.dpf_last_error()
    assert _scatter(stride=40, ng=1 << 31) == dpf.DPF_ERR_PARAM and b"multiple of 16" in L.dpf_last_error()
    assert _scatter(ng=1 << 31, bits=None) == dpf.DPF_ERR_PARAM and b"32 bits" in L.dpf_last_error()
    assert _scatter(bits=None, dbs=P + 8) == dpf.DPF_ERR_PARAM and b"null" in L.dpf_last_error()
    # Nothing to do: DPF_OK without a launch (there is no device here).
    assert _scatter(ng=0) == dpf.DPF_OK
    assert _scatter(kpg=0) == dpf.DPF_OK
    assert _scatter(nrec=0) == dpf.DPF_OK
    # ... but the shape rules hold for an empty call too.
    assert _scatter(ng=0, stride=40) == dpf.DPF_ERR_PARAM


def test_grouped_write_validates_before_touching_a_device():
    L = dpf.lib()
    for rec in (0, 6, 32768 + 4):
        assert _write(rec=rec) == dpf.DPF_ERR_PARAM, rec
        assert _write(rec=rec, kpg=0) == dpf.DPF_ERR_PARAM
    assert _write(logN=64, kl=4096) == dpf.DPF_ERR_PARAM
    assert b"logN > 63" in L.dpf_last_error()
    assert _write(kl=17 + 18 * (LOGN - 7) - 1) == dpf.DPF_ERR_KEYLEN
    assert b"key shorter" in L.dpf_last_error()
    assert _write(nrec=(1 << LOGN) + 1) == dpf.DPF_ERR_PARAM
    assert b"domain" in L.dpf_last_error()
    assert _write(nrec=1 << LOGN, msgs=None) == dpf.DPF_ERR_PARAM and b"null" in L.dpf_last_error()
    assert _write(ng=1 << 16, kpg=1 << 16) == dpf.DPF_ERR_PARAM
    assert b"32 bits" in L.dpf_last_error()
    for name in ("keys", "msgs", "dbs", "work"):
        assert _write(**{name: None}) == dpf.DPF_ERR_PARAM, name
        assert b"null" in L.dpf_last_error()
    for name in ("msgs", "dbs", "work"):
        assert _write(**{name: P + 8}) == dpf.DPF_ERR_PARAM, name
        assert b"misaligned" in L.dpf_last_error()
    # The order of reports: width, key, nrec, key rows, null, misaligned.
    assert _write(rec=6, kl=10) == dpf.DPF_ERR_PARAM
    assert _write(kl=10, nrec=1 << 20) == dpf.DPF_ERR_KEYLEN
    assert _write(nrec=1 << 20, ng=1 << 31) == dpf.DPF_ERR_PARAM and b"domain" in L.dpf_last_error()
    assert _write(ng=1 << 31, keys=None) == dpf.DPF_ERR_PARAM and b"32 bits" in L.dpf_last_error()
    assert _write(keys=None, dbs=P + 8) == dpf.DPF_ERR_PARAM and b"null" in L.dpf_last_error()
    assert _write(ng=0) == dpf.DPF_OK
    assert _write(kpg=0) == dpf.DPF_OK
    assert _write(nrec=0) == dpf.DPF_OK
    assert _write(ng=0, kl=10) == dpf.DPF_ERR_KEYLEN
    # The workspace is the grouped answer's, unchanged: the sum of the parts of its layout.
    r256 = lambda x: (x + 255) // 256 * 256
    assert dpf.pir_grouped_workspace_size(3, 2, LOGN, 20) == (
        r256(dpf.workspace_size(6, LOGN)) + r256(6 * dpf.evalfull_len(LOGN)) + dpf.xor_fold_grouped_workspace_size(3, 2, 20))


def test_handle_entry_rejects_a_null_handle():
    buf = (ctypes.c_uint8 * 256)()
    L = dpf.lib()
    assert L.dpf_pir_db_write_grouped(None, buf, KL, 1, buf) == dpf.DPF_ERR_PARAM
    assert b"null PIR handle" in L.dpf_last_error()
    assert L.dpf_pir_db_write_grouped(None, buf, KL, 0, buf) == dpf.DPF_ERR_PARAM


def test_python_wrappers_exist():
    for name in ("xor_scatter_grouped_dev", "pir_write_grouped_dev", "scatter_grouped_form_for"):
        assert callable(getattr(dpf, name))
    assert hasattr(dpf.PirDB, "write_grouped")
    from dpf import buckets
    assert callable(buckets.write_plan)


def test_form_query_is_the_plan():
    """dpf_scatter_grouped_form_for with cus > 0 needs no device."""
    f = dpf.scatter_grouped_form_for(7, 7, 300, 36, cus=256)
    assert f.route == dpf.SCATTER_GROUPED and f.columns == 2 and f.passes == 2 and f.pass_widths == 8 | 4     # widths 4 and 3: bit w - 1
    assert f.runs == 2 and f.sg_per_run == 1 and f.units == 7 * 2 * 2 and f.launches == 2
    f = dpf.scatter_grouped_form_for(100000, 1, 256, 32, cus=256)
    assert f.route == dpf.SCATTER_GROUPED and f.units == 100000 and f.launches == 1 and f.pass_widths == 1
    assert dpf.scatter_grouped_form_for(1, 70, 600, 32, cus=256).route == dpf.SCATTER_LOOP
    try:
        dpf.set_fold_limits(8, 2)
        f = dpf.scatter_grouped_form_for(3000, 5, 1100, 32, cus=256)     # groups enough for one run each: max_sg cuts them
        assert f.max_blocks == 8 and f.sg_per_run == 2 and f.runs == 3 and f.units == 9000
        assert f.passes == 2 and f.launches == 2 * 1125 and f.pass_widths == 8 | 1
        f = dpf.scatter_grouped_form_for(300, 5, 1100, 32, cus=256)      # fewer workgroups than the chip takes: runs of one
        assert f.sg_per_run == 1 and f.runs == 5 and f.units == 1500 and f.launches == 2 * 188
    finally:
        dpf.set_fold_limits(0, 0)
    L = dpf.lib()
    c = dpf.ScatterGroupedFormC()
    assert L.dpf_scatter_grouped_form_for(3, 2, 300, 6, 256, ctypes.byref(c)) == dpf.DPF_ERR_PARAM
    assert L.dpf_scatter_grouped_form_for(1 << 31, 2, 300, 32, 256, ctypes.byref(c)) == dpf.DPF_ERR_PARAM
    assert L.dpf_scatter_grouped_form_for(3, 2, 300, 32, 256, None) == dpf.DPF_ERR_PARAM
    assert L.dpf_scatter_grouped_form_for(0, 2, 300, 32, 256, ctypes.byref(c)) == dpf.DPF_OK and c.launches == 0
