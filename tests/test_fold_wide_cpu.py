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


# ---- validation table of the three fold and the two slice entry points -----
# Every row is (entry, arguments that differ from a valid call, expected code,
# expected dpf_last_error text).  Rows with two faults pin the order of the
# checks through the text.  Only rows that fail validation, or have nkeys == 0,
# are listed: nothing here reaches a kernel launch.
MAX_REC = 32768   # DPF_PIR_MAX_REC_BYTES (include/dpf_hip.h)
E_REC = "dpf: rec_bytes must be a positive multiple of 32"
E_RECW = E_REC + ", at most DPF_PIR_MAX_REC_BYTES"
E_STRIDE = "dpf: bits_stride must be a multiple of 16"
E_NREC = "dpf: more records than selection bits per key"
E_ALIGN = "dpf: misaligned device buffer"
E_NULL = "dpf: null device buffer"

# entry -> (C function, takes rec_bytes, default rec_bytes, rec_bytes error text, checks d_work % 16)
FOLDS = {
    "fold": ("dpf_xor_fold_dev", True, 32, E_REC, False),
    "sliced": ("dpf_xor_fold_sliced_dev", False, 32, None, False),
    "wide32": ("dpf_xor_fold_sliced_wide_dev", True, 32, E_RECW, False),
    "wide64": ("dpf_xor_fold_sliced_wide_dev", True, 64, E_RECW, True),
}
SLICES = {"slice": ("dpf_pir_db_slice_dev", False), "slice_wide": ("dpf_pir_db_slice_wide_dev", True)}


def _call(entry, **kw):
    L = dpf.lib()
    if entry in FOLDS:
        name, has_rec, rec = FOLDS[entry][:3]
        a = dict(bits=P, stride=16, nkeys=1, dbs=P, nrec=128, rec=rec, ans=P, work=P)
        a.update(kw)
        mid = (a["rec"],) if has_rec else ()
        return getattr(L, name)(0, a["bits"], a["stride"], a["nkeys"], a["dbs"], a["nrec"], *mid, a["ans"], a["work"],
                                None)
    name, has_rec = SLICES[entry]
    a = dict(db=P, nrec=100, rec=64, dbs=P)
    a.update(kw)
    mid = (a["rec"],) if has_rec else ()
    return getattr(L, name)(0, a["db"], a["nrec"], *mid, a["dbs"], None)


def _validation_rows():
    ok, bad = dpf.DPF_OK, dpf.DPF_ERR_PARAM
    rows = []
    for e, (_, has_rec, _, e_rec, work16) in FOLDS.items():
        if has_rec:
            rows += [(e, dict(rec=0), bad, e_rec), (e, dict(rec=48), bad, e_rec)]
            # above the maximum: dpf_xor_fold_dev alone has no cap (nkeys = 0: nothing is launched)
            rows.append((e, dict(rec=MAX_REC + 32, nkeys=0), *((ok, None) if e == "fold" else (bad, e_rec))))
            rows.append((e, dict(rec=48, stride=24, nrec=8), bad, e_rec))              # rec_bytes before bits_stride
            rows.append((e, dict(rec=0, bits=None, dbs=None, ans=None, work=None), bad, e_rec))
        rows.append((e, dict(stride=24, nrec=8), bad, E_STRIDE))
        rows.append((e, dict(stride=24, nrec=1000), bad, E_STRIDE))                    # bits_stride before nrec
        rows.append((e, dict(nrec=129), bad, E_NREC))
        rows.append((e, dict(nrec=129, bits=P + 8), bad, E_NREC))                      # nrec before alignment
        rows += [(e, dict(bits=P + 8), bad, E_ALIGN), (e, dict(dbs=P + 8), bad, E_ALIGN),
                 (e, dict(ans=P + 2), bad, E_ALIGN)]
        # d_work's alignment is checked by the wide sliced form above 32 bytes only, and before nkeys == 0
        rows.append((e, dict(work=P + 8, nkeys=0), *((bad, E_ALIGN) if work16 else (ok, None))))
        rows.append((e, dict(bits=P + 8, ans=None), bad, E_ALIGN))                     # alignment before null
        rows += [(e, {arg: None}, bad, E_NULL) for arg in ("bits", "dbs", "ans", "work")]
        rows.append((e, dict(nkeys=0), ok, None))
        rows.append((e, dict(nkeys=0, bits=None, dbs=None, ans=None, work=None), ok, None))
    for e, (_, has_rec) in SLICES.items():
        if has_rec:
            rows += [(e, dict(rec=r), bad, E_RECW) for r in (0, 48, MAX_REC + 32)]
            rows.append((e, dict(rec=48, db=None), bad, E_RECW))                       # rec_bytes before null
        rows += [(e, dict(db=P + 8), bad, E_ALIGN), (e, dict(dbs=P + 8), bad, E_ALIGN)]
        rows += [(e, dict(db=None), bad, E_NULL), (e, dict(dbs=None), bad, E_NULL)]
        rows.append((e, dict(db=None, dbs=P + 8), bad, E_NULL))                        # null before alignment
    return rows


@pytest.mark.parametrize("entry,args,code,text", _validation_rows(),
                         ids=[r[0] + ":" + ",".join(f"{k}={v}" for k, v in r[1].items()) for r in _validation_rows()])
def test_fold_and_slice_validation_table(entry, args, code, text):
    assert _call(entry, **args) == code
    if text is not None:
        assert dpf.lib().dpf_last_error().decode() == text


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 4000])
def test_sliced_size_is_the_wide_size_at_32(n):
    assert dpf.lib().dpf_pir_db_sliced_size(n) == dpf.lib().dpf_pir_db_sliced_size_wide(n, 32) == max(
        16, (n + 255) // 256 * 256 * 32)
    assert dpf.lib().dpf_pir_db_sliced_size_wide(n, 48) == 0
    assert dpf.lib().dpf_pir_db_sliced_size_wide(n, MAX_REC + 32) == 0


def test_create_wide_rejects_bad_rec_bytes_and_clears_the_handle():
    h = ctypes.c_void_p(1234)
    db = (ctypes.c_uint8 * 96)()
    rc = dpf.lib().dpf_pir_db_create_wide(db, 2, 48, 12, 1, ctypes.byref(h))
    assert rc == dpf.DPF_ERR_PARAM
    assert not h.value
    assert dpf.lib().dpf_pir_db_rec_bytes(None) == 0
