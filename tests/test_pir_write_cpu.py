"""Private writes into a PIR DB (dpf_xor_scatter_*_dev, dpf_pir_write_*_dev,
dpf_pir_db_write), the parts that need no device: the header and the library
agree on the entry points, their argument checks (validation precedes any
device call, so fake aligned addresses are never dereferenced, as in
test_pir_update_cpu.py), and the launch planner as a stand-alone C++ program
under ASan + UBSan."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import dpf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096   # aligned fake device address, never used
ENTRIES = ("dpf_xor_scatter_dev", "dpf_xor_scatter_sliced_wide_dev", "dpf_pir_write_wide_dev",
           "dpf_pir_write_sliced_wide_dev", "dpf_pir_db_write")
LOGN = 12


def _scatter(name, bits=P, stride=64, nkeys=3, msgs=P, db=P, nrec=300, rec=64):
    return getattr(dpf.lib(), name)(0, bits, stride, nkeys, msgs, db, nrec, rec, None)


def _write(name, keys=P, klen=None, nkeys=3, logN=LOGN, pbits=0, prefix=0, msgs=P, db=P, nrec=300, rec=64, work=P):
    klen = dpf.key_len(logN) if klen is None else klen
    return getattr(dpf.lib(), name)(0, keys, klen, nkeys, logN, pbits, prefix, msgs, db, nrec, rec, work, None)


SCATTERS = [lambda **kw: _scatter("dpf_xor_scatter_dev", **kw),
            lambda **kw: _scatter("dpf_xor_scatter_sliced_wide_dev", **kw)]
WRITES = [lambda **kw: _write("dpf_pir_write_wide_dev", **kw),
          lambda **kw: _write("dpf_pir_write_sliced_wide_dev", **kw)]


def test_header_declares_and_library_exports_the_entry_points():
    with open(os.path.join(ROOT, "include", "dpf_hip.h")) as f:
        header = f.read()
    for name in ENTRIES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in dpf.SIGNATURES
        assert getattr(dpf.lib(), name) is not None


@pytest.mark.parametrize("rec", [0, 48, 32800])
def test_dev_entries_reject_bad_rec_bytes(rec):
    for f in SCATTERS + WRITES:
        assert f(rec=rec) == dpf.DPF_ERR_PARAM
        assert f(rec=rec, nkeys=0) == dpf.DPF_ERR_PARAM      # also with nothing to do


def test_dev_entries_reject_null_buffers():
    for f in SCATTERS:
        for arg in ("bits", "msgs", "db"):
            assert f(**{arg: None}) == dpf.DPF_ERR_PARAM, arg
    for f in WRITES:
        for arg in ("keys", "msgs", "db", "work"):
            assert f(**{arg: None}) == dpf.DPF_ERR_PARAM, arg


def test_dev_entries_reject_misaligned_buffers():
    for f in SCATTERS:
        for arg in ("bits", "msgs", "db"):
            assert f(**{arg: P + 8}) == dpf.DPF_ERR_PARAM, arg
    for f in WRITES:
        for arg in ("msgs", "db", "work"):
            assert f(**{arg: P + 8}) == dpf.DPF_ERR_PARAM, arg


def test_scatter_entries_check_the_bits_shape():
    for f in SCATTERS:
        assert f(stride=40) == dpf.DPF_ERR_PARAM              # not a multiple of 16
        assert f(stride=72) == dpf.DPF_ERR_PARAM
        assert f(stride=32, nrec=257) == dpf.DPF_ERR_PARAM    # nrec > 8 * bits_stride
        assert f(stride=48, nrec=385) == dpf.DPF_ERR_PARAM


def test_write_entries_check_the_slice_and_the_key():
    for f in WRITES:
        assert f(nrec=(1 << LOGN) + 1) == dpf.DPF_ERR_PARAM               # more records than the domain
        assert f(pbits=2, prefix=1, nrec=(1 << (LOGN - 2)) + 1) == dpf.DPF_ERR_PARAM
        assert f(pbits=2, prefix=4) == dpf.DPF_ERR_PARAM                  # prefix outside its bits
        assert f(klen=16 + 18 * (LOGN - 7)) == dpf.DPF_ERR_KEYLEN         # one byte short of the last correction word


def test_dev_entries_with_nothing_to_do_launch_nothing():
    """nkeys == 0 or nrec == 0 with valid arguments is DPF_OK before any device call (no GPU here)."""
    for f in SCATTERS + WRITES:
        assert f(nkeys=0) == dpf.DPF_OK
        assert f(nrec=0) == dpf.DPF_OK


def test_handle_entry_rejects_a_null_handle():
    buf = (ctypes.c_uint8 * 256)()
    assert dpf.lib().dpf_pir_db_write(None, buf, dpf.key_len(LOGN), 1, buf) == dpf.DPF_ERR_PARAM
    assert dpf.lib().dpf_pir_db_write(None, buf, dpf.key_len(LOGN), 0, buf) == dpf.DPF_ERR_PARAM


def test_python_wrappers_exist():
    for name in ("xor_scatter_dev", "xor_scatter_sliced_wide_dev", "pir_write_wide_dev", "pir_write_sliced_wide_dev"):
        assert callable(getattr(dpf, name))
    assert hasattr(dpf.PirDB, "write")


def _sanitizer_compiler():
    """A C++ compiler that links -fsanitize=address,undefined here."""
    for cxx in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")):
        if cxx and os.path.exists(cxx):
            yield cxx


def test_scatter_planner_under_sanitizers(tmp_path):
    """tests/c/pir_scatter_plan_test.cpp: over nrec x C x nkeys x max_blocks x
    max_sg the planned (super-group run, column group, key tile) units cover
    every (S, c, k) exactly once and none exceeds a limit.  The program has
    its own main and is run directly (the sanitizer runtimes are linked into
    it)."""
    src = os.path.join(ROOT, "tests", "c", "pir_scatter_plan_test.cpp")
    exe = str(tmp_path / "pir_scatter_plan_test")
    errs = []
    for cxx in _sanitizer_compiler():
        static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
        r = subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", *static,
                            "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I",
                            os.path.join(ROOT, "dpf-go_amd", "csrc"), src, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            break
        errs.append(cxx + ": " + r.stderr[-1500:])
    else:
        pytest.fail("no compiler built the sanitizer program:\n" + "\n".join(errs))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "pir_scatter_plan ok" in r.stdout
