"""In-place update / read-back of a resident PIR DB, the parts that need no
device: argument checks of the two _dev entry points and of the handle entry
points (validation precedes any device call, so fake aligned addresses are
never dereferenced, as in test_fold_wide_cpu.py), and the host planner
(range check, stable sort, keep-last dedupe, shard split) as a stand-alone
C++ program under ASan + UBSan."""
import ctypes
import os
import shutil
import subprocess

import pytest

import dpf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096   # aligned fake device address, never used


def _update(dbs=P, rec=64, idx=P, recs=P, n=3, nrec=100):
    return dpf.lib().dpf_pir_db_update_sliced_wide_dev(0, dbs, nrec, rec, idx, recs, n, None)


def _gather(dbs=P, rec=64, idx=P, out=P, n=3, nrec=100):
    return dpf.lib().dpf_pir_db_gather_sliced_wide_dev(0, dbs, nrec, rec, idx, n, out, None)


@pytest.mark.parametrize("rec", [0, 33, 48])
def test_dev_entries_reject_bad_rec_bytes(rec):
    assert _update(rec=rec) == dpf.DPF_ERR_PARAM
    assert _gather(rec=rec) == dpf.DPF_ERR_PARAM
    assert _update(rec=rec, n=0) == dpf.DPF_ERR_PARAM      # also with nothing to do
    assert _gather(rec=rec, n=0) == dpf.DPF_ERR_PARAM


@pytest.mark.parametrize("rec", [32, 64, 1024])
def test_dev_entries_reject_misaligned_pointers(rec):
    assert _update(rec=rec, dbs=P + 8) == dpf.DPF_ERR_PARAM
    assert _update(rec=rec, recs=P + 8) == dpf.DPF_ERR_PARAM
    assert _update(rec=rec, idx=P + 4) == dpf.DPF_ERR_PARAM
    assert _gather(rec=rec, dbs=P + 8) == dpf.DPF_ERR_PARAM
    assert _gather(rec=rec, out=P + 8) == dpf.DPF_ERR_PARAM
    assert _gather(rec=rec, idx=P + 4) == dpf.DPF_ERR_PARAM


@pytest.mark.parametrize("rec", [32, 64, 1024])
def test_dev_entries_reject_null_pointers(rec):
    for arg in ("dbs", "idx", "recs"):
        assert _update(rec=rec, **{arg: None}) == dpf.DPF_ERR_PARAM
    for arg in ("dbs", "idx", "out"):
        assert _gather(rec=rec, **{arg: None}) == dpf.DPF_ERR_PARAM


@pytest.mark.parametrize("rec", [32, 64, 1024])
def test_dev_entries_with_nothing_to_do_launch_nothing(rec):
    """n == 0 with valid arguments is DPF_OK before any device call (no GPU here)."""
    assert _update(rec=rec, n=0) == dpf.DPF_OK
    assert _gather(rec=rec, n=0) == dpf.DPF_OK
    assert _update(rec=rec, idx=P + 8, n=0) == dpf.DPF_OK      # 8-byte aligned indices are enough


def test_handle_entries_reject_a_null_handle():
    L = dpf.lib()
    idx = (ctypes.c_uint64 * 2)(1, 2)
    buf = (ctypes.c_uint8 * 64)()
    assert L.dpf_pir_db_update(None, idx, buf, 2) == dpf.DPF_ERR_PARAM
    assert L.dpf_pir_db_read(None, idx, 2, buf) == dpf.DPF_ERR_PARAM
    assert L.dpf_pir_db_update(None, idx, buf, 0) == dpf.DPF_ERR_PARAM
    assert L.dpf_pir_db_nrec(None) == 0


def test_python_wrappers_exist():
    for name in ("pir_db_update_sliced_wide_dev", "pir_db_gather_sliced_wide_dev"):
        assert callable(getattr(dpf, name))
    for name in ("update", "read", "nrec"):
        assert hasattr(dpf.PirDB, name)


def _sanitizer_compiler():
    """A C++ compiler that links -fsanitize=address,undefined here."""
    for cxx in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")):
        if cxx and os.path.exists(cxx):
            yield cxx


def test_host_planner_under_sanitizers(tmp_path):
    """tests/c/pir_update_plan_test.cpp: sort stability, keep-last dedupe,
    rejection of an out-of-range index with the plan untouched, the shard
    split at pbits 0, 1 and 3 with boundary indices and empty shards.  The
    program has its own main and is run directly (the sanitizer runtimes are
    linked into it)."""
    src = os.path.join(ROOT, "tests", "c", "pir_update_plan_test.cpp")
    exe = str(tmp_path / "pir_update_plan_test")
    errs = []
    for cxx in _sanitizer_compiler():
        # The runtimes are linked statically (clang's default), so the program
        # runs whatever else the environment preloads.
        static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", *static,
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
    assert "pir_update_plan ok" in r.stdout
