"""The piece plan of the whole-DB read-out and merge
(dpf-go_amd/csrc/pir_export_plan.hpp) needs no device: it is pure integer
arithmetic, checked by a stand-alone C++ program under ASan + UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sanitizer_compiler():
    """A C++ compiler that links -fsanitize=address,undefined here."""
    for cxx in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")):
        if cxx and os.path.exists(cxx):
            yield cxx


def test_export_planner_under_sanitizers(tmp_path):
    """tests/c/pir_export_plan_test.cpp: over kinds (dense, sparse, grouped) x
    shard counts {1, 2, 3, 8} x record counts around super-group and shard
    boundaries x group sizes {1, 255, 256, 257, 300} x ranges (empty, one
    record, all, one off a boundary, across a shard or group boundary) x
    chunks {256, 512, 1280} every wanted record is delivered exactly once and
    in order from where the layout rule puts it, every piece starts on a local
    multiple of 256, stays inside its shard and the chunk, no pad record is
    delivered, and a range outside the DB is refused.  The program has its own
    main and is run directly (the sanitizer runtimes are linked into it)."""
    src = os.path.join(ROOT, "tests", "c", "pir_export_plan_test.cpp")
    exe = str(tmp_path / "pir_export_plan_test")
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
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "pir_export_plan ok" in r.stdout
