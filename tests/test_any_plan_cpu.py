"""The launch plans for records of any width (dpf-go_amd/csrc/pir_fold_plan.hpp,
pir_scatter_plan.hpp) need no device: pure integer arithmetic, checked by a
stand-alone C++ program under ASan + UBSan (as tests/test_fold_plan_cpu.py)."""
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


def test_any_width_planner_under_sanitizers(tmp_path):
    """tests/c/pir_any_plan_test.cpp: over widths x nrec x limits x CU counts,
    the fold and private-write plans cover every existing (super-group, tile)
    cell exactly once and inside the buffer, the tiles a short last column
    lacks are those that would lie past it, a pass starts at byte
    S0 * 256 * rec_bytes, and the plans for multiples of 32 are unchanged.  The
    program has its own main and is run directly (the sanitizer runtimes are
    linked into it)."""
    src = os.path.join(ROOT, "tests", "c", "pir_any_plan_test.cpp")
    exe = str(tmp_path / "pir_any_plan_test")
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
    assert "pir_any_plan ok" in r.stdout
