"""The launch plan of k_eval_bits with a point list per group
(dpf-go_amd/csrc/eval_bits_plan.hpp: the keys of group g evaluated at group
g's own list) needs no device: it is pure arithmetic, replayed wave by wave
by a stand-alone C++ program under ASan + UBSan."""
import functools
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


@functools.lru_cache(maxsize=1)
def _program(tmp):
    src = os.path.join(ROOT, "tests", "c", "eval_bits_group_plan_test.cpp")
    exe = os.path.join(tmp, "eval_bits_group_plan_test")
    errs = []
    for cxx in _sanitizer_compiler():
        static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
        r = subprocess.run([cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", *static,
                            "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I",
                            os.path.join(ROOT, "dpf-go_amd", "csrc"), src, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        errs.append(cxx + ": " + r.stderr[-1500:])
    pytest.fail("no compiler built the sanitizer program:\n" + "\n".join(errs))


def test_eval_bits_group_planner_under_sanitizers(tmp_path_factory):
    """tests/c/eval_bits_group_plan_test.cpp: over npts {1, 64, 127, 128, 129,
    257, 1000} x groups {1, 3, 65} x keys per group {1, 2, 5} x CU counts
    {4, 256} the replayed launch owns every (key, unit) exactly once, loads
    every point from inside the key's own list [g * npts, (g + 1) * npts) of an
    array of exactly groups * npts points, clamps a tail lane to
    g * npts + npts - 1 and keeps it out of the mask, writes the row bytes of
    the ungrouped plan, and has the ungrouped launch's form; the grid limit is
    refused at the ungrouped bound, nlists * npts overflowing 64 bits is
    refused, and keys_per_list = nkeys reproduces the ungrouped form field by
    field.  The program has its own main and is run directly (the sanitizer
    runtimes are linked into it)."""
    exe = _program(str(tmp_path_factory.mktemp("eval_bits_group_plan")))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "eval_bits_group_plan ok" in r.stdout
