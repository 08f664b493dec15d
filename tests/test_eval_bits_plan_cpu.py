"""The launch plan of k_eval_bits (dpf-go_amd/csrc/eval_bits_plan.hpp: Eval of
every key at one shared list of points into packed selection bits) needs no
device: it is pure arithmetic, replayed wave by wave by a stand-alone C++
program under ASan + UBSan."""
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
    src = os.path.join(ROOT, "tests", "c", "eval_bits_plan_test.cpp")
    exe = os.path.join(tmp, "eval_bits_plan_test")
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


def test_eval_bits_planner_under_sanitizers(tmp_path_factory):
    """tests/c/eval_bits_plan_test.cpp: over npts {1, 2, 63, 64, 65, 127, 128,
    129, 255, 256, 257, 1000, 2^20 + 1} x nkeys {1, 3, 64, 65, 4097} x CU
    counts {4, 64, 256} the replayed launch owns every (key, unit) exactly
    once, writes every row byte below dpf_eval_bits_stride(npts) exactly once
    and none beyond, gives the last unit exactly npts - 128 (units - 1) valid
    lanes, never clamps an index past npts - 1, is refused exactly above
    2^31 - 1 workgroups, and takes the frontier level of
    eval_frontier_level(stop, npts) (root walks where eval_form falls back).
    The program has its own main and is run directly (the sanitizer runtimes
    are linked into it)."""
    exe = _program(str(tmp_path_factory.mktemp("eval_bits_plan")))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "eval_bits_plan ok" in r.stdout
