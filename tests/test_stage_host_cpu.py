"""The host side of the host-buffer entry points that needs no device, as
stand-alone C++ programs under sanitizers: the chunk plans of
dpf-go_amd/csrc/stage_plan.hpp (tests/c/stage_plan_test.cpp) and the copy
pool of copy_pool.hpp (tests/c/copy_pool_test.cpp).  Each program has its own
main and is run directly: the sanitizer runtimes are linked into it."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(name, sanitize, tmp_path, extra=()):
    """tests/c/<name>.cpp with -fsanitize=<sanitize>, by the first compiler
    here that links it; (exe, None) or (None, the compilers' errors)."""
    src = os.path.join(ROOT, "tests", "c", name + ".cpp")
    exe = str(tmp_path / (name + "_" + sanitize.split(",")[0]))
    errs = []
    for cxx in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")):
        if not cxx or not os.path.exists(cxx):
            continue
        # The runtimes are linked statically (clang's default), so the program
        # runs whatever else the environment preloads.
        static = []
        if os.path.basename(cxx).startswith("g++"):
            static = ["-static-lib" + {"address": "asan", "undefined": "ubsan", "thread": "tsan"}[s]
                      for s in sanitize.split(",")]
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=" + sanitize, *static,
                            "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", *extra, "-I",
                            os.path.join(ROOT, "dpf-go_amd", "csrc"), src, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe, None
        errs.append(cxx + ": " + r.stderr[-1500:])
    return None, "\n".join(errs)


def _run(exe, marker, **env):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert marker in r.stdout
    return r.stdout


def test_stage_plans_under_sanitizers(tmp_path):
    """Every plan tiles its output exactly once, in order, within the staging
    capacity (a sweep over batch sizes and logN, nothing skipped), and the
    plans of the shapes the benchmarks and tests use have the hand-computed
    chunk sizes, prefixes and offsets."""
    exe, errs = _build("stage_plan_test", "address,undefined", tmp_path)
    assert exe, "no compiler built the sanitizer program:\n" + errs
    out = _run(exe, "stage_plan ok", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    assert ", 0 skipped" in out


def test_copy_pool_under_asan_ubsan(tmp_path):
    """Four caller threads share the pool: copies of one byte, one piece, one
    piece and a byte and several pieces with a ragged end, the parallel first
    touch, and a copy of nothing from null pointers."""
    exe, errs = _build("copy_pool_test", "address,undefined", tmp_path, ["-pthread"])
    assert exe, "no compiler built the sanitizer program:\n" + errs
    _run(exe, "copy_pool ok", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")


def test_copy_pool_under_tsan(tmp_path):
    """The same program under ThreadSanitizer: the job list, the piece
    counters and the hand-over of a finished job between callers and workers."""
    exe, errs = _build("copy_pool_test", "thread", tmp_path, ["-pthread"])
    if exe is None:
        pytest.skip("no compiler links -fsanitize=thread here:\n" + errs)
    _run(exe, "copy_pool ok", TSAN_OPTIONS="halt_on_error=1")
