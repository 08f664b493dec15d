"""The grouped fold's route rule and the launch plan of its matrix-core route
(dpf-go_amd/csrc/pir_group_fold_plan.hpp) need no device: they are pure
integer arithmetic, checked by a stand-alone C++ program under ASan + UBSan."""
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


def test_group_fold_planner_under_sanitizers(tmp_path):
    """tests/c/pir_group_fold_plan_test.cpp: over ngroups x gsg x C x kpg x CU
    counts x limits the matrix-core route folds every (group, super-group,
    column, key) cell exactly once, has no empty run, none across a group
    boundary and none longer than min(kFoldMaxSg, max_sg), keeps every key tile
    inside one group and its shape, the tiles (at most 256 keys) summing to
    kpg, keeps each launch inside the cap, and clears the answers exactly when
    a tile has several runs; the direct route is plan_fold_grouped's plan field
    for field, kpg <= 4 is direct without the knob, and the measured shapes
    take their recorded routes.  The program has its own main and is run
    directly (the sanitizer runtimes are linked into it)."""
    src = os.path.join(ROOT, "tests", "c", "pir_group_fold_plan_test.cpp")
    exe = str(tmp_path / "pir_group_fold_plan_test")
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
    assert "pir_group_fold_plan ok" in r.stdout
