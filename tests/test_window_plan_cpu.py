"""The window plan of the ranged PIR forms (dpf-go_amd/csrc/pir_window_plan.hpp)
needs no device: pure arithmetic, checked by a stand-alone C++ program under
ASan + UBSan, as tests/test_tree_plan_cpu.py checks the tree plans."""
import functools
import os
import re
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
    src = os.path.join(ROOT, "tests", "c", "pir_window_plan_test.cpp")
    exe = os.path.join(tmp, "pir_window_plan_test")
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


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return _program(str(tmp_path_factory.mktemp("window_plan")))


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_window_planner_under_sanitizers(program):
    """tests/c/pir_window_plan_test.cpp: every (first_block, nblocks) at logN
    7..12, random windows and windows that touch the last block at logN 20, 40
    and 63: the pieces tile [row_offset, row_offset + 16 * nblocks) of the row,
    every piece touches the window, P <= 33, what is evaluated outside the
    window is under two pieces and under 1/8 of it (none where s is clamped),
    prefix_bits <= stop; a window inside an aligned subtree of at most twice
    its points takes the subtree route (found by search), one that is itself
    a subtree at row_offset 0, and no other window does; the balanced shard
    split is the sparse kind's.  The program has its
    own main and is run directly (the sanitizer runtimes are linked into it)."""
    out = _run(program)
    assert "pir_window_plan ok" in out
    print(out)


PLAN = re.compile(r"^PLAN (\d+) (\d+) (\d+): route (\d) prefix_bits (\d+) first_prefix (\d+) npieces (\d+) piece_bytes (\d+) "
                  r"row_bytes (\d+) row_offset (\d+)$", re.M)


def test_recorded_plans(program):
    """Small windows worked out by hand, the measured tables' windows
    (tools/pir_window_ab.py), one aligned subtree, a clamped s and a refusal."""
    shard3 = (24, 3 * 5 << 11, 5 << 11)          # shard 3 of 8 of 5 * 2^21 records: it straddles point 2^22
    wins = [(13, 24, 32), (14, 3, 37), (24, 0, 5 << 14), (24, 0, (1 << 16) + 2), (24, 0, 1 << 17), (9, 1, 2), (14, 63, 2),
            (14, 41, 39), shard3, (10, 7, 2)]
    out = _run(program, *[str(x) for w in wins for x in w])
    got = {tuple(int(x) for x in m.groups()[:3]): tuple(int(x) for x in m.groups()[3:]) for m in PLAN.finditer(out)}
    # route prefix_bits first_prefix npieces piece_bytes row_bytes row_offset
    # One subtree of at most twice the window's points:
    assert got[(13, 24, 32)] == (0, 0, 0, 1, 1024, 1024, 384)
    assert got[(14, 3, 37)] == (0, 1, 0, 1, 1024, 1024, 48)
    assert got[(24, 0, 5 << 14)] == (0, 0, 0, 1, 1 << 21, 1 << 21, 0)            # 5 * 2^21 records: the whole domain
    assert got[(24, 0, (1 << 16) + 2)] == (0, 0, 0, 1, 1 << 21, 1 << 21, 0)      # 2^23 + 256 records: twice, less 512
    assert got[(24, 0, 1 << 17)] == (0, 0, 0, 1, 1 << 21, 1 << 21, 0)
    assert got[(9, 1, 2)] == (0, 0, 0, 1, 64, 64, 16)
    # Pieces, where that subtree is larger:
    assert got[(14, 63, 2)] == (1, 7, 63, 2, 16, 32, 0)                          # s clamped at 7
    assert got[(14, 41, 39)] == (1, 6, 20, 20, 32, 640, 16)
    assert got[shard3] == (1, 8, 60, 20, 8192, 20 * 8192, 0)                     # 2^23 points would hold it: 6.4 times
    assert "PLAN 10 7 2: refused" in out
