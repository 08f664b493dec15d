"""The tree kernel's and the batched Eval's launch plans
(dpf-go_amd/csrc/tree_plan.hpp) need no device: they are pure arithmetic,
checked by a stand-alone C++ program under ASan + UBSan.  The same program
lists the kernel forms that tests/test_gpu_tree_forms.py reaches, and the
query entry points (dpf_tree_form_for, dpf_eval_form_for) answer from the same
header without a device when given a CU count."""
import functools
import os
import re
import shutil
import subprocess

import pytest

import dpf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Largest output (bytes of leaves, or Eval result bytes) a form's cheapest
# representative may need.  The plan needs 6 MiB at the most (3 keys at logN 24
# on a 4-CU stream).
CAP = 8 << 20
# Node passes below a prefix exist on the byte-sliced route only, at 128 bytes
# of leaves per node: the deepest such form (d = 7, 512-thread one-key
# workgroups) needs 40 MiB (5 keys to level 17 below a 1-bit prefix on 4 CUs).
CAP_NODEPFX = 40 << 20


def _sanitizer_compiler():
    """A C++ compiler that links -fsanitize=address,undefined here."""
    for cxx in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")):
        if cxx and os.path.exists(cxx):
            yield cxx


@functools.lru_cache(maxsize=1)
def _program(tmp):
    src = os.path.join(ROOT, "tests", "c", "tree_plan_test.cpp")
    exe = os.path.join(tmp, "tree_plan_test")
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
    return _program(str(tmp_path_factory.mktemp("tree_plan")))


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_tree_planner_under_sanitizers(program):
    """tests/c/tree_plan_test.cpp: over key counts x tree depths x prefixes x
    leaf / node launches x CU counts x forced depths every tree plan picks a
    minimal power-of-two workgroup, tiles each key's output exactly once,
    has an exact grid and is refused exactly when that grid exceeds 2^31 - 1;
    uniform, raw, cw_lds, the walk kind, l1 and feedback follow the rules the
    kernel applies, and no workgroup that takes the shared walk has a thread
    past the end.  The batched-Eval plans obey the frontier rule, the
    persistent kernel's conditions and the grid limits.  The recorded plans
    (the benchmark's shapes, test_every_subtree_depth's table) are reproduced.
    The program has its own main and is run directly (the sanitizer runtimes
    are linked into it)."""
    out = _run(program)
    assert "tree_plan ok" in out
    print(out)


FORM = re.compile(r"^FORM (leaf|node|nodepfx) d (\d+) block (\d+) uniform (\d) raw (\d) cw_lds (\d) walk (\d) feedback (\d) "
                  r"prefixed (\d) rep nkeys (\d+) depth (\d+) pb (\d+) cus (\d+) cost (\d+)$", re.M)


def test_no_form_without_a_small_representative(program):
    """Every form of k_evalfull that the GPU matrix's universe reaches on 256,
    64, 16 and 4 CUs has a representative call of at most CAP bytes of
    output (CAP_NODEPFX for node passes below a prefix), so
    tests/test_gpu_tree_forms.py leaves none out; among them are
    the forms that only narrow streams reach at small sizes: 1024-thread
    feedback workgroups with and without the quad walk, and 1024-thread
    per-lane-key workgroups at D = 6 and 7."""
    out = _run(program, "forms")
    forms = [(m[1],) + tuple(int(x) for x in m.groups()[1:]) for m in FORM.finditer(out)]
    totals = dict((k, int(n)) for k, n in re.findall(r"^FORMS (leaf|node|nodepfx) total (\d+)", out, re.M))
    leaf = [f for f in forms if f[0] == "leaf"]
    node = [f for f in forms if f[0] == "node"]
    pfx = [f for f in forms if f[0] == "nodepfx"]
    assert len(leaf) == totals["leaf"] and len(node) == totals["node"] and len(pfx) == totals["nodepfx"]
    assert leaf and node and pfx
    print("reachable forms: %d leaf, %d node; largest representative %d bytes; node launches with a prefix: "
          "%d forms, largest representative %d bytes" % (len(leaf), len(node), max(f[-1] for f in leaf + node),
                                                          len(pfx), max(f[-1] for f in pfx)))
    over = [f for f in leaf + node if f[-1] > CAP] + [f for f in pfx if f[-1] > CAP_NODEPFX]
    assert not over, over
    assert max(f[-1] for f in pfx) == CAP_NODEPFX       # the cap is what the plan needs, no more
    assert {f[6] for f in pfx} >= {dpf.WALK_NONE, dpf.WALK_QUAD}
    assert {f[1:8] for f in pfx} <= {f[1:8] for f in node}
    # kind d block uniform raw cw_lds walk feedback prefixed ...
    fb = [f for f in leaf if f[7]]
    assert fb and all(f[2] == 1024 and f[1] >= 6 and f[3] for f in fb)
    assert {f[6] for f in fb} == {dpf.WALK_NONE, dpf.WALK_QUAD}
    assert {f[1] for f in leaf if f[2] == 1024 and not f[3]} == {6, 7}
    assert {f[1] for f in leaf} == set(range(8)) and {f[1] for f in node} == set(range(8))
    assert {f[2] for f in leaf} == {64, 128, 256, 512, 1024} and {f[2] for f in node} == {64, 128, 256, 512}
    assert not any(f[7] or f[4] for f in node)


def test_form_queries_need_no_device():
    """dpf_tree_form_for / dpf_eval_form_for with a CU count answer from the
    plan header alone: the benchmark's tree shape, a per-lane-key shape, a
    node pass, and the three Eval kernels."""
    f = dpf.tree_form_for(4096, 20, cus=256)
    assert (f.d, f.block, f.grid, f.walk) == (7, 1024, 256, dpf.WALK_NONE)
    assert f.uniform and f.raw and f.feedback and not f.nodes and not f.cw_lds and not f.prio_small
    f = dpf.tree_form_for(70, 16, cus=256)
    assert f.nunits == 70 << f.units_log and f.ltop + f.d == 9 and f.uniform == f.raw == (f.units_log >= 6)
    f = dpf.tree_form_for(1, 24, cus=4)
    assert f.cw_lds and f.walk == dpf.WALK_QUAD and f.l1 == f.ltop - f.w + 6 and f.nunits % f.block == 0
    n = dpf.tree_form_for(70, 16, node_level=7, cus=256)
    assert n.nodes and not n.raw and n.ltop + n.d == 7 and n.nunits == 70 << n.units_log
    with pytest.raises(dpf.DPFPanic):
        dpf.tree_form_for(1, 20, prefix_bits=14, cus=256)
    with pytest.raises(dpf.DPFPanic):
        dpf.tree_form_for(1, 20, node_level=14, cus=256)
    ws = dpf.eval_workspace_size(8, 256, 21)
    e = dpf.eval_form_for(8, 256, 21, ws, True, cus=256)
    assert (e.level, e.kernel, e.block, e.grid, e.cw_staged) == (7, dpf.EVAL_PERSIST, 1024, 1, True)
    assert e.nodes.nodes and e.nodes.ltop + e.nodes.d == 7
    assert not dpf.eval_form_for(8, 256, 22, dpf.eval_workspace_size(8, 256, 22), True, cus=256).cw_staged
    e = dpf.eval_form_for(8, 256, 21, ws, False, cus=256)
    assert (e.level, e.kernel) == (7, dpf.EVAL_PAIR_UNIFORM)
    e = dpf.eval_form_for(8, 256, 21, 8 * (21 - 7 + 2) * 32, True, cus=256)   # the key records alone: root walks
    assert (e.level, e.kernel, e.nodes) == (0, dpf.EVAL_PAIR_UNIFORM, None)
    e = dpf.eval_form_for(3, 33, 9, dpf.eval_workspace_size(3, 33, 9), True, cus=256)
    assert (e.level, e.kernel, e.ragged) == (0, dpf.EVAL_PAIR, True)
