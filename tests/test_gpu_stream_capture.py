"""The stream contract of the device entry points (include/dpf_hip.h:
"Asynchronous on `stream`.  Nothing is synchronised."), held by stream capture.

Every other GPU test passes stream=None, the null stream, which orders itself
against everything: a launch or memset sent to stream 0 instead of the
caller's, a synchronising call left in a composite, or a launch argument
computed on the host from device contents would all stay invisible there.  In
a global-mode stream capture the first two are HIP errors and the third is a
wrong answer at replay, so each case here runs one protocol on one torch side
stream S:

  1. two input sets A and B of one shape (other keys, DB bytes, messages,
     points, indices), their expected outputs computed on the CPU first (the
     oracle plus tests/pir_ref.py);
  2. A loaded, outputs poisoned, the call eager on S: equals expected(A) (and
     the library's lazy host state is warm);
  3. outputs poisoned, the same call captured on S: it returns DPF_OK, and
     after the capture nothing has executed (outputs still poison, a DB that
     is changed in place still in its initial state);
  4. B loaded into the same buffers, replay: expected(B); A again, replay:
     expected(A).  An answer for B that equals A's was baked on the host.

Sliced DBs, as inputs and as the expected state of an in-place operation,
come from the layout's definition in numpy (pir_ref.layout), not from the
slice entry points, which have cases of their own here.

One graph per case, single-stream and linear, replayed twice, then dropped.
The PIR kernel choice stays DPF_PIR_SPLIT: the fused launcher of the
experimental library reads a device symbol synchronously and is not
capturable (include/dpf_hip.h says so), so these cases set split for the
module whatever the environment chose."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "dpf-go_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import dpf                  # noqa: E402
from dpf import synth       # noqa: E402
import oracle               # noqa: E402
import pir_ref as ref       # noqa: E402

pytestmark = pytest.mark.gpu

POISON = 0xAB
GUARD = 64                  # poisoned bytes behind every output
FIRST = (1000, 5000)        # synth.key_seeds(first=...) of set A and of set B
LOGN, NREC = 12, 3000       # dense PIR: not a multiple of 256, below 2^12
STRIDE = 16 * ((NREC + 127) // 128)   # 3072 selection bits a key: 72 of them past nrec
TLOGN, TNK = 16, 9          # tree and Eval cases
NKEYS = (3, 70)             # 70: past the 64-key tile and the 4-key sharing
AES = ("ttable", "bitsliced")


def _bs_tree(logN, prefix_bits=0):
    """Does the byte-sliced back end, when selected, run this subtree?  Only
    from 2^6 leaf blocks per key below the prefix (bs_applicable,
    csrc/bs_kernels.hip: stop >= prefix_bits + kBsDMin + 3, stop = logN - 7);
    a shallower tree is the T-table's whatever dpf_set_aes_impl says."""
    return logN - 7 >= prefix_bits + 6


# The composites under each back end: (aes, logN, nrec).  At logN 12 the
# byte-sliced choice only changes the key expansion (both record kinds are
# built, the tree stays the T-table's), so the byte-sliced tree with its
# frontier pass runs at logN 13, over 6000 records (again no multiple of 256).
#                                 aes     logN  nrec   the tree that runs
COMPOSITE_AES = [pytest.param("ttable", LOGN, NREC, "ttable", id="ttable"),
                 pytest.param("bitsliced", 13, 6000, "bitsliced", id="bitsliced"),
                 pytest.param("bitsliced", LOGN, NREC, "ttable", id="bitsliced-expansion-only")]


def _check_tree(aes, logN, tree, prefix_bits=0):
    """The case runs the tree kernel it is named for, and cannot drop back to the other unnoticed."""
    assert ("bitsliced" if aes == "bitsliced" and _bs_tree(logN, prefix_bits) else "ttable") == tree, (aes, logN)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert dpf.gpu_init(1) >= 1
    prev = dpf.set_pir_kernel("split")
    yield
    dpf.set_pir_kernel(prev)


# ---- inputs and references, computed once and left unchanged -------------------
def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _keys(logN, nk, s, alpha_below=None):
    """The A-share keys of nk pairs of set s (alphas below alpha_below, when given)."""
    al, s0, s1 = synth.key_seeds(nk, logN, first=FIRST[s] + 7 * logN)
    if alpha_below is not None:
        al = al % np.uint64(alpha_below)
    ka, _ = dpf.gen_batch_seeded(al, logN, s0, s1)
    return _frozen(ka)


@functools.lru_cache(maxsize=None)
def _full(logN, nk, s, alpha_below=None):
    return _frozen(oracle.evalfull_batch(_keys(logN, nk, s, alpha_below), logN, nthreads=8))


@functools.lru_cache(maxsize=None)
def _rand(s, tag, *shape):
    """Random bytes of set s; `tag` keeps apart arrays of one shape."""
    return _frozen(np.random.default_rng([s, tag, *shape]).integers(0, 256, shape, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def _points(s, n, logN):
    return _frozen(np.random.default_rng([s, n, logN]).integers(0, 1 << logN, n, dtype=np.uint64))


@functools.lru_cache(maxsize=None)
def _eval_rows(logN, nk, s, npts):
    """[nk][eval_bits_stride(npts)]: Eval of every key of set s at the set's npts shared points, packed."""
    xs = np.tile(_points(s, npts, logN), (nk, 1))
    return _frozen(ref.pack_rows(oracle.eval_batch(_keys(logN, nk, s), xs, logN, nthreads=8), 16 * ((npts + 127) // 128)))


def _indices(s, nrec, n, sort):
    """n record indices of set s with a repeated one, one in the padding of
    the last super-group and one far past the DB."""
    ix = np.random.default_rng([s, nrec, n]).integers(0, nrec, n).astype(np.uint64)
    ix[3] = ix[2]
    ix[5], ix[6] = nrec + 20, 10 ** 12
    ix[7] = nrec - 1
    return _frozen(np.sort(ix, kind="stable") if sort else ix)


# ---- a case: buffers, two input sets, two expectations, the call ---------------
class Plan:
    """Device buffers allocated once; sets[s][name] is loaded into bufs[name]
    before a run of set s, want[s][name] is what bufs[name] must then hold.
    outs are pure outputs (poisoned before every run, GUARD bytes longer than
    the entry point may write); a buffer in both sets and want is changed in
    place (reset to the set's initial state before every run)."""

    def __init__(self, name):
        self.name = name
        self.bufs, self.sets, self.want = {}, ({}, {}), ({}, {})
        self.outs, self.poison = [], (POISON, POISON)
        self.work, self.run = None, None

    def _alloc(self, name, nbytes):
        import torch
        self.bufs[name] = torch.zeros(max(16, nbytes), dtype=torch.uint8, device="cuda")
        return self.bufs[name]

    def inp(self, name, a, b, want=None):
        a, b = (np.ascontiguousarray(x).reshape(-1).view(np.uint8) for x in (a, b))
        assert a.size == b.size
        self.sets[0][name], self.sets[1][name] = a, b
        if want is not None:
            for s in (0, 1):
                self.want[s][name] = np.ascontiguousarray(want[s]).reshape(-1).view(np.uint8)
                assert self.want[s][name].size == a.size
        return self._alloc(name, a.size)

    def out(self, name, wa, wb):
        wa, wb = (np.ascontiguousarray(x).reshape(-1).view(np.uint8) for x in (wa, wb))
        assert wa.size == wb.size
        self.want[0][name], self.want[1][name] = wa, wb
        self.outs.append(name)
        return self._alloc(name, wa.size + GUARD)

    def scratch(self, nbytes):
        self.work = self._alloc("work", nbytes)
        return self.work

    def load(self, s):
        import torch
        for name, a in self.sets[s].items():
            if a.size:
                self.bufs[name][:a.size].copy_(torch.from_numpy(a.copy()))
        for name in self.outs:
            self.bufs[name].fill_(self.poison[s])
        torch.cuda.synchronize()

    def check(self, s, where):
        for name, w in self.want[s].items():
            got = self.bufs[name].cpu().numpy()
            assert np.array_equal(got[:w.size], w), (self.name, where, name)
            if name in self.outs:
                assert (got[w.size:] == self.poison[s]).all(), (self.name, where, name, "bytes past the output")

    def check_untouched(self, s):
        for name in self.outs:
            assert (self.bufs[name].cpu().numpy() == self.poison[s]).all(), \
                (self.name, name, "written while the call was only being captured")
        for name in self.want[s]:
            if name in self.sets[s]:
                assert np.array_equal(self.bufs[name].cpu().numpy()[:self.sets[s][name].size], self.sets[s][name]), \
                    (self.name, name, "changed while the call was only being captured")


def _protocol(plan):
    import torch
    S = torch.cuda.Stream()
    try:
        # 2. eager on the side stream
        plan.load(0)
        plan.run(S)
        S.synchronize()
        torch.cuda.synchronize()
        plan.check(0, "eager")
        # 3. the same call(s), captured: nothing runs
        plan.load(0)
        g = torch.cuda.CUDAGraph()
        failed = ended = None
        try:
            with torch.cuda.graph(g, stream=S):
                try:
                    plan.run(torch.cuda.current_stream())
                except dpf.DPFPanic as e:
                    failed = e
        except RuntimeError as e:          # the capture itself was invalidated
            ended = e
        if failed is not None:
            pytest.fail("%s failed in a stream capture: code %d, dpf_last_error: %s" % (plan.name, failed.code, failed))
        assert ended is None, (plan.name, "the capture did not end cleanly", str(ended))
        torch.cuda.synchronize()
        plan.check_untouched(0)
        # 4. replay over new contents, and over the first ones again
        for s in (1, 0):
            plan.load(s)
            g.replay()
            torch.cuda.synchronize()
            plan.check(s, "replay over set %s" % "AB"[s])
        del g
    finally:
        if plan.work is not None:
            dpf.forget_workspace(plan.work)


def _with_settings(make, aes=None, limits=None):
    """Build the case (CPU references first), then run the protocol under an
    AES back end and / or fold limits, restoring both."""
    plan = make()
    prev = dpf.set_aes_impl(aes) if aes is not None else None
    try:
        if limits is not None:
            dpf.set_fold_limits(*limits)
        _protocol(plan)
    finally:
        dpf.set_fold_limits(0, 0)
        if prev is not None:
            dpf.set_aes_impl(prev)


# ---- tree and Eval ----------------------------------------------------------------
def _tree_plan(form):
    logN, nk = TLOGN, TNK
    kl, ol = dpf.key_len(logN), dpf.evalfull_len(logN)
    p = Plan("dpf_" + form)
    k = p.inp("keys", _keys(logN, nk, 0), _keys(logN, nk, 1))
    w = p.scratch(dpf.workspace_size(nk, logN))
    if form == "evalfull_subtree_dev":
        part = ol >> 2
        o = p.out("out", *[_full(logN, nk, s)[:, 3 * part:4 * part] for s in (0, 1)])
        p.run = lambda st: dpf.evalfull_subtree_dev(k, kl, nk, logN, 2, 3, o, w, stream=st)
        return p
    o = p.out("out", _full(logN, nk, 0), _full(logN, nk, 1))
    if form == "evalfull_batch_dev":
        p.run = lambda st: dpf.evalfull_batch_dev(k, kl, nk, logN, o, w, stream=st)
    else:
        p.name = "dpf_expand_keys_dev + dpf_evalfull_expanded_dev"

        def run(st):
            dpf.expand_keys_dev(k, kl, nk, logN, w, stream=st)
            dpf.evalfull_expanded_dev(w, nk, logN, o, stream=st)
        p.run = run
    return p


@pytest.mark.parametrize("aes", AES)
@pytest.mark.parametrize("form", ["evalfull_batch_dev", "evalfull_subtree_dev", "expand_then_expanded"])
def test_tree(form, aes):
    _check_tree(aes, TLOGN, aes, prefix_bits=2 if form == "evalfull_subtree_dev" else 0)
    _with_settings(lambda: _tree_plan(form), aes=aes)


@pytest.mark.parametrize("frontier", [True, False])
def test_eval_batch_dev(frontier):
    logN, nk, ppk = TLOGN, TNK, 64
    kl = dpf.key_len(logN)
    ws = dpf.eval_workspace_size(nk, ppk if frontier else 1, logN)   # one point per key: no frontier in the size
    assert (dpf.eval_form_for(nk, ppk, logN, ws).level > 0) == frontier

    def make():
        xs = [_points(s, nk * ppk, logN).reshape(nk, ppk) for s in (0, 1)]
        p = Plan("dpf_eval_batch_dev")
        k = p.inp("keys", _keys(logN, nk, 0), _keys(logN, nk, 1))
        x = p.inp("xs", *xs)
        o = p.out("out", *[oracle.eval_batch(_keys(logN, nk, s), xs[s], logN, nthreads=8) for s in (0, 1)])
        w = p.scratch(ws)[:ws]
        p.run = lambda st: dpf.eval_batch_dev(k, kl, nk, x, ppk, logN, o, w, stream=st)
        return p
    _with_settings(make)


@pytest.mark.parametrize("logN", [40, 16])
def test_eval_bits_dev(logN):
    nk, npts = TNK, 1000
    kl, stride = dpf.key_len(logN), dpf.eval_bits_stride(npts)
    assert stride == 128

    def make():
        p = Plan("dpf_eval_bits_dev")
        k = p.inp("keys", _keys(logN, nk, 0), _keys(logN, nk, 1))
        x = p.inp("xs", _points(0, npts, logN), _points(1, npts, logN))
        o = p.out("bits", _eval_rows(logN, nk, 0, npts), _eval_rows(logN, nk, 1, npts))
        w = p.scratch(dpf.eval_bits_workspace_size(nk, npts, logN))
        p.run = lambda st: dpf.eval_bits_dev(k, kl, nk, x, npts, logN, o, stride, w, stream=st)
        return p
    _with_settings(make)


@pytest.mark.parametrize("impl", [dpf.AES_TTABLE, dpf.AES_BITSLICED])
def test_aes_mmo_dev(impl):
    n = 1024

    def make():
        blocks = [_rand(s, 1, n, 16) for s in (0, 1)]
        want = [np.stack([np.frombuffer(oracle.mmo(True, b.tobytes(), aesni=True), np.uint8) for b in blk])
                for blk in blocks]
        p = Plan("dpf_aes_mmo_dev")
        i = p.inp("in", *blocks)
        o = p.out("out", *want)
        p.run = lambda st: dpf.aes_mmo_dev(i, o, n, impl=impl, right=True, stream=st)
        return p
    _with_settings(make)


# ---- slicing ----------------------------------------------------------------------
@pytest.mark.parametrize("form,rec", [("slice", 32), ("slice_wide", 96), ("slice_any", 20)])
def test_slice(form, rec):
    def make():
        dbs = [_rand(s, 2, NREC, rec) for s in (0, 1)]
        p = Plan("dpf_pir_db_%s_dev" % form)
        d = p.inp("db", *dbs)
        o = p.out("dbs", ref.layout(dbs[0]), ref.layout(dbs[1]))
        assert p.want[0]["dbs"].size == dpf.pir_db_sliced_size_any(NREC, rec)
        if form == "slice":
            p.run = lambda st: dpf.pir_db_slice_dev(d, NREC, o, stream=st)
        elif form == "slice_wide":
            p.run = lambda st: dpf.pir_db_slice_wide_dev(d, NREC, rec, o, stream=st)
        else:
            p.run = lambda st: dpf.pir_db_slice_any_dev(d, NREC, rec, o, stream=st)
        return p
    _with_settings(make)


GROUPED = (5, 3, 300, 20)   # ng, kpg, nrec, rec: a launch per group when slicing, one run per group when folding


def test_slice_grouped():
    ng, _, nrec, rec = GROUPED

    def make():
        dbs = [_rand(s, 3, ng, nrec, rec) for s in (0, 1)]
        p = Plan("dpf_pir_db_slice_grouped_dev")
        d = p.inp("db", *dbs)
        o = p.out("dbs", *[ref.layout(ref.grouped_flat(x)) for x in dbs])
        assert p.want[0]["dbs"].size == dpf.pir_db_grouped_size(ng, nrec, rec)
        p.run = lambda st: dpf.pir_db_slice_grouped_dev(d, ng, nrec, rec, o, stream=st)
        return p
    _with_settings(make)


# ---- folds on caller-made bits ------------------------------------------------------
def _fold_plan(form, rec, nk):
    dbs = [_rand(s, 4, NREC, rec) for s in (0, 1)]
    bits = [_rand(s, 5, nk, STRIDE) for s in (0, 1)]
    assert ref.sel_bool(bits[0], 8 * STRIDE)[:, NREC:].any()       # set past nrec too
    p = Plan("dpf_%s_dev" % form)
    b = p.inp("bits", *bits)
    d = p.inp("db", *(dbs if form == "xor_fold" else [ref.layout(x) for x in dbs]))
    a = p.out("ans", *[ref.xor_fold(bits[s], dbs[s], NREC) for s in (0, 1)])
    w = p.scratch(dpf.xor_fold_workspace_size())
    if form == "xor_fold":
        p.run = lambda st: dpf.xor_fold_dev(b, STRIDE, nk, d, NREC, rec, a, w, stream=st)
    elif form == "xor_fold_sliced":
        p.run = lambda st: dpf.xor_fold_sliced_dev(b, STRIDE, nk, d, NREC, a, w, stream=st)
    elif form == "xor_fold_sliced_wide":
        p.run = lambda st: dpf.xor_fold_sliced_wide_dev(b, STRIDE, nk, d, NREC, rec, a, w, stream=st)
    else:
        p.run = lambda st: dpf.xor_fold_sliced_any_dev(b, STRIDE, nk, d, NREC, rec, a, w, stream=st)
    return p


@pytest.mark.parametrize("limits", [(0, 0), (1, 1)])
@pytest.mark.parametrize("nk", NKEYS)
@pytest.mark.parametrize("form,rec", [("xor_fold", 32), ("xor_fold_sliced", 32), ("xor_fold_sliced_wide", 96),
                                      ("xor_fold_sliced_any", 20)])
def test_fold(form, rec, nk, limits):
    _with_settings(lambda: _fold_plan(form, rec, nk), limits=limits)


def _fold_grouped_plan(ng, kpg, nrec, rec):
    nk = ng * kpg
    stride = 16 * ((nrec + 127) // 128) + 16
    dbs = [_rand(s, 6, ng, nrec, rec) for s in (0, 1)]
    bits = [_rand(s, 7, nk, stride) for s in (0, 1)]
    p = Plan("dpf_xor_fold_grouped_dev")
    b = p.inp("bits", *bits)
    d = p.inp("dbs", *[ref.layout(ref.grouped_flat(x)) for x in dbs])
    a = p.out("ans", *[ref.grouped_expect(dbs[s], ref.sel_bool(bits[s], nrec), kpg) for s in (0, 1)])
    w = p.scratch(dpf.xor_fold_grouped_workspace_size(ng, kpg, rec))
    p.run = lambda st: dpf.xor_fold_grouped_dev(b, stride, ng, kpg, d, nrec, rec, a, w, stream=st)
    return p


def _grouped_runs(ng, rec, nrec, cus):
    """Runs a group is cut into by the grouped fold's plan, restated from
    plan_fold_grouped and grouped_want_runs (csrc/pir_group_plan.hpp, the
    builder of the fold's GroupedPlan): whole pairs of super-groups, about 8
    workgroups per CU over the ng * columns cells of a key pass."""
    gsg, cells = (nrec + 255) // 256, ng * ((rec + 31) // 32)
    want = max(1, min(gsg, -(-cus * 8 // cells)))
    per_run = (-(-gsg // want) + 1) // 2 * 2
    return -(-gsg // per_run)


# The last two are the limits of test_gpu_pir_grouped.py's
# test_answers_do_not_depend_on_the_fold_limits: several launches per key pass.
# Limits do not cut a group into runs, though: the runs come from the group's
# super-groups and the CU count.  300 records are two super-groups, one run;
# 600 are three, so two runs, the answers cleared by an earlier launch and
# every run XORed in with atomics.  With five cells that holds on any CU count
# (8 workgroups per CU are already more than one per cell), which is asserted.
@pytest.mark.parametrize("limits", [(0, 0), (1, 1), (2, 0), (7, 0)])
@pytest.mark.parametrize("nrec", [GROUPED[2], 600])
def test_fold_grouped(nrec, limits):
    import torch
    ng, kpg, _, rec = GROUPED
    for cus in (1, torch.cuda.get_device_properties(0).multi_processor_count):
        assert (_grouped_runs(ng, rec, nrec, cus) > 1) == (nrec == 600), (nrec, cus)
    _with_settings(lambda: _fold_grouped_plan(ng, kpg, nrec, rec), limits=limits)


# ---- answer composites: unpack, tree, fold ---------------------------------------------
ANSWER_FORMS = [("pir_answer", 32, False), ("pir_answer_sliced", 32, True), ("pir_answer_wide", 96, False),
                ("pir_answer_sliced_wide", 96, True), ("pir_answer_sliced_any", 20, True)]


def _answer_call(form, k, kl, nk, logN, d, nrec, rec, a, w):
    if form == "pir_answer":
        return lambda st: dpf.pir_answer_dev(k, kl, nk, logN, d, nrec, a, w, stream=st)
    if form == "pir_answer_sliced":
        return lambda st: dpf.pir_answer_sliced_dev(k, kl, nk, logN, d, nrec, a, w, stream=st)
    f = getattr(dpf, form + "_dev")
    return lambda st: f(k, kl, nk, logN, d, nrec, rec, a, w, stream=st)


def _answer_plan(form, rec, sliced, nk, logN=LOGN, nrec=NREC):
    kl = dpf.key_len(logN)
    p = Plan("dpf_%s_dev" % form)
    k = p.inp("keys", _keys(logN, nk, 0), _keys(logN, nk, 1))
    if nrec:
        dbs = [_rand(s, 8, nrec, rec) for s in (0, 1)]
        d = p.inp("db", *([ref.layout(x) for x in dbs] if sliced else dbs))
        a = p.out("ans", *[ref.xor_fold(_full(logN, nk, s), dbs[s], nrec) for s in (0, 1)])
    else:
        d = p.inp("db", np.zeros(16, np.uint8), np.zeros(16, np.uint8))
        a = p.out("ans", np.zeros((nk, rec), np.uint8), np.zeros((nk, rec), np.uint8))
        p.poison = (POISON, 0xCD)          # a clearing only: set B differs in what it must overwrite
    w = p.scratch(dpf.pir_workspace_size(nk, logN))
    p.run = _answer_call(form, k, kl, nk, logN, d, nrec, rec, a, w)
    return p


@pytest.mark.parametrize("aes,logN,nrec,tree", COMPOSITE_AES)
@pytest.mark.parametrize("nk", NKEYS)
@pytest.mark.parametrize("form,rec,sliced", ANSWER_FORMS)
def test_answer(form, rec, sliced, nk, aes, logN, nrec, tree):
    _check_tree(aes, logN, tree)
    _with_settings(lambda: _answer_plan(form, rec, sliced, nk, logN, nrec), aes=aes)


@pytest.mark.parametrize("form,rec,sliced", ANSWER_FORMS)
def test_answer_of_an_empty_db(form, rec, sliced):
    _with_settings(lambda: _answer_plan(form, rec, sliced, 3, nrec=0))


SPARSE = (40, 1000, 20)     # logN, records (= points), rec


def _sparse_plan(nk, write, nrec=SPARSE[1]):
    logN, _, rec = SPARSE
    kl = dpf.key_len(logN)
    p = Plan("dpf_pir_%s_sparse_dev" % ("write" if write else "answer"))
    k = p.inp("keys", _keys(logN, nk, 0), _keys(logN, nk, 1))
    w = p.scratch(dpf.pir_sparse_workspace_size(nk, max(nrec, 1), logN))
    if nrec == 0:
        x = p.inp("points", np.zeros(2, np.uint64), np.zeros(2, np.uint64))
        d = p.inp("dbs", np.zeros(16, np.uint8), np.zeros(16, np.uint8))
        a = p.out("ans", np.zeros((nk, rec), np.uint8), np.zeros((nk, rec), np.uint8))
        p.poison = (POISON, 0xCD)
        p.run = lambda st: dpf.pir_answer_sparse_dev(k, kl, nk, logN, x, d, 0, rec, a, w, stream=st)
        return p
    x = p.inp("points", _points(0, nrec, logN), _points(1, nrec, logN))
    dbs = [_rand(s, 9, nrec, rec) for s in (0, 1)]
    rows = [_eval_rows(logN, nk, s, nrec) for s in (0, 1)]
    if write:
        msgs = [_rand(s, 10, nk, rec) for s in (0, 1)]
        m = p.inp("msgs", *msgs)
        d = p.inp("dbs", *[ref.layout(x_) for x_ in dbs],
                  want=[ref.layout(ref.xor_scatter(dbs[s], rows[s], msgs[s], nrec)) for s in (0, 1)])
        p.run = lambda st: dpf.pir_write_sparse_dev(k, kl, nk, logN, x, m, d, nrec, rec, w, stream=st)
    else:
        d = p.inp("dbs", *[ref.layout(x_) for x_ in dbs])
        a = p.out("ans", *[ref.xor_fold(rows[s], dbs[s], nrec) for s in (0, 1)])
        p.run = lambda st: dpf.pir_answer_sparse_dev(k, kl, nk, logN, x, d, nrec, rec, a, w, stream=st)
    return p


@pytest.mark.parametrize("nk", NKEYS)
def test_answer_sparse(nk):
    _with_settings(lambda: _sparse_plan(nk, False))


def test_answer_sparse_of_an_empty_db():
    _with_settings(lambda: _sparse_plan(3, False, nrec=0))


def _answer_grouped_plan(nrec, logN=9):
    ng, kpg, full_nrec, rec = GROUPED
    nk = ng * kpg
    kl = dpf.key_len(logN)
    p = Plan("dpf_pir_answer_grouped_dev")
    k = p.inp("keys", _keys(logN, nk, 0, full_nrec), _keys(logN, nk, 1, full_nrec))
    w = p.scratch(dpf.pir_grouped_workspace_size(ng, kpg, logN, rec))
    if nrec:
        dbs = [_rand(s, 11, ng, nrec, rec) for s in (0, 1)]
        d = p.inp("dbs", *[ref.layout(ref.grouped_flat(x)) for x in dbs])
        a = p.out("ans", *[ref.grouped_expect(dbs[s], ref.sel_bool(_full(logN, nk, s, full_nrec), nrec), kpg)
                           for s in (0, 1)])
    else:
        d = p.inp("dbs", np.zeros(16, np.uint8), np.zeros(16, np.uint8))
        a = p.out("ans", np.zeros((nk, rec), np.uint8), np.zeros((nk, rec), np.uint8))
        p.poison = (POISON, 0xCD)
    p.run = lambda st: dpf.pir_answer_grouped_dev(k, kl, ng, kpg, logN, d, nrec, rec, a, w, stream=st)
    return p


# 300 records a group need a domain of 2^9; the byte-sliced tree runs from
# 2^13 (the rows' bits past the records then meet zero records only).
@pytest.mark.parametrize("aes,logN,tree", [pytest.param("ttable", 9, "ttable", id="ttable"),
                                           pytest.param("bitsliced", 13, "bitsliced", id="bitsliced"),
                                           pytest.param("bitsliced", 9, "ttable", id="bitsliced-expansion-only")])
def test_answer_grouped(aes, logN, tree):
    _check_tree(aes, logN, tree)
    _with_settings(lambda: _answer_grouped_plan(GROUPED[2], logN), aes=aes)


def test_answer_grouped_of_empty_groups():
    _with_settings(lambda: _answer_grouped_plan(0))


# ---- operations on a DB in place ----------------------------------------------------------
# A sliced buffer is compared whole with the layout's definition applied to the
# expected rows, so the padding of the last super-group is pinned to zero too.
@pytest.mark.parametrize("form,rec", [("update_sliced_wide", 96), ("update_sliced_any", 20)])
def test_update(form, rec):
    n = 40

    def make():
        dbs = [_rand(s, 12, NREC, rec) for s in (0, 1)]
        idx = [_indices(s, NREC, n, sort=True) for s in (0, 1)]
        recs = [_rand(s, 13, n, rec) for s in (0, 1)]
        p = Plan("dpf_pir_db_%s_dev" % form)
        i = p.inp("idx", *idx)
        r = p.inp("recs", *recs)
        d = p.inp("dbs", *[ref.layout(x) for x in dbs],
                  want=[ref.layout(ref.update(dbs[s], idx[s], recs[s])) for s in (0, 1)])
        f = getattr(dpf, "pir_db_%s_dev" % form)
        p.run = lambda st: f(d, NREC, rec, i, r, n, stream=st)
        return p
    _with_settings(make)


@pytest.mark.parametrize("form,rec", [("gather_sliced_wide", 96), ("gather_sliced_any", 20)])
def test_gather(form, rec):
    n = 40

    def make():
        dbs = [_rand(s, 14, NREC, rec) for s in (0, 1)]
        idx = [_indices(s, NREC, n, sort=False) for s in (0, 1)]
        p = Plan("dpf_pir_db_%s_dev" % form)
        i = p.inp("idx", *idx)
        d = p.inp("dbs", *[ref.layout(x) for x in dbs])
        o = p.out("out", *[ref.gather(dbs[s], idx[s]) for s in (0, 1)])
        f = getattr(dpf, "pir_db_%s_dev" % form)
        p.run = lambda st: f(d, NREC, rec, i, n, o, stream=st)
        return p
    _with_settings(make)


SCATTER_FORMS = [("xor_scatter", 32, False), ("xor_scatter_sliced_wide", 96, True),
                 ("xor_scatter_sliced_any", 20, True)]


def _scatter_plan(form, rec, sliced, nk):
    dbs = [_rand(s, 15, NREC, rec) for s in (0, 1)]
    bits = [_rand(s, 16, nk, STRIDE) for s in (0, 1)]
    msgs = [_rand(s, 17, nk, rec) for s in (0, 1)]
    lay = ref.layout if sliced else (lambda x: x)
    p = Plan("dpf_%s_dev" % form)
    b = p.inp("bits", *bits)
    m = p.inp("msgs", *msgs)
    d = p.inp("db", *[lay(x) for x in dbs],
              want=[lay(ref.xor_scatter(dbs[s], bits[s], msgs[s], NREC)) for s in (0, 1)])
    f = getattr(dpf, form + "_dev")
    p.run = lambda st: f(b, STRIDE, nk, m, d, NREC, rec, stream=st)
    return p


@pytest.mark.parametrize("limits", [(0, 0), (1, 1)])
@pytest.mark.parametrize("nk", NKEYS)
@pytest.mark.parametrize("form,rec,sliced", SCATTER_FORMS)
def test_scatter(form, rec, sliced, nk, limits):
    _with_settings(lambda: _scatter_plan(form, rec, sliced, nk), limits=limits)


WRITE_FORMS = [("pir_write_wide", 96, False), ("pir_write_sliced_wide", 96, True), ("pir_write_sliced_any", 20, True)]


def _write_plan(form, rec, sliced, nk, logN, nrec):
    kl = dpf.key_len(logN)
    dbs = [_rand(s, 18, nrec, rec) for s in (0, 1)]
    msgs = [_rand(s, 19, nk, rec) for s in (0, 1)]
    lay = ref.layout if sliced else (lambda x: x)
    p = Plan("dpf_%s_dev" % form)
    k = p.inp("keys", _keys(logN, nk, 0), _keys(logN, nk, 1))
    m = p.inp("msgs", *msgs)
    d = p.inp("db", *[lay(x) for x in dbs],
              want=[lay(ref.xor_scatter(dbs[s], _full(logN, nk, s), msgs[s], nrec)) for s in (0, 1)])
    w = p.scratch(dpf.pir_workspace_size(nk, logN))
    f = getattr(dpf, form + "_dev")
    p.run = lambda st: f(k, kl, nk, logN, m, d, nrec, rec, w, stream=st)
    return p


@pytest.mark.parametrize("aes,logN,nrec,tree", COMPOSITE_AES)
@pytest.mark.parametrize("nk", NKEYS)
@pytest.mark.parametrize("form,rec,sliced", WRITE_FORMS)
def test_write(form, rec, sliced, nk, aes, logN, nrec, tree):
    _check_tree(aes, logN, tree)
    _with_settings(lambda: _write_plan(form, rec, sliced, nk, logN, nrec), aes=aes)


@pytest.mark.parametrize("nk", NKEYS)
def test_write_sparse(nk):
    _with_settings(lambda: _sparse_plan(nk, True))
