"""GPU parity on deep domains (logN 33..63): subtrees of deep keys through the
tree kernels, batched Eval of points with non-zero high words, and PIR answers
and private writes on a deep subtree.  A full EvalFull above logN 32 fits
nowhere, so the expected bytes of a subtree (prefix_bits, prefix) are the
CPU oracle's EvalFull of the key re-rooted at that subtree (oracle.reroot_key,
cross-checked against point evaluation in tests/test_deep_domains_cpu.py), and
the expected Eval bits are oracle.eval_batch.  Everything is bit-exact and
nothing comes from the code under test.

Workspaces: dpf_workspace_size(nkeys, logN) counts a byte-sliced frontier for
the whole tree and cannot be allocated at these depths; a subtree call needs
dpf_pir_workspace_size(nkeys, logN, prefix_bits) at the most (include/dpf_hip.h),
which is what the tests here pass."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import dpf
from dpf import synth
import oracle

pytestmark = pytest.mark.gpu

NT = 16
GUARD = 256


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert dpf.gpu_init(1) >= 1


def _dev(a):
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    if not a.flags.writeable:             # a shared, frozen reference: torch wants a writable source
        a = a.copy()
    return torch.from_numpy(a.view(np.uint8)).cuda()


def _filled(nbytes, fill):
    """nbytes of `fill` on the device, and GUARD more behind them."""
    import torch
    return torch.full((nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")


def _read(buf, nbytes, fill):
    """The first nbytes of a _filled buffer; the guard behind them is untouched."""
    got = buf.cpu().numpy()
    assert (got[nbytes:] == fill).all(), "bytes written past the output"
    return got[:nbytes]


def _work(nk, logN, pb):
    import torch
    return torch.empty(dpf.pir_workspace_size(nk, logN, pb), dtype=torch.uint8, device="cuda")


def _keys_under(nk, logN, pb, prefix, first, low0=None):
    """nk key pairs whose alphas all lie in subtree (pb, prefix); key 0's
    position in the subtree is low0 when given."""
    al, s0, s1 = synth.key_seeds(nk, logN, first=first)
    low = logN - pb
    al = al & np.uint64((1 << low) - 1)
    if low0 is not None:
        al[0] = low0
    al = al | np.uint64(prefix << low)
    ka, kb = dpf.gen_batch_seeded(al, logN, s0, s1)
    return al, ka, kb


def _subtree_want(keys, logN, pb, prefix):
    """uint8[nk][2^(logN - pb - 3)]: EvalFull of every key re-rooted at (pb, prefix)."""
    rk = np.stack([np.frombuffer(oracle.reroot_key(k.tobytes(), logN, pb, prefix), np.uint8) for k in keys])
    return oracle.evalfull_batch(rk, logN - pb, nthreads=NT)


def _prefix_classes(own, pb):
    """The subtree of the alphas, its sibling, the first and the last subtree,
    and past 32 bits one with bits 31 and 32 set below its top bit."""
    ps = [own, own ^ 1, 0, (1 << pb) - 1]
    if pb > 32:
        ps.append((1 << (pb - 1)) | (3 << 31) | 0x5A5)
    return list(dict.fromkeys(ps))


def _own_prefix(logN, pb, first):
    """A prefix of pb bits from the synthetic stream, bits 31 and 32 set where it has them."""
    al, _, _ = synth.key_seeds(1, logN, first=first)
    own = int(al[0]) >> (logN - pb)
    if pb > 32:
        own |= 3 << 31
    return own


# ---- A. every walk form of the tree kernel at ltop >= 33 ---------------------
_DEPTH_CHILD = r'''
import sys
sys.path[:0] = [%r, %r]
import numpy as np, torch, dpf, oracle
from dpf import synth
assert dpf.gpu_init(1) >= 1
LOGN, STOP = 63, 56
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
def keys_under(nk, pb, prefix, first):
    al, s0, s1 = synth.key_seeds(nk, LOGN, first=first)
    low = LOGN - pb
    al = (al & np.uint64((1 << low) - 1)) | np.uint64(prefix << low)
    return (al,) + tuple(dpf.gen_batch_seeded(al, LOGN, s0, s1))
def want(keys, pb, prefix):
    rk = np.stack([np.frombuffer(oracle.reroot_key(k.tobytes(), LOGN, pb, prefix), np.uint8) for k in keys])
    return oracle.evalfull_batch(rk, LOGN - pb, nthreads=8)
def subtree(keys, pb, own, what):
    nk, kl = keys.shape
    n = 16 << (STOP - pb)
    d_keys = dev(keys)
    d_work = torch.empty(dpf.pir_workspace_size(nk, LOGN, pb), dtype=torch.uint8, device="cuda")
    for prefix in (own, (1 << pb) - 1):
        w = want(keys, pb, prefix)
        for expanded, fill in ((False, 0x5A), (True, 0xA5)):
            d_out = torch.full((nk * n + 256,), fill, dtype=torch.uint8, device="cuda")
            if expanded:
                dpf.expand_keys_dev(d_keys, kl, nk, LOGN, d_work)
                dpf.evalfull_expanded_dev(d_work, nk, LOGN, d_out, prefix_bits=pb, prefix=prefix)
            else:
                dpf.evalfull_subtree_dev(d_keys, kl, nk, LOGN, pb, prefix, d_out, d_work)
            torch.cuda.synchronize()
            got = d_out.cpu().numpy()
            assert (got[nk * n:] == fill).all(), (what, "guard")
            assert np.array_equal(got[:nk * n].reshape(nk, n), w), (what, hex(prefix), expanded)
    dpf.forget_workspace(d_work)
own39 = (int(synth.key_seeds(1, LOGN, first=6300)[0][0]) >> 24) | (3 << 31)
_, ka, kb = keys_under(1, 39, own39, 6300)
for k in (ka, kb):
    subtree(k, 39, own39, "1 key, prefix_bits 39")
own47 = (1 << 46) | (3 << 31) | 0x2B5
al, ka, kb = keys_under(70, 47, own47, 6370)
xs = synth.eval_points(70, 256, LOGN)
xs[:, 0] = al
xs[:, 1] = al ^ np.uint64(1 << 40)
for k in (ka, kb):
    subtree(k, 47, own47, "70 keys, prefix_bits 47")
    out = np.full((70, 256), 0x5A, np.uint8)
    dpf.eval_batch(k, xs, LOGN, ngpus=1, out=out)
    assert np.array_equal(out, oracle.eval_batch(k, xs, LOGN, nthreads=8)), "eval"
dpf.gpu_shutdown()
print("done")
'''


@pytest.mark.parametrize("raw", [None, "0"], ids=["raw", "expanded"])
@pytest.mark.parametrize("depth", [0, 1, 2, 3, 4, 7])
def test_every_walk_form_above_32_levels(depth, raw):
    """test_gpu_parity.py::test_every_subtree_depth's shapes moved to the bottom
    of a logN 63 tree (stop 56): the per-thread subtree depth D forced by
    DPF_SUBTREE_DEPTH, from raw key bytes and (DPF_RAW_KEYS=0) from expanded
    records, a fresh child per case (both switches are read once per process).
    Both shares, the subtree of the alphas and the last subtree (prefix 2^pb - 1),
    through dpf_evalfull_subtree_dev and dpf_expand_keys_dev +
    dpf_evalfull_expanded_dev, every byte against the re-rooted keys' EvalFull.
    The threads per launch, and with them the forms of k_evalfull on a 256-CU
    device, are those of that test's table; the path bits now come from a
    64-bit sub = (prefix << units_log) + local shifted by up to 55:

      1 key, prefix_bits 39 (2^17 leaf blocks below the prefix; the prefix has bits 31, 32 and 38 set)
        D   threads  workgroup  ltop  walk
        0   131072   512        56    LDS CWs; quad of lanes per path to level 53, 3 levels per thread
        1    65536   256        55    LDS CWs; quad of lanes per path to level 53, 2 levels per thread
        2    32768   128        54    LDS CWs; one lane per path to level 53, 1 level per thread
        3+   16384..1024  64    53..49  LDS CWs; no shared walk: the tail walk over all ltop levels
      70 keys, prefix_bits 47 (2^9 leaf blocks; one prefix for all, bits 31, 32 and 46 set)
        0    35840   256        56    two workgroups per key: LDS CWs, quad walk to level 54
        1    17920   128        55    LDS CWs, one lane per path to level 54
        2, 3  8960, 4480  64    54, 53  wave-uniform keys, one wave per workgroup: LDS CWs, tail walk
        4, 7  2240, 280   64    52, 49  32, 4 threads per key: the per-lane-key walk, CWs from expanded records
      Eval, 70 keys x 256 points, logN 63: node pass to level 7 (depth min(D, 7)),
        then the persistent walk over 49 levels from the staged 64-bit points;
        every key's alpha and alpha ^ 2^40 are among its points."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DPF_SUBTREE_DEPTH=str(depth))
    env.pop("DPF_RAW_KEYS", None)
    if raw is not None:
        env["DPF_RAW_KEYS"] = raw
    code = _DEPTH_CHILD % (os.path.join(root, "dpf-go_amd"), os.path.join(root, "oracle"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.strip().endswith("done")


# ---- B. the shapes the launcher picks itself, both AES back ends ---------------
def _run_subtrees(keys, logN, pb, prefixes, want, where):
    """Every prefix through dpf_evalfull_subtree_dev and through
    dpf_expand_keys_dev + dpf_evalfull_expanded_dev against want[prefix]."""
    import torch
    nk, kl = keys.shape
    n = 16 << (logN - 7 - pb)
    d_keys, d_work = _dev(keys), _work(nk, logN, pb)
    for prefix in prefixes:
        for expanded, fill in ((False, 0x5A), (True, 0xA5)):
            d_out = _filled(nk * n, fill)
            if expanded:
                dpf.expand_keys_dev(d_keys, kl, nk, logN, d_work)
                dpf.evalfull_expanded_dev(d_work, nk, logN, d_out, prefix_bits=pb, prefix=prefix)
            else:
                dpf.evalfull_subtree_dev(d_keys, kl, nk, logN, pb, prefix, d_out, d_work)
            torch.cuda.synchronize()
            got = _read(d_out, nk * n, fill).reshape(nk, n)
            assert np.array_equal(got, want[prefix]), where + (hex(prefix), "expanded" if expanded else "subtree")
    dpf.forget_workspace(d_work)


def _both_back_ends(run):
    prev = dpf.get_aes_impl()
    try:
        for aes in ("ttable", "bitsliced"):
            dpf.set_aes_impl(aes)
            run(aes)
    finally:
        dpf.set_aes_impl(prev)


@pytest.mark.parametrize("span", [0, 5, 6, 7, 10])
@pytest.mark.parametrize("nk", [1, 3, 70])
@pytest.mark.parametrize("logN", [33, 40, 48, 63])
def test_deep_subtrees_both_back_ends(logN, nk, span):
    """Subtrees of 2^span leaf blocks at the bottom of a deep tree, prefix_bits
    = stop - span, in the shapes pick_shape chooses.  span 0: one thread per
    key walks all stop levels; 5 | 6: the byte-sliced back end starts to apply
    (bs_applicable); 6 | 7: its depth model changes (bs_depth).  The alphas of
    all keys share one prefix: under it the shares XOR to the point function,
    under every other prefix to zero."""
    pb = logN - 7 - span
    own = _own_prefix(logN, pb, first=logN * 100 + span)
    al, ka, kb = _keys_under(nk, logN, pb, own, first=logN * 1000 + nk * 10 + span)
    prefixes = _prefix_classes(own, pb)
    want = {s: {p: _subtree_want(k, logN, pb, p) for p in prefixes} for s, k in (("a", ka), ("b", kb))}
    for p in prefixes:
        x = np.unpackbits(want["a"][p] ^ want["b"][p], axis=1, bitorder="little")
        if p == own:
            assert (x.sum(axis=1) == 1).all()
            assert all(x[k, int(al[k]) & ((1 << (span + 7)) - 1)] == 1 for k in range(nk))
        else:
            assert not x.any()

    def run(aes):
        for s, k in (("a", ka), ("b", kb)):
            _run_subtrees(k, logN, pb, prefixes, want[s], (aes, s))
    _both_back_ends(run)


def test_workgroups_of_several_keys_walk_55_levels():
    """The one walk form the shapes above leave out: wave-uniform keys in a
    workgroup that holds more than one key, so the correction words come from
    the key bytes (or the expanded records) in global memory, not from LDS.
    600 keys x 2^9 leaf blocks under a 47-bit prefix of logN 63: on a 256-CU
    device pick_shape takes D = 1, 256 threads per key in 512-thread
    workgroups, ltop = 55.  Whatever shape a device picks, the bytes are the
    re-rooted keys' EvalFull."""
    logN, nk, pb = 63, 600, 47
    own = (1 << 46) | (3 << 31) | 0x1C3
    _, ka, _ = _keys_under(nk, logN, pb, own, first=66000)
    prefixes = [own, (1 << pb) - 1]
    want = {p: _subtree_want(ka, logN, pb, p) for p in prefixes}
    _both_back_ends(lambda aes: _run_subtrees(ka, logN, pb, prefixes, want, (aes,)))


@pytest.mark.parametrize("logN", [33, 40, 48, 63])
def test_deep_subtrees_of_arbitrary_key_bytes(logN):
    """Keys of random bytes: byte-valued t values (tested != 0, XORed as
    bytes) carried down up to 49 levels to a subtree of 2^7 leaf blocks, and
    down all stop levels to a single one."""
    rng = np.random.default_rng(logN)
    keys = rng.integers(0, 256, (3, dpf.key_len(logN)), dtype=np.uint8)
    keys[0, 16] = 0
    keys[1, 16] = 0xFE
    for span in (7, 0):
        pb = logN - 7 - span
        prefixes = _prefix_classes(_own_prefix(logN, pb, first=77 + logN), pb)
        want = {p: _subtree_want(keys, logN, pb, p) for p in prefixes}
        _both_back_ends(lambda aes: _run_subtrees(keys, logN, pb, prefixes, want, (aes, span)))


# ---- C. batched Eval with real 64-bit points -----------------------------------
NSPECIAL = 12


def _points(al, logN, ppk):
    """[nk][ppk] points: each key's alpha, alpha ^ 1, ^ 127, ^ 128, ^ 2^31,
    ^ 2^32, ^ 2^(logN-1), 0, 2^logN - 1, a duplicate pair, two points with bits
    above logN set (alpha itself with bit logN, and a point with all of them),
    the rest uniform over the domain; each row then rotated by its own amount,
    so that the special points are not all in a wave's first lanes."""
    nk = al.size
    mask = np.uint64((1 << logN) - 1)
    xs = synth.eval_points(nk, ppk, logN, master=0xD0E5 + logN)
    a = al.astype(np.uint64)

    def special():
        for j, flip in enumerate((0, 1, 127, 128, 1 << 31, 1 << 32, 1 << (logN - 1))):
            xs[:, j] = a ^ np.uint64(flip)
        xs[:, 7] = 0
        xs[:, 8] = mask
        xs[:, 9] = xs[:, 20]                          # the duplicate pair
        xs[:, 10] = a | np.uint64(1 << logN)          # logN < 64: ignored bits (dpf.go:194)
        xs[:, 11] = xs[:, 21] | ~mask
    special()
    # x -> x ^ 2^32 maps the domain onto itself, so the rest stay uniform:
    # rows that drew too few high words (logN 33: one bit decides) are mirrored.
    few = ((xs >> np.uint64(32)) != 0).sum(axis=1) * 2 < ppk
    xs[few, NSPECIAL:] ^= np.uint64(1 << 32)
    special()
    for k in range(nk):
        xs[k] = np.roll(xs[k], 37 * k)
    return xs


@functools.lru_cache(maxsize=None)
def _eval_case(logN, nk, ppk):
    """(alphas, ka, kb, xs, expected bits of ka, of kb), computed once per shape."""
    al, s0, s1 = synth.key_seeds(nk, logN, first=9000 + logN + ppk)
    ka, kb = dpf.gen_batch_seeded(al, logN, s0, s1)
    xs = _points(al, logN, ppk)
    assert (((xs >> np.uint64(32)) != 0).sum(axis=1) * 2 >= ppk).all()      # real 64-bit points
    wa = oracle.eval_batch(ka, xs, logN, nthreads=NT)
    wb = oracle.eval_batch(kb, xs, logN, nthreads=NT)
    hit = (xs & np.uint64((1 << logN) - 1)) == al[:, None]
    assert hit.sum(axis=1).min() >= 2                                        # alpha, and alpha with bit logN
    assert np.array_equal(wa ^ wb, hit.astype(np.uint8))
    for a in (al, ka, kb, xs, wa, wb):
        a.setflags(write=False)
    return al, ka, kb, xs, wa, wb


def _eval_dev(keys, xs, logN, work_bytes, offset8=False):
    """dpf_eval_batch_dev with a workspace of work_bytes; offset8 puts d_xs at
    an address that is 8 but not 16 bytes aligned."""
    import torch
    nk, ppk = xs.shape
    d_keys = _dev(keys)
    d_big = torch.zeros(nk * ppk + 2, dtype=torch.int64, device="cuda")
    o = 1 if offset8 else 0
    d_big[o:o + nk * ppk] = torch.from_numpy(xs.reshape(-1).view(np.int64).copy()).cuda()
    d_xs = d_big[o:o + nk * ppk]
    assert d_xs.data_ptr() % 16 == (8 if offset8 else 0)
    d_work = torch.empty(work_bytes, dtype=torch.uint8, device="cuda")
    d_out = _filled(nk * ppk, 0xA5)
    dpf.eval_batch_dev(d_keys, keys.shape[1], nk, d_xs, ppk, logN, d_out, d_work)
    torch.cuda.synchronize()
    return _read(d_out, nk * ppk, 0xA5).reshape(nk, ppk)


PERSIST = [(33, 16, 128), (48, 4, 512), (63, 16, 128), (63, 2, 1024)]


@pytest.mark.parametrize("route", ["host", "dev"])
@pytest.mark.parametrize("logN,nk,ppk", PERSIST)
def test_persistent_eval_rebuilds_64_bit_points(logN, nk, ppk, route):
    """k_eval_persist (2048 queries, points per key a multiple of 128, a
    16-byte-aligned xs, a frontier) puts each point together from the two
    halves its LDS-DMA staged: points with non-zero high words, both shares,
    through dpf_eval_batch and through dpf_eval_batch_dev with
    dpf_eval_workspace_size bytes."""
    assert nk * ppk >= 2048 and ppk % 128 == 0 and dpf.eval_frontier_level(logN, ppk) > 0
    _, ka, kb, xs, wa, wb = _eval_case(logN, nk, ppk)
    for keys, want in ((ka, wa), (kb, wb)):
        if route == "host":
            out = np.full((nk, ppk), 0x5A, np.uint8)
            got = dpf.eval_batch(keys, xs, logN, ngpus=1, out=out)
        else:
            got = _eval_dev(keys, xs, logN, dpf.eval_workspace_size(nk, ppk, logN))
        assert np.array_equal(got, want)


def test_pair_eval_with_uniform_keys_and_64_bit_points():
    """k_eval2<true>: the persistent shape with d_xs only 8-byte aligned."""
    logN, nk, ppk = 63, 16, 128
    _, ka, kb, xs, wa, wb = _eval_case(logN, nk, ppk)
    for keys, want in ((ka, wa), (kb, wb)):
        got = _eval_dev(keys, xs, logN, dpf.eval_workspace_size(nk, ppk, logN), offset8=True)
        assert np.array_equal(got, want)


def test_root_walks_with_64_bit_points():
    """A workspace of the expanded keys alone leaves no room for a frontier:
    every query walks its 41 levels from the root.  (dpf_workspace_size(16, 48)
    itself is 68 TiB: it counts a byte-sliced frontier of the whole tree.)"""
    logN, nk, ppk = 48, 16, 128
    _, ka, kb, xs, wa, wb = _eval_case(logN, nk, ppk)
    records = dpf.eval_workspace_size(nk, 1, logN)                 # one point per key: no frontier in the size
    assert records == (nk * (logN - 7 + 2) * 32 + 255) // 256 * 256 < dpf.eval_workspace_size(nk, ppk, logN)
    for keys, want in ((ka, wa), (kb, wb)):
        assert np.array_equal(_eval_dev(keys, xs, logN, records), want)


# ---- D. PIR answers and private writes on a deep subtree -----------------------
PIR_SHAPES = [(40, 28), (63, 50)]


@functools.lru_cache(maxsize=None)
def _pir_case(logN, pb, nk):
    """nk key pairs with their alphas under one prefix (bits 31 and 32 set
    where it has them), key 0's at the slice's last record; and the selection
    bits bool[nk][2^span] of both shares under that prefix and its sibling."""
    span = logN - pb
    own = (1 << (pb - 1)) | ((3 << 31) if pb > 32 else 0) | 0xABCDE
    al, ka, kb = _keys_under(nk, logN, pb, own, first=logN * 100 + nk, low0=(1 << span) - 1)
    sel = {}
    for prefix in (own, own ^ 1):
        for side, keys in (("a", ka), ("b", kb)):
            full = _subtree_want(keys, logN, pb, prefix)
            sel[prefix, side] = np.unpackbits(full, axis=1, bitorder="little").astype(bool)
            sel[prefix, side].setflags(write=False)
    return al, ka, kb, own, sel


def _fold(sel, db):
    """XOR of the DB rows each key selects: [nk][rec]."""
    out = np.zeros((sel.shape[0], db.shape[1]), np.uint8)
    for k in range(sel.shape[0]):
        rows = db[sel[k]]
        if rows.shape[0]:
            out[k] = np.bitwise_xor.reduce(rows, axis=0)
    return out


def _scatter(db, sel, msgs):
    out = db.copy()
    for k in range(sel.shape[0]):
        out[sel[k]] ^= msgs[k]
    return out


class _Server:
    """One (nrec, rec) DB on the device, row-major and sliced, and the calls on it."""

    def __init__(self, db, keys, logN, pb):
        import torch
        self.nrec, self.rec = db.shape
        self.logN, self.pb = logN, pb
        self.nk, self.kl = keys.shape
        self.d_keys = _dev(keys)
        self.d_db = _dev(db)
        self.size = dpf.pir_db_sliced_size_wide(self.nrec, self.rec)
        self.d_dbs = _filled(self.size, 0x5A)
        dpf.pir_db_slice_wide_dev(self.d_db, self.nrec, self.rec, self.d_dbs)
        self.d_work = _work(self.nk, logN, pb)
        self.d_all = _dev(np.arange(self.nrec, dtype=np.uint64))
        torch.cuda.synchronize()

    def answers(self, prefix):
        """{entry point: its answers [nk][rec]}"""
        import torch
        a = (self.d_keys, self.kl, self.nk, self.logN)
        kw = dict(prefix_bits=self.pb, prefix=prefix)
        calls = {"wide": lambda o: dpf.pir_answer_wide_dev(*a, self.d_db, self.nrec, self.rec, o, self.d_work, **kw),
                 "sliced_wide": lambda o: dpf.pir_answer_sliced_wide_dev(*a, self.d_dbs, self.nrec, self.rec, o,
                                                                         self.d_work, **kw)}
        if self.rec == 32:
            d32 = torch.full((dpf.pir_db_sliced_size(self.nrec),), 0xA5, dtype=torch.uint8, device="cuda")
            dpf.pir_db_slice_dev(self.d_db, self.nrec, d32)
            calls["32"] = lambda o: dpf.pir_answer_dev(*a, self.d_db, self.nrec, o, self.d_work, **kw)
            calls["sliced_32"] = lambda o: dpf.pir_answer_sliced_dev(*a, d32, self.nrec, o, self.d_work, **kw)
        got = {}
        for name, call in calls.items():
            d_ans = _filled(self.nk * self.rec, 0xA5)
            call(d_ans)
            torch.cuda.synchronize()
            got[name] = _read(d_ans, self.nk * self.rec, 0xA5).reshape(self.nk, self.rec)
        return got

    def writes(self, prefix, msgs):
        """{entry point: the whole DB after the write, row-major}; the DBs of this object stay as they were."""
        import torch
        a = (self.d_keys, self.kl, self.nk, self.logN, _dev(msgs))
        kw = dict(prefix_bits=self.pb, prefix=prefix)
        n = self.nrec * self.rec
        rows = _filled(n, 0x5A)
        rows[:n] = self.d_db
        dpf.pir_write_wide_dev(*a, rows, self.nrec, self.rec, self.d_work, **kw)
        sl = self.d_dbs.clone()
        dpf.pir_write_sliced_wide_dev(*a, sl, self.nrec, self.rec, self.d_work, **kw)
        d_out = _filled(n, 0xA5)
        dpf.pir_db_gather_sliced_wide_dev(sl, self.nrec, self.rec, self.d_all, self.nrec, d_out)
        torch.cuda.synchronize()
        _read(sl, self.size, 0x5A)
        return {"wide": _read(rows, n, 0x5A).reshape(self.nrec, self.rec),
                "sliced_wide": _read(d_out, n, 0xA5).reshape(self.nrec, self.rec)}

    def close(self):
        dpf.forget_workspace(self.d_work)


@pytest.mark.parametrize("aes,nk", [("ttable", 1), ("ttable", 5), ("bitsliced", 5), ("ttable", 33), ("ttable", 70)])
@pytest.mark.parametrize("logN,pb", PIR_SHAPES)
def test_pir_on_a_deep_subtree(logN, pb, nk, aes):
    """Slice = subtree (prefix_bits, prefix) of a deep key: 2^12 records under
    a 28-bit prefix of logN 40, 2^13 under a 50-bit prefix of logN 63, whole
    and 77 records short, 32- and 96-byte records; 1 key (the one-key fold),
    5 and 33 (the first two key tiles), 70 (the second scatter key tile).
    Every answer entry against the numpy fold of the re-rooted keys' bits with
    the DB, every write entry against db ^ scatter of the same bits, both
    shares, under the alphas' prefix and its sibling.  Two servers: under the
    alphas' prefix the answers XOR to record alpha - (prefix << span) (zero
    past nrec: key 0's alpha is the slice's last record) and the writes change
    the XOR of the DBs there only; under the sibling nothing shows."""
    al, ka, kb, own, sel = _pir_case(logN, pb, nk)
    span = logN - pb
    n = 1 << span
    prev = dpf.set_aes_impl(aes)
    try:
        for nrec in (n, n - 77):
            for rec in (32, 96):
                rng = np.random.default_rng(logN * 1000 + nk * 10 + rec + nrec)
                db = rng.integers(0, 256, (nrec, rec), dtype=np.uint8)
                msgs = rng.integers(0, 256, (nk, rec), dtype=np.uint8)
                msgs[0] = 0xFF
                servers = {"a": _Server(db, ka, logN, pb), "b": _Server(db, kb, logN, pb)}
                for prefix in (own, own ^ 1):
                    ans, wr = {}, {}
                    for side, srv in servers.items():
                        where = (logN, pb, nk, aes, nrec, rec, hex(prefix), side)
                        s = sel[prefix, side][:, :nrec]
                        ans[side], wr[side] = _fold(s, db), _scatter(db, s, msgs)
                        got = srv.answers(prefix)
                        assert len(got) == (4 if rec == 32 else 2)
                        for name, g in got.items():
                            assert np.array_equal(g, ans[side]), where + ("answer", name)
                        for name, g in srv.writes(prefix, msgs).items():
                            assert np.array_equal(g, wr[side]), where + ("write", name)
                    x, delta = ans["a"] ^ ans["b"], np.zeros_like(db)
                    for k in range(nk):
                        loc = int(al[k]) - (prefix << span)
                        here = prefix == own and loc < nrec
                        assert prefix != own or 0 <= loc < n
                        assert np.array_equal(x[k], db[loc] if here else np.zeros(rec, np.uint8)), (prefix == own, k)
                        if here:
                            delta[loc] ^= msgs[k]
                    assert np.array_equal(wr["a"] ^ wr["b"], delta)
                for srv in servers.values():
                    srv.close()
    finally:
        dpf.set_aes_impl(prev)
