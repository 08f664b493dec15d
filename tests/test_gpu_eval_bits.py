"""dpf_eval_bits_dev: every key evaluated at one shared list of points, the
answers as packed selection-bit rows in EvalFull's bit order.  Every test
compares the whole written span of every row with the CPU oracle
(oracle.eval_batch over the tiled points, packed LSB-first and zero-extended
to the span), never with the code under test; keys are both shares of seeded
Gen, and the XOR of the two shares' rows is checked to be one-hot at the
positions where xs[j] == alpha."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "dpf-go_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import dpf                  # noqa: E402
from dpf import synth       # noqa: E402
import oracle               # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xA5
EXTRA = 32           # two units of slack in bits_stride
XS_OFF = 248         # the points start 8-byte, not 16-byte, aligned inside a poisoned tensor


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert dpf.gpu_init(1) >= 1


@functools.lru_cache(maxsize=None)
def _keys(nk, logN, first):
    """nk key pairs -> (alphas, both shares [2 nk][klen]: A shares then B shares)."""
    al, s0, s1 = synth.key_seeds(nk, logN, first=first)
    ka, kb = dpf.gen_batch_seeded(al, logN, s0, s1)
    keys = np.concatenate([ka, kb])
    keys.setflags(write=False)
    return al, keys


def _expect(keys, xs, logN):
    """Rows of dpf_eval_bits_stride(npts) bytes from the oracle."""
    nk, npts = keys.shape[0], xs.size
    bits = oracle.eval_batch(keys, np.tile(xs, (nk, 1)), logN, nthreads=8)
    rows = np.packbits(bits, axis=1, bitorder="little")
    out = np.zeros((nk, 16 * ((npts + 127) // 128)), np.uint8)
    out[:, :rows.shape[1]] = rows
    return out


def _run(keys, xs, logN, work_bytes=None, stream=None, extra=EXTRA):
    """eval_bits_dev into rows `extra` bytes wider than needed, pre-filled with
    FILL; the points sit in exactly npts * 8 bytes of a larger tensor whose
    other bytes are 0xEE.  Returns the whole buffer [nk][stride]."""
    import torch
    nk, npts = keys.shape[0], xs.size
    stride = dpf.eval_bits_stride(npts) + extra
    assert dpf.eval_bits_stride(npts) == 16 * ((npts + 127) // 128)
    pool = torch.full((XS_OFF + npts * 8 + 4096,), 0xEE, dtype=torch.uint8, device="cuda")
    d_xs = pool[XS_OFF:XS_OFF + npts * 8]
    d_xs.copy_(torch.from_numpy(np.ascontiguousarray(xs, np.uint64).view(np.uint8).copy()))
    d_keys = torch.from_numpy(np.array(keys).reshape(-1)).cuda()
    if work_bytes is None:
        work_bytes = dpf.eval_bits_workspace_size(nk, npts, logN)
    d_work = torch.empty(work_bytes, dtype=torch.uint8, device="cuda")
    d_bits = torch.full((nk * stride,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dpf.eval_bits_dev(d_keys, keys.shape[1], nk, d_xs, npts, logN, d_bits, stride, d_work, stream=stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    dpf.forget_workspace(d_work)
    assert bool((pool[:XS_OFF] == 0xEE).all()) and bool((pool[XS_OFF + npts * 8:] == 0xEE).all())
    return d_bits.cpu().numpy().reshape(nk, stride)


def _check(got, want, npts):
    """The span equals the oracle's rows (so bits >= npts of it are zero), and
    the bytes past the span are untouched."""
    span = want.shape[1]
    assert np.array_equal(got[:, :span], want)
    ub = np.unpackbits(got[:, :span], axis=1, bitorder="little")
    assert not ub[:, npts:].any()
    assert (got[:, span:] == FILL).all()


def _one_hot(rows, alphas, xs, logN):
    """XOR of the two shares' rows: bit j set exactly where xs[j] == alpha
    (path bits above logN are not part of the domain point)."""
    nk = alphas.size
    x = np.unpackbits(rows[:nk] ^ rows[nk:], axis=1, bitorder="little")[:, :xs.size]
    mask = np.uint64((1 << logN) - 1)
    hit = (xs & mask)[None, :] == alphas.astype(np.uint64)[:, None]
    assert np.array_equal(x.astype(bool), hit)


def _points(rng, npts, logN, alphas=()):
    hi = 1 << logN
    xs = rng.integers(0, hi, npts, dtype=np.uint64)
    special = [0, hi - 1]
    for a in alphas:
        a = int(a)
        special += [a, a ^ 1, (a ^ 128) % hi, a]            # alpha twice: a repeated point
    if logN == 63:
        special += [(1 << 63) | int(alphas[0]), (1 << 63) | 5, (1 << 64) - 1] if len(alphas) else [(1 << 63) | 5]
    at = rng.choice(npts, size=min(len(special), npts), replace=False)
    for i, p in zip(at, special):
        xs[i] = np.uint64(p)
    return xs


# ---- tail matrix ---------------------------------------------------------------
@pytest.mark.parametrize("nk", [1, 3, 65])
@pytest.mark.parametrize("npts", [1, 63, 64, 65, 127, 128, 129, 257, 1000])
def test_tail_matrix(npts, nk):
    """Every tail shape at logN 20: the span matches the oracle, its bits at
    positions >= npts are zero, bytes past the span keep their 0xA5, and no
    read leaves the npts * 8 bytes of the points."""
    logN = 20
    pairs = (nk + 1) // 2
    al, both = _keys(pairs, logN, 100 + nk)
    keys = np.empty_like(both)
    keys[0::2], keys[1::2] = both[:pairs], both[pairs:]         # A0 B0 A1 B1 ...: the first nk of them
    keys = keys[:nk]
    rng = np.random.default_rng(npts * 1000 + nk)
    xs = _points(rng, npts, logN, al[:2])
    got = _run(keys, xs, logN)
    want = _expect(keys, xs, logN)
    _check(got, want, npts)
    whole = nk // 2                                             # pairs with both shares in the batch
    if whole:
        span = got[:2 * whole, :want.shape[1]]
        _one_hot(np.concatenate([span[0::2], span[1::2]]), al[:whole], xs, logN)


# ---- depth ---------------------------------------------------------------------
@pytest.mark.parametrize("logN", [7, 8, 13, 33, 40, 63])
def test_depth(logN):
    """stop 0 to 56 at 300 points: uniformly random points plus 0, 2^logN - 1,
    alpha, alpha ^ 1, alpha ^ 128, alpha again, and at logN 63 points with bit
    63 set.  The third key's alpha is left out of the list: its shares' rows
    cancel."""
    npts, nk = 300, 3
    al, keys = _keys(nk, logN, 7000 + logN)
    rng = np.random.default_rng(logN)
    xs = _points(rng, npts, logN, al[:2])
    got = _run(keys, xs, logN)
    want = _expect(keys, xs, logN)
    _check(got, want, npts)
    _one_hot(got[:, :want.shape[1]], al, xs, logN)
    if logN >= 33:
        assert int(al[2]) not in set(int(x) & ((1 << logN) - 1) for x in xs)
        assert not (got[2, :want.shape[1]] ^ got[5, :want.shape[1]]).any()


# ---- routes --------------------------------------------------------------------
def test_frontier_and_root_walk_routes_agree():
    """logN 24, 4133 points: with the full workspace the points share a
    frontier at level L >= 4, with the expanded keys alone every walk starts
    at the root.  Each route matches the oracle on the whole span and the two
    agree byte for byte.  (The plan keeps no persistent form, so there is no
    second kernel threshold to straddle; eval_bits_plan.hpp.)"""
    logN, nk, npts = 24, 3, 4096 + 37
    al, keys = _keys(nk, logN, 31)
    xs = _points(np.random.default_rng(24), npts, logN, al)
    assert dpf.eval_frontier_level(logN, npts) >= 4
    full = dpf.eval_bits_workspace_size(2 * nk, npts, logN)
    records = dpf.eval_workspace_size(2 * nk, 1, logN)          # one point per key: no frontier in the size
    assert records == (2 * nk * (logN - 7 + 2) * 32 + 255) // 256 * 256 < full
    want = _expect(keys, xs, logN)
    a = _run(keys, xs, logN, work_bytes=full)
    b = _run(keys, xs, logN, work_bytes=records)
    _check(a, want, npts)
    _check(b, want, npts)
    assert np.array_equal(a, b)
    _one_hot(a[:, :want.shape[1]], al, xs, logN)


# ---- consistency -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _consistency_case():
    logN, nk, npts = 20, 5, 1000
    al, keys = _keys(nk, logN, 555)
    xs = _points(np.random.default_rng(5), npts, logN, al)
    xs.setflags(write=False)
    want = _expect(keys, xs, logN)
    want.setflags(write=False)
    return logN, al, keys, xs, want


def test_equals_packed_eval_batch_dev():
    """The rows are eval_batch_dev's bytes over per-key tiled points, packed."""
    import torch
    logN, al, keys, xs, want = _consistency_case()
    nk, npts = keys.shape[0], xs.size
    d_keys = torch.from_numpy(np.array(keys).reshape(-1)).cuda()
    d_xs = torch.from_numpy(np.tile(xs, (nk, 1)).view(np.int64).copy()).cuda()
    d_out = torch.empty(nk * npts, dtype=torch.uint8, device="cuda")
    d_work = torch.empty(dpf.eval_workspace_size(nk, npts, logN), dtype=torch.uint8, device="cuda")
    dpf.eval_batch_dev(d_keys, keys.shape[1], nk, d_xs, npts, logN, d_out, d_work)
    torch.cuda.synchronize()
    dpf.forget_workspace(d_work)
    packed = np.packbits(d_out.cpu().numpy().reshape(nk, npts), axis=1, bitorder="little")
    got = _run(keys, xs, logN)
    assert np.array_equal(got[:, :packed.shape[1]], packed)
    _check(got, want, npts)


def test_same_rows_under_the_bitsliced_back_end():
    logN, al, keys, xs, want = _consistency_case()
    prev = dpf.set_aes_impl("bitsliced")
    try:
        got = _run(keys, xs, logN)
    finally:
        dpf.set_aes_impl(prev)
    _check(got, want, xs.size)


def test_same_rows_on_a_four_cu_stream():
    logN, al, keys, xs, want = _consistency_case()
    st = dpf.stream_create_cu_masked(0, 4)
    try:
        got = _run(keys, xs, logN, stream=st)
    finally:
        dpf.stream_destroy(st)
    _check(got, want, xs.size)


def test_rows_feed_the_fold_and_the_scatter():
    """Rows of the minimal stride are d_bits input, with nrec = npts, of the
    sliced fold and scatter: the fold's answers are the numpy XOR of the
    selected records, and the scatter's DB is the numpy dual."""
    import torch
    logN, al, keys, xs, want = _consistency_case()
    nk, npts, rec = keys.shape[0], xs.size, 20
    got = _run(keys, xs, logN, extra=0)
    sel = np.unpackbits(want, axis=1, bitorder="little")[:, :npts].astype(bool)
    rng = np.random.default_rng(99)
    db = rng.integers(0, 256, (npts, rec), dtype=np.uint8)
    d_bits = torch.from_numpy(got.reshape(-1).copy()).cuda()
    d_dbs = torch.zeros(dpf.pir_db_sliced_size_any(npts, rec), dtype=torch.uint8, device="cuda")
    dpf.pir_db_slice_any_dev(torch.from_numpy(db.reshape(-1)).cuda(), npts, rec, d_dbs)
    d_ans = torch.empty(nk * rec, dtype=torch.uint8, device="cuda")
    d_work = torch.empty(dpf.xor_fold_workspace_size(), dtype=torch.uint8, device="cuda")
    dpf.xor_fold_sliced_any_dev(d_bits, got.shape[1], nk, d_dbs, npts, rec, d_ans, d_work)
    torch.cuda.synchronize()
    exp = np.stack([np.bitwise_xor.reduce(db[sel[k]], axis=0) if sel[k].any() else np.zeros(rec, np.uint8)
                    for k in range(nk)])
    assert np.array_equal(d_ans.cpu().numpy().reshape(nk, rec), exp)
    msgs = rng.integers(0, 256, (nk, rec), dtype=np.uint8)
    dpf.xor_scatter_sliced_any_dev(d_bits, got.shape[1], nk, torch.from_numpy(msgs.reshape(-1)).cuda(), d_dbs, npts, rec)
    d_idx = torch.arange(npts, dtype=torch.int64, device="cuda")
    d_rows = torch.empty(npts * rec, dtype=torch.uint8, device="cuda")
    dpf.pir_db_gather_sliced_any_dev(d_dbs, npts, rec, d_idx, npts, d_rows)
    torch.cuda.synchronize()
    after = db.copy()
    for k in range(nk):
        after[sel[k]] ^= msgs[k]
    assert np.array_equal(d_rows.cpu().numpy().reshape(npts, rec), after)
