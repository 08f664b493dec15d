"""Every composite entry point stays inside a d_work of exactly its size
function's bytes.  d_work is cut out of a larger 0x5A-filled buffer at a
256-byte offset, 256 guard bytes on each side: after the call the result is
the oracle's (so every part of the layout was where the launches looked for
it) and both guards are untouched (so no part reaches past the size).

Shapes: the smallest at which every part of a layout exists and its padding
matters -- 3 keys (no multiple of anything), logN 10 and 16, the whole tree and
a quarter of it, 300 records (two super-groups, the second ragged), 20-byte
and 32-byte records, 300 points of a 2^40 domain for the sparse and Eval-bits
forms; both AES back ends where a tree launch is involved.  Expected values
come from the oracle and numpy, never from the code under test."""
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
GUARD, FILL = 256, 0x5A
NK, NREC = 3, 300
SPARSE_LOGN = 40


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert dpf.gpu_init(1) >= 1


@pytest.fixture(params=[dpf.AES_TTABLE, dpf.AES_BITSLICED], ids=["ttable", "bitsliced"])
def aes(request):
    prev = dpf.set_aes_impl(request.param)
    yield request.param
    dpf.set_aes_impl(prev)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


class Work:
    """A d_work of exactly `size` bytes between two guards."""

    def __init__(self, size):
        import torch
        assert size > 0
        self.size = size
        self.whole = torch.full((GUARD + size + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.d_work = self.whole[GUARD:GUARD + size]
        assert self.d_work.data_ptr() % 256 == 0 and self.d_work.numel() == size

    def check(self):
        import torch
        torch.cuda.synchronize()
        dpf.forget_workspace(self.d_work)
        w = self.whole.cpu().numpy()
        assert (w[:GUARD] == FILL).all(), "bytes in front of d_work were written"
        assert (w[GUARD + self.size:] == FILL).all(), "bytes behind d_work's size were written"


@functools.lru_cache(maxsize=None)
def _dense(logN):
    """(keys, full): 3 keys and the oracle's EvalFull bytes of each."""
    alphas, s0, s1 = synth.key_seeds(NK, logN, first=logN)
    alphas[0] = min(NREC - 1, (1 << logN) - 1)          # one key selects inside the DB
    ka, _ = dpf.gen_batch_seeded(alphas, logN, s0, s1)
    full = oracle.evalfull_batch(ka, logN, nthreads=4)
    for a in (ka, full):
        a.setflags(write=False)
    return ka, full


def _subtree(full, pb, prefix):
    n = full.shape[1] >> pb
    return full[:, prefix * n:(prefix + 1) * n]


def _sel(full, pb, prefix, nrec):
    return np.unpackbits(_subtree(full, pb, prefix), axis=1, bitorder="little")[:, :nrec].astype(bool)


@functools.lru_cache(maxsize=None)
def _sparse():
    """(points, keys, sel): 300 points of the 2^40 domain, 3 keys (the first
    at a point of the list) and the oracle's Eval of each key at each point."""
    rng = np.random.default_rng(40)
    pts = rng.integers(0, 1 << SPARSE_LOGN, NREC, dtype=np.uint64)
    alphas, s0, s1 = synth.key_seeds(NK, SPARSE_LOGN, first=7)
    alphas[0] = pts[NREC - 1]
    ka, _ = dpf.gen_batch_seeded(alphas, SPARSE_LOGN, s0, s1)
    sel = oracle.eval_batch(ka, np.tile(pts, (NK, 1)), SPARSE_LOGN, nthreads=4).astype(bool)
    assert sel[0, NREC - 1]
    for a in (pts, ka, sel):
        a.setflags(write=False)
    return pts, ka, sel


def _db(nrec, rec):
    return np.random.default_rng(nrec * 7 + rec).integers(0, 256, (nrec, rec), dtype=np.uint8)


def _msgs(rec):
    return np.random.default_rng(rec).integers(0, 256, (NK, rec), dtype=np.uint8)


def _xor_rows(db, sel):
    out = np.zeros((sel.shape[0], db.shape[1]), np.uint8)
    for k in range(sel.shape[0]):
        if sel[k].any():
            out[k] = np.bitwise_xor.reduce(db[sel[k]], axis=0)
    return out


def _apply(db, sel, msgs):
    out = db.copy()
    for k in range(sel.shape[0]):
        out[sel[k]] ^= msgs[k]
    return out


def _sliced(db):
    import torch
    nrec, rec = db.shape
    dbs = torch.zeros(dpf.pir_db_sliced_size_any(nrec, rec), dtype=torch.uint8, device="cuda")
    dpf.pir_db_slice_any_dev(_dev(db), nrec, rec, dbs)
    return dbs


def _rows(dbs, nrec, rec):
    import torch
    out = torch.empty(nrec * rec, dtype=torch.uint8, device="cuda")
    dpf.pir_db_gather_sliced_any_dev(dbs, nrec, rec, torch.arange(nrec, dtype=torch.int64, device="cuda"), nrec, out)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(nrec, rec)


def _nrec(logN, pb):
    return min(NREC, 1 << (logN - pb))


SUBTREES = [(0, 0), (2, 3)]


@pytest.mark.parametrize("pb,prefix", SUBTREES)
@pytest.mark.parametrize("logN", [10, 16])
def test_evalfull_subtree_dev(logN, pb, prefix, aes):
    import torch
    keys, full = _dense(logN)
    want = _subtree(full, pb, prefix)
    w = Work(dpf.workspace_size(NK, logN))
    d_out = torch.zeros(want.size, dtype=torch.uint8, device="cuda")
    dpf.evalfull_subtree_dev(_dev(keys), keys.shape[1], NK, logN, pb, prefix, d_out, w.d_work)
    w.check()
    assert np.array_equal(d_out.cpu().numpy().reshape(want.shape), want)


@pytest.mark.parametrize("rec", [20, 32])
@pytest.mark.parametrize("pb,prefix", SUBTREES)
@pytest.mark.parametrize("logN", [10, 16])
def test_pir_answer_sliced_any_dev(logN, pb, prefix, rec, aes):
    import torch
    keys, full = _dense(logN)
    nrec = _nrec(logN, pb)
    db = _db(nrec, rec)
    w = Work(dpf.pir_workspace_size(NK, logN, pb))
    d_ans = torch.full((NK * rec,), 0x33, dtype=torch.uint8, device="cuda")
    dpf.pir_answer_sliced_any_dev(_dev(keys), keys.shape[1], NK, logN, _sliced(db), nrec, rec, d_ans, w.d_work,
                                  prefix_bits=pb, prefix=prefix)
    w.check()
    assert np.array_equal(d_ans.cpu().numpy().reshape(NK, rec), _xor_rows(db, _sel(full, pb, prefix, nrec)))


@pytest.mark.parametrize("pb,prefix", SUBTREES)
@pytest.mark.parametrize("logN", [10, 16])
def test_pir_answer_wide_dev(logN, pb, prefix, aes):
    import torch
    rec = 32
    keys, full = _dense(logN)
    nrec = _nrec(logN, pb)
    db = _db(nrec, rec)
    w = Work(dpf.pir_workspace_size(NK, logN, pb))
    d_ans = torch.full((NK * rec,), 0x33, dtype=torch.uint8, device="cuda")
    dpf.pir_answer_wide_dev(_dev(keys), keys.shape[1], NK, logN, _dev(db), nrec, rec, d_ans, w.d_work,
                            prefix_bits=pb, prefix=prefix)
    w.check()
    assert np.array_equal(d_ans.cpu().numpy().reshape(NK, rec), _xor_rows(db, _sel(full, pb, prefix, nrec)))


@pytest.mark.parametrize("rec", [20, 32])
@pytest.mark.parametrize("pb,prefix", SUBTREES)
@pytest.mark.parametrize("logN", [10, 16])
def test_pir_write_sliced_any_dev(logN, pb, prefix, rec, aes):
    keys, full = _dense(logN)
    nrec = _nrec(logN, pb)
    db, msgs = _db(nrec, rec), _msgs(rec)
    dbs = _sliced(db)
    w = Work(dpf.pir_workspace_size(NK, logN, pb))
    dpf.pir_write_sliced_any_dev(_dev(keys), keys.shape[1], NK, logN, _dev(msgs), dbs, nrec, rec, w.d_work,
                                 prefix_bits=pb, prefix=prefix)
    w.check()
    assert np.array_equal(_rows(dbs, nrec, rec), _apply(db, _sel(full, pb, prefix, nrec), msgs))


@pytest.mark.parametrize("rec", [20, 32])
def test_pir_answer_sparse_dev(rec):
    import torch
    pts, keys, sel = _sparse()
    db = _db(NREC, rec)
    w = Work(dpf.pir_sparse_workspace_size(NK, NREC, SPARSE_LOGN))
    d_ans = torch.full((NK * rec,), 0x33, dtype=torch.uint8, device="cuda")
    dpf.pir_answer_sparse_dev(_dev(keys), keys.shape[1], NK, SPARSE_LOGN, _dev(pts), _sliced(db), NREC, rec, d_ans,
                              w.d_work)
    w.check()
    assert np.array_equal(d_ans.cpu().numpy().reshape(NK, rec), _xor_rows(db, sel))


@pytest.mark.parametrize("rec", [20, 32])
def test_pir_write_sparse_dev(rec):
    pts, keys, sel = _sparse()
    db, msgs = _db(NREC, rec), _msgs(rec)
    dbs = _sliced(db)
    w = Work(dpf.pir_sparse_workspace_size(NK, NREC, SPARSE_LOGN))
    dpf.pir_write_sparse_dev(_dev(keys), keys.shape[1], NK, SPARSE_LOGN, _dev(pts), _dev(msgs), dbs, NREC, rec,
                             w.d_work)
    w.check()
    assert np.array_equal(_rows(dbs, NREC, rec), _apply(db, sel, msgs))


def test_eval_bits_dev():
    import torch
    pts, keys, sel = _sparse()
    stride = dpf.eval_bits_stride(NREC)
    w = Work(dpf.eval_bits_workspace_size(NK, NREC, SPARSE_LOGN))
    d_bits = torch.zeros(NK * stride, dtype=torch.uint8, device="cuda")
    dpf.eval_bits_dev(_dev(keys), keys.shape[1], NK, _dev(pts), NREC, SPARSE_LOGN, d_bits, stride, w.d_work)
    w.check()
    got = np.unpackbits(d_bits.cpu().numpy().reshape(NK, stride), axis=1, bitorder="little")[:, :NREC].astype(bool)
    assert np.array_equal(got, sel)


@pytest.mark.parametrize("logN", [10, 16, SPARSE_LOGN])
def test_eval_batch_dev(logN):
    import torch
    if logN == SPARSE_LOGN:
        pts, keys, sel = _sparse()
        xs, want = np.tile(pts, (NK, 1)), sel.astype(np.uint8)
    else:
        keys, full = _dense(logN)
        xs = np.random.default_rng(logN).integers(0, 1 << logN, (NK, NREC), dtype=np.uint64)
        bits = np.unpackbits(full, axis=1, bitorder="little")
        want = np.take_along_axis(bits, xs.astype(np.int64), axis=1)
    w = Work(dpf.eval_workspace_size(NK, NREC, logN))
    d_out = torch.full((NK * NREC,), 0x33, dtype=torch.uint8, device="cuda")
    dpf.eval_batch_dev(_dev(keys), keys.shape[1], NK, _dev(xs), NREC, logN, d_out, w.d_work)
    w.check()
    assert np.array_equal(d_out.cpu().numpy().reshape(NK, NREC), want)
