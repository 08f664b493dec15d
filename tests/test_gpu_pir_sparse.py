"""PIR over a sparse key set: record j lives at domain point points[j]
(dpf_pir_answer_sparse_dev, dpf_pir_write_sparse_dev and the handle made by
dpf_pir_db_create_sparse).  Expected selections come from oracle.eval_batch at
the records' points, expected answers and DBs from numpy; never from the code
under test.  Both servers' shares are run: their answers XOR to the record at
the queried keyword and to zero for an absent keyword.  Everything is
bit-exact.

The two-shard handle needs a process of its own (the device registry is
process-wide): the test at the end runs this file as a script."""
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
GUARD = 256


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert dpf.gpu_init(1) >= 1


def _dev(a):
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


def _xor_rows(db, sel):
    """[nkeys][rec]: XOR of the rows of db that sel[k] (bool [nrec]) selects."""
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


@functools.lru_cache(maxsize=None)
def _case(nrec, nk, logN):
    """(points, alphas, ka, kb, selA, selB): nrec points of the 2^logN domain
    (the second repeats the first from 3 records on; bit 63 plays no part),
    nk key pairs whose even ones query a keyword of the list and whose odd
    ones an absent one, and the oracle's selections of both shares."""
    rng = np.random.default_rng(nrec * 977 + nk * 31 + logN)
    hi = 1 << logN
    pts = rng.integers(0, hi, nrec, dtype=np.uint64)
    if nrec >= 3:
        pts[1] = pts[0]
    if nrec >= 5:
        pts[nrec - 1], pts[nrec // 2] = np.uint64(hi - 1), np.uint64(0)
    have = set(int(p) for p in pts)
    alphas = np.zeros(nk, np.uint64)
    for k in range(nk):
        if k % 2 == 0:
            alphas[k] = pts[(k // 2 * 131) % nrec] if k else pts[0]
        else:
            a = int(rng.integers(0, hi, dtype=np.uint64))
            while a in have:
                a = int(rng.integers(0, hi, dtype=np.uint64))
            alphas[k] = a
    _, s0, s1 = synth.key_seeds(nk, logN, first=nrec + logN)
    ka, kb = dpf.gen_batch_seeded(alphas, logN, s0, s1)
    tiled = np.tile(pts, (nk, 1))
    selA = oracle.eval_batch(ka, tiled, logN, nthreads=8).astype(bool)
    selB = oracle.eval_batch(kb, tiled, logN, nthreads=8).astype(bool)
    assert np.array_equal(selA ^ selB, pts[None, :] == alphas[:, None])
    for a in (pts, alphas, ka, kb, selA, selB):
        a.setflags(write=False)
    return pts, alphas, ka, kb, selA, selB


def _db(nrec, rec):
    return np.random.default_rng(nrec * 7 + rec).integers(0, 256, (nrec, rec), dtype=np.uint8)


def _sliced(db):
    """The any-width sliced layout of db, GUARD bytes of 0x5A behind it."""
    import torch
    nrec, rec = db.shape
    size = dpf.pir_db_sliced_size_any(nrec, rec)
    buf = torch.full((size + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    dpf.pir_db_slice_any_dev(_dev(db), nrec, rec, buf)
    torch.cuda.synchronize()
    return buf, size


NREC = [1, 255, 256, 257, 1000]
REC = [4, 20, 32, 100]
NK = [1, 5, 65]


@pytest.mark.parametrize("logN", [30, 63])
@pytest.mark.parametrize("nk", NK)
@pytest.mark.parametrize("rec", REC)
@pytest.mark.parametrize("nrec", NREC)
def test_answer_sparse_dev(nrec, rec, nk, logN):
    import torch
    pts, alphas, ka, kb, selA, selB = _case(nrec, nk, logN)
    db = _db(nrec, rec)
    dbs, size = _sliced(db)
    d_pts = _dev(pts)
    d_work = torch.empty(dpf.pir_sparse_workspace_size(nk, nrec, logN), dtype=torch.uint8, device="cuda")
    got = []
    for keys, sel in ((ka, selA), (kb, selB)):
        d_ans = torch.full((nk * rec + GUARD,), 0x33, dtype=torch.uint8, device="cuda")
        dpf.pir_answer_sparse_dev(_dev(keys), keys.shape[1], nk, logN, d_pts, dbs, nrec, rec, d_ans, d_work)
        torch.cuda.synchronize()
        a = d_ans.cpu().numpy()
        assert (a[nk * rec:] == 0x33).all()
        got.append(a[:nk * rec].reshape(nk, rec))
        assert np.array_equal(got[-1], _xor_rows(db, sel))
    dpf.forget_workspace(d_work)
    # Two servers: the record(s) at the queried keyword, zero for an absent one.
    assert np.array_equal(got[0] ^ got[1], _xor_rows(db, pts[None, :] == alphas[:, None]))
    assert not (got[0] ^ got[1])[1::2].any()
    if nrec < 3:
        assert np.array_equal((got[0] ^ got[1])[0], db[0])
    assert (dbs.cpu().numpy()[size:] == 0x5A).all()


@pytest.mark.parametrize("logN", [30, 63])
@pytest.mark.parametrize("nk", [1, 65])
@pytest.mark.parametrize("rec", [4, 20, 100])
@pytest.mark.parametrize("nrec", [1, 255, 257, 1000])
def test_write_sparse_dev(nrec, rec, nk, logN):
    """The DB after the write, read back with the gather, is the numpy dual;
    its raw sliced bytes are those of slicing the expected DB, so the padding
    of the last super-group stays zero."""
    import torch
    pts, alphas, ka, kb, selA, selB = _case(nrec, nk, logN)
    db = _db(nrec, rec)
    msgs = np.random.default_rng(nk + rec).integers(0, 256, (nk, rec), dtype=np.uint8)
    msgs[0] = 0xFF
    dbs, size = _sliced(db)
    d_work = torch.empty(dpf.pir_sparse_workspace_size(nk, nrec, logN), dtype=torch.uint8, device="cuda")
    dpf.pir_write_sparse_dev(_dev(ka), ka.shape[1], nk, logN, _dev(pts), _dev(msgs), dbs, nrec, rec, d_work)
    want = _apply(db, selA, msgs)
    d_idx = torch.arange(nrec, dtype=torch.int64, device="cuda")
    d_rows = torch.empty(nrec * rec, dtype=torch.uint8, device="cuda")
    dpf.pir_db_gather_sliced_any_dev(dbs, nrec, rec, d_idx, nrec, d_rows)
    torch.cuda.synchronize()
    assert np.array_equal(d_rows.cpu().numpy().reshape(nrec, rec), want)
    ref, _ = _sliced(want)
    assert torch.equal(dbs, ref)
    # The other server's share: the two DBs now differ at the keywords only.
    dpf.pir_write_sparse_dev(_dev(kb), kb.shape[1], nk, logN, _dev(pts), _dev(msgs), dbs, nrec, rec, d_work)
    torch.cuda.synchronize()
    dpf.forget_workspace(d_work)
    ref, _ = _sliced(_apply(db, pts[None, :] == alphas[:, None], msgs))
    assert torch.equal(dbs, ref)


def _handle_checks(rec, ngpus=1):
    """A sparse PirDB of 1000 records at logN 40: answer, write, answer again,
    update and read by position."""
    logN, nrec, nk = 40, 1000, 12
    pts, alphas, ka, kb, selA, selB = _case(nrec, nk, logN)
    db = _db(nrec, rec)
    pdb = dpf.PirDB(db, logN, ngpus=ngpus, rec_bytes=rec, points=pts)
    assert pdb.nrec == nrec and pdb.rec_bytes == rec
    everything = np.arange(nrec, dtype=np.uint64)
    assert np.array_equal(pdb.read(everything), db)
    a, b = pdb.answer(ka), pdb.answer(kb)
    assert np.array_equal(a, _xor_rows(db, selA)) and np.array_equal(b, _xor_rows(db, selB))
    hit = pts[None, :] == alphas[:, None]
    assert np.array_equal(a ^ b, _xor_rows(db, hit)) and not (a ^ b)[1::2].any()
    assert np.array_equal((a ^ b)[0], db[0] ^ db[1])            # a repeated point: both records together
    msgs = np.random.default_rng(rec).integers(0, 256, (nk, rec), dtype=np.uint8)
    pdb.write(ka, msgs)
    want = _apply(db, selA, msgs)
    assert np.array_equal(pdb.read(everything), want)
    assert np.array_equal(pdb.answer(kb), _xor_rows(want, selB))
    idx = np.array([0, 511, 512, 999, 3, 512], np.uint64)       # any order, both sides of a shard edge, one twice
    recs = np.random.default_rng(rec + 1).integers(0, 256, (idx.size, rec), dtype=np.uint8)
    pdb.update(idx, recs)
    for i, r in zip(idx, recs):
        want[int(i)] = r                                        # of repeated indices the last wins
    assert np.array_equal(pdb.read(idx), want[idx.astype(np.int64)])
    assert np.array_equal(pdb.read(everything), want)
    assert np.array_equal(pdb.answer(ka), _xor_rows(want, selA))
    with pytest.raises(dpf.DPFPanic) as e:
        pdb.update(np.array([nrec], np.uint64), recs[:1])
    assert e.value.code == dpf.DPF_ERR_PARAM
    with pytest.raises(dpf.DPFPanic) as e:
        pdb.answer(ka[:, :16 + 18 * (logN - 7)])
    assert e.value.code == dpf.DPF_ERR_KEYLEN
    pdb.close()
    assert pdb.nrec == 0


@pytest.mark.parametrize("rec", [7, 32])
def test_sparse_handle(rec):
    _handle_checks(rec)


def test_sparse_handle_refuses_points_outside_the_domain():
    logN = 20
    db = _db(4, 32)
    for bad in (1 << logN, (1 << 63) | 5):
        with pytest.raises(dpf.DPFPanic) as e:
            dpf.PirDB(db, logN, rec_bytes=32, points=np.array([1, 2, bad, 3], np.uint64))
        assert e.value.code == dpf.DPF_ERR_PARAM
    with pytest.raises(ValueError):
        dpf.PirDB(db, logN, rec_bytes=32, points=np.array([1, 2, 3], np.uint64))
    with pytest.raises(dpf.DPFPanic):
        dpf.PirDB(db, logN, ngpus=dpf.gpu_count() + 1, rec_bytes=32, points=np.array([1, 2, 3, 4], np.uint64))
    empty = dpf.PirDB(np.zeros((0, 32), np.uint8), logN, rec_bytes=32, points=np.zeros(0, np.uint64))
    al, s0, s1 = synth.key_seeds(3, logN, first=4)
    ka, _ = dpf.gen_batch_seeded(al, logN, s0, s1)
    assert not empty.answer(ka).any()
    empty.close()


def test_dense_handle_on_the_same_records_answers_as_before():
    """A dense PirDB over the records of a sparse one: record i at index i."""
    logN, nrec, rec = 10, 1000, 32
    db = _db(nrec, rec)
    al, s0, s1 = synth.key_seeds(9, logN, first=77)
    ka, kb = dpf.gen_batch_seeded(al, logN, s0, s1)
    dense = dpf.PirDB(db, logN, rec_bytes=rec)
    sparse = dpf.PirDB(db, logN, rec_bytes=rec, points=np.arange(nrec, dtype=np.uint64))
    for keys in (ka, kb):
        sel = np.unpackbits(oracle.evalfull_batch(keys, logN), axis=1, bitorder="little")[:, :nrec].astype(bool)
        want = _xor_rows(db, sel)
        assert np.array_equal(dense.answer(keys), want)
        assert np.array_equal(sparse.answer(keys), want)
    dense.close()
    sparse.close()


def test_two_shard_sparse_handle():
    """gpu_init_devices([0, 0]) and PirDB(..., ngpus=2, points=): shards of
    512 and 488 records, each with its points; answers are XORed on the host."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "two-shards"], capture_output=True, text=True,
                       timeout=240, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith("done")


if __name__ == "__main__":
    dpf.gpu_init_devices([0, 0])
    _handle_checks(7, ngpus=2)
    _handle_checks(32, ngpus=2)
    dpf.gpu_shutdown()
    print("done")
