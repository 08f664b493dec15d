"""GPU parity of the sliced kernels over records of any width (a multiple of 4
bytes; every width through the handle): the layout dbs[S][p][g]
(include/dpf_hip.h), the fold, PIR answer, update, gather, scatter and private
write over it, and PirDB.  Expected values come from the layout's definition
and from numpy XOR folds of the CPU oracle's EvalFull bits or of random bits,
never from the code under test.

Widths: 4 (one tile), 12 and 20 (odd tile counts: one wave gets a real and an
absent tile), 16, 28 (seven tiles), 36 (a full column plus one tile), 48, and
100 / 132 / 260 (4, 5 and 9 columns with a short last one: CG = 4, 1, 1)."""
import functools

import numpy as np
import pytest

import dpf
from dpf import synth
import oracle

pytestmark = pytest.mark.gpu

W = (4, 12, 16, 20, 28, 36, 48, 100, 132, 260)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert dpf.gpu_init(1) >= 1


@pytest.fixture
def fold_limits():
    yield dpf.set_fold_limits
    dpf.set_fold_limits(0, 0)


def _layout(db: np.ndarray) -> np.ndarray:
    """The sliced layout of a row-major (nrec, rec_bytes) DB from its
    definition: u32 dbs[S][p][g], bit j = bit p (bit p%8 of byte p/8) of record
    256 S + 32 g + j; records past nrec are 0."""
    nrec, rec = db.shape
    nsg = (nrec + 255) // 256
    pad = np.zeros((nsg * 256, rec), np.uint8)
    pad[:nrec] = db
    b = np.unpackbits(pad, axis=1, bitorder="little")          # [record][p]
    b = b.reshape(nsg, 8, 32, 8 * rec)                          # [S][g][j][p]
    b = b.transpose(0, 3, 1, 2)                                 # [S][p][g][j]
    return np.packbits(np.ascontiguousarray(b).reshape(-1), bitorder="little")   # LE u32 = 4 bytes of j


def _want(sel: np.ndarray, db: np.ndarray, nrec: int) -> np.ndarray:
    """XOR of the rows i < nrec of db whose bit i (LSB-first) of a selection row is set."""
    bits = np.unpackbits(sel, axis=1, bitorder="little")[:, :nrec].astype(np.float64)
    dbb = np.unpackbits(db[:nrec], axis=1, bitorder="little").astype(np.float64)
    par = (bits @ dbb).astype(np.int64) & 1                     # counts <= nrec: exact
    return np.packbits(par.astype(np.uint8), axis=1, bitorder="little")


@functools.lru_cache(maxsize=None)
def _db(nrec, rec):
    d = synth.db_bytes(max(nrec, 1) * rec, master=synth.MASTER_SEED + 2 + rec).reshape(-1, rec)[:nrec]
    d.setflags(write=False)
    return d


def _dev(a):
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    if a.size == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a.copy()).cuda()


def _slice(db, nrec, rec):
    import torch
    size = dpf.pir_db_sliced_size_any(nrec, rec)
    assert size == max(16, (nrec + 255) // 256 * 256 * rec)
    d_dbs = torch.full((size,), 0x5A, dtype=torch.uint8, device="cuda")     # exactly the layout's size
    dpf.pir_db_slice_any_dev(_dev(db), nrec, rec, d_dbs)
    torch.cuda.synchronize()
    return d_dbs


def _fold(d_bits, stride, nk, d_dbs, nrec, rec):
    """The answers, after checking that nothing past nk * rec bytes was written."""
    import torch
    tail = 64
    d_ans = torch.full((nk * rec + tail,), 0xAB, dtype=torch.uint8, device="cuda")
    d_work = torch.empty(dpf.xor_fold_workspace_size(), dtype=torch.uint8, device="cuda")
    dpf.xor_fold_sliced_any_dev(d_bits, stride, nk, d_dbs, nrec, rec, d_ans, d_work)
    torch.cuda.synchronize()
    a = d_ans.cpu().numpy()
    assert np.all(a[nk * rec:] == 0xAB), "bytes past the answers were written"
    return a[:nk * rec].reshape(nk, rec)


def _keys(nk, logN, nrec, first):
    """nk key pairs whose alphas lie below nrec."""
    al, s0, s1 = synth.key_seeds(nk, logN, first=first)
    al = al % np.uint64(nrec)
    ka, kb = dpf.gen_batch_seeded(al, logN, s0, s1)
    return al, ka, kb


# ---- layout -------------------------------------------------------------------
@pytest.mark.parametrize("nrec", [1, 255, 257, 1000])
def test_slice_any_is_the_documented_layout(nrec):
    for rec in W:
        db = _db(nrec, rec)
        got = _slice(db, nrec, rec).cpu().numpy()
        want = _layout(db)
        assert got.size == want.size == (nrec + 255) // 256 * 256 * rec, rec
        assert np.array_equal(got, want), rec


def test_slice_any_in_chunks_of_whole_super_groups():
    import torch
    nrec = 1000
    for rec in W:
        db = _db(nrec, rec)
        d = torch.full((dpf.pir_db_sliced_size_any(nrec, rec),), 0x5A, dtype=torch.uint8, device="cuda")
        dpf.pir_db_slice_any_dev(_dev(db[:512]), 512, rec, d)
        dpf.pir_db_slice_any_dev(_dev(db[512:]), nrec - 512, rec, d[512 * rec:])
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy(), _layout(db)), rec


def test_any_layout_is_the_wide_layout_at_multiples_of_32():
    nrec = 300
    for rec in (32, 64, 96):
        db = _db(nrec, rec)
        got = _slice(db, nrec, rec).cpu().numpy()
        assert np.array_equal(got, _layout(db))
        import torch
        d = torch.full((dpf.pir_db_sliced_size_wide(nrec, rec),), 0x5A, dtype=torch.uint8, device="cuda")
        dpf.pir_db_slice_wide_dev(_dev(db), nrec, rec, d)
        torch.cuda.synchronize()
        assert np.array_equal(got, d.cpu().numpy())


# ---- fold ---------------------------------------------------------------------
# nkeys: the one-key kernel, every kFoldTiles row (<= 32, <= 64, <= 128, <= 256
# keys at the widths' CG = 4 / 1) and a second key group.
@pytest.mark.parametrize("nk", [1, 2, 33, 65, 129, 300])
@pytest.mark.parametrize("nrec", [1, 257, 1000])
def test_fold_any_matches_numpy(nrec, nk):
    rng = np.random.default_rng(nrec * 1000 + nk)
    stride = ((nrec + 7) // 8 + 15) // 16 * 16
    bits = rng.integers(0, 256, (nk, stride), dtype=np.uint8)
    d_bits = _dev(bits)
    for rec in W:
        db = _db(nrec, rec)
        got = _fold(d_bits, stride, nk, _slice(db, nrec, rec), nrec, rec)
        assert np.array_equal(got, _want(bits, db, nrec)), rec


@pytest.mark.parametrize("rec", [20, 100])
def test_fold_any_in_forced_passes(fold_limits, rec):
    nrec = 5000
    stride = ((nrec + 7) // 8 + 15) // 16 * 16
    db = _db(nrec, rec)
    d_dbs = _slice(db, nrec, rec)
    for nk in (1, 40):
        bits = np.random.default_rng(rec + nk).integers(0, 256, (nk, stride), dtype=np.uint8)
        fold_limits(3, 2)
        got = _fold(_dev(bits), stride, nk, d_dbs, nrec, rec)
        fold_limits(0, 0)
        assert np.array_equal(got, _want(bits, db, nrec)), nk


# ---- PIR answer -----------------------------------------------------------------
@pytest.mark.parametrize("rec", [20, 100])
def test_pir_answer_any(rec):
    import torch
    logN, nrec, nk = 12, 3000, 5
    al, ka, kb = _keys(nk, logN, nrec, first=900 + rec)
    db = _db(nrec, rec)
    d_dbs = _slice(db, nrec, rec)
    kl = dpf.key_len(logN)
    d_work = torch.empty(dpf.pir_workspace_size(nk, logN), dtype=torch.uint8, device="cuda")
    shares = []
    for keys in (ka, kb):
        d_ans = torch.full((nk * rec + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        dpf.pir_answer_sliced_any_dev(_dev(keys), kl, nk, logN, d_dbs, nrec, rec, d_ans, d_work)
        torch.cuda.synchronize()
        a = d_ans.cpu().numpy()
        assert np.all(a[nk * rec:] == 0xAB)
        a = a[:nk * rec].reshape(nk, rec)
        assert np.array_equal(a, _want(oracle.evalfull_batch(keys, logN, nthreads=4), db, nrec))
        shares.append(a)
    x = shares[0] ^ shares[1]
    for k in range(nk):
        assert np.array_equal(x[k], db[int(al[k])])


def test_pir_answer_any_on_a_subtree():
    import torch
    logN, pb, prefix, nk, rec, nrec = 12, 2, 3, 5, 20, 1000
    _, ka, _ = _keys(nk, logN, 1 << logN, first=77)
    full = oracle.evalfull_batch(ka, logN, nthreads=4)
    q = full.shape[1] // 4
    quarter = np.ascontiguousarray(full[:, prefix * q:(prefix + 1) * q])
    db = _db(nrec, rec)
    d_work = torch.empty(dpf.pir_workspace_size(nk, logN, pb), dtype=torch.uint8, device="cuda")
    d_ans = torch.full((nk * rec,), 0xAB, dtype=torch.uint8, device="cuda")
    dpf.pir_answer_sliced_any_dev(_dev(ka), dpf.key_len(logN), nk, logN, _slice(db, nrec, rec), nrec, rec, d_ans, d_work,
                                  prefix_bits=pb, prefix=prefix)
    torch.cuda.synchronize()
    assert np.array_equal(d_ans.cpu().numpy().reshape(nk, rec), _want(quarter, db, nrec))


# ---- update and gather ------------------------------------------------------------
@pytest.mark.parametrize("rec", [12, 36, 100])
def test_update_and_gather_any(rec):
    import torch
    nrec = 1000
    rng = np.random.default_rng(rec)
    db = _db(nrec, rec).copy()
    d_dbs = _slice(db, nrec, rec)
    # Sorted: sparse ones with repeats, a dense run of 70 consecutive records
    # across a super-group boundary, and one index past nrec.
    idx = np.concatenate([[3, 3, 3, 40, 255, 256, 256], np.arange(480, 550), [700, 999, 999, nrec + 5]]).astype(np.uint64)
    assert np.all(idx[1:] >= idx[:-1])
    recs = rng.integers(0, 256, (idx.size, rec), dtype=np.uint8)
    dpf.pir_db_update_sliced_any_dev(d_dbs, nrec, rec, _dev(idx.view(np.uint8)).view(torch.int64), _dev(recs), idx.size)
    torch.cuda.synchronize()
    for i, r in zip(idx, recs):                                 # in order: the last of equal indices wins
        if i < nrec:
            db[int(i)] = r
    assert np.array_equal(d_dbs.cpu().numpy(), _layout(db))
    # Gather: any order, repeats, zeros past nrec.
    gi = np.array([999, 0, 513, 513, nrec, 3, 255, 256, nrec + 100, 481], np.uint64)
    d_out = torch.full((gi.size * rec + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    dpf.pir_db_gather_sliced_any_dev(d_dbs, nrec, rec, _dev(gi.view(np.uint8)).view(torch.int64), gi.size, d_out)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(out[gi.size * rec:] == 0xAB)
    want = np.stack([db[int(i)] if i < nrec else np.zeros(rec, np.uint8) for i in gi])
    assert np.array_equal(out[:gi.size * rec].reshape(gi.size, rec), want)


# ---- scatter and private write ------------------------------------------------------
def _xor_into(db, sel, msgs, nrec):
    """db[i] ^= XOR of msgs[k] over keys k with bit i of sel[k] set, i < nrec."""
    bits = np.unpackbits(sel, axis=1, bitorder="little")[:, :nrec].astype(np.float64)   # [k][i]
    mb = np.unpackbits(msgs, axis=1, bitorder="little").astype(np.float64)             # [k][p]
    par = (bits.T @ mb).astype(np.int64) & 1
    return db ^ np.packbits(par.astype(np.uint8), axis=1, bitorder="little")


@pytest.mark.parametrize("nk", [3, 70])
@pytest.mark.parametrize("rec", [12, 36, 100])
def test_scatter_any(rec, nk):
    import torch
    nrec = 1000
    rng = np.random.default_rng(rec * 100 + nk)
    stride = 144                                                # 1152 selection bits: set past nrec too
    bits = rng.integers(0, 256, (nk, stride), dtype=np.uint8)
    assert np.unpackbits(bits, axis=1, bitorder="little")[:, nrec:].any()
    msgs = rng.integers(0, 256, (nk, rec), dtype=np.uint8)
    db = _db(nrec, rec)
    d_dbs = _slice(db, nrec, rec)
    dpf.xor_scatter_sliced_any_dev(_dev(bits), stride, nk, _dev(msgs), d_dbs, nrec, rec)
    torch.cuda.synchronize()
    # the layout of the updated DB: in particular the records past nrec are still zero
    assert np.array_equal(d_dbs.cpu().numpy(), _layout(_xor_into(db, bits, msgs, nrec)))


@pytest.mark.parametrize("nk", [3, 70])
@pytest.mark.parametrize("rec", [12, 36, 100])
def test_pir_write_any(rec, nk):
    import torch
    logN, nrec = 12, 3000
    _, ka, _ = _keys(nk, logN, 1 << logN, first=500 + rec)
    full = oracle.evalfull_batch(ka, logN, nthreads=4)          # pseudorandom bits, set past nrec too
    msgs = np.random.default_rng(rec + nk).integers(0, 256, (nk, rec), dtype=np.uint8)
    db = _db(nrec, rec)
    d_dbs = _slice(db, nrec, rec)
    d_work = torch.empty(dpf.pir_workspace_size(nk, logN), dtype=torch.uint8, device="cuda")
    dpf.pir_write_sliced_any_dev(_dev(ka), dpf.key_len(logN), nk, logN, _dev(msgs), d_dbs, nrec, rec, d_work)
    torch.cuda.synchronize()
    assert np.array_equal(d_dbs.cpu().numpy(), _layout(_xor_into(db, full, msgs, nrec)))


# ---- the handle takes every width ------------------------------------------------------
@pytest.mark.parametrize("rec", [1, 3, 20, 33, 100])
def test_handle_any_width(rec):
    logN, nrec, nk = 12, 3000, 6
    al, ka, kb = _keys(nk, logN, nrec, first=300 + rec)
    db = _db(nrec, rec).copy()
    rng = np.random.default_rng(rec)
    pa, pb = dpf.PirDB(db, logN, ngpus=1, rec_bytes=rec), dpf.PirDB(db, logN, ngpus=1, rec_bytes=rec)
    try:
        assert pa.nrec == nrec and dpf.lib().dpf_pir_db_rec_bytes(pa._h) == rec
        a, b = pa.answer(ka), pb.answer(kb)
        assert a.shape == (nk, rec)
        assert np.array_equal(a, _want(oracle.evalfull_batch(ka, logN, nthreads=4), db, nrec))
        for k in range(nk):
            assert np.array_equal((a ^ b)[k], db[int(al[k])])
        # update (any order, the last of equal indices wins) and read (the caller's order)
        idx = np.array([2999, 5, 5, 256, 1000, 0, 5], np.uint64)
        recs = rng.integers(0, 256, (idx.size, rec), dtype=np.uint8)
        for p in (pa, pb):
            p.update(idx, recs)
        for i, r in zip(idx, recs):
            db[int(i)] = r
        ri = np.array([5, 2999, 0, 1, 256, 5, 1000, 2998], np.uint64)
        assert np.array_equal(pa.read(ri), db[ri.astype(np.int64)])
        # an index past nrec: DPF_ERR_PARAM, nothing changed
        for call in (lambda: pa.update(np.array([1, nrec], np.uint64), recs[:2]), lambda: pa.read(np.array([nrec], np.uint64))):
            with pytest.raises(dpf.DPFPanic) as e:
                call()
            assert e.value.code == dpf.DPF_ERR_PARAM
        assert np.array_equal(pa.read(np.arange(nrec, dtype=np.uint64)), db)
        # private write: both servers apply the messages under their key shares
        msgs = rng.integers(0, 256, (nk, rec), dtype=np.uint8)
        pa.write(ka, msgs)
        pb.write(kb, msgs)
        da, dbb = pa.read(np.arange(nrec, dtype=np.uint64)), pb.read(np.arange(nrec, dtype=np.uint64))
        assert np.array_equal(da, _xor_into(db, oracle.evalfull_batch(ka, logN, nthreads=4), msgs, nrec))
        delta = np.zeros_like(db)
        for k in range(nk):
            delta[int(al[k])] ^= msgs[k]
        assert np.array_equal(da ^ dbb, delta)
        # and the answers follow the DB as it now is
        assert np.array_equal(pa.answer(kb), _want(oracle.evalfull_batch(kb, logN, nthreads=4), da, nrec))
        assert pa.nrec == nrec
    finally:
        pa.close()
        pb.close()
