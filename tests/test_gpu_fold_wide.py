"""GPU parity of the matrix-core fold over records wider than 32 bytes: the
wide sliced layout dbs[S][c][n][g] (include/dpf_hip.h), the fold and PIR
entry points over it and the wide PIR handle.  Expected answers are numpy
folds of the CPU oracle's EvalFull bits (or of random bits) with the row-major
payload, never the code under test."""
import numpy as np
import pytest

import dpf
from dpf import synth
import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert dpf.gpu_init(1) >= 1


@pytest.fixture
def fold_limits():
    yield dpf.set_fold_limits
    dpf.set_fold_limits(0, 0)


def _keys(nk, logN, first=0):
    al, s0, s1 = synth.key_seeds(nk, logN, first=first)
    ka, kb = dpf.gen_batch_seeded(al, logN, s0, s1)
    return al, ka, kb


def _want(full: np.ndarray, payload: np.ndarray, nrec: int) -> np.ndarray:
    """XOR of payload rows i < nrec with bit i (LSB-first) of each selection row set."""
    bits = np.unpackbits(full, axis=1, bitorder="little")[:, :nrec].astype(bool)
    out = np.zeros((full.shape[0], payload.shape[1]), np.uint8)
    for k in range(full.shape[0]):
        sel = payload[:nrec][bits[k]]
        if sel.shape[0]:
            out[k] = np.bitwise_xor.reduce(sel, axis=0)
    return out


def _layout(db: np.ndarray) -> np.ndarray:
    """The wide sliced layout of a row-major (nrec, rec_bytes) DB, from its
    definition: u32 dbs[S][c][n][g], bit j = bit n of bytes [32c, 32c+32) of
    record 256 S + 32 g + j (bit n of a column = bit n%8 of its byte n/8);
    records past nrec are 0."""
    nrec, rec = db.shape
    C, nsg = rec // 32, (nrec + 255) // 256
    pad = np.zeros((nsg * 256, rec), np.uint8)
    pad[:nrec] = db
    b = np.unpackbits(pad, axis=1, bitorder="little")          # [record][256 c + n]
    b = b.reshape(nsg, 8, 32, C, 256)                          # [S][g][j][c][n]
    b = b.transpose(0, 3, 4, 1, 2)                             # [S][c][n][g][j]
    return np.packbits(np.ascontiguousarray(b).reshape(-1), bitorder="little")   # LE u32 = 4 bytes of j


def _dev(a):
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    if a.size == 0:
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a).cuda()


def _slice_wide(db, nrec, rec):
    import torch
    d_dbs = torch.full((dpf.pir_db_sliced_size_wide(nrec, rec),), 0x5A, dtype=torch.uint8, device="cuda")
    dpf.pir_db_slice_wide_dev(_dev(db), nrec, rec, d_dbs)
    torch.cuda.synchronize()
    return d_dbs


def _fold_wide(d_bits, stride, nk, d_dbs, nrec, rec):
    import torch
    d_ans = torch.full((max(nk * rec, 16),), 0xAB, dtype=torch.uint8, device="cuda")   # overwritten, not accumulated
    d_work = torch.empty(dpf.xor_fold_workspace_size(), dtype=torch.uint8, device="cuda")
    dpf.xor_fold_sliced_wide_dev(d_bits, stride, nk, d_dbs, nrec, rec, d_ans, d_work)
    torch.cuda.synchronize()
    return d_ans.cpu().numpy()[:nk * rec].reshape(nk, rec)


def _fold_rows(d_bits, stride, nk, db, nrec, rec):
    import torch
    d_ans = torch.full((max(nk * rec, 16),), 0xAB, dtype=torch.uint8, device="cuda")
    d_work = torch.empty(dpf.xor_fold_workspace_size(), dtype=torch.uint8, device="cuda")
    dpf.xor_fold_dev(d_bits, stride, nk, _dev(db), nrec, rec, d_ans, d_work)
    torch.cuda.synchronize()
    return d_ans.cpu().numpy()[:nk * rec].reshape(nk, rec)


# ---- 1. layout --------------------------------------------------------------
@pytest.mark.parametrize("nrec,rec", [(300, 64), (256, 96), (1, 160), (1000, 1024), (777, 32)])
def test_wide_slice_is_the_documented_layout(nrec, rec):
    import torch
    db = np.random.default_rng(nrec + rec).integers(0, 256, (nrec, rec), dtype=np.uint8)
    got = _slice_wide(db, nrec, rec).cpu().numpy()
    want = _layout(db)
    assert got.size == want.size == (nrec + 255) // 256 * 256 * rec
    assert np.array_equal(got, want)
    if rec == 32:
        d32 = torch.empty(dpf.pir_db_sliced_size(nrec), dtype=torch.uint8, device="cuda")
        dpf.pir_db_slice_dev(_dev(db), nrec, d32)
        torch.cuda.synchronize()
        assert np.array_equal(got, d32.cpu().numpy())


# ---- 2. chunked slicing -----------------------------------------------------
def test_wide_slice_in_chunks_of_whole_super_groups():
    import torch
    nrec, rec = 1000, 128
    db = np.random.default_rng(2).integers(0, 256, (nrec, rec), dtype=np.uint8)
    whole = _slice_wide(db, nrec, rec).cpu().numpy()
    d = torch.full((dpf.pir_db_sliced_size_wide(nrec, rec),), 0x5A, dtype=torch.uint8, device="cuda")
    dpf.pir_db_slice_wide_dev(_dev(db[:512]), 512, rec, d)
    dpf.pir_db_slice_wide_dev(_dev(db[512:]), nrec - 512, rec, d[512 * rec:])
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), whole)
    assert np.array_equal(whole, _layout(db))


def test_slice_in_chunks_at_32_bytes():
    """The same through the 32-byte entry: records [0, 512) and [512, 1000)
    sliced into one buffer give the whole-DB slice."""
    import torch
    nrec = 1000
    db = np.random.default_rng(3).integers(0, 256, (nrec, 32), dtype=np.uint8)
    whole = torch.full((dpf.pir_db_sliced_size(nrec),), 0x5A, dtype=torch.uint8, device="cuda")
    dpf.pir_db_slice_dev(_dev(db), nrec, whole)
    d = torch.full((dpf.pir_db_sliced_size(nrec),), 0x5A, dtype=torch.uint8, device="cuda")
    dpf.pir_db_slice_dev(_dev(db[:512]), 512, d)
    dpf.pir_db_slice_dev(_dev(db[512:]), nrec - 512, d[512 * 32:])
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), whole.cpu().numpy())
    assert np.array_equal(whole.cpu().numpy(), _layout(db))


# ---- 3. fold against the oracle's bits --------------------------------------
# The one-key path, key tiles 1/2/4/8, a second 256-key pass, C = 1, 2, 3, 4,
# 5, 8, 16, 32 and 33, ragged last super-groups, nrec = 0 and 1.
@pytest.mark.parametrize("logN,nk,rec,nrec", [
    (7, 1, 64, 128), (9, 3, 96, 300), (12, 33, 64, 4096), (12, 64, 256, 4000), (13, 65, 128, 8192),
    (12, 129, 160, 4096), (12, 256, 64, 4096), (12, 300, 96, 3001), (8, 5, 1024, 1), (10, 7, 128, 0),
    (11, 64, 1056, 2048), (14, 64, 512, 16384 - 77), (12, 40, 32, 4096),
])
def test_wide_fold_matches_oracle(logN, nk, rec, nrec):
    import torch
    _, ka, _ = _keys(nk, logN, first=1300 + nk)
    full = oracle.evalfull_batch(ka, logN, nthreads=8)
    stride = full.shape[1]
    db = synth.db_bytes(max(nrec, 1) * rec).reshape(-1, rec)[:nrec]
    d_bits = _dev(full)
    d_dbs = _slice_wide(db, nrec, rec)
    got = _fold_wide(d_bits, stride, nk, d_dbs, nrec, rec)
    assert np.array_equal(got, _want(full, db, nrec))
    assert np.array_equal(got, _fold_rows(d_bits, stride, nk, db, nrec, rec))
    if rec == 32:
        d_ans = torch.full((nk * 32,), 0xAB, dtype=torch.uint8, device="cuda")
        d_work = torch.empty(dpf.xor_fold_workspace_size(), dtype=torch.uint8, device="cuda")
        dpf.xor_fold_sliced_dev(d_bits, stride, nk, d_dbs, nrec, d_ans, d_work)
        torch.cuda.synchronize()
        assert np.array_equal(got, d_ans.cpu().numpy().reshape(nk, 32))


# ---- 4. forced passes -------------------------------------------------------
@pytest.mark.parametrize("max_blocks,max_sg,nk,rec,nrec", [
    (1, 1, 64, 64, 8192), (3, 5, 33, 96, 29993), (2, 3, 129, 256, 20000), (7, 2, 1, 128, 9999),
    (5, 4, 300, 64, 12345), (3, 5, 33, 32, 29993), (2, 3, 300, 32, 20000),
])
def test_wide_fold_forced_passes(fold_limits, max_blocks, max_sg, nk, rec, nrec):
    rng = np.random.default_rng(nk * 7 + nrec + rec)
    stride = ((nrec + 7) // 8 + 15) // 16 * 16
    bits = rng.integers(0, 256, (nk, stride), dtype=np.uint8)
    db = synth.db_bytes(nrec * rec).reshape(nrec, rec)
    d_bits = _dev(bits)
    d_dbs = _slice_wide(db, nrec, rec)
    base = _fold_wide(d_bits, stride, nk, d_dbs, nrec, rec)
    fold_limits(max_blocks, max_sg)
    forced = _fold_wide(d_bits, stride, nk, d_dbs, nrec, rec)
    fold_limits(0, 0)
    assert np.array_equal(forced, base)
    assert np.array_equal(base, _want(bits, db, nrec))


# ---- 5. exact counts --------------------------------------------------------
def test_wide_fold_counts_past_2p24_in_one_workgroup(fold_limits):
    """test_gpu_fold.py::test_sliced_fold_counts_past_2p24_in_one_workgroup for
    the wide launcher: 2^24 + 2^21 records of an all-ones 64-byte-record DB,
    one workgroup per launch; every answer byte is 0xFF or 0x00 by the parity
    of the key's selected count."""
    import torch
    nk, rec, nrec = 32, 64, (1 << 24) + (1 << 21)
    stride = nrec // 8
    rng = np.random.default_rng(5)
    bits = np.full((nk, stride), 0xFF, np.uint8)
    holes = rng.random((nk, stride)) < 0.125
    bits[holes] = rng.integers(0, 256, int(holes.sum()), dtype=np.uint8)
    d_dbs = torch.full((dpf.pir_db_sliced_size_wide(nrec, rec),), 0xFF, dtype=torch.uint8, device="cuda")
    fold_limits(1, 0)
    got = _fold_wide(_dev(bits), stride, nk, d_dbs, nrec, rec)
    par = np.unpackbits(bits, axis=1).sum(axis=1) & 1
    want = np.where(par[:, None] == 1, 0xFF, 0).astype(np.uint8) * np.ones((1, rec), np.uint8)
    assert np.array_equal(got, want)


# ---- 6. PIR answer on a subtree ---------------------------------------------
def test_wide_pir_answer_on_a_subtree():
    import torch
    logN, pb, prefix, nk, rec, nrec = 12, 2, 3, 20, 128, 1000
    _, ka, _ = _keys(nk, logN, first=61)
    full = oracle.evalfull_batch(ka, logN, nthreads=8)
    q = full.shape[1] // 4
    quarter = np.ascontiguousarray(full[:, prefix * q:(prefix + 1) * q])
    db = synth.db_bytes(nrec * rec).reshape(nrec, rec)
    kl = dpf.key_len(logN)
    d_keys = _dev(ka)
    d_work = torch.empty(dpf.pir_workspace_size(nk, logN, pb), dtype=torch.uint8, device="cuda")
    d_dbs = _slice_wide(db, nrec, rec)
    res = []
    for f, d in ((dpf.pir_answer_sliced_wide_dev, d_dbs), (dpf.pir_answer_wide_dev, _dev(db))):
        d_ans = torch.full((nk * rec,), 0xAB, dtype=torch.uint8, device="cuda")
        f(d_keys, kl, nk, logN, d, nrec, rec, d_ans, d_work, prefix_bits=pb, prefix=prefix)
        torch.cuda.synchronize()
        res.append(d_ans.cpu().numpy().reshape(nk, rec))
    assert np.array_equal(res[0], res[1])
    assert np.array_equal(res[0], _want(quarter, db, nrec))


# ---- 7. handle --------------------------------------------------------------
def test_wide_handle_two_server_property():
    logN, nk, rec = 12, 40, 256
    nrec = 1 << logN
    al, ka, kb = _keys(nk, logN, first=71)
    db = synth.db_bytes(nrec * rec).reshape(nrec, rec)
    pdb = dpf.PirDB(db, logN, ngpus=1, rec_bytes=rec)
    a, b = pdb.answer(ka), pdb.answer(kb)
    pdb.close()
    assert a.shape == (nk, rec)
    x = a ^ b
    for k in range(nk):
        assert np.array_equal(x[k], db[int(al[k])])


def test_wide_handle_at_32_bytes_and_short_db():
    logN, nk = 12, 40
    al, ka, kb = _keys(nk, logN, first=72)
    db32 = synth.db_bytes((1 << logN) * 32).reshape(-1, 32)
    p32 = dpf.PirDB(db32, logN)
    want = p32.answer(ka)
    p32.close()
    h = dpf._vp()
    d = np.ascontiguousarray(db32).reshape(-1)
    dpf._check(dpf.lib().dpf_pir_db_create_wide(dpf._buf(d), 1 << logN, 32, logN, 1, dpf.ctypes.byref(h)))
    assert dpf.lib().dpf_pir_db_rec_bytes(h) == 32
    got = np.zeros((nk, 32), np.uint8)
    dpf._check(dpf.lib().dpf_pir_answer(h, dpf._buf(ka), ka.shape[1], nk, dpf._buf(got)))
    dpf.lib().dpf_pir_db_free(h)
    assert np.array_equal(got, want)
    # nrec = 3000 < 2^12 records of 96 bytes
    nrec, rec = 3000, 96
    db = synth.db_bytes(nrec * rec).reshape(nrec, rec)
    pdb = dpf.PirDB(db, logN, ngpus=1, rec_bytes=rec)
    x = pdb.answer(ka) ^ pdb.answer(kb)
    pdb.close()
    for k in range(nk):
        a = int(al[k])
        assert np.array_equal(x[k], db[a] if a < nrec else np.zeros(rec, np.uint8))


# ---- 8. bad buffers ---------------------------------------------------------
def test_wide_pir_answer_rejects_bad_buffers():
    import torch
    logN, nk, rec = 12, 2, 64
    _, ka, _ = _keys(nk, logN, first=5)
    kl = dpf.key_len(logN)
    d_keys = _dev(ka)
    d = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    w = torch.empty(dpf.pir_workspace_size(nk, logN), dtype=torch.uint8, device="cuda")
    for f in (dpf.pir_answer_wide_dev, dpf.pir_answer_sliced_wide_dev):
        for db, ans, work in ((None, d, w), (d, None, w), (d, d, None), (d[1:], d, w), (d, d[2:], w),
                              (d, d, w[4:])):
            with pytest.raises(dpf.DPFPanic) as e:
                f(d_keys, kl, nk, logN, db, 100, rec, ans, work)
            assert e.value.code == dpf.DPF_ERR_PARAM
