"""Records of a resident PIR DB updated and read back in place
(dpf_pir_db_update_sliced_wide_dev, dpf_pir_db_gather_sliced_wide_dev and
the handle's update / read).  Expected values are numpy restatements of the
wide sliced layout's definition (include/dpf_hip.h) over the modified
row-major DB, and CPU-oracle answers over it; never the code under test.

The two-shard and the row-major (DPF_PIR_FOLD=lds) handles need a process of
their own (the device registry and the fold choice are process-wide): the
tests at the end run this file as a script."""
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


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert dpf.gpu_init(1) >= 1


def _layout(db: np.ndarray) -> np.ndarray:
    """u32 dbs[S][c][n][g] as bytes: bit j of the word = bit n of bytes
    [32c, 32c+32) of record 256 S + 32 g + j, bit n of a column being bit n%8
    of its byte n/8; records past nrec are 0 (include/dpf_hip.h)."""
    nrec, rec = db.shape
    C, nsg = rec // 32, (nrec + 255) // 256
    pad = np.zeros((nsg * 256, rec), np.uint8)
    pad[:nrec] = db
    b = np.unpackbits(pad, axis=1, bitorder="little")          # [256 S + 32 g + j][256 c + n]
    b = b.reshape(nsg, 8, 32, C, 256).transpose(0, 3, 4, 1, 2)  # [S][c][n][g][j]
    return np.packbits(np.ascontiguousarray(b).reshape(-1), bitorder="little")


def _dev(a):
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    if a.size == 0:                       # the entry points refuse null pointers, also with n = 0
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    return torch.from_numpy(a.view(np.uint8)).cuda()


def _slice(db):
    import torch
    nrec, rec = db.shape
    d_dbs = torch.full((dpf.pir_db_sliced_size_wide(nrec, rec),), 0x5A, dtype=torch.uint8, device="cuda")
    dpf.pir_db_slice_wide_dev(_dev(db), nrec, rec, d_dbs)
    torch.cuda.synchronize()
    return d_dbs


def _update(d_dbs, nrec, rec, idx, recs):
    import torch
    idx = np.asarray(idx, np.uint64)
    dpf.pir_db_update_sliced_wide_dev(d_dbs, nrec, rec, _dev(idx), _dev(recs), idx.size)
    torch.cuda.synchronize()


def _gather(d_dbs, nrec, rec, idx):
    import torch
    idx = np.asarray(idx, np.uint64)
    d_out = torch.full((max(idx.size * rec, 16),), 0xAB, dtype=torch.uint8, device="cuda")
    dpf.pir_db_gather_sliced_wide_dev(d_dbs, nrec, rec, _dev(idx), idx.size, d_out)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()[:idx.size * rec].reshape(idx.size, rec)


def _apply(db, idx, recs, nrec=None):
    """The modified row-major DB: updates in order (the last of equal indices
    wins), indices >= nrec skipped."""
    out = db.copy()
    for i, r in zip(idx, recs):
        if int(i) < (db.shape[0] if nrec is None else nrec):
            out[int(i)] = r
    return out


SHAPES = [(300, 32), (300, 64), (1000, 96), (1, 160), (777, 1024)]


def _index_set(kind, nrec):
    """Non-decreasing record indices of one kind, clamped into the DB (a
    one-record DB folds every kind onto record 0)."""
    top = nrec - 1
    S = 256 if nrec >= 512 else 0            # a middle super-group where there is one
    g = 32 * 5 if nrec >= 256 else 0
    if kind == "first":
        idx = [0]
    elif kind == "last":
        idx = [top]
    elif kind == "one_word":                 # same S, same g, different j
        idx = sorted({min(S + g + 3, top), min(S + g + 17, top)})
    elif kind == "several_g":                # one super-group, words g = 0, 1, 2, 4, 7
        idx = sorted({min(S + o, top) for o in (1, 40, 95, 130, 255)})
    elif kind == "every_sg":                 # one record in each super-group
        idx = sorted({min(256 * s + (7 * s + 5) % 256, top) for s in range((nrec + 255) // 256)})
    elif kind == "duplicate":                # the same index twice, different payloads: the later wins
        a = min(S + g + 9, top)
        idx = [a, a, top] if top > a else [a, a]
    elif kind == "all":
        idx = list(range(nrec))
    elif kind == "none":
        idx = []
    return np.array(idx, np.uint64)


@pytest.mark.parametrize("kind", ["first", "last", "one_word", "several_g", "every_sg", "duplicate", "all", "none"])
@pytest.mark.parametrize("nrec,rec", SHAPES)
def test_update_leaves_the_documented_layout(nrec, rec, kind):
    """The whole sliced buffer after the update equals the layout's definition
    applied to the modified DB: the records changed, no other record harmed,
    the padding of the last super-group still zero."""
    rng = np.random.default_rng(nrec * 31 + rec)
    db = rng.integers(0, 256, (nrec, rec), dtype=np.uint8)
    idx = _index_set(kind, nrec)
    recs = rng.integers(0, 256, (idx.size, rec), dtype=np.uint8)
    if kind == "duplicate":
        assert idx[0] == idx[1] and not np.array_equal(recs[0], recs[1])
    d_dbs = _slice(db)
    _update(d_dbs, nrec, rec, idx, recs)
    want = _layout(_apply(db, idx, recs))
    got = d_dbs.cpu().numpy()
    assert got.size == want.size
    assert np.array_equal(got, want)
    if kind == "all":                        # the same as slicing the new DB
        assert np.array_equal(got, _slice(recs).cpu().numpy())


def test_update_skips_indices_past_nrec():
    """400 lies in the padding of the last super-group, 512 and 10^12 past the
    buffer: all three are skipped, the padding stays zero."""
    nrec, rec = 300, 64
    rng = np.random.default_rng(4)
    db = rng.integers(0, 256, (nrec, rec), dtype=np.uint8)
    idx = np.array([5, 260, 299, 400, 512, 10 ** 12], np.uint64)
    recs = rng.integers(0, 256, (idx.size, rec), dtype=np.uint8)
    d_dbs = _slice(db)
    _update(d_dbs, nrec, rec, idx, recs)
    assert np.array_equal(d_dbs.cpu().numpy(), _layout(_apply(db, idx, recs, nrec)))
    only_bad = idx[3:]
    _update(d_dbs, nrec, rec, only_bad, recs[3:])
    assert np.array_equal(d_dbs.cpu().numpy(), _layout(_apply(db, idx, recs, nrec)))


def test_update_in_chunks_of_several_indices_per_workgroup():
    """Dense updates (more than two per super-group on average) take the
    launch shape in which one workgroup looks at several indices: runs that
    start, end and continue across those chunks, with duplicates."""
    nrec, rec = 2000, 64
    rng = np.random.default_rng(6)
    db = rng.integers(0, 256, (nrec, rec), dtype=np.uint8)
    for n in (40, 300, 1500, 6000):
        idx = np.sort(rng.integers(0, nrec, n)).astype(np.uint64)
        recs = rng.integers(0, 256, (n, rec), dtype=np.uint8)
        d_dbs = _slice(db)
        _update(d_dbs, nrec, rec, idx, recs)
        assert np.array_equal(d_dbs.cpu().numpy(), _layout(_apply(db, idx, recs))), n


@pytest.mark.parametrize("rec", [32, 96])
def test_update_of_consecutive_records(rec):
    """Runs of consecutive records take a transposing path from 16 records per
    64-entry batch: lengths around that threshold and around 64, odd starts,
    runs across word and super-group boundaries, a run broken by a gap or by a
    duplicate inside one batch (the per-update path), one run per call and
    all of them in one call."""
    nrec = 2000
    rng = np.random.default_rng(rec)
    db = rng.integers(0, 256, (nrec, rec), dtype=np.uint8)
    runs = [np.arange(5, 5 + 16), np.arange(100, 100 + 63), np.arange(250, 250 + 70), np.arange(600, 600 + 15),
            np.arange(1000, 1000 + 129), np.arange(1279, 1279 + 17), np.arange(1536, 1536 + 256),
            np.concatenate([np.arange(1800, 1830), [1835, 1840]]),
            np.sort(np.concatenate([np.arange(1900, 1940), [1920]])), np.arange(nrec - 20, nrec)]
    for idx in runs + [np.concatenate(runs)]:
        idx = idx.astype(np.uint64)
        recs = rng.integers(0, 256, (idx.size, rec), dtype=np.uint8)
        d_dbs = _slice(db)
        _update(d_dbs, nrec, rec, idx, recs)
        assert np.array_equal(d_dbs.cpu().numpy(), _layout(_apply(db, idx, recs))), idx[:3]


@pytest.mark.parametrize("nrec,rec", SHAPES)
def test_gather_returns_the_rows(nrec, rec):
    rng = np.random.default_rng(nrec + rec)
    db = rng.integers(0, 256, (nrec, rec), dtype=np.uint8)
    idx = rng.integers(0, nrec, 50).astype(np.uint64)          # random order, repeats
    idx[[3, 17, 40]] = [nrec, nrec + 300, 10 ** 12]             # out of range: zeros
    idx[[5, 6]] = idx[4]
    want = np.zeros((idx.size, rec), np.uint8)
    ok = idx < nrec
    want[ok] = db[idx[ok].astype(np.int64)]
    d_dbs = _slice(db)
    assert np.array_equal(_gather(d_dbs, nrec, rec, idx), want)
    # after an update the gather returns the new records
    up = np.unique(idx[ok])[::2]
    recs = rng.integers(0, 256, (up.size, rec), dtype=np.uint8)
    _update(d_dbs, nrec, rec, up, recs)
    want[ok] = _apply(db, up, recs)[idx[ok].astype(np.int64)]
    assert np.array_equal(_gather(d_dbs, nrec, rec, idx), want)
    assert _gather(d_dbs, nrec, rec, []).shape == (0, rec)     # n = 0


def test_fold_after_update_matches_oracle():
    import torch
    logN, nk, rec, nrec = 12, 40, 64, 4000
    al, s0, s1 = synth.key_seeds(nk, logN, first=1500)
    ka, _ = dpf.gen_batch_seeded(al, logN, s0, s1)
    full = oracle.evalfull_batch(ka, logN, nthreads=8)
    rng = np.random.default_rng(8)
    db = synth.db_bytes(nrec * rec).reshape(nrec, rec)
    idx = np.unique(rng.integers(0, nrec, 100)).astype(np.uint64)
    recs = rng.integers(0, 256, (idx.size, rec), dtype=np.uint8)
    d_dbs = _slice(db)
    _update(d_dbs, nrec, rec, idx, recs)
    d_ans = torch.full((nk * rec,), 0xAB, dtype=torch.uint8, device="cuda")
    d_work = torch.empty(dpf.xor_fold_workspace_size(), dtype=torch.uint8, device="cuda")
    dpf.xor_fold_sliced_wide_dev(_dev(full), full.shape[1], nk, d_dbs, nrec, rec, d_ans, d_work)
    torch.cuda.synchronize()
    new = _apply(db, idx, recs)
    bits = np.unpackbits(full, axis=1, bitorder="little")[:, :nrec].astype(bool)
    want = np.stack([np.bitwise_xor.reduce(new[bits[k]], axis=0) if bits[k].any() else np.zeros(rec, np.uint8)
                     for k in range(nk)])
    assert np.array_equal(d_ans.cpu().numpy().reshape(nk, rec), want)


def _oracle_answers(keys, logN, db):
    """oracle.pir_answer_batch per 32-byte column of the records."""
    nrec, rec = db.shape
    cols = [oracle.pir_answer_batch(keys, logN, np.ascontiguousarray(db[:, c:c + 32]), nrec)[:, 0, :]
            for c in range(0, rec, 32)]
    return np.concatenate(cols, axis=1)


def _handle_checks(rec, ngpus=1, first=90):
    """A handle at logN 12: unsorted updates with a duplicate on both sides of
    the middle of the DB (the shard boundary of a two-shard handle), then the
    two-server property, the oracle's answers, read-back in the caller's
    order, and a refused update that changes nothing."""
    logN, nk = 12, 40
    nrec = 1 << logN
    half = nrec // 2
    rng = np.random.default_rng(rec + ngpus)
    db = synth.db_bytes(nrec * rec).reshape(nrec, rec).copy()
    pdb = dpf.PirDB(db, logN, ngpus=ngpus, rec_bytes=rec)
    assert pdb.nrec == nrec
    idx = np.array([half, 3000, half - 1, 0, nrec - 1, half + 257, 5, half - 1, 100, 2047 - 256, half + 31],
                   np.uint64)                                    # unsorted, half - 1 twice
    recs = rng.integers(0, 256, (idx.size, rec), dtype=np.uint8)
    assert not np.array_equal(recs[2], recs[7])
    pdb.update(idx, recs)
    new = _apply(db, idx, recs)
    assert np.array_equal(new[half - 1], recs[7])
    al, s0, s1 = synth.key_seeds(nk, logN, first=first)
    al = al.copy()
    al[:idx.size] = idx                                          # alphas among the updated records
    ka, kb = dpf.gen_batch_seeded(al, logN, s0, s1)
    a, b = pdb.answer(ka), pdb.answer(kb)
    x = a ^ b
    for k in range(nk):
        assert np.array_equal(x[k], new[int(al[k])]), k
    assert np.array_equal(a, _oracle_answers(ka, logN, new))
    order = np.array([nrec - 1, half - 1, 7, half, 0, half - 1, 3000, 1234, half + 257], np.uint64)
    assert np.array_equal(pdb.read(order), new[order.astype(np.int64)])
    assert pdb.read([]).shape == (0, rec)
    with pytest.raises(dpf.DPFPanic) as e:
        pdb.update(np.array([9, nrec, 11], np.uint64), rng.integers(0, 256, (3, rec), dtype=np.uint8))
    assert e.value.code == dpf.DPF_ERR_PARAM
    with pytest.raises(dpf.DPFPanic) as e:
        pdb.read(np.array([nrec + 5], np.uint64))
    assert e.value.code == dpf.DPF_ERR_PARAM
    assert np.array_equal(pdb.answer(ka), a)
    assert np.array_equal(pdb.read(np.array([9, 11], np.uint64)), new[[9, 11]])
    pdb.close()
    assert pdb.nrec == 0


@pytest.mark.parametrize("rec", [256, 32])
def test_handle_update_and_read(rec):
    _handle_checks(rec)


def test_handle_of_a_short_db_refuses_to_grow():
    logN, rec, nrec = 12, 96, 3000
    db = synth.db_bytes(nrec * rec).reshape(nrec, rec)
    pdb = dpf.PirDB(db, logN, rec_bytes=rec)
    assert pdb.nrec == nrec
    with pytest.raises(dpf.DPFPanic) as e:
        pdb.update([nrec], np.zeros((1, rec), np.uint8))
    assert e.value.code == dpf.DPF_ERR_PARAM
    new = np.full((1, rec), 0xC3, np.uint8)
    pdb.update([nrec - 1], new)
    assert np.array_equal(pdb.read([nrec - 1, 0]), np.concatenate([new, db[:1]]))
    pdb.close()


def _child(mode):
    import subprocess
    env = dict(os.environ)
    env.pop("DPF_PIR_FOLD", None)
    if mode == "lds":
        env["DPF_PIR_FOLD"] = "lds"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode], capture_output=True, text=True, timeout=240,
                       env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith("done")


def test_two_shard_handle_update_and_read():
    """gpu_init_devices([0, 0]) and PirDB(..., ngpus=2): updates and reads on
    both sides of the shard boundary, each routed to its shard."""
    _child("two-shards")


def test_row_major_handle_update_and_read():
    """DPF_PIR_FOLD=lds keeps the shards row-major: the plain scatter and
    gather kernels (two shards, so the routing runs as well)."""
    _child("lds")


if __name__ == "__main__":
    dpf.gpu_init_devices([0, 0])
    for rec_bytes in (64, 32):
        _handle_checks(rec_bytes, ngpus=2, first=120)
    dpf.gpu_shutdown()
    print("done")
