"""Grouped PIR: one launch answers many small DBs (groups), each with its own
keys (dpf_pir_db_slice_grouped_dev, dpf_xor_fold_grouped_dev,
dpf_pir_answer_grouped_dev and the handle made by dpf_pir_db_create_grouped).
Expected selections come from oracle.evalfull_batch, expected answers and DBs
from numpy; never from the code under test.  Both servers' shares are run:
their answers XOR to the queried record of the key's own group.  Everything is
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
from dpf import buckets     # noqa: E402
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


def _expect(db, sel, kpg):
    """[ngroups * kpg][rec]: row g * kpg + j is the XOR of the rows of db[g]
    that sel[g * kpg + j] (bool [nrec]) selects."""
    out = np.zeros((sel.shape[0], db.shape[2]), np.uint8)
    for r in range(sel.shape[0]):
        if sel[r].any():
            out[r] = np.bitwise_xor.reduce(db[r // kpg][sel[r]], axis=0)
    return out


@functools.lru_cache(maxsize=None)
def _case(logN, nrec, ng, kpg):
    """(alphas, ka, kb, selA, selB) of ng * kpg key pairs in group order, each
    at a point below nrec (the first and the last record among them), and the
    oracle's selections of both shares over the nrec records of a group."""
    nk = ng * kpg
    rng = np.random.default_rng(logN * 1009 + nrec * 31 + ng * 7 + kpg)
    alphas = rng.integers(0, nrec, nk, dtype=np.uint64)
    alphas[0], alphas[nk - 1] = 0, nrec - 1
    _, s0, s1 = synth.key_seeds(nk, logN, first=nrec + ng)
    ka, kb = dpf.gen_batch_seeded(alphas, logN, s0, s1)
    sel = [np.unpackbits(oracle.evalfull_batch(k, logN, nthreads=8), axis=1, bitorder="little")[:, :nrec].astype(bool)
           for k in (ka, kb)]
    assert np.array_equal(sel[0] ^ sel[1], np.arange(nrec, dtype=np.uint64)[None, :] == alphas[:, None])
    for a in (alphas, ka, kb, sel[0], sel[1]):
        a.setflags(write=False)
    return alphas, ka, kb, sel[0], sel[1]


@functools.lru_cache(maxsize=None)
def _db(ng, nrec, rec):
    db = np.random.default_rng(ng * 13 + nrec * 7 + rec).integers(0, 256, (ng, nrec, rec), dtype=np.uint8)
    db.setflags(write=False)
    return db


def _grouped(db):
    """The grouped sliced layout of db [ng][nrec][rec], GUARD bytes of 0x5A behind it."""
    import torch
    ng, nrec, rec = db.shape
    size = dpf.pir_db_grouped_size(ng, nrec, rec)
    assert size == max(16, ng * dpf.pir_group_stride(nrec) * rec)
    buf = torch.full((size + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    dpf.pir_db_slice_grouped_dev(_dev(db), ng, nrec, rec, buf)
    torch.cuda.synchronize()
    return buf, size


def _answer_dev(keys, logN, ng, kpg, dbs, nrec, rec):
    """dpf_pir_answer_grouped_dev with guards behind d_ans and d_work."""
    import torch
    nk = ng * kpg
    ws = dpf.pir_grouped_workspace_size(ng, kpg, logN, rec)
    d_work = torch.full((ws + GUARD,), 0x33, dtype=torch.uint8, device="cuda")
    d_ans = torch.full((nk * rec + GUARD,), 0x33, dtype=torch.uint8, device="cuda")
    dpf.pir_answer_grouped_dev(_dev(keys), keys.shape[1], ng, kpg, logN, dbs, nrec, rec, d_ans, d_work)
    torch.cuda.synchronize()
    dpf.forget_workspace(d_work)
    a = d_ans.cpu().numpy()
    assert (a[nk * rec:] == 0x33).all()
    assert (d_work[ws:].cpu().numpy() == 0x33).all()
    return a[:nk * rec].reshape(nk, rec)


# (logN, nrec): a key row shorter than a super-group; one whole super-group;
# two, the second nearly empty; four; twenty, several runs per group with a
# ragged last one when the groups are few.
SHAPES = [(7, 100), (8, 256), (9, 257), (10, 1000), (13, 5000)]
REC = [4, 20, 32, 100]
GROUPS = [(1, 1), (2, 3), (3, 5), (65, 1), (65, 2)]


@pytest.mark.parametrize("ng,kpg", GROUPS)
@pytest.mark.parametrize("rec", REC)
@pytest.mark.parametrize("logN,nrec", SHAPES)
def test_answer_grouped_dev(logN, nrec, rec, ng, kpg):
    alphas, ka, kb, selA, selB = _case(logN, nrec, ng, kpg)
    db = _db(ng, nrec, rec)
    dbs, size = _grouped(db)
    got = []
    for keys, sel in ((ka, selA), (kb, selB)):
        got.append(_answer_dev(keys, logN, ng, kpg, dbs, nrec, rec))
        assert np.array_equal(got[-1], _expect(db, sel, kpg))
    # Two servers: the record at alpha of the key's own group.
    want = np.stack([db[r // kpg][int(alphas[r])] for r in range(ng * kpg)])
    assert np.array_equal(got[0] ^ got[1], want)
    assert (dbs.cpu().numpy()[size:] == 0x5A).all()


@pytest.mark.parametrize("ng,kpg", [(65, 2), (3, 5)])
@pytest.mark.parametrize("rec", REC)
@pytest.mark.parametrize("logN,nrec", SHAPES)
def test_answers_do_not_depend_on_the_fold_limits(logN, nrec, rec, ng, kpg):
    """max_blocks 2 and 7 force many launches per key pass; the answers are
    those of the default plan and of numpy."""
    _, ka, _, selA, _ = _case(logN, nrec, ng, kpg)
    db = _db(ng, nrec, rec)
    dbs, _ = _grouped(db)
    base = _answer_dev(ka, logN, ng, kpg, dbs, nrec, rec)
    assert np.array_equal(base, _expect(db, selA, kpg))
    try:
        for mb in (2, 7):
            dpf.set_fold_limits(mb, 0)
            assert np.array_equal(_answer_dev(ka, logN, ng, kpg, dbs, nrec, rec), base), mb
    finally:
        dpf.set_fold_limits(0, 0)


@pytest.mark.parametrize("ng,kpg", [(3, 5), (65, 1)])
def test_bits_past_nrec_select_only_zero_records(ng, kpg):
    """nrec = 100 at logN 10: the EvalFull rows carry 924 pseudo-random bits
    past the group's records, 156 of them inside the group's super-group."""
    logN, nrec, rec = 10, 100, 20
    alphas, ka, kb, selA, selB = _case(logN, nrec, ng, kpg)
    db = _db(ng, nrec, rec)
    dbs, _ = _grouped(db)
    a = _answer_dev(ka, logN, ng, kpg, dbs, nrec, rec)
    b = _answer_dev(kb, logN, ng, kpg, dbs, nrec, rec)
    assert np.array_equal(a, _expect(db, selA, kpg)) and np.array_equal(b, _expect(db, selB, kpg))
    assert np.array_equal(a ^ b, np.stack([db[r // kpg][int(alphas[r])] for r in range(ng * kpg)]))


@pytest.mark.parametrize("ng,kpg", [(1, 1), (3, 5), (65, 2)])
@pytest.mark.parametrize("nrec,rec,extra", [(100, 20, 16), (257, 4, 48), (1000, 100, 0), (5000, 32, 112)])
def test_fold_grouped_on_caller_made_bits(nrec, rec, extra, ng, kpg):
    """Random bit rows with a stride larger than the records need; the bits at
    positions >= nrec are random too."""
    import torch
    nk = ng * kpg
    stride = (nrec + 127) // 128 * 16 + extra
    rows = np.random.default_rng(nrec + rec + nk).integers(0, 256, (nk, stride), dtype=np.uint8)
    sel = np.unpackbits(rows, axis=1, bitorder="little")[:, :nrec].astype(bool)
    db = _db(ng, nrec, rec)
    dbs, size = _grouped(db)
    ws = dpf.xor_fold_grouped_workspace_size(ng, kpg, rec)
    d_work = torch.full((ws + GUARD,), 0x33, dtype=torch.uint8, device="cuda")
    d_ans = torch.full((nk * rec + GUARD,), 0x33, dtype=torch.uint8, device="cuda")
    dpf.xor_fold_grouped_dev(_dev(rows), stride, ng, kpg, dbs, nrec, rec, d_ans, d_work)
    torch.cuda.synchronize()
    a = d_ans.cpu().numpy()
    assert (a[nk * rec:] == 0x33).all() and (d_work[ws:].cpu().numpy() == 0x33).all()
    assert np.array_equal(a[:nk * rec].reshape(nk, rec), _expect(db, sel, kpg))
    assert (dbs.cpu().numpy()[size:] == 0x5A).all()


@pytest.mark.parametrize("ng", [1, 3, 65])
@pytest.mark.parametrize("nrec,rec", [(100, 20), (256, 32), (257, 4), (1000, 100)])
def test_slice_grouped_is_the_slice_of_the_padded_flat_db(nrec, rec, ng):
    import torch
    db = _db(ng, nrec, rec)
    dbs, size = _grouped(db)
    gs = dpf.pir_group_stride(nrec)
    flat = np.zeros((ng, gs, rec), np.uint8)
    flat[:, :nrec] = db
    assert dpf.pir_db_sliced_size_any(ng * gs, rec) == size
    ref = torch.full((size + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    dpf.pir_db_slice_any_dev(_dev(flat), ng * gs, rec, ref)
    torch.cuda.synchronize()
    assert torch.equal(dbs, ref)


def test_empty_groups_answer_zero():
    import torch
    ng, kpg, rec, logN = 3, 2, 20, 8
    _, ka, _, _, _ = _case(logN, 256, ng, kpg)
    dbs = torch.zeros(16, dtype=torch.uint8, device="cuda")
    assert not _answer_dev(ka, logN, ng, kpg, dbs, 0, rec).any()


def _handle_checks(rec, ng, ngpus=1):
    """A grouped PirDB of ng groups of 300 records at logN 9, 3 keys per group:
    answer, update across a group edge, read everything, answer again."""
    logN, nrec, kpg = 9, 300, 3
    alphas, ka, kb, selA, selB = _case(logN, nrec, ng, kpg)
    db = _db(ng, nrec, rec)
    pdb = dpf.PirDB(db, logN, ngpus=ngpus, rec_bytes=rec, groups=ng)
    assert pdb.nrec == ng * nrec and pdb.ngroups == ng and pdb.rec_bytes == rec
    everything = np.arange(ng * nrec, dtype=np.uint64)
    assert np.array_equal(pdb.read(everything), db.reshape(ng * nrec, rec))
    a, b = pdb.answer(ka), pdb.answer(kb)
    assert np.array_equal(a, _expect(db, selA, kpg)) and np.array_equal(b, _expect(db, selB, kpg))
    assert np.array_equal(a ^ b, np.stack([db[r // kpg][int(alphas[r])] for r in range(ng * kpg)]))
    # Any order, both sides of the edge between the last two groups (a shard
    # edge with two shards), the first and the last record, one index twice.
    e = (ng - 1) * nrec
    idx = np.array([e, e - 1, 0, ng * nrec - 1, 299, 300, e], np.uint64)
    recs = np.random.default_rng(rec + 1).integers(0, 256, (idx.size, rec), dtype=np.uint8)
    pdb.update(idx, recs)
    want = db.reshape(ng * nrec, rec).copy()
    for i, r in zip(idx, recs):
        want[int(i)] = r                                        # of repeated indices the last wins
    assert np.array_equal(pdb.read(idx), want[idx.astype(np.int64)])
    assert np.array_equal(pdb.read(everything), want)
    want3 = want.reshape(ng, nrec, rec)
    assert np.array_equal(pdb.answer(ka), _expect(want3, selA, kpg))
    assert np.array_equal(pdb.answer(kb), _expect(want3, selB, kpg))
    with pytest.raises(dpf.DPFPanic) as ex:
        pdb.update(np.array([0, ng * nrec], np.uint64), recs[:2])
    assert ex.value.code == dpf.DPF_ERR_PARAM
    assert np.array_equal(pdb.read(everything), want)           # one bad index: nothing changed
    if ng > 1:
        with pytest.raises(dpf.DPFPanic) as ex:
            pdb.answer(ka[:ng * kpg - 1])                       # not a multiple of the groups
        assert ex.value.code == dpf.DPF_ERR_PARAM
    with pytest.raises(dpf.DPFPanic) as ex:
        pdb.write(ka, np.zeros((ng * kpg, rec), np.uint8))
    assert ex.value.code == dpf.DPF_ERR_PARAM
    with pytest.raises(dpf.DPFPanic) as ex:
        pdb.answer(ka[:, :16 + 18 * (logN - 7)])
    assert ex.value.code == dpf.DPF_ERR_KEYLEN
    assert np.array_equal(pdb.read(everything), want)
    pdb.close()
    assert pdb.nrec == 0 and pdb.ngroups == 0


@pytest.mark.parametrize("rec", [7, 32])
def test_grouped_handle(rec):
    _handle_checks(rec, 7)


def test_other_handles_report_one_group():
    db = _db(1, 300, 32)[0]
    pdb = dpf.PirDB(db, 9, rec_bytes=32)
    assert pdb.ngroups == 1
    pdb.close()
    with pytest.raises(dpf.DPFPanic):
        dpf.PirDB(_db(2, 300, 32), 9, ngpus=dpf.gpu_count() + 1, rec_bytes=32, groups=2)
    with pytest.raises(ValueError):
        dpf.PirDB(_db(1, 300, 32), 9, rec_bytes=32, groups=7)


def test_batch_code_end_to_end():
    """dpf/buckets.py over a grouped PirDB: 3000 records of 20 bytes in 12
    buckets, a client wanting 8 of them sends one key pair per bucket."""
    n, rec, nb, seed = 3000, 20, 12, 3
    db = np.random.default_rng(5).integers(0, 256, (n, rec), dtype=np.uint8)
    lay = buckets.layout(n, nb, seed=seed)
    bdb, logN = buckets.build(db, lay)
    wanted = np.random.default_rng(seed).choice(n, 8, replace=False)
    got = buckets.assign(wanted, lay)
    al = buckets.alphas(got, lay)
    _, s0, s1 = synth.key_seeds(nb, logN, first=17)
    ka, kb = dpf.gen_batch_seeded(al, logN, s0, s1)
    pdb = dpf.PirDB(bdb, logN, rec_bytes=rec, groups=nb)
    assert pdb.ngroups == nb and pdb.nrec == nb * lay.cap
    x = pdb.answer(ka) ^ pdb.answer(kb)
    pdb.close()
    assert sorted(got.values()) == sorted(int(w) for w in wanted)
    for b, r in got.items():
        assert np.array_equal(x[b], db[r])
    for b in set(range(nb)) - set(got):
        assert np.array_equal(x[b], bdb[b, 0])                  # the dummy query of an unused bucket


def test_two_shard_grouped_handle():
    """gpu_init_devices([0, 0]) and PirDB(..., ngpus=2, groups=3): shards of
    two groups and of one; each answers its own groups' keys."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "two-shards"], capture_output=True, text=True,
                       timeout=240, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith("done")


if __name__ == "__main__":
    dpf.gpu_init_devices([0, 0])
    _handle_checks(7, 3, ngpus=2)
    _handle_checks(32, 3, ngpus=2)
    dpf.gpu_shutdown()
    print("done")
