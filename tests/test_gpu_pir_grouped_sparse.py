"""Grouped keyword PIR: many small DBs, record i of group g at domain point
points[g][i], the keys of a group evaluated at that group's own points in one
launch (dpf_eval_bits_grouped_dev, dpf_pir_answer_grouped_sparse_dev,
dpf_pir_write_grouped_sparse_dev and the handle made by
dpf_pir_db_create_grouped_sparse).  Expected bits come from oracle.eval_batch
at each group's points, expected answers and DBs from numpy; never from the
code under test.  Both servers' shares are run.  Everything is bit-exact, with
guard bytes behind every output.

Every group has its own point list, the lists are pairwise disjoint, and every
group has a key that queries a point of its own list and of no other: a kernel
that read another group's list would answer zero where a record is expected.

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
GK = [(1, 1), (3, 2), (5, 5)]           # (groups, keys per group); 5 keys: two scatter passes


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert dpf.gpu_init(1) >= 1


def _dev(a):
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


def _absent(g, j):
    """Key j of group g asks for a keyword its group does not hold."""
    return (g + j) % 3 == 2


@functools.lru_cache(maxsize=None)
def _case(ng, kpg, nrec, logN):
    """(pts [ng][nrec], alphas [ng][kpg], ka, kb, selA, selB [ng * kpg][nrec]):
    pairwise disjoint point lists (inside a list the second point repeats the
    first from 3 records on, and the domain's ends appear from 5 on in group
    0), key pairs that query a point of their own group's list or, where
    _absent, of no list, and the oracle's selections of both shares at each
    key's own group's points."""
    rng = np.random.default_rng(ng * 7919 + kpg * 977 + nrec * 31 + logN)
    hi = 1 << logN
    while True:
        pts = rng.integers(1, hi - 1, (ng, nrec), dtype=np.uint64)
        if np.unique(pts).size == pts.size:
            break
    if nrec >= 3:
        pts[:, 1] = pts[:, 0]
    if nrec >= 5:
        pts[0, nrec - 1], pts[0, nrec // 2] = np.uint64(hi - 1), np.uint64(0)
    have = set(int(p) for p in pts.reshape(-1))
    alphas = np.zeros((ng, kpg), np.uint64)
    for g in range(ng):
        for j in range(kpg):
            if _absent(g, j):
                a = int(rng.integers(0, hi, dtype=np.uint64))
                while a in have:
                    a = int(rng.integers(0, hi, dtype=np.uint64))
                alphas[g, j] = a
            else:
                alphas[g, j] = pts[g, (j * 131) % nrec]
    # Present in its own group's list, absent from every other group's.
    for g in range(ng):
        for j in range(kpg):
            for o in range(ng):
                assert (alphas[g, j] in pts[o]) == (o == g and not _absent(g, j))
    nk = ng * kpg
    _, s0, s1 = synth.key_seeds(nk, logN, first=nrec + logN + 1000 * ng)
    ka, kb = dpf.gen_batch_seeded(alphas.reshape(-1), logN, s0, s1)
    own = np.repeat(pts, kpg, axis=0)                      # [nk][nrec]: every key's own list
    selA = oracle.eval_batch(ka, own, logN, nthreads=8).astype(bool)
    selB = oracle.eval_batch(kb, own, logN, nthreads=8).astype(bool)
    assert np.array_equal(selA ^ selB, own == alphas.reshape(-1, 1))
    for a in (pts, alphas, ka, kb, selA, selB):
        a.setflags(write=False)
    return pts, alphas, ka, kb, selA, selB


def _hit(pts, alphas):
    kpg = alphas.shape[1]
    return np.repeat(pts, kpg, axis=0) == alphas.reshape(-1, 1)


def _db(ng, nrec, rec):
    return np.random.default_rng(ng * 131 + nrec * 7 + rec).integers(0, 256, (ng, nrec, rec), dtype=np.uint8)


def _answers(db, sel):
    """[ng * kpg][rec]: key k of group g = k // kpg XORs the rows of db[g] that sel[k] selects."""
    ng, _, rec = db.shape
    kpg = sel.shape[0] // ng
    out = np.zeros((sel.shape[0], rec), np.uint8)
    for k in range(sel.shape[0]):
        if sel[k].any():
            out[k] = np.bitwise_xor.reduce(db[k // kpg][sel[k]], axis=0)
    return out


def _apply(db, sel, msgs):
    out = db.copy()
    kpg = sel.shape[0] // db.shape[0]
    for k in range(sel.shape[0]):
        out[k // kpg][sel[k]] ^= msgs[k]
    return out


def _sliced(db):
    """The grouped layout of db [ng][nrec][rec], GUARD bytes of 0x5A behind it."""
    import torch
    ng, nrec, rec = db.shape
    size = dpf.pir_db_grouped_size(ng, nrec, rec)
    buf = torch.full((size + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    dpf.pir_db_slice_grouped_dev(_dev(db), ng, nrec, rec, buf)
    torch.cuda.synchronize()
    return buf, size


def _flat(dbs, ng, nrec, rec):
    """The grouped layout read back as the flat DB [ng][group stride][rec]."""
    import torch
    gs = dpf.pir_group_stride(nrec)
    out = torch.empty(ng * gs * rec, dtype=torch.uint8, device="cuda")
    dpf.pir_db_unslice_any_dev(dbs, ng * gs, rec, out)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(ng, gs, rec)


# ---- dpf_eval_bits_grouped_dev ------------------------------------------------
def _rows(sel, stride):
    """sel [nk][npts] as packed rows of `stride` bytes, zero past npts."""
    out = np.zeros((sel.shape[0], stride), np.uint8)
    packed = np.packbits(sel, axis=1, bitorder="little")
    out[:, :packed.shape[1]] = packed
    return out


@pytest.mark.parametrize("logN", [30, 63])
@pytest.mark.parametrize("ng,kpg", GK)
@pytest.mark.parametrize("nrec", [1, 127, 128, 129, 257])
def test_eval_bits_grouped_dev(nrec, ng, kpg, logN):
    """Rows of span + 16 bytes: the span is the oracle's bits with zeros past
    npts, the 16 bytes behind it and the guard keep their poison.  The full
    workspace (frontier) and the expanded keys alone (root walks) give the
    same bits; one group gives dpf_eval_bits_dev's rows."""
    import torch
    pts, alphas, ka, kb, selA, selB = _case(ng, kpg, nrec, logN)
    nk = ng * kpg
    span = dpf.eval_bits_stride(nrec)
    stride = span + 16
    d_pts = _dev(pts)
    works = [dpf.eval_bits_workspace_size(nk, nrec, logN), dpf.eval_workspace_size(nk, 1, logN)]
    for keys, sel in ((ka, selA), (kb, selB)):
        want = _rows(sel, span)
        for wb in works:
            d_work = torch.empty(wb, dtype=torch.uint8, device="cuda")
            d_bits = torch.full((nk * stride + GUARD,), 0xC3, dtype=torch.uint8, device="cuda")
            dpf.eval_bits_grouped_dev(_dev(keys), keys.shape[1], ng, kpg, d_pts, nrec, logN, d_bits, stride, d_work)
            torch.cuda.synchronize()
            dpf.forget_workspace(d_work)
            b = d_bits.cpu().numpy()
            assert (b[nk * stride:] == 0xC3).all()
            rows = b[:nk * stride].reshape(nk, stride)
            assert (rows[:, span:] == 0xC3).all()
            assert np.array_equal(rows[:, :span], want), (nrec, ng, kpg, logN, wb)
        if ng == 1:
            d_work = torch.empty(works[0], dtype=torch.uint8, device="cuda")
            d_one = torch.zeros(nk * span, dtype=torch.uint8, device="cuda")
            dpf.eval_bits_dev(_dev(keys), keys.shape[1], nk, d_pts, nrec, logN, d_one, span, d_work)
            torch.cuda.synchronize()
            dpf.forget_workspace(d_work)
            assert np.array_equal(d_one.cpu().numpy().reshape(nk, span), want)


# ---- the composites -----------------------------------------------------------
NREC = [1, 128, 129, 256, 257, 600]
REC = [4, 20, 32, 100]
# Every nrec with every (groups, kpg); the widths and the two domains go round.
COMPOSITE = [(nrec, REC[(i + j) % 4], gk, (30, 63)[(i + j) % 2])
             for i, nrec in enumerate(NREC) for j, gk in enumerate(GK)]


@pytest.mark.parametrize("nrec,rec,gk,logN", COMPOSITE)
def test_answer_grouped_sparse_dev(nrec, rec, gk, logN):
    import torch
    ng, kpg = gk
    nk = ng * kpg
    pts, alphas, ka, kb, selA, selB = _case(ng, kpg, nrec, logN)
    db = _db(ng, nrec, rec)
    dbs, size = _sliced(db)
    d_pts = _dev(pts)
    ws = dpf.pir_grouped_sparse_workspace_size(ng, kpg, nrec, logN, rec)
    d_work = torch.full((ws + GUARD,), 0x77, dtype=torch.uint8, device="cuda")
    got = []
    for keys, sel in ((ka, selA), (kb, selB)):
        d_ans = torch.full((nk * rec + GUARD,), 0x33, dtype=torch.uint8, device="cuda")
        dpf.pir_answer_grouped_sparse_dev(_dev(keys), keys.shape[1], ng, kpg, logN, d_pts, dbs, nrec, rec, d_ans, d_work)
        torch.cuda.synchronize()
        a = d_ans.cpu().numpy()
        assert (a[nk * rec:] == 0x33).all()
        got.append(a[:nk * rec].reshape(nk, rec))
        assert np.array_equal(got[-1], _answers(db, sel))
    dpf.forget_workspace(d_work)
    # Two servers: the record(s) at the queried keyword of the queried group, zero for an absent keyword.
    x = got[0] ^ got[1]
    assert np.array_equal(x, _answers(db, _hit(pts, alphas)))
    for g in range(ng):
        for j in range(kpg):
            if _absent(g, j):
                assert not x[g * kpg + j].any()
            elif nrec < 3:
                assert np.array_equal(x[g * kpg + j], db[g, (j * 131) % nrec])
    assert (dbs.cpu().numpy()[size:] == 0x5A).all() and (d_work.cpu().numpy()[ws:] == 0x77).all()


@pytest.mark.parametrize("nrec,rec,gk,logN", COMPOSITE)
def test_write_grouped_sparse_dev(nrec, rec, gk, logN):
    """After one server's write the DB is the numpy dual; after the other's,
    the two shares have changed the DB at (g, alpha) only.  Flat positions
    [nrec, group stride) of every group stay zero."""
    import torch
    ng, kpg = gk
    nk = ng * kpg
    pts, alphas, ka, kb, selA, selB = _case(ng, kpg, nrec, logN)
    db = _db(ng, nrec, rec)
    msgs = np.random.default_rng(nk + rec).integers(0, 256, (nk, rec), dtype=np.uint8)
    msgs[0] = 0xFF
    dbs, size = _sliced(db)
    d_pts, d_msgs = _dev(pts), _dev(msgs)
    ws = dpf.pir_grouped_sparse_workspace_size(ng, kpg, nrec, logN, rec)
    d_work = torch.full((ws + GUARD,), 0x77, dtype=torch.uint8, device="cuda")
    dpf.pir_write_grouped_sparse_dev(_dev(ka), ka.shape[1], ng, kpg, logN, d_pts, d_msgs, dbs, nrec, rec, d_work)
    torch.cuda.synchronize()
    flat = _flat(dbs, ng, nrec, rec)
    assert np.array_equal(flat[:, :nrec], _apply(db, selA, msgs))
    assert not flat[:, nrec:].any()
    dpf.pir_write_grouped_sparse_dev(_dev(kb), kb.shape[1], ng, kpg, logN, d_pts, d_msgs, dbs, nrec, rec, d_work)
    torch.cuda.synchronize()
    dpf.forget_workspace(d_work)
    flat = _flat(dbs, ng, nrec, rec)
    assert np.array_equal(flat[:, :nrec], _apply(db, _hit(pts, alphas), msgs))
    assert not flat[:, nrec:].any()
    assert (dbs.cpu().numpy()[size:] == 0x5A).all() and (d_work.cpu().numpy()[ws:] == 0x77).all()


def test_empty_groups_and_empty_batches():
    """nrec == 0: the answer zeroes d_ans, the write is a no-op; no groups or no keys: nothing runs."""
    import torch
    logN, rec, ng, kpg = 30, 20, 3, 2
    _, _, ka, _, _, _ = _case(ng, kpg, 1, logN)
    d_work = torch.empty(dpf.pir_grouped_sparse_workspace_size(ng, kpg, 0, logN, rec), dtype=torch.uint8, device="cuda")
    d_ans = torch.full((ng * kpg * rec + GUARD,), 0x33, dtype=torch.uint8, device="cuda")
    dbs = torch.full((dpf.pir_db_grouped_size(ng, 0, rec),), 0x5A, dtype=torch.uint8, device="cuda")
    d_pts = torch.zeros(16, dtype=torch.uint8, device="cuda")
    dpf.pir_answer_grouped_sparse_dev(_dev(ka), ka.shape[1], ng, kpg, logN, d_pts, dbs, 0, rec, d_ans, d_work)
    torch.cuda.synchronize()
    a = d_ans.cpu().numpy()
    assert not a[:ng * kpg * rec].any() and (a[ng * kpg * rec:] == 0x33).all()
    d_ans.fill_(0x33)
    d_msgs = torch.full((ng * kpg * rec,), 0xFF, dtype=torch.uint8, device="cuda")
    dpf.pir_write_grouped_sparse_dev(_dev(ka), ka.shape[1], ng, kpg, logN, d_pts, d_msgs, dbs, 0, rec, d_work)
    dpf.pir_answer_grouped_sparse_dev(_dev(ka), ka.shape[1], 0, kpg, logN, d_pts, dbs, 5, rec, d_ans, d_work)
    dpf.pir_answer_grouped_sparse_dev(_dev(ka), ka.shape[1], ng, 0, logN, d_pts, dbs, 5, rec, d_ans, d_work)
    torch.cuda.synchronize()
    assert (d_ans.cpu().numpy() == 0x33).all() and (dbs.cpu().numpy() == 0x5A).all()


# ---- stream capture -------------------------------------------------------------
@pytest.mark.parametrize("write", [False, True])
def test_composites_in_a_stream_capture(write):
    """The composite run eagerly on a side stream, then captured on it (a
    linear chain: nothing executes during the capture), then replayed once:
    the replay leaves what the eager run left."""
    import torch
    ng, kpg, nrec, rec, logN = 3, 2, 257, 20, 30
    nk = ng * kpg
    pts, alphas, ka, kb, selA, selB = _case(ng, kpg, nrec, logN)
    db = _db(ng, nrec, rec)
    first, size = _sliced(db)
    dbs = first.clone()
    msgs = np.random.default_rng(5).integers(0, 256, (nk, rec), dtype=np.uint8)
    d_keys, d_pts, d_msgs = _dev(ka), _dev(pts), _dev(msgs)
    d_ans = torch.empty(nk * rec + GUARD, dtype=torch.uint8, device="cuda")
    d_work = torch.empty(dpf.pir_grouped_sparse_workspace_size(ng, kpg, nrec, logN, rec), dtype=torch.uint8, device="cuda")

    def load():
        dbs.copy_(first)
        d_ans.fill_(0xAB)
        torch.cuda.synchronize()

    def run(st):
        if write:
            dpf.pir_write_grouped_sparse_dev(d_keys, ka.shape[1], ng, kpg, logN, d_pts, d_msgs, dbs, nrec, rec, d_work,
                                             stream=st)
        else:
            dpf.pir_answer_grouped_sparse_dev(d_keys, ka.shape[1], ng, kpg, logN, d_pts, dbs, nrec, rec, d_ans, d_work,
                                              stream=st)

    def state():
        torch.cuda.synchronize()
        return dbs.cpu().numpy().copy(), d_ans.cpu().numpy().copy()

    S = torch.cuda.Stream()
    try:
        load()
        before = state()
        run(S)
        S.synchronize()
        eager = state()
        if write:
            assert np.array_equal(_flat(dbs, ng, nrec, rec)[:, :nrec], _apply(db, selA, msgs))
        else:
            assert np.array_equal(eager[1][:nk * rec].reshape(nk, rec), _answers(db, selA))
        assert (eager[0][size:] == 0x5A).all() and (eager[1][nk * rec:] == 0xAB).all()
        load()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=S):
            run(torch.cuda.current_stream())
        untouched = state()
        assert np.array_equal(untouched[0], before[0]) and np.array_equal(untouched[1], before[1])
        g.replay()
        replayed = state()
        assert np.array_equal(replayed[0], eager[0]) and np.array_equal(replayed[1], eager[1])
        del g
    finally:
        dpf.forget_workspace(d_work)


# ---- the handle -------------------------------------------------------------------
def _handle_checks(rec, ngpus=1):
    """A grouped keyword PirDB of 5 groups of 300 records at logN 40."""
    logN, ng, kpg, nrec = 40, 5, 2, 300
    nk = ng * kpg
    pts, alphas, ka, kb, selA, selB = _case(ng, kpg, nrec, logN)
    db = _db(ng, nrec, rec)
    pdb = dpf.PirDB(db, logN, ngpus=ngpus, rec_bytes=rec, points=pts, groups=ng)
    assert pdb.nrec == ng * nrec and pdb.ngroups == ng and pdb.rec_bytes == rec
    everything = np.arange(ng * nrec, dtype=np.uint64)
    flat = lambda d: d.reshape(ng * nrec, rec)
    assert np.array_equal(pdb.read(everything), flat(db))
    a, b = pdb.answer(ka), pdb.answer(kb)
    assert np.array_equal(a, _answers(db, selA)) and np.array_equal(b, _answers(db, selB))
    hit = _hit(pts, alphas)
    assert np.array_equal(a ^ b, _answers(db, hit))
    assert np.array_equal((a ^ b)[0], db[0, 0] ^ db[0, 1])           # a repeated point: both records together
    assert not (a ^ b)[kpg * 1 + 1].any() and _absent(1, 1)           # an absent keyword
    msgs = np.random.default_rng(rec).integers(0, 256, (nk, rec), dtype=np.uint8)
    pdb.write_grouped(ka, msgs)
    want = _apply(db, selA, msgs)
    assert np.array_equal(pdb.read(everything), flat(want))
    assert np.array_equal(pdb.answer(kb), _answers(want, selB))
    idx = np.array([0, 299, 300, 899, 900, 1499, 3, 300], np.uint64)  # group edges, both shards, one twice
    recs = np.random.default_rng(rec + 1).integers(0, 256, (idx.size, rec), dtype=np.uint8)
    pdb.update(idx, recs)
    for i, r in zip(idx, recs):
        flat(want)[int(i)] = r                                         # of repeated indices the last wins
    assert np.array_equal(pdb.read(idx), flat(want)[idx.astype(np.int64)])
    assert np.array_equal(pdb.export(), flat(want))
    assert np.array_equal(pdb.export(250, 700), flat(want)[250:950])
    assert np.array_equal(pdb.answer(ka), _answers(want, selA))
    other = np.random.default_rng(rec + 2).integers(0, 256, (700, rec), dtype=np.uint8)
    pdb.xor_records(other, first=250)
    flat(want)[250:950] ^= other
    assert np.array_equal(pdb.export(), flat(want))
    assert np.array_equal(pdb.answer(kb), _answers(want, selB))
    with pytest.raises(dpf.DPFPanic) as e:
        pdb.write(ka, msgs)
    assert e.value.code == dpf.DPF_ERR_PARAM
    for call in (lambda: pdb.answer(ka[:nk - 1]), lambda: pdb.write_grouped(ka[:nk - 1], msgs[:nk - 1]),
                 lambda: pdb.update(np.array([ng * nrec], np.uint64), recs[:1])):
        with pytest.raises(dpf.DPFPanic) as e:
            call()
        assert e.value.code == dpf.DPF_ERR_PARAM
    with pytest.raises(dpf.DPFPanic) as e:
        pdb.answer(ka[:, :16 + 18 * (logN - 7)])
    assert e.value.code == dpf.DPF_ERR_KEYLEN
    assert np.array_equal(pdb.export(), flat(want))                   # the refused calls changed nothing
    pdb.clear()
    assert not pdb.answer(ka).any() and not pdb.export().any()
    # The points survive clear: both shares written into the empty table leave the messages at the keywords.
    pdb.write_grouped(ka, msgs)
    pdb.write_grouped(kb, msgs)
    assert np.array_equal(pdb.export(), flat(_apply(np.zeros_like(db), hit, msgs)))
    pdb.close()
    assert pdb.nrec == 0 and pdb.ngroups == 0


@pytest.mark.parametrize("rec", [7, 32])
def test_grouped_sparse_handle(rec):
    _handle_checks(rec)


def test_grouped_sparse_handle_refusals():
    logN = 20
    db = _db(2, 2, 32)
    for bad in (1 << logN, (1 << 63) | 5):
        with pytest.raises(dpf.DPFPanic) as e:
            dpf.PirDB(db, logN, rec_bytes=32, points=np.array([1, 2, bad, 3], np.uint64), groups=2)
        assert e.value.code == dpf.DPF_ERR_PARAM
    with pytest.raises(ValueError):
        dpf.PirDB(db, logN, rec_bytes=32, points=np.array([1, 2, 3], np.uint64), groups=2)
    with pytest.raises(dpf.DPFPanic):
        dpf.PirDB(db, logN, ngpus=dpf.gpu_count() + 1, rec_bytes=32, points=np.array([1, 2, 3, 4], np.uint64), groups=2)
    # More records in a group than the domain has points: allowed, points repeat.
    many = dpf.PirDB(np.ones((2 * 200, 4), np.uint8), 7, rec_bytes=4, points=np.arange(400, dtype=np.uint64) % 128, groups=2)
    assert many.nrec == 400
    many.close()
    empty = dpf.PirDB(np.zeros((0, 32), np.uint8), logN, rec_bytes=32, points=np.zeros(0, np.uint64), groups=3)
    al, s0, s1 = synth.key_seeds(3, logN, first=4)
    ka, _ = dpf.gen_batch_seeded(al, logN, s0, s1)
    assert not empty.answer(ka).any()
    empty.close()


def test_two_shard_grouped_sparse_handle():
    """gpu_init_devices([0, 0]) and PirDB(..., ngpus=2, points=, groups=5):
    shards of 3 and 2 whole groups, each with its groups' points."""
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
