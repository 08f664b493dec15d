"""Grouped PIR with many keys per group: the matrix-core grouped fold
(k_fold_grouped_mfma) against the direct one (k_fold_grouped) and against
numpy, through dpf_pir_answer_grouped_dev, dpf_xor_fold_grouped_dev, the
grouped and grouped-sparse handles and dpf/buckets.py.

Every case runs three times: env DPF_GROUP_FOLD_ROUTE forced to mfma, forced
to direct, and unset (the route rule), and asserts through
dpf.fold_grouped_form_for which route ran.  The three runs must be byte-equal
and equal to the expectation, which comes from oracle.evalfull_batch /
oracle.eval_batch and numpy, never from the library.  Both servers' shares are
run: their answers XOR to the queried records.  Guard bytes behind d_ans,
d_work and d_dbs must be intact.  Everything is bit-exact."""
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
KNOB = "DPF_GROUP_FOLD_ROUTE"
D, M = dpf.FOLD_GROUPED_DIRECT, dpf.FOLD_GROUPED_MFMA
ROUTES = ("mfma", "direct", None)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert dpf.gpu_init(1) >= 1


def _dev(a):
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


def _set_route(monkeypatch, knob, ng, kpg, nrec, rec):
    """Set the knob (None: unset) and return the form the next call takes,
    having checked that its route is the forced one, or the rule's."""
    if knob is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, knob)
    form = dpf.fold_grouped_form_for(ng, kpg, nrec, rec)
    want = {"mfma": M, "direct": D, None: M if kpg >= 5 else D}[knob]
    assert form.route == want, (knob, form)
    return form


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


def _fold_dev(rows, stride, ng, kpg, dbs, nrec, rec):
    """dpf_xor_fold_grouped_dev on caller-made bit rows, with the same guards."""
    import torch
    nk = ng * kpg
    ws = dpf.xor_fold_grouped_workspace_size(ng, kpg, rec)
    d_work = torch.full((ws + GUARD,), 0x33, dtype=torch.uint8, device="cuda")
    d_ans = torch.full((nk * rec + GUARD,), 0x33, dtype=torch.uint8, device="cuda")
    dpf.xor_fold_grouped_dev(_dev(rows), stride, ng, kpg, dbs, nrec, rec, d_ans, d_work)
    torch.cuda.synchronize()
    a = d_ans.cpu().numpy()
    assert (a[nk * rec:] == 0x33).all() and (d_work[ws:].cpu().numpy() == 0x33).all()
    return a[:nk * rec].reshape(nk, rec)


# (logN, nrec): a key row of 4 words, shorter than a super-group; one whole
# super-group; two, the second nearly empty; four; twenty: several staged
# blocks, an odd rest, several runs when the groups are few.
SHAPES = [(7, 100), (8, 256), (9, 257), (10, 1000), (13, 5000)]
# One bit tile (waves without tiles only stage); 5 tiles; FULL; CG 2; a short last column; CG 4.
REC = [4, 20, 32, 64, 100, 128]
# Key tiles of 32 (8 live rows), 64 (33 live rows), 64 (full), 32 in many groups,
# 128 (100 live rows), 256 (129 live rows), and two key tiles, the second with 4 rows.
GROUPS = [(1, 8), (3, 33), (2, 64), (65, 9), (2, 100), (2, 129), (1, 260)]
# Every rec with every (ngroups, kpg), hence with every key-tile shape; the shapes cycle through them.
CASES = [(*SHAPES[(i + j) % len(SHAPES)], rec, ng, kpg) for i, rec in enumerate(REC) for j, (ng, kpg) in enumerate(GROUPS)]


def test_the_cases_cover_every_axis_and_pair():
    assert {c[:2] for c in CASES} == set(SHAPES) and {c[2] for c in CASES} == set(REC)
    assert {(c[2],) + c[3:] for c in CASES} == {(rec, ng, kpg) for rec in REC for ng, kpg in GROUPS}
    # ... and the forms they take on the matrix-core route: every tile shape's key count, CG 1, 2 and 4.
    forms = {(f.keys_per_tile, f.columns_per_wg)
             for f in (dpf.fold_grouped_form_for(ng, kpg, nrec, rec, cus=256) for _, nrec, rec, ng, kpg in CASES)}
    assert forms == {(32, 1), (32, 2), (32, 4), (64, 1), (128, 1), (128, 2), (256, 1)}


@pytest.mark.parametrize("logN,nrec,rec,ng,kpg", CASES)
def test_answer_grouped_many_keys(monkeypatch, logN, nrec, rec, ng, kpg):
    alphas, ka, kb, selA, selB = _case(logN, nrec, ng, kpg)
    db = _db(ng, nrec, rec)
    dbs, size = _grouped(db)
    wantA, wantB = _expect(db, selA, kpg), _expect(db, selB, kpg)
    queried = np.stack([db[r // kpg][int(alphas[r])] for r in range(ng * kpg)])
    assert np.array_equal(wantA ^ wantB, queried)
    for knob in ROUTES:
        form = _set_route(monkeypatch, knob, ng, kpg, nrec, rec)
        a = _answer_dev(ka, logN, ng, kpg, dbs, nrec, rec)
        b = _answer_dev(kb, logN, ng, kpg, dbs, nrec, rec)
        assert np.array_equal(a, wantA), (knob, form)              # so the three runs are byte-equal too
        assert np.array_equal(b, wantB), (knob, form)
        assert np.array_equal(a ^ b, queried)
    assert (dbs.cpu().numpy()[size:] == 0x5A).all()


@pytest.mark.parametrize("logN,nrec,rec,ng,kpg", [(9, 257, 20, 3, 2), (13, 5000, 100, 65, 1), (7, 100, 32, 65, 1)])
def test_forced_matrix_core_route_with_tiles_almost_empty(monkeypatch, logN, nrec, rec, ng, kpg):
    """One or two live rows in a tile of 32: the rows behind them are zeros, not the next group's keys."""
    alphas, ka, kb, selA, selB = _case(logN, nrec, ng, kpg)
    db = _db(ng, nrec, rec)
    dbs, size = _grouped(db)
    got = {}
    for knob in ROUTES:
        form = _set_route(monkeypatch, knob, ng, kpg, nrec, rec)
        assert form.keys_per_tile == (32 if knob == "mfma" else 4)
        got[knob] = (_answer_dev(ka, logN, ng, kpg, dbs, nrec, rec), _answer_dev(kb, logN, ng, kpg, dbs, nrec, rec))
        assert np.array_equal(got[knob][0], _expect(db, selA, kpg)) and np.array_equal(got[knob][1], _expect(db, selB, kpg))
    assert np.array_equal(got["mfma"][0], got["direct"][0]) and np.array_equal(got["mfma"][0], got[None][0])
    assert (dbs.cpu().numpy()[size:] == 0x5A).all()


@pytest.mark.parametrize("nrec,rec,extra,ng,kpg", [(100, 20, 16, 3, 33), (257, 4, 48, 65, 9), (1000, 100, 0, 2, 129),
                                                   (5000, 32, 112, 1, 260), (5000, 128, 16, 2, 100)])
def test_fold_grouped_on_caller_made_bits(monkeypatch, nrec, rec, extra, ng, kpg):
    """Random bit rows with a stride larger than the records need; the bits at
    positions >= nrec are random too and meet zero records only."""
    nk = ng * kpg
    stride = (nrec + 127) // 128 * 16 + extra
    rows = np.random.default_rng(nrec + rec + nk).integers(0, 256, (nk, stride), dtype=np.uint8)
    sel = np.unpackbits(rows, axis=1, bitorder="little")[:, :nrec].astype(bool)
    db = _db(ng, nrec, rec)
    dbs, size = _grouped(db)
    want = _expect(db, sel, kpg)
    for knob in ROUTES:
        form = _set_route(monkeypatch, knob, ng, kpg, nrec, rec)
        assert np.array_equal(_fold_dev(rows, stride, ng, kpg, dbs, nrec, rec), want), (knob, form)
    assert (dbs.cpu().numpy()[size:] == 0x5A).all()


@pytest.mark.parametrize("logN,nrec,rec,ng,kpg", [(13, 5000, 32, 2, 64), (10, 1000, 20, 65, 9), (13, 5000, 64, 1, 260)])
def test_answers_do_not_depend_on_the_fold_limits(monkeypatch, logN, nrec, rec, ng, kpg):
    """max_blocks 2 and 7 force many launches per key tile, max_sg 1 runs of
    one super-group (a partial staged block each, cleared answers and atomic
    XORs): the answers are those of the default plan and of numpy."""
    _, ka, _, selA, _ = _case(logN, nrec, ng, kpg)
    db = _db(ng, nrec, rec)
    dbs, _ = _grouped(db)
    want = _expect(db, selA, kpg)
    base = _set_route(monkeypatch, "mfma", ng, kpg, nrec, rec)
    assert np.array_equal(_answer_dev(ka, logN, ng, kpg, dbs, nrec, rec), want)
    try:
        for limits in ((2, 0), (7, 0), (0, 1)):
            dpf.set_fold_limits(*limits)
            for knob in ROUTES:
                form = _set_route(monkeypatch, knob, ng, kpg, nrec, rec)
                if knob == "mfma" and limits[0]:
                    assert form.max_blocks == limits[0] and form.launches > base.launches
                if knob == "mfma" and limits[1]:
                    assert form.sg_per_run == 1 and form.atomic == (nrec > 256) and form.runs == (nrec + 255) // 256
                assert np.array_equal(_answer_dev(ka, logN, ng, kpg, dbs, nrec, rec), want), (limits, knob, form)
    finally:
        dpf.set_fold_limits(0, 0)


def test_a_captured_fold_replays_its_clear(monkeypatch):
    """dpf_xor_fold_grouped_dev on the matrix-core route with several runs per
    group, captured once: the clear of the answers is part of the graph, so
    each replay over poisoned answers is exact."""
    import torch
    ng, kpg, nrec, rec = 2, 64, 5000, 32
    form = _set_route(monkeypatch, "mfma", ng, kpg, nrec, rec)
    assert form.runs > 1 and form.atomic
    nk, stride = ng * kpg, (nrec + 127) // 128 * 16
    rows = np.random.default_rng(77).integers(0, 256, (nk, stride), dtype=np.uint8)
    sel = np.unpackbits(rows, axis=1, bitorder="little")[:, :nrec].astype(bool)
    db = _db(ng, nrec, rec)
    dbs, size = _grouped(db)
    want = _expect(db, sel, kpg)
    ws = dpf.xor_fold_grouped_workspace_size(ng, kpg, rec)
    d_work = torch.full((ws + GUARD,), 0x33, dtype=torch.uint8, device="cuda")
    d_ans = torch.full((nk * rec + GUARD,), 0x33, dtype=torch.uint8, device="cuda")
    d_bits = _dev(rows)
    S = torch.cuda.Stream()
    run = lambda st: dpf.xor_fold_grouped_dev(d_bits, stride, ng, kpg, dbs, nrec, rec, d_ans, d_work, stream=st)
    run(S)                                                          # eager on the side stream first
    S.synchronize()
    torch.cuda.synchronize()
    assert np.array_equal(d_ans.cpu().numpy()[:nk * rec].reshape(nk, rec), want)
    d_ans.fill_(0x33)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=S):
        run(torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert (d_ans.cpu().numpy() == 0x33).all()                      # captured, not run
    for poison in (0xA5, 0xFF):
        d_ans.fill_(poison)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        a = d_ans.cpu().numpy()
        assert np.array_equal(a[:nk * rec].reshape(nk, rec), want), poison
        assert (a[nk * rec:] == poison).all() and (d_work[ws:].cpu().numpy() == 0x33).all()
    del g
    assert (dbs.cpu().numpy()[size:] == 0x5A).all()


def test_grouped_handle_with_16_keys_per_group(monkeypatch):
    logN, nrec, ng, kpg, rec = 9, 300, 7, 16, 20
    alphas, ka, kb, selA, selB = _case(logN, nrec, ng, kpg)
    db = _db(ng, nrec, rec)
    pdb = dpf.PirDB(db, logN, rec_bytes=rec, groups=ng)
    try:
        for knob in ROUTES:
            _set_route(monkeypatch, knob, ng, kpg, nrec, rec)
            a, b = pdb.answer(ka), pdb.answer(kb)
            assert np.array_equal(a, _expect(db, selA, kpg)) and np.array_equal(b, _expect(db, selB, kpg)), knob
            assert np.array_equal(a ^ b, np.stack([db[r // kpg][int(alphas[r])] for r in range(ng * kpg)]))
    finally:
        pdb.close()


def test_grouped_sparse_handle_with_9_keys_per_group(monkeypatch):
    """Records at points of a 2^40 domain; expected bits from oracle.eval_batch at each key's own group's points."""
    logN, nrec, ng, kpg, rec = 40, 300, 5, 9, 36
    rng = np.random.default_rng(4049)
    pts = rng.integers(0, 1 << logN, (ng, nrec), dtype=np.uint64)
    assert np.unique(pts).size == pts.size
    alphas = np.stack([pts[g, (np.arange(kpg) * 131) % nrec] for g in range(ng)])
    _, s0, s1 = synth.key_seeds(ng * kpg, logN, first=91)
    ka, kb = dpf.gen_batch_seeded(alphas.reshape(-1), logN, s0, s1)
    own = np.repeat(pts, kpg, axis=0)
    selA = oracle.eval_batch(ka, own, logN, nthreads=8).astype(bool)
    selB = oracle.eval_batch(kb, own, logN, nthreads=8).astype(bool)
    assert np.array_equal(selA ^ selB, own == alphas.reshape(-1, 1))
    db = _db(ng, nrec, rec)
    pdb = dpf.PirDB(db, logN, rec_bytes=rec, points=pts, groups=ng)
    try:
        for knob in ROUTES:
            _set_route(monkeypatch, knob, ng, kpg, nrec, rec)
            a, b = pdb.answer(ka), pdb.answer(kb)
            assert np.array_equal(a, _expect(db, selA, kpg)) and np.array_equal(b, _expect(db, selB, kpg)), knob
            assert np.array_equal(a ^ b, np.stack([db[g, (j * 131) % nrec] for g in range(ng) for j in range(kpg)]))
    finally:
        pdb.close()


def test_nine_clients_over_twelve_buckets_end_to_end(monkeypatch):
    """dpf/buckets.py: 9 clients, each wanting 8 of 3000 records, send one key
    pair per bucket; the server answers all of them as 9 keys per group."""
    n, rec, nb, ncl = 3000, 20, 12, 9
    db = np.random.default_rng(5).integers(0, 256, (n, rec), dtype=np.uint8)
    lay = buckets.layout(n, nb, seed=3)
    bdb, logN = buckets.build(db, lay)
    got, ka, kb = [], [], []
    for c in range(ncl):
        wanted = np.random.default_rng(100 + c).choice(n, 8, replace=False)
        got.append(buckets.assign(wanted, lay))
        assert sorted(got[-1].values()) == sorted(int(w) for w in wanted)
        _, s0, s1 = synth.key_seeds(nb, logN, first=17 + 100 * c)
        a, b = dpf.gen_batch_seeded(buckets.alphas(got[-1], lay), logN, s0, s1)
        ka.append(a)
        kb.append(b)
    pdb = dpf.PirDB(bdb, logN, rec_bytes=rec, groups=nb)
    try:
        for knob in ROUTES:
            _set_route(monkeypatch, knob, nb, ncl, lay.cap, rec)
            x = buckets.split_answers(pdb.answer(buckets.merge_clients(ka)) ^ pdb.answer(buckets.merge_clients(kb)), ncl)
            for c in range(ncl):
                for b, r in got[c].items():
                    assert np.array_equal(x[c, b], db[r]), (knob, c, b)
                for b in set(range(nb)) - set(got[c]):
                    assert np.array_equal(x[c, b], bdb[b, 0])       # the dummy query of an unused bucket
    finally:
        pdb.close()
