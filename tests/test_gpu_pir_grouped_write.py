"""Grouped private writes: one scatter launch XORs messages into many small
DBs (groups), each under its own keys (dpf_xor_scatter_grouped_dev,
dpf_pir_write_grouped_dev, dpf_pir_db_write_grouped / PirDB.write_grouped).

The expected DB is computed in numpy: pir_ref.xor_scatter per group over the
caller's [ngroups][nrec][rec] array, then pir_ref.layout(pir_ref.grouped_flat)
-- never by the code under test, and the device DB itself is loaded from that
layout, not made by the slice entry.  The WHOLE sliced buffer is compared,
every group's padding included, with guard bytes behind it.  Selection rows
of the composites come from oracle.evalfull_batch.  Everything is bit-exact.

Which branch of the plan and of the kernel a shape reaches is asserted through
the plan (dpf.scatter_grouped_form_for), not assumed.

The two-shard handle needs a process of its own (the device registry is
process-wide): the test at the end runs this file as a script."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "dpf-go_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import dpf                  # noqa: E402
from dpf import buckets     # noqa: E402
from dpf import synth       # noqa: E402
import oracle               # noqa: E402
import pir_ref as ref       # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 256
G, L = dpf.SCATTER_GROUPED, dpf.SCATTER_LOOP


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert dpf.gpu_init(1) >= 1


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _dev(a):
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


@functools.lru_cache(maxsize=None)
def _rand(tag, *shape):
    return _frozen(np.random.default_rng([tag, *shape]).integers(0, 256, shape, dtype=np.uint8))


def _sliced(db):
    """The grouped sliced layout of db [ng][nrec][rec] from its definition."""
    return ref.layout(ref.grouped_flat(db))


def _scattered(db, rows, msgs, kpg):
    """db [ng][nrec][rec] after the grouped write of rows / msgs [ng * kpg]: numpy, group by group."""
    nrec = db.shape[1]
    return np.stack([ref.xor_scatter(db[g], rows[g * kpg:(g + 1) * kpg], msgs[g * kpg:(g + 1) * kpg], nrec)
                     for g in range(db.shape[0])])


def _load(db):
    """A device buffer holding the grouped layout of db, GUARD bytes of 0x5A behind it."""
    import torch
    ng, nrec, rec = db.shape
    lay = _sliced(db)
    assert lay.size == dpf.pir_db_grouped_size(ng, nrec, rec) == ng * dpf.pir_group_stride(nrec) * rec
    buf = torch.full((lay.size + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    buf[:lay.size].copy_(torch.from_numpy(lay.copy()))
    return buf, lay.size


def _same(buf, size, db):
    """The whole buffer is the layout of db (padding included) and the guard is intact."""
    got = buf.cpu().numpy()
    assert (got[size:] == 0x5A).all(), "bytes past the DB were written"
    return np.array_equal(got[:size], _sliced(db))


# ---- scatter from caller-made bits ----------------------------------------------
# (ng, nrec, rec, kpg, stride, limits, what the plan must say).  The smallest
# shapes that reach every branch of the plan and of the kernel:
#   nrec 1 (stride 16: a row of 4 words, fewer than a super-group's 8), 255,
#   256, 257, 300 (stride 48: 12 words, no multiple of 8), 600 (3 super-groups:
#   a group splits into runs), 1100 (5 super-groups: with 1100 groups a run
#   is several super-groups long, and max_sg = 2 forces runs of 2, 2 and 1);
#   rec 4 and 12 (a short only column), 28 (message rows not 16-byte aligned),
#   32, 36 (a short last column of 32 rows), 96, 160 (more than 4 columns);
#   kpg 1, 2, 3, 4 (one pass of each width), 5, 7, 9 (passes of 4 and a last
#   one of 1, 3 and 1), 70 on the loop route (past the dense scatter's 64-key tile);
#   300 groups under max_blocks = 8: several launches per pass.
def W(*widths):
    """The form's pass_widths: bit w - 1 for a key pass of width w."""
    return sum(1 << (w - 1) for w in set(widths))


def _passes(widths, n):
    return lambda f: f.route == G and f.pass_widths == widths and f.passes == n


CASES = [
    pytest.param(1, 1, 4, 1, 16, (0, 0), _passes(W(1), 1), id="one-record"),
    pytest.param(2, 255, 12, 2, 32, (0, 0), _passes(W(2), 1), id="255x12-kpg2"),
    pytest.param(7, 256, 28, 3, 32, (0, 0), _passes(W(3), 1), id="256x28-kpg3"),
    pytest.param(7, 257, 32, 4, 48, (0, 0), lambda f: _passes(W(4), 1)(f) and f.columns == 1, id="257x32-kpg4"),
    pytest.param(7, 300, 36, 5, 48, (0, 0), lambda f: _passes(W(4, 1), 2)(f) and f.columns == 2, id="300x36-kpg5"),
    pytest.param(7, 300, 96, 7, 80, (0, 0), _passes(W(4, 3), 2), id="300x96-kpg7"),
    pytest.param(7, 600, 160, 9, 80, (0, 0),
                 lambda f: _passes(W(4, 1), 3)(f) and f.columns == 5 and f.runs > 1, id="600x160-kpg9-runs"),
    pytest.param(65, 255, 12, 9, 32, (0, 0), lambda f: _passes(W(4, 1), 3)(f) and f.launches == 3, id="65-groups-kpg9"),
    pytest.param(1, 600, 32, 70, 80, (0, 0), lambda f: f.route == L, id="loop-kpg70"),
    pytest.param(2, 600, 36, 70, 80, (0, 0), lambda f: f.route == L, id="loop-kpg70-rec36"),
    pytest.param(300, 257, 32, 5, 48, (8, 0),
                 lambda f: _passes(W(4, 1), 2)(f) and f.max_blocks == 8 and f.launches > 2 * f.passes, id="300-groups-max-blocks-8"),
    pytest.param(7, 1100, 36, 7, 144, (8, 0),
                 lambda f: _passes(W(4, 3), 2)(f) and f.runs == 5 and f.launches > f.passes, id="1100-max-blocks-8"),
    # Groups enough that a workgroup walks several super-groups (the next one's loads in flight):
    # runs of 3 and 2 on the 256 CUs of an MI355X; max_sg = 2 cuts them to 2, 2 and 1.
    pytest.param(1100, 1100, 4, 3, 144, (0, 0), lambda f: _passes(W(3), 1)(f) and f.sg_per_run >= 2, id="1100-groups-long-runs"),
    pytest.param(1100, 1100, 4, 3, 144, (8, 2),
                 lambda f: _passes(W(3), 1)(f) and f.sg_per_run == 2 and f.runs == 3 and f.max_blocks == 8, id="1100-groups-max-sg-2"),
]


@pytest.mark.parametrize("ones", [False, True], ids=["random-rows", "all-ones"])
@pytest.mark.parametrize("ng,nrec,rec,kpg,stride,limits,plan_says", CASES)
def test_scatter_grouped_on_caller_made_bits(ng, nrec, rec, kpg, stride, limits, plan_says, ones):
    """Random rows (random past nrec and past the records' last word too) and
    rows of all ones: the whole buffer equals numpy's, so every group's
    padding stayed zero whatever the bits said."""
    import torch
    nk = ng * kpg
    assert stride % 16 == 0 and stride * 8 >= nrec
    rows = np.full((nk, stride), 0xFF, np.uint8) if ones else _rand(1, nk, stride)
    msgs = _rand(2, nk, rec)
    db = _rand(3, ng, nrec, rec)
    want = _scattered(db, rows, msgs, kpg)
    buf, size = _load(db)
    d_rows, d_msgs = _dev(rows), _dev(msgs)
    try:
        dpf.set_fold_limits(*limits)
        form = dpf.scatter_grouped_form_for(ng, kpg, nrec, rec)
        assert plan_says(form), form
        dpf.xor_scatter_grouped_dev(d_rows, stride, ng, kpg, d_msgs, buf, nrec, rec)
        torch.cuda.synchronize()
    finally:
        dpf.set_fold_limits(0, 0)
    assert _same(buf, size, want)
    assert np.array_equal(d_rows.cpu().numpy(), rows.reshape(-1)) and np.array_equal(d_msgs.cpu().numpy(), msgs.reshape(-1))


def test_dummy_keys_and_empty_calls_change_nothing():
    import torch
    ng, nrec, rec, kpg, stride = 7, 300, 36, 3, 48
    db = _rand(4, ng, nrec, rec)
    buf, size = _load(db)
    rows = _dev(np.full((ng * kpg, stride), 0xFF, np.uint8))
    dpf.xor_scatter_grouped_dev(rows, stride, ng, kpg, _dev(np.zeros((ng * kpg, rec), np.uint8)), buf, nrec, rec)
    msgs = _dev(_rand(5, ng * kpg, rec))
    dpf.xor_scatter_grouped_dev(rows, stride, 0, kpg, msgs, buf, nrec, rec)
    dpf.xor_scatter_grouped_dev(rows, stride, ng, 0, msgs, buf, nrec, rec)
    dpf.xor_scatter_grouped_dev(rows, stride, ng, kpg, msgs, buf, 0, rec)
    torch.cuda.synchronize()
    assert _same(buf, size, db)


# ---- the composite: tree pass + scatter ---------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(logN, nrec, ng, kpg):
    """(alphas, ka, kb, rowsA, rowsB): ng * kpg key pairs in group order at
    points below nrec (the first and the last record among them) and the
    oracle's EvalFull rows of both shares."""
    nk = ng * kpg
    rng = np.random.default_rng(logN * 1009 + nrec * 31 + ng * 7 + kpg)
    alphas = rng.integers(0, nrec, nk, dtype=np.uint64)
    alphas[0], alphas[nk - 1] = 0, nrec - 1
    _, s0, s1 = synth.key_seeds(nk, logN, first=nrec + ng + 3)
    ka, kb = dpf.gen_batch_seeded(alphas, logN, s0, s1)
    rows = [oracle.evalfull_batch(k, logN, nthreads=8) for k in (ka, kb)]
    return tuple(_frozen(a) for a in (alphas, ka, kb, rows[0], rows[1]))


def _write_dev(keys, logN, ng, kpg, msgs, buf, nrec, rec):
    """dpf_pir_write_grouped_dev with a guard behind d_work."""
    import torch
    ws = dpf.pir_grouped_workspace_size(ng, kpg, logN, rec)
    d_work = torch.full((ws + GUARD,), 0x33, dtype=torch.uint8, device="cuda")
    dpf.pir_write_grouped_dev(_dev(keys), keys.shape[1], ng, kpg, logN, _dev(msgs), buf, nrec, rec, d_work)
    torch.cuda.synchronize()
    dpf.forget_workspace(d_work)
    assert (d_work[ws:].cpu().numpy() == 0x33).all()


@pytest.mark.parametrize("aes", ["ttable", "bitsliced"])
@pytest.mark.parametrize("logN,nrec,rec", [(7, 100, 20), (9, 300, 36), (12, 3000, 32)])
def test_pir_write_grouped_dev(logN, nrec, rec, aes):
    """Both servers apply the same messages under their key shares: each DB is
    the numpy scatter of the oracle's EvalFull rows, and the XOR of the two
    DBs differs from before by m_k at (g, alpha_k) only."""
    ng, kpg = 3, 5
    alphas, ka, kb, rowsA, rowsB = _case(logN, nrec, ng, kpg)
    msgs = _rand(6, ng * kpg, rec)
    db = [_rand(7 + s, ng, nrec, rec) for s in (0, 1)]
    after = []
    prev = dpf.set_aes_impl(aes)
    try:
        for s, (keys, rows) in enumerate(((ka, rowsA), (kb, rowsB))):
            buf, size = _load(db[s])
            _write_dev(keys, logN, ng, kpg, msgs, buf, nrec, rec)
            want = _scattered(db[s], rows, msgs, kpg)
            assert _same(buf, size, want), (aes, s)
            after.append(buf.cpu().numpy()[:size])
    finally:
        dpf.set_aes_impl(prev)
    delta = np.zeros((ng, nrec, rec), np.uint8)
    for r in range(ng * kpg):
        delta[r // kpg, int(alphas[r])] ^= msgs[r]
    assert np.array_equal(after[0] ^ after[1], _sliced(db[0] ^ db[1] ^ delta))


def test_grouped_write_agrees_with_what_exists():
    """The grouped write equals a loop of dpf_pir_write_sliced_any_dev over each
    group's flat range; with both shares applied to one DB the records at
    (g, alpha_k) changed by m_k, and dpf_pir_answer_grouped_dev reads them back."""
    import torch
    logN, nrec, rec, ng, kpg = 9, 300, 20, 3, 4          # kpg * rec = 80: every group's messages 16-byte aligned
    alphas, ka, kb, rowsA, rowsB = _case(logN, nrec, ng, kpg)
    alphas = alphas.copy()
    msgs = _rand(9, ng * kpg, rec)
    db = _rand(10, ng, nrec, rec)
    gs, kl = dpf.pir_group_stride(nrec), ka.shape[1]
    one, size = _load(db)
    loop, _ = _load(db)
    d_msgs = _dev(msgs)
    w = torch.empty(dpf.pir_workspace_size(kpg, logN), dtype=torch.uint8, device="cuda")
    for keys in (ka, kb):
        _write_dev(keys, logN, ng, kpg, msgs, one, nrec, rec)
        d_keys = _dev(keys)
        for g in range(ng):
            dpf.pir_write_sliced_any_dev(d_keys[g * kpg * kl:(g + 1) * kpg * kl], kl, kpg, logN,
                                         d_msgs[g * kpg * rec:(g + 1) * kpg * rec], loop[g * gs * rec:(g + 1) * gs * rec],
                                         nrec, rec, w)
        torch.cuda.synchronize()
        assert torch.equal(one, loop)
    dpf.forget_workspace(w)
    want = db.copy()
    for r in range(ng * kpg):
        want[r // kpg, int(alphas[r])] ^= msgs[r]
    assert _same(one, size, want)
    ws = dpf.pir_grouped_workspace_size(ng, kpg, logN, rec)
    d_work = torch.empty(ws, dtype=torch.uint8, device="cuda")
    ans = []
    for keys in (ka, kb):
        d_ans = torch.empty(ng * kpg * rec, dtype=torch.uint8, device="cuda")
        dpf.pir_answer_grouped_dev(_dev(keys), kl, ng, kpg, logN, one, nrec, rec, d_ans, d_work)
        torch.cuda.synchronize()
        ans.append(d_ans.cpu().numpy().reshape(ng * kpg, rec))
    dpf.forget_workspace(d_work)
    assert np.array_equal(ans[0] ^ ans[1], np.stack([want[r // kpg, int(alphas[r])] for r in range(ng * kpg)]))


# ---- the handle ------------------------------------------------------------------------
def _handle_checks(rec, ng, ngpus=1):
    """A grouped PirDB of ng groups of 300 records at logN 9, 3 keys per group:
    write_grouped under both shares, read everything and answer against numpy;
    then the refusals, after which the DB is unchanged."""
    logN, nrec, kpg = 9, 300, 3
    alphas, ka, kb, rowsA, rowsB = _case(logN, nrec, ng, kpg)
    db = _rand(11, ng, nrec, rec)
    msgs = _rand(12, ng * kpg, rec)
    pdb = dpf.PirDB(db, logN, ngpus=ngpus, rec_bytes=rec, groups=ng)
    everything = np.arange(ng * nrec, dtype=np.uint64)
    pdb.write_grouped(ka, msgs)
    want = _scattered(db, rowsA, msgs, kpg)
    assert np.array_equal(pdb.read(everything), want.reshape(ng * nrec, rec))
    sel = [np.unpackbits(r, axis=1, bitorder="little")[:, :nrec].astype(bool) for r in (rowsA, rowsB)]
    assert np.array_equal(pdb.answer(ka), ref.grouped_expect(want, sel[0], kpg))
    pdb.write_grouped(kb, msgs)                                  # the other share: (g, alpha_k) ^= m_k is what is left
    want = db.copy()
    for r in range(ng * kpg):
        want[r // kpg, int(alphas[r])] ^= msgs[r]
    assert np.array_equal(pdb.read(everything), want.reshape(ng * nrec, rec))
    assert np.array_equal(pdb.answer(ka) ^ pdb.answer(kb), np.stack([want[r // kpg, int(alphas[r])] for r in range(ng * kpg)]))
    pdb.write_grouped(ka[:0], msgs[:0])                          # nothing to do
    if ng > 1:
        with pytest.raises(dpf.DPFPanic) as ex:
            pdb.write_grouped(ka[:ng * kpg - 1], msgs[:ng * kpg - 1])   # not a multiple of the groups
        assert ex.value.code == dpf.DPF_ERR_PARAM
    with pytest.raises(dpf.DPFPanic) as ex:
        pdb.write_grouped(ka[:, :16 + 18 * (logN - 7)], msgs)
    assert ex.value.code == dpf.DPF_ERR_KEYLEN
    with pytest.raises(dpf.DPFPanic) as ex:
        pdb.write(ka, msgs)                                      # the dense write still refuses a grouped handle
    assert ex.value.code == dpf.DPF_ERR_PARAM and "dpf_pir_db_write_grouped" in str(ex.value)
    assert np.array_equal(pdb.read(everything), want.reshape(ng * nrec, rec))
    pdb.close()


@pytest.mark.parametrize("rec", [7, 32])
def test_grouped_handle_write(rec):
    _handle_checks(rec, 7)


def test_other_handles_refuse_a_grouped_write():
    db = _rand(13, 300, 32)
    pdb = dpf.PirDB(db, 9, rec_bytes=32)
    _, ka, _, _, _ = _case(9, 300, 1, 3)
    with pytest.raises(dpf.DPFPanic) as ex:
        pdb.write_grouped(ka, np.zeros((3, 32), np.uint8))
    assert ex.value.code == dpf.DPF_ERR_PARAM
    assert np.array_equal(pdb.read(np.arange(300, dtype=np.uint64)), db)
    pdb.close()


def test_batch_code_write_then_read():
    """dpf/buckets.py both ways over one grouped PirDB: 2000 records of 20
    bytes, 3-fold replicated in 12 buckets.  A client XORs deltas into 8
    records by writing every replica (write_plan: kpg short keys per bucket,
    dummies in the unused slots), then reads them back with one key per bucket.
    One handle stands for the pair of servers: both key shares are applied to
    it, which leaves what the two servers hold in XOR."""
    n, rec, nb, m, seed = 2000, 20, 12, 8, 3
    db = np.random.default_rng(5).integers(0, 256, (n, rec), dtype=np.uint8)
    lay = buckets.layout(n, nb, seed=seed)
    bdb, logN = buckets.build(db, lay)
    wanted = np.random.default_rng(seed).choice(n, m, replace=False)
    deltas = {int(r): np.random.default_rng(int(r)).integers(1, 256, rec, dtype=np.uint8) for r in wanted}
    need = np.bincount(lay.bucket[wanted].reshape(-1), minlength=nb).max()       # replicas in the fullest bucket
    assert need >= 2                                                            # 24 replicas, 12 buckets
    with pytest.raises(buckets.BucketOverflow):
        buckets.write_plan(deltas, lay, int(need) - 1)
    kpg = int(need)
    al, msgs = buckets.write_plan(deltas, lay, kpg)
    cover = buckets.write_plan({}, lay, kpg, rec_bytes=rec)                     # an all-dummy batch: cover traffic
    assert cover[0].shape == (nb, kpg) and cover[1].shape == (nb, kpg, rec) and not cover[1].any()
    assert al.shape == (nb, kpg) and msgs.shape == (nb, kpg, rec)
    assert int((msgs.reshape(nb * kpg, rec).any(axis=1)).sum()) == 3 * m        # the others are dummies
    _, s0, s1 = synth.key_seeds(nb * kpg, logN, first=23)
    wa, wb = dpf.gen_batch_seeded(al.reshape(-1), logN, s0, s1)
    pdb = dpf.PirDB(bdb, logN, rec_bytes=rec, groups=nb)
    pdb.write_grouped(wa, cover[1])                                             # changes nothing
    assert np.array_equal(pdb.read(np.arange(nb * lay.cap, dtype=np.uint64)), bdb.reshape(nb * lay.cap, rec))
    pdb.write_grouped(wa, msgs)
    pdb.write_grouped(wb, msgs)
    new = db.copy()
    for r, d in deltas.items():
        new[r] ^= d
    want_bdb, _ = buckets.build(new, lay)
    assert np.array_equal(pdb.read(np.arange(nb * lay.cap, dtype=np.uint64)), want_bdb.reshape(nb * lay.cap, rec))
    got = buckets.assign(wanted, lay)
    _, s0, s1 = synth.key_seeds(nb, logN, first=17)
    ra, rb = dpf.gen_batch_seeded(buckets.alphas(got, lay), logN, s0, s1)
    x = pdb.answer(ra) ^ pdb.answer(rb)
    pdb.close()
    assert sorted(got.values()) == sorted(int(w) for w in wanted)
    for b, r in got.items():
        assert np.array_equal(x[b], db[r] ^ deltas[r])                          # old XOR delta


# ---- the stream contract ------------------------------------------------------------
def _protocol(name, bufs, sets, want, run, work=None):
    """tests/test_gpu_stream_capture.py's protocol for an in-place operation:
    set A eager on a side stream; the same call captured in global mode, during
    which nothing may execute (the DB keeps its initial state); the graph
    replayed over set B, then over A again.  XOR makes a second application
    visible, and an answer for B that equals A's was baked on the host."""
    import torch

    def load(s):
        for k, a in sets[s].items():
            bufs[k][:a.size].copy_(torch.from_numpy(a.copy()))
        torch.cuda.synchronize()

    def holds(k, a):
        return np.array_equal(bufs[k].cpu().numpy()[:a.size], a)

    S = torch.cuda.Stream()
    try:
        load(0)
        run(S)
        S.synchronize()
        torch.cuda.synchronize()
        assert holds("db", want[0]), (name, "eager")
        load(0)
        g = torch.cuda.CUDAGraph()
        failed = ended = None
        try:
            with torch.cuda.graph(g, stream=S):
                try:
                    run(torch.cuda.current_stream())
                except dpf.DPFPanic as e:
                    failed = e
        except RuntimeError as e:              # the capture itself was invalidated
            ended = e
        if failed is not None:
            pytest.fail("%s failed in a stream capture: code %d, dpf_last_error: %s" % (name, failed.code, failed))
        assert ended is None, (name, "the capture did not end cleanly", str(ended))
        torch.cuda.synchronize()
        assert holds("db", sets[0]["db"]), (name, "changed while the call was only being captured")
        for s in (1, 0):
            load(s)
            g.replay()
            torch.cuda.synchronize()
            assert holds("db", want[s]), (name, "replay over set %s" % "AB"[s])
            assert (bufs["db"].cpu().numpy()[want[s].size:] == 0x5A).all(), (name, "bytes past the DB")
        del g
    finally:
        if work is not None:
            dpf.forget_workspace(work)


def _stream_bufs(sets):
    import torch
    bufs = {}
    for k, a in sets[0].items():
        assert a.size == sets[1][k].size
        bufs[k] = torch.full((a.size + (GUARD if k == "db" else 0),), 0x5A, dtype=torch.uint8, device="cuda")
    return bufs


@pytest.mark.parametrize("ng,nrec,rec,kpg,stride,limits,route", [
    pytest.param(7, 600, 36, 7, 80, (0, 0), G, id="grouped"),
    pytest.param(7, 600, 36, 7, 80, (2, 1), G, id="grouped-limits"),
    pytest.param(2, 600, 36, 70, 80, (0, 0), L, id="loop"),
])
def test_scatter_grouped_dev_is_stream_ordered_and_capturable(ng, nrec, rec, kpg, stride, limits, route):
    nk = ng * kpg
    sets, want = [], []
    for s in (0, 1):
        db, rows, msgs = _rand(20 + s, ng, nrec, rec), _rand(22 + s, nk, stride), _rand(24 + s, nk, rec)
        sets.append({"db": _sliced(db), "bits": rows.reshape(-1), "msgs": msgs.reshape(-1)})
        want.append(_sliced(_scattered(db, rows, msgs, kpg)))
    b = _stream_bufs(sets)
    try:
        dpf.set_fold_limits(*limits)
        assert dpf.scatter_grouped_form_for(ng, kpg, nrec, rec).route == route
        _protocol("dpf_xor_scatter_grouped_dev", b, sets, want,
                  lambda st: dpf.xor_scatter_grouped_dev(b["bits"], stride, ng, kpg, b["msgs"], b["db"], nrec, rec, stream=st))
    finally:
        dpf.set_fold_limits(0, 0)


@pytest.mark.parametrize("aes,logN,nrec", [("ttable", 9, 300), ("bitsliced", 13, 6000)])
def test_pir_write_grouped_dev_is_stream_ordered_and_capturable(aes, logN, nrec):
    """At logN 13 the byte-sliced back end runs its own tree (from 2^6 leaf blocks a key)."""
    import torch
    ng, kpg, rec = 3, 5, 20
    cases = (_case(logN, nrec, ng, kpg), _case(logN, nrec - 1, ng, kpg))      # two key sets of one shape
    sets, want = [], []
    for s in (0, 1):
        db, msgs = _rand(26 + s, ng, nrec, rec), _rand(28 + s, ng * kpg, rec)
        sets.append({"db": _sliced(db), "keys": cases[s][1].reshape(-1), "msgs": msgs.reshape(-1)})
        want.append(_sliced(_scattered(db, cases[s][3], msgs, kpg)))
    b = _stream_bufs(sets)
    kl = cases[0][1].shape[1]
    w = torch.empty(dpf.pir_grouped_workspace_size(ng, kpg, logN, rec), dtype=torch.uint8, device="cuda")
    prev = dpf.set_aes_impl(aes)
    try:
        _protocol("dpf_pir_write_grouped_dev", b, sets, want,
                  lambda st: dpf.pir_write_grouped_dev(b["keys"], kl, ng, kpg, logN, b["msgs"], b["db"], nrec, rec, w, stream=st),
                  work=w)
    finally:
        dpf.set_aes_impl(prev)


def test_two_shard_grouped_handle_write():
    """gpu_init_devices([0, 0]) and PirDB(..., ngpus=2, groups=7) at rec 7 and
    32: shards of four groups and of three (logical devices: one GPU opened
    twice), then groups=3, shards of two and of one; each shard receives its
    own groups' key and message rows."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "two-shards"], capture_output=True, text=True,
                       timeout=240, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith("done")


if __name__ == "__main__":
    dpf.gpu_init_devices([0, 0])
    _handle_checks(7, 7, ngpus=2)           # shards of 4 groups and of 3
    _handle_checks(32, 7, ngpus=2)
    _handle_checks(32, 3, ngpus=2)          # of 2 and of 1
    dpf.gpu_shutdown()
    print("done")
