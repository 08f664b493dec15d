"""dpf/buckets.py, the keyword variant of the batch-code example, end to end
against a numpy server: host only.  The selections of both servers come from
oracle.eval_batch at each bucket's own points, as the grouped keyword PirDB
computes them on the device.  The seed below was chosen on the CPU so that the
cuckoo assignment of the 9 asked keywords into 12 buckets succeeds and no
bucket holds more than KPG replicas of the written keywords; the tests assert
both."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "dpf-go_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import dpf                  # noqa: E402
from dpf import buckets, synth   # noqa: E402
import oracle               # noqa: E402

N, NBUCKETS, NWANT, REC, LOGN, SEED, KPG = 600, 12, 8, 20, 40, 0, 3


def _table():
    rng = np.random.default_rng(11)
    keywords = rng.choice(1 << 48, N, replace=False).astype(np.uint64)
    db = rng.integers(0, 256, (N, REC), dtype=np.uint8)
    db[db.sum(axis=1) == 0, 0] = 1                     # no all-zero record: a hit is told from a miss
    lay = buckets.keyword_layout(keywords, NBUCKETS, seed=SEED)
    bdb, bpts, logN = buckets.keyword_build(db, keywords, lay, LOGN, seed=SEED)
    return keywords, db, lay, bdb, bpts, logN


def _replicas(lay, r):
    """The distinct (bucket, position) slots that hold record r."""
    return sorted(set((int(b), int(p)) for b, p in zip(lay.bucket[r], lay.pos[r])))


def _server(keys, bdb, bpts, logN):
    """[nbuckets][kpg] selections (bool [cap]) of one server's key rows [nbuckets * kpg]."""
    kpg = keys.shape[0] // bpts.shape[0]
    return oracle.eval_batch(keys, np.repeat(bpts, kpg, axis=0), logN, nthreads=4).astype(bool)


def _keys(alphas, logN, first):
    _, s0, s1 = synth.key_seeds(alphas.size, logN, first=first)
    return dpf.gen_batch_seeded(alphas.reshape(-1), logN, s0, s1)


def test_build_places_every_replica_at_its_keywords_point():
    keywords, db, lay, bdb, bpts, logN = _table()
    pts = buckets.keyword_points(keywords, logN, seed=SEED)
    assert logN == LOGN and pts.dtype == np.uint64 and (pts < (1 << LOGN)).all() and np.unique(pts).size == N
    assert bdb.shape == (NBUCKETS, lay.cap, REC) and bpts.shape == (NBUCKETS, lay.cap) and bpts.dtype == np.uint64
    slots = [s for r in range(N) for s in _replicas(lay, r)]
    assert len(set(slots)) == len(slots) < 3 * N       # no slot used twice; some record's hashes collide on a bucket
    fill = np.bincount([b for b, _ in slots], minlength=NBUCKETS)
    assert fill.max() == lay.cap and fill.min() < lay.cap     # some bucket is padded
    for j in range(lay.bucket.shape[1]):
        assert np.array_equal(bdb[lay.bucket[:, j], lay.pos[:, j]], db)
        assert np.array_equal(bpts[lay.bucket[:, j], lay.pos[:, j]], pts)
    for b in range(NBUCKETS):
        assert np.unique(bpts[b, :fill[b]]).size == fill[b]     # a record is in a bucket once: no point repeats
        pad = bpts[b, fill[b]:]
        assert not bdb[b, fill[b]:].any()              # zero records ...
        assert (pad == pad[:1]).all()                  # ... at one repeated point ...
        assert not np.isin(pad[:1], bpts[b, :fill[b]]).any() and (pad < (1 << LOGN)).all()   # ... that no record has


def test_keyword_queries_come_back_from_two_numpy_servers():
    keywords, db, lay, bdb, bpts, logN = _table()
    rng = np.random.default_rng(12)
    want_idx = rng.choice(N, NWANT, replace=False)
    absent = np.uint64(12345)
    assert absent not in keywords
    asked = np.concatenate([keywords[want_idx], [absent]])
    # The client knows its keywords only: their candidate buckets and points are public hashes.
    mine = buckets.keyword_layout(asked, NBUCKETS, seed=SEED)
    assert np.array_equal(mine.bucket[:NWANT], lay.bucket[want_idx])
    assignment = buckets.assign(range(asked.size), mine)
    assert sorted(assignment.values()) == list(range(asked.size))
    al = buckets.keyword_alphas(assignment, buckets.keyword_points(asked, logN, seed=SEED), bpts, logN)
    assert al.shape == (NBUCKETS,) and al.dtype == np.uint64
    for b in range(NBUCKETS):
        if b not in assignment:
            assert al[b] not in bpts[b]                # a point absent from that bucket
    ka, kb = _keys(al, logN, first=500)
    ans = np.zeros((NBUCKETS, REC), np.uint8)
    for keys in (ka, kb):
        sel = _server(keys, bdb, bpts, logN)
        for b in range(NBUCKETS):
            if sel[b].any():
                ans[b] ^= np.bitwise_xor.reduce(bdb[b][sel[b]], axis=0)
    for b in range(NBUCKETS):
        if b not in assignment or assignment[b] == NWANT:
            assert not ans[b].any()                    # an unused bucket, and the absent keyword
        else:
            assert np.array_equal(ans[b], db[want_idx[assignment[b]]])


def test_write_plan_round_changes_exactly_the_replicas():
    keywords, db, lay, bdb, bpts, logN = _table()
    pts = buckets.keyword_points(keywords, logN, seed=SEED)
    rng = np.random.default_rng(13)
    written = rng.choice(N, 4, replace=False)
    deltas = {int(r): rng.integers(1, 256, REC, dtype=np.uint8) for r in written}
    al, msgs = buckets.keyword_write_plan(deltas, lay, pts, bpts, logN, KPG)
    assert al.shape == (NBUCKETS, KPG) and msgs.shape == (NBUCKETS, KPG, REC)
    used = msgs.any(axis=2)
    nrep = sum(len(_replicas(lay, r)) for r in deltas)
    assert used.sum() == nrep
    for b in range(NBUCKETS):
        for s in range(KPG):
            if not used[b, s]:
                assert al[b, s] not in bpts[b]         # a dummy: an absent point, an all-zero message
    ka, kb = _keys(al, logN, first=900)
    shares = []
    for keys in (ka, kb):
        sel = _server(keys, bdb, bpts, logN)
        mine = bdb.copy()
        for k in range(NBUCKETS * KPG):
            mine[k // KPG][sel[k]] ^= msgs.reshape(-1, REC)[k]
        shares.append(mine)
    changed = shares[0] ^ shares[1]                    # both servers started from the same table
    want = np.zeros_like(bdb)
    for r, d in deltas.items():
        for b, p in _replicas(lay, r):
            want[b, p] ^= d
    assert np.array_equal(changed, want)
    assert (want.reshape(-1, REC).any(axis=1)).sum() == nrep
    # An empty plan is cover traffic: all dummies.
    al0, msgs0 = buckets.keyword_write_plan({}, lay, pts, bpts, logN, KPG, rec_bytes=REC)
    assert not msgs0.any() and all(al0[b, s] not in bpts[b] for b in range(NBUCKETS) for s in range(KPG))
