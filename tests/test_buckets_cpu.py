"""dpf/buckets.py, the batch-code example over a grouped PirDB: host only.
The seeds below were chosen on the CPU so that the cuckoo assignment of 8
wanted records into 12 buckets succeeds for each; the test asserts that it
does."""
import numpy as np
import pytest

from dpf import buckets

N, NBUCKETS, NWANT = 3000, 12, 8
SEEDS = [0, 1, 3, 4, 5]


def _wanted(seed):
    return np.random.default_rng(seed).choice(N, NWANT, replace=False)


@pytest.mark.parametrize("seed", SEEDS)
def test_assignment_puts_each_wanted_record_into_a_bucket_of_its_own(seed):
    lay = buckets.layout(N, NBUCKETS, seed=seed)
    assert lay.bucket.shape == lay.pos.shape == (N, 3)
    assert ((lay.bucket >= 0) & (lay.bucket < NBUCKETS)).all()
    wanted = _wanted(seed)
    got = buckets.assign(wanted, lay)
    assert sorted(got.values()) == sorted(int(w) for w in wanted)     # every one placed, in distinct buckets (dict keys)
    for b, rec in got.items():
        assert b in lay.bucket[rec]                                   # one of its own candidates
    al = buckets.alphas(got, lay)
    assert al.shape == (NBUCKETS,) and al.dtype == np.uint64
    for b in range(NBUCKETS):
        if b not in got:
            assert al[b] == 0
        else:
            j = list(lay.bucket[got[b]]).index(b)
            assert al[b] == lay.pos[got[b], j]


@pytest.mark.parametrize("seed", SEEDS)
def test_build_puts_every_record_where_the_layout_says(seed):
    lay = buckets.layout(N, NBUCKETS, seed=seed)
    db = np.random.default_rng(seed + 100).integers(0, 256, (N, 20), dtype=np.uint8)
    bdb, logN = buckets.build(db, lay)
    assert bdb.shape == (NBUCKETS, lay.cap, 20)
    assert lay.cap <= (1 << logN) and (logN == 7 or lay.cap > (1 << (logN - 1)))
    for j in range(3):
        assert np.array_equal(bdb[lay.bucket[:, j], lay.pos[:, j]], db)
    # Positions inside a bucket are 0 .. fill - 1, each used once; the rest is zero padding.
    fill = np.bincount(lay.bucket.reshape(-1), minlength=NBUCKETS)
    assert fill.max() == lay.cap and fill.sum() == 3 * N
    for b in range(NBUCKETS):
        assert sorted(lay.pos[lay.bucket == b]) == list(range(fill[b]))
        assert not bdb[b, fill[b]:].any()


def test_layout_is_a_function_of_its_arguments():
    a, b = buckets.layout(500, 7, seed=9), buckets.layout(500, 7, seed=9)
    assert np.array_equal(a.bucket, b.bucket) and np.array_equal(a.pos, b.pos) and a.cap == b.cap
    assert not np.array_equal(a.bucket, buckets.layout(500, 7, seed=10).bucket)


def test_more_wanted_records_than_buckets_overflows():
    lay = buckets.layout(N, 4, seed=0)
    with pytest.raises(buckets.BucketOverflow):
        buckets.assign(np.arange(5), lay)
