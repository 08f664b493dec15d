"""dpf/buckets.py: merge_clients / split_answers, the batching of several
clients' per-bucket keys into keys_per_group = nclients keys per bucket and
the way back on the answers.  numpy only."""
import numpy as np
import pytest

from dpf import buckets


def test_merge_is_group_order_and_split_is_its_inverse():
    nb, kl, rec, ncl = 12, 51, 20, 9
    rng = np.random.default_rng(1)
    keys = [rng.integers(0, 256, (nb, kl), dtype=np.uint8) for _ in range(ncl)]
    merged = buckets.merge_clients(keys)
    assert merged.shape == (nb * ncl, kl) and merged.dtype == np.uint8 and merged.flags.c_contiguous
    for b in range(nb):
        for c in range(ncl):
            assert np.array_equal(merged[b * ncl + c], keys[c][b])      # row g * kpg + j: bucket g, client j
    # "Answers" that name their row: the split hands every client its own buckets in order.
    ans = rng.integers(0, 256, (nb * ncl, rec), dtype=np.uint8)
    out = buckets.split_answers(ans, ncl)
    assert out.shape == (ncl, nb, rec) and out.flags.c_contiguous
    for c in range(ncl):
        for b in range(nb):
            assert np.array_equal(out[c, b], ans[b * ncl + c])
    # The round trip on the keys themselves.
    back = buckets.split_answers(merged, ncl)
    for c in range(ncl):
        assert np.array_equal(back[c], keys[c])
    assert np.array_equal(buckets.merge_clients(list(back)), merged)


def test_one_client_is_the_identity():
    k = np.arange(5 * 7, dtype=np.uint8).reshape(5, 7)
    assert np.array_equal(buckets.merge_clients([k]), k)
    assert np.array_equal(buckets.split_answers(k, 1)[0], k)


def test_bad_shapes_are_refused():
    k = np.zeros((4, 8), np.uint8)
    with pytest.raises(ValueError):
        buckets.merge_clients([])
    with pytest.raises(ValueError):
        buckets.merge_clients([k, np.zeros((5, 8), np.uint8)])
    with pytest.raises(ValueError):
        buckets.merge_clients([k, np.zeros(8, np.uint8)])
    with pytest.raises(ValueError):
        buckets.split_answers(np.zeros((10, 4), np.uint8), 3)
    with pytest.raises(ValueError):
        buckets.split_answers(np.zeros((10, 4), np.uint8), 0)
