"""Batch-code bucketing for multi-query PIR over a grouped PirDB: an example.

A client that wants m records of an n-record table does not send m keys over
the whole domain.  The server keeps the table as nbuckets ~ 1.5 m buckets, each
record copied into its nhash = 3 candidate buckets (public hashes of its
index); the client places each wanted record into a bucket of its own by
cuckoo moves and sends ONE short key per bucket, over the bucket's small
domain: a dummy point in the buckets it does not use, so the servers learn
nothing from which buckets are queried.  On the server the buckets are the
groups of `dpf.PirDB(bucket_db, logN, rec_bytes=rec, groups=nbuckets)`.

A private write is the other way round: the table is kept consistent only if
every replica of a changed record changes, so a client that XORs deltas into m
records sends kpg short keys per bucket (write_plan: one per replica that falls
into the bucket, dummies with an all-zero message in the unused slots) to
`PirDB.write_grouped`, instead of m keys over the whole domain per replica.

Keyword PIR over buckets (the keyword_* functions below): the records are keyed
by keywords, not by an index.  A public hash sends a keyword to a point of a
2^logN domain (logN 40 .. 63: large enough that two keywords do not collide)
and further hashes send it to its nhash candidate buckets.  A bucket then holds
its records at their keywords' points, the groups of
`dpf.PirDB(bucket_db, logN, rec_bytes=rec, points=bucket_points, groups=nbuckets)`,
and a client key for a bucket is Gen(point_of(keyword), logN): the servers
evaluate every bucket's keys at that bucket's own points in one launch.  A
keyword the table does not hold reads as the zero record.

This is documentation that runs, not a protocol implementation: host-only,
numpy-only, with a fixed integer mix in the place of a keyed hash, no
treatment of failure probability and no padding of the number of queries.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

_M = (1 << 64) - 1


class BucketOverflow(Exception):
    """assign() found no placement within its bound on cuckoo kicks, or
    write_plan() a bucket that needs more keys than it was given."""


class Layout(NamedTuple):
    nbuckets: int
    bucket: np.ndarray   # [n][nhash] int64: record i's candidate buckets (may repeat)
    pos: np.ndarray      # [n][nhash] int64: its position inside each
    cap: int             # records in the fullest bucket


def _mix(seed: int, j: int, i: np.ndarray) -> np.ndarray:
    """A fixed 64-bit integer mix of (seed, j, i): splitmix64's finalizer."""
    with np.errstate(over="ignore"):
        x = i.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64((seed * 0xBF58476D1CE4E5B9 + j + 1) & _M)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def layout(n: int, nbuckets: int, nhash: int = 3, seed: int = 0) -> Layout:
    """Each record's candidate buckets, and its position inside each: the
    records of a bucket in index order (a record whose hashes collide on one
    bucket is stored there once per hash)."""
    return _layout_of(np.arange(n, dtype=np.uint64), nbuckets, nhash, seed)


def _layout_of(idx: np.ndarray, nbuckets: int, nhash: int, seed: int, once: bool = False) -> Layout:
    """layout() of records named by the uint64 values idx (their indices, or
    their keywords).  once: a record whose hashes collide on one bucket is
    stored there once, every colliding hash naming the same position."""
    n = idx.size
    bucket = np.stack([(_mix(seed, j, idx) % np.uint64(nbuckets)).astype(np.int64) for j in range(nhash)], axis=1)
    pos = np.zeros((n, nhash), np.int64)
    fill = np.zeros(nbuckets, np.int64)
    for i in range(n):
        for j in range(nhash):
            same = [k for k in range(j) if bucket[i, k] == bucket[i, j]] if once else []
            if same:
                pos[i, j] = pos[i, same[0]]
                continue
            pos[i, j] = fill[bucket[i, j]]
            fill[bucket[i, j]] += 1
    return Layout(nbuckets, bucket, pos, int(fill.max()) if n else 0)


def build(db: np.ndarray, lay: Layout):
    """(bucket_db [nbuckets][cap][rec] zero-padded, logN): the server's grouped
    DB and the domain that covers a bucket (at least 7, the smallest a key has)."""
    db = np.ascontiguousarray(db, dtype=np.uint8)
    out = np.zeros((lay.nbuckets, max(lay.cap, 1), db.shape[1]), np.uint8)
    for j in range(lay.bucket.shape[1]):
        out[lay.bucket[:, j], lay.pos[:, j]] = db
    return out, max(7, (max(lay.cap, 1) - 1).bit_length())


def assign(wanted, lay: Layout, max_kicks: int = 200) -> dict:
    """{bucket: record}: every wanted record in one of its own candidate
    buckets, no two in the same one, by cuckoo moves: a record whose
    candidates are all taken evicts an occupant, which is placed again.
    Raises BucketOverflow after max_kicks evictions."""
    owner: dict = {}
    kicks = 0
    for first in dict.fromkeys(int(w) for w in wanted):
        rec, last = first, -1
        while True:
            cand = [int(b) for b in lay.bucket[rec]]
            free = [b for b in cand if b not in owner]
            if free:
                owner[free[0]] = rec
                break
            kicks += 1
            if kicks > max_kicks:
                raise BucketOverflow("no placement of %d records into %d buckets within %d kicks"
                                     % (len(set(int(w) for w in wanted)), lay.nbuckets, max_kicks))
            away = [b for b in cand if b != last] or cand      # not straight back where it came from
            last = away[kicks % len(away)]                      # a deterministic walk over the candidates
            owner[last], rec = rec, owner[last]
    return owner


def alphas(assignment: dict, lay: Layout) -> np.ndarray:
    """[nbuckets] uint64: the point to query in every bucket (0 in unused ones)."""
    a = np.zeros(lay.nbuckets, np.uint64)
    for b, rec in assignment.items():
        j = [int(x) for x in lay.bucket[rec]].index(b)
        a[b] = lay.pos[rec, j]
    return a


def merge_clients(keys_per_client) -> np.ndarray:
    """[nbuckets * nclients][key_len] in group order from a list of per-client
    [nbuckets][key_len] key arrays: a server that batches the queries of several
    clients answers them as keys_per_group = nclients keys per bucket, row
    b * nclients + c being client c's key for bucket b.  Many keys per group are
    one matrix-core pass over the buckets per 256 clients."""
    ks = [np.ascontiguousarray(k, dtype=np.uint8) for k in keys_per_client]
    if not ks or any(k.ndim != 2 or k.shape != ks[0].shape for k in ks):
        raise ValueError("every client sends one [nbuckets][key_len] array of the same shape")
    return np.ascontiguousarray(np.stack(ks, axis=1)).reshape(ks[0].shape[0] * len(ks), ks[0].shape[1])


def split_answers(ans, nclients: int) -> np.ndarray:
    """[nclients][nbuckets][rec]: merge_clients' inverse on the answers
    [nbuckets * nclients][rec] of the merged keys; entry c is client c's."""
    ans = np.ascontiguousarray(ans)
    if nclients <= 0 or ans.ndim != 2 or ans.shape[0] % nclients:
        raise ValueError("answers are [nbuckets * nclients][rec]")
    return np.ascontiguousarray(ans.reshape(ans.shape[0] // nclients, nclients, ans.shape[1]).transpose(1, 0, 2))


def write_plan(deltas: dict, lay: Layout, kpg: int, rec_bytes: int = None, points=None, dummy=None):
    """(alphas [nbuckets][kpg] uint64, msgs [nbuckets][kpg][rec] uint8) for
    `PirDB.write_grouped`: {record: XOR delta (rec bytes)} turned into one key
    slot per replica of every record, at the replica's position in its bucket
    with the delta as its message.  Unused slots are dummies: point 0 with an
    all-zero message, which changes nothing, so the servers learn nothing from
    which buckets are written.  rec_bytes is the record width; it may be left
    out where deltas is not empty (an empty one with rec_bytes is an all-dummy
    batch, cover traffic).  Raises BucketOverflow when a bucket holds more
    replicas of the changed records than kpg.  points ([n] uint64) and dummy
    ([nbuckets] uint64) are keyword_write_plan's: a replica is then addressed
    by its record's point instead of its position, a dummy slot of bucket b by
    dummy[b] instead of 0."""
    items = [(int(r), np.ascontiguousarray(d, dtype=np.uint8).reshape(-1)) for r, d in deltas.items()]
    if rec_bytes is None and not items:
        raise ValueError("rec_bytes is needed where there are no deltas to take the width from")
    rec = int(rec_bytes) if rec_bytes is not None else items[0][1].size
    al = np.zeros((lay.nbuckets, kpg), np.uint64)
    if dummy is not None:
        al[:] = np.asarray(dummy, np.uint64).reshape(-1, 1)
    msgs = np.zeros((lay.nbuckets, kpg, rec), np.uint8)
    used = np.zeros(lay.nbuckets, np.int64)
    for r, d in items:
        if d.size != rec:
            raise ValueError("every delta must be %d bytes wide" % rec)
        for j in range(lay.bucket.shape[1]):
            b = int(lay.bucket[r, j])
            if points is not None and b in lay.bucket[r, :j]:
                continue                                    # keyword_layout stores the record there once
            if used[b] == kpg:
                raise BucketOverflow("bucket %d needs more than %d keys" % (b, kpg))
            al[b, used[b]] = lay.pos[r, j] if points is None else points[r]
            msgs[b, used[b]] = d
            used[b] += 1
    return al, msgs


# ---- keyword PIR over buckets ------------------------------------------------
_POINT_HASH = 63   # _mix's j of the keyword -> point hash (the bucket hashes use 0 .. nhash - 1)


def keyword_points(keywords, logN: int, seed: int = 0) -> np.ndarray:
    """[n] uint64: every keyword's point of the 2^logN domain (a public hash)."""
    kw = np.ascontiguousarray(keywords, dtype=np.uint64).reshape(-1)
    return _mix(seed, _POINT_HASH, kw) & np.uint64((1 << logN) - 1)


def keyword_layout(keywords, nbuckets: int, nhash: int = 3, seed: int = 0) -> Layout:
    """layout() by keyword: record i's candidate buckets are hashes of
    keywords[i], so a client computes the candidates of a keyword it wants
    (keyword_layout of its own short list) without knowing the table.  A
    record whose hashes collide on one bucket is stored there ONCE (both
    hashes name the same position): two replicas at one point of one bucket
    would be selected together and cancel."""
    return _layout_of(np.ascontiguousarray(keywords, dtype=np.uint64).reshape(-1), nbuckets, nhash, seed, once=True)


def _absent_point(points: np.ndarray, logN: int) -> int:
    """The smallest point of the 2^logN domain that is not in `points`."""
    have = set(int(p) for p in points)
    p = 0
    while p in have:
        p += 1
    if p >> logN:
        raise BucketOverflow("a bucket holds every point of the 2^%d domain" % logN)
    return p


def keyword_build(db: np.ndarray, keywords, lay: Layout, logN: int, seed: int = 0):
    """(bucket_db [nbuckets][cap][rec], bucket_points [nbuckets][cap] uint64,
    logN): the server's grouped keyword DB.  Slot lay.pos of a bucket holds a
    replica of a record and its keyword's point.  A bucket shorter than cap is
    padded: every pad slot is a zero record, and all pads of a bucket sit at
    one repeated point that none of the bucket's records has.  Reads never see
    a pad (it is zero, and no keyword of the bucket hashes to its point), but a
    pad record absorbs a write aimed at its point: a key for that point with a
    non-zero message would be XORed into every pad of the bucket, so writers
    send dummies with an all-zero message only (keyword_write_plan does)."""
    db = np.ascontiguousarray(db, dtype=np.uint8)
    pts = keyword_points(keywords, logN, seed)
    cap = max(lay.cap, 1)
    out = np.zeros((lay.nbuckets, cap, db.shape[1]), np.uint8)
    bpts = np.zeros((lay.nbuckets, cap), np.uint64)
    fill = np.zeros(lay.nbuckets, np.int64)
    for j in range(lay.bucket.shape[1]):
        out[lay.bucket[:, j], lay.pos[:, j]] = db
        bpts[lay.bucket[:, j], lay.pos[:, j]] = pts
        np.maximum.at(fill, lay.bucket[:, j], lay.pos[:, j] + 1)
    for b in range(lay.nbuckets):
        if fill[b] < cap:
            bpts[b, fill[b]:] = _absent_point(bpts[b, :fill[b]], logN)
    return out, bpts, logN


def keyword_alphas(assignment: dict, wanted_points, bucket_points: np.ndarray, logN: int) -> np.ndarray:
    """[nbuckets] uint64: the point to query in every bucket.  assignment is
    assign()'s {bucket: i} over the client's own list of wanted keywords
    (keyword_layout of that list), wanted_points their points: bucket b is
    asked for point_of(keyword i).  An unused bucket is asked for a point
    absent from that bucket, which reads as zero.  The example looks one up in
    bucket_points to be exact; a real client draws a random point of the
    domain, which misses the bucket except with probability cap / 2^logN."""
    a = np.array([_absent_point(bucket_points[b], logN) for b in range(bucket_points.shape[0])], np.uint64)
    for b, i in assignment.items():
        a[b] = wanted_points[i]
    return a


def keyword_write_plan(deltas: dict, lay: Layout, points, bucket_points: np.ndarray, logN: int, kpg: int,
                       rec_bytes: int = None):
    """write_plan() for the grouped keyword DB: {record: XOR delta} turned into
    (alphas [nbuckets][kpg] uint64, msgs [nbuckets][kpg][rec]) for
    `PirDB.write_grouped`, one slot per replica, addressed by the record's
    point (points: keyword_points of the table's keywords).  Unused slots are
    dummies at a point absent from their bucket with an all-zero message."""
    dummy = np.array([_absent_point(bucket_points[b], logN) for b in range(bucket_points.shape[0])], np.uint64)
    return write_plan(deltas, lay, kpg, rec_bytes, points=np.asarray(points, np.uint64), dummy=dummy)
