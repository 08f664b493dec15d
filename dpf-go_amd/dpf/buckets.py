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
    idx = np.arange(n, dtype=np.uint64)
    bucket = np.stack([(_mix(seed, j, idx) % np.uint64(nbuckets)).astype(np.int64) for j in range(nhash)], axis=1)
    pos = np.zeros((n, nhash), np.int64)
    fill = np.zeros(nbuckets, np.int64)
    for i in range(n):
        for j in range(nhash):
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


def write_plan(deltas: dict, lay: Layout, kpg: int, rec_bytes: int = None):
    """(alphas [nbuckets][kpg] uint64, msgs [nbuckets][kpg][rec] uint8) for
    `PirDB.write_grouped`: {record: XOR delta (rec bytes)} turned into one key
    slot per replica of every record, at the replica's position in its bucket
    with the delta as its message.  Unused slots are dummies: point 0 with an
    all-zero message, which changes nothing, so the servers learn nothing from
    which buckets are written.  rec_bytes is the record width; it may be left
    out where deltas is not empty (an empty one with rec_bytes is an all-dummy
    batch, cover traffic).  Raises BucketOverflow when a bucket holds more
    replicas of the changed records than kpg."""
    items = [(int(r), np.ascontiguousarray(d, dtype=np.uint8).reshape(-1)) for r, d in deltas.items()]
    if rec_bytes is None and not items:
        raise ValueError("rec_bytes is needed where there are no deltas to take the width from")
    rec = int(rec_bytes) if rec_bytes is not None else items[0][1].size
    al = np.zeros((lay.nbuckets, kpg), np.uint64)
    msgs = np.zeros((lay.nbuckets, kpg, rec), np.uint8)
    used = np.zeros(lay.nbuckets, np.int64)
    for r, d in items:
        if d.size != rec:
            raise ValueError("every delta must be %d bytes wide" % rec)
        for j in range(lay.bucket.shape[1]):
            b = int(lay.bucket[r, j])
            if used[b] == kpg:
                raise BucketOverflow("bucket %d needs more than %d keys" % (b, kpg))
            al[b, used[b]] = lay.pos[r, j]
            msgs[b, used[b]] = d
            used[b] += 1
    return al, msgs
