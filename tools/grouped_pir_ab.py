#!/usr/bin/env python3
"""Grouped PIR (dpf_pir_answer_grouped_dev) against the two ways the library
offered before it for the same queries.

A table of 2^--log-n records of --rec-bytes is kept as b = 1.5 m buckets of its
3-fold replicated copy (a batch code), 3 n / b records a bucket, so that a
client wanting m records sends one short key per bucket.  Timed per m:
  (a) dpf_pir_answer_grouped_dev over the b buckets, one key each;
  (b) the same work without the grouped fold: one tree pass of the b keys at
      the bucket's logN (dpf_evalfull_batch_dev), then one
      dpf_xor_fold_sliced_any_dev per bucket on that bucket's part of the
      grouped layout.  Its per-bucket calls are issued from Python; what is
      measured is the time the device needs to get through them, which is
      bounded below by the host's issue rate: that cost is the reason the
      grouped fold exists, and it is part of (b);
  (c) the unbucketed dpf_pir_answer_sliced_any_dev: m keys over the whole table.
Then (a) against (b) at 96 groups for keys_per_group 1, 2, 4, 8 (the fold of
(b) is the matrix-core fold from 2 keys), with the two folds alone beside the
composites (a_fold, b_fold: the tree pass is common to both).

One MI355X, one process, the variants alternate inside every pair.  A figure
is the mean of --launches calls between two device events (warm-up calls
first), in microseconds; the summary gives the median over the pairs, the
min-max spread and in how many pairs (a) beat (b).  The answers of (a) and (b)
are compared byte for byte before anything is timed.  The DB bytes are random:
the kernels' time does not depend on them.

    python tools/grouped_pir_ab.py --out profiles/grouped_pir/ab.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dpf-go_amd"))

import dpf                  # noqa: E402
from dpf import synth       # noqa: E402


def timed(fn, launches, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / launches


def random_bytes(n):
    """n random bytes on the device, made in pieces (a 64-bit randint of the whole size would triple the memory)."""
    import torch
    t = torch.empty(n, dtype=torch.uint8, device="cuda")
    step = 1 << 28
    for o in range(0, n, step):
        t[o:o + step].random_(0, 256)
    return t


def keys_for(nk, logN, hi):
    al, s0, s1 = synth.key_seeds(nk, logN, first=nk + logN)
    al = al % np.uint64(hi)
    ka, _ = dpf.gen_batch_seeded(al, logN, s0, s1)
    return ka


def grouped(ng, kpg, cap, rec, dbs, args, out, tag, extra=None):
    """(a) and (b) over ng groups of cap records; returns the summary."""
    import torch
    logN = max(7, (cap - 1).bit_length())
    nk = ng * kpg
    ka = keys_for(nk, logN, cap)
    kl = ka.shape[1]
    d_keys = torch.from_numpy(ka.reshape(-1)).cuda()
    gs = dpf.pir_group_stride(cap)
    stride = dpf.evalfull_len(logN)
    w_a = torch.empty(dpf.pir_grouped_workspace_size(ng, kpg, logN, rec), dtype=torch.uint8, device="cuda")
    w_tree = torch.empty(dpf.workspace_size(nk, logN), dtype=torch.uint8, device="cuda")
    bits = torch.empty(nk * stride, dtype=torch.uint8, device="cuda")
    w_fold = torch.empty(dpf.xor_fold_workspace_size(), dtype=torch.uint8, device="cuda")
    w_gfold = torch.empty(dpf.xor_fold_grouped_workspace_size(ng, kpg, rec), dtype=torch.uint8, device="cuda")
    ans_a = torch.empty(nk * rec, dtype=torch.uint8, device="cuda")
    ans_b = torch.empty(nk * rec, dtype=torch.uint8, device="cuda")
    ans_f = torch.empty(nk * rec, dtype=torch.uint8, device="cuda")
    db_of = [dbs[g * gs * rec:(g + 1) * gs * rec] for g in range(ng)]
    bits_of = [bits[g * kpg * stride:(g + 1) * kpg * stride] for g in range(ng)]
    ans_of = [ans_b[g * kpg * rec:(g + 1) * kpg * rec] for g in range(ng)]

    def a():
        dpf.pir_answer_grouped_dev(d_keys, kl, ng, kpg, logN, dbs, cap, rec, ans_a, w_a)

    def tree():
        dpf.evalfull_batch_dev(d_keys, kl, nk, logN, bits, w_tree)

    def b_fold():
        for g in range(ng):
            dpf.xor_fold_sliced_any_dev(bits_of[g], stride, kpg, db_of[g], cap, rec, ans_of[g], w_fold)

    def b():
        tree()
        b_fold()

    def a_fold():
        dpf.xor_fold_grouped_dev(bits, stride, ng, kpg, dbs, cap, rec, ans_f, w_gfold)

    a()
    b()
    a_fold()
    torch.cuda.synchronize()
    assert torch.equal(ans_a, ans_b), "the grouped answers differ from the per-bucket folds"
    assert torch.equal(ans_f, ans_b), "the grouped fold differs from the per-bucket folds"
    names = ["a", "b", "a_fold", "b_fold", "tree"]
    fns = [a, b, a_fold, b_fold, tree]
    if extra:
        names.append("c")
        fns.append(extra)
    rows = []
    for p in range(args.pairs):
        r = dict(tag, ngroups=ng, kpg=kpg, cap=cap, logN=logN, rec_bytes=rec, pair=p)
        for name, fn in zip(names, fns):
            r[name] = round(timed(fn, args.launches, args.warmup), 2)
        rows.append(r)
        out.write(json.dumps(r) + "\n")
        out.flush()
    s = dict(tag, ngroups=ng, kpg=kpg, cap=cap, logN=logN, rec_bytes=rec, pairs=args.pairs, launches=args.launches,
             a_beats_b=sum(r["a"] < r["b"] for r in rows))
    if extra:
        s["a_beats_c"] = sum(r["a"] < r["c"] for r in rows)
    for name in names:
        v = [r[name] for r in rows]
        s[name] = {"median": round(statistics.median(v), 2), "min": min(v), "max": max(v)}
    out.write(json.dumps({"summary": s}) + "\n")
    out.flush()
    print(json.dumps({"summary": s}))
    for t in (w_a, w_tree):
        dpf.forget_workspace(t)
    return s


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_pir", "ab.jsonl"))
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log-n", type=int, default=24)
    ap.add_argument("--rec-bytes", type=int, default=32)
    ap.add_argument("--queries", default="64,256")
    ap.add_argument("--kpg", default="1,2,4,8")
    args = ap.parse_args()
    assert dpf.gpu_init(1) >= 1, "no gfx950 device"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    n, rec, logN = 1 << args.log_n, args.rec_bytes, args.log_n
    dbs3 = random_bytes(3 * n * rec)          # the replicated table: every bucket count below divides 3 n
    flat = dbs3[:n * rec]                     # and, for (c), a table of n records
    with open(args.out, "w") as out:
        for m in (int(x) for x in args.queries.split(",") if x):
            b = 3 * m // 2
            assert (3 * n) % b == 0 and (3 * n // b) % 256 == 0, "buckets of whole super-groups only"
            kc = keys_for(m, logN, n)
            d_kc = torch.from_numpy(kc.reshape(-1)).cuda()
            w_c = torch.empty(dpf.pir_workspace_size(m, logN), dtype=torch.uint8, device="cuda")
            ans_c = torch.empty(m * rec, dtype=torch.uint8, device="cuda")

            def c():
                dpf.pir_answer_sliced_any_dev(d_kc, kc.shape[1], m, logN, flat, n, rec, ans_c, w_c)

            grouped(b, 1, 3 * n // b, rec, dbs3, args, out, {"what": "queries", "m": m}, extra=c)
            dpf.forget_workspace(w_c)
            del w_c
        for kpg in (int(x) for x in args.kpg.split(",") if x):
            grouped(96, kpg, 3 * n // 96, rec, dbs3, args, out, {"what": "kpg"})


if __name__ == "__main__":
    main()
