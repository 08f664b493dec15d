#!/usr/bin/env python3
"""Grouped keyword PIR in one Eval-bits launch (dpf_pir_answer_grouped_sparse_dev,
dpf_pir_write_grouped_sparse_dev) against what a server ran before it for the
same buckets: one dpf_pir_answer_sparse_dev / dpf_pir_write_sparse_dev per group
on the same stream, over the same grouped DB (a group whose nrec is a multiple
of 256 is a sliced DB of its own inside the grouped layout) and the same
points.

One MI355X, one process, interleaved pairs.  Per shape and pair, in this
order: (a) the grouped-sparse answer; (b) the per-group loop of sparse answers;
(a) the grouped-sparse write; (b) the per-group loop of sparse writes.  A
figure is the mean of --launches calls between two device events (warm-up calls
first), in microseconds, so the loop's figure includes the host's cost of
issuing its calls through ctypes wherever that exceeds the device's; the
summary line gives the median over the pairs and the min-max spread.  The two
routes' answers and written DBs are compared byte for byte before anything is
timed.

    python tools/grouped_sparse_ab.py --out profiles/grouped_sparse/ab.jsonl
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


def shape(ng, log_rec, kpg, logN, rec, pairs, launches, warmup, out):
    import torch
    nrec = 1 << log_rec
    assert nrec % 256 == 0, "the per-group baseline reads a group as a sliced DB of its own"
    nk = ng * kpg
    rng = np.random.default_rng(ng * 64 + log_rec)
    pts = rng.integers(0, 1 << logN, (ng, nrec), dtype=np.uint64)
    al = pts[np.arange(ng).repeat(kpg), rng.integers(0, nrec, nk)]       # every key's keyword is in its group's list
    _, s0, s1 = synth.key_seeds(nk, logN, first=log_rec)
    ka, _ = dpf.gen_batch_seeded(al, logN, s0, s1)
    kl = ka.shape[1]
    d_keys = torch.from_numpy(ka.reshape(-1)).cuda()
    d_pts = torch.from_numpy(pts.view(np.int64).reshape(-1)).cuda()
    d_msgs = torch.randint(0, 256, (nk * rec,), dtype=torch.uint8, device="cuda")
    size = dpf.pir_db_grouped_size(ng, nrec, rec)
    gbytes = nrec * rec                                                  # a group of the grouped layout
    dbs_a = torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda")
    dbs_b = dbs_a.clone()
    w_a = torch.empty(dpf.pir_grouped_sparse_workspace_size(ng, kpg, nrec, logN, rec), dtype=torch.uint8, device="cuda")
    w_b = torch.empty(dpf.pir_sparse_workspace_size(kpg, nrec, logN), dtype=torch.uint8, device="cuda")
    ans_a = torch.empty(nk * rec, dtype=torch.uint8, device="cuda")
    ans_b = torch.empty(nk * rec, dtype=torch.uint8, device="cuda")
    # The loop's per-group views, made once: slicing tensors is not what is timed.
    keys_g = [d_keys[g * kpg * kl:(g + 1) * kpg * kl] for g in range(ng)]
    pts_g = [d_pts[g * nrec:(g + 1) * nrec] for g in range(ng)]
    msgs_g = [d_msgs[g * kpg * rec:(g + 1) * kpg * rec] for g in range(ng)]
    ans_g = [ans_b[g * kpg * rec:(g + 1) * kpg * rec] for g in range(ng)]
    db_g = [dbs_b[g * gbytes:(g + 1) * gbytes] for g in range(ng)]

    def a_answer():
        dpf.pir_answer_grouped_sparse_dev(d_keys, kl, ng, kpg, logN, d_pts, dbs_a, nrec, rec, ans_a, w_a)

    def b_answer():
        for g in range(ng):
            dpf.pir_answer_sparse_dev(keys_g[g], kl, kpg, logN, pts_g[g], db_g[g], nrec, rec, ans_g[g], w_b)

    def a_write():
        dpf.pir_write_grouped_sparse_dev(d_keys, kl, ng, kpg, logN, d_pts, d_msgs, dbs_a, nrec, rec, w_a)

    def b_write():
        for g in range(ng):
            dpf.pir_write_sparse_dev(keys_g[g], kl, kpg, logN, pts_g[g], msgs_g[g], db_g[g], nrec, rec, w_b)

    a_answer()
    b_answer()
    torch.cuda.synchronize()
    assert torch.equal(ans_a, ans_b), "the two routes' answers differ"
    a_write()
    b_write()
    torch.cuda.synchronize()
    assert torch.equal(dbs_a, dbs_b), "the two routes' written DBs differ"
    names = ["a_answer", "b_answer", "a_write", "b_write"]
    fns = [a_answer, b_answer, a_write, b_write]
    rows = []
    for p in range(pairs):
        r = {"ngroups": ng, "nrec": nrec, "kpg": kpg, "logN": logN, "rec_bytes": rec, "pair": p}
        for name, fn in zip(names, fns):
            r[name] = round(timed(fn, launches, warmup), 2)
        rows.append(r)
        out.write(json.dumps(r) + "\n")
        out.flush()
    summary = {"ngroups": ng, "nrec": nrec, "kpg": kpg, "logN": logN, "rec_bytes": rec, "pairs": pairs,
               "launches": launches, "frontier_level": dpf.eval_frontier_level(logN, nrec),
               "a": "one grouped-sparse call", "b": "one sparse call per group, same stream"}
    for name in names:
        v = [r[name] for r in rows]
        summary[name] = {"median": round(statistics.median(v), 2), "min": min(v), "max": max(v)}
    for what in ("answer", "write"):
        summary[what + "_b_over_a"] = round(summary["b_" + what]["median"] / summary["a_" + what]["median"], 2)
    out.write(json.dumps({"summary": summary}) + "\n")
    out.flush()
    print(json.dumps({"summary": summary}))
    for t in (w_a, w_b):
        dpf.forget_workspace(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_sparse", "ab.jsonl"))
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--logN", type=int, default=40)
    ap.add_argument("--rec-bytes", type=int, default=32)
    ap.add_argument("--kpg", type=int, default=1)
    ap.add_argument("--shapes", default="96x14,384x12,8x18", help="groups x log2(records per group), comma separated")
    args = ap.parse_args()
    assert dpf.gpu_init(1) >= 1, "no gfx950 device"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        for s in args.shapes.split(","):
            ng, lr = (int(x) for x in s.split("x"))
            shape(ng, lr, args.kpg, args.logN, args.rec_bytes, args.pairs, args.launches, args.warmup, out)


if __name__ == "__main__":
    main()
