#!/usr/bin/env python3
"""Eval at shared points into selection bits (dpf_eval_bits_dev) against what
the library offered before it for the same rows: dpf_eval_batch_dev over
per-key tiled points, then a torch pack of its bytes to bits.

One MI355X, one process, interleaved pairs.  Per shape and pair, in this
order: (a) eval_bits_dev; (b) eval_batch_dev over the tiled points + the pack,
with the tiling timed on its own; then the sparse answer end to end, (a) + the
sliced fold against (b) + the same fold.  A figure is the mean of --launches
launches between two device events (warm-up launches first), in microseconds;
the summary line gives the median over the pairs and the min-max spread.  The
two routes' rows and answers are compared byte for byte before anything is
timed.

    python tools/sparse_pir_ab.py --out profiles/sparse_pir/ab.jsonl
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


def shape(nk, log_pts, logN, rec, pairs, launches, warmup, out):
    import torch
    npts = 1 << log_pts
    al, s0, s1 = synth.key_seeds(nk, logN, first=log_pts)
    ka, _ = dpf.gen_batch_seeded(al, logN, s0, s1)
    kl = ka.shape[1]
    rng = np.random.default_rng(log_pts)
    xs = rng.integers(0, 1 << logN, npts, dtype=np.uint64)
    xs[:nk] = al                                           # every key's keyword is in the list
    d_keys = torch.from_numpy(ka.reshape(-1)).cuda()
    d_xs = torch.from_numpy(xs.view(np.int64)).cuda()
    stride = dpf.eval_bits_stride(npts)
    assert stride == npts // 8
    w_bits = torch.empty(dpf.eval_bits_workspace_size(nk, npts, logN), dtype=torch.uint8, device="cuda")
    w_eval = torch.empty(dpf.eval_workspace_size(nk, npts, logN), dtype=torch.uint8, device="cuda")
    w_fold = torch.empty(dpf.xor_fold_workspace_size(), dtype=torch.uint8, device="cuda")
    rows_a = torch.empty(nk * stride, dtype=torch.uint8, device="cuda")
    tiled = torch.empty((nk, npts), dtype=torch.int64, device="cuda")
    bytes_b = torch.empty(nk * npts, dtype=torch.uint8, device="cuda")
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device="cuda")
    dbs = torch.randint(0, 256, (dpf.pir_db_sliced_size_any(npts, rec),), dtype=torch.uint8, device="cuda")
    ans_a = torch.empty(nk * rec, dtype=torch.uint8, device="cuda")
    ans_b = torch.empty(nk * rec, dtype=torch.uint8, device="cuda")
    rows_b = [None]

    def a_bits():
        dpf.eval_bits_dev(d_keys, kl, nk, d_xs, npts, logN, rows_a, stride, w_bits)

    def b_tile():
        tiled.copy_(d_xs.expand(nk, npts))

    def b_eval():
        dpf.eval_batch_dev(d_keys, kl, nk, tiled, npts, logN, bytes_b, w_eval)

    def b_pack():
        rows_b[0] = (bytes_b.view(nk, npts // 8, 8) * weights).sum(dim=2, dtype=torch.uint8)

    def b_all():
        b_tile()
        b_eval()
        b_pack()

    def fold(rows, ans):
        dpf.xor_fold_sliced_any_dev(rows, stride, nk, dbs, npts, rec, ans, w_fold)

    def a_answer():
        a_bits()
        fold(rows_a, ans_a)

    def b_answer():
        b_all()
        fold(rows_b[0], ans_b)

    a_answer()
    b_answer()
    torch.cuda.synchronize()
    assert torch.equal(rows_a.view(nk, stride), rows_b[0]), "the two routes' rows differ"
    assert torch.equal(ans_a, ans_b), "the two routes' answers differ"
    form = dpf.eval_form_for(nk, npts, logN, w_eval.numel(), True)
    names = ["a_bits", "b_tile", "b_eval", "b_pack", "b_all", "a_answer", "b_answer"]
    fns = [a_bits, b_tile, b_eval, b_pack, b_all, a_answer, b_answer]
    rows = []
    for p in range(pairs):
        r = {"nkeys": nk, "npts": npts, "logN": logN, "rec_bytes": rec, "pair": p}
        for name, fn in zip(names, fns):
            r[name] = round(timed(fn, launches, warmup), 2)
        rows.append(r)
        out.write(json.dumps(r) + "\n")
        out.flush()
    summary = {"nkeys": nk, "npts": npts, "logN": logN, "rec_bytes": rec, "pairs": pairs, "launches": launches,
               "bits_kernel": "k_eval_bits (one unit per wave; the only form)", "frontier_level": form.level,
               "eval_batch_kernel": form.kernel}
    for name in names:
        v = [r[name] for r in rows]
        summary[name] = {"median": round(statistics.median(v), 2), "min": min(v), "max": max(v)}
    out.write(json.dumps({"summary": summary}) + "\n")
    out.flush()
    print(json.dumps({"summary": summary}))
    for t in (w_bits, w_eval):
        dpf.forget_workspace(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_pir", "ab.jsonl"))
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--logN", type=int, default=40)
    ap.add_argument("--rec-bytes", type=int, default=32)
    ap.add_argument("--shapes", default="64x20,16x22", help="nkeys x log2(points), comma separated")
    args = ap.parse_args()
    assert dpf.gpu_init(1) >= 1, "no gfx950 device"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        for s in args.shapes.split(","):
            nk, lp = (int(x) for x in s.split("x"))
            shape(nk, lp, args.logN, args.rec_bytes, args.pairs, args.launches, args.warmup, out)


if __name__ == "__main__":
    main()
