#!/usr/bin/env python3
"""PIR over a record range (dpf_pir_answer_window_dev) against what a server
ran before it for the same records, and the window plan's two routes against
each other.  32-byte records, one MI355X, one process, interleaved.

Per shape and pair, in this order:
  a       dpf_pir_answer_window_dev, whichever route the plan takes;
  b       the parent's call: dpf_pir_answer_sliced_any_dev over the whole
          subtree that holds the records (tables: logN = ceil(log2 nrec));
  p       the pieces route put together from public entries, whatever the plan
          says: dpf_subkeys_dev, dpf_evalfull_batch_dev over the nkeys * P
          sub-keys, dpf_xor_fold_sliced_any_dev from row_offset;
  a_tree, b_tree, p_tree   the same without the fold.
Shapes: tables of --nrec records from point 0; shard 0 of 8 of the 5 * 2^21
table (a, p: the balanced split's 5 * 2^18 records; b: the subtree split's 2^21
under prefix (3, 0)); shard 3 of 8 of the balanced split, records [15 * 2^18,
20 * 2^18), which straddle point 2^22 (b: the subtree (1, 0) of 2^23 points
that holds them, dpf_evalfull_subtree_dev and the fold from the shard's
offset).  k_subkeys alone is timed at 64 keys with 32 prefixes of 5 levels
(all there are) and with 33 of 6.

A figure is the mean of --launches calls between two device events (warm-up
calls first), in microseconds; the summary line gives the median over the
pairs and the min-max spread.  The routes' answers are compared byte for byte
before anything is timed.

    python tools/pir_window_ab.py --out profiles/pir_window/ab.jsonl
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

REC = 32


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


def run(what, names, fns, meta, args, out):
    rows = []
    for p in range(args.pairs):
        r = dict(meta, what=what, pair=p)
        for name, fn in zip(names, fns):
            r[name] = round(timed(fn, args.launches, args.warmup), 2)
        rows.append(r)
        out.write(json.dumps(r) + "\n")
        out.flush()
    summary = dict(meta, what=what, pairs=args.pairs, launches=args.launches)
    for name in names:
        v = [r[name] for r in rows]
        summary[name] = {"median": round(statistics.median(v), 2), "min": min(v), "max": max(v)}
    for name in names[1:]:
        if name.endswith("_tree") == names[0].endswith("_tree"):
            summary[name + "_over_" + names[0]] = round(summary[name]["median"] / summary[names[0]]["median"], 3)
    out.write(json.dumps({"summary": summary}) + "\n")
    out.flush()
    print(json.dumps({"summary": summary}), flush=True)


def pieces_route(d_keys, kl, nk, logN, fb, nb, dbs, nrec, ans):
    """(answer, tree) closures of the pieces route from public entries, and what they evaluate."""
    import torch
    sp = max((128 * nb).bit_length() - 1 - 4, 7)
    pb, bs = logN - sp, sp - 7
    first, P = fb >> bs, ((fb + nb - 1) >> bs) - (fb >> bs) + 1
    sl, row = kl - 18 * pb, P * (16 << bs)
    off = 16 * (fb - (first << bs))
    sub = torch.empty(nk * P * sl, dtype=torch.uint8, device="cuda")
    rows = torch.empty(nk * row + 16, dtype=torch.uint8, device="cuda")
    work = torch.empty(dpf.pir_workspace_size(nk * P, sp, 0), dtype=torch.uint8, device="cuda")
    fwork = torch.empty(dpf.xor_fold_workspace_size(), dtype=torch.uint8, device="cuda")

    def tree():
        dpf.subkeys_dev(d_keys, kl, nk, logN, pb, first, P, sub)
        dpf.evalfull_batch_dev(sub, sl, nk * P, sp, rows, work)

    def answer():
        tree()
        dpf.xor_fold_sliced_any_dev(rows[off:], row, nk, dbs, nrec, REC, ans, fwork)

    return answer, tree, {"npieces": P, "piece_log": sp, "points_pieces": row * 8}


def shape(what, nk, logN, first_rec, nrec, b_pb, b_prefix, dbs, args, out):
    """Records [first_rec, first_rec + nrec) of dbs' table; b: the subtree (b_pb, b_prefix) that holds them."""
    import torch
    al, s0, s1 = synth.key_seeds(nk, logN, first=nk)
    al = np.uint64(first_rec) + al % np.uint64(nrec)          # every alpha inside the records
    ka, _ = dpf.gen_batch_seeded(al, logN, s0, s1)
    kl = ka.shape[1]
    d_keys = torch.from_numpy(ka.reshape(-1)).cuda()
    fb, nb = first_rec // 128, nrec // 128
    span = 1 << (logN - b_pb)                                  # b's points, from b_prefix * span
    b_off = first_rec - b_prefix * span
    assert 0 <= b_off and b_off + nrec <= span
    db = dbs[first_rec * REC:(first_rec + nrec) * REC]         # whole super-groups: a sliced DB of its own
    w_a = torch.empty(dpf.pir_window_workspace_size(nk, logN, first_rec, nrec, REC), dtype=torch.uint8, device="cuda")
    w_b = torch.empty(dpf.pir_workspace_size(nk, logN, b_pb), dtype=torch.uint8, device="cuda")
    fwork = torch.empty(dpf.xor_fold_workspace_size(), dtype=torch.uint8, device="cuda")
    ans = [torch.empty(nk * REC, dtype=torch.uint8, device="cuda") for _ in range(3)]
    f = dpf.window_form_for(logN, fb, nb)
    rows_a = torch.empty(nk * f.row_bytes, dtype=torch.uint8, device="cuda")
    rows_b = torch.empty(nk * span // 8 + 16, dtype=torch.uint8, device="cuda")

    def a():
        dpf.pir_answer_window_dev(d_keys, kl, nk, logN, first_rec, db, nrec, REC, ans[0], w_a)

    def a_tree():
        dpf.evalfull_window_dev(d_keys, kl, nk, logN, fb, nb, rows_a, f.row_bytes, w_a)

    def b_tree():
        dpf.evalfull_subtree_dev(d_keys, kl, nk, logN, b_pb, b_prefix, rows_b, w_b)

    if b_off == 0:
        def b():
            dpf.pir_answer_sliced_any_dev(d_keys, kl, nk, logN, db, nrec, REC, ans[1], w_b, prefix_bits=b_pb, prefix=b_prefix)
    else:
        def b():
            b_tree()
            dpf.xor_fold_sliced_any_dev(rows_b[b_off // 8:], span // 8, nk, db, nrec, REC, ans[1], fwork)

    p, p_tree, pm = pieces_route(d_keys, kl, nk, logN, fb, nb, db, nrec, ans[2])
    for fn in (a, b, p):
        fn()
    torch.cuda.synchronize()
    assert torch.equal(ans[0], ans[1]) and torch.equal(ans[0], ans[2]), "the routes' answers differ"
    assert ans[0].any(), "an all-zero answer checks nothing"
    meta = dict(pm, nkeys=nk, logN=logN, first_rec=first_rec, nrec=nrec, route=f.route, prefix_bits=f.prefix_bits,
                points_a=f.row_bytes * 8, points_b=span)
    run(what, ["a", "b", "p", "a_tree", "b_tree", "p_tree"], [a, b, p, a_tree, b_tree, p_tree], meta, args, out)
    for t in (w_a, w_b):
        dpf.forget_workspace(t)


def subkeys(args, out):
    import torch
    logN, nk = 24, 64
    _, s0, s1 = synth.key_seeds(nk, logN)
    ka, _ = dpf.gen_batch_seeded(np.arange(nk, dtype=np.uint64), logN, s0, s1)
    d_keys = torch.from_numpy(ka.reshape(-1)).cuda()
    d_sub = torch.empty(nk * 33 * ka.shape[1], dtype=torch.uint8, device="cuda")
    kl = ka.shape[1]
    run("k_subkeys", ["pieces32_levels5", "pieces33_levels6"],
        [lambda: dpf.subkeys_dev(d_keys, kl, nk, logN, 5, 0, 32, d_sub),
         lambda: dpf.subkeys_dev(d_keys, kl, nk, logN, 6, 7, 33, d_sub)], {"nkeys": nk, "logN": logN}, args, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pir_window", "ab.jsonl"))
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nrec", default="%d,%d,%d" % (5 << 21, (1 << 23) + 256, 1 << 24))
    ap.add_argument("--nkeys", default="1,16,64")
    args = ap.parse_args()
    import torch
    assert dpf.gpu_init(1) >= 1, "no gfx950 device"
    sizes = [int(x) for x in args.nrec.split(",")]
    assert all(n % 256 == 0 for n in sizes), "whole super-groups: a prefix of the sliced DB is a sliced DB"
    # One sliced DB of random records; every shape reads a prefix of it.
    dbs = torch.randint(0, 256, (max(sizes + [5 << 21]) * REC,), dtype=torch.uint8, device="cuda")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        subkeys(args, out)
        for nk in (int(x) for x in args.nkeys.split(",")):
            for nrec in sizes:
                shape("table", nk, int(nrec - 1).bit_length(), 0, nrec, 0, 0, dbs, args, out)
            shape("shard0_of_8", nk, 24, 0, 5 << 18, 3, 0, dbs, args, out)
            shape("shard0_of_8_subtree_split", nk, 24, 0, 1 << 21, 3, 0, dbs, args, out)
            shape("shard3_of_8", nk, 24, 15 << 18, 5 << 18, 1, 0, dbs, args, out)


if __name__ == "__main__":
    main()
