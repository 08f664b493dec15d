#!/usr/bin/env python3
"""Grouped private writes (dpf_pir_write_grouped_dev) against the way the
library offered before them for the same writes, and against the memory floor.

A table of 2^--log-n records of --rec-bytes is kept 3-fold replicated in b
groups (the buckets of a batch code), 3 n / b records a group.  Timed per b:
  (a) dpf_pir_write_grouped_dev over the b groups, kpg keys each;
  (b) the same work without the grouped scatter: one tree pass of the b * kpg
      keys at the group's logN (dpf_evalfull_batch_dev), then one
      dpf_xor_scatter_sliced_any_dev per group on that group's part of the
      grouped layout.  Its per-group calls are issued from Python; what is
      measured is the time the device needs to get through them, which is
      bounded below by the host's issue rate: that cost is part of (b);
  (c) a device-to-device copy of the grouped DB: one read and one write of
      every byte, the floor of any scatter pass.
Then at 96 groups a sweep over keys_per_group with the scatters alone beside
the composites (the tree pass is common to all): a_grouped and a_loop are
dpf_xor_scatter_grouped_dev with the route forced to the grouped kernel and to
the launcher's own loop of dense scatters (DPF_GROUP_SCATTER_ROUTE, read at
every call), a_rule the route the plan's rule picks, b_scatter the Python loop
of (b).  The crossover of a_grouped and a_loop is what the route rule of
csrc/pir_group_scatter_plan.hpp is fitted to.

One MI355X, one process, the variants alternate inside every pair.  A figure
is the mean of --launches calls between two device events (warm-up calls
first), in microseconds; the summary gives the median over the pairs, the
min-max spread and in how many pairs (a) beat (b).  The DBs that (a), both
forced routes and (b) leave are compared byte for byte before anything is
timed.  The DB bytes are random: the kernels' time does not depend on them.

    python tools/grouped_write_ab.py --out profiles/grouped_write/ab.jsonl
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

KNOB = "DPF_GROUP_SCATTER_ROUTE"


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


def forced(route, fn):
    def run():
        os.environ[KNOB] = route
        try:
            fn()
        finally:
            os.environ.pop(KNOB, None)
    return run


def grouped(ng, kpg, cap, rec, dbs, spare, args, out, tag, floor):
    """(a), (b), the scatters alone and (c) over ng groups of cap records; returns the summary."""
    import torch
    logN = max(7, (cap - 1).bit_length())
    nk = ng * kpg
    ka = keys_for(nk, logN, cap)
    kl = ka.shape[1]
    d_keys = torch.from_numpy(ka.reshape(-1)).cuda()
    msgs = random_bytes(nk * rec)
    gs = dpf.pir_group_stride(cap)
    stride = dpf.evalfull_len(logN)
    size = ng * gs * rec
    w_a = torch.empty(dpf.pir_grouped_workspace_size(ng, kpg, logN, rec), dtype=torch.uint8, device="cuda")
    w_tree = torch.empty(dpf.workspace_size(nk, logN), dtype=torch.uint8, device="cuda")
    bits = torch.empty(nk * stride, dtype=torch.uint8, device="cuda")
    db_of = [dbs[g * gs * rec:(g + 1) * gs * rec] for g in range(ng)]
    bits_of = [bits[g * kpg * stride:(g + 1) * kpg * stride] for g in range(ng)]
    msgs_of = [msgs[g * kpg * rec:(g + 1) * kpg * rec] for g in range(ng)]
    form = dpf.scatter_grouped_form_for(ng, kpg, cap, rec)

    def a():
        dpf.pir_write_grouped_dev(d_keys, kl, ng, kpg, logN, msgs, dbs, cap, rec, w_a)

    def tree():
        dpf.evalfull_batch_dev(d_keys, kl, nk, logN, bits, w_tree)

    def b_scatter():
        for g in range(ng):
            dpf.xor_scatter_sliced_any_dev(bits_of[g], stride, kpg, msgs_of[g], db_of[g], cap, rec)

    def b():
        tree()
        b_scatter()

    def a_rule():
        dpf.xor_scatter_grouped_dev(bits, stride, ng, kpg, msgs, dbs, cap, rec)

    a_grouped, a_loop = forced("grouped", a_rule), forced("loop", a_rule)

    # Every way leaves the same DB, byte for byte, from the same start.
    spare[:size].copy_(dbs[:size])
    a()
    torch.cuda.synchronize()
    after = dbs[:size].clone()
    assert not torch.equal(spare[:size], after), "the write changed nothing"
    for name, way in (("b", b), ("a_grouped", a_grouped), ("a_loop", a_loop), ("b_scatter", b_scatter)):
        dbs[:size].copy_(spare[:size])
        way()                                  # (the bits are those of the tree pass that b ran)
        torch.cuda.synchronize()
        assert torch.equal(dbs[:size], after), "%s does not leave the DB that (a) leaves" % name
    del after

    names = ["a", "b", "a_rule", "a_grouped", "a_loop", "b_scatter", "tree", "c"]
    fns = [a, b, a_rule, a_grouped, a_loop, b_scatter, tree, lambda: floor(size)]
    rows = []
    for p in range(args.pairs):
        r = dict(tag, ngroups=ng, kpg=kpg, cap=cap, logN=logN, rec_bytes=rec, pair=p, route=form.route)
        for name, fn in zip(names, fns):
            r[name] = round(timed(fn, args.launches, args.warmup), 2)
        rows.append(r)
        out.write(json.dumps(r) + "\n")
        out.flush()
    s = dict(tag, ngroups=ng, kpg=kpg, cap=cap, logN=logN, rec_bytes=rec, pairs=args.pairs, launches=args.launches,
             route=form.route, passes=form.passes, db_bytes=size,
             a_beats_b=sum(r["a"] < r["b"] for r in rows),
             grouped_beats_loop=sum(r["a_grouped"] < r["a_loop"] for r in rows))
    for name in names:
        v = [r[name] for r in rows]
        s[name] = {"median": round(statistics.median(v), 2), "min": min(v), "max": max(v)}
    s["a_over_c"] = round(s["a"]["median"] / s["c"]["median"], 3)
    s["a_grouped_over_c"] = round(s["a_grouped"]["median"] / s["c"]["median"], 3)
    out.write(json.dumps({"summary": s}) + "\n")
    out.flush()
    print(json.dumps({"summary": s}), flush=True)
    for t in (w_a, w_tree):
        dpf.forget_workspace(t)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_write", "ab.jsonl"))
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log-n", type=int, default=24)
    ap.add_argument("--rec-bytes", type=int, default=32)
    ap.add_argument("--groups", default="96,384")
    ap.add_argument("--kpg", default="1,2,4,8,16,64")
    args = ap.parse_args()
    assert dpf.gpu_init(1) >= 1, "no gfx950 device"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    n, rec = 1 << args.log_n, args.rec_bytes
    dbs3 = random_bytes(3 * n * rec)          # the replicated table: every group count below divides 3 n
    spare = random_bytes(3 * n * rec)         # the copy's target, and the DB's state before the writes

    def floor(size):
        spare[:size].copy_(dbs3[:size])

    with open(args.out, "w") as out:
        for b in (int(x) for x in args.groups.split(",") if x):
            assert (3 * n) % b == 0 and (3 * n // b) % 256 == 0, "groups of whole super-groups only"
            grouped(b, 1, 3 * n // b, rec, dbs3, spare, args, out, {"what": "groups"}, floor)
        for kpg in (int(x) for x in args.kpg.split(",") if x):
            grouped(96, kpg, 3 * n // 96, rec, dbs3, spare, args, out, {"what": "kpg"}, floor)


if __name__ == "__main__":
    main()
