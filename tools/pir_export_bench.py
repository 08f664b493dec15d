#!/usr/bin/env python3
"""Cost of reading a resident PIR DB out whole (profiles/pir_export/README.md).

Kernel, per shape (2^24 x 32 B, 2^22 x 256 B, 2^24 x 16 B) on one GPU, device
events, every round timing each of these once, one after the other, so that
the figures of a round share the chip's state (interleaved A/B):
  unslice  dpf_pir_db_unslice_any_dev of the whole DB (k_unslice_db);
  (a)      dpf_pir_db_slice_any_dev over the same DB (k_slice_db, the mirror traffic);
  (b)      a device-to-device copy of the same bytes;
  (c)      the only route before: dpf_pir_db_gather_sliced_any_dev with idx = arange(nrec);
  xor      dpf_pir_db_xor_sliced_dev over the same bytes (k_xor_words).
Medians over --reps rounds after --warm rounds, min-max beside them, and the
number of rounds in which unslice beat (c).  The un-sliced rows are compared
with the DB before anything is timed.

Handle (--handle), host clock, whole DB: PirDB.export() against
PirDB.read(arange(nrec)), and PirDB.xor_records(whole DB) and PirDB.clear()
against close + PirDB(...) (free + create).

    python tools/pir_export_bench.py --handle --out profiles/pir_export/pir_export.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dpf-go_amd"))

import dpf  # noqa: E402


def stats(ts):
    return [float(np.median(ts)), float(min(ts)), float(max(ts))]


def kernel_rounds(cases, reps, warm):
    """cases: [(name, fn)].  Every round times each case once, in order."""
    import torch
    ts = {name: [] for name, _ in cases}
    for r in range(warm + reps):
        for name, fn in cases:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warm:
                ts[name].append(a.elapsed_time(b))
    return ts


def wall_ms(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return stats(ts)


def run_kernel(logN, rec, reps, warm, rng):
    import torch
    nrec = 1 << logN
    nbytes = nrec * rec
    db = rng.integers(0, 256, (nrec, rec), dtype=np.uint8)
    d_db = torch.from_numpy(db.reshape(-1)).cuda()
    d_dbs = torch.empty(dpf.pir_db_sliced_size_any(nrec, rec), dtype=torch.uint8, device="cuda")
    d_out = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    d_idx = torch.arange(nrec, dtype=torch.int64, device="cuda")
    dpf.pir_db_slice_any_dev(d_db, nrec, rec, d_dbs)
    dpf.pir_db_unslice_any_dev(d_dbs, nrec, rec, d_out)
    torch.cuda.synchronize()
    assert torch.equal(d_out, d_db), "unslice(slice(db)) != db"
    d_other = d_dbs.clone()
    cases = [("unslice", lambda: dpf.pir_db_unslice_any_dev(d_dbs, nrec, rec, d_out)),
             ("slice", lambda: dpf.pir_db_slice_any_dev(d_db, nrec, rec, d_other)),
             ("copy", lambda: d_out.copy_(d_db)),
             ("gather", lambda: dpf.pir_db_gather_sliced_any_dev(d_dbs, nrec, rec, d_idx, nrec, d_out)),
             ("xor", lambda: dpf.pir_db_xor_sliced_dev(d_other, d_dbs, nbytes))]
    ts = kernel_rounds(cases, reps, warm)
    res = {"kind": "kernel", "logN": logN, "rec_bytes": rec, "db_mib": nbytes >> 20, "reps": reps}
    for name, _ in cases:
        res[name + "_ms"] = stats(ts[name])
    res["unslice_gbs"] = 2 * nbytes / (res["unslice_ms"][0] * 1e-3) / 1e9            # read + written
    res["unslice_beats_gather_rounds"] = int(sum(u < g for u, g in zip(ts["unslice"], ts["gather"])))
    res["unslice_over_slice"] = res["unslice_ms"][0] / res["slice_ms"][0]
    res["unslice_over_copy"] = res["unslice_ms"][0] / res["copy_ms"][0]
    res["gather_over_unslice"] = res["gather_ms"][0] / res["unslice_ms"][0]
    return res


def run_handle(logN, rec, reps, rng):
    nrec = 1 << logN
    db = rng.integers(0, 256, (nrec, rec), dtype=np.uint8)
    holder = {"pdb": dpf.PirDB(db, logN, ngpus=1, rec_bytes=rec)}

    def recreate():
        holder["pdb"].close()
        holder["pdb"] = dpf.PirDB(db, logN, ngpus=1, rec_bytes=rec)
    res = {"kind": "handle", "logN": logN, "rec_bytes": rec, "db_mib": nrec * rec >> 20, "reps": reps}
    res["recreate_ms"] = wall_ms(recreate, reps)
    pdb = holder["pdb"]
    everything = np.arange(nrec, dtype=np.uint64)
    assert np.array_equal(pdb.export(), db)
    res["export_ms"] = wall_ms(pdb.export, reps)
    res["read_all_ms"] = wall_ms(lambda: pdb.read(everything), reps)
    res["xor_records_ms"] = wall_ms(lambda: pdb.xor_records(db), reps)
    res["clear_ms"] = wall_ms(pdb.clear, reps)
    pdb.xor_records(db)
    assert np.array_equal(pdb.export(1000, 4096), db[1000:5096])
    pdb.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--tag", default="", help="copied into every result line")
    ap.add_argument("--shapes", default="24x32,22x256,24x16", help="logN x rec_bytes, comma separated")
    ap.add_argument("--handle", action="store_true", help="also time the handle's export / xor_records / clear")
    ap.add_argument("--handle-shapes", default="24x32,22x256")
    a = ap.parse_args()
    import torch
    assert dpf.gpu_init(1) >= 1
    rng = np.random.default_rng(2025)
    lines = []
    print("| shape | unslice ms (min-max) | (a) slice | (b) copy | (c) gather, arange | xor | unslice GB/s | / (a) | / (b) | (c) / unslice | rounds unslice < (c) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for s in a.shapes.split(","):
        logN, rec = (int(x) for x in s.split("x"))
        r = run_kernel(logN, rec, a.reps, a.warm, rng)
        lines.append(r)
        print("| 2^%d x %d B | %.3f (%.3f-%.3f) | %.3f | %.3f | %.3f | %.3f | %.0f | %.2f | %.2f | %.1f | %d / %d |"
              % (logN, rec, *r["unslice_ms"], r["slice_ms"][0], r["copy_ms"][0], r["gather_ms"][0], r["xor_ms"][0],
                 r["unslice_gbs"], r["unslice_over_slice"], r["unslice_over_copy"], r["gather_over_unslice"],
                 r["unslice_beats_gather_rounds"], a.reps))
        sys.stdout.flush()
    if a.handle:
        print("| shape | export() ms (min-max) | read(arange) ms | xor_records(all) ms | clear() ms | free + create ms |")
        print("|---|---|---|---|---|---|")
        for s in a.handle_shapes.split(","):
            logN, rec = (int(x) for x in s.split("x"))
            r = run_handle(logN, rec, max(3, a.reps // 5), rng)
            lines.append(r)
            print("| 2^%d x %d B | %.1f (%.1f-%.1f) | %.1f | %.1f | %.2f | %.1f |"
                  % (logN, rec, *r["export_ms"], r["read_all_ms"][0], r["xor_records_ms"][0], r["clear_ms"][0],
                     r["recreate_ms"][0]))
            sys.stdout.flush()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in lines:
                r["device"] = torch.cuda.get_device_name(0)
                if a.tag:
                    r["tag"] = a.tag
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
