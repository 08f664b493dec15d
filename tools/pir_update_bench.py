#!/usr/bin/env python3
"""Cost of changing records of a resident PIR DB (profiles/pir_update/README.md).

For a 2^24 x 32-byte and a 2^22 x 256-byte DB on one GPU:
  (a) the route without an update entry: dpf_pir_db_free + dpf_pir_db_create_wide
      from the modified host DB (host clock; the call is synchronous);
  (b) k_slice_db over the whole device-resident row-major DB (device events);
  (c) dpf_pir_db_update_sliced_wide_dev for 1, 2^10, 2^16, 2^20 uniformly random
      records and for a dense contiguous run of 2^20 records (device events),
      with the bytes each must move -- 16 KiB per touched tile (8 KiB read and
      8 KiB written) plus the records and their indices -- and the share of
      the 6.2 TB/s streaming rate those bytes over the time come to.  Timed
      twice: repeated as it is (the same tiles every time: the small cases
      then run from the caches) and "cold", after 1 GiB of other memory was
      overwritten; the share is taken from the cold time.  One record is one
      launch between two events: launch and event overhead, not traffic;
  (d) the handle form of (c), PirDB.update from host arrays in random order
      and in sorted order (host clock; sort, split, PCIe and the kernel).
Every timed shape is warmed up first; figures are medians of --reps runs.
After the timed updates a sample of the records is read back and compared.

    python tools/pir_update_bench.py --out profiles/pir_update/pir_update.json
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

STREAM_TBS = 6.2   # measured streaming rate of the chip, TB/s


def ev_ms(fn, reps, warm=2, pre=None):
    """Device-event time of fn(); pre() is enqueued before the first event of
    every repetition (outside the timed window)."""
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if pre is not None:
            pre()
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def wall_ms(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def index_sets(nrec, rng):
    sets = []
    for n in (1, 1 << 10, 1 << 16, 1 << 20):
        sets.append(("random %d" % n, np.sort(rng.choice(nrec, n, replace=False)).astype(np.uint64)))
    sets.append(("dense run %d" % (1 << 20), (np.arange(1 << 20) + 12345).astype(np.uint64)))
    return sets


def run(logN, rec, reps, rng):
    import torch
    nrec = 1 << logN
    C = rec // 32
    db = rng.integers(0, 256, (nrec, rec), dtype=np.uint8)
    res = {"logN": logN, "rec_bytes": rec, "db_mib": nrec * rec >> 20, "update": []}

    holder = {"pdb": dpf.PirDB(db, logN, ngpus=1, rec_bytes=rec)}

    def recreate():
        holder["pdb"].close()
        holder["pdb"] = dpf.PirDB(db, logN, ngpus=1, rec_bytes=rec)
    res["recreate_ms"] = wall_ms(recreate, max(3, reps // 4))
    pdb = holder["pdb"]

    d_db = torch.from_numpy(db.reshape(-1)).cuda()
    d_dbs = torch.empty(dpf.pir_db_sliced_size_wide(nrec, rec), dtype=torch.uint8, device="cuda")
    res["slice_ms"] = ev_ms(lambda: dpf.pir_db_slice_wide_dev(d_db, nrec, rec, d_dbs), reps)
    del d_db
    # Every repetition of a case rewrites the same tiles, so without more the
    # small cases run from the L2 / the 256 MiB last-level cache.  The "cold"
    # figure overwrites 1 GiB of other memory before each repetition.
    flush = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")

    for name, idx in index_sets(nrec, rng):
        n = idx.size
        recs = rng.integers(0, 256, (n, rec), dtype=np.uint8)
        d_idx = torch.from_numpy(idx.view(np.int64)).cuda()
        d_recs = torch.from_numpy(recs.reshape(-1)).cuda()
        dev = ev_ms(lambda: dpf.pir_db_update_sliced_wide_dev(d_dbs, nrec, rec, d_idx, d_recs, n), reps)
        cold = ev_ms(lambda: dpf.pir_db_update_sliced_wide_dev(d_dbs, nrec, rec, d_idx, d_recs, n), reps,
                     pre=lambda: flush.fill_(1))
        tiles = int(np.unique(idx >> np.uint64(8)).size) * C
        nbytes = tiles * 16384 + n * (rec + 8)
        # read a sample back through the gather entry
        k = min(n, 64)
        d_out = torch.empty(max(k * rec, 16), dtype=torch.uint8, device="cuda")
        dpf.pir_db_gather_sliced_wide_dev(d_dbs, nrec, rec, d_idx[n - k:], k, d_out)
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy()[:k * rec].reshape(k, rec), recs[n - k:]), name
        perm = rng.permutation(n)
        hidx, hrecs = idx[perm], recs[perm]
        host = wall_ms(lambda: pdb.update(hidx, hrecs), max(3, reps // 4))
        assert np.array_equal(pdb.read(hidx[:k]), hrecs[:k]), name
        host_sorted = wall_ms(lambda: pdb.update(idx, recs), max(3, reps // 4))
        res["update"].append({"set": name, "n": n, "tiles": tiles, "bytes": nbytes, "dev_ms": dev,
                              "dev_cold_ms": cold,
                              "dev_share_of_stream": nbytes / (cold[0] * 1e-3) / (STREAM_TBS * 1e12),
                              "handle_ms": host, "handle_sorted_ms": host_sorted})
        del d_idx, d_recs
    pdb.close()
    del flush
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--shapes", default="24x32,22x256", help="logN x rec_bytes, comma separated")
    a = ap.parse_args()
    import torch
    assert dpf.gpu_init(1) >= 1
    rng = np.random.default_rng(2024)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "shapes": []}
    for s in a.shapes.split(","):
        logN, rec = (int(x) for x in s.split("x"))
        r = run(logN, rec, a.reps, rng)
        out["shapes"].append(r)
        print("## 2^%d x %d B (%d MiB): free + create %.1f ms, k_slice_db of the whole DB %.3f ms"
              % (logN, rec, r["db_mib"], r["recreate_ms"][0], r["slice_ms"][0]))
        print("| update | touched tiles | bytes to move | device ms, repeated (min-max) | device ms, cold (min-max) | cold: of %.1f TB/s | handle ms (min-max) | handle ms, sorted input |" % STREAM_TBS)
        print("|---|---|---|---|---|---|---|---|")
        for u in r["update"]:
            print("| %s | %d | %.2f MiB | %.4f (%.4f-%.4f) | %.4f (%.4f-%.4f) | %.1f %% | %.3f (%.3f-%.3f) | %.3f |"
                  % (u["set"], u["tiles"], u["bytes"] / 2 ** 20, *u["dev_ms"], *u["dev_cold_ms"], 100 * u["dev_share_of_stream"],
                     *u["handle_ms"], u["handle_sorted_ms"][0]))
        sys.stdout.flush()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
