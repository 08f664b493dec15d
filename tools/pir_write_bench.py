#!/usr/bin/env python3
"""Cost of a private write into a resident sliced PIR DB (profiles/pir_write/README.md).

For each shape (2^logN records of rec_bytes, B keys) on one GPU, by device
events after a warm-up, medians of --reps runs with their range:
  tree     the subtree EvalFull of the B keys into the workspace
           (dpf_evalfull_subtree_dev: the tree launch of the write);
  scatter  dpf_xor_scatter_sliced_wide_dev over those selection bits
           (k_scatter_sliced: one pass over the DB per 64 keys);
  write    the whole dpf_pir_write_sliced_wide_dev step;
  copy     hipMemcpyDtoDAsync of the same sliced buffer, in the same run: the
           floor, the same bytes read once and written once.
Before the timed runs the two servers' shares of one batch are applied to the
same buffer and a sample of records (the alphas among them) is read back: the
DB must have changed at the alphas only, by the messages written there.

    python tools/pir_write_bench.py --out profiles/pir_write/pir_write.json
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dpf-go_amd"))

import dpf  # noqa: E402
from dpf import synth  # noqa: E402

SHAPES = "24x32x1,24x32x16,24x32x64,24x32x256,23x64x16,23x64x64,19x1024x16,19x1024x64"


def hip_runtime():
    """The HIP runtime this process already has loaded (torch's): one runtime per process."""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no libamdhip64 loaded in this process")


INNER = 5   # calls between one pair of events: the window is a millisecond or more


def ev_ms(fn, reps, warm=3):
    """Device-event time of one fn(): each repetition times INNER back-to-back calls."""
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(INNER):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / INNER)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def run(logN, rec, B, reps, hip, rng):
    import torch
    nrec = 1 << logN
    size = dpf.pir_db_sliced_size_wide(nrec, rec)
    kl = dpf.key_len(logN)
    al, s0, s1 = synth.key_seeds(B, logN, first=7000)
    ka, kb = dpf.gen_batch_seeded(al, logN, s0, s1)
    msgs = rng.integers(0, 256, (B, rec), dtype=np.uint8)
    d_ka, d_kb = torch.from_numpy(ka.reshape(-1)).cuda(), torch.from_numpy(kb.reshape(-1)).cuda()
    d_msgs = torch.from_numpy(msgs.reshape(-1)).cuda()
    # Any sliced buffer is a DB: random words (2^logN is a multiple of 256, so there is no padding).
    d_dbs = torch.randint(0, 2 ** 31 - 1, (size // 4,), dtype=torch.int32, device="cuda").view(torch.uint8)
    d_copy = torch.empty_like(d_dbs)
    d_work = torch.empty(dpf.pir_workspace_size(B, logN, 0), dtype=torch.uint8, device="cuda")
    stride = dpf.evalfull_len(logN)
    d_bits = torch.empty(B * stride, dtype=torch.uint8, device="cuda")

    # Check: A's and B's shares of the batch change the DB at the alphas only.
    sample = np.unique(np.concatenate([al, rng.integers(0, nrec, 256).astype(np.uint64)]))
    d_idx = torch.from_numpy(sample.view(np.int64)).cuda()

    def gather():
        d_out = torch.empty(sample.size * rec, dtype=torch.uint8, device="cuda")
        dpf.pir_db_gather_sliced_wide_dev(d_dbs, nrec, rec, d_idx, sample.size, d_out)
        torch.cuda.synchronize()
        return d_out.cpu().numpy().reshape(sample.size, rec)
    before = gather()
    for d_k in (d_ka, d_kb):
        dpf.pir_write_sliced_wide_dev(d_k, kl, B, logN, d_msgs, d_dbs, nrec, rec, d_work)
    delta = np.zeros_like(before)
    for k in range(B):
        delta[np.searchsorted(sample, al[k])] ^= msgs[k]
    assert np.array_equal(gather(), before ^ delta), "two-server check failed"

    ts = torch.cuda.current_stream()
    st = ts.cuda_stream

    def copy():
        rc = hip.hipMemcpyDtoDAsync(ctypes.c_void_p(d_copy.data_ptr()), ctypes.c_void_p(d_dbs.data_ptr()),
                                    ctypes.c_size_t(size), ctypes.c_void_p(st))
        assert rc == 0, rc

    r = {"logN": logN, "rec_bytes": rec, "nkeys": B, "db_mib": size >> 20, "bits_mib": B * stride >> 20}
    r["copy_ms"] = ev_ms(copy, reps)
    r["tree_ms"] = ev_ms(lambda: dpf.evalfull_subtree_dev(d_ka, kl, B, logN, 0, 0, d_bits, d_work, stream=ts), reps)
    r["scatter_ms"] = ev_ms(lambda: dpf.xor_scatter_sliced_wide_dev(d_bits, stride, B, d_msgs, d_dbs, nrec, rec,
                                                                    stream=ts), reps)
    r["write_ms"] = ev_ms(lambda: dpf.pir_write_sliced_wide_dev(d_ka, kl, B, logN, d_msgs, d_dbs, nrec, rec, d_work,
                                                                stream=ts), reps)
    r["copy_again_ms"] = ev_ms(copy, reps)                      # the floor once more, after the others
    r["scatter_over_copy"] = r["scatter_ms"][0] / min(r["copy_ms"][0], r["copy_again_ms"][0])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--shapes", default=SHAPES, help="logN x rec_bytes x keys, comma separated")
    a = ap.parse_args()
    import torch
    assert dpf.gpu_init(1) >= 1
    hip = hip_runtime()
    hip.hipMemcpyDtoDAsync.restype = ctypes.c_int
    rng = np.random.default_rng(2025)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "shapes": []}
    print("| records x bytes | keys | copy us (min-max) | tree us | scatter us (min-max) | write us | scatter / copy |")
    print("|---|---|---|---|---|---|---|")
    for s in a.shapes.split(","):
        logN, rec, B = (int(x) for x in s.split("x"))
        r = run(logN, rec, B, a.reps, hip, rng)
        out["shapes"].append(r)
        c = min(r["copy_ms"], r["copy_again_ms"])
        print("| 2^%d x %d | %d | %.1f (%.1f-%.1f) | %.1f | %.1f (%.1f-%.1f) | %.1f | %.2f |"
              % (logN, rec, B, c[0] * 1e3, c[1] * 1e3, c[2] * 1e3, r["tree_ms"][0] * 1e3, r["scatter_ms"][0] * 1e3,
                 r["scatter_ms"][1] * 1e3, r["scatter_ms"][2] * 1e3, r["write_ms"][0] * 1e3, r["scatter_over_copy"]))
        sys.stdout.flush()
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
