"""Time of the matrix-core fold over the sliced DB (and, with --op, of the
slicing, the private write's scatter and the in-place update) by record width, for A/B runs
of two builds of the library: one process measures one library (raw ctypes,
so a build from before the _any entry points loads too), and a driver
alternates processes of the two builds in pairs.  The DB and the selection
bits are random device bytes (the fold's time does not depend on them).

  python tools/fold_any_ab.py --lib dpf-go_amd/lib/libdpf_hip.so --entry any --widths 16,32,48,64 \
      [--nrec 16777216] [--nkeys 1,16,64] [--steps 30] [--reps 3] [--op fold|slice|scatter|update]
(--op update: --nkeys is the number of updates, sorted random indices.)

Prints one JSON line per (width, nkeys): the median over --reps of the mean
time of --steps folds between two synchronizes, and every repeat."""
import argparse
import ctypes
import json
import time

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--entry", choices=("any", "wide"), default="any")
    ap.add_argument("--widths", default="16,32,48,64")
    ap.add_argument("--nkeys", default="1,16,64")
    ap.add_argument("--nrec", type=int, default=1 << 24)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tag", default="")
    ap.add_argument("--op", choices=("fold", "slice", "scatter", "update"), default="fold")
    a = ap.parse_args()
    L = ctypes.CDLL(a.lib)
    vp, sz, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64
    fold = getattr(L, "dpf_xor_fold_sliced_%s_dev" % a.entry)
    fold.restype = ctypes.c_int
    fold.argtypes = [ctypes.c_int, vp, sz, sz, vp, u64, sz, vp, vp, vp]
    slice_ = getattr(L, "dpf_pir_db_slice_%s_dev" % a.entry)
    slice_.argtypes = [ctypes.c_int, vp, u64, sz, vp, vp]
    scatter = getattr(L, "dpf_xor_scatter_sliced_%s_dev" % a.entry)
    scatter.argtypes = [ctypes.c_int, vp, sz, sz, vp, vp, u64, sz, vp]
    update = getattr(L, "dpf_pir_db_update_sliced_%s_dev" % a.entry)
    update.argtypes = [ctypes.c_int, vp, u64, sz, vp, vp, sz, vp]
    L.dpf_xor_fold_workspace_size.restype = sz
    assert L.dpf_gpu_init(1) >= 1
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    nrec = a.nrec
    stride = (nrec // 8 + 15) // 16 * 16
    widths = [int(w) for w in a.widths.split(",")]
    nkeys = [int(k) for k in a.nkeys.split(",")] if a.op != "slice" else [0]
    d_work = torch.empty(L.dpf_xor_fold_workspace_size(), dtype=torch.uint8, device=dev)
    d_bits = torch.randint(0, 256, (max(nkeys) * stride if a.op in ("fold", "scatter") else 16,), dtype=torch.uint8,
                           device=dev)
    for w in widths:
        d_dbs = torch.randint(0, 256, ((nrec + 255) // 256 * 256 * w,), dtype=torch.uint8, device=dev)
        d_ans = torch.randint(0, 256, (max(max(nkeys) * w, 16),), dtype=torch.uint8, device=dev)   # answers / messages / records
        d_db = d_dbs.clone() if a.op == "slice" else None                         # a row-major DB of the same size
        for nk in nkeys:
            d_idx = torch.sort(torch.randint(0, nrec, (max(nk, 1),), dtype=torch.int64, device=dev)).values

            def run(n):
                for _ in range(n):
                    if a.op == "fold":
                        rc = fold(0, d_bits.data_ptr(), stride, nk, d_dbs.data_ptr(), nrec, w, d_ans.data_ptr(),
                                  d_work.data_ptr(), st.cuda_stream)
                    elif a.op == "slice":
                        rc = slice_(0, d_db.data_ptr(), nrec, w, d_dbs.data_ptr(), st.cuda_stream)
                    elif a.op == "scatter":
                        rc = scatter(0, d_bits.data_ptr(), stride, nk, d_ans.data_ptr(), d_dbs.data_ptr(), nrec, w,
                                     st.cuda_stream)
                    else:
                        rc = update(0, d_dbs.data_ptr(), nrec, w, d_idx.data_ptr(), d_ans.data_ptr(), nk, st.cuda_stream)
                    assert rc == 0, rc
                torch.cuda.synchronize()
            run(5)                                             # warm-up
            us = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                run(a.steps)
                us.append((time.perf_counter() - t0) / a.steps * 1e6)
            us.sort()
            print(json.dumps({"tag": a.tag, "op": a.op, "entry": a.entry, "rec_bytes": w, "nkeys": nk, "nrec": nrec,
                              "us": round(us[len(us) // 2], 2), "all_us": [round(x, 2) for x in us]}), flush=True)
        del d_dbs, d_ans


if __name__ == "__main__":
    main()
