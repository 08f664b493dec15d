#!/usr/bin/env python3
"""Grouped PIR with many keys per group: the matrix-core grouped fold against
the direct one, against the parent commit's library and against a per-group
loop of the dense matrix-core fold.

A table of 2^24 records is kept 3-fold replicated as ngroups buckets (a batch
code); a server that batches the queries of kpg clients answers kpg keys per
bucket.  Timed per (shape, kpg), the fold alone (*_fold) and the composite
answer with its tree pass:
  a         this build, the route its rule picks;
  a_mfma    this build, DPF_GROUP_FOLD_ROUTE=mfma;
  a_direct  this build, DPF_GROUP_FOLD_ROUTE=direct;
  p         the library given by --parent-lib (built from the parent commit
            into a directory of its own), in a worker process of its own;
  b         one dense dpf_xor_fold_sliced_any_dev per group (after one tree
            pass of all keys for the composite), issued from Python.

Method, that of tools/grouped_pir_ab.py: one MI355X; a figure is the mean of
--launches calls between two device events after --warmup calls, in
microseconds; --pairs pairs, every variant once per pair and the order rotated
from pair to pair; median and min-max per variant.  Two worker processes (this
build, the parent) hold the same DB and keys (same seeds) and are driven in
turn by this process, which never opens the device: only one of them has work
on the GPU at a time.  Before anything is timed every variant's answers are
compared byte for byte inside a worker and by SHA-256 between the workers.
The DB bytes are random: the kernels' time does not depend on them.
Control: --parent-lib set to this build's own library times the same code in
both workers, which shows what the second process alone contributes.

    python tools/grouped_pir_keys_ab.py --parent-lib /path/to/parent/libdpf_hip.so \
        --out profiles/grouped_pir_mfma/ab.jsonl
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = "DPF_GROUP_FOLD_ROUTE"
# (name, ngroups, records per group, rec_bytes, keys per group)
KPG = (4, 5, 8, 12, 16, 32, 64, 256)
SHAPES = [("96x2^19x32", 96, 1 << 19, 32, KPG), ("384x2^17x32", 384, 1 << 17, 32, KPG),
          ("96x2^16x256", 96, 1 << 16, 256, (4, 8, 16, 64)), ("4096x2^12x32", 4096, 1 << 12, 32, (4, 8, 16, 64))]


# ---- worker: holds the device, runs what it is told -----------------------------
def worker():
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "dpf-go_amd"))
    import ctypes
    import dpf
    from dpf import synth
    probe = ctypes.CDLL(dpf.LIB_PATH)
    for name in list(dpf.SIGNATURES):          # an older library: without the entries it does not have
        if not hasattr(probe, name):
            del dpf.SIGNATURES[name]
    has_form = "dpf_fold_grouped_form_for" in dpf.SIGNATURES
    assert dpf.gpu_init(1) >= 1, "no gfx950 device"
    st = {}

    def timed(fn, launches, warmup):
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

    def setup(ng, cap, rec, kpg):
        for t in st.get("work", ()):
            dpf.forget_workspace(t)
        st.clear()
        torch.cuda.empty_cache()
        logN = max(7, (cap - 1).bit_length())
        nk = ng * kpg
        al, s0, s1 = synth.key_seeds(nk, logN, first=nk + logN)
        ka, _ = dpf.gen_batch_seeded(al % np.uint64(cap), logN, s0, s1)
        kl = ka.shape[1]
        d_keys = torch.from_numpy(ka.reshape(-1)).cuda()
        gs, stride = dpf.pir_group_stride(cap), dpf.evalfull_len(logN)
        torch.manual_seed(ng * 31 + rec)
        dbs = torch.empty(ng * gs * rec, dtype=torch.uint8, device="cuda")
        for o in range(0, dbs.numel(), 1 << 28):
            dbs[o:o + (1 << 28)].random_(0, 256)
        u8 = lambda n: torch.empty(n, dtype=torch.uint8, device="cuda")
        w_a, w_tree = u8(dpf.pir_grouped_workspace_size(ng, kpg, logN, rec)), u8(dpf.workspace_size(nk, logN))
        bits, w_fold = u8(nk * stride), u8(dpf.xor_fold_workspace_size())
        w_gfold = u8(dpf.xor_fold_grouped_workspace_size(ng, kpg, rec))
        ans, ans_b = u8(nk * rec), u8(nk * rec)
        db_of = [dbs[g * gs * rec:(g + 1) * gs * rec] for g in range(ng)]
        bits_of = [bits[g * kpg * stride:(g + 1) * kpg * stride] for g in range(ng)]
        ans_of = [ans_b[g * kpg * rec:(g + 1) * kpg * rec] for g in range(ng)]
        st["work"] = (w_a, w_tree)

        def route(knob):
            if knob is None:
                os.environ.pop(KNOB, None)
            else:
                os.environ[KNOB] = knob

        def answer(knob):
            def f():
                route(knob)
                dpf.pir_answer_grouped_dev(d_keys, kl, ng, kpg, logN, dbs, cap, rec, ans, w_a)
            return f

        def fold(knob):
            def f():
                route(knob)
                dpf.xor_fold_grouped_dev(bits, stride, ng, kpg, dbs, cap, rec, ans, w_gfold)
            return f

        def tree():
            dpf.evalfull_batch_dev(d_keys, kl, nk, logN, bits, w_tree)

        def b_fold():
            for g in range(ng):
                dpf.xor_fold_sliced_any_dev(bits_of[g], stride, kpg, db_of[g], cap, rec, ans_of[g], w_fold)

        def b():
            tree()
            b_fold()

        st["fns"] = {"a": answer(None), "a_mfma": answer("mfma"), "a_direct": answer("direct"), "p": answer(None), "b": b,
                     "a_fold": fold(None), "a_mfma_fold": fold("mfma"), "a_direct_fold": fold("direct"),
                     "p_fold": fold(None), "b_fold": b_fold, "tree": tree}
        # Answers before timing: the per-group loop is the reference inside this worker.
        b()
        torch.cuda.synchronize()
        ref = ans_b.clone()
        for name in ("a", "a_mfma", "a_direct", "a_fold", "a_mfma_fold", "a_direct_fold"):
            ans.fill_(0x33)
            st["fns"][name]()
            torch.cuda.synchronize()
            assert torch.equal(ans, ref), "%s differs from the per-group folds" % name
        route(None)
        out = {"sha": hashlib.sha256(ref.cpu().numpy().tobytes()).hexdigest(), "logN": logN}
        if has_form:
            for knob in (None, "mfma", "direct"):
                route(knob)
                out["form_" + str(knob)] = dpf.fold_grouped_form_for(ng, kpg, cap, rec)._asdict()
            route(None)
        return out

    for line in sys.stdin:
        req = json.loads(line)
        if req["cmd"] == "setup":
            rep = setup(req["ng"], req["cap"], req["rec"], req["kpg"])
        elif req["cmd"] == "time":
            rep = {"us": round(timed(st["fns"][req["name"]], req["launches"], req["warmup"]), 2)}
            os.environ.pop(KNOB, None)
        else:
            break
        sys.stdout.write(json.dumps(rep) + "\n")
        sys.stdout.flush()
    dpf.gpu_shutdown()


# ---- driver --------------------------------------------------------------------
class Worker:
    def __init__(self, lib):
        env = dict(os.environ)
        env.pop(KNOB, None)
        if lib:
            env["DPF_LIB"] = os.path.abspath(lib)
        else:
            env.pop("DPF_LIB", None)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True, env=env)

    def ask(self, **req):
        self.p.stdin.write(json.dumps(req) + "\n")
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError("a worker ended (exit %s) on %r" % (self.p.wait(), req))
        return json.loads(line)

    def close(self):
        try:
            self.p.stdin.write(json.dumps({"cmd": "end"}) + "\n")
            self.p.stdin.close()
        except OSError:
            pass
        self.p.wait(timeout=60)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--parent-lib", default="", help="the parent commit's libdpf_hip.so (variant p); empty: no p")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_pir_mfma", "ab.jsonl"))
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="", help="comma-separated names out of: " + ", ".join(s[0] for s in SHAPES))
    ap.add_argument("--kpg", default="", help="comma-separated keys per group out of each shape's list (default: all)")
    args = ap.parse_args()
    if args.worker:
        return worker()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    new, old = Worker(""), Worker(args.parent_lib) if args.parent_lib else None
    names = ["a", "a_mfma", "a_direct", "b", "a_fold", "a_mfma_fold", "a_direct_fold", "b_fold", "tree"]
    if old:
        names += ["p", "p_fold"]
    picked = [s for s in SHAPES if not args.shapes or s[0] in args.shapes.split(",")]
    try:
        with open(args.out, "w") as out:
            for shape, ng, cap, rec, kpgs in picked:
                for kpg in kpgs:
                    if args.kpg and str(kpg) not in args.kpg.split(","):
                        continue
                    info = new.ask(cmd="setup", ng=ng, cap=cap, rec=rec, kpg=kpg)
                    if old:
                        assert old.ask(cmd="setup", ng=ng, cap=cap, rec=rec, kpg=kpg)["sha"] == info["sha"], \
                            "the parent's answers differ"
                    rows = []
                    for pair in range(args.pairs):
                        r = {"shape": shape, "ngroups": ng, "cap": cap, "rec_bytes": rec, "kpg": kpg, "pair": pair}
                        order = names[pair % len(names):] + names[:pair % len(names)]
                        for name in order:
                            w = old if name.startswith("p") else new
                            r[name] = w.ask(cmd="time", name=name, launches=args.launches, warmup=args.warmup)["us"]
                        rows.append(r)
                        out.write(json.dumps(r) + "\n")
                        out.flush()
                    rule = info["form_None"]["route"]
                    s = {"shape": shape, "ngroups": ng, "cap": cap, "rec_bytes": rec, "kpg": kpg, "logN": info["logN"],
                         "pairs": args.pairs, "launches": args.launches, "rule_route": "mfma" if rule else "direct",
                         "form_mfma": info["form_mfma"]}
                    for name in names:
                        v = [r[name] for r in rows]
                        s[name] = {"median": round(statistics.median(v), 2), "min": min(v), "max": max(v)}
                    for x, y in (("a", "b"), ("a", "p"), ("a_fold", "b_fold"), ("a_fold", "p_fold"),
                                 ("a_mfma_fold", "a_direct_fold"), ("a_mfma", "a_direct"), ("a_direct_fold", "p_fold")):
                        if y in names:
                            s["%s_beats_%s" % (x, y)] = sum(r[x] < r[y] for r in rows)
                    out.write(json.dumps({"summary": s}) + "\n")
                    out.flush()
                    print(json.dumps({"summary": s}), flush=True)
    finally:
        new.close()
        if old:
            old.close()


if __name__ == "__main__":
    main()
