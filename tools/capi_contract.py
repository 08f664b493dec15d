#!/usr/bin/env python3
"""The argument contract of the C ABI, as data: which return code and which
dpf_last_error text every device-resident entry point, every dpf_pir_db_create*
form and every size function gives for a matrix of good and bad arguments.

    DPF_LIB=<library of the commit to record> tools/capi_contract.py --record tests/golden/capi_contract.json
    tools/capi_contract.py --check tests/golden/capi_contract.json

Both run where no GPU is visible (--check refuses to make a single call unless
dpf_gpu_init(0) is DPF_ERR_NODEV): the device pointers are fake addresses, and
a case that got as far as a device call (DPF_ERR_HIP, DPF_ERR_NODEV) is not
recorded, so the fixture holds exactly the calls that are decided before one.
tests/test_capi_contract_cpu.py replays it; record it from the commit a
refactor starts from, never from the refactored library.

A case is [arguments, code] or [arguments, code, index into "messages"] (the
text only where the code is nonzero: after a success it is stale).  Arguments
are integers and nulls, and the tokens of BUFFERS for the few real host
buffers the create calls read."""
import argparse
import ctypes
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dpf-go_amd"))
import dpf  # noqa: E402

ERR_NODEV, ERR_HIP = dpf.DPF_ERR_NODEV, dpf.DPF_ERR_HIP
P = 1 << 12                      # fake device addresses: P * (1 + position), 4 KiB aligned, never dereferenced
LOGN, STOP, PB = 20, 13, 2
KMIN = 17 + 18 * STOP
KLEN = 33 + 18 * STOP
MAXREC = 32768
REC_BYTES = (0, 4, 6, 20, 32, 48, 64, MAXREC, MAXREC + 4, MAXREC + 32)

# Real host memory behind the tokens: two points inside 2^20 and one outside, a
# 64-byte DB (never read: no call here gets as far as an upload).
BUFFERS = {"@pts": [5, 1 << 18], "@pts_out": [5, 1 << 30], "@db": 64, "@handle": None, "@form": None}


def load():
    L = ctypes.CDLL(dpf.LIB_PATH)
    for name, (res, args) in dpf.SIGNATURES.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


class Caller:
    def __init__(self, L):
        self.L = L
        self.keep = [(ctypes.c_uint64 * 2)(*BUFFERS["@pts"]), (ctypes.c_uint64 * 2)(*BUFFERS["@pts_out"]),
                     (ctypes.c_uint8 * BUFFERS["@db"])()]
        self.tok = {"@pts": ctypes.cast(self.keep[0], ctypes.POINTER(ctypes.c_uint64)),
                    "@pts_out": ctypes.cast(self.keep[1], ctypes.POINTER(ctypes.c_uint64)),
                    "@db": ctypes.cast(self.keep[2], ctypes.POINTER(ctypes.c_uint8))}

    def __call__(self, fn, args):
        """-> [code] | [code, text]; a create call's code is -100 if it left *handle non-null."""
        handle = ctypes.c_void_p(1)
        self.tok["@handle"], self.tok["@form"] = ctypes.byref(handle), ctypes.byref(dpf.EvalFormC())
        real = [self.tok[a] if isinstance(a, str) else a for a in args]
        rc = getattr(self.L, fn)(*real)
        if dpf.SIGNATURES[fn][0] is not ctypes.c_int:
            return [int(rc)]                       # a size function: its value
        if "@handle" in args and handle.value is not None:
            return [-100, "handle not cleared"]
        return [rc] if rc == 0 else [rc, self.L.dpf_last_error().decode()]


# ---- the matrix ------------------------------------------------------------
# An entry point is a list of (name, kind, valid value); the kind picks the
# single mutations.  Pointers get distinct fake addresses by position.
def ptr(name):
    return (name, "ptr", None)


KEYS = [("klen", "klen", KLEN), ("nkeys", "nkeys", 2), ("logN", "logN", LOGN)]
SUB = [("pb", "pb", PB), ("prefix", "prefix", 1)]
DEV, STREAM = ("device", "fixed", 0), ("stream", "fixed", None)
REC = ("rec", "rec", 32)
STRIDE = ("stride", "stride", 48)


def nrec(limit):
    return ("nrec", "nrec", (300, limit))


SLICE = 1 << (LOGN - PB)          # records of the subtree (PB, prefix)


def answer(rec, db="d_db"):
    return [DEV, ptr("d_keys")] + KEYS + SUB + [ptr(db), nrec(SLICE)] + ([REC] if rec else []) + \
           [ptr("d_ans"), ptr("d_work"), STREAM]


def write():
    return [DEV, ptr("d_keys")] + KEYS + SUB + [ptr("d_msgs"), ptr("d_db"), nrec(SLICE), REC, ptr("d_work"), STREAM]


def fold(rec):
    return [DEV, ptr("d_bits"), STRIDE, ("nkeys", "nkeys", 2), ptr("d_db"), nrec(48 * 8)] + ([REC] if rec else []) + \
           [ptr("d_ans"), ptr("d_work"), STREAM]


def scatter():
    return [DEV, ptr("d_bits"), STRIDE, ("nkeys", "nkeys", 2), ptr("d_msgs"), ptr("d_db"), nrec(48 * 8), REC, STREAM]


def slice_(rec):
    return [DEV, ptr("d_db"), nrec(None)] + ([REC] if rec else []) + [ptr("d_dbs"), STREAM]


def update():
    return [DEV, ptr("d_dbs"), nrec(None), REC, ptr("d_idx"), ptr("d_recs"), ("n", "count", 3), STREAM]


def gather():
    return [DEV, ptr("d_dbs"), nrec(None), REC, ptr("d_idx"), ("n", "count", 3), ptr("d_out"), STREAM]


def create(sparse, rec):
    return ([("points", "hostpts", "@pts")] if sparse else []) + \
           [("db", "hostptr", "@db"), ("nrec", "nrec", (2, None if sparse else 1 << LOGN))] + ([REC] if rec else []) + \
           [("logN", "logN", LOGN), ("ngpus", "count", 1), ("handle", "hostptr", "@handle")]


ENTRIES = {
    "dpf_evalfull_batch_dev": [DEV, ptr("d_keys")] + KEYS + [ptr("d_out"), ptr("d_work"), STREAM],
    "dpf_evalfull_subtree_dev": [DEV, ptr("d_keys")] + KEYS + SUB + [ptr("d_out"), ptr("d_work"), STREAM],
    "dpf_eval_batch_dev": [DEV, ptr("d_keys")] + KEYS[:2] + [ptr("d_xs"), ("ppk", "count", 5), KEYS[2], ptr("d_out"),
                                                             ptr("d_work"), ("work_bytes", "wb", 1 << 20), STREAM],
    "dpf_eval_bits_dev": [DEV, ptr("d_keys")] + KEYS[:2] + [ptr("d_xs"), ("npts", "nrec", (300, 48 * 8)), KEYS[2],
                                                            ptr("d_bits"), STRIDE, ptr("d_work"),
                                                            ("work_bytes", "wb", 1 << 20), STREAM],
    "dpf_expand_keys_dev": [DEV, ptr("d_keys")] + KEYS + [ptr("d_work"), STREAM],
    "dpf_evalfull_expanded_dev": [DEV, ptr("d_work"), KEYS[1], KEYS[2]] + SUB + [ptr("d_out"), STREAM],
    "dpf_aes_mmo_dev": [DEV, ("impl", "enum3", 0), ("right", "fixed", 1), ptr("d_in"), ptr("d_out"),
                        ("nblocks", "blocks", 8), ("reps", "fixed", 1), STREAM],
    "dpf_pir_answer_dev": answer(False),
    "dpf_pir_answer_sliced_dev": answer(False, "d_dbs"),
    "dpf_pir_answer_wide_dev": answer(True),
    "dpf_pir_answer_sliced_wide_dev": answer(True, "d_dbs"),
    "dpf_pir_answer_sliced_any_dev": answer(True, "d_dbs"),
    "dpf_xor_fold_dev": fold(True),
    "dpf_xor_fold_sliced_dev": fold(False),
    "dpf_xor_fold_sliced_wide_dev": fold(True),
    "dpf_xor_fold_sliced_any_dev": fold(True),
    "dpf_pir_db_slice_dev": slice_(False),
    "dpf_pir_db_slice_wide_dev": slice_(True),
    "dpf_pir_db_slice_any_dev": slice_(True),
    "dpf_pir_db_update_sliced_wide_dev": update(),
    "dpf_pir_db_update_sliced_any_dev": update(),
    "dpf_pir_db_gather_sliced_wide_dev": gather(),
    "dpf_pir_db_gather_sliced_any_dev": gather(),
    "dpf_xor_scatter_dev": scatter(),
    "dpf_xor_scatter_sliced_wide_dev": scatter(),
    "dpf_xor_scatter_sliced_any_dev": scatter(),
    "dpf_pir_write_wide_dev": write(),
    "dpf_pir_write_sliced_wide_dev": write(),
    "dpf_pir_write_sliced_any_dev": write(),
    "dpf_pir_answer_sparse_dev": [DEV, ptr("d_keys")] + KEYS + [ptr("d_points"), ptr("d_dbs"), nrec(None), REC,
                                                                ptr("d_ans"), ptr("d_work"), STREAM],
    "dpf_pir_write_sparse_dev": [DEV, ptr("d_keys")] + KEYS + [ptr("d_points"), ptr("d_msgs"), ptr("d_dbs"),
                                                               nrec(None), REC, ptr("d_work"), STREAM],
    "dpf_pir_db_create": create(False, False),
    "dpf_pir_db_create_wide": create(False, True),
    "dpf_pir_db_create_any": create(False, True),
    "dpf_pir_db_create_sparse": create(True, True),
}


def mutations(spec, i, key_len_of):
    """The single mutations of parameter i: a list of {position: value}."""
    name, kind, valid = spec[i]
    pos = {n: j for j, (n, _, _) in enumerate(spec)}
    one = lambda vals: [{i: v} for v in vals]
    if kind == "ptr":
        base = P * (1 + i)
        return one([None, base + 2, base + 4, base + 8])
    if kind == "hostptr":
        return one([None])
    if kind == "hostpts":
        return one([None, "@pts_out"])
    if kind == "rec":
        return one(REC_BYTES)
    if kind == "stride":
        return one([0, 8, 16, 24])
    if kind == "nrec":
        lim = valid[1]
        return one([0, 1] if lim is None else [0, lim, lim + 1])
    if kind == "pb":
        return one([0, STOP, STOP + 1]) + [{i: STOP, pos["prefix"]: (1 << STOP) - 1}]
    if kind == "prefix":
        return one([0, (1 << PB) - 1, 1 << PB])
    if kind == "klen":
        return one([KMIN - 1, KMIN, KLEN])
    if kind == "logN":
        out = one([0, 7, 20, 63, 64])
        if "klen" in pos:                      # ... and with a key of that logN's length
            out += [{i: v, pos["klen"]: key_len_of(v)} for v in (0, 7, 63, 64)]
        return out
    if kind == "nkeys":
        return one([0, 2])
    if kind == "count":
        return one([0, 2])
    if kind == "wb":
        return one([0, 2 * (STOP + 2) * 32 - 1, 2 * (STOP + 2) * 32, 1 << 12])
    if kind == "enum3":
        return one([0, 1, 2])
    if kind == "blocks":
        return one([0, 7, 16])
    return []


def entry_cases(fn, spec, key_len_of):
    base = [P * (1 + i) if k == "ptr" else (v[0] if k == "nrec" else v) for i, (_, k, v) in enumerate(spec)]
    singles = {i: mutations(spec, i, key_len_of) for i in range(len(spec))}
    muts = [{}] + [m for i in singles for m in singles[i]]
    ptrs = [i for i, (_, k, _) in enumerate(spec) if k in ("ptr", "hostptr", "hostpts")]
    # Pairs, so that the order of the reports is pinned: a null with a
    # misaligned pointer, a bad width with a short key, and each of a bad
    # width / stride / record count / short key with a null or misaligned one.
    for a, b in itertools.permutations(ptrs, 2):
        if spec[b][1] == "ptr":
            muts += [{a: None, b: P * (1 + b) + off} for off in (2, 8)]
    kinds = {k: i for i, (_, k, _) in enumerate(spec)}
    bad = []
    if "rec" in kinds:
        bad += [{kinds["rec"]: 6}, {kinds["rec"]: MAXREC + 32}]
    if "klen" in kinds:
        bad += [{kinds["klen"]: KMIN - 1}]
    if "stride" in kinds:
        bad += [{kinds["stride"]: 8}, {kinds["stride"]: 64, kinds["nrec"]: 64 * 8 + 1}]
    if "pb" in kinds:
        bad += [{kinds["pb"]: STOP + 1}] + ([{kinds["nrec"]: SLICE + 1}] if "nrec" in kinds else [])
    if "logN" in kinds:
        bad += [{kinds["logN"]: 64}]
    for x, y in itertools.combinations(bad, 2):
        if not set(x) & set(y):
            muts.append({**x, **y})
    for x in bad:
        for p_ in ptrs:
            muts.append({**x, p_: None})
            if spec[p_][1] == "ptr":
                muts.append({**x, p_: P * (1 + p_) + 4})
    for z in ("nkeys", "nrec"):                 # nothing to do: which checks still hold
        if z in kinds:
            for x in bad:
                if kinds[z] not in x:
                    muts.append({**x, kinds[z]: 0})
            for p_ in ptrs:
                if spec[p_][1] == "ptr":
                    muts += [{kinds[z]: 0, p_: None}, {kinds[z]: 0, p_: P * (1 + p_) + 2}]
    seen, out = set(), []
    for m in muts:
        args = list(base)
        for i, v in m.items():
            args[i] = v
        if "@pts_out" in args or "@pts" in args:
            assert args[kinds["nrec"]] <= 2    # the point scan reads nrec real points: never past the buffer
        key = json.dumps(args)
        if key not in seen:
            seen.add(key)
            out.append(args)
    return out


NK, LOGNS, NPTS = (0, 1, 3, 64, 65), (0, 7, 13, 20, 40, 63, 70), (0, 1, 128, 129, 300, (1 << 20) + 1)


def size_cases():
    stop_of = lambda n: max(n - 7, 0)
    g = {
        "dpf_key_len": [[n] for n in LOGNS],
        "dpf_evalfull_len": [[n] for n in LOGNS],
        "dpf_workspace_size": [[k, n] for k in NK for n in LOGNS],
        "dpf_eval_workspace_size": [[k, p, n] for k in NK for p in NPTS for n in LOGNS],
        "dpf_eval_frontier_level": [[n, p] for n in LOGNS for p in NPTS],
        "dpf_eval_bits_stride": [[p] for p in NPTS],
        "dpf_eval_bits_workspace_size": [[k, p, n] for k in NK for p in NPTS for n in LOGNS],
        "dpf_pir_sparse_workspace_size": [[k, p, n] for k in NK for p in NPTS for n in LOGNS],
        "dpf_xor_fold_workspace_size": [[]],
        "dpf_pir_workspace_size": [[k, n, pb] for k in NK for n in LOGNS
                                   for pb in sorted({0, 2, stop_of(n), stop_of(n) + 1})],
        "dpf_pir_db_sliced_size": [[p] for p in NPTS],
        "dpf_pir_db_sliced_size_wide": [[p, r] for p in NPTS for r in REC_BYTES],
        "dpf_pir_db_sliced_size_any": [[p, r] for p in NPTS for r in REC_BYTES],
    }
    # The Eval form query shares dpf_eval_batch_dev's workspace rule (code and text only).
    g["dpf_eval_form_for"] = [[k, p, n, wb, 1, 256, f] for k in (0, 2) for p in (0, 5) for n in (20, 4097)
                              for wb in (0, 959, 960, 4096, 1 << 20) for f in ("@form", None)]
    return g


def all_cases(L):
    cases = {fn: entry_cases(fn, spec, lambda n: int(L.dpf_key_len(n))) for fn, spec in ENTRIES.items()}
    cases.update(size_cases())
    return cases


def guard(L):
    rc = L.dpf_gpu_init(0)
    if rc != ERR_NODEV:
        sys.exit(f"capi_contract: a GPU is visible (dpf_gpu_init(0) = {rc}); no call made")


def record(path):
    L = load()
    guard(L)
    call = Caller(L)
    messages, out, dropped = [], {}, 0
    for fn, argsets in all_cases(L).items():
        rows = []
        for args in argsets:
            r = call(fn, args)
            if dpf.SIGNATURES[fn][0] is ctypes.c_int and r[0] in (ERR_NODEV, ERR_HIP):
                dropped += 1
                continue
            if len(r) == 2:
                if r[1] not in messages:
                    messages.append(r[1])
                r = [r[0], messages.index(r[1])]
            rows.append([args] + r)
        out[fn] = rows
    with open(path, "w") as f:
        f.write('{"messages": ' + json.dumps(messages, indent=1) + ',\n"buffers": ' + json.dumps(BUFFERS) +
                ',\n"cases": {\n')
        f.write(",\n".join(json.dumps(fn) + ": [\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) +
                           "]" for fn, rows in out.items()))
        f.write("}}\n")
    n = sum(len(r) for r in out.values())
    print(f"recorded {n} cases of {len(out)} functions ({dropped} reached a device call: dropped) -> {path}")


def check(path):
    L = load()
    guard(L)
    fx = json.load(open(path))
    assert fx["buffers"] == BUFFERS, "the fixture was recorded with other host buffers"
    call = Caller(L)
    n, bad = 0, []
    for fn, rows in fx["cases"].items():
        for row in rows:
            args, want = row[0], row[1:]
            if len(want) == 2:
                want = [want[0], fx["messages"][want[1]]]
            got = call(fn, args)
            n += 1
            if got != want:
                bad.append(f"{fn}{tuple(args)}: got {got}, recorded {want}")
    for b in bad[:40]:
        print(b)
    print(f"{n} cases, {len(bad)} mismatches")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--record", metavar="JSON")
    ap.add_argument("--check", metavar="JSON")
    a = ap.parse_args()
    if a.record:
        record(a.record)
    if a.check:
        sys.exit(check(a.check))
