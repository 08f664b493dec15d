"""Form-complete parity matrix of the tree kernel (k_evalfull) and the batched
Eval kernels.  k_evalfull is one source but about a hundred kernels at run
time: per-thread depth D, workgroup size, wave-uniform or per-lane keys,
leaves or nodes, raw key bytes or expanded records, correction words in LDS,
no / lane / quad shared walk, progress-feedback priority, zero or non-zero
prefix.  The launch plan (csrc/tree_plan.hpp, asked through
dpf.tree_form_for) says which form a call takes; this file asks it for every
call of a universe of small calls, keeps the cheapest call per distinct form,
and runs every one of them against the CPU oracle byte for byte, on the whole
device and on streams masked to 64, 16 and 4 CUs (which make the same choices
as a device of that size).  A failure names the form and the call.

Universe (the same as tests/c/tree_plan_test.cpp lists without a device):
nkeys 1..70, 96, 128, 130, 256, 300, 512, 513, 1024, 2048, 2056, 4096, 4100;
prefix_bits 0..12; leaf launches at logN 7..32; node launches to level 3..22
(at least 3 levels below the prefix).  A node launch to level L in 4..16 with
no prefix is the batched-Eval frontier of 2^(L+1) points per key; the others
are the byte-sliced back end's frontier pass at logN = level + 10."""
import functools

import numpy as np
import pytest

import dpf
from dpf import synth
import oracle

pytestmark = pytest.mark.gpu

NT = 16
GUARD = 256
FILL = 0x5A
# Largest output of a form's cheapest representative (bytes of leaves, or Eval
# result bytes): the plan needs 6 MiB (3 keys at logN 24 on 4 CUs).
CAP = 8 << 20
# Node passes below a prefix exist on the byte-sliced route only, which writes
# 128 bytes of leaves per node: the cheapest call of the deepest such form
# (d = 7, 512-thread one-key workgroups: 5 keys to level 17 below a 1-bit
# prefix on 4 CUs) needs 40 MiB, so that is their cap.
CAP_NODEPFX = 40 << 20
NKEYS = list(range(1, 71)) + [96, 128, 130, 256, 300, 512, 513, 1024, 2048, 2056, 4096, 4100]
MASKED = (64, 16, 4)
KEY_FIELDS = ("nodes", "d", "block", "uniform", "raw", "cw_lds", "walk", "feedback")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert dpf.gpu_init(1) >= 1


def _ncu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _cus_list():
    ncu = _ncu()
    return [ncu] + [c for c in MASKED if c < ncu]


def _form(nk, logN, pb, level, cus, _c=dpf.TreeFormC()):
    """The form key of a tree launch, or None where the plan refuses it."""
    if dpf.lib().dpf_tree_form_for(nk, logN, pb, level, cus, _c) != 0:
        return None
    return (_c.nodes, _c.d, _c.block, _c.uniform, _c.raw, _c.cw_lds, _c.walk, _c.feedback)


def _name(key, prefixed=None):
    s = " ".join("%s=%d" % kv for kv in zip(KEY_FIELDS, key))
    return s if prefixed is None else s + " prefixed=%d" % prefixed


@functools.lru_cache(maxsize=1)
def _universe():
    """{kind: {form: (cost, nkeys, logN, prefix_bits, level, cus)}}: the
    cheapest call of every form.  kind "leaf": form + whether a prefix is
    given; "node": the form of a node pass, whatever the prefix; "nodepfx":
    the forms of node passes below a prefix, again (they exist on the
    byte-sliced route only, at 128 bytes of leaves per node: CAP_NODEPFX)."""
    best = {"leaf": {}, "node": {}, "nodepfx": {}}

    def keep(kind, key, rep):
        cur = best[kind].get(key)
        if cur is None or rep[0] < cur[0]:
            best[kind][key] = rep

    for cus in _cus_list():
        for nk in NKEYS:
            for pb in range(13):
                for logN in range(7, 33):
                    stop = logN - 7
                    if stop < pb:
                        continue
                    key = _form(nk, logN, pb, 0, cus)
                    if key is not None:
                        keep("leaf", key + (int(pb != 0),), (nk * (16 << (stop - pb)), nk, logN, pb, 0, cus))
                for level in range(max(3, pb + 3), 23):
                    if pb == 0 and 4 <= level <= 16:      # the Eval frontier of 2^(level+1) points per key
                        logN, cost = level + 8, nk * (2 << level)
                    else:                                 # the byte-sliced back end's frontier pass
                        logN, cost = level + 10, nk * (16 << (level + 3 - pb))
                    key = _form(nk, logN, pb, level, cus)
                    if key is None:
                        continue
                    keep("node", key, (cost, nk, logN, pb, level, cus))
                    if pb:
                        keep("nodepfx", key, (cost, nk, logN, pb, level, cus))
    return best


class _Streams:
    """A plain stream for the device's own CU count, CU-masked ones below it."""

    def __init__(self):
        self.ncu = _ncu()
        self.made = {}

    def get(self, cus):
        if cus >= self.ncu:
            return None
        if cus not in self.made:
            self.made[cus] = dpf.stream_create_cu_masked(0, cus)
        return self.made[cus]

    def close(self):
        import torch
        torch.cuda.synchronize()
        for s in self.made.values():
            dpf.stream_destroy(s)


@pytest.fixture(scope="module")
def streams():
    s = _Streams()
    yield s
    s.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()


def _sync(stream):
    import torch
    if stream is None:
        torch.cuda.synchronize()
    else:
        stream.synchronize()


def _prefixes(pb):
    """No prefix; else a non-zero one: the last subtree, and one with mixed bits."""
    if pb == 0:
        return [0]
    return list(dict.fromkeys([(1 << pb) - 1, 0xAAAA & ((1 << pb) - 1)]))


def _subtree_want(keys, logN, pb, prefix):
    """uint8[nk][2^(logN - pb - 3)]: EvalFull of every key re-rooted at (pb, prefix)."""
    if pb == 0:
        return oracle.evalfull_batch(keys, logN, nthreads=NT)
    rk = np.stack([np.frombuffer(oracle.reroot_key(k.tobytes(), logN, pb, prefix), np.uint8) for k in keys])
    return oracle.evalfull_batch(rk, logN - pb, nthreads=NT)


def _run_subtree(keys, logN, pb, prefix, stream, expanded, what):
    """One share through dpf_evalfull_subtree_dev (or expand + expanded_dev)
    into a 0x5A-filled buffer with a guard behind it, against the oracle.
    Returns the mismatch as a line for the test's report, or None."""
    import torch
    nk, kl = keys.shape
    nbytes = nk * (16 << (logN - 7 - pb))
    d_keys = _dev(keys)
    d_work = torch.empty(dpf.pir_workspace_size(nk, logN, pb), dtype=torch.uint8, device="cuda")
    out = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if expanded:
        dpf.expand_keys_dev(d_keys, kl, nk, logN, d_work, stream=stream)
        dpf.evalfull_expanded_dev(d_work, nk, logN, out, pb, prefix, stream=stream)
    else:
        dpf.evalfull_subtree_dev(d_keys, kl, nk, logN, pb, prefix, out, d_work, stream=stream)
    _sync(stream)
    got = out.cpu().numpy()
    dpf.forget_workspace(d_work)
    assert (got[nbytes:] == FILL).all(), "bytes written past the output: " + what
    want = _subtree_want(keys, logN, pb, prefix).reshape(-1)
    if np.array_equal(got[:nbytes], want):
        return None
    bad = np.flatnonzero(got[:nbytes] != want)
    return "%s: %d of %d bytes differ from the oracle, first at %d" % (what, bad.size, nbytes, int(bad[0]))


def _report(failures):
    """Every call that differs, one line each, so a run names every form that broke."""
    assert not failures, "%d calls differ from the oracle:\n" % len(failures) + "\n".join(failures)


def _shares(nk, logN, first):
    al, s0, s1 = synth.key_seeds(nk, logN, first=first)
    return (al,) + tuple(dpf.gen_batch_seeded(al, logN, s0, s1))


def test_universe_leaves_no_form_out():
    """Every form the universe reaches on this device has a representative
    under its cap (8 MiB; 40 MiB for node passes below a prefix), so none is
    left out, and the forms that only narrow streams reach at small sizes
    are among them."""
    u = _universe()
    leaf, node, pfx = u["leaf"], u["node"], u["nodepfx"]
    print("reachable forms: %d leaf (%d without, %d with a prefix), %d node, %d node below a prefix (largest %d bytes)"
          % (len(leaf), sum(1 for k in leaf if not k[-1]), sum(1 for k in leaf if k[-1]), len(node), len(pfx),
             max(r[0] for r in pfx.values())))
    over = [(_name(k), r) for kind in (leaf, node) for k, r in kind.items() if r[0] > CAP]
    over += [(_name(k, 1), r) for k, r in pfx.items() if r[0] > CAP_NODEPFX]
    assert not over, over
    assert set(pfx) <= set(node)
    fb = [k for k in leaf if k[7]]
    assert {k[6] for k in fb} == {dpf.WALK_NONE, dpf.WALK_QUAD} and all(k[2] == 1024 and k[1] >= 6 for k in fb)
    assert {k[1] for k in leaf if k[2] == 1024 and not k[3]} == {6, 7}
    assert {k[1] for k in leaf} == set(range(8)) and {k[1] for k in node} == set(range(8))


@pytest.mark.parametrize("which", ["device"] + ["cus%d" % c for c in MASKED])
def test_leaf_forms_vs_oracle(which, streams):
    """Every leaf form whose cheapest call runs on this CU count: from key
    bytes (RAW where the plan says so), then from expanded records, each share
    its own call, every prefix class; output and guard checked."""
    cus = streams.ncu if which == "device" else int(which[3:])
    reps = sorted((k, r) for k, r in _universe()["leaf"].items() if r[5] == cus)
    if which != "device" and cus > streams.ncu:      # no such stream here: the universe held no such count
        assert not reps
        return
    launches, failures = 0, []
    for i, (key, (cost, nk, logN, pb, _, _)) in enumerate(reps):
        assert _form(nk, logN, pb, 0, cus) == key[:-1]
        _, ka, kb = _shares(nk, logN, first=1000 * logN + 17 * nk + pb)
        for share, keys in (("a", ka), ("b", kb)):
            for prefix in _prefixes(pb):
                for expanded in (False, True):
                    what = "leaf form [%s] %s: nkeys %d logN %d prefix (%d, %#x) cus %d share %s" % (
                        _name(key[:-1], key[-1]), "expanded records" if expanded else "key bytes", nk, logN, pb, prefix,
                        cus, share)
                    failures += filter(None, [_run_subtree(keys, logN, pb, prefix, streams.get(cus), expanded, what)])
                    launches += 1
    print("%s: %d leaf forms, %d launches" % (which, len(reps), launches))
    _report(failures)


def _frontier_points(al, logN, L, ppk, seed):
    """xs[nk][ppk]: node j of the 2^L frontier nodes in the top L bits of points
    2j and 2j+1 (and of every later one, round robin), pseudo-random low bits;
    the key's alpha and the two ends of the domain among them, each in the
    place of a point of its own node."""
    nk = len(al)
    low = logN - L
    rng = np.random.default_rng(seed)
    node = (np.arange(ppk, dtype=np.uint64) >> np.uint64(1)) % np.uint64(1 << L)
    xs = (node[None, :] << np.uint64(low)) | rng.integers(0, 1 << low, size=(nk, ppk), dtype=np.uint64)
    xs[:, 0] = 0
    xs[:, 2 * ((1 << L) - 1)] = (1 << logN) - 1
    for k in range(nk):
        xs[k, 2 * (int(al[k]) >> low) + 1] = al[k]
    assert ((xs >> np.uint64(low)) == node[None, :]).all() and set(node.tolist()) == set(range(1 << L))
    return xs


@pytest.mark.parametrize("kinds", ["node", "nodepfx"])
def test_node_forms_vs_oracle(kinds, streams):
    """Every node form ("node"), and every node form below a prefix again
    ("nodepfx").  Without a prefix and to a level the Eval frontier takes:
    dpf_eval_batch_dev with the full workspace, every frontier node the start
    of a query, so every node the pass writes is checked through the oracle's
    Eval.  The others: the byte-sliced back end's frontier pass
    (dpf_evalfull_subtree_dev), whose every node feeds leaves."""
    import torch
    u = _universe()
    reps = [(kinds, k, r) for k, r in sorted(u[kinds].items())]
    prev = dpf.get_aes_impl()
    launches, failures = 0, []
    try:
        for kind, key, (cost, nk, logN, pb, level, cus) in reps:
            stream = streams.get(cus)
            what = "%s form [%s]: nkeys %d logN %d level %d prefix_bits %d cus %d" % (kind, _name(key), nk, logN, level,
                                                                                    pb, cus)
            assert _form(nk, logN, pb, level, cus) == key, what
            al, ka, kb = _shares(nk, logN, first=500 * level + 13 * nk + pb)
            if pb == 0 and 4 <= level <= 16:
                ppk = 2 << level
                ws = dpf.eval_workspace_size(nk, ppk, logN)
                e = dpf.eval_form_for(nk, ppk, logN, ws, True, cus)
                assert e.level == level and e.nodes is not None, what
                assert tuple(int(getattr(e.nodes, f)) for f in KEY_FIELDS) == key, what
                xs = _frontier_points(al, logN, level, ppk, seed=level * 1000 + nk)
                d_xs = torch.from_numpy(xs.reshape(-1).view(np.int64)).cuda()
                assert d_xs.data_ptr() % 16 == 0
                for share, keys in (("a", ka), ("b", kb)):
                    d_work = torch.empty(ws, dtype=torch.uint8, device="cuda")
                    out = torch.full((nk * ppk + GUARD,), FILL, dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    dpf.eval_batch_dev(_dev(keys), keys.shape[1], nk, d_xs, ppk, logN, out, d_work, stream=stream)
                    _sync(stream)
                    got = out.cpu().numpy()
                    assert (got[nk * ppk:] == FILL).all(), "bytes written past the output: " + what
                    want = oracle.eval_batch(keys, xs, logN, nthreads=NT).reshape(-1)
                    bad = np.flatnonzero(got[:nk * ppk] != want)
                    if bad.size:
                        failures.append("%s share %s: %d of %d Eval results differ, first at query %d" % (
                            what, share, bad.size, nk * ppk, int(bad[0])))
                    launches += 1
            else:
                # stop - 3 = level: the byte-sliced kernel's shallower depth, taken below 2^17 lanes of depth 4
                assert logN - 10 == level and (nk << max(level - pb - 4, 0)) < 131072, what
                dpf.set_aes_impl("bitsliced")
                try:
                    for share, keys in (("a", ka), ("b", kb)):
                        for prefix in _prefixes(pb):
                            failures += filter(None, [_run_subtree(
                                keys, logN, pb, prefix, stream, False,
                                what + " prefix %#x share %s (byte-sliced leaves)" % (prefix, share))])
                            launches += 1
                finally:
                    dpf.set_aes_impl(prev)
    finally:
        dpf.set_aes_impl(prev)
    print("%s: %d forms, %d launches" % (kinds, len(reps), launches))
    _report(failures)


EVAL_KERNELS = {dpf.EVAL_PERSIST: "k_eval_persist", dpf.EVAL_PAIR_UNIFORM: "k_eval2<uniform>", dpf.EVAL_PAIR: "k_eval2"}


def test_eval_forms_vs_oracle():
    """One call for every (kernel, frontier or root walks, key records staged
    in LDS or read by scalar loads, 16-byte-aligned or 8-byte-offset points,
    ragged last workgroup) combination the plan reports over logN 9, 13, 20,
    21, 22, 32 and small key and point counts, against the oracle's Eval."""
    import torch
    best = {}
    for logN in (9, 13, 20, 21, 22, 32):
        for nk in (1, 2, 3, 5, 8, 17, 33, 70):
            for ppk in (1, 7, 33, 96, 128, 256, 257, 384, 1024):
                if nk * ppk > 1 << 17:
                    continue
                for full in (True, False):
                    ws = dpf.eval_workspace_size(nk, ppk, logN) if full else nk * (logN - 7 + 2) * 32
                    for aligned in (True, False):
                        e = dpf.eval_form_for(nk, ppk, logN, ws, aligned)
                        key = (e.kernel, e.level > 0, e.cw_staged, aligned, e.ragged)
                        if key not in best or nk * ppk < best[key][0]:
                            best[key] = (nk * ppk, nk, ppk, logN, ws)
    kernels = {k[0] for k in best}
    assert kernels == set(EVAL_KERNELS), kernels
    assert {k[2] for k in best if k[0] == dpf.EVAL_PERSIST} == {True, False}
    assert {k[1] for k in best if k[0] != dpf.EVAL_PERSIST} == {True, False}
    assert {k[4] for k in best} == {True, False} and {k[3] for k in best if k[0] != dpf.EVAL_PERSIST} == {True, False}
    failures = []
    for key, (nq, nk, ppk, logN, ws) in sorted(best.items()):
        what = "Eval form [%s frontier=%d staged=%d aligned=%d ragged=%d]: nkeys %d ppk %d logN %d workspace %d" % (
            (EVAL_KERNELS[key[0]],) + tuple(int(x) for x in key[1:]) + (nk, ppk, logN, ws))
        al, ka, kb = _shares(nk, logN, first=77 * logN + nk + ppk)
        xs = synth.eval_points(nk, ppk, logN, master=logN * ppk + nk)
        xs[:, 0] = al
        if ppk > 2:
            xs[:, 1] = 0
            xs[:, 2] = (1 << logN) - 1
        d_big = torch.zeros(nq + 2, dtype=torch.int64, device="cuda")
        off = 0 if key[3] else 1
        if d_big.data_ptr() % 16:
            off ^= 1
        d_xs = d_big[off:off + nq]
        d_xs.copy_(torch.from_numpy(xs.reshape(-1).view(np.int64)))
        assert (d_xs.data_ptr() % 16 == 0) == key[3], what
        for share, keys in (("a", ka), ("b", kb)):
            d_work = torch.empty(ws, dtype=torch.uint8, device="cuda")
            out = torch.full((nq + GUARD,), FILL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            dpf.eval_batch_dev(_dev(keys), keys.shape[1], nk, d_xs, ppk, logN, out, d_work)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert (got[nq:] == FILL).all(), "bytes written past the output: " + what
            want = oracle.eval_batch(keys, xs, logN, nthreads=NT).reshape(-1)
            bad = np.flatnonzero(got[:nq] != want)
            if bad.size:
                failures.append("%s share %s: %d of %d results differ, first at query %d" % (what, share, bad.size, nq,
                                                                                           int(bad[0])))
    print("%d Eval forms" % len(best))
    _report(failures)
