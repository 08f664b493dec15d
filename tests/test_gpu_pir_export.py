"""The whole-DB read-out of a resident PIR DB: dpf_pir_db_unslice_any_dev and
_unslice_grouped_dev (the inverse of slicing), dpf_pir_db_xor_sliced_dev (the
merge of two sliced buffers) and the handle's export / xor_records / clear on
dense, sparse and grouped handles.  Expected values are numpy restatements of
the layout's definition (tests/pir_ref.py) and CPU-oracle selections over the
row-major DB; never the code under test.

The two-shard and the row-major (DPF_PIR_FOLD=lds) handles need a process of
their own (the device registry and the fold choice are process-wide): the
tests at the end run this file as a script."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "dpf-go_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import dpf                  # noqa: E402
from dpf import synth       # noqa: E402
import oracle               # noqa: E402
import pir_ref as ref       # noqa: E402

pytestmark = pytest.mark.gpu
POISON, GUARD = 0xAB, 64


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert dpf.gpu_init(1) >= 1


def _rand(tag, *shape):
    return np.random.default_rng([tag, *shape]).integers(0, 256, shape, dtype=np.uint8)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()


def _out(nbytes):
    import torch
    return torch.full((nbytes + GUARD,), POISON, dtype=torch.uint8, device="cuda")


def _check_out(d_out, want):
    got = d_out.cpu().numpy()
    want = np.ascontiguousarray(want).reshape(-1)
    assert np.array_equal(got[:want.size], want)
    assert (got[want.size:] == POISON).all(), "bytes past the output"


# ---- the device entries -----------------------------------------------------------------
# One tile, an odd tile count, a short last column after a full one, several
# columns, a short last super-group; the last two: rows that are no multiple of
# 16 bytes in a full group of 4 columns (32 tiles, then 1) and in 3 columns.
UNSLICE_SHAPES = [(1, 160), (255, 4), (256, 32), (257, 36), (300, 12), (300, 32), (300, 64), (513, 20), (1000, 96),
                  (1000, 100), (777, 1024), (300, 132), (300, 68)]


@pytest.mark.parametrize("nrec,rec", UNSLICE_SHAPES)
def test_unslice_returns_the_rows_and_nothing_else(nrec, rec):
    """The input is the layout of random records over all 256 * nsg rows, so
    the rows past nrec are garbage; exactly the first nrec rows come back and
    the bytes behind them stay as they were."""
    import torch
    nsg = (nrec + 255) // 256
    rows = _rand(1, 256 * nsg, rec)
    d_dbs = _dev(ref.layout(rows))
    assert d_dbs.numel() == dpf.pir_db_sliced_size_any(nrec, rec)
    d_db = _out(nrec * rec)
    dpf.pir_db_unslice_any_dev(d_dbs, nrec, rec, d_db)
    torch.cuda.synchronize()
    _check_out(d_db, rows[:nrec])


@pytest.mark.parametrize("rec", [32, 20])
def test_slice_then_unslice_is_the_identity(rec):
    import torch
    nrec = 3000
    db = _rand(2, nrec, rec)
    d_dbs = torch.full((dpf.pir_db_sliced_size_any(nrec, rec),), 0x5A, dtype=torch.uint8, device="cuda")
    dpf.pir_db_slice_any_dev(_dev(db), nrec, rec, d_dbs)
    d_db = _out(nrec * rec)
    dpf.pir_db_unslice_any_dev(d_dbs, nrec, rec, d_db)
    torch.cuda.synchronize()
    _check_out(d_db, db)
    # A range of whole super-groups: both pointers offset by 2 of them.
    off = 2 * 256 * rec
    d_part = _out((nrec - 512) * rec)
    dpf.pir_db_unslice_any_dev(d_dbs[off:], nrec - 512, rec, d_part)
    torch.cuda.synchronize()
    _check_out(d_part, db[512:])
    d_db.fill_(POISON)
    dpf.pir_db_unslice_any_dev(d_dbs[off:], 300, rec, d_db[off:])          # ... and a short run inside the output
    torch.cuda.synchronize()
    got = d_db.cpu().numpy()
    assert (got[:off] == POISON).all() and (got[off + 300 * rec:] == POISON).all()
    assert np.array_equal(got[off:off + 300 * rec].reshape(300, rec), db[512:812])


@pytest.mark.parametrize("ng,nrec,rec", [(3, 300, 20), (5, 256, 32), (2, 1, 64), (4, 700, 36)])
def test_unslice_grouped(ng, nrec, rec):
    import torch
    db = _rand(3, ng, nrec, rec)
    flat = ref.grouped_flat(db)
    gs = flat.shape[0] // ng
    flat = flat.reshape(ng, gs, rec).copy()
    flat[:, nrec:] = _rand(4, ng, gs - nrec, rec)                 # garbage behind every group: not delivered
    d_dbs = _dev(ref.layout(flat.reshape(ng * gs, rec)))
    assert d_dbs.numel() == dpf.pir_db_grouped_size(ng, nrec, rec)
    d_db = _out(ng * nrec * rec)
    dpf.pir_db_unslice_grouped_dev(d_dbs, ng, nrec, rec, d_db)
    torch.cuda.synchronize()
    _check_out(d_db, db)


def test_xor_sliced():
    import torch
    nrec, rec = 1000, 96
    a, b = _rand(5, nrec, rec), _rand(6, nrec, rec)
    la, lb = ref.layout(a), ref.layout(b)
    d_a = _out(la.size)
    d_a[:la.size].copy_(torch.from_numpy(la))
    d_b = _dev(lb)
    dpf.pir_db_xor_sliced_dev(d_a, d_b, la.size)
    torch.cuda.synchronize()
    _check_out(d_a, ref.layout(a ^ b))
    assert np.array_equal(d_b.cpu().numpy(), lb)
    dpf.pir_db_xor_sliced_dev(d_a, d_b, 0)                          # nothing to do
    torch.cuda.synchronize()
    _check_out(d_a, ref.layout(a ^ b))


# ---- the handle ---------------------------------------------------------------------------
# A kind of handle over a flat DB [N][rec] in the caller's index space: how it
# is made, a batch of key pairs, the records each key selects (from the CPU
# oracle) and the private write that takes them.
class Kind:
    def __init__(self, name, logN, N, rec, nk, groups=None, points=False, ngpus=1):
        self.name, self.logN, self.N, self.rec, self.nk, self.groups, self.ngpus = name, logN, N, rec, nk, groups, ngpus
        self.pts = None
        per = N // groups if groups else N
        al, s0, s1 = synth.key_seeds(nk, logN, first=300 + N + rec)
        if points:
            self.pts = np.random.default_rng([7, N]).integers(0, 1 << logN, N, dtype=np.uint64)
            al = self.pts[np.random.default_rng([8, N]).integers(0, N, nk)]     # every key hits a record
        else:
            al = al % np.uint64(per)
        self.alphas = al
        self.ka, self.kb = dpf.gen_batch_seeded(al, logN, s0, s1)

    def make(self, db):
        return dpf.PirDB(db, self.logN, ngpus=self.ngpus, rec_bytes=self.rec, points=self.pts, groups=self.groups)

    @functools.lru_cache(maxsize=None)
    def sel(self, share):
        """bool [nk][N]: the records of the caller's index space that each key of a share selects."""
        keys = (self.ka, self.kb)[share]
        if self.pts is not None:
            return oracle.eval_batch(keys, np.tile(self.pts, (self.nk, 1)), self.logN, nthreads=8).astype(bool)
        per = self.N // self.groups if self.groups else self.N
        rows = ref.sel_bool(oracle.evalfull_batch(keys, self.logN, nthreads=8), per)
        if not self.groups:
            return rows
        kpg = self.nk // self.groups
        out = np.zeros((self.nk, self.N), bool)
        for r in range(self.nk):
            out[r, (r // kpg) * per:(r // kpg + 1) * per] = rows[r]
        return out

    def hit(self):
        """bool [nk][N]: what the two shares select together, the records at each key's alpha."""
        return self.sel(0) ^ self.sel(1)

    def write(self, pdb, share, msgs):
        (pdb.write_grouped if self.groups else pdb.write)((self.ka, self.kb)[share], msgs)


def _answers(db, sel):
    out = np.zeros((sel.shape[0], db.shape[1]), np.uint8)
    for k in range(sel.shape[0]):
        if sel[k].any():
            out[k] = np.bitwise_xor.reduce(db[sel[k]], axis=0)
    return out


def _written(db, sel, msgs):
    par = (sel.T.astype(np.float64) @ np.unpackbits(msgs, axis=1, bitorder="little").astype(np.float64)).astype(np.int64) & 1
    return db ^ np.packbits(par.astype(np.uint8), axis=1, bitorder="little")


def _ranges(N):
    return [(0, 1), (255, 2), (256, 256), (257, 1000), (N - 1, 1), (0, 0), (N, 0)]


def _handle_checks(kind, boundary=None):
    """export of the whole DB and of ranges; after a private write under each
    share on a server of its own the two exports XOR to the messages at the
    alphas; xor_records over an unaligned range, then export and answer;
    clear, then the whole DB XORed back in; refused ranges change nothing.
    boundary: a caller index with records of two shards on its sides."""
    N, rec, nk = kind.N, kind.rec, kind.nk
    dbA, dbB = _rand(20, N, rec), _rand(21, N, rec)
    msgs = _rand(22, nk, rec)
    a, b = kind.make(dbA), kind.make(dbB)
    assert a.nrec == N
    assert np.array_equal(a.export(), dbA)
    ranges = _ranges(N) + ([(boundary - 1, 2), (boundary - 300, 600), (boundary, 1)] if boundary else [])
    for first, n in ranges:
        n = min(n, N - first)
        got = a.export(first, n)
        assert got.shape == (n, rec) and np.array_equal(got, dbA[first:first + n]), (first, n)
    assert np.array_equal(a.export(300), dbA[300:])
    # Private writes, one share per server.
    kind.write(a, 0, msgs)
    kind.write(b, 1, msgs)
    wantA = _written(dbA, kind.sel(0), msgs)
    assert np.array_equal(a.export(), wantA)
    assert np.array_equal(b.export(), _written(dbB, kind.sel(1), msgs))
    both = _written(dbA ^ dbB, kind.hit(), msgs)
    assert kind.hit().sum(axis=1).min() >= 1 and not np.array_equal(both, dbA ^ dbB)
    assert np.array_equal(a.export() ^ b.export(), both)
    # The other server's share merged in: an unaligned range first, then the rest.
    lo, hi = (boundary - 259, boundary + 300) if boundary else (257, min(N, 257 + 1000))
    other = b.export()
    a.xor_records(other[lo:hi], first=lo)
    want = wantA.copy()
    want[lo:hi] ^= other[lo:hi]
    assert np.array_equal(a.export(), want)
    assert np.array_equal(a.answer(kind.ka), _answers(want, kind.sel(0)))
    a.xor_records(other[:lo])
    a.xor_records(other[hi:], first=hi)
    a.xor_records(other[:0], first=N)                               # nothing to do
    assert np.array_equal(a.export(), both)
    assert np.array_equal(a.answer(kind.ka) ^ a.answer(kind.kb), _answers(both, kind.hit()))
    # Refused ranges change nothing.
    L, scratch = dpf.lib(), other.copy()                            # (refused before the buffer is looked at)
    for first, n in [(N, 1), (N + 1, 0), (0, N + 1), (5, (1 << 64) - 3), ((1 << 64) - 1, 2)]:
        assert L.dpf_pir_db_export(a._h, first, n, dpf._buf(scratch)) == dpf.DPF_ERR_PARAM, (first, n)
        assert b"outside the DB" in L.dpf_last_error()
        assert L.dpf_pir_db_xor_records(a._h, first, n, dpf._buf(scratch)) == dpf.DPF_ERR_PARAM, (first, n)
    assert np.array_equal(scratch, other)
    for call in (lambda: a.export(N, 1), lambda: a.export(N - 1, 2), lambda: a.xor_records(other[:2], first=N - 1)):
        with pytest.raises(dpf.DPFPanic) as e:
            call()
        assert e.value.code == dpf.DPF_ERR_PARAM
    assert np.array_equal(a.export(), both)
    # Clear, and the whole DB XORed back in.
    a.clear()
    assert not a.export().any()
    assert not a.answer(kind.ka).any()
    a.xor_records(both)
    assert np.array_equal(a.export(), both)
    assert np.array_equal(a.answer(kind.kb), _answers(both, kind.sel(1)))
    if kind.pts is not None:                                        # a sparse handle kept its points
        assert np.array_equal(a.answer(kind.ka) ^ a.answer(kind.kb), _answers(both, kind.hit()))
    a.close()
    b.close()


def _kind(name, ngpus=1):
    if name == "dense32":
        return Kind(name, 12, 3000, 32, 9, ngpus=ngpus)
    if name == "dense5":
        return Kind(name, 12, 3000, 5, 9, ngpus=ngpus)
    if name == "dense64":
        return Kind(name, 12, 3000, 64, 9, ngpus=ngpus)
    if name == "sparse":
        return Kind(name, 40, 1000, 20, 9, points=True, ngpus=ngpus)
    return Kind(name, 9, 900, 20, 6, groups=3, ngpus=ngpus)         # G = 3 groups of 300 records


KINDS = ["dense32", "dense5", "sparse", "grouped"]


@pytest.mark.parametrize("name", KINDS)
def test_handle_export_merge_clear(name):
    _handle_checks(_kind(name))


@pytest.mark.parametrize("name", KINDS)
def test_handle_in_pieces_of_one_super_group(name):
    """dpf_set_export_limits at one super-group's bytes: the same results through many pieces."""
    kind = _kind(name)
    try:
        dpf.set_export_limits(256 * ((kind.rec + 3) // 4 * 4))
        _handle_checks(kind)
    finally:
        dpf.set_export_limits(0)


def test_empty_handles():
    for pdb in (dpf.PirDB(np.zeros((0, 32), np.uint8), 12, rec_bytes=32),
                dpf.PirDB(np.zeros((0, 20), np.uint8), 9, rec_bytes=20, groups=0)):
        assert pdb.export().shape[0] == 0
        pdb.xor_records(np.zeros((0, pdb.rec_bytes), np.uint8))
        pdb.clear()
        with pytest.raises(dpf.DPFPanic):
            pdb.export(0, 1)
        pdb.close()


def _child(mode):
    import subprocess
    env = dict(os.environ)
    env.pop("DPF_PIR_FOLD", None)
    if mode == "lds":
        env["DPF_PIR_FOLD"] = "lds"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode], capture_output=True, text=True, timeout=240,
                       env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith("done")


def test_two_shard_handles():
    """gpu_init_devices([0, 0]) and ngpus=2: export, xor_records and clear over
    ranges that cross the shard boundary, dense (record 2048 of 3000) and
    grouped (groups 0, 1 | 2), whole and in pieces of one super-group."""
    _child("two-shards")


def test_row_major_handle():
    """DPF_PIR_FOLD=lds keeps the shards row-major: plain copies and a plain XOR of rows (two shards)."""
    _child("lds")


if __name__ == "__main__":
    dpf.gpu_init_devices([0, 0])
    if sys.argv[1] == "lds":
        _handle_checks(_kind("dense64", ngpus=2), boundary=2048)
    else:
        for limit in (0, 256 * 20):
            dpf.set_export_limits(limit)
            _handle_checks(_kind("dense5", ngpus=2), boundary=2048)
            _handle_checks(_kind("dense32", ngpus=2), boundary=2048)
            _handle_checks(_kind("grouped", ngpus=2), boundary=600)
        dpf.set_export_limits(0)
    dpf.gpu_shutdown()
    print("done")
