"""Private writes: messages XORed into the records that EvalFull bits select
(dpf_xor_scatter_dev, dpf_xor_scatter_sliced_wide_dev, dpf_pir_write_wide_dev,
dpf_pir_write_sliced_wide_dev and the handle's write).  Expected values come
from oracle.evalfull_batch plus numpy and from the numpy restatement of the
wide sliced layout's definition (include/dpf_hip.h); never from the code under
test.  Everything is bit-exact.

The two-shard and the row-major (DPF_PIR_FOLD=lds) handles need a process of
their own (the device registry and the fold choice are process-wide): the
tests at the end run this file as a script."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "dpf-go_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import dpf                  # noqa: E402
from dpf import synth       # noqa: E402
import oracle               # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 256


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert dpf.gpu_init(1) >= 1


def _layout(db: np.ndarray) -> np.ndarray:
    """u32 dbs[S][c][n][g] as bytes: bit j of the word = bit n of bytes
    [32c, 32c+32) of record 256 S + 32 g + j, bit n of a column being bit n%8
    of its byte n/8; records past nrec are 0 (include/dpf_hip.h)."""
    nrec, rec = db.shape
    C, nsg = rec // 32, (nrec + 255) // 256
    pad = np.zeros((nsg * 256, rec), np.uint8)
    pad[:nrec] = db
    b = np.unpackbits(pad, axis=1, bitorder="little")          # [256 S + 32 g + j][256 c + n]
    b = b.reshape(nsg, 8, 32, C, 256).transpose(0, 3, 4, 1, 2)  # [S][c][n][g][j]
    return np.packbits(np.ascontiguousarray(b).reshape(-1), bitorder="little")


def _dev(a):
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    if a.size == 0:                       # the entry points refuse null pointers, also with nothing to do
        return torch.zeros(16, dtype=torch.uint8, device="cuda")
    if not a.flags.writeable:             # a shared, frozen reference: torch wants a writable source
        a = a.copy()
    return torch.from_numpy(a.view(np.uint8)).cuda()


def _guarded(nbytes, fill):
    import torch
    return torch.full((nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")


def _sliced(db, nrec, rec, fill=0x5A):
    """The sliced DB in a buffer GUARD bytes longer, pre-filled with `fill`."""
    import torch
    size = dpf.pir_db_sliced_size_wide(nrec, rec)
    buf = _guarded(size, fill)
    if nrec:
        dpf.pir_db_slice_wide_dev(_dev(db), nrec, rec, buf)
    torch.cuda.synchronize()
    return buf, size


def _rows(db, fill=0x5A):
    import torch
    buf = _guarded(max(db.size, 16), fill)
    buf[:db.size] = _dev(db)[:db.size]
    torch.cuda.synchronize()
    return buf


def _apply(db, sel, msgs):
    """db[i] ^= XOR of msgs[k] over the keys with sel[k][i] (bool [nkeys][nrec])."""
    out = db.copy()
    if sel.shape[0] <= 8 or db.shape[0] < 4096:
        for k in range(sel.shape[0]):
            out[sel[k]] ^= msgs[k]
        return out
    # Many keys over many records: eight keys at a time through the table of
    # the XORs of their 256 subsets (the same sum, fewer passes over the DB).
    for k0 in range(0, sel.shape[0], 8):
        m = msgs[k0:k0 + 8]
        table = np.zeros((256, db.shape[1]), np.uint8)
        for j in range(m.shape[0]):
            table[((np.arange(256) >> j) & 1) == 1] ^= m[j]
        out ^= table[np.packbits(sel[k0:k0 + 8], axis=0, bitorder="little")[0]]
    return out


def _messages(rng, nkeys, rec):
    """Random messages with an all-ones and (from two keys) an all-zero one."""
    m = rng.integers(0, 256, (nkeys, rec), dtype=np.uint8)
    if nkeys >= 1:
        m[0] = 0xFF
    if nkeys >= 2:
        m[nkeys // 2] = 0
    return m


# ---- 1 / 2. the scatter over given bits --------------------------------------
SHAPES = [(300, 32, 1), (300, 64, 3), (1000, 96, 33), (1, 160, 2), (777, 1024, 5), (8197, 32, 64), (600, 32, 65),
          (600, 64, 130)]
LIMITED = [(1000, 96, 33), (8197, 32, 64)]


@functools.lru_cache(maxsize=None)
def _case(nrec, rec, nkeys):
    """(db, bits, stride, msgs, expected row-major DB, its sliced layout), computed once per shape.
    Rows of the bits do not start on 32-byte boundaries, and every bit at a
    position >= nrec is set."""
    rng = np.random.default_rng(nrec * 131 + rec * 7 + nkeys)
    stride = 16 * ((nrec + 127) // 128) + 16
    db = rng.integers(0, 256, (nrec, rec), dtype=np.uint8)
    bits = rng.integers(0, 256, (nkeys, stride), dtype=np.uint8)
    ub = np.unpackbits(bits, axis=1, bitorder="little")
    ub[:, nrec:] = 1
    bits = np.packbits(ub, axis=1, bitorder="little")
    msgs = _messages(rng, nkeys, rec)
    want = _apply(db, ub[:, :nrec].astype(bool), msgs)
    for a in (db, bits, msgs, want):
        a.setflags(write=False)
    lay = _layout(want)
    lay.setflags(write=False)
    return db, bits, stride, msgs, want, lay


def _scatter_sliced(nrec, rec, nkeys):
    import torch
    db, bits, stride, msgs, _, _ = _case(nrec, rec, nkeys)
    buf, size = _sliced(db, nrec, rec)
    dpf.xor_scatter_sliced_wide_dev(_dev(bits), stride, nkeys, _dev(msgs), buf, nrec, rec)
    torch.cuda.synchronize()
    return buf, size


def _check_sliced(nrec, rec, nkeys):
    buf, size = _scatter_sliced(nrec, rec, nkeys)
    got = buf.cpu().numpy()
    lay = _case(nrec, rec, nkeys)[5]
    assert size == lay.size
    assert np.array_equal(got[:size], lay)                      # padding of the last super-group included
    assert (got[size:] == 0x5A).all()


@pytest.mark.parametrize("nrec,rec,nkeys", SHAPES)
def test_scatter_sliced_leaves_the_documented_layout(nrec, rec, nkeys):
    _check_sliced(nrec, rec, nkeys)


@pytest.mark.parametrize("limits", [(1, 1), (3, 5), (2, 0)])
@pytest.mark.parametrize("nrec,rec,nkeys", LIMITED)
def test_scatter_sliced_under_fold_limits(nrec, rec, nkeys, limits):
    """One workgroup per launch with one super-group each, three workgroups
    with runs of five, two workgroups with long runs: several launches per key
    tile, runs across staging rounds, a run that ends inside one."""
    dpf.set_fold_limits(*limits)
    try:
        _check_sliced(nrec, rec, nkeys)
    finally:
        dpf.set_fold_limits(0, 0)


@pytest.mark.parametrize("nrec,rec,nkeys", SHAPES)
def test_scatter_rows_matches_expected_and_the_sliced_result(nrec, rec, nkeys):
    import torch
    db, bits, stride, msgs, want, _ = _case(nrec, rec, nkeys)
    buf = _rows(db)
    dpf.xor_scatter_dev(_dev(bits), stride, nkeys, _dev(msgs), buf, nrec, rec)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[:db.size].reshape(nrec, rec), want)
    assert (got[db.size:] == 0x5A).all()
    sbuf, _ = _scatter_sliced(nrec, rec, nkeys)
    d_out = torch.full((nrec * rec,), 0xAB, dtype=torch.uint8, device="cuda")
    dpf.pir_db_gather_sliced_wide_dev(sbuf, nrec, rec, _dev(np.arange(nrec, dtype=np.uint64)), nrec, d_out)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), got[:db.size])


# ---- 3. pir_write_*_dev with real keys ---------------------------------------
NK = 37


@functools.lru_cache(maxsize=None)
def _keys(logN):
    """37 key pairs, keys 0 and 1 sharing an alpha; both shares' EvalFull from the oracle."""
    al, s0, s1 = synth.key_seeds(NK, logN, first=300 + logN)
    al = al.copy()
    al[1] = al[0]
    ka, kb = dpf.gen_batch_seeded(al, logN, s0, s1)
    fa = oracle.evalfull_batch(ka, logN, nthreads=8)
    fb = oracle.evalfull_batch(kb, logN, nthreads=8)
    return al, ka, kb, fa, fb


def _slice_sel(full, logN, pb, prefix, nrec):
    """bool [nkeys][nrec]: the selection bits of subtree (pb, prefix)."""
    n = 1 << (logN - pb)
    ub = np.unpackbits(full, axis=1, bitorder="little")[:, :1 << logN]
    return ub[:, prefix * n:prefix * n + nrec].astype(bool)


def _write_dev(sliced, keys, logN, pb, prefix, msgs, db, nrec, rec):
    """The row-major DB after dpf_pir_write_(sliced_)wide_dev, read back whole.
    Sliced: the last super-group is compared with the layout's definition
    (padding included) by the caller through the returned raw tail."""
    import torch
    nk = keys.shape[0]
    d_work = torch.empty(dpf.pir_workspace_size(nk, logN, pb), dtype=torch.uint8, device="cuda")
    if sliced:
        buf, size = _sliced(db, nrec, rec)
        dpf.pir_write_sliced_wide_dev(_dev(keys), keys.shape[1], nk, logN, _dev(msgs), buf, nrec, rec, d_work,
                                      prefix_bits=pb, prefix=prefix)
        d_out = torch.full((nrec * rec,), 0xAB, dtype=torch.uint8, device="cuda")
        dpf.pir_db_gather_sliced_wide_dev(buf, nrec, rec, _dev(np.arange(nrec, dtype=np.uint64)), nrec, d_out)
        torch.cuda.synchronize()
        raw = buf.cpu().numpy()
        assert (raw[size:] == 0x5A).all()
        return d_out.cpu().numpy().reshape(nrec, rec), raw[size - 256 * rec:size]
    buf = _rows(db)
    dpf.pir_write_wide_dev(_dev(keys), keys.shape[1], nk, logN, _dev(msgs), buf, nrec, rec, d_work, prefix_bits=pb,
                           prefix=prefix)
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    assert (raw[db.size:] == 0x5A).all()
    return raw[:db.size].reshape(nrec, rec), None


@pytest.mark.parametrize("aes", ["ttable", "bitsliced"])
@pytest.mark.parametrize("logN", [8, 10, 13, 16])
def test_pir_write_dev_with_real_keys(logN, aes):
    """Both servers' writes on every subtree of prefix_bits 0 and 2, full and
    ragged slices, 32- and 96-byte records, 1 and 37 keys (keys 0 and 1 share
    an alpha), sliced and row-major: each server's DB equals the oracle's
    selection applied in numpy, and the XOR of the two servers' DBs differs
    from zero only at the alphas, by the XOR of the messages written there.
    Four (records, width, keys) combinations hold every pair of values of
    the three; all four run at prefix_bits 0 and the subtrees of prefix_bits 2
    share them, one each.  logN 8 has one tree level (stop = logN - 7), so
    prefix_bits 2 is refused there and prefix_bits 1 runs in its place."""
    al, ka, kb, fa, fb = _keys(logN)
    prev = dpf.set_aes_impl(aes)
    try:
        combos = [(False, 32, NK), (True, 96, NK), (False, 96, 1), (True, 32, 1)]
        deep = 2 if logN - 7 >= 2 else 1
        if deep != 2:
            import torch
            d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
            for f in (dpf.pir_write_wide_dev, dpf.pir_write_sliced_wide_dev):
                with pytest.raises(dpf.DPFPanic) as e:
                    f(_dev(ka[:1]), ka.shape[1], 1, logN, d, d, 16, 32, d, prefix_bits=2, prefix=0)
                assert e.value.code == dpf.DPF_ERR_PARAM
            assert not d.any()
        plan = [(0, 0, c) for c in combos]
        nsub = 1 << deep
        plan += [(deep, i % nsub, c) for i, c in enumerate(combos)]
        for pb, prefix, (ragged, rec, nk) in plan:
            n = 1 << (logN - pb)
            nrec = n - min(n // 2, 77) if ragged else n
            rng = np.random.default_rng(logN * 1000 + pb * 100 + prefix * 10 + rec + nk)
            db = rng.integers(0, 256, (nrec, rec), dtype=np.uint8)
            msgs = _messages(rng, nk, rec)
            got = {}
            for side, keys, full in (("a", ka, fa), ("b", kb, fb)):
                want = _apply(db, _slice_sel(full[:nk], logN, pb, prefix, nrec), msgs)
                for sliced in (True, False):
                    res, tail = _write_dev(sliced, keys[:nk], logN, pb, prefix, msgs, db, nrec, rec)
                    where = (logN, pb, prefix, ragged, rec, nk, side, sliced)
                    assert np.array_equal(res, want), where
                    if sliced:
                        last = (nrec - 1) // 256 * 256
                        assert np.array_equal(tail, _layout(want[last:])), where
                got[side] = want
            # Two-server property over the slice (from equal DBs).
            diff = got["a"] ^ got["b"]
            delta = np.zeros_like(diff)
            for k in range(nk):
                loc = int(al[k]) - prefix * n
                if 0 <= loc < nrec:
                    delta[loc] ^= msgs[k]
            assert np.array_equal(diff, delta), (logN, pb, prefix, ragged, rec, nk)
            if nk > 1 and pb == 0 and not ragged:
                assert np.array_equal(diff[int(al[0])], msgs[0] ^ msgs[1])      # the shared alpha: both messages
    finally:
        dpf.set_aes_impl(prev)


# ---- 4. degenerate cases -----------------------------------------------------
@pytest.mark.parametrize("nkeys,nrec", [(0, 300), (5, 0), (0, 0)])
def test_nothing_to_do_leaves_the_buffers_untouched(nkeys, nrec):
    import torch
    rec = 64
    _, ka, _, _, _ = _keys(10)
    d_any = torch.full((4096,), 0x11, dtype=torch.uint8, device="cuda")
    for sliced in (True, False):
        buf = _guarded(dpf.pir_db_sliced_size_wide(max(nrec, 1), rec), 0x77)
        before = buf.cpu().numpy()
        f = dpf.xor_scatter_sliced_wide_dev if sliced else dpf.xor_scatter_dev
        f(d_any, 64, nkeys, d_any, buf, nrec, rec)
        w = dpf.pir_write_sliced_wide_dev if sliced else dpf.pir_write_wide_dev
        d_work = torch.empty(dpf.pir_workspace_size(max(nkeys, 1), 10, 0), dtype=torch.uint8, device="cuda")
        w(_dev(ka[:max(nkeys, 1)]), ka.shape[1], nkeys, 10, d_any, buf, nrec, rec, d_work)
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), before)
    assert (d_any.cpu().numpy() == 0x11).all()


# ---- 5. handle ---------------------------------------------------------------
def _oracle_answers(keys, logN, db):
    """oracle.pir_answer_batch per 32-byte column of the records."""
    nrec, rec = db.shape
    cols = [oracle.pir_answer_batch(keys, logN, np.ascontiguousarray(db[:, c:c + 32]), nrec)[:, 0, :]
            for c in range(0, rec, 32)]
    return np.concatenate(cols, axis=1)


def _handle_checks(rec, ngpus=1, nrec=None):
    """PirDB.write at logN 12 (37 keys, two sharing an alpha), then the whole
    DB read back and a batch of PIR answers over it; a wrong message shape and
    a short key change nothing."""
    logN = 12
    nrec = (1 << logN) if nrec is None else nrec
    al, ka, kb, fa, _ = _keys(logN)
    rng = np.random.default_rng(rec * 3 + ngpus)
    db = synth.db_bytes(nrec * rec).reshape(nrec, rec).copy()
    msgs = _messages(rng, NK, rec)
    pdb = dpf.PirDB(db, logN, ngpus=ngpus, rec_bytes=rec)
    pdb.write(ka, msgs)
    want = _apply(db, _slice_sel(fa, logN, 0, 0, nrec), msgs)
    everything = np.arange(nrec, dtype=np.uint64)
    assert np.array_equal(pdb.read(everything), want)
    al2, s0, s1 = synth.key_seeds(20, logN, first=900)
    q, _ = dpf.gen_batch_seeded(al2, logN, s0, s1)
    assert np.array_equal(pdb.answer(q), _oracle_answers(q, logN, want))
    with pytest.raises(ValueError):
        pdb.write(ka, msgs[:, :rec - 1])
    with pytest.raises(ValueError):
        pdb.write(ka, msgs[:NK - 1])
    with pytest.raises(dpf.DPFPanic) as e:
        pdb.write(ka[:, :16 + 18 * (logN - 7)], msgs)            # one byte short of the last correction word
    assert e.value.code == dpf.DPF_ERR_KEYLEN
    assert np.array_equal(pdb.read(everything), want)
    pdb.write(ka[:0], msgs[:0])                                  # no keys: nothing happens
    # The other server's share of the same batch: the two DBs now differ at the alphas only.
    pdb.write(kb, msgs)
    delta = np.zeros_like(db)
    for k in range(NK):
        if int(al[k]) < nrec:
            delta[int(al[k])] ^= msgs[k]
    assert np.array_equal(pdb.read(everything), db ^ delta)      # (A-share then B-share = the plain XOR at alpha)
    pdb.close()


@pytest.mark.parametrize("rec,nrec", [(32, None), (96, 3000)])
def test_handle_write(rec, nrec):
    _handle_checks(rec, nrec=nrec)


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


def test_two_shard_handle_write():
    """gpu_init_devices([0, 0]) and PirDB(..., ngpus=2): every shard applies the batch to its slice."""
    _child("two-shards")


def test_row_major_handle_write():
    """DPF_PIR_FOLD=lds keeps the shards row-major: the plain scatter kernel (two shards)."""
    _child("lds")


if __name__ == "__main__":
    dpf.gpu_init_devices([0, 0])
    _handle_checks(64, ngpus=2)
    _handle_checks(32, ngpus=2, nrec=3000)
    dpf.gpu_shutdown()
    print("done")
