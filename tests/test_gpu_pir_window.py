"""PIR over any record range on the GPU: the device re-root (dpf_subkeys_dev)
byte for byte against oracle.reroot_key, the window EvalFull against the same
slice of oracle.evalfull, the window answers and writes against numpy
(tests/pir_ref.py) over the oracle's selection bits, the subtree route against
the dense entry point, the stream contract by the protocol of
tests/test_gpu_stream_capture.py, and the ranged handle against a numpy model
of the DB (in the process at one GPU; over 2 and 3 logical devices in a child
process, this file run as a script).  Everything runs with both key shares,
the tree cases under both AES back ends.  References are computed once per
module and left unchanged."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "dpf-go_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import dpf                              # noqa: E402
from dpf import shard, synth            # noqa: E402
import oracle                           # noqa: E402
import pir_ref as ref                   # noqa: E402

pytestmark = pytest.mark.gpu
SHARES = (0, 1)
AES = ("ttable", "bitsliced")
GUARD, POISON = 64, 0xAB


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert dpf.gpu_init(1) >= 1
    prev = dpf.set_pir_kernel("split")
    yield
    dpf.set_pir_kernel(prev)


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _pairs(logN, nk, first=300):
    """(alphas, A-share keys, B-share keys) of nk pairs."""
    al, s0, s1 = synth.key_seeds(nk, logN, first=first + 11 * logN)
    ka, kb = dpf.gen_batch_seeded(al, logN, s0, s1)
    return _frozen(al), _frozen(ka), _frozen(kb)


def _keys(logN, nk, share, first=300):
    return _pairs(logN, nk, first)[1 + share]


@functools.lru_cache(maxsize=None)
def _full(logN, nk, share):
    return _frozen(oracle.evalfull_batch(_keys(logN, nk, share), logN, nthreads=8))


@functools.lru_cache(maxsize=None)
def _rand(tag, *shape):
    return _frozen(np.random.default_rng([tag, *shape]).integers(0, 256, shape, dtype=np.uint8))


def _dev(a, extra=0, fill=POISON):
    """A device copy of the bytes of `a` with `extra` poisoned bytes behind them (16-byte-aligned, at least 16)."""
    import torch
    a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    t = torch.full((max(16, a.size + extra),), fill, dtype=torch.uint8, device="cuda")
    if a.size:
        t[:a.size].copy_(torch.from_numpy(a.copy()))
    return t


def _empty(nbytes):
    import torch
    return torch.full((max(16, nbytes),), POISON, dtype=torch.uint8, device="cuda")


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---- sub-keys -----------------------------------------------------------------------
def _check_subkeys(keys, logN, pb, first, npfx, misalign=0):
    """dpf_subkeys_dev over one run of prefixes == oracle.reroot_key of every (key, prefix); the bytes behind
    d_sub stay poison.  misalign: byte offset of d_keys and d_sub from a 16-byte boundary."""
    nk, kl = keys.shape
    sl = kl - 18 * pb
    dk = _dev(np.concatenate([np.zeros(misalign, np.uint8), keys.reshape(-1)]))[misalign:]
    out = _empty(misalign + nk * npfx * sl + GUARD)
    dpf.subkeys_dev(dk, kl, nk, logN, pb, first, npfx, out[misalign:])
    got = _host(out)
    assert (got[:misalign] == POISON).all() and (got[misalign + nk * npfx * sl:] == POISON).all(), "guard bytes written"
    got = got[misalign:misalign + nk * npfx * sl].reshape(nk, npfx, sl)
    for k in range(nk):
        for p in range(npfx):
            want = np.frombuffer(oracle.reroot_key(keys[k].tobytes(), logN, pb, first + p), np.uint8)
            assert np.array_equal(got[k, p], want), (logN, pb, first + p, k)


@pytest.mark.parametrize("share", SHARES)
def test_subkeys_every_prefix_at_logN_13(share):
    keys = _keys(13, 3, share)
    for pb in range(1, 7):
        _check_subkeys(keys, 13, pb, 0, 1 << pb)
    _check_subkeys(keys, 13, 6, 61, 3, misalign=3)         # a run that ends at the last prefix; odd buffer addresses
    _check_subkeys(keys, 13, 0, 0, 1)                      # the identity
    assert dpf.window_form_for(13, 31, 4).sub_key_len == keys.shape[1] - 18 * 6


@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("logN,pb", [(40, 33), (63, 56)])
def test_subkeys_of_deep_domains(logN, pb, share):
    keys = _keys(logN, 3, share)
    rng = np.random.default_rng([logN, pb])
    _check_subkeys(keys, logN, pb, 0, 2)
    _check_subkeys(keys, logN, pb, (1 << pb) - 2, 2)
    for r in rng.integers(0, (1 << pb) - 3, 3):
        _check_subkeys(keys, logN, pb, int(r), 3)
    al = int(_pairs(logN, 3)[0][0])                        # the path of a key's own alpha, and its neighbours
    _check_subkeys(keys, logN, pb, min(max((al >> (logN - pb)) - 1, 0), (1 << pb) - 3), 3)


@pytest.mark.parametrize("share", SHARES)
def test_subkeys_of_long_and_malformed_keys(share):
    logN, nk = 13, 3
    keys = _keys(logN, nk, share)
    long_ = np.concatenate([keys, _rand(40 + share, nk, 5)], axis=1)    # 5 trailing bytes: the final CW moves with them
    for pb in (1, 4, 6):
        _check_subkeys(long_, logN, pb, 0, 1 << pb)
    bad = keys.copy()
    rng = np.random.default_rng(41 + share)
    bad[:, 16] = (2, 0x80, 0xFF)                                        # t and the CW t bytes: values other than 0 and 1
    for lvl in range(logN - 7):
        bad[:, 17 + 18 * lvl + 16: 17 + 18 * lvl + 18] = rng.integers(2, 256, (nk, 2))
    for pb in (1, 3, 6):
        _check_subkeys(bad, logN, pb, 0, 1 << pb)
    # A short key whose final CW overlaps its last record still re-roots above that record.
    short = keys[:, :keys.shape[1] - 7]
    _check_subkeys(short, logN, 5, 0, 32)


# ---- window rows ----------------------------------------------------------------------
# The last four take the pieces route whatever the crossover (the subtree that
# holds them is over three times their size): s clamped at 7, 20 pieces of
# 2^8 points, and pieces of 2^13 points, which the byte-sliced tree runs.
WINDOWS = [(14, 0, 128), (14, 1, 1), (14, 3, 37), (14, 63, 2), (14, 127, 1), (14, 5, 123), (9, 1, 2), (6, 0, 1),
           (14, 60, 8), (14, 41, 39), (19, 1000, 1100), (19, 1001, 1111)]
PIECES = {(14, 63, 2), (14, 60, 8), (14, 41, 39), (19, 1000, 1100), (19, 1001, 1111)}


def _enclosed(fb, nb):
    """Does an aligned subtree of at most twice the window's points hold the window?"""
    return 1 << (fb ^ (fb + nb - 1)).bit_length() <= 2 * nb


def _check_rows(logN, fb, nb, nk, share, pad=0):
    keys = _keys(logN, nk, share)
    kl = keys.shape[1]
    f = dpf.window_form_for(logN, fb, nb, kl)
    stride = f.row_bytes + pad
    dk = _dev(keys)
    rows = _empty(nk * stride + GUARD)
    work = _empty(dpf.evalfull_window_workspace_size(nk, logN, fb, nb))
    try:
        dpf.evalfull_window_dev(dk, kl, nk, logN, fb, nb, rows, stride, work)
        got = _host(rows)
    finally:
        dpf.forget_workspace(work)
    assert (got[nk * stride:] == POISON).all(), "bytes behind the last row written"
    got = got[:nk * stride].reshape(nk, stride)
    want = _full(logN, nk, share)[:, 16 * fb:16 * (fb + nb)]
    assert np.array_equal(got[:, f.row_offset:f.row_offset + 16 * nb], want), (logN, fb, nb, share)
    if pad:
        assert (got[:, f.row_bytes:] == POISON).all(), "bytes between the rows written"
    return f


@pytest.mark.parametrize("aes", AES)
@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("logN,fb,nb", WINDOWS)
def test_window_rows(logN, fb, nb, share, aes):
    prev = dpf.set_aes_impl(aes)
    try:
        for nk in (1, 3):
            f = _check_rows(logN, fb, nb, nk, share)
        assert _enclosed(fb, nb) == ((logN, fb, nb) not in PIECES)
        assert f.route == (dpf.WINDOW_PIECES if (logN, fb, nb) in PIECES else dpf.WINDOW_SUBTREE)
        _check_rows(logN, fb, nb, 3, share, pad=32)        # a larger stride: a launch per key
    finally:
        dpf.set_aes_impl(prev)


# ---- answers and writes ------------------------------------------------------------------
PLOGN = 16
NKEYS = (1, 5, 65)
FIRSTS = (0, 128, 128 * 37, 128 * 63)     # 128 * 63: 255, 256 and 5000 records from there straddle point 2^13 (pieces)


def _nrecs(first):
    return (1, 255, 256, 5000, (1 << PLOGN) - first)


@functools.lru_cache(maxsize=None)
def _db(rec):
    return _rand(50, 1 << PLOGN, rec)                     # record j of the domain, for every window


def _window_sel(logN, nk, share, first, nrec):
    """Packed selection rows of records [first, first + nrec): the oracle's EvalFull bytes from first / 8."""
    return _full(logN, nk, share)[:, first // 8:first // 8 + 16 * ((nrec + 127) // 128)]


def _fold(rows, db, nrec):
    """ref.xor_fold in float32 (the counts stay below 2^24: exact), for the 2^16-record windows."""
    assert nrec < 1 << 24
    bits = ref.sel_bool(rows, nrec).astype(np.float32)
    dbb = np.unpackbits(db[:nrec], axis=1, bitorder="little").astype(np.float32)
    par = (bits @ dbb).astype(np.int64) & 1
    return np.packbits(par.astype(np.uint8), axis=1, bitorder="little")


@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("rec", [4, 8, 32, 100])          # 8: what the handle makes of 7-byte records
@pytest.mark.parametrize("first", FIRSTS)
def test_answer_window(first, rec, share):
    nkmax, kl = max(NKEYS), dpf.key_len(PLOGN)
    dk = _dev(_keys(PLOGN, nkmax, share))
    for nrec in _nrecs(first):
        db = _db(rec)[first:first + nrec]
        want = _fold(_window_sel(PLOGN, nkmax, share, first, nrec), db, nrec)
        dbs = _dev(ref.layout(db))
        for nk in NKEYS:
            ans = _empty(nk * rec + GUARD)
            work = _empty(dpf.pir_window_workspace_size(nk, PLOGN, first, nrec, rec))
            try:
                dpf.pir_answer_window_dev(dk, kl, nk, PLOGN, first, dbs, nrec, rec, ans, work)
                got = _host(ans)
            finally:
                dpf.forget_workspace(work)
            assert np.array_equal(got[:nk * rec].reshape(nk, rec), want[:nk]), (first, nrec, rec, nk, share)
            assert (got[nk * rec:] == POISON).all()


@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("rec", [4, 8, 32, 100])
@pytest.mark.parametrize("first", FIRSTS)
def test_write_window(first, rec, share):
    """The sliced DB after the write, whole, equals the layout's definition of
    the expected records: the padding of the last super-group stays zero."""
    nkmax, kl = max(NKEYS), dpf.key_len(PLOGN)
    dk = _dev(_keys(PLOGN, nkmax, share))
    msgs = _rand(51 + share, nkmax, rec)
    dm = _dev(msgs)
    for nrec in _nrecs(first):
        db = _db(rec)[first:first + nrec]
        sel = _window_sel(PLOGN, nkmax, share, first, nrec)
        lay = ref.layout(db)
        for nk in NKEYS:
            dbs = _dev(lay, extra=GUARD)
            work = _empty(dpf.pir_window_workspace_size(nk, PLOGN, first, nrec, rec))
            try:
                dpf.pir_write_window_dev(dk, kl, nk, PLOGN, first, dm, dbs, nrec, rec, work)
                got = _host(dbs)
            finally:
                dpf.forget_workspace(work)
            want = ref.layout(ref.xor_scatter(db, sel[:nk], msgs[:nk], nrec))
            assert want.size == dpf.pir_db_sliced_size_any(nrec, rec)
            assert np.array_equal(got[:want.size], want), (first, nrec, rec, nk, share)
            assert (got[want.size:] == POISON).all()


def test_alpha_below_inside_and_above_the_window():
    """Both shares' answers XOR to the record at alpha where alpha lies in the
    window and to zero elsewhere; both shares' writes change that record alone."""
    first, nrec, rec, logN = 128 * 37, 5000, 32, PLOGN
    alphas = np.array([0, first - 1, first, first + 4999, first + 5000, 60000, first + 2500], np.uint64)
    nk = alphas.size
    _, s0, s1 = synth.key_seeds(nk, logN, first=900)
    ka, kb = dpf.gen_batch_seeded(alphas, logN, s0, s1)
    db = _db(rec)[first:first + nrec]
    msgs = _rand(53, nk, rec)
    inside = (alphas >= first) & (alphas < first + nrec)
    ans, after = [], []
    for keys in (ka, kb):
        dk, dbs, a, dm = _dev(keys), _dev(ref.layout(db)), _empty(nk * rec), _dev(msgs)
        work = _empty(dpf.pir_window_workspace_size(nk, logN, first, nrec, rec))
        try:
            dpf.pir_answer_window_dev(dk, keys.shape[1], nk, logN, first, dbs, nrec, rec, a, work)
            ans.append(_host(a)[:nk * rec].reshape(nk, rec).copy())
            dpf.pir_write_window_dev(dk, keys.shape[1], nk, logN, first, dm, dbs, nrec, rec, work)
            after.append(_host(dbs)[:dpf.pir_db_sliced_size_any(nrec, rec)].copy())
        finally:
            dpf.forget_workspace(work)
    x = ans[0] ^ ans[1]
    want_db = db.copy()
    for k in range(nk):
        assert np.array_equal(x[k], db[int(alphas[k]) - first] if inside[k] else np.zeros(rec, np.uint8)), k
        if inside[k]:
            want_db[int(alphas[k]) - first] ^= msgs[k]
    # (a ^ m_a) ^ (a ^ m_b) = m_a ^ m_b, and layout is linear: the two servers' DBs differ by the messages at alpha.
    assert np.array_equal(after[0] ^ after[1], ref.layout(want_db ^ db))


@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("nrec,route,pb,npieces", [(5000, dpf.WINDOW_SUBTREE, 40 - 13, 1), (128 * 62 - 50, dpf.WINDOW_PIECES, 40 - 8, 32)])
def test_window_of_a_deep_domain(nrec, route, pb, npieces, share):
    logN, first, rec, nk = 40, 128 * ((1 << 30) + 3), 20, 5
    alphas = np.array([first + 7, first + nrec - 1, first - 1, first + nrec, 12345], np.uint64)
    _, s0, s1 = synth.key_seeds(nk, logN, first=950)
    keys = dpf.gen_batch_seeded(alphas, logN, s0, s1)[share]
    xs = np.tile(np.uint64(first) + np.arange(nrec, dtype=np.uint64), (nk, 1))
    sel = ref.pack_rows(oracle.eval_batch(keys, xs, logN, nthreads=8), 16 * ((nrec + 127) // 128))
    db, msgs = _rand(54, nrec, rec), _rand(55, nk, rec)
    f = dpf.window_form_for(logN, first // 128, (nrec + 127) // 128)
    assert (f.route, f.prefix_bits, f.npieces) == (route, pb, npieces)
    dk, dbs, a, dm = _dev(keys), _dev(ref.layout(db)), _empty(nk * rec), _dev(msgs)
    work = _empty(dpf.pir_window_workspace_size(nk, logN, first, nrec, rec))
    try:
        dpf.pir_answer_window_dev(dk, keys.shape[1], nk, logN, first, dbs, nrec, rec, a, work)
        assert np.array_equal(_host(a)[:nk * rec].reshape(nk, rec), ref.xor_fold(sel, db, nrec))
        dpf.pir_write_window_dev(dk, keys.shape[1], nk, logN, first, dm, dbs, nrec, rec, work)
        want = ref.layout(ref.xor_scatter(db, sel, msgs, nrec))
        assert np.array_equal(_host(dbs)[:want.size], want)
    finally:
        dpf.forget_workspace(work)


@pytest.mark.parametrize("share", SHARES)
def test_subtree_route_is_the_dense_entry_point(share):
    """An aligned window takes WINDOW_SUBTREE, and its answers are
    pir_answer_sliced_any_dev's with the matching prefix, byte for byte."""
    logN, nk, rec = PLOGN, 5, 20
    for fb, nb in ((0, 512), (256, 256), (96, 32), (511, 1)):
        f = dpf.window_form_for(logN, fb, nb)
        assert (f.route, f.npieces, f.row_offset, f.first_prefix) == (dpf.WINDOW_SUBTREE, 1, 0, fb // nb)
        assert 1 << (logN - f.prefix_bits) == 128 * nb
    for fb, nb in ((1, 2), (0, 3), (1, 511), (70, 40)):                 # inside a subtree of at most twice their size
        f = dpf.window_form_for(logN, fb, nb)
        assert (f.route, f.npieces) == (dpf.WINDOW_SUBTREE, 1) and f.row_bytes <= 32 * nb
    for fb, nb in ((63, 2), (37, 40), (255, 2), (200, 100)):
        assert dpf.window_form_for(logN, fb, nb).route == dpf.WINDOW_PIECES
    first, nrec = 128 * 256, 128 * 256 - 77           # subtree (1, 1), some records short of it
    keys = _keys(logN, nk, share)
    db = _db(rec)[first:first + nrec]
    dk, dbs = _dev(keys), _dev(ref.layout(db))
    a, b = _empty(nk * rec), _empty(nk * rec)
    w1 = _empty(dpf.pir_window_workspace_size(nk, logN, first, nrec, rec))
    w2 = _empty(dpf.pir_workspace_size(nk, logN, 1))
    try:
        dpf.pir_answer_window_dev(dk, keys.shape[1], nk, logN, first, dbs, nrec, rec, a, w1)
        dpf.pir_answer_sliced_any_dev(dk, keys.shape[1], nk, logN, dbs, nrec, rec, b, w2, prefix_bits=1, prefix=1)
        got = _host(a)[:nk * rec]
        assert np.array_equal(got, _host(b)[:nk * rec])
        assert np.array_equal(got.reshape(nk, rec), ref.xor_fold(_window_sel(logN, nk, share, first, nrec), db, nrec))
    finally:
        dpf.forget_workspace(w1)
        dpf.forget_workspace(w2)


# ---- stream order and capture ------------------------------------------------------------
def _cap():
    import test_gpu_stream_capture as cap   # (Plan and the protocol; its tests are collected from its own file)
    return cap


CLOGN, CFB, CNB = 14, 41, 39                 # 20 pieces of 2^8 points, the window from byte 16 of a row to its end
CFIRST, CNREC = 128 * CFB, 128 * CNB - 50


@pytest.mark.parametrize("share", SHARES)
def test_capture_subkeys(share):
    cap = _cap()
    nk, pb, first, npfx = 3, 6, 20, 20
    ks = [_keys(CLOGN, nk, share, first=s) for s in cap.FIRST]

    def make():
        want = [np.stack([np.frombuffer(oracle.reroot_key(k.tobytes(), CLOGN, pb, first + p), np.uint8)
                          for k in keys for p in range(npfx)]) for keys in ks]
        p = cap.Plan("dpf_subkeys_dev")
        k = p.inp("keys", *ks)
        o = p.out("sub", *want)
        p.run = lambda st: dpf.subkeys_dev(k, ks[0].shape[1], nk, CLOGN, pb, first, npfx, o, stream=st)
        return p
    cap._with_settings(make)


@pytest.mark.parametrize("aes", AES)
@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("logN,fb,nb", [(CLOGN, CFB, CNB), (19, 1001, 1111)])
def test_capture_evalfull_window(logN, fb, nb, share, aes):
    cap = _cap()
    nk = 3
    ks = [_keys(logN, nk, share, first=s) for s in cap.FIRST]
    f = dpf.window_form_for(logN, fb, nb)
    assert f.route == dpf.WINDOW_PIECES and f.row_offset + 16 * nb == f.row_bytes   # the window ends a row: all of a row is pinned

    def make():
        # Whole rows: the pieces cover blocks [fb - row_offset / 16, ...) of the domain.
        b0 = fb - f.row_offset // 16
        want = [oracle.evalfull_batch(k, logN, nthreads=8)[:, 16 * b0:16 * b0 + f.row_bytes] for k in ks]
        p = cap.Plan("dpf_evalfull_window_dev")
        k = p.inp("keys", *ks)
        o = p.out("rows", *want)
        w = p.scratch(dpf.evalfull_window_workspace_size(nk, logN, fb, nb))
        p.run = lambda st: dpf.evalfull_window_dev(k, ks[0].shape[1], nk, logN, fb, nb, o, f.row_bytes, w, stream=st)
        return p
    cap._with_settings(make, aes=aes)


@pytest.mark.parametrize("aes", AES)
@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("write", [False, True])
def test_capture_pir_window(write, share, aes):
    cap = _cap()
    nk, rec, logN = 5, 20, CLOGN
    ks = [_keys(logN, nk, share, first=s) for s in cap.FIRST]

    def make():
        sel = [oracle.evalfull_batch(k, logN, nthreads=8)[:, CFIRST // 8:CFIRST // 8 + 16 * CNB] for k in ks]
        dbs = [cap._rand(s, 60, CNREC, rec) for s in (0, 1)]
        p = cap.Plan("dpf_pir_%s_window_dev" % ("write" if write else "answer"))
        k = p.inp("keys", *ks)
        w = p.scratch(dpf.pir_window_workspace_size(nk, logN, CFIRST, CNREC, rec))
        if write:
            msgs = [cap._rand(s, 61, nk, rec) for s in (0, 1)]
            m = p.inp("msgs", *msgs)
            d = p.inp("dbs", *[ref.layout(x) for x in dbs],
                      want=[ref.layout(ref.xor_scatter(dbs[s], sel[s], msgs[s], CNREC)) for s in (0, 1)])
            p.run = lambda st: dpf.pir_write_window_dev(k, ks[0].shape[1], nk, logN, CFIRST, m, d, CNREC, rec, w, stream=st)
        else:
            d = p.inp("dbs", *[ref.layout(x) for x in dbs])
            a = p.out("ans", *[ref.xor_fold(sel[s], dbs[s], CNREC) for s in (0, 1)])
            p.run = lambda st: dpf.pir_answer_window_dev(k, ks[0].shape[1], nk, logN, CFIRST, d, CNREC, rec, a, w, stream=st)
        return p
    cap._with_settings(make, aes=aes)


# ---- the ranged handle ----------------------------------------------------------------------
def _handle_checks(nrec, rec, ngpus):
    """Every operation of PirDB(..., ranged=True) against a numpy model of the DB."""
    logN = max(7, int(nrec - 1).bit_length())
    rng = np.random.default_rng([nrec, rec, ngpus])
    model = rng.integers(0, 256, (nrec, rec), dtype=np.uint8)
    h = dpf.PirDB(model, logN, ngpus=ngpus, rec_bytes=rec, ranged=True)
    try:
        assert h.nrec == nrec and h.ngroups == 1
        ranges = [shard.record_range(nrec, ngpus, r) for r in range(ngpus)]
        assert ranges[-1][1] == nrec
        nk = 6
        alphas = np.array([0, nrec - 1, ranges[-1][0] - 1 if ngpus > 1 else 1, min(ranges[0][1], nrec - 1), nrec // 2,
                           (1 << logN) - 1], np.uint64)
        _, s0, s1 = synth.key_seeds(nk, logN, first=1000 + nrec)
        ka, kb = dpf.gen_batch_seeded(alphas, logN, s0, s1)
        sels = [ref.sel_bool(oracle.evalfull_batch(k, logN, nthreads=4), nrec) for k in (ka, kb)]

        def fold(sel):
            out = np.zeros((nk, rec), np.uint8)
            for k in range(nk):
                if sel[k].any():
                    out[k] = np.bitwise_xor.reduce(model[sel[k]], axis=0)
            return out

        def check_answers(where):
            got = [h.answer(k) for k in (ka, kb)]
            for s in SHARES:
                assert np.array_equal(got[s], fold(sels[s])), (where, s)
            x = got[0] ^ got[1]
            for k in range(nk):
                a = int(alphas[k])
                assert np.array_equal(x[k], model[a] if a < nrec else np.zeros(rec, np.uint8)), (where, k)

        check_answers("created")
        assert np.array_equal(h.export(), model)
        # update / read, across the shard borders
        idx = np.array(sorted({0, nrec - 1, *(lo for lo, _ in ranges if lo < nrec), *(hi - 1 for lo, hi in ranges if hi > lo),
                               nrec // 3}), np.uint64)
        recs = rng.integers(0, 256, (idx.size, rec), dtype=np.uint8)
        h.update(idx, recs)
        model[idx.astype(np.int64)] = recs
        assert np.array_equal(h.read(idx[::-1]), model[idx[::-1].astype(np.int64)])
        with pytest.raises(dpf.DPFPanic):
            h.update(np.array([nrec], np.uint64), recs[:1])
        check_answers("updated")
        # private write with one share, then the other: the model changes at alpha only
        msgs = rng.integers(0, 256, (nk, rec), dtype=np.uint8)
        for s, keys in enumerate((ka, kb)):
            h.write(keys, msgs)
            for k in range(nk):
                model[sels[s][k]] ^= msgs[k]
        assert np.array_equal(h.export(), model)
        check_answers("written")
        with pytest.raises(dpf.DPFPanic):
            h.write_grouped(ka, msgs)
        with pytest.raises(dpf.DPFPanic):
            h.write(ka[:, :10], msgs)
        # export of a range over a border, merge, clear
        lo, n = max(0, ranges[0][1] - 5), min(11, nrec - max(0, ranges[0][1] - 5))
        assert np.array_equal(h.export(lo, n), model[lo:lo + n])
        other = rng.integers(0, 256, (n, rec), dtype=np.uint8)
        h.xor_records(other, lo)
        model[lo:lo + n] ^= other
        assert np.array_equal(h.export(), model)
        check_answers("merged")
        with pytest.raises(dpf.DPFPanic):
            h.export(nrec - 1, 2)
        h.clear()
        model[:] = 0
        assert not h.export().any() and not h.answer(ka).any() and h.nrec == nrec
    finally:
        h.close()
    return ranges


@pytest.mark.parametrize("rec", [7, 32])
@pytest.mark.parametrize("nrec", [1000, 5 * (1 << 10) + 3])
def test_ranged_handle_on_one_gpu(nrec, rec):
    _handle_checks(nrec, rec, 1)


def test_ranged_handle_refuses_what_it_cannot_hold():
    db = np.zeros((300, 8), np.uint8)
    with pytest.raises(dpf.DPFPanic):
        dpf.PirDB(db, 8, ngpus=1, rec_bytes=8, ranged=True)          # 300 records, 2^8 points
    with pytest.raises(dpf.DPFPanic):
        dpf.PirDB(db, 10, ngpus=dpf.gpu_count() + 1, rec_bytes=8, ranged=True)
    with pytest.raises(ValueError):
        dpf.PirDB(db, 10, rec_bytes=8, ranged=True, groups=3)


def test_ranged_handle_over_two_and_three_shards():
    """gpu_init_devices([0, 0, 0]) and PirDB(..., ngpus in {2, 3}, ranged=True)
    over logical devices (one GPU opened three times) at 1000 and 5 * 2^10 + 3
    records of 7 and 32 bytes; 1000 records over three shards leave the last
    one empty, and it still answers zero."""
    import subprocess
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "shards"], capture_output=True, text=True,
                       timeout=240, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith("done")


if __name__ == "__main__":
    assert dpf.gpu_init_devices([0, 0, 0]) == 3
    empty = 0
    for ngpus in (2, 3):
        for nrec in (1000, 5 * (1 << 10) + 3):
            for rec in (7, 32):
                empty += sum(lo == hi for lo, hi in _handle_checks(nrec, rec, ngpus))
    assert empty == 2            # 1000 records over 3 shards, at both widths
    print("done")
