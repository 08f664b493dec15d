"""Deep domains (logN 33..63) on the CPU: the two oracle helpers that stand in
for a full EvalFull nothing can hold, and the C ABI's subtree validation at
logN 63.  No GPU compute.

oracle.reroot_key turns a deep key into the key of one of its subtrees, so
oracle.evalfull_batch and pir_answer_batch give the subtree's slice;
oracle.evalfull_subtree_by_points gives the same slice by Eval (dpf.go:171-211)
of every point of it.  They share the AES and nothing else: the first follows
evalFullRecursive's steps (dpf.go:213-241), the second the reference's Eval."""
import numpy as np
import pytest

import dpf
from dpf import synth
import oracle

NT = 8

# (logN, span): the subtree holds 2^span points, prefix_bits = logN - span
CASES = [(20, 13), (33, 12), (40, 16), (48, 11), (63, 10), (63, 17)]


def _bits(a):
    return np.unpackbits(np.asarray(a, np.uint8), bitorder="little")


def _prefixes(alpha, logN, span):
    pb = logN - span
    ps = [alpha >> span, (alpha >> span) ^ 1, 0, (1 << pb) - 1]
    if pb > 32:
        ps.append((1 << (pb - 1)) | (3 << 31) | 0x5A5)   # bits 31 and 32, and one above bit 33
        assert ps[-1] >> 34 and ps[-1] < (1 << pb)
    return ps


def _slice(key, logN, pb, prefix):
    k = np.frombuffer(oracle.reroot_key(key, logN, pb, prefix), np.uint8).reshape(1, -1)
    return oracle.evalfull_batch(k, logN - pb, nthreads=1)[0]


@pytest.mark.parametrize("logN,span", CASES)
def test_rerooted_key_agrees_with_point_evaluation(logN, span):
    """Both shares, every prefix class: EvalFull of the re-rooted key ==
    Eval of every point of the subtree; the shares XOR to the point function
    restricted to the subtree (one-hot under alpha's prefix, zero elsewhere)."""
    pb = logN - span
    al, s0, s1 = synth.key_seeds(1, logN, first=3300 + logN + span)
    ka, kb = dpf.gen_batch_seeded(al, logN, s0, s1)
    alpha = int(al[0])
    shares = [ka[0].tobytes(), kb[0].tobytes()]
    full = [oracle.evalfull(k, logN) for k in shares] if logN == 20 else None   # the whole domain, where it fits
    n = (1 << span) // 8
    for prefix in _prefixes(alpha, logN, span):
        got = []
        for i, k in enumerate(shares):
            a = _slice(k, logN, pb, prefix)
            b = oracle.evalfull_subtree_by_points(k, logN, pb, prefix, NT)
            assert a.shape == b.shape == (n,)
            assert np.array_equal(a, b), (logN, span, hex(prefix))
            if full is not None:
                assert a.tobytes() == full[i][prefix * n:(prefix + 1) * n]
            got.append(a)
        x = _bits(got[0] ^ got[1])
        if prefix == alpha >> span:
            assert x.sum() == 1 and x[alpha & ((1 << span) - 1)] == 1
        else:
            assert not x.any()


def test_rerooting_malformed_keys():
    """Arbitrary key bytes at logN 48 (byte-valued t through 37 levels, an
    unmasked root LSB) and a well-formed key with 9 trailing bytes (the final
    CW is the last 16 bytes, dpf.go:206,219)."""
    rng = np.random.default_rng(48)
    logN, span = 48, 11
    pb = logN - span
    rnd = rng.integers(0, 256, dpf.key_len(logN), dtype=np.uint8)
    rnd[16] = 0xA4
    al, s0, s1 = synth.key_seeds(1, logN, first=4809)
    ka, _ = dpf.gen_batch_seeded(al, logN, s0, s1)
    tail = np.concatenate([ka[0], rng.integers(0, 256, 9, dtype=np.uint8)])
    for key, alpha in ((rnd, 0x5A5A5A5A5A5A), (tail, int(al[0]))):
        for prefix in _prefixes(alpha, logN, span):
            a = _slice(key.tobytes(), logN, pb, prefix)
            assert np.array_equal(a, oracle.evalfull_subtree_by_points(key, logN, pb, prefix, NT)), hex(prefix)
    assert len(oracle.reroot_key(tail.tobytes(), logN, pb, 0)) == dpf.key_len(span) + 9


def test_rerooting_nothing_is_the_key_itself():
    al, s0, s1 = synth.key_seeds(1, 33)
    ka, _ = dpf.gen_batch_seeded(al, 33, s0, s1)
    assert oracle.reroot_key(ka[0].tobytes(), 33, 0, 0) == ka[0].tobytes()


# ---- subtree validation of the C ABI at logN 63, before any device call ----
LOGN, STOP = 63, 56
P = 1 << 16          # fake, 16-byte-aligned device address: never dereferenced


def _entries():
    """name -> call(nkeys, prefix_bits, prefix, nrec); nrec is None for the
    entries without a DB."""
    L = dpf.lib()
    kl = dpf.key_len(LOGN)
    tree = {
        "dpf_evalfull_subtree_dev": lambda nk, pb, p, _: L.dpf_evalfull_subtree_dev(0, P, kl, nk, LOGN, pb, p, P, P, None),
        "dpf_evalfull_expanded_dev": lambda nk, pb, p, _: L.dpf_evalfull_expanded_dev(0, P, nk, LOGN, pb, p, P, None),
    }
    pir = {
        "dpf_pir_answer_dev":
            lambda nk, pb, p, nr: L.dpf_pir_answer_dev(0, P, kl, nk, LOGN, pb, p, P, nr, P, P, None),
        "dpf_pir_answer_sliced_dev":
            lambda nk, pb, p, nr: L.dpf_pir_answer_sliced_dev(0, P, kl, nk, LOGN, pb, p, P, nr, P, P, None),
        "dpf_pir_answer_wide_dev":
            lambda nk, pb, p, nr: L.dpf_pir_answer_wide_dev(0, P, kl, nk, LOGN, pb, p, P, nr, 96, P, P, None),
        "dpf_pir_answer_sliced_wide_dev":
            lambda nk, pb, p, nr: L.dpf_pir_answer_sliced_wide_dev(0, P, kl, nk, LOGN, pb, p, P, nr, 96, P, P, None),
        "dpf_pir_write_wide_dev":
            lambda nk, pb, p, nr: L.dpf_pir_write_wide_dev(0, P, kl, nk, LOGN, pb, p, P, P, nr, 96, P, None),
        "dpf_pir_write_sliced_wide_dev":
            lambda nk, pb, p, nr: L.dpf_pir_write_sliced_wide_dev(0, P, kl, nk, LOGN, pb, p, P, P, nr, 96, P, None),
    }
    return tree, pir


ENTRY_NAMES = ["dpf_evalfull_subtree_dev", "dpf_evalfull_expanded_dev", "dpf_pir_answer_dev",
               "dpf_pir_answer_sliced_dev", "dpf_pir_answer_wide_dev", "dpf_pir_answer_sliced_wide_dev",
               "dpf_pir_write_wide_dev", "dpf_pir_write_sliced_wide_dev"]


@pytest.mark.parametrize("name", ENTRY_NAMES)
def test_subtree_arguments_are_validated_at_logN_63(name):
    """A prefix of 2^prefix_bits (one past the last subtree, also where it
    needs more than 32 bits), prefix_bits = stop + 1 and a DB of one record
    more than the subtree's domain are DPF_ERR_PARAM at every entry point that
    takes a subtree; the deepest subtree there is, with no keys, is DPF_OK.
    The pointers are fake: every check comes before the first device call."""
    tree, pir = _entries()
    call = {**tree, **pir}[name]
    for pb in (0, 1, 31, 32, 33, 39, 50, STOP):
        nrec = min(1 << (LOGN - pb), 1 << 20)
        assert call(4, pb, 1 << pb, nrec) == dpf.DPF_ERR_PARAM, (name, pb)
        assert "prefix" in dpf.lib().dpf_last_error().decode()
    assert call(4, STOP + 1, 0, 128) == dpf.DPF_ERR_PARAM
    assert call(4, STOP + 1, (1 << (STOP + 1)) - 1, 128) == dpf.DPF_ERR_PARAM
    if name in pir:
        for pb in (28, 33, 50, STOP):
            assert call(4, pb, (1 << pb) - 1, (1 << (LOGN - pb)) + 1) == dpf.DPF_ERR_PARAM, (name, pb)
            assert "records" in dpf.lib().dpf_last_error().decode()
    assert call(0, STOP, (1 << STOP) - 1, 128) == dpf.DPF_OK
