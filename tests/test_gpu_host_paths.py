"""Host-buffer entry points on the chunked paths of the staging pipeline
(dpf-go_amd/csrc/stage_plan.hpp), every byte against the oracle: batched Eval
over several chunks with a ragged last one, EvalFull in subtree slabs of each
key, and EvalFull in groups of whole keys with a ragged last group."""
import numpy as np
import pytest

import dpf
from dpf import synth
import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert dpf.gpu_init(1) >= 1


@pytest.mark.parametrize("ppk", [1500032, 1400001])
def test_host_eval_batch_three_chunks_ragged_last(ppk):
    """5 keys whose points fill 12 MB each: chunks of 2, 2 and 1 keys through
    the two staging slots (the third chunk reuses the first's).  1500032 is a
    multiple of 128 (the persistent Eval kernel); 1400001 is odd (the
    per-pair kernel, with pairs that straddle keys)."""
    logN, nk = 12, 5
    al, s0, s1 = synth.key_seeds(nk, logN, first=1212)
    ka, _ = dpf.gen_batch_seeded(al, logN, s0, s1)
    xs = np.ascontiguousarray(synth.eval_points(ppk, nk, logN).T)   # one stream per point: nk draws, not ppk
    got = dpf.eval_batch(ka, xs, logN, ngpus=1)
    assert np.array_equal(got, oracle.eval_batch(ka, xs, logN, nthreads=8))


@pytest.mark.parametrize("impl", ["ttable", "bitsliced"])
@pytest.mark.parametrize("nk", [1, 3])
def test_host_evalfull_batch_subtree_slabs(nk, impl):
    """logN = 26 is 8 MiB a key: every key leaves in 4 subtree slabs of 2 MiB
    (ADVICE r06 asked for this check).  The T-table back end runs each slab
    straight from the key bytes, the byte-sliced one from the expanded
    records."""
    logN = 26
    al, s0, s1 = synth.key_seeds(nk, logN, first=2600 + nk)
    ka, _ = dpf.gen_batch_seeded(al, logN, s0, s1)
    prev = dpf.set_aes_impl(impl)
    try:
        got = dpf.evalfull_batch(ka, logN, ngpus=1)
    finally:
        dpf.set_aes_impl(prev)
    assert np.array_equal(got, oracle.evalfull_batch(ka, logN, nthreads=8))


def test_host_evalfull_batch_ragged_second_chunk():
    """300 keys at logN = 20: a chunk of 256 whole keys, then one of 44."""
    logN, nk = 20, 300
    al, s0, s1 = synth.key_seeds(nk, logN, first=3003)
    ka, _ = dpf.gen_batch_seeded(al, logN, s0, s1)
    got = dpf.evalfull_batch(ka, logN, ngpus=1)
    assert np.array_equal(got, oracle.evalfull_batch(ka, logN, nthreads=8))
