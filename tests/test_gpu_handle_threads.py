"""The thread contract of the resident PIR handle and of the host-buffer paths
(include/dpf_hip.h: "All functions are thread-safe (per-device mutex +
stream)"; "a concurrent dpf_pir_answer sees the shard wholly before or wholly
after" each update chunk or write batch).

The staging buffers of a device (keys, workspace, output, points) are shared
by every handle on it and by the host-buffer dpf_evalfull_batch /
dpf_eval_batch, and are freed and reallocated when they grow; only the
device's mutex protects them.  Each test here runs, on one device and from
Python threads (ctypes releases the GIL, so the calls truly overlap):

  - a writer: a fixed number of update (or private write) calls that flip the
    whole DB (or one record) between two known states;
  - two readers: answer() of 16 key pairs at fixed alphas, the two shares
    XORed, in a loop until the writer is done; one of them also read()s the
    alphas.  Every call must show one state, never a mix;
  - a stager: host-buffer evalfull_batch and eval_batch with 1, 8, 64, 8, 1
    keys, so that the shared staging grows under the others;
  - a second handle of another record width, answered against its own fixed
    expectation.

Every expected value is computed before the threads start.  A run in which no
reader call fell between two writer calls proves nothing, so that count is
asserted to be at least one.

Widths: 32 and 20 (multiples of 4: plain staging copies), and for the write
test also 7 (padded to 8 on the device: messages, reads and answers go through
pitched copies); the second handle takes a width of the other kind."""
import os
import sys
import threading
import time

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

LOGN, NREC, NPROBE = 12, 3000, 16
WRITER_CALLS = 300
JOIN_SECONDS = 120
OTHER_REC = {32: 7, 20: 33, 7: 32}
STAGE_LOGN, STAGE_PPK, STAGE_CYCLE = 16, 64, (1, 8, 64, 8, 1)


STUCK = []                  # names of tests whose threads did not finish: a call may still be on the GPU


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert dpf.gpu_init(1) >= 1


@pytest.fixture(autouse=True)
def _nothing_after_a_stuck_thread():
    """Once a join has timed out, every later case of this module fails before it opens a handle."""
    if STUCK:
        pytest.fail("not run: a thread of %s never finished, so nothing more is started on the GPU here" % STUCK[0])


def _pairs(alphas, first):
    _, s0, s1 = synth.key_seeds(len(alphas), LOGN, first=first)
    return dpf.gen_batch_seeded(np.asarray(alphas, np.uint64), LOGN, s0, s1)


class Race:
    """The threads of one test around a writer; errors are collected and
    re-raised by run(), which also returns the overlap count."""

    def __init__(self):
        self.errors, self.lock = [], threading.Lock()
        self.stop, self.writer_done = threading.Event(), threading.Event()
        self.ready = []                  # one event per looping thread: its first call has returned
        self.calls = []                  # (start, end) of every reader answer() call
        self.first_done = self.last_begin = None
        self.threads = []
        self.stuck = False               # a join timed out: a call may still hold the handles
        self.handles = []

    def own(self, handle):
        self.handles.append(handle)
        return handle

    def close(self):
        """Free the handles (in a finally: a failed check must not leave them
        resident), unless a thread may still be inside a call on one of them."""
        if not self.stuck:
            for h in self.handles:
                h.close()

    def _guard(self, fn, *args):
        def body():
            try:
                fn(*args)
            except BaseException as e:   # noqa: B902 -- handed to the main thread
                with self.lock:
                    self.errors.append(e)
                self.stop.set()
        return body

    def looping(self, step):
        """step(i) again and again until the writer is done (at least once)."""
        ready = threading.Event()
        self.ready.append(ready)

        def loop():
            try:
                i = 0
                while True:
                    step(i)
                    ready.set()
                    i += 1
                    if self.writer_done.is_set() or self.stop.is_set():
                        return
            finally:
                ready.set()
        self.threads.append(threading.Thread(target=self._guard(loop), daemon=True))

    def writer(self, call, n):
        def write():
            for ev in self.ready:        # every other thread is in its loop
                ev.wait(JOIN_SECONDS)
            try:
                for i in range(n):
                    if self.stop.is_set():
                        return
                    if i == n - 1:
                        self.last_begin = time.perf_counter()
                    call(i)
                    if i == 0:
                        self.first_done = time.perf_counter()
            finally:
                self.writer_done.set()
        self.threads.append(threading.Thread(target=self._guard(write), daemon=True))

    def timed(self, fn, *args):
        t0 = time.perf_counter()
        r = fn(*args)
        with self.lock:
            self.calls.append((t0, time.perf_counter()))
        return r

    def run(self):
        for t in self.threads:
            t.start()
        deadline = time.monotonic() + JOIN_SECONDS
        for t in self.threads:
            t.join(max(0.0, deadline - time.monotonic()))
        if any(t.is_alive() for t in self.threads):
            self.stop.set()
            self.stuck = True
            STUCK.append(os.environ.get("PYTEST_CURRENT_TEST", "an earlier test"))
            pytest.fail("a thread did not finish in %d s; the rest of this module is not run" % JOIN_SECONDS)
        if self.errors:
            raise self.errors[0]
        assert self.first_done is not None and self.last_begin is not None
        return sum(1 for a, b in self.calls if a > self.first_done and b < self.last_begin)


def _side_threads(race, rec):
    """The stager and the second handle (owned by the race, which closes it)."""
    al, s0, s1 = synth.key_seeds(64, STAGE_LOGN, first=7000)
    sk, _ = dpf.gen_batch_seeded(al, STAGE_LOGN, s0, s1)
    sfull = oracle.evalfull_batch(sk, STAGE_LOGN, nthreads=8)
    sxs = synth.eval_points(64, STAGE_PPK, STAGE_LOGN)
    sbits = oracle.eval_batch(sk, sxs, STAGE_LOGN, nthreads=8)

    def stage(i):
        n = STAGE_CYCLE[i % len(STAGE_CYCLE)]
        got = dpf.evalfull_batch(sk[:n], STAGE_LOGN, ngpus=1)
        assert np.array_equal(got, sfull[:n]), ("evalfull_batch beside a PIR handle", n, i)
        got = dpf.eval_batch(sk[:n], sxs[:n], STAGE_LOGN, ngpus=1)
        assert np.array_equal(got, sbits[:n]), ("eval_batch beside a PIR handle", n, i)
    race.looping(stage)

    orec = OTHER_REC[rec]
    odb = np.random.default_rng(rec + 77).integers(0, 256, (NREC, orec), dtype=np.uint8)
    oka, _ = _pairs(np.random.default_rng(rec + 78).integers(0, NREC, 8), first=8000)
    owant = ref.xor_fold(oracle.evalfull_batch(oka, LOGN, nthreads=8), odb, NREC)
    other = race.own(dpf.PirDB(odb, LOGN, rec_bytes=orec))

    def answer_other(i):
        assert np.array_equal(other.answer(oka), owant), ("the second handle's answers", i)
    race.looping(answer_other)


def _case(rec):
    """D0, D1 (different in every record), the probes' alphas and key pairs."""
    rng = np.random.default_rng(rec)
    d0 = rng.integers(0, 256, (NREC, rec), dtype=np.uint8)
    flip = rng.integers(0, 256, (NREC, rec), dtype=np.uint8)
    flip[:, 0] |= 1
    d1 = d0 ^ flip
    alphas = np.concatenate([[0, NREC - 1], rng.choice(np.arange(1, NREC - 1), NPROBE - 2, replace=False)])
    alphas = alphas.astype(np.uint64)
    ka, kb = _pairs(alphas, first=6000 + rec)
    return d0, d1, alphas, ka, kb


def _probe(pdb, both):
    ans = pdb.answer(both)
    return ans[:NPROBE] ^ ans[NPROBE:]


@pytest.mark.parametrize("rec", [32, 20])      # (300 pitched uploads of 3000 rows at width 7 take 7 s)
def test_update_against_answer(rec):
    d0, d1, alphas, ka, kb = _case(rec)
    both = np.concatenate([ka, kb])
    ix = alphas.astype(np.int64)
    states = (d0[ix], d1[ix])
    perm = np.random.default_rng(rec + 1).permutation(NREC).astype(np.uint64)
    new = (np.ascontiguousarray(d0[perm.astype(np.int64)]), np.ascontiguousarray(d1[perm.astype(np.int64)]))
    everything = np.arange(NREC, dtype=np.uint64)

    def one_state(x, what, i):
        assert any(np.array_equal(x, s) for s in states), \
            (what, "call", i, "a torn DB: probes equal to D0 / D1:",
             [int(np.array_equal(x[j], d0[ix[j]])) for j in range(NPROBE)],
             [int(np.array_equal(x[j], d1[ix[j]])) for j in range(NPROBE)])

    race = Race()
    try:
        pdb = race.own(dpf.PirDB(d0, LOGN, rec_bytes=rec))
        _side_threads(race, rec)
        race.looping(lambda i: one_state(race.timed(_probe, pdb, both), "answer", i))

        def answer_and_read(i):
            one_state(race.timed(_probe, pdb, both), "answer", i)
            one_state(pdb.read(alphas), "read", i)
        race.looping(answer_and_read)
        race.writer(lambda i: pdb.update(perm, new[(i + 1) % 2]), WRITER_CALLS)
        overlap = race.run()
        print("update against answer, rec %d: %d reader calls, %d between the writer's first and last call"
              % (rec, len(race.calls), overlap))
        assert np.array_equal(pdb.read(everything), d0)          # 300 flips: back at D0
    finally:
        race.close()
    assert overlap >= 1, "no reader call overlapped the writer: the run proves nothing"


@pytest.mark.parametrize("rec", [32, 20, 7])
def test_write_against_answer(rec):
    d0, _, alphas, ka, kb = _case(rec)
    both = np.concatenate([ka, kb])
    ix = alphas.astype(np.int64)
    j = 5                                                        # the probe whose record the writer flips
    m = np.random.default_rng(rec + 2).integers(1, 256, rec, dtype=np.uint8)
    wkeys = np.stack([ka[j], kb[j]])
    wmsgs = np.stack([m, m])
    base = d0[ix]
    flipped = base.copy()
    flipped[j] ^= m
    everything = np.arange(NREC, dtype=np.uint64)

    def one_state(x, what, i):
        # One key applied without the other shows as pseudorandom garbage at every probe.
        assert np.array_equal(x, base) or np.array_equal(x, flipped), \
            (what, "call", i, "probes equal to D0:", [int(np.array_equal(x[q], base[q])) for q in range(NPROBE)],
             "target equal to D0[j] ^ m:", bool(np.array_equal(x[j], flipped[j])))

    race = Race()
    try:
        pdb = race.own(dpf.PirDB(d0, LOGN, rec_bytes=rec))
        _side_threads(race, rec)
        race.looping(lambda i: one_state(race.timed(_probe, pdb, both), "answer", i))

        def answer_and_read(i):
            one_state(race.timed(_probe, pdb, both), "answer", i)
            one_state(pdb.read(alphas), "read", i)
        race.looping(answer_and_read)
        race.writer(lambda i: pdb.write(wkeys, wmsgs), WRITER_CALLS)
        overlap = race.run()
        print("write against answer, rec %d: %d reader calls, %d between the writer's first and last call"
              % (rec, len(race.calls), overlap))
        assert np.array_equal(pdb.read(everything), d0)          # an even number of flips
    finally:
        race.close()
    assert overlap >= 1, "no reader call overlapped the writer: the run proves nothing"
