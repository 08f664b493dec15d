"""The stream contract of the whole-DB read-out's device entry points
(dpf_pir_db_unslice_any_dev, dpf_pir_db_unslice_grouped_dev,
dpf_pir_db_xor_sliced_dev), held by the protocol of
tests/test_gpu_stream_capture.py on a side stream: eager, then captured
(nothing executes: outputs still poison, a buffer changed in place still in its
initial state), then replayed over a second input set and over the first
again.  One linear graph per case.  Sliced inputs and the expected state of the
merge come from the layout's definition in numpy (pir_ref.layout)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "dpf-go_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import dpf                              # noqa: E402
import pir_ref as ref                   # noqa: E402
import test_gpu_stream_capture as cap   # noqa: E402  (Plan and the protocol; its tests are collected from its own file)

pytestmark = pytest.mark.gpu
NREC = cap.NREC                         # 3000: not a multiple of 256


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert dpf.gpu_init(1) >= 1


@pytest.mark.parametrize("rec", [20, 96])
def test_unslice(rec):
    def make():
        dbs = [cap._rand(s, 30, NREC, rec) for s in (0, 1)]
        p = cap.Plan("dpf_pir_db_unslice_any_dev")
        d = p.inp("dbs", *[ref.layout(x) for x in dbs])
        o = p.out("db", *dbs)
        p.run = lambda st: dpf.pir_db_unslice_any_dev(d, NREC, rec, o, stream=st)
        return p
    cap._with_settings(make)


def test_unslice_grouped():
    ng, _, nrec, rec = cap.GROUPED      # a launch per group: groups of 300 records have padding

    def make():
        dbs = [cap._rand(s, 31, ng, nrec, rec) for s in (0, 1)]
        p = cap.Plan("dpf_pir_db_unslice_grouped_dev")
        d = p.inp("dbs", *[ref.layout(ref.grouped_flat(x)) for x in dbs])
        o = p.out("db", *dbs)
        p.run = lambda st: dpf.pir_db_unslice_grouped_dev(d, ng, nrec, rec, o, stream=st)
        return p
    cap._with_settings(make)


def test_xor_sliced():
    rec = 20

    def make():
        mine = [cap._rand(s, 32, NREC, rec) for s in (0, 1)]
        other = [cap._rand(s, 33, NREC, rec) for s in (0, 1)]
        p = cap.Plan("dpf_pir_db_xor_sliced_dev")
        o = p.inp("other", *[ref.layout(x) for x in other])
        d = p.inp("dbs", *[ref.layout(x) for x in mine], want=[ref.layout(mine[s] ^ other[s]) for s in (0, 1)])
        nbytes = p.sets[0]["dbs"].size
        assert nbytes == dpf.pir_db_sliced_size_any(NREC, rec)
        p.run = lambda st: dpf.pir_db_xor_sliced_dev(d, o, nbytes, stream=st)
        return p
    cap._with_settings(make)
