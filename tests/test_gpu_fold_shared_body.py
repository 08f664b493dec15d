"""Every dense instantiation of the matrix-core fold, once: k_fold_mfma is
compiled per tile shape (dpfh::kFoldTiles, 7), FULL (whole 32-byte columns or
not) and NTDB (nontemporal DB loads), 28 kernels that all run the one loop of
csrc/fold_mfma_body.inc.  Nontemporal loads start at 256 MiB of DB, so no small
test reached half of them; here the cases run once with default loads and once
in a child process with DPF_FOLD_NT_MIN=1 (the knob is read once per process).

A case is (keys, rec_bytes): xor_fold_sliced_any_dev against the numpy fold of
tests/pir_ref.py, bit-exact, at two sizes.  nrec = 2873 is 12 super-groups with
a partial last one, and max_blocks = 1 makes one workgroup walk the whole run:
the paired block loop, the clamped prefetch and selection rows that end inside
the last super-group (92 words of its 96).  Twelve super-groups are 3 staged
blocks of the SG = 4 shapes (2, 5, 6: a pair and the odd tail block) but 6 of
the SG = 2 shapes (0, 1, 3, 4: pairs only), so every case also runs at
nrec = 3100, 13 super-groups: 7 blocks for SG = 2, the last one the odd tail
block and half filled, and 4 for SG = 4 with one super-group in the last.

The grouped kernels' instantiations are covered by
test_gpu_pir_grouped_manykeys.py::test_the_cases_cover_every_axis_and_pair."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "dpf-go_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import dpf                  # noqa: E402
import pir_ref              # noqa: E402

pytestmark = pytest.mark.gpu

NRECS = (2873, 3100)
# (keys, rec_bytes FULL, rec_bytes not FULL, tile shape)
SHAPES = [(5, 128, 100, 0), (5, 64, 36, 1), (5, 32, 20, 2), (40, 32, 20, 3), (100, 64, 36, 4), (100, 32, 20, 5),
          (200, 32, 20, 6)]
CASES = [(nk, rec) for nk, full, part, _ in SHAPES for rec in (full, part)]
FOLD_TILE_COUNT = 7         # dpfh::kFoldTileCount


def fold_tile_index(nk, rec):
    """dpfh::fold_cg (the largest of 4, 2, 1 that divides the columns) and dpfh::fold_tile_index, restated."""
    C = (rec + 31) // 32
    cg = 4 if C % 4 == 0 else 2 if C % 2 == 0 else 1
    if nk <= 32:
        return 0 if cg == 4 else 1 if cg == 2 else 2
    if nk <= 64:
        return 3
    if nk <= 128:
        return 4 if cg >= 2 else 5
    return 6


def test_the_cases_cover_every_tile_shape_full_and_not():
    assert len(CASES) == 14
    for nk, full, part, shape in SHAPES:
        assert full % 32 == 0 and part % 32 != 0 and part % 4 == 0
        assert fold_tile_index(nk, full) == fold_tile_index(nk, part) == shape
    assert sorted(s[3] for s in SHAPES) == list(range(FOLD_TILE_COUNT))


@pytest.fixture
def fold_limits():
    yield dpf.set_fold_limits
    dpf.set_fold_limits(0, 0)


def _fold_matches(nk, rec, NREC):
    """True if the case's answers are the numpy fold's (the caller has set max_blocks = 1)."""
    import torch
    STRIDE = ((NREC + 7) // 8 + 15) // 16 * 16
    rng = np.random.default_rng(1000 * nk + rec + NREC)
    bits = rng.integers(0, 256, (nk, STRIDE), dtype=np.uint8)
    db = rng.integers(0, 256, (NREC, rec), dtype=np.uint8)
    d_dbs = torch.empty(dpf.pir_db_sliced_size_any(NREC, rec), dtype=torch.uint8, device="cuda")
    dpf.pir_db_slice_any_dev(torch.from_numpy(db.reshape(-1)).cuda(), NREC, rec, d_dbs)
    d_ans = torch.full((nk * rec,), 0xAB, dtype=torch.uint8, device="cuda")
    d_work = torch.empty(dpf.xor_fold_workspace_size(), dtype=torch.uint8, device="cuda")
    dpf.xor_fold_sliced_any_dev(torch.from_numpy(bits.reshape(-1)).cuda(), STRIDE, nk, d_dbs, NREC, rec, d_ans, d_work)
    torch.cuda.synchronize()
    return np.array_equal(d_ans.cpu().numpy().reshape(nk, rec), pir_ref.xor_fold(bits, db, NREC))


@pytest.mark.parametrize("nk,rec", CASES)
def test_dense_fold_default_loads(fold_limits, nk, rec):
    assert dpf.gpu_init(1) >= 1
    fold_limits(1, 0)                                          # one workgroup per launch walks the whole run
    for nrec in NRECS:
        assert _fold_matches(nk, rec, nrec), nrec


def test_dense_fold_nontemporal_loads():
    """All 14 cases at both sizes in one fresh process with DPF_FOLD_NT_MIN=1: every DB takes the NTDB kernels."""
    env = dict(os.environ, DPF_FOLD_NT_MIN="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.split()
    assert lines == ["%d,%d,%d:pass" % (nk, rec, nrec) for nk, rec in CASES for nrec in NRECS] + ["done"], r.stdout[-2000:]


if __name__ == "__main__":
    assert os.environ.get("DPF_FOLD_NT_MIN") == "1"
    assert dpf.gpu_init(1) >= 1
    dpf.set_fold_limits(1, 0)
    bad = 0
    for _nk, _rec in CASES:
        for _nrec in NRECS:
            ok = _fold_matches(_nk, _rec, _nrec)
            bad += not ok
            print("%d,%d,%d:%s" % (_nk, _rec, _nrec, "pass" if ok else "FAIL"), flush=True)
    print("done")
    sys.exit(1 if bad else 0)
