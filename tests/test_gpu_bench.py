"""bench.py as a caller runs it: a plain run times exactly --steps steps and
reports ms_per_step, and --dump-outputs writes what the last timed step left
in its output buffer: checked byte for byte against the oracle's EvalFull
(dpf.go:243-262) of the same seeded keys."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import dpf
from dpf import synth
import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# 70 keys x 1 KiB: dumped whole.  40 keys x 128 KiB = 5 MiB > DUMP_SAMPLE
# bytes: the seeded sample and the per-key sums.
@pytest.mark.parametrize("nkeys,logN", [(70, 13), (40, 20)])
def test_plain_run_dumps_the_last_steps_output(tmp_path, nkeys, logN):
    out = str(tmp_path / "dump")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--spinup", "0", "--nkeys", str(nkeys), "--logN", str(logN), "--dump-outputs", out],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["ms_per_step"] > 0 and d["unit"] == "points/s" and d["higher_is_better"] is True
    assert abs(d["value"] - nkeys * (1 << logN) / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    # a plain run measures nothing beside its steps
    for k in ("cpu_baseline", "workloads", "api", "single_call"):
        assert k not in d
    assert list(d["aes_variants"]) == [d["config"]["aes"]]

    al, s0, s1 = synth.key_seeds(nkeys, logN)
    ka, _ = dpf.gen_batch_seeded(al, logN, s0, s1)
    want = oracle.evalfull_batch(ka, logN, nthreads=4)
    got = np.load(os.path.join(out, "evalfull_out.npy"))
    assert got.dtype == np.float32
    if want.size <= bench.DUMP_SAMPLE:
        assert sorted(os.listdir(out)) == ["evalfull_out.npy"]
        assert np.array_equal(got, want.reshape(-1).astype(np.float32))
    else:
        assert sorted(os.listdir(out)) == ["evalfull_out.npy", "evalfull_out_rowsum.npy"]
        idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, want.size, bench.DUMP_SAMPLE, dtype=np.int64))
        assert np.array_equal(got, want.reshape(-1)[idx].astype(np.float32))
        sums = np.load(os.path.join(out, "evalfull_out_rowsum.npy"))
        assert sums.dtype == np.float64
        assert np.array_equal(sums, want.sum(axis=1, dtype=np.int64).astype(np.float64))
