"""The C ABI's argument contract, replayed: tests/golden/capi_contract.json
holds, for every device-resident entry point, every dpf_pir_db_create* form
and every size function, the return code and the dpf_last_error text (or the
size) of some thousands of good and bad calls that are decided before any
device call.  It was recorded from the library before the C ABI was split
into its translation units; tools/capi_contract.py has the matrix and
re-records it (only ever from the commit a refactor starts from).

The replay runs in a fresh child process that sees no GPU, and the child makes
no call unless dpf_gpu_init(0) is DPF_ERR_NODEV there: the device pointers of
the cases are fake addresses, so a check that went missing shows up as a
mismatched code, never as a launch on one of them."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "capi_contract.py")
FIXTURE = os.path.join(ROOT, "tests", "golden", "capi_contract.json")
# An ordinal list that names no device, for every layer that reads one.
NO_GPU = {"HIP_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "", "GPU_DEVICE_ORDINAL": ""}


def test_every_recorded_call_answers_as_recorded():
    r = subprocess.run([sys.executable, TOOL, "--check", FIXTURE], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, **NO_GPU))
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.endswith(" 0 mismatches") and int(last.split()[0]) > 3000, last
