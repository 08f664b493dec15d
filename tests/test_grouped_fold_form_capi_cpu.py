"""dpf_fold_grouped_form_for: what the grouped fold launches for a shape, without
a device (cus > 0): the header declares it, the library exports it and the
Python table has it; good calls on both routes, the bad-argument cases, env
DPF_GROUP_FOLD_ROUTE in both settings (read at every call), and
dpf_set_fold_limits.  The workspace sizes of the grouped forms do not depend
on the route: the matrix-core grouped fold writes no scratch."""
import ctypes
import os
import re

import pytest

import dpf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, M = dpf.FOLD_GROUPED_DIRECT, dpf.FOLD_GROUPED_MFMA
KNOB = "DPF_GROUP_FOLD_ROUTE"


@pytest.fixture(autouse=True)
def _no_knob(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)


def test_header_declares_and_library_exports_the_query():
    with open(os.path.join(ROOT, "include", "dpf_hip.h")) as f:
        header = f.read()
    assert re.search(r"^int dpf_fold_grouped_form_for\(", header, re.M)
    assert re.search(r"^#define DPF_FOLD_GROUPED_DIRECT 0\b", header, re.M)
    assert re.search(r"^#define DPF_FOLD_GROUPED_MFMA 1\b", header, re.M)
    assert KNOB in header and "launch per 256 keys" in header
    assert "dpf_fold_grouped_form_for" in dpf.SIGNATURES
    assert dpf.lib().dpf_fold_grouped_form_for is not None
    assert callable(dpf.fold_grouped_form_for) and (D, M) == (0, 1)
    # The struct of the header and the ctypes one: the same fields in the same order.
    body = re.search(r"typedef struct dpf_fold_grouped_form \{(.*?)\} dpf_fold_grouped_form;", header, re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|uint64_t)\s+(\w+);", body, re.M)
    want = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
    assert [(n, want[t]) for t, n in fields] == list(dpf.FoldGroupedFormC._fields_)


def test_form_query_is_the_plan():
    # Up to 4 keys a group: the direct route, the grouped fold's plan as it was.
    f = dpf.fold_grouped_form_for(7, 3, 300, 36, cus=256)
    assert f.route == D and f.columns_per_wg == 1 and f.keys_per_tile == 4
    assert f.passes == 2 and f.launches == 2 and f.units == 7 * 2 * f.runs         # widths 2 and 1
    f = dpf.fold_grouped_form_for(100000, 1, 256, 32, cus=256)
    assert f.route == D and f.units == 100000 and f.launches == 1 and f.runs == 1 and not f.atomic
    f = dpf.fold_grouped_form_for(96, 4, 1 << 19, 32, cus=256)
    assert f.route == D and f.passes == 1 and f.runs > 1 and f.atomic
    # From 5: the matrix cores, one pass and one launch per 256 keys of every group.
    f = dpf.fold_grouped_form_for(96, 16, 1 << 19, 32, cus=256)
    assert f.route == M and f.keys_per_tile == 32 and f.columns_per_wg == 1 and f.passes == 1 and f.launches == 1
    assert f.atomic and f.runs * f.sg_per_run >= 2048 > (f.runs - 1) * f.sg_per_run and f.units == 96 * f.runs
    assert f.units % 512 == 0                                                       # whole rounds of 2 workgroups a CU
    f = dpf.fold_grouped_form_for(96, 256, 1 << 19, 32, cus=256)
    assert (f.route, f.keys_per_tile, f.runs, f.sg_per_run, f.units, f.passes) == (M, 256, 8, 256, 768, 1)
    f = dpf.fold_grouped_form_for(2, 260, 5000, 32, cus=256)                        # two key tiles: 256 and 4
    assert f.route == M and f.keys_per_tile == 256 and f.passes == 2 and f.launches == 2
    f = dpf.fold_grouped_form_for(4096, 9, 4096, 128, cus=256)                      # CG 4, groups enough: one run, no clear
    assert (f.route, f.columns_per_wg, f.keys_per_tile, f.runs, f.sg_per_run, f.atomic) == (M, 4, 32, 1, 16, 0)
    assert f.units == 4096 and f.launches == 1 and f.max_blocks == 1 << 20
    f = dpf.fold_grouped_form_for(3, 33, 1000, 64, cus=256)                         # 64-key shape: one column a workgroup
    assert f.route == M and f.keys_per_tile == 64 and f.columns_per_wg == 1 and f.units == 3 * 2 * f.runs
    f = dpf.fold_grouped_form_for(3, 100, 1000, 100, cus=256)                       # 4 columns, the last short: CG 2
    assert f.route == M and f.keys_per_tile == 128 and f.columns_per_wg == 2 and f.units == 3 * 2 * f.runs


def test_bad_arguments_and_nothing_to_do():
    L = dpf.lib()
    c = dpf.FoldGroupedFormC()
    assert L.dpf_fold_grouped_form_for(3, 9, 300, 6, 256, ctypes.byref(c)) == dpf.DPF_ERR_PARAM          # width
    assert L.dpf_fold_grouped_form_for(3, 9, 300, 0, 256, ctypes.byref(c)) == dpf.DPF_ERR_PARAM
    assert L.dpf_fold_grouped_form_for(1 << 31, 2, 300, 32, 256, ctypes.byref(c)) == dpf.DPF_ERR_PARAM   # 2^32 key rows
    assert L.dpf_fold_grouped_form_for(3, 9, 300, 32, 256, None) == dpf.DPF_ERR_PARAM                    # null form
    assert b"form query" in L.dpf_last_error()
    for ng, kpg, nrec in ((0, 9, 300), (3, 0, 300), (3, 9, 0)):
        assert L.dpf_fold_grouped_form_for(ng, kpg, nrec, 32, 256, ctypes.byref(c)) == dpf.DPF_OK
        assert c.launches == 0 and c.units == 0 and c.passes == 0 and not c.atomic, (ng, kpg, nrec)


def test_the_knob_forces_the_route_at_every_call(monkeypatch):
    shape = (65, 2, 1000, 32)
    assert dpf.fold_grouped_form_for(*shape, cus=256).route == D
    monkeypatch.setenv(KNOB, "mfma")
    f = dpf.fold_grouped_form_for(*shape, cus=256)
    assert f.route == M and f.keys_per_tile == 32 and f.passes == 1
    assert dpf.fold_grouped_form_for(96, 16, 1 << 19, 32, cus=256).route == M
    monkeypatch.setenv(KNOB, "direct")
    f = dpf.fold_grouped_form_for(96, 16, 1 << 19, 32, cus=256)
    assert f.route == D and f.keys_per_tile == 4 and f.passes == 4 and f.launches == 4
    assert dpf.fold_grouped_form_for(*shape, cus=256).route == D
    monkeypatch.delenv(KNOB)
    assert dpf.fold_grouped_form_for(96, 16, 1 << 19, 32, cus=256).route == M


def test_the_fold_limits_apply():
    try:
        dpf.set_fold_limits(7, 0)
        f = dpf.fold_grouped_form_for(65, 9, 5000, 32, cus=256)
        assert f.route == M and f.max_blocks == 7 and f.launches == (f.units + 6) // 7
        dpf.set_fold_limits(0, 1)                     # below a staged block: runs of one super-group
        f = dpf.fold_grouped_form_for(3000, 9, 5000, 32, cus=256)
        assert f.route == M and (f.sg_per_run, f.runs, f.units, f.atomic) == (1, 20, 60000, 1) and f.launches == 1
        dpf.set_fold_limits(0, 8)
        f = dpf.fold_grouped_form_for(3000, 9, 5000, 32, cus=256)
        assert (f.sg_per_run, f.runs) == (8, 3)
        dpf.set_fold_limits(2, 0)
        f = dpf.fold_grouped_form_for(3, 2, 1000, 32, cus=256)
        assert f.route == D and f.max_blocks == 2 and f.launches == (f.units + 1) // 2
    finally:
        dpf.set_fold_limits(0, 0)


def test_workspace_sizes_do_not_depend_on_the_route(monkeypatch):
    sizes = []
    for knob in (None, "direct", "mfma"):
        if knob:
            monkeypatch.setenv(KNOB, knob)
        sizes.append((dpf.xor_fold_grouped_workspace_size(96, 64, 32), dpf.pir_grouped_workspace_size(96, 64, 12, 32),
                      dpf.pir_grouped_sparse_workspace_size(96, 64, 4096, 40, 32)))
    assert sizes[0] == sizes[1] == sizes[2] and all(s > 0 for s in sizes[0])
    assert dpf.xor_fold_grouped_workspace_size(96, 64, 32) == dpf.xor_fold_grouped_workspace_size(3, 2, 20)
