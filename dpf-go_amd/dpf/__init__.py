"""dpf — Python mirror of dkales/dpf-go's package ``dpf`` over libdpf_hip.so.

Same names, argument meaning and error behaviour as the Go API
(/root/reference/dpf/dpf.go):

    Gen(alpha, logN)   -> (ka, kb)     dpf.go:71   (host; seeds from getrandom)
    Eval(k, x, logN)   -> 0 | 1        dpf.go:171  (gfx950 kernel)
    EvalFull(k, logN)  -> bytes        dpf.go:243  (gfx950 kernel)

Where Go panics, these raise ``DPFPanic`` ("dpf: invalid parameters" for Gen,
dpf.go:72-74).  Batched and device-resident forms are added for the engine.

There is no CPU evaluation path: the HIP library must be built
(``make -C dpf-go_amd``) and a gfx950 device must be visible, otherwise
evaluation raises.
"""
from __future__ import annotations

import collections
import ctypes
import os
from typing import Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DPF_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libdpf_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "dpf_hip.h")

DPF_OK = 0
DPF_ERR_PARAM = -1
DPF_ERR_KEYLEN = -2
DPF_ERR_NODEV = -3
DPF_ERR_HIP = -4
DPF_ERR_NOMEM = -5
AES_TTABLE = 0
AES_BITSLICED = 1


class DPFPanic(RuntimeError):
    """Raised where the Go reference panics (or the device path fails)."""

    def __init__(self, code: int, msg: str):
        super().__init__(msg or f"dpf: error {code}")
        self.code = code


_u8p = ctypes.POINTER(ctypes.c_uint8)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_sz = ctypes.c_size_t
_u32 = ctypes.c_uint32
_u64 = ctypes.c_uint64
_int = ctypes.c_int
_vp = ctypes.c_void_p


class TreeFormC(ctypes.Structure):
    """dpf_tree_form (include/dpf_hip.h)."""
    _fields_ = [("d", _u32), ("block", _u32), ("w", _u32), ("ltop", _u32), ("units_log", _u32), ("walk", _u32),
                ("l1", _u32), ("uniform", ctypes.c_uint8), ("nodes", ctypes.c_uint8), ("raw", ctypes.c_uint8),
                ("cw_lds", ctypes.c_uint8), ("feedback", ctypes.c_uint8), ("prio_small", ctypes.c_uint8),
                ("pad_", ctypes.c_uint8 * 2), ("nunits", _u64), ("grid", _u64), ("sub_base", _u64)]


class EvalFormC(ctypes.Structure):
    """dpf_eval_form (include/dpf_hip.h)."""
    _fields_ = [("level", _u32), ("kernel", _u32), ("block", _u32), ("cw_staged", ctypes.c_uint8),
                ("ragged", ctypes.c_uint8), ("pad_", ctypes.c_uint8 * 2), ("grid", _u64), ("nodes", TreeFormC)]


class ScatterGroupedFormC(ctypes.Structure):
    """dpf_scatter_grouped_form (include/dpf_hip.h)."""
    _fields_ = [("route", _u32), ("columns", _u32), ("pass_widths", _u32), ("pad_", _u32), ("runs", _u64),
                ("sg_per_run", _u64), ("units", _u64), ("max_blocks", _u64), ("passes", _u64), ("launches", _u64)]


class FoldGroupedFormC(ctypes.Structure):
    """dpf_fold_grouped_form (include/dpf_hip.h)."""
    _fields_ = [("route", _u32), ("columns_per_wg", _u32), ("keys_per_tile", _u32), ("atomic", _u32), ("runs", _u64),
                ("sg_per_run", _u64), ("units", _u64), ("passes", _u64), ("launches", _u64), ("max_blocks", _u64)]


class WindowFormC(ctypes.Structure):
    """dpf_window_form (include/dpf_hip.h)."""
    _fields_ = [("route", _u32), ("prefix_bits", _u32), ("first_prefix", _u64), ("npieces", _u64), ("piece_bytes", _u64),
                ("row_bytes", _u64), ("row_offset", _u64), ("sub_key_len", _u64)]


# name -> (restype, argtypes); must cover every function in include/dpf_hip.h
SIGNATURES = {
    "dpf_tree_form_for": (_int, [_sz, _u32, _u32, _u32, _int, ctypes.POINTER(TreeFormC)]),
    "dpf_eval_form_for": (_int, [_sz, _sz, _u32, _sz, _int, _int, ctypes.POINTER(EvalFormC)]),
    "dpf_last_error": (ctypes.c_char_p, []),
    "dpf_key_len": (_sz, [_u32]),
    "dpf_evalfull_len": (_sz, [_u32]),
    "dpf_workspace_size": (_sz, [_sz, _u32]),
    "dpf_gpu_init": (_int, [_int]),
    "dpf_gpu_init_devices": (_int, [ctypes.POINTER(_int), _int]),
    "dpf_gpu_shutdown": (None, []),
    "dpf_gpu_count": (_int, []),
    "dpf_gen_seeded": (_int, [_u64, _u32, _u8p, _u8p, _u8p, _u8p]),
    "dpf_gen": (_int, [_u64, _u32, _u8p, _u8p]),
    "dpf_gen_batch_seeded": (_int, [_u64p, _u32, _u8p, _u8p, _sz, _u8p, _u8p, _int]),
    "dpf_keys_pack": (_int, [ctypes.POINTER(_vp), ctypes.POINTER(_sz), _sz, _sz, _u8p]),
    "dpf_keys_unpack": (_int, [_u8p, _sz, _sz, ctypes.POINTER(_vp)]),
    "dpf_eval": (_int, [_u8p, _sz, _u64, _u32, _u8p]),
    "dpf_evalfull": (_int, [_u8p, _sz, _u32, _u8p]),
    "dpf_evalfull_batch": (_int, [_u8p, _sz, _sz, _u32, _u8p, _int]),
    "dpf_eval_batch": (_int, [_u8p, _sz, _sz, _u64p, _sz, _u32, _u8p, _int]),
    "dpf_evalfull_split": (_int, [_u8p, _sz, _u32, _u8p, _int]),
    "dpf_evalfull_batch_dev": (_int, [_int, _vp, _sz, _sz, _u32, _vp, _vp, _vp]),
    "dpf_evalfull_subtree_dev": (_int, [_int, _vp, _sz, _sz, _u32, _u32, _u64, _vp, _vp, _vp]),
    "dpf_eval_workspace_size": (_sz, [_sz, _sz, _u32]),
    "dpf_eval_frontier_level": (_u32, [_u32, _sz]),
    "dpf_eval_batch_dev": (_int, [_int, _vp, _sz, _sz, _vp, _sz, _u32, _vp, _vp, _sz, _vp]),
    "dpf_eval_bits_stride": (_sz, [_sz]),
    "dpf_eval_bits_workspace_size": (_sz, [_sz, _sz, _u32]),
    "dpf_eval_bits_dev": (_int, [_int, _vp, _sz, _sz, _vp, _sz, _u32, _vp, _sz, _vp, _sz, _vp]),
    "dpf_pir_sparse_workspace_size": (_sz, [_sz, _u64, _u32]),
    "dpf_pir_answer_sparse_dev": (_int, [_int, _vp, _sz, _sz, _u32, _vp, _vp, _u64, _sz, _vp, _vp, _vp]),
    "dpf_pir_write_sparse_dev": (_int, [_int, _vp, _sz, _sz, _u32, _vp, _vp, _vp, _u64, _sz, _vp, _vp]),
    "dpf_pir_db_create_sparse": (_int, [_u64p, _u8p, _u64, _sz, _u32, _int, ctypes.POINTER(_vp)]),
    "dpf_window_form_for": (_int, [_u32, _u64, _u64, _sz, ctypes.POINTER(WindowFormC)]),
    "dpf_subkeys_dev": (_int, [_int, _vp, _sz, _sz, _u32, _u32, _u64, _u64, _vp, _vp]),
    "dpf_evalfull_window_workspace_size": (_sz, [_sz, _u32, _u64, _u64]),
    "dpf_evalfull_window_dev": (_int, [_int, _vp, _sz, _sz, _u32, _u64, _u64, _vp, _sz, _vp, _vp]),
    "dpf_pir_window_workspace_size": (_sz, [_sz, _u32, _u64, _u64, _sz]),
    "dpf_pir_answer_window_dev": (_int, [_int, _vp, _sz, _sz, _u32, _u64, _vp, _u64, _sz, _vp, _vp, _vp]),
    "dpf_pir_write_window_dev": (_int, [_int, _vp, _sz, _sz, _u32, _u64, _vp, _vp, _u64, _sz, _vp, _vp]),
    "dpf_pir_db_create_ranged": (_int, [_u8p, _u64, _sz, _u32, _int, ctypes.POINTER(_vp)]),
    "dpf_pir_group_stride": (_u64, [_u64]),
    "dpf_pir_db_grouped_size": (_sz, [_u64, _u64, _sz]),
    "dpf_pir_db_slice_grouped_dev": (_int, [_int, _vp, _u64, _u64, _sz, _vp, _vp]),
    "dpf_xor_fold_grouped_workspace_size": (_sz, [_u64, _u64, _sz]),
    "dpf_xor_fold_grouped_dev": (_int, [_int, _vp, _sz, _u64, _u64, _vp, _u64, _sz, _vp, _vp, _vp]),
    "dpf_pir_grouped_workspace_size": (_sz, [_u64, _u64, _u32, _sz]),
    "dpf_pir_answer_grouped_dev": (_int, [_int, _vp, _sz, _u64, _u64, _u32, _vp, _u64, _sz, _vp, _vp, _vp]),
    "dpf_pir_db_create_grouped": (_int, [_u8p, _u64, _u64, _sz, _u32, _int, ctypes.POINTER(_vp)]),
    "dpf_pir_db_ngroups": (_u64, [_vp]),
    "dpf_xor_scatter_grouped_dev": (_int, [_int, _vp, _sz, _u64, _u64, _vp, _vp, _u64, _sz, _vp]),
    "dpf_pir_write_grouped_dev": (_int, [_int, _vp, _sz, _u64, _u64, _u32, _vp, _vp, _u64, _sz, _vp, _vp]),
    "dpf_pir_db_write_grouped": (_int, [_vp, _u8p, _sz, _sz, _u8p]),
    "dpf_scatter_grouped_form_for": (_int, [_u64, _u64, _u64, _sz, _int, ctypes.POINTER(ScatterGroupedFormC)]),
    "dpf_fold_grouped_form_for": (_int, [_u64, _u64, _u64, _sz, _int, ctypes.POINTER(FoldGroupedFormC)]),
    "dpf_eval_bits_grouped_dev": (_int, [_int, _vp, _sz, _u64, _u64, _vp, _sz, _u32, _vp, _sz, _vp, _sz, _vp]),
    "dpf_pir_grouped_sparse_workspace_size": (_sz, [_u64, _u64, _u64, _u32, _sz]),
    "dpf_pir_answer_grouped_sparse_dev": (_int, [_int, _vp, _sz, _u64, _u64, _u32, _vp, _vp, _u64, _sz, _vp, _vp, _vp]),
    "dpf_pir_write_grouped_sparse_dev": (_int, [_int, _vp, _sz, _u64, _u64, _u32, _vp, _vp, _vp, _u64, _sz, _vp, _vp]),
    "dpf_pir_db_create_grouped_sparse": (_int, [_u64p, _u8p, _u64, _u64, _sz, _u32, _int, ctypes.POINTER(_vp)]),
    "dpf_pir_db_unslice_any_dev": (_int, [_int, _vp, _u64, _sz, _vp, _vp]),
    "dpf_pir_db_unslice_grouped_dev": (_int, [_int, _vp, _u64, _u64, _sz, _vp, _vp]),
    "dpf_pir_db_xor_sliced_dev": (_int, [_int, _vp, _vp, _sz, _vp]),
    "dpf_pir_db_export": (_int, [_vp, _u64, _u64, _u8p]),
    "dpf_pir_db_xor_records": (_int, [_vp, _u64, _u64, _u8p]),
    "dpf_pir_db_clear": (_int, [_vp]),
    "dpf_set_export_limits": (_int, [_sz]),
    "dpf_expand_keys_dev": (_int, [_int, _vp, _sz, _sz, _u32, _vp, _vp]),
    "dpf_evalfull_expanded_dev": (_int, [_int, _vp, _sz, _u32, _u32, _u64, _vp, _vp]),
    "dpf_forget_workspace": (_int, [_vp]),
    "dpf_set_small_call_path": (_int, [_int]),
    "dpf_get_small_call_path": (_int, []),
    "dpf_small_call_max_logN": (ctypes.c_uint32, []),
    "dpf_set_aes_impl": (_int, [_int]),
    "dpf_get_aes_impl": (_int, []),
    "dpf_set_eval_kernel": (_int, [_int]),
    "dpf_get_eval_kernel": (_int, []),
    "dpf_set_pir_kernel": (_int, [_int]),
    "dpf_get_pir_kernel": (_int, []),
    "dpf_pir_kernel_for": (_int, [_sz, _u32, _u32]),
    "dpf_aes_mmo_dev": (_int, [_int, _int, _int, _vp, _vp, _sz, _u32, _vp]),
    "dpf_xor_fold_workspace_size": (_sz, []),
    "dpf_xor_fold_dev": (_int, [_int, _vp, _sz, _sz, _vp, _u64, _sz, _vp, _vp, _vp]),
    "dpf_pir_workspace_size": (_sz, [_sz, _u32, _u32]),
    "dpf_pir_answer_dev": (_int, [_int, _vp, _sz, _sz, _u32, _u32, _u64, _vp, _u64, _vp, _vp, _vp]),
    "dpf_pir_db_sliced_size": (_sz, [_u64]),
    "dpf_pir_db_slice_dev": (_int, [_int, _vp, _u64, _vp, _vp]),
    "dpf_pir_answer_sliced_dev": (_int, [_int, _vp, _sz, _sz, _u32, _u32, _u64, _vp, _u64, _vp, _vp, _vp]),
    "dpf_xor_fold_sliced_dev": (_int, [_int, _vp, _sz, _sz, _vp, _u64, _vp, _vp, _vp]),
    "dpf_set_fold_limits": (_int, [_u32, _u32]),
    "dpf_pir_db_sliced_size_wide": (_sz, [_u64, _sz]),
    "dpf_pir_db_slice_wide_dev": (_int, [_int, _vp, _u64, _sz, _vp, _vp]),
    "dpf_xor_fold_sliced_wide_dev": (_int, [_int, _vp, _sz, _sz, _vp, _u64, _sz, _vp, _vp, _vp]),
    "dpf_pir_answer_sliced_wide_dev": (_int, [_int, _vp, _sz, _sz, _u32, _u32, _u64, _vp, _u64, _sz, _vp, _vp, _vp]),
    "dpf_pir_answer_wide_dev": (_int, [_int, _vp, _sz, _sz, _u32, _u32, _u64, _vp, _u64, _sz, _vp, _vp, _vp]),
    "dpf_pir_db_update_sliced_wide_dev": (_int, [_int, _vp, _u64, _sz, _vp, _vp, _sz, _vp]),
    "dpf_pir_db_gather_sliced_wide_dev": (_int, [_int, _vp, _u64, _sz, _vp, _sz, _vp, _vp]),
    "dpf_xor_scatter_dev": (_int, [_int, _vp, _sz, _sz, _vp, _vp, _u64, _sz, _vp]),
    "dpf_xor_scatter_sliced_wide_dev": (_int, [_int, _vp, _sz, _sz, _vp, _vp, _u64, _sz, _vp]),
    "dpf_pir_write_wide_dev": (_int, [_int, _vp, _sz, _sz, _u32, _u32, _u64, _vp, _vp, _u64, _sz, _vp, _vp]),
    "dpf_pir_write_sliced_wide_dev": (_int, [_int, _vp, _sz, _sz, _u32, _u32, _u64, _vp, _vp, _u64, _sz, _vp, _vp]),
    "dpf_pir_db_write": (_int, [_vp, _u8p, _sz, _sz, _u8p]),
    "dpf_pir_db_create_wide": (_int, [_u8p, _u64, _sz, _u32, _int, ctypes.POINTER(_vp)]),
    "dpf_pir_db_rec_bytes": (_sz, [_vp]),
    "dpf_pir_db_sliced_size_any": (_sz, [_u64, _sz]),
    "dpf_pir_db_slice_any_dev": (_int, [_int, _vp, _u64, _sz, _vp, _vp]),
    "dpf_xor_fold_sliced_any_dev": (_int, [_int, _vp, _sz, _sz, _vp, _u64, _sz, _vp, _vp, _vp]),
    "dpf_pir_answer_sliced_any_dev": (_int, [_int, _vp, _sz, _sz, _u32, _u32, _u64, _vp, _u64, _sz, _vp, _vp, _vp]),
    "dpf_pir_db_update_sliced_any_dev": (_int, [_int, _vp, _u64, _sz, _vp, _vp, _sz, _vp]),
    "dpf_pir_db_gather_sliced_any_dev": (_int, [_int, _vp, _u64, _sz, _vp, _sz, _vp, _vp]),
    "dpf_xor_scatter_sliced_any_dev": (_int, [_int, _vp, _sz, _sz, _vp, _vp, _u64, _sz, _vp]),
    "dpf_pir_write_sliced_any_dev": (_int, [_int, _vp, _sz, _sz, _u32, _u32, _u64, _vp, _vp, _u64, _sz, _vp, _vp]),
    "dpf_pir_db_create_any": (_int, [_u8p, _u64, _sz, _u32, _int, ctypes.POINTER(_vp)]),
    "dpf_pir_db_nrec": (_u64, [_vp]),
    "dpf_pir_db_update": (_int, [_vp, _u64p, _u8p, _sz]),
    "dpf_pir_db_read": (_int, [_vp, _u64p, _sz, _u8p]),
    "dpf_pir_db_create": (_int, [_u8p, _u64, _u32, _int, ctypes.POINTER(_vp)]),
    "dpf_pir_answer": (_int, [_vp, _u8p, _sz, _sz, _u8p]),
    "dpf_pir_db_free": (None, [_vp]),
    "dpf_stream_create_cu_masked": (_int, [_int, _u32, _u32, ctypes.POINTER(_vp)]),
    "dpf_stream_destroy": (_int, [_vp]),
}

_lib: Optional[ctypes.CDLL] = None


def lib() -> ctypes.CDLL:
    """Load libdpf_hip.so (raises if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} missing: build it with `make -C dpf-go_amd` (no CPU fallback exists)")
        # One HIP runtime per process: torch ships its own libamdhip64.so
        # (DT_NEEDED "libamdhip64.so"), ours resolves "libamdhip64.so.7".
        # Loading torch first makes both bind to torch's copy, so device
        # pointers and streams handed over from torch are valid here.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def _check(rc: int) -> None:
    if rc != DPF_OK:
        msg = lib().dpf_last_error().decode(errors="replace")
        raise DPFPanic(rc, msg)


def _buf(a: np.ndarray):
    return a.ctypes.data_as(_u8p)


def _as_u8(b) -> np.ndarray:
    if isinstance(b, np.ndarray):
        return np.ascontiguousarray(b, dtype=np.uint8)
    return np.frombuffer(bytes(b), dtype=np.uint8)


def key_len(logN: int) -> int:
    return int(lib().dpf_key_len(logN))


def evalfull_len(logN: int) -> int:
    return int(lib().dpf_evalfull_len(logN))


def workspace_size(nkeys: int, logN: int) -> int:
    return int(lib().dpf_workspace_size(nkeys, logN))


def gpu_init(ngpus: int = 0) -> int:
    rc = lib().dpf_gpu_init(ngpus)
    if rc < 0:
        _check(rc)
    return rc


def gpu_init_devices(ordinals: Sequence[int]) -> int:
    """Open exactly these HIP ordinals (one process per GPU: its own only)."""
    ids = (_int * len(ordinals))(*ordinals)
    rc = lib().dpf_gpu_init_devices(ids, len(ordinals))
    if rc < 0:
        _check(rc)
    return rc


def gpu_shutdown() -> None:
    lib().dpf_gpu_shutdown()


def gpu_count() -> int:
    """Devices the library has open (dpf_gpu_count)."""
    return int(lib().dpf_gpu_count())


# ------------------------------------------------------- key wire format ---
def keys_pack(keys: Sequence[bytes], key_len: Optional[int] = None) -> np.ndarray:
    """[DPFkey, ...] -> uint8[n, key_len], the batch layout of every batched
    entry point (dpf_keys_pack).  Keys are the reference's bytes (dpf.go:7);
    all must have the same length (DPFPanic DPF_ERR_KEYLEN otherwise)."""
    bufs = [_as_u8(k) for k in keys]
    n = len(bufs)
    kl = key_len if key_len is not None else (bufs[0].size if n else 0)
    out = np.empty((n, kl), np.uint8)
    if n == 0:
        return out
    ptrs = (_vp * n)(*[b.ctypes.data for b in bufs])
    lens = (_sz * n)(*[b.size for b in bufs])
    _check(lib().dpf_keys_pack(ptrs, lens, n, kl, _buf(out)))
    return out


def keys_unpack(packed: np.ndarray) -> list:
    """uint8[n, key_len] -> [DPFkey (bytes), ...] (dpf_keys_unpack)."""
    a = np.ascontiguousarray(packed, dtype=np.uint8)
    n, kl = a.shape
    outs = [np.empty(kl, np.uint8) for _ in range(n)]
    if n:
        ptrs = (_vp * n)(*[o.ctypes.data for o in outs])
        _check(lib().dpf_keys_unpack(_buf(a), kl, n, ptrs))
    return [o.tobytes() for o in outs]


# ------------------------------------------------------------------ Gen ---
def gen_seeded(alpha: int, logN: int, s0: bytes, s1: bytes) -> Tuple[bytes, bytes]:
    """Gen with the two crypto/rand seeds (dpf.go:80-81) supplied."""
    if logN > 63 or logN < 0 or alpha < 0 or alpha >= (1 << logN):
        raise DPFPanic(DPF_ERR_PARAM, "dpf: invalid parameters")
    n = key_len(logN)
    ka = np.zeros(n, np.uint8)
    kb = np.zeros(n, np.uint8)
    _check(lib().dpf_gen_seeded(alpha, logN, _buf(_as_u8(s0)), _buf(_as_u8(s1)), _buf(ka), _buf(kb)))
    return ka.tobytes(), kb.tobytes()


def Gen(alpha: int, logN: int) -> Tuple[bytes, bytes]:
    """dpf.go:71 — two key shares for the point function at alpha."""
    if logN > 63 or logN < 0 or alpha < 0 or alpha >= (1 << logN):
        raise DPFPanic(DPF_ERR_PARAM, "dpf: invalid parameters")
    n = key_len(logN)
    ka = np.zeros(n, np.uint8)
    kb = np.zeros(n, np.uint8)
    _check(lib().dpf_gen(alpha, logN, _buf(ka), _buf(kb)))
    return ka.tobytes(), kb.tobytes()


def gen_batch_seeded(alphas: Sequence[int], logN: int, s0s: np.ndarray, s1s: np.ndarray,
                     nthreads: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """Batched seeded Gen on host threads -> (ka[n, klen], kb[n, klen])."""
    al = np.ascontiguousarray(alphas, dtype=np.uint64)
    n = al.shape[0]
    s0 = np.ascontiguousarray(s0s, dtype=np.uint8).reshape(n, 16)
    s1 = np.ascontiguousarray(s1s, dtype=np.uint8).reshape(n, 16)
    kl = key_len(logN)
    ka = np.zeros((n, kl), np.uint8)
    kb = np.zeros((n, kl), np.uint8)
    _check(lib().dpf_gen_batch_seeded(al.ctypes.data_as(_u64p), logN, _buf(s0), _buf(s1), n, _buf(ka), _buf(kb),
                                      nthreads))
    return ka, kb


# ----------------------------------------------------------- evaluation ---
def Eval(k: bytes, x: int, logN: int) -> int:
    """dpf.go:171 — the share of f_alpha(x), 0 or 1.  A latency-bound single
    call: the key bytes go to C without a numpy copy."""
    kb = k if isinstance(k, bytes) else _as_u8(k).tobytes()
    out = ctypes.c_uint8(0)
    rc = _eval_fn()(kb, len(kb), x & 0xFFFFFFFFFFFFFFFF, logN, ctypes.byref(out))
    if rc != DPF_OK:
        _check(rc)
    return out.value


_eval_proto = None


def _eval_fn():
    """dpf_eval with a bytes key argument (c_char_p: no copy)."""
    global _eval_proto
    if _eval_proto is None:
        f = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint32,
                             ctypes.POINTER(ctypes.c_uint8))
        _eval_proto = f(("dpf_eval", lib()))
    return _eval_proto


def EvalFull(key: bytes, logN: int, out: Optional[np.ndarray] = None) -> memoryview:
    """dpf.go:243 — the share of f_alpha over the whole domain, packed bits.

    Returns a writable bytes-like view of a fresh buffer (the Go function
    returns a fresh []byte, dpf.go:251): dpf_evalfull writes every byte of it
    once, with no zero fill before and no copy after.  `out` (uint8,
    evalfull_len(logN) bytes, C-contiguous) reuses a caller buffer instead."""
    if logN > 63:   # the reference panics allocating 2^(logN-3) bytes (dpf.go:251)
        raise DPFPanic(DPF_ERR_PARAM, "dpf: logN > 63")
    kk = _as_u8(key)
    n = evalfull_len(logN)
    if out is None:
        out = np.empty(n, np.uint8)
    assert out.dtype == np.uint8 and out.flags.c_contiguous and out.size == n
    _check(lib().dpf_evalfull(_buf(kk), kk.size, logN, _buf(out)))
    return out.reshape(-1).data


def evalfull_batch(keys: np.ndarray, logN: int, ngpus: int = 0, out: Optional[np.ndarray] = None) -> np.ndarray:
    """keys[n, klen] uint8 -> out[n, evalfull_len(logN)] uint8 (written into `out` when given)."""
    kk = np.ascontiguousarray(keys, dtype=np.uint8)
    n, kl = kk.shape
    if out is None:
        out = np.empty((n, evalfull_len(logN)), np.uint8)
    assert out.dtype == np.uint8 and out.flags.c_contiguous and out.shape == (n, evalfull_len(logN))
    _check(lib().dpf_evalfull_batch(_buf(kk), kl, n, logN, _buf(out), ngpus))
    return out


def eval_batch(keys: np.ndarray, xs: np.ndarray, logN: int, ngpus: int = 0,
               out: Optional[np.ndarray] = None) -> np.ndarray:
    """keys[n, klen], xs[n, p] uint64 -> out[n, p] uint8 (0/1), written into `out` when given."""
    kk = np.ascontiguousarray(keys, dtype=np.uint8)
    x = np.ascontiguousarray(xs, dtype=np.uint64)
    n, kl = kk.shape
    p = x.shape[1]
    if out is None:
        out = np.empty((n, p), np.uint8)
    assert out.dtype == np.uint8 and out.flags.c_contiguous and out.shape == (n, p)
    _check(lib().dpf_eval_batch(_buf(kk), kl, n, x.ctypes.data_as(_u64p), p, logN, _buf(out), ngpus))
    return out


def evalfull_split(key: bytes, logN: int, ngpus: int, out: Optional[np.ndarray] = None) -> np.ndarray:
    """One EvalFull split by top-level subtree over ngpus devices -> uint8
    array of evalfull_len(logN) bytes (written into `out` when given)."""
    kk = _as_u8(key)
    if out is None:
        out = np.empty(evalfull_len(logN), np.uint8)
    assert out.dtype == np.uint8 and out.flags.c_contiguous and out.size == evalfull_len(logN)
    _check(lib().dpf_evalfull_split(_buf(kk), kk.size, logN, _buf(out), ngpus))
    return out


# --------------------------------------------- device-resident (torch) ---
def _ptr(t) -> int:
    return 0 if t is None else int(t.data_ptr())


def _stream_handle(stream) -> int:
    return int(stream.cuda_stream) if stream is not None else 0


def evalfull_batch_dev(d_keys, key_len_: int, nkeys: int, logN: int, d_out, d_work, device: int = 0,
                       stream=None) -> None:
    """Enqueue EvalFull of nkeys HBM-resident keys on `stream` (torch stream)."""
    _check(lib().dpf_evalfull_batch_dev(device, _ptr(d_keys), key_len_, nkeys, logN, _ptr(d_out), _ptr(d_work),
                                        _stream_handle(stream)))


def evalfull_subtree_dev(d_keys, key_len_: int, nkeys: int, logN: int, prefix_bits: int, prefix: int, d_out,
                         d_work, device: int = 0, stream=None) -> None:
    _check(lib().dpf_evalfull_subtree_dev(device, _ptr(d_keys), key_len_, nkeys, logN, prefix_bits, prefix,
                                          _ptr(d_out), _ptr(d_work), _stream_handle(stream)))


def eval_workspace_size(nkeys: int, pts_per_key: int, logN: int) -> int:
    return int(lib().dpf_eval_workspace_size(nkeys, pts_per_key, logN))


def eval_frontier_level(logN: int, pts_per_key: int) -> int:
    """Depth of the shared frontier eval_batch_dev uses with a full workspace (0: root walks)."""
    return int(lib().dpf_eval_frontier_level(logN, pts_per_key))


WALK_NONE, WALK_LANE, WALK_QUAD = 0, 1, 2
EVAL_PERSIST, EVAL_PAIR_UNIFORM, EVAL_PAIR, EVAL_TRIE_KERNEL = 0, 1, 2, 3
TreeForm = collections.namedtuple(
    "TreeForm", "d block w ltop units_log walk l1 uniform nodes raw cw_lds feedback prio_small nunits grid sub_base")
EvalForm = collections.namedtuple("EvalForm", "level kernel block cw_staged ragged grid nodes")


def _tree_form(c: TreeFormC) -> "TreeForm":
    return TreeForm(*[bool(getattr(c, f)) if f in ("uniform", "nodes", "raw", "cw_lds", "feedback", "prio_small")
                      else int(getattr(c, f)) for f in TreeForm._fields])


def tree_form_for(nkeys: int, logN: int, prefix_bits: int = 0, node_level: int = 0, cus: int = 0) -> "TreeForm":
    """The form of the tree kernel (dpf_tree_form_for) that the leaf launch of
    evalfull_subtree_dev(nkeys, logN, prefix_bits) takes (node_level = 0), or
    the node pass down to node_level.  cus <= 0: the current device's / the
    calling thread's stream budget.  Needs no device when cus > 0.  Describes
    the current kernels; not a stable contract."""
    c = TreeFormC()
    _check(lib().dpf_tree_form_for(nkeys, logN, prefix_bits, node_level, cus, ctypes.byref(c)))
    return _tree_form(c)


def eval_form_for(nkeys: int, pts_per_key: int, logN: int, work_bytes: int, xs_aligned16: bool = True,
                  cus: int = 0) -> "EvalForm":
    """What eval_batch_dev runs for this shape, workspace size and xs alignment (dpf_eval_form_for)."""
    c = EvalFormC()
    _check(lib().dpf_eval_form_for(nkeys, pts_per_key, logN, work_bytes, 1 if xs_aligned16 else 0, cus,
                                   ctypes.byref(c)))
    return EvalForm(int(c.level), int(c.kernel), int(c.block), bool(c.cw_staged), bool(c.ragged), int(c.grid),
                    _tree_form(c.nodes) if c.level > 0 else None)


def eval_batch_dev(d_keys, key_len_: int, nkeys: int, d_xs, pts_per_key: int, logN: int, d_out, d_work,
                   device: int = 0, stream=None) -> None:
    """Batched Eval on HBM tensors; d_work's size picks root walks or a shared frontier."""
    nbytes = int(d_work.numel() * d_work.element_size())
    _check(lib().dpf_eval_batch_dev(device, _ptr(d_keys), key_len_, nkeys, _ptr(d_xs), pts_per_key, logN,
                                    _ptr(d_out), _ptr(d_work), nbytes, _stream_handle(stream)))


def eval_bits_stride(npts: int) -> int:
    """Bytes of a bit row eval_bits_dev writes: 16 * ceil(npts / 128)."""
    return int(lib().dpf_eval_bits_stride(npts))


def eval_bits_workspace_size(nkeys: int, npts: int, logN: int) -> int:
    """Expanded keys plus the frontier (eval_workspace_size); nothing that grows as nkeys * npts."""
    return int(lib().dpf_eval_bits_workspace_size(nkeys, npts, logN))


def eval_bits_dev(d_keys, key_len_: int, nkeys: int, d_xs, npts: int, logN: int, d_bits, bits_stride: int, d_work,
                  device: int = 0, stream=None) -> None:
    """Every key at the npts shared points d_xs (uint64), as selection-bit
    rows d_bits[nkeys][bits_stride]: bit j % 8 of byte j / 8 of row k is
    Eval(key_k, d_xs[j]) (dpf_eval_bits_dev).  d_work's size picks root walks
    or a shared frontier, as for eval_batch_dev."""
    nbytes = int(d_work.numel() * d_work.element_size())
    _check(lib().dpf_eval_bits_dev(device, _ptr(d_keys), key_len_, nkeys, _ptr(d_xs), npts, logN, _ptr(d_bits),
                                   bits_stride, _ptr(d_work), nbytes, _stream_handle(stream)))


def eval_bits_grouped_dev(d_keys, key_len_: int, ngroups: int, keys_per_group: int, d_xs, npts: int, logN: int, d_bits,
                          bits_stride: int, d_work, device: int = 0, stream=None) -> None:
    """eval_bits_dev with a point list per group: d_xs is [ngroups][npts]
    uint64, tight, and row g * keys_per_group + k of d_bits holds the bits of
    that key at group g's own points (dpf_eval_bits_grouped_dev).  d_work is
    sized as for eval_bits_dev with ngroups * keys_per_group keys."""
    nbytes = int(d_work.numel() * d_work.element_size())
    _check(lib().dpf_eval_bits_grouped_dev(device, _ptr(d_keys), key_len_, ngroups, keys_per_group, _ptr(d_xs), npts, logN,
                                           _ptr(d_bits), bits_stride, _ptr(d_work), nbytes, _stream_handle(stream)))


def expand_keys_dev(d_keys, key_len_: int, nkeys: int, logN: int, d_work, device: int = 0, stream=None) -> None:
    _check(lib().dpf_expand_keys_dev(device, _ptr(d_keys), key_len_, nkeys, logN, _ptr(d_work),
                                     _stream_handle(stream)))


def evalfull_expanded_dev(d_work, nkeys: int, logN: int, d_out, prefix_bits: int = 0, prefix: int = 0,
                          device: int = 0, stream=None) -> None:
    _check(lib().dpf_evalfull_expanded_dev(device, _ptr(d_work), nkeys, logN, prefix_bits, prefix, _ptr(d_out),
                                           _stream_handle(stream)))


def forget_workspace(d_work) -> None:
    """Drop the library's record of what was expanded into d_work (call before freeing it)."""
    _check(lib().dpf_forget_workspace(_ptr(d_work)))


def set_aes_impl(impl) -> int:
    """Select the tree kernels' AES back end ("ttable"/"bitsliced" or 0/1); returns the previous one."""
    if isinstance(impl, str):
        impl = {"ttable": AES_TTABLE, "lds-ttable": AES_TTABLE, "bitsliced": AES_BITSLICED}[impl]
    rc = lib().dpf_set_aes_impl(impl)
    if rc < 0:
        _check(rc)
    return rc


def get_aes_impl() -> int:
    return int(lib().dpf_get_aes_impl())


EVAL_WALK, EVAL_TRIE = 0, 1


def set_eval_kernel(kernel) -> int:
    """Select the batched Eval kernel ("walk"/"trie" or 0/1); returns the previous one."""
    if isinstance(kernel, str):
        kernel = {"walk": EVAL_WALK, "trie": EVAL_TRIE}[kernel]
    rc = lib().dpf_set_eval_kernel(kernel)
    if rc < 0:
        _check(rc)
    return rc


def get_eval_kernel() -> int:
    return int(lib().dpf_get_eval_kernel())


PIR_SPLIT, PIR_FUSED, PIR_FUSED_ANY = 0, 1, 2


def set_pir_kernel(kernel) -> int:
    """Select the sliced PIR kernel ("split"/"fused"/"fused-any" or 0/1/2); returns the previous one."""
    if isinstance(kernel, str):
        kernel = {"split": PIR_SPLIT, "fused": PIR_FUSED, "fused-any": PIR_FUSED_ANY}[kernel]
    rc = lib().dpf_set_pir_kernel(kernel)
    if rc < 0:
        _check(rc)
    return rc


def get_pir_kernel() -> int:
    return int(lib().dpf_get_pir_kernel())


def pir_kernel_for(nkeys: int, logN: int, prefix_bits: int = 0) -> int:
    """PIR_FUSED or PIR_SPLIT: what pir_answer_sliced_dev runs for this shape now."""
    return int(lib().dpf_pir_kernel_for(nkeys, logN, prefix_bits))


SMALL_AUTO, SMALL_GPU, SMALL_HOST = 0, 1, 2


def set_small_call_path(mode) -> int:
    """Route of the single-key Eval/EvalFull ("auto"/"gpu"/"host" or 0/1/2,
    include/dpf_hip.h); returns the previous mode."""
    if isinstance(mode, str):
        mode = {"auto": SMALL_AUTO, "gpu": SMALL_GPU, "host": SMALL_HOST}[mode]
    rc = lib().dpf_set_small_call_path(mode)
    if rc < 0:
        _check(rc)
    return rc


def get_small_call_path() -> int:
    return int(lib().dpf_get_small_call_path())


def small_call_max_logN() -> int:
    return int(lib().dpf_small_call_max_logN())


def aes_mmo_dev(d_in, d_out, nblocks: int, impl: int = AES_TTABLE, right: bool = False, reps: int = 1,
                device: int = 0, stream=None) -> None:
    """aes128MMO iterated `reps` times over nblocks HBM blocks (both back ends)."""
    _check(lib().dpf_aes_mmo_dev(device, impl, 1 if right else 0, _ptr(d_in), _ptr(d_out), nblocks, reps,
                                 _stream_handle(stream)))


# ------------------------------------------------- CU-partitioned streams ---
def stream_create_cu_masked(cu_first: int, cu_count: int, device: int = 0):
    """A torch stream (ExternalStream) whose kernels run only on CUs
    [cu_first, cu_first + cu_count) of `device`; the _dev entry points size
    their grids to those CUs.  Release with stream_destroy()."""
    import torch
    h = _vp()
    _check(lib().dpf_stream_create_cu_masked(device, cu_first, cu_count, ctypes.byref(h)))
    return torch.cuda.ExternalStream(h.value, device=torch.device("cuda", device))


def stream_destroy(stream) -> None:
    _check(lib().dpf_stream_destroy(_stream_handle(stream)))


# ------------------------------------------------------- streaming fold ---
def xor_fold_workspace_size() -> int:
    return int(lib().dpf_xor_fold_workspace_size())


def xor_fold_dev(d_bits, bits_stride: int, nkeys: int, d_payload, nrec: int, rec_bytes: int, d_ans, d_work,
                 device: int = 0, stream=None) -> None:
    """ans[k] = XOR of payload records i (rec_bytes each) whose bit i is set
    in EvalFull output k, on the device (dpf_xor_fold_dev)."""
    _check(lib().dpf_xor_fold_dev(device, _ptr(d_bits), bits_stride, nkeys, _ptr(d_payload), nrec, rec_bytes,
                                  _ptr(d_ans), _ptr(d_work), _stream_handle(stream)))


# ------------------------------------------------------------------ PIR ---
def pir_workspace_size(nkeys: int, logN: int, prefix_bits: int = 0) -> int:
    return int(lib().dpf_pir_workspace_size(nkeys, logN, prefix_bits))


def pir_answer_dev(d_keys, key_len_: int, nkeys: int, logN: int, d_db, nrec: int, d_ans, d_work,
                   prefix_bits: int = 0, prefix: int = 0, device: int = 0, stream=None) -> None:
    """Server answers (nkeys x 32 B) for the DB slice of subtree (prefix_bits, prefix)."""
    _check(lib().dpf_pir_answer_dev(device, _ptr(d_keys), key_len_, nkeys, logN, prefix_bits, prefix, _ptr(d_db),
                                    nrec, _ptr(d_ans), _ptr(d_work), _stream_handle(stream)))


def pir_db_sliced_size(nrec: int) -> int:
    return int(lib().dpf_pir_db_sliced_size(nrec))


def pir_db_slice_dev(d_db, nrec: int, d_dbs, device: int = 0, stream=None) -> None:
    """Bit-sliced copy of a row-major 32-B-record DB for the MFMA fold (built once per DB)."""
    _check(lib().dpf_pir_db_slice_dev(device, _ptr(d_db), nrec, _ptr(d_dbs), _stream_handle(stream)))


def pir_answer_sliced_dev(d_keys, key_len_: int, nkeys: int, logN: int, d_dbs, nrec: int, d_ans, d_work,
                          prefix_bits: int = 0, prefix: int = 0, device: int = 0, stream=None) -> None:
    """pir_answer_dev over the bit-sliced DB (the matrix-core fold)."""
    _check(lib().dpf_pir_answer_sliced_dev(device, _ptr(d_keys), key_len_, nkeys, logN, prefix_bits, prefix,
                                           _ptr(d_dbs), nrec, _ptr(d_ans), _ptr(d_work), _stream_handle(stream)))


def xor_fold_sliced_dev(d_bits, bits_stride: int, nkeys: int, d_dbs, nrec: int, d_ans, d_work, device: int = 0,
                        stream=None) -> None:
    """xor_fold_dev for 32-B records over the bit-sliced DB (the matrix-core fold)."""
    _check(lib().dpf_xor_fold_sliced_dev(device, _ptr(d_bits), bits_stride, nkeys, _ptr(d_dbs), nrec, _ptr(d_ans),
                                         _ptr(d_work), _stream_handle(stream)))


def pir_db_sliced_size_wide(nrec: int, rec_bytes: int) -> int:
    """Bytes of the wide bit-sliced layout of nrec records of rec_bytes (a multiple of 32)."""
    return int(lib().dpf_pir_db_sliced_size_wide(nrec, rec_bytes))


def pir_db_slice_wide_dev(d_db, nrec: int, rec_bytes: int, d_dbs, device: int = 0, stream=None) -> None:
    """Wide bit-sliced copy dbs[S][c][n][g] of a row-major DB of rec_bytes-byte records."""
    _check(lib().dpf_pir_db_slice_wide_dev(device, _ptr(d_db), nrec, rec_bytes, _ptr(d_dbs), _stream_handle(stream)))


def xor_fold_sliced_wide_dev(d_bits, bits_stride: int, nkeys: int, d_dbs, nrec: int, rec_bytes: int, d_ans, d_work,
                             device: int = 0, stream=None) -> None:
    """xor_fold_dev over the wide bit-sliced DB (the matrix-core fold, any rec_bytes = 32 C)."""
    _check(lib().dpf_xor_fold_sliced_wide_dev(device, _ptr(d_bits), bits_stride, nkeys, _ptr(d_dbs), nrec, rec_bytes,
                                              _ptr(d_ans), _ptr(d_work), _stream_handle(stream)))


def pir_answer_sliced_wide_dev(d_keys, key_len_: int, nkeys: int, logN: int, d_dbs, nrec: int, rec_bytes: int, d_ans,
                               d_work, prefix_bits: int = 0, prefix: int = 0, device: int = 0, stream=None) -> None:
    """Server answers (nkeys x rec_bytes) over the wide bit-sliced DB slice of subtree (prefix_bits, prefix)."""
    _check(lib().dpf_pir_answer_sliced_wide_dev(device, _ptr(d_keys), key_len_, nkeys, logN, prefix_bits, prefix,
                                                _ptr(d_dbs), nrec, rec_bytes, _ptr(d_ans), _ptr(d_work),
                                                _stream_handle(stream)))


def pir_answer_wide_dev(d_keys, key_len_: int, nkeys: int, logN: int, d_db, nrec: int, rec_bytes: int, d_ans, d_work,
                        prefix_bits: int = 0, prefix: int = 0, device: int = 0, stream=None) -> None:
    """pir_answer_dev for rec_bytes-byte records (row-major DB, the LDS fold)."""
    _check(lib().dpf_pir_answer_wide_dev(device, _ptr(d_keys), key_len_, nkeys, logN, prefix_bits, prefix, _ptr(d_db),
                                         nrec, rec_bytes, _ptr(d_ans), _ptr(d_work), _stream_handle(stream)))


def pir_db_update_sliced_wide_dev(d_dbs, nrec: int, rec_bytes: int, d_idx, d_recs, n: int, device: int = 0,
                                  stream=None) -> None:
    """Set record d_idx[i] (uint64, non-decreasing; last of equal ones wins,
    >= nrec skipped) of the wide bit-sliced DB to d_recs[i], in place."""
    _check(lib().dpf_pir_db_update_sliced_wide_dev(device, _ptr(d_dbs), nrec, rec_bytes, _ptr(d_idx), _ptr(d_recs), n,
                                                   _stream_handle(stream)))


def pir_db_gather_sliced_wide_dev(d_dbs, nrec: int, rec_bytes: int, d_idx, n: int, d_out, device: int = 0,
                                  stream=None) -> None:
    """d_out[i] = record d_idx[i] (any order; zeros for >= nrec) of the wide bit-sliced DB, row-major."""
    _check(lib().dpf_pir_db_gather_sliced_wide_dev(device, _ptr(d_dbs), nrec, rec_bytes, _ptr(d_idx), n, _ptr(d_out),
                                                   _stream_handle(stream)))


def xor_scatter_dev(d_bits, bits_stride: int, nkeys: int, d_msgs, d_db, nrec: int, rec_bytes: int, device: int = 0,
                    stream=None) -> None:
    """Row-major DB record i ^= XOR of the messages d_msgs[k] (rec_bytes each)
    whose EvalFull output k has bit i set, i < nrec, in place (dpf_xor_scatter_dev)."""
    _check(lib().dpf_xor_scatter_dev(device, _ptr(d_bits), bits_stride, nkeys, _ptr(d_msgs), _ptr(d_db), nrec,
                                     rec_bytes, _stream_handle(stream)))


def xor_scatter_sliced_wide_dev(d_bits, bits_stride: int, nkeys: int, d_msgs, d_dbs, nrec: int, rec_bytes: int,
                                device: int = 0, stream=None) -> None:
    """xor_scatter_dev over the wide bit-sliced DB (bits past nrec ignored: the padding stays zero)."""
    _check(lib().dpf_xor_scatter_sliced_wide_dev(device, _ptr(d_bits), bits_stride, nkeys, _ptr(d_msgs), _ptr(d_dbs),
                                                 nrec, rec_bytes, _stream_handle(stream)))


def pir_write_wide_dev(d_keys, key_len_: int, nkeys: int, logN: int, d_msgs, d_db, nrec: int, rec_bytes: int, d_work,
                       prefix_bits: int = 0, prefix: int = 0, device: int = 0, stream=None) -> None:
    """Private write into the row-major DB slice of subtree (prefix_bits,
    prefix): the subtree EvalFull of the keys, then xor_scatter_dev of their
    messages (d_work: pir_workspace_size bytes)."""
    _check(lib().dpf_pir_write_wide_dev(device, _ptr(d_keys), key_len_, nkeys, logN, prefix_bits, prefix, _ptr(d_msgs),
                                        _ptr(d_db), nrec, rec_bytes, _ptr(d_work), _stream_handle(stream)))


def pir_write_sliced_wide_dev(d_keys, key_len_: int, nkeys: int, logN: int, d_msgs, d_dbs, nrec: int, rec_bytes: int,
                              d_work, prefix_bits: int = 0, prefix: int = 0, device: int = 0, stream=None) -> None:
    """pir_write_wide_dev over the wide bit-sliced DB slice."""
    _check(lib().dpf_pir_write_sliced_wide_dev(device, _ptr(d_keys), key_len_, nkeys, logN, prefix_bits, prefix,
                                               _ptr(d_msgs), _ptr(d_dbs), nrec, rec_bytes, _ptr(d_work),
                                               _stream_handle(stream)))


# ---- records of any width (a multiple of 4 bytes) over the sliced layout ----
def pir_db_sliced_size_any(nrec: int, rec_bytes: int) -> int:
    """Bytes of the bit-sliced layout of nrec records of rec_bytes (a multiple of 4; 0 for a bad width)."""
    return int(lib().dpf_pir_db_sliced_size_any(nrec, rec_bytes))


def pir_db_slice_any_dev(d_db, nrec: int, rec_bytes: int, d_dbs, device: int = 0, stream=None) -> None:
    """Bit-sliced copy dbs[S][p][g] of a row-major DB of rec_bytes-byte records (any multiple of 4)."""
    _check(lib().dpf_pir_db_slice_any_dev(device, _ptr(d_db), nrec, rec_bytes, _ptr(d_dbs), _stream_handle(stream)))


def xor_fold_sliced_any_dev(d_bits, bits_stride: int, nkeys: int, d_dbs, nrec: int, rec_bytes: int, d_ans, d_work,
                            device: int = 0, stream=None) -> None:
    """xor_fold_sliced_wide_dev for any rec_bytes that is a multiple of 4."""
    _check(lib().dpf_xor_fold_sliced_any_dev(device, _ptr(d_bits), bits_stride, nkeys, _ptr(d_dbs), nrec, rec_bytes,
                                             _ptr(d_ans), _ptr(d_work), _stream_handle(stream)))


def pir_answer_sliced_any_dev(d_keys, key_len_: int, nkeys: int, logN: int, d_dbs, nrec: int, rec_bytes: int, d_ans,
                              d_work, prefix_bits: int = 0, prefix: int = 0, device: int = 0, stream=None) -> None:
    """pir_answer_sliced_wide_dev for any rec_bytes that is a multiple of 4."""
    _check(lib().dpf_pir_answer_sliced_any_dev(device, _ptr(d_keys), key_len_, nkeys, logN, prefix_bits, prefix,
                                               _ptr(d_dbs), nrec, rec_bytes, _ptr(d_ans), _ptr(d_work),
                                               _stream_handle(stream)))


def pir_db_update_sliced_any_dev(d_dbs, nrec: int, rec_bytes: int, d_idx, d_recs, n: int, device: int = 0,
                                 stream=None) -> None:
    """pir_db_update_sliced_wide_dev for any rec_bytes that is a multiple of 4."""
    _check(lib().dpf_pir_db_update_sliced_any_dev(device, _ptr(d_dbs), nrec, rec_bytes, _ptr(d_idx), _ptr(d_recs), n,
                                                  _stream_handle(stream)))


def pir_db_gather_sliced_any_dev(d_dbs, nrec: int, rec_bytes: int, d_idx, n: int, d_out, device: int = 0,
                                 stream=None) -> None:
    """pir_db_gather_sliced_wide_dev for any rec_bytes that is a multiple of 4."""
    _check(lib().dpf_pir_db_gather_sliced_any_dev(device, _ptr(d_dbs), nrec, rec_bytes, _ptr(d_idx), n, _ptr(d_out),
                                                  _stream_handle(stream)))


def xor_scatter_sliced_any_dev(d_bits, bits_stride: int, nkeys: int, d_msgs, d_dbs, nrec: int, rec_bytes: int,
                               device: int = 0, stream=None) -> None:
    """xor_scatter_sliced_wide_dev for any rec_bytes that is a multiple of 4."""
    _check(lib().dpf_xor_scatter_sliced_any_dev(device, _ptr(d_bits), bits_stride, nkeys, _ptr(d_msgs), _ptr(d_dbs),
                                                nrec, rec_bytes, _stream_handle(stream)))


def pir_write_sliced_any_dev(d_keys, key_len_: int, nkeys: int, logN: int, d_msgs, d_dbs, nrec: int, rec_bytes: int,
                             d_work, prefix_bits: int = 0, prefix: int = 0, device: int = 0, stream=None) -> None:
    """pir_write_sliced_wide_dev for any rec_bytes that is a multiple of 4."""
    _check(lib().dpf_pir_write_sliced_any_dev(device, _ptr(d_keys), key_len_, nkeys, logN, prefix_bits, prefix,
                                              _ptr(d_msgs), _ptr(d_dbs), nrec, rec_bytes, _ptr(d_work),
                                              _stream_handle(stream)))


# ---- windows of the domain: sub-keys, window EvalFull, PIR over any record range ----
WINDOW_SUBTREE, WINDOW_PIECES = 0, 1
WindowForm = collections.namedtuple(
    "WindowForm", "route prefix_bits first_prefix npieces piece_bytes row_bytes row_offset sub_key_len")


def window_form_for(logN: int, first_block: int, nblocks: int, key_len_: Optional[int] = None) -> "WindowForm":
    """How the window forms evaluate leaf blocks [first_block, first_block +
    nblocks) of a 2^logN domain (dpf_window_form_for): one aligned subtree
    (WINDOW_SUBTREE) or npieces re-rooted sub-keys per key (WINDOW_PIECES),
    the window starting at byte row_offset of a row.  Needs no device."""
    c = WindowFormC()
    _check(lib().dpf_window_form_for(logN, first_block, nblocks, key_len(logN) if key_len_ is None else key_len_,
                                     ctypes.byref(c)))
    return WindowForm(*[int(getattr(c, f)) for f in WindowForm._fields])


def subkeys_dev(d_keys, key_len_: int, nkeys: int, logN: int, prefix_bits: int, first_prefix: int, nprefix: int, d_sub,
                device: int = 0, stream=None) -> None:
    """The device form of oracle.reroot_key: d_sub[k * nprefix + p] := key k as
    the key of subtree (prefix_bits, first_prefix + p), key_len_ - 18 *
    prefix_bits bytes each."""
    _check(lib().dpf_subkeys_dev(device, _ptr(d_keys), key_len_, nkeys, logN, prefix_bits, first_prefix, nprefix,
                                 _ptr(d_sub), _stream_handle(stream)))


def evalfull_window_workspace_size(nkeys: int, logN: int, first_block: int, nblocks: int) -> int:
    return int(lib().dpf_evalfull_window_workspace_size(nkeys, logN, first_block, nblocks))


def evalfull_window_dev(d_keys, key_len_: int, nkeys: int, logN: int, first_block: int, nblocks: int, d_rows,
                        row_stride: int, d_work, device: int = 0, stream=None) -> None:
    """EvalFull of every key over the window's pieces: row k (window_form_for:
    row_bytes, the window's 16 * nblocks bytes from row_offset) at d_rows + k *
    row_stride."""
    _check(lib().dpf_evalfull_window_dev(device, _ptr(d_keys), key_len_, nkeys, logN, first_block, nblocks, _ptr(d_rows),
                                         row_stride, _ptr(d_work), _stream_handle(stream)))


def pir_window_workspace_size(nkeys: int, logN: int, first_rec: int, nrec: int, rec_bytes: int) -> int:
    return int(lib().dpf_pir_window_workspace_size(nkeys, logN, first_rec, nrec, rec_bytes))


def pir_answer_window_dev(d_keys, key_len_: int, nkeys: int, logN: int, first_rec: int, d_dbs, nrec: int, rec_bytes: int,
                          d_ans, d_work, device: int = 0, stream=None) -> None:
    """Server answers (nkeys x rec_bytes) over records [first_rec, first_rec +
    nrec) of the domain (first_rec a multiple of 128), d_dbs their any-width
    sliced layout: the window EvalFull, then the sliced fold."""
    _check(lib().dpf_pir_answer_window_dev(device, _ptr(d_keys), key_len_, nkeys, logN, first_rec, _ptr(d_dbs), nrec,
                                           rec_bytes, _ptr(d_ans), _ptr(d_work), _stream_handle(stream)))


def pir_write_window_dev(d_keys, key_len_: int, nkeys: int, logN: int, first_rec: int, d_msgs, d_dbs, nrec: int,
                         rec_bytes: int, d_work, device: int = 0, stream=None) -> None:
    """The dual: record first_rec + j ^= XOR of the messages d_msgs[k] of the keys whose EvalFull has that bit set."""
    _check(lib().dpf_pir_write_window_dev(device, _ptr(d_keys), key_len_, nkeys, logN, first_rec, _ptr(d_msgs),
                                          _ptr(d_dbs), nrec, rec_bytes, _ptr(d_work), _stream_handle(stream)))


# ---- PIR over a sparse key set: record j lives at domain point d_points[j] ----
def pir_sparse_workspace_size(nkeys: int, nrec: int, logN: int) -> int:
    return int(lib().dpf_pir_sparse_workspace_size(nkeys, nrec, logN))


def pir_answer_sparse_dev(d_keys, key_len_: int, nkeys: int, logN: int, d_points, d_dbs, nrec: int, rec_bytes: int,
                          d_ans, d_work, device: int = 0, stream=None) -> None:
    """Server answers (nkeys x rec_bytes): the XOR of the records j of the
    sliced DB (any multiple of 4 bytes) with Eval(key, d_points[j]) = 1."""
    _check(lib().dpf_pir_answer_sparse_dev(device, _ptr(d_keys), key_len_, nkeys, logN, _ptr(d_points), _ptr(d_dbs),
                                           nrec, rec_bytes, _ptr(d_ans), _ptr(d_work), _stream_handle(stream)))


def pir_write_sparse_dev(d_keys, key_len_: int, nkeys: int, logN: int, d_points, d_msgs, d_dbs, nrec: int,
                         rec_bytes: int, d_work, device: int = 0, stream=None) -> None:
    """The dual: record j ^= XOR of the messages d_msgs[k] of the keys with Eval(key_k, d_points[j]) = 1."""
    _check(lib().dpf_pir_write_sparse_dev(device, _ptr(d_keys), key_len_, nkeys, logN, _ptr(d_points), _ptr(d_msgs),
                                          _ptr(d_dbs), nrec, rec_bytes, _ptr(d_work), _stream_handle(stream)))


# ---- grouped PIR: ngroups small DBs of one shape, each with its own keys ----
def pir_group_stride(nrec: int) -> int:
    """Flat records a group of nrec records takes in the grouped layout: nrec rounded up to 256."""
    return int(lib().dpf_pir_group_stride(nrec))


def pir_db_grouped_size(ngroups: int, nrec: int, rec_bytes: int) -> int:
    """Bytes of the grouped sliced layout (0 for a bad width or an overflowing product)."""
    return int(lib().dpf_pir_db_grouped_size(ngroups, nrec, rec_bytes))


def pir_db_slice_grouped_dev(d_db, ngroups: int, nrec: int, rec_bytes: int, d_dbs, device: int = 0, stream=None) -> None:
    """The grouped layout of a row-major d_db [ngroups][nrec][rec_bytes]: group g,
    record i at flat position g * pir_group_stride(nrec) + i of one sliced DB."""
    _check(lib().dpf_pir_db_slice_grouped_dev(device, _ptr(d_db), ngroups, nrec, rec_bytes, _ptr(d_dbs),
                                              _stream_handle(stream)))


def xor_fold_grouped_workspace_size(ngroups: int, keys_per_group: int, rec_bytes: int) -> int:
    return int(lib().dpf_xor_fold_grouped_workspace_size(ngroups, keys_per_group, rec_bytes))


def xor_fold_grouped_dev(d_bits, bits_stride: int, ngroups: int, keys_per_group: int, d_dbs, nrec: int, rec_bytes: int,
                         d_ans, d_work, device: int = 0, stream=None) -> None:
    """Answers (ngroups * keys_per_group x rec_bytes): row g * keys_per_group + j
    of d_bits selects among the nrec records of group g."""
    _check(lib().dpf_xor_fold_grouped_dev(device, _ptr(d_bits), bits_stride, ngroups, keys_per_group, _ptr(d_dbs), nrec,
                                          rec_bytes, _ptr(d_ans), _ptr(d_work), _stream_handle(stream)))


def pir_grouped_workspace_size(ngroups: int, keys_per_group: int, logN: int, rec_bytes: int) -> int:
    return int(lib().dpf_pir_grouped_workspace_size(ngroups, keys_per_group, logN, rec_bytes))


def pir_answer_grouped_dev(d_keys, key_len_: int, ngroups: int, keys_per_group: int, logN: int, d_dbs, nrec: int,
                           rec_bytes: int, d_ans, d_work, device: int = 0, stream=None) -> None:
    """One tree pass of all ngroups * keys_per_group keys (d_keys in group
    order) over the 2^logN domain of a group, then xor_fold_grouped_dev."""
    _check(lib().dpf_pir_answer_grouped_dev(device, _ptr(d_keys), key_len_, ngroups, keys_per_group, logN, _ptr(d_dbs),
                                            nrec, rec_bytes, _ptr(d_ans), _ptr(d_work), _stream_handle(stream)))


SCATTER_GROUPED, SCATTER_LOOP = 0, 1
ScatterGroupedForm = collections.namedtuple(
    "ScatterGroupedForm", "route columns pass_widths runs sg_per_run units max_blocks passes launches")


def xor_scatter_grouped_dev(d_bits, bits_stride: int, ngroups: int, keys_per_group: int, d_msgs, d_dbs, nrec: int,
                            rec_bytes: int, device: int = 0, stream=None) -> None:
    """The dual of xor_fold_grouped_dev: group g, record i ^= XOR of the
    messages d_msgs[g * keys_per_group + k] whose row of d_bits has bit i set.
    The zero records behind every group's nrec stay zero.  No workspace."""
    _check(lib().dpf_xor_scatter_grouped_dev(device, _ptr(d_bits), bits_stride, ngroups, keys_per_group, _ptr(d_msgs),
                                             _ptr(d_dbs), nrec, rec_bytes, _stream_handle(stream)))


def pir_write_grouped_dev(d_keys, key_len_: int, ngroups: int, keys_per_group: int, logN: int, d_msgs, d_dbs,
                          nrec: int, rec_bytes: int, d_work, device: int = 0, stream=None) -> None:
    """One tree pass of all ngroups * keys_per_group keys (group order) over a
    group's 2^logN domain, then xor_scatter_grouped_dev.  d_work holds
    pir_grouped_workspace_size bytes."""
    _check(lib().dpf_pir_write_grouped_dev(device, _ptr(d_keys), key_len_, ngroups, keys_per_group, logN, _ptr(d_msgs),
                                           _ptr(d_dbs), nrec, rec_bytes, _ptr(d_work), _stream_handle(stream)))


def scatter_grouped_form_for(ngroups: int, keys_per_group: int, nrec: int, rec_bytes: int,
                             cus: int = 0) -> "ScatterGroupedForm":
    """What xor_scatter_grouped_dev launches for this shape under the current
    fold limits (dpf_scatter_grouped_form_for).  Needs no device when cus > 0."""
    c = ScatterGroupedFormC()
    _check(lib().dpf_scatter_grouped_form_for(ngroups, keys_per_group, nrec, rec_bytes, cus, ctypes.byref(c)))
    return ScatterGroupedForm(*[int(getattr(c, f)) for f in ScatterGroupedForm._fields])


FOLD_GROUPED_DIRECT, FOLD_GROUPED_MFMA = 0, 1
FoldGroupedForm = collections.namedtuple(
    "FoldGroupedForm", "route columns_per_wg keys_per_tile atomic runs sg_per_run units passes launches max_blocks")


def fold_grouped_form_for(ngroups: int, keys_per_group: int, nrec: int, rec_bytes: int, cus: int = 0) -> "FoldGroupedForm":
    """What xor_fold_grouped_dev launches for this shape under the current fold
    limits and env DPF_GROUP_FOLD_ROUTE (dpf_fold_grouped_form_for): the direct
    route of up to 4 keys per pass or the matrix-core route of up to 256.
    Needs no device when cus > 0."""
    c = FoldGroupedFormC()
    _check(lib().dpf_fold_grouped_form_for(ngroups, keys_per_group, nrec, rec_bytes, cus, ctypes.byref(c)))
    return FoldGroupedForm(*[int(getattr(c, f)) for f in FoldGroupedForm._fields])


# ---- grouped keyword PIR: every group's records at its own points ----
def pir_grouped_sparse_workspace_size(ngroups: int, keys_per_group: int, nrec: int, logN: int, rec_bytes: int) -> int:
    return int(lib().dpf_pir_grouped_sparse_workspace_size(ngroups, keys_per_group, nrec, logN, rec_bytes))


def pir_answer_grouped_sparse_dev(d_keys, key_len_: int, ngroups: int, keys_per_group: int, logN: int, d_points, d_dbs,
                                  nrec: int, rec_bytes: int, d_ans, d_work, device: int = 0, stream=None) -> None:
    """Record i of group g lives at d_points[g][i] (uint64 [ngroups][nrec],
    tight): eval_bits_grouped_dev of all ngroups * keys_per_group keys (group
    order) into d_work, then xor_fold_grouped_dev.  d_dbs is the grouped
    layout; d_work holds pir_grouped_sparse_workspace_size bytes."""
    _check(lib().dpf_pir_answer_grouped_sparse_dev(device, _ptr(d_keys), key_len_, ngroups, keys_per_group, logN,
                                                   _ptr(d_points), _ptr(d_dbs), nrec, rec_bytes, _ptr(d_ans), _ptr(d_work),
                                                   _stream_handle(stream)))


def pir_write_grouped_sparse_dev(d_keys, key_len_: int, ngroups: int, keys_per_group: int, logN: int, d_points, d_msgs,
                                 d_dbs, nrec: int, rec_bytes: int, d_work, device: int = 0, stream=None) -> None:
    """The dual of pir_answer_grouped_sparse_dev: eval_bits_grouped_dev, then
    xor_scatter_grouped_dev.  The same workspace."""
    _check(lib().dpf_pir_write_grouped_sparse_dev(device, _ptr(d_keys), key_len_, ngroups, keys_per_group, logN,
                                                  _ptr(d_points), _ptr(d_msgs), _ptr(d_dbs), nrec, rec_bytes, _ptr(d_work),
                                                  _stream_handle(stream)))


# ---- whole-DB read-out: un-slice, XOR-merge ----
def pir_db_unslice_any_dev(d_dbs, nrec: int, rec_bytes: int, d_db, device: int = 0, stream=None) -> None:
    """The inverse of pir_db_slice_any_dev: d_db [nrec][rec_bytes] row-major from
    the sliced layout; exactly nrec rows are written."""
    _check(lib().dpf_pir_db_unslice_any_dev(device, _ptr(d_dbs), nrec, rec_bytes, _ptr(d_db), _stream_handle(stream)))


def pir_db_unslice_grouped_dev(d_dbs, ngroups: int, nrec: int, rec_bytes: int, d_db, device: int = 0,
                               stream=None) -> None:
    """The inverse of pir_db_slice_grouped_dev: d_db [ngroups][nrec][rec_bytes],
    tight, from the grouped layout; the padding behind each group is not written."""
    _check(lib().dpf_pir_db_unslice_grouped_dev(device, _ptr(d_dbs), ngroups, nrec, rec_bytes, _ptr(d_db),
                                                _stream_handle(stream)))


def pir_db_xor_sliced_dev(d_dbs, d_other, nbytes: int, device: int = 0, stream=None) -> None:
    """d_dbs ^= d_other over nbytes (a multiple of 16): two sliced buffers of one shape merged."""
    _check(lib().dpf_pir_db_xor_sliced_dev(device, _ptr(d_dbs), _ptr(d_other), nbytes, _stream_handle(stream)))


def set_export_limits(chunk_bytes: int = 0) -> None:
    """Tuning / test limit of the staging bytes of one piece of PirDB.export /
    xor_records (0 = default, 256 MiB; dpf_set_export_limits).  Results do not
    depend on it."""
    _check(lib().dpf_set_export_limits(chunk_bytes))


def set_fold_limits(max_blocks: int = 0, max_sg_per_block: int = 0) -> None:
    """Tuning / test limits of the fold launches (0 = default): workgroups per
    launch, and super-groups (256 records) per matrix-core fold workgroup;
    larger DBs fold in passes (dpf_set_fold_limits).  Answers do not depend
    on them."""
    _check(lib().dpf_set_fold_limits(max_blocks, max_sg_per_block))


class PirDB:
    """A DB of rec_bytes-byte records (any width from 1 byte; default 32
    whatever the array's shape; widths that are not a multiple of 32 go
    through dpf_pir_db_create_any) resident in HBM, sharded by top-level subtree over
    ngpus GPUs; answer() returns each key's XOR-inner-product, (n, rec_bytes)
    (host XOR of the per-GPU partials).

    With `points` (uint64, one per record) the handle is the sparse kind
    (dpf_pir_db_create_sparse, keyword PIR): record j lives at domain point
    points[j] instead of at index j, points may repeat (such records are
    selected together), shards are record ranges over any number of GPUs, and
    update()/read() take a record's position in the list.  The points are
    fixed at creation.

    With `ranged=True` the handle is the ranged dense kind
    (dpf_pir_db_create_ranged): record j still lives at domain point j, but
    the shards are balanced record ranges (shard.record_range) over any number
    of GPUs, each evaluated as a window of the domain (pir_answer_window_dev),
    so a table that is not a power of two costs what its records cost and no
    GPU is left empty.  Every method behaves as on the dense kind.

    With `groups=G` the handle is the grouped kind (dpf_pir_db_create_grouped):
    db is [G * nrec, rec] or [G, nrec, rec], G DBs of one shape, each with its
    own 2^logN domain and its own keys.  answer() takes keys [G * kpg, key_len]
    in group order (row g * kpg + j queries group g) and returns the answers
    in the same order; shards are ranges of whole groups over any number of
    GPUs; update()/read() take idx = g * nrec + i; write() is refused, the
    private write of a grouped handle is write_grouped().

    With `points` and `groups=G` together the handle is the grouped keyword
    kind (dpf_pir_db_create_grouped_sparse): `points` holds one uint64 per
    record in group order, [G * nrec] or [G, nrec], and record i of group g
    lives at domain point points[g][i] of a 2^logN domain (logN <= 63; nrec
    may exceed 2^logN, points may repeat within a group).  The keys of group g
    are evaluated at group g's own points in one launch for all groups.  In
    every other respect it is a grouped handle: answer() and write_grouped()
    take rows in group order, write() is refused, update() / read() / export()
    / xor_records() take idx = g * nrec + i, and clear() keeps the points."""

    def __init__(self, db: np.ndarray, logN: int, ngpus: int = 1, rec_bytes: int = 32, points=None, groups=None,
                 ranged: bool = False):
        d = np.ascontiguousarray(db, dtype=np.uint8).reshape(-1)
        if rec_bytes <= 0 or d.size % rec_bytes:
            raise ValueError("DB size must be a multiple of %d bytes" % rec_bytes)
        if ranged and (points is not None or groups is not None):
            raise ValueError("ranged=True is a kind of its own: no points, no groups")
        self.logN = logN
        self.rec_bytes = rec_bytes
        nrec = d.size // rec_bytes
        h = _vp()
        if ranged:
            _check(lib().dpf_pir_db_create_ranged(_buf(d), nrec, rec_bytes, logN, ngpus, ctypes.byref(h)))
        elif groups is not None:
            if groups < 0 or (nrec % groups if groups else nrec):
                raise ValueError("the DB must hold the same number of records for each of %d groups" % groups)
            per = nrec // groups if groups else 0
            if points is not None:
                pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1)
                if pts.size != nrec:
                    raise ValueError("points must hold one uint64 per record")
                _check(lib().dpf_pir_db_create_grouped_sparse(pts.ctypes.data_as(_u64p), _buf(d), groups, per, rec_bytes,
                                                              logN, ngpus, ctypes.byref(h)))
            else:
                _check(lib().dpf_pir_db_create_grouped(_buf(d), groups, per, rec_bytes, logN, ngpus, ctypes.byref(h)))
        elif points is not None:
            pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1)
            if pts.size != nrec:
                raise ValueError("points must hold one uint64 per record")
            _check(lib().dpf_pir_db_create_sparse(pts.ctypes.data_as(_u64p), _buf(d), nrec, rec_bytes, logN, ngpus,
                                                  ctypes.byref(h)))
        elif rec_bytes == 32:
            _check(lib().dpf_pir_db_create(_buf(d), nrec, logN, ngpus, ctypes.byref(h)))
        elif rec_bytes % 32 == 0:
            _check(lib().dpf_pir_db_create_wide(_buf(d), nrec, rec_bytes, logN, ngpus, ctypes.byref(h)))
        else:
            _check(lib().dpf_pir_db_create_any(_buf(d), nrec, rec_bytes, logN, ngpus, ctypes.byref(h)))
        self._h = h

    @property
    def nrec(self) -> int:
        """Records the handle holds, asked of the handle (dpf_pir_db_nrec).
        Read-only, and 0 once the handle is closed: it used to be a plain
        attribute that kept the count given to the constructor."""
        return int(lib().dpf_pir_db_nrec(self._h))

    @property
    def ngroups(self) -> int:
        """Groups of a grouped handle; 1 for the other kinds, 0 once closed (dpf_pir_db_ngroups)."""
        return int(lib().dpf_pir_db_ngroups(self._h))

    def answer(self, keys: np.ndarray) -> np.ndarray:
        kk = np.ascontiguousarray(keys, dtype=np.uint8)
        n, kl = kk.shape
        ans = np.zeros((n, int(lib().dpf_pir_db_rec_bytes(self._h))), np.uint8)
        _check(lib().dpf_pir_answer(self._h, _buf(kk), kl, n, _buf(ans)))
        return ans

    def update(self, idx, recs) -> None:
        """Record idx[i] := recs[i] in place (any order; of repeated indices
        the last wins).  One index >= nrec raises DPFPanic (DPF_ERR_PARAM)
        and changes nothing."""
        ix = np.ascontiguousarray(idx, dtype=np.uint64).reshape(-1)
        r = np.ascontiguousarray(recs, dtype=np.uint8).reshape(-1)
        if r.size != ix.size * self.rec_bytes:
            raise ValueError("recs must hold len(idx) records of %d bytes" % self.rec_bytes)
        _check(lib().dpf_pir_db_update(self._h, ix.ctypes.data_as(_u64p), _buf(r), ix.size))

    def write(self, keys, msgs) -> None:
        """Private write: record i ^= XOR of the messages msgs[k] (rec_bytes
        each) whose key has bit i of its EvalFull set.  Two servers applying
        the same messages under their key shares change the XOR of their DBs
        by msgs[k] at alpha_k only.  A short key raises DPFPanic and changes
        nothing."""
        kk = np.ascontiguousarray(keys, dtype=np.uint8)
        if kk.ndim != 2:
            raise ValueError("keys must be a (nkeys, key_len) array")
        m = np.ascontiguousarray(msgs, dtype=np.uint8).reshape(-1)
        if m.size != kk.shape[0] * self.rec_bytes:
            raise ValueError("msgs must hold len(keys) messages of %d bytes" % self.rec_bytes)
        _check(lib().dpf_pir_db_write(self._h, _buf(kk), kk.shape[1], kk.shape[0], _buf(m)))

    def write_grouped(self, keys, msgs) -> None:
        """Private write of a grouped handle: keys [G * kpg, key_len] and msgs
        [G * kpg, rec_bytes] in group order; record i of group g ^= XOR of the
        messages of group g's keys whose EvalFull has bit i set.  A key with
        an all-zero message is a dummy.  A key count that is no multiple of
        the groups, a handle that is not grouped or a short key raises
        DPFPanic and changes nothing."""
        kk = np.ascontiguousarray(keys, dtype=np.uint8)
        if kk.ndim != 2:
            raise ValueError("keys must be a (nkeys, key_len) array")
        m = np.ascontiguousarray(msgs, dtype=np.uint8).reshape(-1)
        if m.size != kk.shape[0] * self.rec_bytes:
            raise ValueError("msgs must hold len(keys) messages of %d bytes" % self.rec_bytes)
        _check(lib().dpf_pir_db_write_grouped(self._h, _buf(kk), kk.shape[1], kk.shape[0], _buf(m)))

    def read(self, idx) -> np.ndarray:
        """The records idx[i] as the DB now holds them, (len(idx), rec_bytes), in the caller's order."""
        ix = np.ascontiguousarray(idx, dtype=np.uint64).reshape(-1)
        out = np.zeros((ix.size, self.rec_bytes), np.uint8)
        _check(lib().dpf_pir_db_read(self._h, ix.ctypes.data_as(_u64p), ix.size, _buf(out)))
        return out

    def export(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """The records [first, first + n) as the DB now holds them, (n, rec_bytes);
        n=None: up to the end.  The whole-DB read-out: no index list, pieces
        of whole super-groups un-sliced on the device.  A range outside the DB
        raises DPFPanic (DPF_ERR_PARAM)."""
        if first < 0 or (n is not None and n < 0):
            raise ValueError("first and n must not be negative")
        if n is None:
            n = max(0, self.nrec - first)
        out = np.zeros((n, self.rec_bytes), np.uint8)
        _check(lib().dpf_pir_db_export(self._h, first, n, _buf(out)))
        return out

    def xor_records(self, recs, first: int = 0) -> None:
        """Record first + i ^= recs[i]: the other server's exported share merged
        into this one.  A range outside the DB raises DPFPanic and changes
        nothing."""
        r = np.ascontiguousarray(recs, dtype=np.uint8).reshape(-1)
        if first < 0 or r.size % self.rec_bytes:
            raise ValueError("recs must hold whole records of %d bytes, first must not be negative" % self.rec_bytes)
        _check(lib().dpf_pir_db_xor_records(self._h, first, r.size // self.rec_bytes, _buf(r)))

    def clear(self) -> None:
        """Every record := 0 (the next epoch's empty table); a sparse or grouped keyword handle keeps its points."""
        _check(lib().dpf_pir_db_clear(self._h))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            lib().dpf_pir_db_free(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
