"""Size functions and argument checks of the window entry points
(include/dpf_hip.h: dpf_window_form_for, dpf_subkeys_dev,
dpf_evalfull_window_dev, the two PIR window composites and
dpf_pir_db_create_ranged).  No device is needed: the forms and sizes are
arithmetic, and every DPF_ERR_PARAM / DPF_ERR_KEYLEN case returns before any
device call.  The checks run in a fresh child process that sees no GPU (this
file, run as a script), and the child makes no call unless dpf_gpu_init(0) is
DPF_ERR_NODEV there: the device pointers are fake addresses, so a check that
went missing shows up as a wrong code, never as a launch on one of them."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_GPU = {"HIP_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "", "GPU_DEVICE_ORDINAL": ""}

P = 1 << 20      # an aligned fake device address
LOGN = 40
KL = 33 + 18 * (LOGN - 7)
SHORT = 17 + 18 * (LOGN - 7) - 1

NAMES = ("dpf_window_form_for", "dpf_subkeys_dev", "dpf_evalfull_window_workspace_size", "dpf_evalfull_window_dev",
         "dpf_pir_window_workspace_size", "dpf_pir_answer_window_dev", "dpf_pir_write_window_dev",
         "dpf_pir_db_create_ranged")


def _plan(logN, fb, nb):
    """pir_window_plan.hpp's window_plan, restated: (route, prefix_bits, first_prefix, npieces, piece_bytes, row_offset)."""
    if logN < 7:
        return 0, 0, 0, 1, 16, 0
    m = nb.bit_length() - 1 + 7
    eb = (fb ^ (fb + nb - 1)).bit_length()       # the smallest aligned run of 2^eb blocks that holds the window
    if 1 << eb <= 2 * nb:
        return 0, logN - eb - 7, fb >> eb, 1, 16 << eb, 16 * (fb - (fb >> eb << eb))
    s = max(m - 4, 7)
    first = fb >> (s - 7)
    return 1, logN - s, first, ((fb + nb - 1) >> (s - 7)) - first + 1, 16 << (s - 7), 16 * (fb - (first << (s - 7)))


def check_names(dpf, L):
    for name in NAMES:
        assert name in dpf.SIGNATURES and hasattr(L, name), name


def check_forms(dpf, L):
    for logN, fb, nb in ((14, 0, 128), (14, 1, 1), (14, 3, 37), (14, 63, 2), (14, 127, 1), (14, 5, 123), (9, 1, 2), (6, 0, 1),
                         (14, 41, 39), (16, 37, 40), (40, (1 << 30) + 3, 40), (40, (1 << 30) + 3, 62), (63, (1 << 56) - 1, 1),
                         (63, 1, (1 << 56) - 1), (63, (1 << 55) - 3, 9), (24, 0, 5 << 14), (24, 3 * 5 << 11, 5 << 11)):
        for extra in (0, 5):
            kl = dpf.key_len(logN) + extra
            f = dpf.window_form_for(logN, fb, nb, kl)
            route, pb, first, P_, piece, off = _plan(logN, fb, nb)
            assert (f.route, f.prefix_bits, f.first_prefix, f.npieces, f.piece_bytes, f.row_offset) == \
                (route, pb, first, P_, piece, off), (logN, fb, nb, f)
            assert f.row_bytes == P_ * piece and f.sub_key_len == (kl - 18 * pb if route else kl)
            assert f.npieces <= 33 and f.row_offset + 16 * nb <= f.row_bytes and f.prefix_bits <= max(logN - 7, 0)
    assert dpf.window_form_for(14, 41, 39).sub_key_len == 51 == dpf.key_len(8)   # 20 pieces of 2^8 points
    assert dpf.window_form_for(14, 41, 39).route == dpf.WINDOW_PIECES and dpf.window_form_for(14, 3, 37).route == dpf.WINDOW_SUBTREE
    form = dpf.WindowFormC()
    q = lambda *a: L.dpf_window_form_for(*a, ctypes.byref(form))
    assert L.dpf_window_form_for(14, 0, 1, 500, None) == dpf.DPF_ERR_PARAM
    assert q(64, 0, 1, 4096) == dpf.DPF_ERR_PARAM and b"logN > 63" in L.dpf_last_error()
    assert q(14, 0, 1, 17 + 18 * 7 - 1) == dpf.DPF_ERR_KEYLEN
    for fb, nb in ((0, 0), (128, 1), (127, 2), (0, 129), (1, (1 << 64) - 1)):
        assert q(14, fb, nb, 500) == dpf.DPF_ERR_PARAM and b"window outside" in L.dpf_last_error(), (fb, nb)
    assert q(6, 0, 2, 33) == dpf.DPF_ERR_PARAM and q(6, 1, 1, 33) == dpf.DPF_ERR_PARAM


def check_subkeys(dpf, L):
    def sub(keys=P, kl=KL, nk=3, logN=LOGN, pb=33, first=0, npfx=4, out=P):
        return L.dpf_subkeys_dev(0, keys, kl, nk, logN, pb, first, npfx, out, None)

    assert sub(logN=64, kl=4096) == dpf.DPF_ERR_PARAM and b"logN > 63" in L.dpf_last_error()
    assert sub(kl=SHORT) == dpf.DPF_ERR_KEYLEN and b"key shorter" in L.dpf_last_error()
    assert sub(pb=34) == dpf.DPF_ERR_PARAM and b"prefix_bits" in L.dpf_last_error()          # prefix_bits > stop
    assert sub(logN=6, kl=33, pb=1) == dpf.DPF_ERR_PARAM and b"prefix_bits" in L.dpf_last_error()
    assert sub(first=(1 << 33) - 3) == dpf.DPF_ERR_PARAM and b"prefix out of range" in L.dpf_last_error()
    assert sub(first=1 << 33, npfx=1) == dpf.DPF_ERR_PARAM and b"prefix out of range" in L.dpf_last_error()
    assert sub(first=0, npfx=(1 << 33) + 1) == dpf.DPF_ERR_PARAM
    assert sub(first=(1 << 64) - 1, npfx=2) == dpf.DPF_ERR_PARAM                              # the sum wraps
    assert sub(pb=0, first=0, npfx=2) == dpf.DPF_ERR_PARAM
    # The final CW must lie behind the records walked: 33 + 18 * prefix_bits bytes.
    assert sub(kl=17 + 18 * 33 + 15) == dpf.DPF_ERR_KEYLEN and b"prefix_bits" in L.dpf_last_error()
    for name in ("keys", "out"):
        assert sub(**{name: None}) == dpf.DPF_ERR_PARAM and b"null" in L.dpf_last_error(), name
    # The order: logN, key, prefix_bits, the run, the key's tail, null.
    assert sub(kl=SHORT, pb=34) == dpf.DPF_ERR_KEYLEN
    assert sub(pb=34, first=1 << 40) == dpf.DPF_ERR_PARAM and b"prefix_bits" in L.dpf_last_error()
    assert sub(first=1 << 40, keys=None) == dpf.DPF_ERR_PARAM and b"prefix out of range" in L.dpf_last_error()
    # Nothing to do: DPF_OK without a launch.
    assert sub(nk=0, keys=None, out=None) == dpf.DPF_OK and sub(npfx=0, keys=None, out=None) == dpf.DPF_OK
    assert sub(nk=0, pb=34) == dpf.DPF_ERR_PARAM


def check_evalfull_window(dpf, L):
    def ev(keys=P, kl=KL, nk=3, logN=LOGN, fb=41, nb=39, rows=P, stride=640, work=P):
        return L.dpf_evalfull_window_dev(0, keys, kl, nk, logN, fb, nb, rows, stride, work, None)

    assert dpf.window_form_for(LOGN, 41, 39).row_bytes == 640
    assert ev(logN=64, kl=4096) == dpf.DPF_ERR_PARAM and b"logN > 63" in L.dpf_last_error()
    assert ev(kl=SHORT) == dpf.DPF_ERR_KEYLEN
    assert ev(nb=0) == dpf.DPF_ERR_PARAM and b"window outside" in L.dpf_last_error()
    assert ev(fb=(1 << 33) - 2, nb=3) == dpf.DPF_ERR_PARAM and b"window outside" in L.dpf_last_error()
    assert ev(fb=1 << 33, nb=1) == dpf.DPF_ERR_PARAM
    for stride in (624, 632, 16, 0, 641):                                # short, or not a multiple of 16
        assert ev(stride=stride) == dpf.DPF_ERR_PARAM and b"row_stride" in L.dpf_last_error(), stride
    assert ev(fb=4, nb=4, stride=48) == dpf.DPF_ERR_PARAM               # the subtree route: one piece of 64 bytes
    for name in ("keys", "rows", "work"):
        assert ev(**{name: None}) == dpf.DPF_ERR_PARAM and b"null" in L.dpf_last_error(), name
    for name in ("rows", "work"):
        assert ev(**{name: P + 8}) == dpf.DPF_ERR_PARAM and b"misaligned" in L.dpf_last_error(), name
    # The order: logN, key, window, stride, null, misaligned.
    assert ev(kl=SHORT, nb=0) == dpf.DPF_ERR_KEYLEN
    assert ev(nb=0, stride=8) == dpf.DPF_ERR_PARAM and b"window outside" in L.dpf_last_error()
    assert ev(stride=8, keys=None) == dpf.DPF_ERR_PARAM and b"row_stride" in L.dpf_last_error()
    assert ev(keys=None, rows=P + 8) == dpf.DPF_ERR_PARAM and b"null" in L.dpf_last_error()
    assert ev(nk=0, keys=None, rows=None, work=None) == dpf.DPF_OK
    assert ev(nk=0, stride=8) == dpf.DPF_ERR_PARAM


def _composite(dpf, L, call, nullable, aligned16, aligned4=()):
    for rec in (0, 6, 32768 + 4):                                        # a bad rec_bytes
        assert call(rec=rec) == dpf.DPF_ERR_PARAM and b"rec_bytes" in L.dpf_last_error(), rec
    assert call(logN=64, kl=4096) == dpf.DPF_ERR_PARAM and b"logN > 63" in L.dpf_last_error()
    assert call(kl=SHORT) == dpf.DPF_ERR_KEYLEN and b"key shorter" in L.dpf_last_error()
    for first in (1, 64, 127, 128 * 37 + 1):                             # first_rec % 128 != 0
        assert call(first=first) == dpf.DPF_ERR_PARAM and b"multiple of 128" in L.dpf_last_error(), first
    assert call(first=(1 << LOGN) - 128, nrec=129) == dpf.DPF_ERR_PARAM and b"outside" in L.dpf_last_error()
    assert call(first=1 << LOGN, nrec=1) == dpf.DPF_ERR_PARAM and b"outside" in L.dpf_last_error()
    assert call(first=1 << (LOGN + 1), nrec=0) == dpf.DPF_ERR_PARAM
    assert call(first=0, nrec=(1 << LOGN) + 1) == dpf.DPF_ERR_PARAM
    assert call(first=128, nrec=(1 << 64) - 1) == dpf.DPF_ERR_PARAM     # the sum wraps
    for name in nullable:
        assert call(**{name: None}) == dpf.DPF_ERR_PARAM and b"null" in L.dpf_last_error(), name
    for name in aligned16:
        assert call(**{name: P + 8}) == dpf.DPF_ERR_PARAM and b"misaligned" in L.dpf_last_error(), name
    for name in aligned4:
        assert call(**{name: P + 2}) == dpf.DPF_ERR_PARAM and b"misaligned" in L.dpf_last_error(), name
    # The order: rec_bytes, logN, key, first_rec, the range, null, misaligned.
    assert call(rec=6, logN=64) == dpf.DPF_ERR_PARAM and b"rec_bytes" in L.dpf_last_error()
    assert call(kl=SHORT, first=1) == dpf.DPF_ERR_KEYLEN
    assert call(first=1, nrec=1 << 41) == dpf.DPF_ERR_PARAM and b"multiple of 128" in L.dpf_last_error()
    assert call(nrec=1 << 41, keys=None) == dpf.DPF_ERR_PARAM and b"outside" in L.dpf_last_error()
    assert call(keys=None, dbs=P + 8) == dpf.DPF_ERR_PARAM and b"null" in L.dpf_last_error()
    assert call(nk=0, kl=10) == dpf.DPF_ERR_KEYLEN and call(nk=0, rec=6) == dpf.DPF_ERR_PARAM


def check_composites(dpf, L):
    def answer(keys=P, kl=KL, nk=3, logN=LOGN, first=128 * 37, dbs=P, nrec=5000, rec=20, ans=P, work=P):
        return L.dpf_pir_answer_window_dev(0, keys, kl, nk, logN, first, dbs, nrec, rec, ans, work, None)

    def write(keys=P, kl=KL, nk=3, logN=LOGN, first=128 * 37, msgs=P, dbs=P, nrec=5000, rec=20, work=P):
        return L.dpf_pir_write_window_dev(0, keys, kl, nk, logN, first, msgs, dbs, nrec, rec, work, None)

    _composite(dpf, L, answer, ("keys", "dbs", "ans", "work"), ("dbs", "work"), ("ans",))
    _composite(dpf, L, write, ("keys", "msgs", "dbs", "work"), ("msgs", "dbs", "work"))
    # Buffers the answer has no work for may be null; the write wants them all, as the other scatters do.
    assert answer(nk=0, keys=None, dbs=None, ans=None, work=None) == dpf.DPF_OK
    assert answer(nrec=0, dbs=None, ans=None) == dpf.DPF_ERR_PARAM      # the answers are still zeroed
    assert write(nk=0) == dpf.DPF_OK and write(nrec=0) == dpf.DPF_OK
    assert write(nk=0, msgs=None) == dpf.DPF_ERR_PARAM and b"null" in L.dpf_last_error()


def check_sizes(dpf, L):
    a256 = lambda x: (x + 255) // 256 * 256
    fold = dpf.xor_fold_workspace_size()
    for nk, logN, fb, nb in ((1, 14, 41, 39), (5, 16, 37, 40), (65, 16, 63, 40), (3, 40, (1 << 30) + 3, 62), (2, 14, 63, 2),
                             (7, 24, 3 * 5 << 11, 5 << 11)):
        f = dpf.window_form_for(logN, fb, nb)
        assert f.route == dpf.WINDOW_PIECES
        s = logN - f.prefix_bits
        # [sub-keys of the canonical length | tree workspace of nk * P keys at logN' = s | rows (+16) | partials]
        front = a256(nk * f.npieces * dpf.key_len(s)) + a256(dpf.pir_workspace_size(nk * f.npieces, s, 0) - fold -
                                                              a256(nk * f.npieces * (16 << (s - 7))))
        assert dpf.evalfull_window_workspace_size(nk, logN, fb, nb) == front, (nk, logN, fb, nb)
        for nrec in (128 * nb, 128 * nb - 127):
            assert dpf.pir_window_workspace_size(nk, logN, 128 * fb, nrec, 20) == \
                front + a256(nk * f.row_bytes + 16) + fold, (nk, logN, fb, nrec)
    # One subtree (the window itself, or one of at most twice its points): the
    # dense composite's tree workspace, no sub-keys.
    for fb, nb, pb, first in ((256, 256, 1, 1), (1, 511, 0, 0), (70, 40, 3, 1)):
        f = dpf.window_form_for(16, fb, nb)
        assert (f.route, f.prefix_bits, f.first_prefix, f.row_offset) == (dpf.WINDOW_SUBTREE, pb, first, 16 * (fb % (512 >> pb)))
        tree = dpf.pir_workspace_size(4, 16, pb) - fold - a256(4 * f.row_bytes)
        assert dpf.evalfull_window_workspace_size(4, 16, fb, nb) == tree
        assert dpf.pir_window_workspace_size(4, 16, 128 * fb, 128 * nb - 5, 32) == tree + a256(4 * f.row_bytes + 16) + fold
    # Refused arguments have no size; no records need the ABI's minimum.
    assert dpf.evalfull_window_workspace_size(1, 14, 127, 2) == 0 and dpf.evalfull_window_workspace_size(1, 64, 0, 1) == 0
    assert dpf.pir_window_workspace_size(1, 14, 64, 10, 32) == 0 and dpf.pir_window_workspace_size(1, 14, 0, 10, 6) == 0
    assert dpf.pir_window_workspace_size(1, 14, 128, (1 << 14) - 127, 32) == 0
    assert dpf.pir_window_workspace_size(1, 14, 128, 0, 32) == 16


def check_handle(dpf, L):
    h = ctypes.c_void_p(1)
    db = (ctypes.c_uint8 * 128)()
    u8 = ctypes.cast(db, ctypes.POINTER(ctypes.c_uint8))
    create = L.dpf_pir_db_create_ranged
    assert create(u8, 4, 32, 10, 1, None) == dpf.DPF_ERR_PARAM                       # null handle pointer
    for rec in (0, 32768 + 1):
        h = ctypes.c_void_p(1)
        assert create(u8, 4, rec, 10, 1, ctypes.byref(h)) == dpf.DPF_ERR_PARAM and h.value is None
        assert b"rec_bytes" in L.dpf_last_error()
    h = ctypes.c_void_p(1)
    assert create(u8, 4, 32, 64, 1, ctypes.byref(h)) == dpf.DPF_ERR_PARAM and h.value is None
    assert create(u8, 5, 32, 2, 1, ctypes.byref(h)) == dpf.DPF_ERR_PARAM and b"larger than 2^logN" in L.dpf_last_error()
    assert create(u8, 4, 32, 10, 3, ctypes.byref(h)) == dpf.DPF_ERR_NODEV            # any count: the devices are asked next


def check_record_range(dpf):
    from dpf import shard
    for nrec in (0, 1, 255, 256, 257, 1000, 5 * (1 << 10) + 3, 5 << 21):
        for world in (1, 2, 3, 5, 8):
            got = [shard.record_range(nrec, world, r) for r in range(world)]
            per = -(-(-(-nrec // 256)) // world) * 256
            assert got == [(min(nrec, r * per), min(nrec, r * per + per)) for r in range(world)]
            assert got[0][0] == 0 and got[-1][1] == nrec and all(a[1] == b[0] for a, b in zip(got, got[1:]))
            assert all(lo % 128 == 0 or lo == nrec for lo, _ in got)
    assert [shard.record_range(5 << 21, 8, r)[1] - shard.record_range(5 << 21, 8, r)[0] for r in range(8)] == [5 << 18] * 8


def child():
    sys.path.insert(0, os.path.join(ROOT, "dpf-go_amd"))
    import dpf
    L = dpf.lib()
    assert L.dpf_gpu_init(0) == dpf.DPF_ERR_NODEV, "the child must see no GPU"
    check_names(dpf, L)
    check_forms(dpf, L)
    check_subkeys(dpf, L)
    check_evalfull_window(dpf, L)
    check_composites(dpf, L)
    check_sizes(dpf, L)
    check_handle(dpf, L)
    check_record_range(dpf)
    print("window capi ok")


def test_window_entries_validate_before_touching_a_device():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, **NO_GPU))
    assert r.returncode == 0 and "window capi ok" in r.stdout, r.stdout[-3000:] + r.stderr[-6000:]


if __name__ == "__main__" and sys.argv[1:] == ["--child"]:
    child()
