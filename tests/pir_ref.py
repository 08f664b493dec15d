"""Plain numpy references of the PIR operations, shared by the test files
that need them (a helper module, not a test file): the sliced layout from its
definition, the XOR fold and its dual the XOR scatter, update / gather of
records, and the grouped expectation.  Everything here restates
include/dpf_hip.h on the CPU and never calls the code under test.

Selection rows are EvalFull's packed bits: bit i of a row is bit i % 8 of its
byte i / 8."""
import numpy as np


def sel_bool(rows: np.ndarray, nrec: int) -> np.ndarray:
    """bool [nkeys][nrec] of packed selection rows uint8 [nkeys][stride]; bits at positions >= nrec are dropped."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    return np.unpackbits(rows, axis=1, bitorder="little")[:, :nrec].astype(bool)


def pack_rows(bits: np.ndarray, stride: int) -> np.ndarray:
    """uint8 [nkeys][stride] of 0/1 answers [nkeys][npts], zero bits behind the last point."""
    out = np.zeros((bits.shape[0], stride), np.uint8)
    p = np.packbits(np.ascontiguousarray(bits, dtype=np.uint8), axis=1, bitorder="little")
    out[:, :p.shape[1]] = p
    return out


def layout(db: np.ndarray) -> np.ndarray:
    """The sliced layout of a row-major (nrec, rec_bytes) DB, rec_bytes a
    multiple of 4, from its definition: u32 dbs[S][p][g], bit j = bit p (bit
    p % 8 of byte p / 8) of record 256 S + 32 g + j; records past nrec are 0.
    For rec_bytes = 32 C it is the wide layout dbs[S][c][n][g], p = 256 c + n."""
    nrec, rec = db.shape
    nsg = (nrec + 255) // 256
    pad = np.zeros((nsg * 256, rec), np.uint8)
    pad[:nrec] = db
    b = np.unpackbits(pad, axis=1, bitorder="little")          # [record][p]
    b = b.reshape(nsg, 8, 32, 8 * rec).transpose(0, 3, 1, 2)    # [S][p][g][j]
    return np.packbits(np.ascontiguousarray(b).reshape(-1), bitorder="little")   # LE u32 = 4 bytes of j


def grouped_flat(db: np.ndarray) -> np.ndarray:
    """The flat DB of a grouped one [ngroups][nrec][rec]: every group padded
    with zero records to a multiple of 256 (dpf_pir_group_stride)."""
    ng, nrec, rec = db.shape
    gs = (nrec + 255) // 256 * 256
    flat = np.zeros((ng, gs, rec), np.uint8)
    flat[:, :nrec] = db
    return flat.reshape(ng * gs, rec)


def xor_fold(rows: np.ndarray, db: np.ndarray, nrec: int) -> np.ndarray:
    """[nkeys][rec]: the XOR of the records i < nrec of db whose bit i of a selection row is set."""
    bits = sel_bool(rows, nrec).astype(np.float64)
    dbb = np.unpackbits(db[:nrec], axis=1, bitorder="little").astype(np.float64)
    par = (bits @ dbb).astype(np.int64) & 1                     # counts <= nrec < 2^53: exact
    return np.packbits(par.astype(np.uint8), axis=1, bitorder="little")


def xor_scatter(db: np.ndarray, rows: np.ndarray, msgs: np.ndarray, nrec: int) -> np.ndarray:
    """db with record i ^= XOR of msgs[k] over the keys k with bit i of rows[k] set, i < nrec."""
    bits = sel_bool(rows, nrec).astype(np.float64)              # [k][i]
    mb = np.unpackbits(msgs, axis=1, bitorder="little").astype(np.float64)   # [k][p]
    par = (bits.T @ mb).astype(np.int64) & 1
    out = db.copy()
    out[:nrec] ^= np.packbits(par.astype(np.uint8), axis=1, bitorder="little")
    return out


def update(db: np.ndarray, idx, recs, nrec=None) -> np.ndarray:
    """The modified row-major DB: updates in order (the last of equal indices wins), indices >= nrec skipped."""
    n = db.shape[0] if nrec is None else nrec
    out = db.copy()
    for i, r in zip(idx, recs):
        if int(i) < n:
            out[int(i)] = r
    return out


def gather(db: np.ndarray, idx, nrec=None) -> np.ndarray:
    """[len(idx)][rec]: record idx[i] in the caller's order, zeros for idx[i] >= nrec."""
    n = db.shape[0] if nrec is None else nrec
    ix = np.asarray(idx, np.uint64)
    out = np.zeros((ix.size, db.shape[1]), np.uint8)
    ok = ix < n
    out[ok] = db[ix[ok].astype(np.int64)]
    return out


def grouped_expect(db: np.ndarray, sel: np.ndarray, kpg: int) -> np.ndarray:
    """[ngroups * kpg][rec]: row g * kpg + j is the XOR of the rows of db[g]
    (db [ngroups][nrec][rec]) that sel[g * kpg + j] (bool [nrec]) selects."""
    out = np.zeros((sel.shape[0], db.shape[2]), np.uint8)
    for r in range(sel.shape[0]):
        if sel[r].any():
            out[r] = np.bitwise_xor.reduce(db[r // kpg][sel[r]], axis=0)
    return out
