"""Host restatement, in numpy, of the walk tape's cell-sorted index and of the order in which the
device sums over it (include/wos.h "Walk tape adjoint, indexed", csrc/wos_tape_index.hip): the
yardstick of tests/test_tape_index_cpu.py and tests/test_gpu_tape_index.py.

(a) index(): the canonical term list of one segment (a dict as tape_adjoint_model.read_segments
    returns it), stably sorted by cell: row [cells + 1], id, w, cell.
(b) rowsum(): the per-row sums of x[id] * w in the device's float32 operation order, a function
    of the row offsets and the tile constant alone.
"""
import numpy as np

FIRST = 0x80000000  # id bit 31: a first-ball term (takes c, not a)
CHUNK = 64          # terms a wave reduces at once


def index(seg, cells, dtype=np.float32):
    """row, id, w, cell of a segment's index.  dtype: the type thr * nrm is formed in -- float32
    is the device's single rounding, float64 the exact product (for the float64 reference)."""
    code, cnt, slot = seg["code"], seg["cnt"], seg["slot"].astype(np.int64)
    T = code.shape[0]
    rec = (code & 1) != 0
    # 1. the first balls, by task
    t = np.nonzero(rec & (seg["cell0"] < cells))[0]
    cell_a = seg["cell0"][t].astype(np.int64)
    id_a = (t.astype(np.uint32) | np.uint32(FIRST))
    w_a = seg["gnorm"][t].astype(dtype)
    # 2. the filled entry slots, by slot
    owner = np.full(int(slot[-1]), -1, np.int64)
    for j in range(T):
        if rec[j]:
            n = min(int(cnt[j] & np.uint32(0x7FFFFFFF)), int(slot[j + 1] - slot[j]))
            owner[slot[j]:slot[j] + n] = j
    e = np.nonzero(owner >= 0)[0]
    e = e[seg["cell"][e] < cells]
    cell_b = seg["cell"][e].astype(np.int64)
    id_b = owner[e].astype(np.uint32)
    w_b = seg["thr"][e].astype(dtype) * seg["nrm"][e].astype(dtype)
    cell = np.concatenate([cell_a, cell_b])
    order = np.argsort(cell, kind="stable")
    row = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=cells))]).astype(np.uint32)
    return row, np.concatenate([id_a, id_b])[order], np.concatenate([w_a, w_b])[order], cell[order].astype(np.uint32)


def gather(id, a, c):
    """x per term: c[task] for a first-ball term, a[task] else."""
    task = (id & np.uint32(FIRST - 1)).astype(np.int64)
    return np.where((id & np.uint32(FIRST)) != 0, np.asarray(c)[task], np.asarray(a)[task])


def rowsum64(row, id, w, a, c):
    """The per-row sums in float64, in any order: the value the ordered float32 sum approximates."""
    n_rows = row.shape[0] - 1
    cell = np.repeat(np.arange(n_rows), np.diff(row.astype(np.int64)))
    out = np.zeros(n_rows)
    np.add.at(out, cell, gather(id, a, c).astype(np.float64) * w.astype(np.float64))
    return out


def rowsum(row, id, w, a, c, tile):
    """float32 [n_rows]: the device's sums of one segment, from zero.
    v_i = fl(x_i w_i); per chunk of 64 consecutive terms the steps off = 1, 2, .., 32 of
    v_l = fl(v_l + v_{l + off}) where l + off is in the chunk and of l's row, all lanes at once;
    the run heads are the pieces (row, chunk); a row's pieces of one tile are added in chunk order,
    its tile sums in tile order."""
    f4 = np.float32
    assert tile % CHUNK == 0
    row = row.astype(np.int64)
    n_rows, n = row.shape[0] - 1, int(row[-1])
    out = np.zeros(n_rows, f4)
    if n == 0:
        return out
    v = gather(id, np.asarray(a, f4), np.asarray(c, f4)).astype(f4) * w.astype(f4)
    assert v.dtype == f4
    cell = np.repeat(np.arange(n_rows), np.diff(row))
    pad = -n % CHUNK
    K = np.concatenate([cell, np.full(pad, -1)]).reshape(-1, CHUNK)
    V = np.concatenate([v, np.zeros(pad, f4)]).reshape(-1, CHUNK)
    for off in (1, 2, 4, 8, 16, 32):
        same = K[:, :-off] == K[:, off:]
        V[:, :-off] = np.where(same, V[:, :-off] + V[:, off:], V[:, :-off])
    K, V = K.ravel(), V.ravel()
    pos = np.arange(K.shape[0])
    head = np.nonzero((K >= 0) & ((pos % CHUNK == 0) | (K != np.roll(K, 1))))[0]
    total = {}     # row -> the sum of its finished tiles
    current = {}   # row -> (tile, the sum of its pieces of that tile so far)
    for i in head:
        r, k, piece = int(K[i]), int(i) // tile, V[i]
        if r in current and current[r][0] == k:
            current[r] = (k, f4(current[r][1] + piece))
            continue
        if r in current:
            total[r] = current[r][1] if r not in total else f4(total[r] + current[r][1])
        current[r] = (k, piece)
    for r, (k, s) in current.items():
        out[r] = f4(0.0) + (s if r not in total else f4(total[r] + s))  # out starts at +0
    return out


def selftest_rows(rng, tile, n_tasks=300):
    """A hand-built index for the sum's self-test: rows of 0, 1, 0, 0, 2, 63, 64, 65 terms, a
    filler up to the first tile boundary, then tile - 1 (starts on a boundary), tile, tile + 1
    (ends on one), 3 tile + 7 (starts on one) and an empty last row; 7 tile + 7 terms.  ids with
    and without bit 31, weights spread over 2^-20 .. 2^20.  Returns row, id, w."""
    lengths = [0, 1, 0, 0, 2, 63, 64, 65, tile - 195, tile - 1, tile, tile + 1, 3 * tile + 7, 0]
    assert tile > 195 and sum(lengths) % tile != 0
    row = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
    assert row[9] == tile and row[12] == 4 * tile
    return (row,) + random_terms(rng, int(row[-1]), n_tasks)


def random_terms(rng, n, n_tasks):
    id = rng.integers(0, n_tasks, n).astype(np.uint32) | np.where(rng.random(n) < 0.3, np.uint32(FIRST), np.uint32(0))
    w = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 21, n)).astype(np.float32)
    return id, w
