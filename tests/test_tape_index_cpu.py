"""The walk tape's cell-sorted index without a GPU: the five entry points are declared in
include/wos.h, exported by the built library and bound by wos_amd._lib; the ABI version stays 10;
and the host model of tests/tape_index_model.py -- the yardstick of tests/test_gpu_tape_index.py --
holds the terms of tape_adjoint_model.adjoint, and its ordered float32 sum depends on the order."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import tape_adjoint_model as tm
import tape_index_model as im
import wos_amd
from wos_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "wos.h")
INDEX_API = ("wos_tape_index_build", "wos_tape_index_get_info", "wos_tape_index_read", "wos_tape_vjp_indexed",
             "wos_selftest_tape_rowsum")


def test_index_entry_points_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(wos_[a-z0-9_]+)\s*\(", txt))
    assert set(INDEX_API) <= declared
    L = wos_amd.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (wos_[a-z0-9_]+)$", out, flags=re.M))
    for name in INDEX_API:
        assert name in exported and name in _lib.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes, name
    assert "selftest_tape_rowsum" in wos_amd.__all__ and callable(wos_amd.selftest_tape_rowsum)


def test_abi_version_stays_10():
    assert wos_amd.load_library().wos_abi_version() == _lib.ABI_VERSION == 10
    assert re.search(r"#define WOS_ABI_VERSION 10\b", open(HEADER).read())


def test_info_struct_and_field_ids_mirror_the_header():
    txt = open(HEADER).read()
    assert txt.index("} wos_tape_field;") < txt.index("typedef enum wos_tape_index_field")  # a new enum, after the old
    body = re.search(r"typedef enum wos_tape_index_field \{(.*?)\} wos_tape_index_field;", txt, flags=re.S).group(1)
    ids = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"WOS_TAPE_INDEX_([A-Z0-9_]+) = (\d+)", body)}
    assert ids == {k: v[0] for k, v in _lib.TAPE_INDEX_FIELDS.items()}
    assert {"row", "id", "w"} <= set(ids)
    body = re.search(r"typedef struct wos_tape_index_info \{(.*?)\} wos_tape_index_info;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = []
    for typ, names in re.findall(r"(int32_t|int64_t)\s+([^;]+);", body):
        members += [(n.strip(), C.c_int32 if typ == "int32_t" else C.c_int64) for n in names.split(",")]
    assert members == list(_lib.TapeIndexInfo._fields_)
    assert [n for n, _ in members] == ["built", "n_segments", "n_terms", "n_cells", "max_terms_per_cell", "bytes",
                                       "tile_terms"]


def test_null_arguments_are_invalid_without_a_device():
    L = wos_amd.load_library()
    buf = np.zeros(4, np.float32)
    info = _lib.TapeIndexInfo()
    tile = C.c_int32(0)
    calls = {
        "wos_tape_index_build": lambda: L.wos_tape_index_build(None, 0),
        "wos_tape_index_get_info": lambda: L.wos_tape_index_get_info(None, C.byref(info)),
        "wos_tape_index_read": lambda: L.wos_tape_index_read(None, 0, 0, 0, 1, buf.ctypes.data),
        "wos_tape_vjp_indexed": lambda: L.wos_tape_vjp_indexed(None, None, 1, buf.ctypes.data, None, buf.ctypes.data,
                                                                None, None, 0),
        "wos_selftest_tape_rowsum": lambda: L.wos_selftest_tape_rowsum(None, 1, None, None, None, None, 1, 1, None,
                                                                        C.byref(tile), 0),
    }
    assert set(calls) == set(INDEX_API)
    for name, call in calls.items():
        assert call() == -1, name
        assert name.encode() in L.wos_last_error(), (name, L.wos_last_error())
    assert tile.value > 0 and tile.value % im.CHUNK == 0  # the tile constant comes back even so


def _upstream(rng, n, dim):
    return rng.standard_normal(n), rng.standard_normal((n, dim))


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("n_anti", [1, 2])
@pytest.mark.parametrize("use_cv", [True, False])
def test_index_holds_the_adjoints_terms(dim, n_anti, use_cv):
    """The model's index (thr nrm formed exactly, in float64) summed per row in float64 is
    tape_adjoint_model.adjoint.  Pure float64 and fewer than 1e4 terms per cell, so 1e-12 relative
    to the cell's absolute mass M is a hundred times k 2^-53 (as test_model_is_a_transpose_pair)."""
    rng = np.random.default_rng(200 * dim + 20 * n_anti + use_cv)
    cells, wpp = 35, 6 * n_anti
    segs = [tm.synthetic_segment(rng, dim, 7, wpp, cells), tm.synthetic_segment(rng, dim, 4, wpp, cells)]
    prm = {"dim": dim, "wpp": wpp, "n_anti": n_anti, "use_cv": use_cv, "ignore_source": False}
    P, G = _upstream(rng, 11, dim)
    ref, M, k = tm.adjoint(segs, P, G, prm, cells)
    rec = np.concatenate([(s["code"] & 1) != 0 for s in segs])
    assert 0 < rec.sum() < rec.size and np.count_nonzero(ref) > cells // 2  # dropped walks, a reached grid
    got, b0 = np.zeros(cells), 0
    for seg in segs:
        nb = seg["pstate"].shape[0]
        a, c = tm.adjoint_records(seg, P[b0:b0 + nb], G[b0:b0 + nb], prm)
        b0 += nb
        row, id, w, cell = im.index(seg, cells, np.float64)
        got += im.rowsum64(row, id, w, a, c)
        # the structure: sorted by cell, first balls before entries and both by task within a cell
        assert row[0] == 0 and row[-1] == id.size == w.size and np.all(np.diff(row.astype(np.int64)) >= 0)
        assert np.array_equal(cell, np.repeat(np.arange(cells), np.diff(row.astype(np.int64))))
        for r in range(cells):
            ids = id[row[r]:row[r + 1]].astype(np.int64)
            first = (ids & im.FIRST) != 0
            assert np.all(np.diff(first.astype(int)) <= 0) and np.all(np.diff(ids[first]) > 0)
            assert np.all(np.diff(ids[~first]) >= 0)
        # the float32 index differs from it in w's single rounding only
        row32, id32, w32, _ = im.index(seg, cells)
        assert w32.dtype == np.float32 and np.array_equal(row32, row) and np.array_equal(id32, id)
        assert np.array_equal(w32, w.astype(np.float32))
    assert np.all(np.abs(got - ref) <= 1e-12 * M), float(np.max(np.abs(got - ref) / np.maximum(M, 1e-300)))
    # terms of dead points are in the index with a = c = 0; with ignore_source the index is not used
    assert int(np.sum(k)) <= sum(int(im.index(s, cells)[0][-1]) for s in segs)


def test_index_drops_cells_beyond_the_grid():
    rng = np.random.default_rng(3)
    seg = tm.synthetic_segment(rng, 2, 5, 4, 35)
    full = im.index(seg, 35)
    cut = im.index(seg, 20)
    assert cut[0].size == 21 and cut[0][-1] < full[0][-1]
    assert np.array_equal(cut[0], full[0][:21]) and np.array_equal(cut[1], full[1][:cut[0][-1]])


def _rows(rng, tile):
    row, id, w = im.selftest_rows(rng, tile)
    return row, id, w, rng.standard_normal(300).astype(np.float32), rng.standard_normal(300).astype(np.float32)


@pytest.mark.parametrize("tile", [256, 1024])
def test_ordered_float_sum_is_close_and_has_teeth(tile):
    """The ordered float32 sum is within k 2^-24 M of the float64 sum, and it is a function of the
    order: with every row's terms reversed at least one row's bits change, so the bit comparison
    of tests/test_gpu_tape_index.py against this model cannot pass by accident."""
    rng = np.random.default_rng(tile)
    row, id, w, a, c = _rows(rng, tile)
    got = im.rowsum(row, id, w, a, c, tile)
    assert got.dtype == np.float32 and got.shape == (row.size - 1,)
    r64 = row.astype(np.int64)
    k = np.diff(r64)
    ref = im.rowsum64(row, id, w, a, c)
    M = im.rowsum64(row, id, np.abs(w), np.abs(a), np.abs(c))
    assert np.all(np.abs(got - ref) <= (k + 1) * 2.0 ** -24 * M)
    assert not np.any(got[k == 0]) and np.array_equal(got[k == 1], (im.gather(id, a, c) * w)[r64[:-1][k == 1]])
    rev = np.concatenate([np.arange(r64[r], r64[r + 1])[::-1] for r in range(k.size)]).astype(np.int64)
    other = im.rowsum(row, id[rev], w[rev], a, c, tile)
    differ = other.view(np.uint32) != got.view(np.uint32)
    assert np.any(differ), "a reversed-order sum must differ from the model's in at least one row's bits"
    assert not np.any(differ[k <= 1])
    # ... and of the tile constant, for the rows that cross tiles (weights of one scale, so that
    # the regrouped partial sums are not all absorbed by a few large terms)
    w1 = rng.standard_normal(w.size).astype(np.float32)
    mine = im.rowsum(row, id, w1, a, c, tile).view(np.uint32)
    differ = np.zeros(k.size, bool)
    for other_tile in (im.CHUNK, 2 * tile, 4 * tile):
        differ |= im.rowsum(row, id, w1, a, c, other_tile).view(np.uint32) != mine
    assert np.any(differ) and not np.any(differ[k <= im.CHUNK])
