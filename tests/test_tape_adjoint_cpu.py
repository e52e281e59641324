"""The walk tape's adjoint without a GPU: wos_tape_vjp and wos_tape_read are declared in
include/wos.h, exported by the built library and bound by wos_amd._lib; the ABI version stays 10;
and the host model of tests/tape_adjoint_model.py -- the yardstick of tests/test_gpu_tape_adjoint.py
-- is a transpose pair: <Y, A f> = <A^T Y, f> on hand-built tapes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import tape_adjoint_model as tm
import wos_amd
from wos_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "wos.h")
ADJOINT_API = ("wos_tape_vjp", "wos_tape_read")


def test_adjoint_entry_points_declared_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(wos_[a-z0-9_]+)\s*\(", txt))
    assert set(ADJOINT_API) <= declared
    L = wos_amd.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (wos_[a-z0-9_]+)$", out, flags=re.M))
    for name in ADJOINT_API:
        assert name in exported and name in _lib.EXPORTS and hasattr(L, name), name


def test_abi_version_stays_10():
    assert wos_amd.load_library().wos_abi_version() == _lib.ABI_VERSION == 10
    assert re.search(r"#define WOS_ABI_VERSION 10\b", open(HEADER).read())


def test_field_ids_mirror_the_header():
    body = re.search(r"typedef enum wos_tape_field \{(.*?)\} wos_tape_field;", open(HEADER).read(), flags=re.S).group(1)
    ids = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"WOS_TAPE_([A-Z0-9_]+) = (\d+)", body)}
    assert ids.pop("segment_points") == _lib.TAPE_SEGMENT_POINTS
    mine = {("e_" + k if k in ("cell", "thr", "nrm") else k): v[0] for k, v in _lib.TAPE_FIELDS.items()}
    assert mine == ids
    assert set(_lib.TAPE_FIELDS) == set(tm.FIELDS)


def test_null_arguments_are_invalid_without_a_device():
    L = wos_amd.load_library()
    buf = np.zeros(4, np.float32)
    assert L.wos_tape_vjp(None, None, 1, buf.ctypes.data, None, buf.ctypes.data, None, None, 0) == -1
    assert b"wos_tape_vjp" in L.wos_last_error()
    assert L.wos_tape_read(None, 0, 0, 0, 1, buf.ctypes.data) == -1
    assert b"wos_tape_read" in L.wos_last_error()


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("n_anti", [1, 2])
@pytest.mark.parametrize("use_cv", [True, False])
def test_model_is_a_transpose_pair(dim, n_anti, use_cv):
    """Pure float64 and fewer than 1e4 terms per inner product, so 1e-12 relative is a hundred
    times k 2^-53.  Relative to sum |Y| |A f|, which bounds both sides' rounding."""
    rng = np.random.default_rng(100 * dim + 10 * n_anti + use_cv)
    cells, wpp = 35, 6 * n_anti  # several pairs
    segs = [tm.synthetic_segment(rng, dim, 7, wpp, cells), tm.synthetic_segment(rng, dim, 4, wpp, cells)]
    prm = {"dim": dim, "wpp": wpp, "n_anti": n_anti, "use_cv": use_cv, "ignore_source": False}
    n = 11
    rec = np.concatenate([(s["code"] & 1) != 0 for s in segs])
    assert 0 < rec.sum() < rec.size and sum(int(tm._walks(s)[2].sum()) for s in segs) > 30
    f = rng.standard_normal(cells)
    P, G = rng.standard_normal(n), rng.standard_normal((n, dim))
    p1, g1, n_est = tm.forward(segs, f, prm, np.float64)
    p0, g0, _ = tm.forward(segs, np.zeros(cells), prm, np.float64)
    assert n_est[0] == n_est[7] == 0 and np.all(np.delete(n_est, [0, 7]) > 0) and np.any(n_est < wpp)
    lhs = np.dot(P, p1 - p0) + np.sum(G * (g1 - g0))
    AtY, M, k = tm.adjoint(segs, P, G, prm, cells)
    rhs = np.dot(AtY, f)
    scale = np.dot(np.abs(f), M)
    assert scale > 0 and np.count_nonzero(AtY) > cells // 2
    assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs, scale)
    # the masks: p of point 1 and the gradient of point 2 do not depend on their upstream
    P2, G2 = P.copy(), G.copy()
    P2[0], G2[0], P2[1], G2[2] = 7.0, -3.0, 5.0, 9.0
    P2[7], G2[7], P2[8], G2[9] = 7.0, -3.0, 5.0, 9.0  # the same points of the second segment
    again = tm.adjoint(segs, P2, G2, prm, cells)[0]
    assert np.array_equal(again, AtY)
    # with ignore_source the map does not depend on the grid
    off = dict(prm, ignore_source=True)
    assert not np.any(tm.adjoint(segs, P, G, off, cells)[0])
    a, b = tm.forward(segs, f, off, np.float64), tm.forward(segs, np.zeros(cells), off, np.float64)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
