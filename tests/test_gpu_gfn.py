"""The Green's-function members on the device (wos_selftest_gfn: the shipped Gfn<DIM, RB> members
and FreeSpace2, one lane per item) against the CPU oracle bit for bit, against each other where the
kernels rely on an equality, and against the 50-digit truth table under the derived bounds
(tests/gfn_model.py, tests/golden/gfn_truth.npz; DESIGN.md "Green's-function probe").  No mpmath
here: the table holds the model's values and bounds.
"""
import numpy as np
import pytest

import gfn_cases as C
import oracle_lib
from wos_amd import _lib, selftest_gfn

pytestmark = pytest.mark.gpu

_cache = {}


def device(d, mode):
    """The probe's result over rows_of(d, mode), one call per (d, mode)."""
    if (d, mode) not in _cache:
        _cache[(d, mode)] = selftest_gfn(d, mode, C.table()[f"items{d}"][C.rows_of(d, mode)])
    return _cache[(d, mode)]


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_probe_equals_oracle(d, mode):
    """Every slot of every item, bit for bit; infinities and signed zeros as they are, NaNs in the
    same places (gfn_cases.same_bits)."""
    dev = device(d, mode)
    ora = oracle_lib.gfn(d, mode, C.table()[f"items{d}"][C.rows_of(d, mode)])
    same = C.same_bits(dev, ora)
    bad = np.argwhere(~same)
    assert same.all(), (len(bad), [(int(i), int(j), float(dev[i, j]), float(ora[i, j])) for i, j in bad[:8]])


@pytest.mark.parametrize("mode", [1, 2])
def test_fused_forms_and_set_ball(mode):
    """2D reference members: evaluate_k0i0 / gradient_norm_k1i1 fed from one bessel_ik<true, true> equal
    evaluate() / gradient_norm(), and set_ball on the point-setup kernel's values leaves update_ball's
    members, bit for bit; the tag says which items take them."""
    dev = device(2, mode)
    tag1 = dev[:, 5] == 1.0
    assert tag1.sum() > 2000
    assert C.same_bits(dev[tag1][:, [15, 16]], dev[tag1][:, [6, 7]]).all()
    assert C.same_bits(dev[tag1][:, 17:22], dev[tag1][:, 0:5]).all()
    assert not dev[~tag1][:, 15:22].any()


@pytest.mark.parametrize("d", [2, 3])
def test_robust_equals_reference_below_threshold(d):
    """Every item with mu R <= 80 (the reference grid rows come first in both modes' results)."""
    T = C.table()
    rows1 = C.rows_of(d, 1)
    low = T[f"X{d}"][rows1] <= C.ROBUST_MUR
    pos2 = np.searchsorted(C.rows_of(d, 2), rows1)
    ref, rob = device(d, 1), device(d, 2)[pos2]
    assert low.sum() > 2000
    assert C.same_bits(ref[low], rob[low]).all()
    assert (rob[low][:, 5] == 1.0).all() and (device(d, 2)[:, 5][T[f"X{d}"] > C.ROBUST_MUR] == 2.0).all()


@pytest.mark.parametrize("d", [2, 3])
def test_robust_is_finite(d):
    """Every slot of every item; on the free-space sweep's rows only the free-space slots (their
    x, y lie outside the unit ball those rows carry)."""
    rob = device(d, 2)
    fin = np.isfinite(rob)
    fin[C.table()[f"kind{d}"] == 2, :26] = True
    assert fin.all(), np.argwhere(~fin)[:8]


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_probe_within_bounds_of_truth(d, mode):
    C.check_report(d, mode, C.compare(d, mode, device(d, mode)))


def test_refusals():
    L = _lib.load()
    INVALID = -1  # include/wos.h WOS_E_INVALID
    it = np.ascontiguousarray(C.table()["items2"][:4])
    out = np.zeros((4, _lib.GFN_OUT), np.float32)
    assert L.wos_selftest_gfn(2, 0, it.ctypes.data, 4, out.ctypes.data, 0) == _lib.WOS_OK
    assert L.wos_selftest_gfn(2, 0, it.ctypes.data, 0, out.ctypes.data, 0) == _lib.WOS_OK
    # n = 0 before anything touches the device: not even a device index is looked at
    assert L.wos_selftest_gfn(3, 2, it.ctypes.data, 0, out.ctypes.data, 1 << 20) == _lib.WOS_OK
    assert L.wos_selftest_gfn(2, 0, None, 4, out.ctypes.data, 0) == INVALID
    assert L.wos_selftest_gfn(2, 0, it.ctypes.data, 4, None, 0) == INVALID
    assert L.wos_selftest_gfn(2, 0, it.ctypes.data, -1, out.ctypes.data, 0) == INVALID
    for dim in (1, 4, 0):
        assert L.wos_selftest_gfn(dim, 0, it.ctypes.data, 4, out.ctypes.data, 0) == INVALID
    for mode in (-1, 3):
        assert L.wos_selftest_gfn(2, mode, it.ctypes.data, 4, out.ctypes.data, 0) == INVALID
    assert selftest_gfn(3, 1, np.zeros((0, _lib.GFN_ITEM), np.float32)).shape == (0, _lib.GFN_OUT)
