"""Express layout (include/wos.h wos_set_express_layout; DESIGN.md, Length hints), the parts that need no GPU.
The walk kernel and wos_selftest_express_slot share one mapping (csrc/wos_scene.h express_slot): claim c, position
j -> entry of the express list.  An entry lost or handed out twice is not a scheduling matter (a lost walk leaves a
stale record), so the whole table is walked: every list length 0..300, every solo tier 0..nx, both stripe modes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import wos_amd
from wos_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wos.h")
NAMES = ("wos_set_express_layout", "wos_get_express_layout", "wos_express_layout_stats", "wos_selftest_express_slot",
         "wos_selftest_simd_ids")


@pytest.mark.parametrize("stripe", [0, 1])
@pytest.mark.parametrize("epw", [1, 2, 3, 4, 8, 64])
def test_every_entry_exactly_once(epw, stripe):
    for nx in range(0, 301):
        # rows (n_solo, claim, j, entry) over n_solo 0..nx, claims 0..nx+1, j 0..epw+1: everything that is not "none"
        t = wos_amd.selftest_express_slot(nx, epw, stripe).astype(np.int64)
        ns, c, j, e = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
        assert len(t) == (nx + 1) * nx, (nx, len(t))  # nx entries under each of the nx + 1 solo tiers: nothing else
        if nx == 0:
            continue
        assert e.min() >= 0 and e.max() < nx and ns.max() <= nx
        # each entry of [0, nx) exactly once under every solo tier
        assert (np.bincount(ns * nx + e, minlength=(nx + 1) * nx) == 1).all(), nx
        # the non-empty claims: the solo tier's, then ceil((nx - n_solo) / epw)
        claims = np.unique(ns * (nx + 2) + c)
        per = np.bincount(claims // (nx + 2), minlength=nx + 1)
        k = np.arange(nx + 1)
        np.testing.assert_array_equal(per, k + (nx - k + epw - 1) // epw, err_msg=str(nx))
        # a claim's entries sit at j = 0 .. n - 1 (the walk kernel counts them and fills the ring from 0)
        key = ns * (nx + 2) + c
        cnt = np.bincount(key)
        assert (j < cnt[key]).all() and j.max() < epw, nx
        # the solo tier: claim c holds entry c alone; below it the longest walks first, one of each band when striped
        solo = c < ns
        assert (e[solo] == c[solo]).all() and (j[solo] == 0).all() and (e[~solo] >= ns[~solo]).all(), nx
        G = (nx - ns + epw - 1) // epw
        i = c - ns
        want = np.where(solo, c, ns + (i + j * G if stripe else i * epw + j))
        np.testing.assert_array_equal(e, want, err_msg=str(nx))


def test_symbols_and_abi():
    L = wos_amd.load_library()
    txt = open(HEADER).read()
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.EXPORTS, name
        assert re.search(r"\b%s\(" % name, txt), name
    for name in ("set_express_layout", "express_layout", "express_layout_stats", "selftest_express_slot",
                 "selftest_simd_ids"):
        assert name in wos_amd.__all__ and callable(getattr(wos_amd, name)), name
    assert L.wos_abi_version() == 10 == _lib.ABI_VERSION
    assert re.search(r"#define WOS_ABI_VERSION 10\b", txt)


def test_setter_clamps_without_a_device():
    wos_amd.set_express_layout()
    default = wos_amd.express_layout()
    assert 0 <= default["solo_min"] <= 1023 and default["stripe"] in (0, 1) and default["placement"] in (0, 1)
    try:
        wos_amd.set_express_layout(80, 1, 1)
        assert wos_amd.express_layout() == {"solo_min": 80, "stripe": 1, "placement": 1}
        wos_amd.set_express_layout(0, 0, 0)  # 0: no solo tier, blocks, rotating
        assert wos_amd.express_layout() == {"solo_min": 0, "stripe": 0, "placement": 0}
        wos_amd.set_express_layout(10 ** 9, 10 ** 9, 10 ** 9)  # clamped, never refused
        assert wos_amd.express_layout() == {"solo_min": 1023, "stripe": 1, "placement": 1}
        wos_amd.set_express_layout(-1, 0, -7)  # a negative value: that one's default
        assert wos_amd.express_layout() == {"solo_min": default["solo_min"], "stripe": 0,
                                            "placement": default["placement"]}
        wos_amd.set_length_hints(8, 16, 4, 100, 3)  # the other setter leaves the layout alone
        assert wos_amd.express_layout()["stripe"] == 0
    finally:
        wos_amd.set_express_layout()
        wos_amd.set_length_hints()
    assert wos_amd.express_layout() == default
    # no solve ran on the device (or there is none): all zero, no error
    out = (C.c_int64 * 2)(7, 7)
    assert wos_amd.load_library().wos_express_layout_stats(63, out) == 0 and list(out) == [0, 0]
    assert wos_amd.load_library().wos_express_layout_stats(-1, out) != 0
