"""Length hints, the parts that need no GPU: the additive symbols and the flag (ABI still 10), the
setter's host side, and the hint key -- every field of it decides whether a list may be used."""
import ctypes as C
import os
import re

import wos_amd
from wos_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wos.h")


def test_symbols_flag_and_abi():
    L = wos_amd.load_library()
    for name in ("wos_set_length_hints", "wos_length_hint_stats", "wos_selftest_hint_key"):
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    txt = open(HEADER).read()
    for name in ("wos_set_length_hints", "wos_length_hint_stats", "wos_selftest_hint_key"):
        assert re.search(r"\b%s\(" % name, txt), name
    m = re.search(r"#define WOS_SCHED_NO_LENGTH_HINTS\s+\(?0x([0-9a-fA-F]+)u\)?", txt)
    assert m and int(m.group(1), 16) == 0x40 == _lib.SCHED_NO_LENGTH_HINTS
    others = {int(v, 16) for v in re.findall(r"#define WOS_SCHED_\w+\s+0x([0-9a-fA-F]+)u", txt)}
    assert 0x40 not in others  # a bit of its own
    assert L.wos_abi_version() == 10 == _lib.ABI_VERSION
    assert re.search(r"#define WOS_ABI_VERSION 10\b", txt)


def test_setter_and_getter_without_a_device():
    wos_amd.set_length_hints(8, 16, 4, 100, 3)
    wos_amd.set_length_hints(10 ** 9, 10 ** 9, 10 ** 9, 10 ** 9, 10 ** 9)  # clamped, never refused
    wos_amd.set_length_hints()  # the defaults
    out = (C.c_int64 * 4)(7, 7, 7, 7)
    # no solve ran on the device (or there is none): all zero, no error
    assert wos_amd.load_library().wos_length_hint_stats(63, out) == 0 and list(out) == [0, 0, 0, 0]
    assert wos_amd.load_library().wos_length_hint_stats(-1, out) != 0


def test_every_key_field_is_significant():
    fields = wos_amd.selftest_hint_key()
    # dim wpp n_walks n_anti | n index_base index_stride | seed geometry | maxWalkLength stepsBeforeTikhonov
    # stepsBeforeMaximalSpheres cosine ignoreDirichlet ignoreNeumann ignoreSource forceEstimate watertight
    # doubleSided | epsilonShell minStarRadius silhouettePrecision rouletteThreshold absorption
    assert len(fields) == 24
    assert all(fields), [k for k, f in enumerate(fields) if not f]
    assert wos_amd.load_library().wos_selftest_hint_key(-1) == -1
