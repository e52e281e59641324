"""The walk tape's C ABI without a GPU (include/wos.h "Walk tape"): the four entry points are
declared, exported by the built library and bound by wos_amd._lib, the ABI version stays 10,
and the argument checks that need no device answer WOS_E_INVALID.  The recording and the
replay themselves: tests/test_gpu_tape.py."""
import ctypes as C
import os
import re
import subprocess

import wos_amd
from wos_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "wos.h")
TAPE_API = ("wos_tape_record", "wos_tape_solve", "wos_tape_get_info", "wos_tape_destroy")


def test_tape_entry_points_declared_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(wos_[a-z0-9_]+)\s*\(", txt))
    assert set(TAPE_API) <= declared
    L = wos_amd.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (wos_[a-z0-9_]+)$", out, flags=re.M))
    for name in TAPE_API:
        assert name in exported and name in _lib.EXPORTS and hasattr(L, name), name


def test_abi_version_stays_10():
    assert wos_amd.load_library().wos_abi_version() == _lib.ABI_VERSION == 10
    assert re.search(r"#define WOS_ABI_VERSION 10\b", open(HEADER).read())


def test_tape_info_mirrors_the_header():
    """wos_tape_info's members in the header's order, as wos_amd._lib.TapeInfo declares them."""
    txt = open(HEADER).read()
    body = re.search(r"typedef struct wos_tape_info \{(.*?)\} wos_tape_info;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*\]", "", n).strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [n for n, _ in _lib.TapeInfo._fields_]
    assert C.sizeof(_lib.TapeInfo) == 6 * 4 + 5 * 8 + 8  # the trailing int32 padded to the int64 alignment


def test_null_arguments_are_invalid_without_a_device():
    L = wos_amd.load_library()
    h = C.c_void_p()
    assert L.wos_tape_record(None, None, None, 0, 0, 1, 0, C.byref(h), None, None, 0) == -1
    assert b"wos_tape_record" in L.wos_last_error()
    assert L.wos_tape_solve(None, None, 1, None, None, None, None, None, None, None, None, 0) == -1
    assert b"wos_tape_solve" in L.wos_last_error()
    assert L.wos_tape_get_info(None, None) == -1
    assert L.wos_tape_destroy(None) == 0
