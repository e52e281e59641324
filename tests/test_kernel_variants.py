"""CPU check of the one place that chooses the first-ball and walk kernel instantiations
(csrc/wos_variant.h kernel_variant, built here with plain g++ through
tests/native/host_scene_shim.cpp).  Every schedule choice leaves results bit-identical, so no
GPU test can see a wrong choice; this one enumerates all of them against the rules as they
stood in the hand-written launchers before the table:

* first ball  <dim, robust, 4 channels if the scene holds several else 1>;
* walk, solve, robust      <dim, GG, false, true, NEU = true, SPR = false, NC>;
* walk, solve, not robust  <dim, GG, false, false, NEU = !neumann_inert,
                            SPR = 2D and LDS geometry and tail_spread, NC>;
* walk, boundary start     2D and one channel only: <2, GG, true, robust, true, false, 1>.
"""
import ctypes as C
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "neural-monte-carlo-fluid-simulation_amd", "csrc")
MAX_CHANNELS = 4  # csrc/wos_scene.h kMaxChannels


@pytest.fixture(scope="module")
def variants(tmp_path_factory):
    """{(dim, robust, n_channels, geom_global, neumann_inert, tail_spread, bstart):
        (dim, geom_global, bstart, robust, neumann, spread, channels, valid)} over the full product."""
    out = str(tmp_path_factory.mktemp("kv") / "libhs.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-I", CSRC,
                    os.path.join(HERE, "native", "host_scene_shim.cpp"), os.path.join(CSRC, "wos_host_scene.cpp"),
                    os.path.join(CSRC, "wos_fcpw_bvh.cpp"), "-o", out], check=True)
    shim = C.CDLL(out)
    table = {}
    for key in itertools.product((2, 3), (0, 1), (1, 2, 4), (0, 1), (0, 1), (0, 1), (0, 1)):
        r = (C.c_int * 8)()
        shim.hs_kernel_variant(*key, r)
        table[key] = tuple(r)
    assert len(table) == 2 * 2 * 3 * 2 * 2 * 2 * 2  # 192
    return table


def test_header_is_host_only():
    """wos_variant.h compiles on its own with plain g++ (it includes wos_scene.h, which needs <stdint.h> only)."""
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, "-x", "c++", "-"],
                   input=b'#include "wos_variant.h"\n', check=True)


def test_every_combination(variants):
    for (dim, robust, nch, gg, inert, spread, bstart), got in variants.items():
        nc = MAX_CHANNELS if nch > 1 else 1
        if bstart:
            if dim != 2 or nch != 1:
                assert got[7] == 0, (dim, robust, nch, gg, inert, spread, bstart)
                continue
            want = (2, gg, 1, robust, 1, 0, 1, 1)
        elif robust:
            want = (dim, gg, 0, 1, 1, 0, nc, 1)
        else:
            want = (dim, gg, 0, 0, 0 if inert else 1, 1 if (dim == 2 and not gg and spread) else 0, nc, 1)
        assert got == want, (dim, robust, nch, gg, inert, spread, bstart)


def test_instantiation_counts(variants):
    valid = [v for v in variants.values() if v[7]]
    walks = {v[:7] for v in valid}  # <DIM, GG, BSTART, RB, NEU, SPR, NC>
    first_balls = {(v[0], v[3], v[6]) for v in valid if not v[2]}  # <DIM, RB, NC>; boundary start has none
    assert len(walks) == 32
    assert len(first_balls) == 8
    # tail spread: only <2, false, false, false, NEU, true, NC>; robust and boundary start: full Neumann, no spread
    assert {v for v in walks if v[5]} == {(2, 0, 0, 0, neu, 1, nc) for neu in (0, 1) for nc in (1, MAX_CHANNELS)}
    assert all(v[4] == 1 and v[5] == 0 for v in walks if v[2] or v[3])


def test_boundary_start_is_2d_single_channel(variants):
    for (dim, robust, nch, gg, inert, spread, bstart), got in variants.items():
        if bstart:
            assert bool(got[7]) == (dim == 2 and nch == 1)
        else:
            assert got[7] == 1
