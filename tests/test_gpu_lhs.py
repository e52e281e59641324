"""The first-ball kernel's stratified sampler, probed on the device (wos_selftest_lhs,
wos_selftest_lhs_permute) and compared bit for bit with the oracle's sequential
generateStratifiedSamples (oracle_lhs; sampling.h:435-457) and with the plain swap loop.

The sampler picks its code by the strata count alone: four shuffles (registers with one or two
64-lane chunks, pointer jumping in LDS, lane 0's loop), the packed 3D one-pass forms, one to
four points per wave, LDS-staged or global jump constants, and the replay of the partners when a
bounded draw hits PCG32's rejection threshold.  The probes run the kernel's own device functions
on the kernel's LDS layout, so each branch is pinned without a solve around it."""
import numpy as np
import pytest

import lhs_cases
from wos_amd import _lib, selftest_lhs, selftest_lhs_permute, selftest_lhs_permute_slots

pytestmark = pytest.mark.gpu

NSTRAT_ALL = list(range(2, 321, 2)) + [384, 512, 600, 1100]


def _oracle_lhs(oracle, key, gidx, nstrat, dims):
    return np.stack([oracle.lhs(oracle.seed32(key, int(i), 0, 0), nstrat, dims) for i in gidx]).reshape(
        len(gidx), nstrat, dims)


@pytest.mark.parametrize("jump_lds", [1, 0])
@pytest.mark.parametrize("dim", [2, 3])
def test_every_even_nstrat_bit_exact(gpu, oracle, dim, jump_lds):
    """Every even strata count 2..320 and 384, 512, 600, 1100: 8 point indices each (small,
    beyond 2^31 and beyond 2^40; 8 is no multiple of the 3 points a wave packs for 17..21
    pairs), jump constants staged in LDS as a solve stages them, and all from the global table."""
    for nstrat in NSTRAT_ALL:
        gidx = np.array([0, 1, 2, 3 + nstrat, 65537 * nstrat, 2**31 + 5 + nstrat, 2**40 + 7, 2**40 + 8 + nstrat],
                        np.int64)
        got = selftest_lhs(lhs_cases.KEY, gidx, nstrat // 2, dim, jump_lds=jump_lds)
        want = _oracle_lhs(oracle, lhs_cases.KEY, gidx, nstrat, dim - 1)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=f"nstrat {nstrat}")


@pytest.mark.parametrize("jump_lds", [1, 0])
@pytest.mark.parametrize("nstrat,dims", sorted(lhs_cases.REPLAY))
def test_replay_indices_bit_exact(gpu, oracle, nstrat, dims, jump_lds):
    """Point indices whose shuffle draws reject (tests/test_lhs_cpu.py shows they do), each with
    its two neighbours, which do not: the wave's lane 0 redraws every partner of that point from
    the sequential stream, and only of that point."""
    for idx in lhs_cases.REPLAY[(nstrat, dims)]:
        gidx = np.array([idx - 1, idx, idx + 1], np.int64)
        got = selftest_lhs(lhs_cases.KEY, gidx, nstrat // 2, dims + 1, jump_lds=jump_lds)
        want = _oracle_lhs(oracle, lhs_cases.KEY, gidx, nstrat, dims)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=f"index {idx}")


# ---------------------------------------------------------------------------------------------
# injected partner tables
# ---------------------------------------------------------------------------------------------
NSTRAT_TABLES = [2, 62, 64, 66, 126, 128, 130, 190, 192, 194, 254, 256]
IMPL_MAX = {_lib.LHS_REG1: 64, _lib.LHS_REG2: 128, _lib.LHS_LDS: 256, _lib.LHS_PACK_R1: 64, _lib.LHS_PACK_R2: 128}
N_RANDOM = 200


def partner_tables(n, rng):
    """[6 + N_RANDOM, n] valid tables (partner[j] in [j, n)): identity; the chain j -> j + 1
    (a link chain of length n: the most pointer-jumping rounds); every step onto n - 1 (one
    target: pred and last cross the 64-lane chunks); j + 64 and j + 63 clamped (targets exactly
    across a chunk edge); fixed points alternating with movers; random tables."""
    j = np.arange(n)
    t = [j, np.minimum(j + 1, n - 1), np.full(n, n - 1), np.minimum(j + 64, n - 1), np.minimum(j + 63, n - 1),
         np.where(j % 2 == 0, j, j + rng.integers(0, 1 << 30, n) % (n - j))]
    t += [j + rng.integers(0, 1 << 30, n) % (n - j) for _ in range(N_RANDOM)]
    return np.stack(t).astype(np.int32)


def swap_loop(values, partner):
    """for i in dims: for j in range(n): swap(a[j, i], a[partner[i][j], i]) -- on every table
    at once.  values [count, n, sd], partner [count, sd, n]."""
    a = values.copy()
    rows = np.arange(a.shape[0])
    for i in range(a.shape[2]):
        for j in range(a.shape[1]):
            o = partner[:, i, j]
            t = a[:, j, i].copy()
            a[:, j, i] = a[rows, o, i]
            a[rows, o, i] = t
    return a


@pytest.mark.parametrize("impl", sorted(IMPL_MAX))
def test_injected_partner_tables(gpu, impl):
    """Each shuffle implementation against the plain swap loop on adversarial and random tables,
    at the strata counts around every 64-lane chunk edge it can hold.  Two dimensions and the
    packed forms' slots each get a different table; unused slots must come back untouched."""
    packed = impl in (_lib.LHS_PACK_R1, _lib.LHS_PACK_R2)
    cap = selftest_lhs_permute_slots(impl)
    rng = np.random.default_rng(1000 + impl)
    for n in [n for n in NSTRAT_TABLES if n <= IMPL_MAX[impl]]:
        base = partner_tables(n, rng)
        count = base.shape[0]
        for sd in ([2] if packed else [1, 2]):
            # dimension i of slot s: the list of tables rolled by 7 s + 3 i, so no two agree
            partner = np.stack([np.stack([np.roll(base, 7 * s + 3 * i, axis=0) for i in range(sd)], axis=1)
                                for s in range(cap)], axis=1)
            values = rng.permutation(count * cap * n * sd).astype(np.float32).reshape(count, cap, n, sd)
            for slots in range(1, cap + 1):
                got = selftest_lhs_permute(impl, partner, values, slots=slots)
                want = values.copy()
                for s in range(slots):
                    want[:, s] = swap_loop(values[:, s], partner[:, s])
                np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32),
                                              err_msg=f"impl {impl} nstrat {n} sd {sd} slots {slots}")
