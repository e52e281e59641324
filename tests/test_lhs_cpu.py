"""The stratified-sampler tests that need no GPU: the replay candidates of the GPU tests
really reject, the full-solve sweep visits every plan of the sampler, and the permute probe
refuses what does not fit (before it touches a device)."""
import numpy as np
import pytest

import lhs_cases
import wos_amd
from wos_amd import _lib


def test_python_pcg_matches_oracle(oracle):
    for idx in (0, 1, 7, 2**31 + 5, 2**40 + 7, 2**63 + 11):
        assert lhs_cases.seed32(lhs_cases.KEY, idx, 0, 0) == oracle.seed32(lhs_cases.KEY, idx, 0, 0)
    for n, dims in ((2, 1), (5, 2), (64, 1), (66, 2)):
        s, _ = lhs_cases.lhs_python(12345 + n, n, dims)
        np.testing.assert_array_equal(s.view(np.uint32), oracle.lhs(12345 + n, n, dims).view(np.uint32))


@pytest.mark.parametrize("nstrat,dims", sorted(lhs_cases.REPLAY))
def test_replay_candidates_reject(oracle, nstrat, dims):
    """Each candidate index: some bounded draw of its shuffle falls below 2^32 mod bound (so
    the kernel must replay the partners from the sequential stream), and the oracle equals a
    Fisher-Yates in Python that honours the rejection.  The neighbours idx - 1 and idx + 1,
    which share the candidate's pack in the solves of test_gpu_first_ball_regimes.py, do not."""
    for idx in lhs_cases.REPLAY[(nstrat, dims)]:
        seed = lhs_cases.seed32(lhs_cases.KEY, idx, 0, 0)
        s, rejected = lhs_cases.lhs_python(seed, nstrat, dims)
        assert rejected > 0, idx
        np.testing.assert_array_equal(s.view(np.uint32), oracle.lhs(seed, nstrat, dims).view(np.uint32))
        for nb in (idx - 1, idx + 1):
            assert lhs_cases.lhs_python(lhs_cases.seed32(lhs_cases.KEY, nb, 0, 0), nstrat, dims)[1] == 0, nb


PLAN_KEYS = ("points_per_wave", "one_pass", "shuffle", "pair_passes", "jump_mixed", "shuffle_chunks")


def _plan(n_pairs, dim):
    p = wos_amd.selftest_lhs_plan(n_pairs, dim)
    return tuple(p[k] for k in PLAN_KEYS)


@pytest.mark.parametrize("dim", [2, 3])
def test_sweep_visits_every_plan(dim):
    """The walk counts test_gpu_first_ball_regimes.py solves against the oracle visit every
    distinct plan (points per wave, one-pass shuffle, shuffle and its chunks, pair passes,
    jump-constant path) of n_pairs 1..320, and both neighbours of every n_pairs at which the
    plan changes -- as the shipped constants give them (wos_selftest_lhs_plan)."""
    swept = {lhs_cases.n_pairs_of(nw, anti) for d, nw, anti in lhs_cases.sweep_cases() if d == dim}
    plans = {n: _plan(n, dim) for n in range(1, 322)}
    missing = {plans[n] for n in range(1, 321)} - {plans[n] for n in swept if n <= 320}
    assert not missing, [dict(zip(PLAN_KEYS, m)) for m in missing]
    for n in range(1, 320):
        if plans[n] != plans[n + 1]:
            assert n in swept and n + 1 in swept, (n, dict(zip(PLAN_KEYS, plans[n])), dict(zip(PLAN_KEYS, plans[n + 1])))


def test_plan_constants():
    p = wos_amd.selftest_lhs_plan(64, 2)
    assert p["point_grab"] >= 1 and p["lds_budget"] > 4 * p["wave_lds_bytes"] > 0
    assert [wos_amd.selftest_lhs_plan(n, 3)["points_per_wave"] for n in (16, 17, 21, 22, 32, 33)] == [4, 3, 3, 2, 2, 1]
    assert [wos_amd.selftest_lhs_plan(n, 3)["one_pass"] for n in (21, 22, 32, 33, 64, 65)] == [0, 1, 1, 1, 1, 0]
    assert all(wos_amd.selftest_lhs_plan(n, 2)["one_pass"] == 0 for n in range(1, 322))


@pytest.mark.parametrize("impl,nstrat,sd,slots", [
    (_lib.LHS_REG1, 66, 1, 1), (_lib.LHS_REG2, 130, 1, 1), (_lib.LHS_LDS, 258, 1, 1), (_lib.LHS_PACK_R1, 66, 2, 1),
    (_lib.LHS_PACK_R2, 130, 2, 1), (_lib.LHS_PACK_R1, 64, 2, 3), (_lib.LHS_PACK_R2, 128, 2, 2),
    (_lib.LHS_PACK_R1, 64, 1, 1), (_lib.LHS_SERIAL, 64, 1, 1), (_lib.LHS_REG1, 64, 3, 1)])
def test_permute_probe_refuses_what_does_not_fit(impl, nstrat, sd, slots):
    cap = wos_amd.selftest_lhs_permute_slots(impl)
    partner = np.tile(np.arange(nstrat, dtype=np.int32), (1, cap, sd, 1))
    values = np.zeros((1, cap, nstrat, sd), np.float32)
    with pytest.raises(wos_amd.WosError, match="wos_selftest_lhs_permute"):
        wos_amd.selftest_lhs_permute(impl, partner, values, slots=slots)


def test_permute_probe_refuses_bad_partner():
    partner = np.arange(8, dtype=np.int32).reshape(1, 1, 1, 8).copy()
    partner[0, 0, 0, 3] = 2  # below its own step
    with pytest.raises(wos_amd.WosError, match="partner out of range"):
        wos_amd.selftest_lhs_permute(_lib.LHS_REG1, partner, np.zeros((1, 1, 8, 1), np.float32))
    partner[0, 0, 0, 3] = 8
    with pytest.raises(wos_amd.WosError, match="partner out of range"):
        wos_amd.selftest_lhs_permute(_lib.LHS_REG1, partner, np.zeros((1, 1, 8, 1), np.float32))
