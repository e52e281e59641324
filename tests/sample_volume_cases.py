"""The balls, streams and lane masks of the source-sample tests (tests/test_sample_volume_cpu.py,
tests/test_gpu_sample_volume.py; DESIGN.md "Source-sample probe").  numpy only.

An item is (R, lambda, yukawa, c[3], dir[3]) with a 32-bit stream seed (include/wos.h WOS_SV_ITEM,
oracle/wos_oracle.h ORACLE_SV_ITEM).  A case holds at most 4096 items and few distinct balls, many
streams each: the accept test of tests/sample_volume_model.py judges a ball's iterations together.
"""
import functools

import numpy as np

ITEM = 9
MAX_ITEMS = 4096
LAMBDAS = (10.0, 50.0, 350.0)
SLOW_MIN_LONG, SLOW_MIN_LIMIT = 64, 16  # items beyond the LDS jump table (> 128 iterations), items at 1000
LONG_ITERS, LIMIT = 128, 1000


def _dirs(dim, n, rng):
    v = rng.standard_normal((n, 3))
    v[:, dim:] = 0.0
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v.astype(np.float32)


def _case(dim, balls, n, seed):
    """n items cycling through balls [(R, lambda, yukawa)]: neighbouring lanes hold different balls."""
    assert n <= MAX_ITEMS
    rng = np.random.default_rng(seed)
    b = np.asarray(balls, np.float64)
    it = np.zeros((n, ITEM), np.float32)
    it[:, :3] = b[np.arange(n) % len(b)]
    c = rng.uniform(-1.0, 1.0, (n, 3))
    c[:, dim:] = 0.0
    it[:, 3:6] = c
    it[:, 6:9] = _dirs(dim, n, rng)
    seeds = (np.uint32(0x51ED2701 + 977 * seed) + np.arange(n, dtype=np.uint32) * np.uint32(2654435761)).astype(np.uint32)
    return it, seeds


def _radius(mu_r, lam):
    return float(np.float32(mu_r / np.sqrt(lam)))


@functools.lru_cache(maxsize=None)
def case(name, dim):
    """(items, seeds, robust) of family `name`: robust marks the cases of the robust kernels alone."""
    if name == "ordinary":
        # mu R log-spaced from 3e-3 to 60, six radii per lambda
        balls = [(_radius(m, lam), lam, 1) for lam in LAMBDAS for m in np.geomspace(3e-3, 60.0, 6)]
        return _case(dim, balls, 4096, 1 + dim) + (False,)
    if name == "slow":
        lam = 350.0
        if dim == 3:
            # the float norm cancels to <= 0 (mu R = 3e-3, 3e-4: loops to the limit), to positive noise
            # (1e-3: long loops), the near-wall ball at the minimum star radius, and the long loops of mu R = 60
            mus = (3e-3, 3e-4, 1e-3, 2e-3, 60.0)
        else:
            # the 2D analogue: below mu R = 4.9e-4 the float I0(mu R) is 1 and the float norm the constant
            # (1 - 2 pi fl(1 / 2 pi)) / lambda > 0, too large by (4e-8 / lambda) / (R^2 / 4): loops grow as the
            # ball shrinks and reach the limit near mu R = 2e-5
            mus = (2e-5, 1e-5, 5e-5, 1e-4, 60.0)
        balls = [(_radius(m, lam), lam, 1) for m in mus] + [(1e-3, lam, 1)]
        return _case(dim, balls, 1024, 11 + dim) + (False,)
    if name == "mixed":
        if dim == 2:  # lambda = 350, R alternating across mu R = 80
            return _case(dim, [(4.0, 350.0, 1), (4.5, 350.0, 1)], 1024, 21) + (False,)
        # the robust kernels: scaled (mu R > 80) and unscaled balls alternating
        return _case(dim, [(4.0, 350.0, 1), (4.5, 350.0, 1), (0.5, 350.0, 1), (6.0, 350.0, 1)], 1024, 23) + (True,)
    if name == "mixed_dense":
        # three lanes in four on the fast path: a full wave is dense (own generation) with fallback lanes beside
        if dim == 2:
            return _case(dim, [(4.0, 350.0, 1), (0.5, 350.0, 1), (4.5, 350.0, 1), (2.0, 350.0, 1)], 1024, 25) + (False,)
        return _case(dim, [(4.0, 350.0, 1), (0.5, 350.0, 1), (4.5, 350.0, 1), (2.0, 350.0, 1)], 1024, 27) + (True,)
    if name == "harmonic":
        return _case(dim, [(0.05, 350.0, 0), (0.5, 350.0, 0), (2.0, 350.0, 0)], 1024, 31 + dim) + (False,)
    raise KeyError(name)


FAMILIES = ("ordinary", "slow", "mixed", "mixed_dense", "harmonic")


def distribution_ball(dim, mu_r, n=65536):
    """One ball at lambda = 50 and n streams with consecutive seeds."""
    lam = 50.0
    it = np.zeros((n, ITEM), np.float32)
    it[:, 0] = _radius(mu_r, lam)
    it[:, 1] = lam
    it[:, 2] = 1
    it[:, 6] = 1
    return it, (np.uint32(1000003) + np.arange(n, dtype=np.uint32)).astype(np.uint32)


DISTRIBUTION_MU_R = (0.1, 3.0, 30.0)


# ---- lane masks -------------------------------------------------------------------------------------
def _low(n):
    return (1 << n) - 1 if n < 64 else (1 << 64) - 1


def _spread(n):
    """n lanes spread over the wave (not the low ones: ranks differ from lane numbers)."""
    lanes = sorted({(k * 64) // n for k in range(n)})
    return sum(1 << l for l in lanes)


def mask_sets(plans):
    """{name: [mask, ...]} -- one pattern of waves each, repeated over a case's items.  plans: the
    library's schedule constants (wos_selftest_sample_volume's plan) of every shipped (dim, fb), so a
    retuned sampler moves the masks with it."""
    wave = plans[0]["wave"]
    sets = {"all": [_low(wave)], "alternating": [0x5555555555555555], "empty_between": [_low(wave), 0, _low(wave)]}
    own_min = {p["own_min"] for p in plans}
    for m in sorted(own_min):
        sets[f"lanes_{m}"] = [_spread(m)]          # the own generation's threshold ...
        sets[f"lanes_{m - 1}"] = [_spread(m - 1)]  # ... and the sparse side of it
    for b in sorted({p["bmin"] for p in plans}):
        n = wave // b + 1  # nact * bmin crosses the wave: `per` goes from 1 to 2
        if 1 < n - 1 and n <= wave:
            sets[f"lanes_{n}"] = [_spread(n)]
            sets[f"lanes_{n - 1}"] = [_spread(n - 1)]
    sets["lanes_3"] = [_spread(3) << 1]  # B = wave / 3
    sets["lanes_2"] = [(1 << 5) | (1 << 58)]  # B capped
    for l in (0, 37, wave - 1):
        sets[f"solo_{l}"] = [1 << l]
    return sets


def tile(pattern, n):
    """The masks of `pattern` repeated while whole patterns fit n items; (masks uint64, items used)."""
    per = sum(bin(m).count("1") for m in pattern)
    reps = n // per
    return np.array(list(pattern) * reps, np.uint64), reps * per


def wave_of_item(masks):
    """For the items the masks name, in order: the wave index and the lane."""
    w, l = [], []
    for i, m in enumerate(masks):
        m = int(m)
        for lane in range(64):
            if (m >> lane) & 1:
                w.append(i); l.append(lane)
    return np.array(w, np.int64), np.array(l, np.int64)
