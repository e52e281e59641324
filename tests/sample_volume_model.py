"""An independent model of the source sample (sampleVolume + rejectionSampleGreensFn): the PCG32
stream in exact integer arithmetic, the replay of a reported loop, the accept test in float64 against
the mathematics, and the distribution of the accepted radius (tests/test_sample_volume_cpu.py,
tests/test_gpu_sample_volume.py; DESIGN.md "Source-sample probe").  No oracle code, no device code.

The stream
----------
PCG32 with increment 3 (initseq 1): state' = state * M + 3 mod 2^64.  seed_state is the seed rule
(0 -> step -> + seed -> step).  advance(s, k) is the LCG's closed form, s M^k + 3 (M^k - 1) / (M - 1),
with the division made exact by working modulo 2^64 (M - 1).  draw(s) is the float the generator
makes from state s: the top 23 bits of the permuted output times 2^-23, exact in float32.

The replay
----------
Iteration j of the loop takes draw 2j for u and draw 2j + 1 for the radius.  A loop that reports
iters = k stands at advance(s0, 2k), its radius is fl(draw(2k - 1) R) in float32, clamped as the
reference clamps it (max with 1e-4, then R / 2 if above R), and out = c + r dir in float32, one
rounding per operation.  All of it must equal the reported values bit for bit.

The accept test
---------------
Iteration (u, x) accepts iff u < T(r) = pdfRadius(r) / bound with r = fl(x R),
pdfRadius = G(r) |S^(d-1)| r^(d-1) / norm.  `bound` is the reference's heuristic, a handful of IEEE
float operations on R and lambda that numpy's float32 repeats exactly.  G and norm are the
mathematical functions (scipy.special, float64, in the exponentially scaled forms so that no
intermediate overflows; gfn_model's 50-digit values confirm them in the CPU test) at the float
arguments the code forms, mu r = fl(r fl(sqrt(lambda))) and mu R, as gfn_model.truth takes them.

The band
--------
The shipped test computes T in float.  Its error follows gfn_model.Err's rules node by node (a float
rounding adds u = 2^-24 relative, an A&S Bessel value a = 1e-6 relative, sums add absolute errors,
products and quotients relative ones), written here to first order in float64 with a 2 % allowance
for the dropped second-order terms, over the same expression trees as gfn_model.bounds:

  2D   q = K - I A0 / A1, each of K, I, A0, A1 an A&S value rounded to float (a + u):
       e_q = (a + u) K + (3 (a + u) + 2 u) t + u |q|,  t = I A0 / A1
  3D   e = fexp(-x) (u), e2 = e e (3u), s = (1 - e2) / 2e:
       e_s = (3u e2 + u (1 - e2)) / 2e + 2u s; A1 = sinh(mu R) the same at X, A0 = e^-X (u);
       t = A0 s / A1: e_t = t (3u + e_s / s + e_A1 / A1);  e_q = u e^-x + e_t + u |q|
  harmonic 2D   log(R / r): u (1 + |log|) + u from the quotient
  scaled (robust) balls   the same trees in double, rounded once: e_q = u |q| + 8 2^-50 e^-x (3D),
       the 2D A&S form as above
  evaluate = q / (|S| r^(d-2)) in double, rounded: e_ev = e_q / (...) + u |ev|
  the two float divisions p / pdfSphere and pdfRadius / bound, the rounding of pdfSphere and of
  ev / norm: 4u relative

This part of the band (band_small) is per iteration.  The norm is different: it is one float per
ball, (1 - |S| pk) / lambda with pk = 1 / (2 pi I0(mu R)) or mu R / (4 pi sinh(mu R)), and below
mu R ~ 0.1 the subtraction cancels: its relative error rho_n = e_pk |S| pk / |1 - |S| pk| + u reaches
4e-4 at mu R = 0.1 in 2D and 1e-2 at mu R = 0.05 in 3D, and passes 1 below mu R ~ 3e-3 (2D) and
~ 1e-2 (3D), where the float norm is rounding noise (3D: <= 0 for some balls, whose loops then run to
the limit; 2D: I0 rounds to 1 below mu R = 4.9e-4 and the norm is the constant (1 - 2 pi fl(1 / 2 pi))
/ lambda > 0).  A per-iteration band rho_n T would leave whole balls unjudged, and a family's share
of iterations in a band far above what float rounding on a 2^-23 grid of draws explains.  But the
error is the same for every iteration of a ball: the shipped test is u < kappa T(r) up to band_small
with ONE kappa per ball, |kappa - 1| <= rho_n (any kappa once rho_n >= 1).  So the model judges a
ball's iterations together: every accept gives kappa > (u - band_small) / T, every reject
kappa <= (u + band_small) / T; the ball is consistent iff these and |kappa - 1| <= rho_n leave an
interval [L, U].  One decision on the wrong side of that interval empties it.  An iteration is
"in band" -- counted, not judged -- iff its decision does not follow for every kappa in [L, U]:
a few iterations per ball next to the interval, however wide rho_n is.
"""
import numpy as np
from scipy import special as sp

M64 = (1 << 64) - 1
MULT = 0x5851F42D4C957F2D
INC = 3
LIMIT = 1000
RCLAMP = np.float32(1e-4)
ROBUST_MUR = np.float32(80.0)
U = 2.0 ** -24
UD = 2.0 ** -50
EPS_AS = 1e-6
SLACK = 1.02


# ---- the stream, exact ----------------------------------------------------------------------------
def seed_state(seed):
    s = INC  # (0 * M + 3)
    s = (s + int(seed)) & M64
    return (s * MULT + INC) & M64


def advance(s, k):
    """The state k draws after s, by the closed form."""
    big = (1 << 64) * (MULT - 1)
    mk = pow(MULT, k, big)
    return (mk * s + INC * ((mk - 1) // (MULT - 1))) & M64


def output(s):
    xs = (((s >> 18) ^ s) >> 27) & 0xFFFFFFFF
    rot = s >> 59
    return ((xs >> rot) | (xs << ((-rot) & 31))) & 0xFFFFFFFF


def draw(s):
    return np.float32((output(s) >> 9) * 2.0 ** -23)


def _draw_v(s):
    """draw over a uint64 array."""
    xs = (((s >> np.uint64(18)) ^ s) >> np.uint64(27)).astype(np.uint32)
    rot = (s >> np.uint64(59)).astype(np.uint32)
    o = (xs >> rot) | (xs << ((np.uint32(32) - rot) & np.uint32(31)))
    return ((o >> np.uint32(9)).astype(np.float64) * 2.0 ** -23).astype(np.float32)


def is_harmonic_closed_form(dim, item):
    return dim == 3 and item[2] == 0


# ---- the replay -----------------------------------------------------------------------------------
def replay(dim, item, seed, k):
    """(state, r, out[3]) after a loop of k iterations on item; r None for the 3D harmonic closed
    form (two draws, no loop: its radius goes through the float cbrt and cos)."""
    s0 = seed_state(seed)
    R = np.float32(item[0])
    if is_harmonic_closed_form(dim, item):
        return advance(s0, 2), None, None
    x = draw(advance(s0, 2 * k - 1))
    r = np.float32(x * R)
    r = max(RCLAMP, r)
    if r > R:
        r = np.float32(R / np.float32(2.0))
    out = np.zeros(3, np.float32)
    for i in range(dim):
        out[i] = np.float32(item[3 + i]) + np.float32(r * np.float32(item[6 + i]))
    return advance(s0, 2 * k), r, out


# ---- the ball -------------------------------------------------------------------------------------
def float_ball(dim, R, lam, yuk):
    """The float arguments the code forms: mu, mu R, the sampler's bound (float32, exact replay)."""
    R, lam = np.float32(R), np.float32(lam)
    sl = np.sqrt(lam, dtype=np.float32)
    X = np.float32(R * sl)
    if not yuk:
        return sl, X, np.float32(np.float32(1.5) / R)
    a, b = (np.float32(2.2), np.float32(0.6)) if dim == 2 else (np.float32(2.0), np.float32(0.5))
    aR, aL, bR, bL = a / R, a / lam, b * np.sqrt(R, dtype=np.float32), b * sl
    bound = max(max(aR, aL), max(bR, bL)) if R <= lam else max(min(aR, aL), min(bR, bL))
    return sl, X, np.float32(bound)


def on_fast_path(dim, R, lam, yuk, robust):
    """The balls sample_volume_wave samples cooperatively (the others take the sequential loop)."""
    _, X, _ = float_ball(dim, R, lam, yuk)
    if not yuk:
        return False
    return bool(X < ROBUST_MUR) if dim == 2 else not (robust and X > ROBUST_MUR)


def _sinh_parts(x):
    """(e^-x, sinh x, the error bound of the float sinh tree) at x (float64)."""
    e = np.exp(-x)
    e2 = e * e
    s = -np.expm1(-2.0 * x) / (2.0 * e)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e_s = (3 * U * e2 + U * (1 - e2)) / (2 * e) + 2 * U * s
    return e, s, e_s


def ball_norm(dim, R, lam, yuk, X):
    """(norm, rho_n): the mathematical norm at the float arguments and the relative error bound of
    the float one (inf where the analysis leaves no information)."""
    R, lam, X = float(R), float(lam), float(X)
    if not yuk:
        return R * R / (4.0 if dim == 2 else 6.0), 2 * U
    if dim == 2:
        i0e = sp.ive(0, X)  # I0 e^-X
        inv = np.exp(-X) / i0e  # |S| pk = 1 / I0(X)
        s = (sp.i0(X) - 1.0) / sp.i0(X) if X < 50 else 1.0 - inv
        e_pk = (EPS_AS + 2 * U) * inv
    else:
        inv = X / np.sinh(X) if X < 50 else 2.0 * X * np.exp(-X)  # |S| pk = X / sinh X
        # 1 - X / sinh X without cancellation: (sinh X - X) / sinh X, series below X = 0.1
        s = (X * X / 6.0 - 7.0 * X ** 4 / 360.0 + 31.0 * X ** 6 / 15120.0) if X < 0.1 else 1.0 - inv
        _, sh, e_sh = _sinh_parts(np.float64(X))
        rel = e_sh / sh if X <= float(ROBUST_MUR) + 8 else 0.0  # (scaled balls: double throughout)
        e_pk = (rel + 2 * U) * inv
    rho = SLACK * (e_pk / abs(s) + U) if s != 0 else np.inf
    return s / lam, (rho if rho < 1.0 else np.inf)


def threshold(dim, R, lam, yuk, r):
    """(T, band_small) at the float32 radii r of one ball, float64: the mathematical acceptance
    threshold and the error bound of the shipped float test without the norm's."""
    sl, X, bound = float_ball(dim, R, lam, yuk)
    nrm, _ = ball_norm(dim, R, lam, yuk, X)
    r32 = np.asarray(r, np.float32)
    x = (r32 * sl).astype(np.float64)  # mu r as the code forms it
    rr, Rd, Xd = r32.astype(np.float64), float(R), float(X)
    area = 2 * np.pi if dim == 2 else 4 * np.pi
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if not yuk:
            assert dim == 2
            lg = np.log(Rd / rr)
            ev, e_ev = lg / area, (U * (2 + np.abs(lg)) + U * np.abs(lg)) / area
        elif dim == 2:
            K = sp.k0(x)
            t = sp.ive(0, x) * (sp.kve(0, Xd) / sp.ive(0, Xd)) * np.exp(x - 2.0 * Xd)
            q = K - t
            a = EPS_AS + U
            e_q = a * K + (3 * a + 2 * U) * t + U * np.abs(q)
            ev, e_ev = q / area, e_q / area + U * np.abs(q) / area
        else:
            e, s, e_s = _sinh_parts(x)
            eX, sX, e_sX = _sinh_parts(np.float64(Xd))
            t = np.exp(x - 2.0 * Xd) * (-np.expm1(-2.0 * x)) / (-np.expm1(-2.0 * Xd))
            q = e - t
            if Xd > float(ROBUST_MUR):  # a scaled ball where robust, an underflowed one where not: not judged here
                e_q = U * np.abs(q) + 8 * UD * e
            else:
                e_q = U * e + t * (3 * U + e_s / s + e_sX / sX) + U * np.abs(q)
            ev, e_ev = q / (area * rr), e_q / (area * rr) + U * np.abs(q) / (area * rr)
        cfac = area * rr ** (dim - 1) / (nrm * float(bound))
        T = ev * cfac
        band = SLACK * (e_ev * np.abs(cfac) + 4 * U * np.abs(T))
    return T, band


def iterations(seeds, iters):
    """(item index, iteration index, u, x) of every iteration of loops of `iters` iterations."""
    seeds = np.asarray(seeds, np.uint32)
    iters = np.asarray(iters, np.int64)
    st = np.array([seed_state(s) for s in seeds], np.uint64)
    who, jj, uu, xx = [], [], [], []
    live = np.arange(seeds.size)
    m, c = np.uint64(MULT), np.uint64(INC)
    with np.errstate(over="ignore"):
        for j in range(int(iters.max()) if iters.size else 0):
            live = live[iters[live] > j]
            s = st[live]
            s1 = s * m + c
            who.append(live.copy()); jj.append(np.full(live.size, j)); uu.append(_draw_v(s)); xx.append(_draw_v(s1))
            st[live] = s1 * m + c
    cat = lambda a, t: np.concatenate(a) if a else np.zeros(0, t)
    return cat(who, np.int64), cat(jj, np.int64), cat(uu, np.float32), cat(xx, np.float32)


def judge(dim, items, seeds, iters):
    """Every ball of items judged as the module text says.  Returns a dict of counts: iterations,
    in_band, limit (loops at the limit), balls, and `bad`: the balls (R, lambda, yukawa, L, U) whose
    decisions no single kappa explains."""
    items = np.asarray(items, np.float32)
    iters = np.asarray(iters, np.int64)
    res = {"iterations": 0, "in_band": 0, "limit": int((iters == LIMIT).sum()), "balls": 0, "unbounded_norm": 0,
           "bad": []}
    keys, inv = np.unique(items[:, :3], axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    for b, (R, lam, yuk) in enumerate(keys):
        if is_harmonic_closed_form(dim, (R, lam, yuk)):
            continue
        sel = np.flatnonzero(inv == b)
        who, j, u, x = iterations(seeds[sel], iters[sel])
        k = iters[sel][who]
        r = (x * np.float32(R)).astype(np.float32)
        T, band = threshold(dim, R, lam, bool(yuk), r)
        _, X, _ = float_ball(dim, R, lam, bool(yuk))
        _, rho = ball_norm(dim, R, lam, bool(yuk), X)
        last = j == k - 1
        acc = last & (k < LIMIT)
        rej = ~last  # (the last iteration of a loop at the limit may be either: left out)
        ud = u.astype(np.float64)
        ok = np.isfinite(T) & np.isfinite(band) & (T > 0)
        lo_k, hi_k = (max(0.0, 1 - rho), 1 + rho) if np.isfinite(rho) else (0.0, np.inf)
        with np.errstate(divide="ignore", invalid="ignore"):
            lo_i = np.where(ok, (ud - band) / T, -np.inf)
            hi_i = np.where(ok, (ud + band) / T, np.inf)
        L = max([lo_k] + lo_i[acc & ok].tolist())
        Uu = min([hi_k] + hi_i[rej & ok].tolist())
        # T <= 0 (r = R, or a radius where the bracket has cancelled): an accept needs u inside the band
        flat = np.isfinite(T) & np.isfinite(band) & (T <= 0)
        wrong_flat = int((acc & flat & (ud > band)).sum())
        if not (L <= Uu) or wrong_flat:
            res["bad"].append((float(R), float(lam), int(yuk), L, Uu, wrong_flat))
        with np.errstate(invalid="ignore"):
            sure = (acc & ok & (ud + band < L * T)) | (rej & ok & (ud - band >= Uu * T)) | (rej & flat & (ud > band))
        counted = acc | rej
        res["iterations"] += int(counted.sum())
        res["in_band"] += int((counted & ~sure).sum())
        res["balls"] += 1
        res["unbounded_norm"] += int(not np.isfinite(rho))
    return res


# ---- the accepted radius's distribution -------------------------------------------------------------
def radius_cdf(dim, R, lam, yuk, n=200001):
    """(grid, cdf, bound_active): the CDF of the accepted radius on (0, R), density proportional to
    min(1, pdfRadius / bound); bound_active: pdfRadius exceeds the heuristic bound somewhere."""
    g = np.linspace(0.0, float(R), n)[1:-1].astype(np.float32)
    T, _ = threshold(dim, R, lam, yuk, g)
    T = np.nan_to_num(np.maximum(T, 0.0))
    dens = np.minimum(1.0, T)
    gd = np.concatenate([[0.0], g.astype(np.float64), [float(R)]])
    dens = np.concatenate([[0.0], dens, [0.0]])
    cdf = np.concatenate([[0.0], np.cumsum(0.5 * (dens[1:] + dens[:-1]) * np.diff(gd))])
    return gd, cdf / cdf[-1], bool((T > 1.0).any())


def dkw_distance(dim, R, lam, yuk, radii):
    """sup |F_n - F| of the clamped accepted radii against radius_cdf, and bound_active."""
    gd, cdf, active = radius_cdf(dim, R, lam, yuk)
    rs = np.sort(np.asarray(radii, np.float64))
    n = rs.size
    F = np.interp(rs, gd, cdf)
    F = np.where(rs <= float(RCLAMP), np.interp(float(RCLAMP), gd, cdf), F)  # the clamp's atom
    hi = np.arange(1, n + 1) / n - F
    lo = F - np.arange(0, n) / n
    inside = rs > float(RCLAMP)
    return float(max(hi.max(), lo[inside].max() if inside.any() else 0.0)), active
