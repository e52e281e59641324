"""The Green's function of the ball in arbitrary precision, and the rounding-error bound of
the float expressions that evaluate it (tests/test_gfn_cpu.py, tests/test_gpu_gfn.py,
tests/golden/make_gfn_truth.py; DESIGN.md "Green's-function probe").

The mathematics, written once
-----------------------------
For Delta G - lambda G = -delta on the ball |y - c| < R of R^d with G = 0 on the sphere, the
Green's function with its pole at x expands in the angular modes of x about c.  With
nu = d/2 - 1, mu = sqrt(lambda) and r = |y - c|, the radial part of mode l is

    G_l(r) = (2 pi)^(-d/2) mu^(nu+l) r^(-nu) [K_(nu+l)(mu r) - I_(nu+l)(mu r) K_(nu+l)(mu R) / I_(nu+l)(mu R)]

(mode_yukawa; harmonic limit in mode_harmonic).  l = 0 is the centred Green's function
G(r).  l = 1 is the radial part of grad_x G(x, y) at x = c, the gradient with respect to
the pole that the walk's gradient estimate uses: grad_x G = G_1(r) (y - c) / r.  Every member
of the code's Gfn follows from these two functions:

    evaluate                    G_0(r)
    gradient_norm               G_1(r) / r      (distributions.h:428-431, 515-518, 634-641,
                                761-775: the reference's gradientNorm is the pole gradient --
                                the harmonic one carries -1/R^d and the Yukawa one
                                K_(nu+1)(mu R) / I_(nu+1)(mu R) -- not |G_0'(r)| / r)
    poisson_kernel              R^(d-1) (-G_0'(R))
    norm                        int_B G_0 = |S^(d-1)| int_0^R G_0 r^(d-1) dr
    dir_sampled_poisson_kernel  rho^(d-1) (-G_0'(rho)) at rho = |y - c|, over the harmonic
                                ball's value 1 / |S^(d-1)|
    poisson_kernel_gradient     grad_x of the Poisson kernel at x = c (distributions.h:464-468,
                                551-555, 680-685, 816-821): R^(d-1) (-G_1'(R)) (ySurf - c) / R
    evaluate_xy                 the reference's own off-centre expression (distributions.h:
                                422-425, 509-512, 616-631, 743-758; "an approximation of the
                                infinite series expression, except when x coincides with c"):
                                G_0(r1) - G_0(r2), r1 = max(rClamp, |y - x|),
                                r2 = (R^2 - (x - c).(y - c)) / R.  It is modelled as that
                                expression, not as the exact off-centre Green's function.

The derived members exist twice: by mp.diff / mp.quad of G_l (derived_*), and in the closed
form that follows from the Wronskian I_v K_v' - I_v' K_v = -1/z and the divergence theorem
(the functions the truth table uses; it would take minutes by quadrature).  The CPU test
holds the two against each other, G_l against its radial equation, its boundary value and
its singularity, and the harmonic l = 1 mode against the derivative of the method-of-images
Green's function.

The free-space functions of the splat (FreeSpace2) follow from G(r) = K_0(mu r) / 2 pi
(-log r / 2 pi) in the same way: grad_x G = G'(r) (x - y) / r, P = n . grad_y G,
grad_x P = n f + (n . (x - y)) f'(r) (x - y) / r with f = -G'(r) / r.

What the truth is a function of
-------------------------------
The code forms its arguments in float: mu = fl(sqrt(lambda)), mu R = fl(R mu), mu r = fl(r mu),
the geometric differences, dot products, norms and clamps.  float_args reproduces exactly
that float32 arithmetic (numpy), and the truth is the mathematical function at those floats
(x = mu r and X = mu R enter the Bessel functions, r, R and mu the algebraic factors), so the
bound below needs no conditioning term: it is the error of evaluating the expression, not
of forming its arguments.

The bound
---------
Err mirrors each shipped expression once, node by node, carrying the exact value v of the
node and a rigorous bound e on the error of the computed one:

    a float rounding          e += 2^-24 (|v| + e)    (2^-150 more where |v| < FLT_MIN)
    a double operation        e += 2^-50 (|v| + e)
    an A&S Bessel value       e  = EPS_AS |v|         (tests/test_oracle.py's bound)
    a +- b                    e_a + e_b               (cancellation widens the bound)
    a * b                     e_a |b| + |a| e_b + e_a e_b
    a / b                     (e_a |b| + |a| e_b) / (|b| (|b| - e_b)), infinite once e_b >= |b|

This is tol = (k 2^-24 + a EPS_AS) S of the issue applied at every addition of the expression
tree: S is the sum of the absolute values of the terms, carried through products and
quotients, k and a the roundings and Bessel values on the path (Err.k, Err.a count them).
A node whose float value leaves the float range (|v| > FLT_MAX, or a quotient whose divisor
underflowed to where its error bound reaches its value) marks the result `out`: the only pairs
a test may leave out, and only above mu R = 85.  A finite divisor whose error bound reaches
its value (the 3D float members below mu R ~ 1e-2, where cosh - sinh / x cancels completely)
gives an infinite bound: the expression carries no information there, and the test counts
those pairs too.
"""
import functools

import mpmath as mp

from gfn_cases import RCLAMP, ROBUST_MUR, float_args  # noqa: F401

mp.mp.dps = 50
mpf = mp.mpf

U = mpf(2) ** -24
UD = mpf(2) ** -50
EPS_AS = mpf("1e-6")
FLT_MAX = mpf(2) ** 128 - mpf(2) ** 104
FLT_MIN = mpf(2) ** -126

# per-item scalar slots of the truth table (vector members are these times a float vector)
#   ball-level (functions of R, lambda alone) and item-level
BALL_SLOTS = ("A0", "A1", "B0", "B1", "pk", "norm", "pkg")
ITEM_SLOTS = ("ev", "gn", "dpk", "exy", "fsG", "fsg", "fsc")


@functools.lru_cache(maxsize=1 << 14)
def _bessel(kind, o, x, prec):
    return mp.besselk(o, x) if kind == "k" else mp.besseli(o, x)


def besselk(o, x):  # (integer orders take milliseconds at 50 digits: every caller shares them)
    return _bessel("k", o, x, mp.mp.prec)


def besseli(o, x):
    return _bessel("i", o, x, mp.mp.prec)


def sphere_area(d):
    return 2 * mp.pi if d == 2 else 4 * mp.pi


# ---- the radial modes -------------------------------------------------------------------------
def bracket(d, l, x, X):
    """K_(nu+l)(x) - I_(nu+l)(x) K_(nu+l)(X) / I_(nu+l)(X): mode l's radial solution, zero at x = X."""
    o = mpf(d) / 2 - 1 + l
    return besselk(o, x) - besseli(o, x) * besselk(o, X) / besseli(o, X)


def mode_yukawa(d, l, r, R, mu):
    """G_l(r) of the Yukawa ball."""
    nu = mpf(d) / 2 - 1
    return (2 * mp.pi) ** (-mpf(d) / 2) * mu ** (nu + l) * r ** (-nu) * bracket(d, l, mu * r, mu * R)


def mode_harmonic(d, l, r, R):
    """lambda -> 0 of mode_yukawa: the solutions r^l and r^(2-d-l) (log r for d = 2, l = 0)."""
    A = sphere_area(d)
    if l == 0:
        return mp.log(R / r) / A if d == 2 else (1 / r - 1 / R) / A
    return (r ** (1 - d) - r / R ** d) / A


def images_green(d, xv, yv, R):
    """The harmonic Green's function of the ball about 0 with its pole at xv (method of images)."""
    A = sphere_area(d)
    dxy = mp.sqrt(sum((a - b) ** 2 for a, b in zip(xv, yv)))
    x2 = sum(a * a for a in xv)
    y2 = sum(a * a for a in yv)
    xy = sum(a * b for a, b in zip(xv, yv))
    w = mp.sqrt(x2 * y2 / (R * R) - 2 * xy + R * R)  # |x| |y - x*| / R
    if d == 2:
        return (mp.log(w) - mp.log(dxy)) / A
    return (1 / dxy - 1 / w) / A


# ---- members by differentiation and quadrature (self-checks) ----------------------------------------
def _G(d, l, R, lam):
    if lam == 0:
        return lambda r: mode_harmonic(d, l, r, R)
    mu = mp.sqrt(lam)
    return lambda r: mode_yukawa(d, l, r, R, mu)


def derived_members(d, r, R, lam):
    G0, G1 = _G(d, 0, R, lam), _G(d, 1, R, lam)
    A = sphere_area(d)
    return {
        "ev": G0(r),
        "gn": G1(r) / r,
        "pk": R ** (d - 1) * -mp.diff(G0, R),
        "norm": A * mp.quad(lambda s: G0(s) * s ** (d - 1), [0, R / 2, R]),
        "dpk": A * r ** (d - 1) * -mp.diff(G0, r),
        "pkg": R ** (d - 1) * -mp.diff(G1, R) / R,
    }


# ---- members in closed form, at the code's arguments ------------------------------------------------
def members(d, lam, R, r, mu, x, X, xd):
    """The scalar members; lam == 0: harmonic.  x = mu r, X = mu R, xd = mu rho of dir_sampled.
    Where the float arguments are redundant (x and mu r, X and mu R, lambda and mu^2 agree only up
    to their roundings) each member takes the ones its shipped expression takes -- the function of
    consistent arguments is the same (test_members_closed_form_vs_derived)."""
    A = sphere_area(d)
    if lam == 0:
        return {"ev": mode_harmonic(d, 0, r, R), "gn": mode_harmonic(d, 1, r, R) / r, "pk": 1 / A,
                "norm": R * R / (2 * d), "dpk": mpf(1), "pkg": d / (A * R * R),
                "A0": mpf(0), "A1": mpf(0), "B0": mpf(0), "B1": mpf(0)}
    nu = mpf(d) / 2 - 1
    c = (2 * mp.pi) ** (-mpf(d) / 2)
    pk = c * X ** nu / besseli(nu, X)  # Wronskian at R
    out = {
        # mu^nu r^-nu = x^nu r^(-2 nu);  mu^(nu+1) r^(-nu-1) = mu x^nu r^(-2 nu - 1)
        "ev": c * x ** nu * r ** (-2 * nu) * bracket(d, 0, x, X),
        "gn": c * mu * x ** nu * r ** (-2 * nu - 1) * bracket(d, 1, x, X),
        "pk": pk,
        "norm": (1 - A * pk) / lam,  # divergence theorem on Delta G - lambda G = -delta
        "dpk": A * c * xd ** (nu + 1) * (besselk(nu + 1, xd) + besseli(nu + 1, xd) * besselk(nu, X)
                                         / besseli(nu, X)),
        # mu^(nu+1) R^(d-3-nu): 2D mu / R, 3D mu^(3/2) R^(-1/2) = lambda X^(-1/2)
        "pkg": c * (mu / R if d == 2 else lam / mp.sqrt(X)) / besseli(nu + 1, X),
    }
    if d == 2:
        out.update(A0=besselk(0, X), A1=besseli(0, X), B0=besselk(1, X), B1=besseli(1, X))
    else:
        # the code's 3D members are K_(1/2), I_(1/2), K_(3/2), I_(3/2) without sqrt(pi / 2X), sqrt(2 / pi X)
        k, i = mp.sqrt(2 * X / mp.pi), mp.sqrt(mp.pi * X / 2)
        out.update(A0=k * besselk(nu, X), A1=i * besseli(nu, X), B0=k * besselk(nu + 1, X),
                   B1=i * besseli(nu + 1, X))
    return out


def scaled_2d_members(X):
    """ke0 ie0 ke1 ie1 at mu R: the members of a 2D scaled ball."""
    return {"A0": mp.exp(X) * besselk(0, X), "A1": mp.exp(-X) * besseli(0, X),
            "B0": mp.exp(X) * besselk(1, X), "B1": mp.exp(-X) * besseli(1, X)}


def evaluate_xy(d, lam, R, mu, X, r1, r2, x1, x2, w=None, p=None):
    """G_0(r1) - G_0(r2); harmonic 2D from the code's two log arguments w = R^2 - xc.yc, p = R r1."""
    if lam == 0:
        if d == 2:
            return (mp.log(w) - mp.log(p)) / (2 * mp.pi)
        return (1 / r1 - R / w) / (4 * mp.pi)
    nu = mpf(d) / 2 - 1
    c = (2 * mp.pi) ** (-mpf(d) / 2)
    return c * (x1 ** nu * r1 ** (-2 * nu) * bracket(d, 0, x1, X) - x2 ** nu * r2 ** (-2 * nu) * bracket(d, 0, x2, X))


# ---- free space, 2D -----------------------------------------------------------------------------------
def fs_G(lam, r, mu=None, x=None):
    if lam == 0:
        return -mp.log(r) / (2 * mp.pi)
    return besselk(0, mu * r if x is None else x) / (2 * mp.pi)


def fs_scalars(lam, r, mu, x):
    """G, g = -G'(r) / r and c = -f'(r) / r (f = g): grad G = -xy g, P = nd g, grad P = n g - nd c xy."""
    if lam == 0:
        return {"fsG": fs_G(0, r), "fsg": 1 / (2 * mp.pi * r * r), "fsc": 2 / (2 * mp.pi * r ** 4)}
    K0, K1 = besselk(0, x), besselk(1, x)
    K2 = besselk(2, x)
    g = mu * K1 / (2 * mp.pi * r)
    # f' = mu / 2 pi (mu K1'(x) / r - K1 / r^2), K1' = -(K0 + K2) / 2
    c = (mu * K1 + r * lam * (K0 + K2) / 2) / (2 * mp.pi * r ** 3)  # (lambda where the code takes it)
    return {"fsG": K0 / (2 * mp.pi), "fsg": g, "fsc": c}


def fs_derived(lam, r):
    """fs_scalars by mp.diff of G(r) (self-check; consistent arguments)."""
    mu = mp.sqrt(lam) if lam else None
    G = lambda s: fs_G(lam, s, mu)
    f = lambda s: -mp.diff(G, s) / s
    return {"fsG": G(r), "fsg": f(r), "fsc": -mp.diff(f, r) / r}


# ---- the code's float arguments: gfn_cases.float_args (numpy only, shared with the GPU test) --------


def _m(v):
    return mpf(float(v))


def truth(d, yukawa, it, ball_only=False, fs_only=False):
    """Every scalar slot of item `it` (BALL_SLOTS + ITEM_SLOTS; mp.nan where it does not apply)."""
    a = float_args(d, it)
    lam = _m(a["lam"]) if yukawa else 0
    out = {}
    if not fs_only:
        m = members(d, lam, _m(a["R"]), _m(a["r"]), _m(a["sl"]), _m(a["x"]), _m(a["X"]), _m(a["xd"]))
        if yukawa and d == 2 and a["X"] > ROBUST_MUR:
            m.update({k + "s": v for k, v in scaled_2d_members(_m(a["X"])).items()})
        out.update(m)
        ok = a["r2"] > 0 and a["w"] > 0
        out["exy"] = evaluate_xy(d, lam, _m(a["R"]), _m(a["sl"]), _m(a["X"]), _m(a["r1"]), _m(a["r2"]), _m(a["x1"]),
                                 _m(a["x2"]), _m(a["w"]), _m(a["p"])) if ok else mp.nan
    else:
        out.update({k: mp.nan for k in BALL_SLOTS + ("ev", "gn", "dpk", "exy")})
    if d == 2:
        out.update(fs_scalars(lam, _m(a["fr"]), _m(a["sl"]), _m(a["fx"])))
    else:
        out.update(fsG=mp.nan, fsg=mp.nan, fsc=mp.nan)
    return out


# ---- the error bound ------------------------------------------------------------------------------------
class Err:
    """A node of a shipped expression: exact value v, error bound e of the computed value, the
    roundings k and Bessel values a on its path, `out` once a float left the float range."""
    __slots__ = ("v", "e", "k", "a", "out")
    ctx = "f"  # "f": every operation rounds to float; "d": to double

    def __init__(self, v, e=0, k=0, a=0, out=False):
        self.v, self.e, self.k, self.a, self.out = mpf(v), mpf(e), k, a, out

    def _rnd(self):
        av = abs(self.v)
        if Err.ctx == "d":
            self.e += UD * (av + self.e)
        else:
            if av > FLT_MAX:
                self.out = True
            self.e += U * (av + self.e)
            if av < FLT_MIN:
                self.e += mpf(2) ** -150
        self.k += 1
        return self

    def to_float(self):  # a double result rounded to float
        ctx, Err.ctx = Err.ctx, "f"
        r = Err(self.v, self.e, self.k, self.a, self.out)._rnd()
        Err.ctx = ctx
        return r

    @staticmethod
    def lift(o):
        return o if isinstance(o, Err) else Err(o)

    def __add__(self, o):
        o = Err.lift(o)
        return Err(self.v + o.v, self.e + o.e, max(self.k, o.k), max(self.a, o.a), self.out or o.out)._rnd()

    def __sub__(self, o):
        o = Err.lift(o)
        return Err(self.v - o.v, self.e + o.e, max(self.k, o.k), max(self.a, o.a), self.out or o.out)._rnd()

    __radd__ = __add__

    def __rsub__(self, o):
        return Err.lift(o) - self

    def __neg__(self):
        return Err(-self.v, self.e, self.k, self.a, self.out)

    def __mul__(self, o):
        o = Err.lift(o)
        e = self.e * abs(o.v) + abs(self.v) * o.e + self.e * o.e
        return Err(self.v * o.v, e, self.k + o.k, self.a + o.a, self.out or o.out)._rnd()

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Err.lift(o)
        b = abs(o.v)
        out = self.out or o.out
        if o.e >= b:
            # no information about the divisor; an underflowed one is a float-range exit
            if Err.ctx == "f" and b < FLT_MIN:
                out = True
            e = mp.inf
        else:
            e = (self.e * b + abs(self.v) * o.e) / (b * (b - o.e))
        return Err(self.v / o.v if o.v != 0 else mp.inf, e, self.k + o.k, self.a + o.a, out)._rnd()

    def __rtruediv__(self, o):
        return Err.lift(o) / self

    def exp(self):  # exp in double (detmath), rounded to the context
        v = mp.exp(self.v)
        r = Err(v, v * mp.expm1(self.e) if self.e < 700 else mp.inf, self.k, self.a, self.out)
        if Err.ctx == "f":
            r.e += UD * v
        return r._rnd()

    def log(self):
        if self.e >= abs(self.v) or self.v <= 0:
            return Err(mp.log(abs(self.v)) if self.v != 0 else 0, mp.inf, self.k, self.a, self.out)
        r = Err(mp.log(self.v), -mp.log1p(-self.e / self.v), self.k, self.a, self.out)
        if Err.ctx == "f":
            r.e += UD * abs(r.v)
        return r._rnd()


class _Double:
    def __enter__(self):
        self.prev, Err.ctx = Err.ctx, "d"

    def __exit__(self, *a):
        Err.ctx = self.prev


def _bess(kind, x, scaled=False):
    """An A&S value in double at the exact float x (bessk0 ... or the scaled ke / ie)."""
    f = {"k0": lambda: besselk(0, x), "k1": lambda: besselk(1, x), "i0": lambda: besseli(0, x),
         "i1": lambda: besseli(1, x)}[kind]()
    if scaled:
        f *= mp.exp(x) if kind[0] == "k" else mp.exp(-x)
    return Err(f, EPS_AS * abs(f), 0, 1)


def _i32s(x):  # i32_scaled, in double
    e2 = (Err(-2) * x).exp()
    return Err(mpf(1) / 2) * ((1 + e2) - (1 - e2) / x)


TWO_PI, FOUR_PI = 2 * mp.pi, 4 * mp.pi  # (their double values are off by 2^-54: inside one double rounding)


def _sinh_cosh_f(x):
    """The float cosh, sinh, K32, I32 of the 3D members from e = fexp(-x)."""
    e = (-Err.lift(x)).exp()
    e2 = e * e
    den = Err(2) * e
    ch, sh = (1 + e2) / den, (1 - e2) / den
    k32 = e * (1 + Err(1) / x)
    i32 = ch - sh / x
    return e, ch, sh, k32, i32


def bounds(d, mode, it):
    """{slot: Err} of the shipped expressions of item `it` under mode (0, 1, 2): the scalar slots of
    truth(), with Err.v the exact value the expression approximates."""
    a = float_args(d, it)
    R, lam, r, sl, X, x, xd = (_m(a[k]) for k in ("R", "lam", "r", "sl", "X", "x", "xd"))
    r1, r2, x1, x2, w, p = (_m(a[k]) for k in ("r1", "r2", "x1", "x2", "w", "p"))
    E = Err
    Err.ctx = "f"
    o = {}
    xy_ok = a["r2"] > 0 and a["w"] > 0
    if mode == 0:
        if d == 2:
            o["ev"] = (E(R) / r).log() / TWO_PI
            o["gn"] = (1 / (E(r) * r) - 1 / (E(R) * R)) / TWO_PI
            o["norm"] = E(R) * R / 4
            o["pkg"] = 2 / (E(TWO_PI) * R * R)  # (2 d_k) / s per unit d_k
            if xy_ok:
                o["exy"] = (E(w).log() - E(p).log()) / TWO_PI
        else:
            o["ev"] = (1 / E(r) - 1 / E(R)) / FOUR_PI
            o["gn"] = (1 / (E(r) * r * r) - 1 / (E(R) * R * R)) / FOUR_PI
            o["norm"] = E(R) * R / 6
            o["pkg"] = 3 / (E(FOUR_PI) * R * R)
            if xy_ok:
                o["exy"] = (1 / E(r1) - E(R) / w) / FOUR_PI
        o["pk"] = E(1 / sphere_area(d))._rnd()
        o["dpk"] = E(1)
    elif mode == 1 or a["X"] <= ROBUST_MUR:
        if d == 2:
            A0, A1 = _bess("k0", X).to_float(), _bess("i0", X).to_float()
            B0, B1 = _bess("k1", X).to_float(), _bess("i1", X).to_float()
            q0 = lambda t: _bess("k0", t).to_float() - _bess("i0", t).to_float() * A0 / A1
            o["ev"] = q0(x) / TWO_PI
            o["gn"] = E(sl) * (_bess("k1", x).to_float() - _bess("i1", x).to_float() * B0 / B1) / (E(TWO_PI) * r)
            with _Double():
                pk = 1 / (E(TWO_PI) * A1)
            o["pk"] = pk.to_float()
            o["pkg"] = E(sl) / (E(R) * B1) / E(TWO_PI)._rnd()
            o["dpk"] = E(xd) * (_bess("k1", xd).to_float() + _bess("i1", xd).to_float() * A0 / A1)
            if xy_ok:
                o["exy"] = (q0(x1) - q0(x2)) / TWO_PI
        else:
            A0, _, A1, B0, B1 = _sinh_cosh_f(X)
            e, ch, sh, k32, i32 = _sinh_cosh_f(x)
            o["ev"] = (e - A0 * sh / A1) / (E(FOUR_PI) * r)
            o["gn"] = E(sl) * (k32 - i32 * B0 / B1) / (E(FOUR_PI) * (E(r) * r))
            with _Double():
                pk = E(X) / (E(FOUR_PI) * A1)
            o["pk"] = pk.to_float()
            o["pkg"] = E(lam) / B1 / E(FOUR_PI)._rnd()
            ed, chd, shd, k32d, i32d = _sinh_cosh_f(xd)
            o["dpk"] = E(xd) * (k32d + i32d * A0 / A1)
            if xy_ok:
                e1, _, s1, _, _ = _sinh_cosh_f(x1)
                e2, _, s2, _, _ = _sinh_cosh_f(x2)
                o["exy"] = ((e1 - A0 * s1 / A1) / r1 - (e2 - A0 * s2 / A1) / r2) / FOUR_PI
        with _Double():
            nrm = (1 - E(sphere_area(d)) * o["pk"]) / lam
        o["norm"] = nrm.to_float()
        o.update(A0=A0, A1=A1, B0=B0, B1=B1)
    else:  # scaled members: double, rounded once
        with _Double():
            if d == 2:
                A0, A1 = _bess("k0", X, True).to_float(), _bess("i0", X, True).to_float()
                B0, B1 = _bess("k1", X, True).to_float(), _bess("i1", X, True).to_float()
                o.update(A0=A0, A1=A1, B0=B0, B1=B1)

                def q0(t):
                    return (-E(t)).exp() * (_bess("k0", t, True) - _bess("i0", t, True) * (A0 / A1)
                                            * (2 * (E(t) - X)).exp())
                o["ev"] = (q0(x) / TWO_PI).to_float()
                tt = (2 * (E(x) - X)).exp()
                q = (-E(x)).exp() * (_bess("k1", x, True) - _bess("i1", x, True) * (B0 / B1) * tt)
                o["gn"] = (E(sl) * q / (E(TWO_PI) * r)).to_float()
                o["pk"] = ((-E(X)).exp() / (E(TWO_PI) * A1)).to_float()
                QR = (E(sl) * (-E(X)).exp() / (E(R) * B1)).to_float()
                td = (2 * (E(xd) - X)).exp()
                o["dpk"] = (E(xd) * (-E(xd)).exp() * (_bess("k1", xd, True) + _bess("i1", xd, True) * (A0 / A1)
                                                       * td)).to_float()
                if xy_ok:
                    o["exy"] = ((q0(x1) - q0(x2)) / TWO_PI).to_float()
            else:
                o.update(A0=E(0), A1=E(0), B0=E(0), B1=E(0))

                def q0(t):
                    return (-E(t)).exp() - (E(t) - 2 * E(X)).exp() * (1 - (-2 * E(t)).exp()) / (1 - (-2 * E(X)).exp())
                o["ev"] = (q0(x) / (E(FOUR_PI) * r)).to_float()
                tt = (2 * (E(x) - X)).exp()
                q = (-E(x)).exp() * ((1 + 1 / E(x)) - _i32s(E(x)) * ((1 + 1 / E(X)) / _i32s(E(X))) * tt)
                Err.ctx = "f"
                r2f = E(r) * r
                Err.ctx = "d"
                o["gn"] = (E(sl) * q / (E(FOUR_PI) * r2f)).to_float()
                o["pk"] = (E(X) * 2 * (-E(X)).exp() / (E(FOUR_PI) * (1 - (-2 * E(X)).exp()))).to_float()
                QR = (E(lam) * (-E(X)).exp() / _i32s(E(X))).to_float()
                td = (2 * (E(xd) - X)).exp()
                qd = (1 + 1 / E(xd)) + _i32s(E(xd)) * (2 / (1 - (-2 * E(X)).exp())) * td
                o["dpk"] = (E(xd) * (-E(xd)).exp() * qd).to_float()
                if xy_ok:
                    o["exy"] = ((q0(x1) / r1 - q0(x2) / r2) / FOUR_PI).to_float()
            o["norm"] = ((1 - E(sphere_area(d)) * o["pk"]) / lam).to_float()
        Err.ctx = "f"
        o["pkg"] = QR / E(sphere_area(d))._rnd()
    if d == 2:
        Err.ctx = "f"
        fr, fx = _m(a["fr"]), _m(a["fx"])
        if mode == 0:
            o["fsG"] = -(E(fr).log()) / TWO_PI
            o["fsg"] = 1 / (E(TWO_PI) * (E(fr) * fr))
            # c of grad P = (n - c' xy) / s, c' = 2 nd / r^2: per unit nd
            o["fsc"] = E(2) / (E(fr) * fr) / (E(TWO_PI) * (E(fr) * fr))
        else:
            K0, K1 = _bess("k0", fx).to_float(), _bess("k1", fx).to_float()
            with _Double():
                K2d = _bess("k0", fx) + (E(2) / fx) * _bess("k1", fx)
            K2 = K2d.to_float()
            o["fsG"] = K0 / TWO_PI
            Qr1 = E(sl) * K1
            o["fsg"] = Qr1 / (E(TWO_PI) * fr)
            Qr2 = E(lam) * (K0 + K2) / 2
            o["fsc"] = (1 / (E(fr) * fr)) * (Qr1 + E(fr) * Qr2) / (E(TWO_PI) * fr)
    Err.ctx = "f"
    return o


def tolerance(err, t):
    """The bound of one slot against truth t: (tol, out).  Subnormal truth: floor FLT_MIN."""
    tol = err.e
    if abs(t) < FLT_MIN and tol < FLT_MIN:
        tol = FLT_MIN
    return tol, err.out
