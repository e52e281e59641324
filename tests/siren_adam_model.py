"""Models of the fused Adam step (wos_adam_step, include/wos.h "Fused Adam step") for the tests:
step32, a numpy restatement that holds every operation in np.float32, one at a time -- the norm's
256 chains and its pairwise order included -- which the device must equal bit for bit; step64, the
same formulas in float64 with the double scalars unrounded, which equals torch.optim.Adam in float64;
and bound(), the per-element error bound B between two float32 evaluations of the step."""
import numpy as np

F = np.float32
U = 2.0 ** -24


def scalars(lr, betas, eps, step):
    """The step's five scalars (and eps) in double, as torch's single-tensor Adam computes them."""
    b1, b2 = float(betas[0]), float(betas[1])
    return {"b2": b2, "omb1": 1.0 - b1, "omb2": 1.0 - b2, "bc2": (1.0 - b2 ** step) ** 0.5,
            "ss": float(lr) / (1.0 - b1 ** step), "eps": float(eps)}


def norm32(flat):
    """sqrtf of the sum of squares in the kernel's order: thread t chains acc = acc + g[e] * g[e] over
    e = t, t + 256, ..., then the 256 sums pairwise (t, t + 128), (t, t + 64), ..."""
    g = np.asarray(flat, F).reshape(-1)
    sq = g * g  # the product rounded, then the sum
    rows = (sq.size + 255) // 256
    padded = np.zeros(rows * 256, F)
    padded[:sq.size] = sq  # a padding term adds +0 to a non-negative sum: the same bits as leaving it out
    acc = np.zeros(256, F)
    for row in padded.reshape(rows, 256):
        acc = acc + row
    w = 128
    while w >= 1:
        acc[:w] = acc[:w] + acc[w:2 * w]
        w >>= 1
    return np.sqrt(acc[0])


def clip32(norm, max_grad_norm):
    """min(max_grad_norm / (norm + 1e-6), 1) as torch.clamp(max=1) takes it: a NaN quotient stays NaN."""
    q = F(max_grad_norm) / (F(norm) + F(1e-6))
    return F(1.0) if q >= F(1.0) else q


def step32(params, grads, m, v, step, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None):
    """One step in float32.  params, grads: lists of arrays; m, v: flat arrays in that order.
    Returns (params', m', v', norm) as new float32 arrays; norm is None without clipping."""
    s = {k: F(x) for k, x in scalars(lr, betas, eps, step).items()}  # each rounded to float once
    g = np.concatenate([np.asarray(a, F).reshape(-1) for a in grads])
    p = np.concatenate([np.asarray(a, F).reshape(-1) for a in params])
    m, v = np.asarray(m, F), np.asarray(v, F)
    norm = None
    if max_grad_norm is not None and max_grad_norm > 0:
        norm = norm32(g)
        g = g * clip32(norm, max_grad_norm)
    dm = g - m
    wm = s["omb1"] * dm
    m1 = m + wm
    vb = v * s["b2"]
    og = s["omb2"] * g
    ogg = og * g
    v1 = vb + ogg
    root = np.sqrt(v1)
    rb = root / s["bc2"]
    den = rb + s["eps"]
    ratio = m1 / den
    upd = s["ss"] * ratio
    p1 = p - upd
    for a in (m1, v1, p1):
        assert a.dtype == F
    out, at = [], 0
    for a in params:
        out.append(p1[at:at + a.size].reshape(a.shape))
        at += a.size
    return out, m1, v1, norm


def step64(params, grads, m, v, step, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None):
    """The same formulas in float64.  Returns (params', m', v', norm, extras): extras holds the flat
    float64 quantities bound() needs -- p', the update delta, den, the clipped gradient, the old m,
    ss, and whether the clip was active."""
    s = scalars(lr, betas, eps, step)
    g = np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in grads])
    p = np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in params])
    m, v = np.asarray(m, np.float64), np.asarray(v, np.float64)
    norm, active = None, False
    if max_grad_norm is not None and max_grad_norm > 0:
        norm = float(np.sqrt(np.sum(g * g)))
        c = min(float(max_grad_norm) / (norm + 1e-6), 1.0)
        active = c < 1.0
        g = g * c
    m1 = m + s["omb1"] * (g - m)
    v1 = v * s["b2"] + (s["omb2"] * g) * g
    den = np.sqrt(v1) / s["bc2"] + s["eps"]
    delta = s["ss"] * (m1 / den)
    p1 = p - delta
    out, at = [], 0
    for a in params:
        out.append(p1[at:at + a.size].reshape(a.shape))
        at += a.size
    extras = {"p": p1, "delta": delta, "den": den, "g": g, "m": m, "ss": s["ss"], "clip_active": active, "n": g.size}
    return out, m1, v1, norm, extras


def bound(x):
    """B = u |p'| + 12 u |delta| + 4 u ss (|m| + |g'|) / den + e_c (ss |g'| / den + |delta|), per flat
    element, from step64's extras: the final subtraction's half ulp; six once-rounded operations on
    the update, on each side of a comparison; the cancellation in m', whose error is relative to
    |m| + |g'| and not to |m'|; and, when the clip is active, the worst-case sum-of-squares error of
    the clip coefficient, e_c = (N / 2 + 4) u."""
    e_c = (x["n"] / 2 + 4) * U if x["clip_active"] else 0.0
    return (U * np.abs(x["p"]) + 12 * U * np.abs(x["delta"]) + 4 * U * x["ss"] * (np.abs(x["m"]) + np.abs(x["g"])) / x["den"]
            + e_c * (x["ss"] * np.abs(x["g"]) / x["den"] + np.abs(x["delta"])))


def problem(shapes, seed=0, state=True, top=2, subnormal=False):
    """(params, grads, m, v) float32 for tensors of `shapes`: gradients over seven decades with exact
    zeros, |g| in {0} U [10^(top - 7), 10^top] -- every intermediate is exactly zero or normal, also
    after a clip to a norm of 0.1 -- and, with state, moments as some earlier steps would leave them
    (v >= 0).  top=2 keeps the norm of 1000 elements below 1e3, top=0 that of a 3 x 256 network.
    subnormal: an eighth of the elements (eight at the least) get |g| in [1e-23, 1e-19], so that
    (1 - beta2) g g is subnormal or underflows to zero; with state, every other one of them has v = 0
    (v' is that product), every fourth a subnormal v and every third a subnormal m on input."""
    rng = np.random.default_rng(seed)
    total = sum(int(np.prod(s)) for s in shapes)

    def grads_like():
        mag = 10.0 ** rng.uniform(top - 7, top, total)
        g = (mag * rng.choice([-1.0, 1.0], total)).astype(F)
        g[rng.random(total) < 0.1] = 0.0
        return g
    g = grads_like()
    p = rng.standard_normal(total).astype(F)
    if state:
        m = (0.1 * grads_like()).astype(F)
        v = (grads_like().astype(np.float64) ** 2 * 0.01).astype(F)
        zero = g == 0
        m[zero & (rng.random(total) < 0.5)] = 0.0  # g = m = v = 0 at some elements: den = eps
        v[m == 0] = 0.0
    else:
        m, v = np.zeros(total, F), np.zeros(total, F)
    if subnormal:  # drawn last: the values above are those of subnormal=False
        tiny = rng.choice(total, max(8, total // 8), replace=False)

        def small(lo, hi, count):
            return (10.0 ** rng.uniform(lo, hi, count) * rng.choice([-1.0, 1.0], count)).astype(F)
        g[tiny] = small(-23, -19, tiny.size)
        if state:
            v[tiny[::2]] = 0.0
            v[tiny[1::4]] = np.abs(small(-44, -39, tiny[1::4].size))
            m[tiny[::3]] = small(-44, -39, tiny[::3].size)

    def split(flat):
        out, at = [], 0
        for s in shapes:
            n = int(np.prod(s))
            out.append(flat[at:at + n].reshape(s).copy())
            at += n
        return out
    return split(p), split(g), m, v


def net_shapes(d, H, L, d_out):
    """The tensor list of a SIREN in pack() order: weights, then biases."""
    w = [(H, d)] + [(H, H)] * L + [(d_out, H)]
    b = [(H,)] * (L + 1) + [(d_out,)]
    return w + b
