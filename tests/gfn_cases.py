"""The Green's-function probe's truth table (tests/golden/gfn_truth.npz) held against a probe
result -- the CPU oracle's (tests/test_gfn_cpu.py) or the device's (tests/test_gpu_gfn.py).
numpy only: no test that runs on the GPU evaluates the model.  Layouts: include/wos.h
wos_selftest_gfn, tests/golden/make_gfn_truth.py; the bound: tests/gfn_model.py.
"""
import os

import numpy as np

TRUTH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gfn_truth.npz")
RCLAMP = np.float32(1e-4)
ROBUST_MUR = 80.0
U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
f32 = np.float32

# result columns of the scalar slots (include/wos.h)
COL = {"A0": 0, "A1": 1, "B0": 2, "B1": 3, "pk": 8, "norm": 9, "ev": 6, "gn": 7, "dpk": 13, "exy": 14, "fsG": 26}
# members a comparison reports, in the order of the table in DESIGN.md
MEMBERS = ("A0", "A1", "B0", "B1", "evaluate", "gradient_norm", "gradient", "poisson_kernel", "norm",
           "poisson_kernel_gradient", "dir_sampled_poisson_kernel", "evaluate_xy", "pdf_sphere_uniform",
           "fs_evaluate", "fs_gradient", "fs_poisson", "fs_poisson_gradient")


def _dot(a, b, d):
    s = f32(f32(a[0] * b[0]) + f32(a[1] * b[1]))
    if d == 3:
        s = f32(s + f32(a[2] * b[2]))
    return s


def float_args(d, it):
    """The float32 values the code forms from item `it` before any member arithmetic: mu, mu R,
    mu r, the differences, dot products, norms and clamps, in the code's own operation order."""
    it = np.asarray(it, np.float32)
    R, lam, r = it[0], it[1], it[2]
    c, dr, x, y = it[3:3 + d], it[6:6 + d], it[9:9 + d], it[12:12 + d]
    sl = np.sqrt(lam, dtype=np.float32)
    a = {"R": R, "lam": lam, "r": r, "sl": sl, "X": f32(R * sl), "x": f32(r * sl)}
    yVol = (c + (r * dr).astype(np.float32)).astype(np.float32)
    ySurf = (c + (R * dr).astype(np.float32)).astype(np.float32)
    a["dV"] = (yVol - c).astype(np.float32)
    a["dS"] = (ySurf - c).astype(np.float32)
    rho = max(RCLAMP, np.sqrt(_dot(a["dV"], a["dV"], d), dtype=np.float32))
    a["xd"] = f32(rho * sl)
    yx, xc, yc = (y - x).astype(np.float32), (x - c).astype(np.float32), (y - c).astype(np.float32)
    a["r1"] = max(RCLAMP, np.sqrt(_dot(yx, yx, d), dtype=np.float32))
    a["w"] = f32(f32(R * R) - _dot(xc, yc, d))
    a["p"] = f32(R * a["r1"])
    with np.errstate(all="ignore"):
        a["r2"] = f32(a["w"] / R)
        a["x1"], a["x2"] = f32(a["r1"] * sl), f32(a["r2"] * sl)
    if d == 2:
        a["n"] = it[15:17]
        a["xy"] = (x - y).astype(np.float32)
        a["fr"] = max(it[17], np.sqrt(f32(f32(yx[0] * yx[0]) + f32(yx[1] * yx[1])), dtype=np.float32))
        a["fx"] = f32(a["fr"] * sl)
    return a


_table = None


def table():
    global _table
    if _table is None:
        with np.load(TRUTH) as z:
            _table = {k: z[k] for k in z.files}
        for d in (2, 3):
            items = _table[f"items{d}"]
            args = [float_args(d, it) for it in items]
            _table[f"X{d}"] = np.asarray([a["X"] for a in args], np.float64)
            for k in ("dV", "dS") + (("xy", "n") if d == 2 else ()):
                _table[f"{k}{d}"] = np.asarray([a[k] for a in args], np.float64)
            _table[f"r{d}"] = items[:, 2].astype(np.float64)
    return _table


def rows_of(d, mode):
    """The items a mode runs: the reference grid and the free-space sweep; mode 2 the robust grid too."""
    kind = table()[f"kind{d}"]
    return np.flatnonzero(kind != 1) if mode != 2 else np.arange(len(kind))


def _truth_tol(d, mode):
    """truth [n, S], tol [n, S], out [n, S] over rows_of(d, mode); NaN truth or tol: not pinned."""
    T = table()
    rows = rows_of(d, mode)
    if mode == 0:
        return T[f"th{d}"], T[f"eh{d}"].astype(np.float64), np.zeros(T[f"th{d}"].shape, bool)
    truth = T[f"ty{d}"][rows].copy()
    tol = T[f"e1{d}"][rows].astype(np.float64)
    out = T[f"out1{d}"][rows].copy()
    if mode == 2:
        idx2 = T[f"idx2{d}"]
        tol[idx2] = T[f"e2{d}"]
        out[idx2] = False
        ts = T[f"tys{d}"][idx2]
        m = truth[idx2, :4]
        truth[idx2, :4] = np.where(np.isfinite(ts), ts, np.nan if d == 3 else m)
    return truth, tol, out


def compare(d, mode, res):
    """Holds the probe result res [rows_of(d, mode), 32] against the truth.  Returns
    {member: {"max": largest err / tol, "item": its row, "n": pairs compared, "skipped": pairs left
    out because a float intermediate leaves the float range, "unbounded": pairs whose bound is
    infinite, "skipped_min_muR": the smallest mu R among the skipped}}.

    The vector members are the table's scalar times a float vector the code formed (dV = yVol - c,
    dS = ySurf - c, xy = x - y, n): with s the scalar, e_s its bound and v the vector component,
      s v              e_s |v| + 2 u |s v|                         (one product, one more rounding)
      P = nd g         nd = n . xy formed in float: |nd - exact| <= 2 u (|n0 xy0| + |n1 xy1|) = e_nd;
                       e_g |nd| + g e_nd + 2 u |P|
      grad P           n_k g - nd c xy_k: e_g |n_k| + e_c |nd xy_k| + c |xy_k| e_nd
                       + 3 u (|n_k g| + |nd c xy_k|)
    """
    T = table()
    rows = rows_of(d, mode)
    res = np.asarray(res, np.float64)
    assert res.shape == (len(rows), 32), res.shape
    truth, tol, out = _truth_tol(d, mode)
    slot = {s: k for k, s in enumerate(T["slots"])}
    X = T[f"X{d}"][rows]
    report = {}

    def hold(name, got, want, bound, flag):
        pinned = np.isfinite(want) & ~np.isnan(bound)
        skipped = pinned & flag
        unbounded = pinned & ~flag & np.isinf(bound)
        use = pinned & ~flag & ~np.isinf(bound)
        bound = np.where(np.abs(want) < FLT_MIN, np.maximum(bound, FLT_MIN), bound)
        with np.errstate(all="ignore"):
            err = np.abs(got - want)
            ratio = np.where(err == 0, 0.0, err / bound)
        ratio = np.where(use, np.where(np.isnan(ratio), np.inf, ratio), 0.0)
        e = report.setdefault(name, {"max": 0.0, "item": -1, "n": 0, "skipped": 0, "unbounded": 0,
                                     "skipped_min_muR": None})
        if ratio.size and ratio.max() >= e["max"] and use.any():
            e["max"], e["item"] = float(ratio.max()), int(rows[np.argmax(ratio)])
        e["n"] += int(use.sum())
        e["skipped"] += int(skipped.sum())
        e["unbounded"] += int(unbounded.sum())
        if skipped.any():
            m = float(X[skipped].min())
            e["skipped_min_muR"] = m if e["skipped_min_muR"] is None else min(m, e["skipped_min_muR"])

    def col(s):
        k = slot[s]
        return truth[:, k], tol[:, k], out[:, k]

    names = {"A0": "A0", "A1": "A1", "B0": "B0", "B1": "B1", "pk": "poisson_kernel", "norm": "norm", "ev": "evaluate",
             "gn": "gradient_norm", "dpk": "dir_sampled_poisson_kernel", "exy": "evaluate_xy", "fsG": "fs_evaluate"}
    for s, name in names.items():
        if s == "fsG" and d == 3:
            continue
        t, e, o = col(s)
        hold(name, res[:, COL[s]], t, e, o)
    dV, dS = T[f"dV{d}"][rows], T[f"dS{d}"][rows]
    for k in range(d):
        with np.errstate(invalid="ignore"):  # (an infinite bound times a zero component: not pinned)
            t, e, o = col("gn")
            hold("gradient", res[:, 23 + k], t * dV[:, k], e * np.abs(dV[:, k]) + 2 * U * np.abs(t * dV[:, k]), o)
            t, e, o = col("pkg")
            hold("poisson_kernel_gradient", res[:, 10 + k], t * dS[:, k],
                 e * np.abs(dS[:, k]) + 2 * U * np.abs(t * dS[:, k]), o)
    r = T[f"r{d}"][rows]
    pdf = 1.0 / (2 * np.pi * r) if d == 2 else 1.0 / (4 * np.pi * r * r)
    hold("pdf_sphere_uniform", res[:, 22], pdf, 2 * U * pdf, np.zeros(len(rows), bool))
    if d == 2:
        xy, n = T["xy2"][rows], T["n2"][rows]
        g, eg, og = col("fsg")
        c, ec, oc = col("fsc")
        nd = n[:, 0] * xy[:, 0] + n[:, 1] * xy[:, 1]
        e_nd = 2 * U * (np.abs(n[:, 0] * xy[:, 0]) + np.abs(n[:, 1] * xy[:, 1]))
        for k in range(2):
            v = -xy[:, k]
            hold("fs_gradient", res[:, 27 + k], g * v, eg * np.abs(v) + 2 * U * np.abs(g * v), og)
            a, b = n[:, k] * g, nd * c * xy[:, k]
            hold("fs_poisson_gradient", res[:, 30 + k], a - b,
                 eg * np.abs(n[:, k]) + ec * np.abs(nd * xy[:, k]) + c * np.abs(xy[:, k]) * e_nd
                 + 3 * U * (np.abs(a) + np.abs(b)), og | oc)
        P = nd * g
        hold("fs_poisson", res[:, 29], P, eg * np.abs(nd) + g * e_nd + 2 * U * np.abs(P), og)
    return report


def same_bits(a, b):
    """Bit equality of two float32 arrays, every NaN counted as one pattern (a NaN's sign and payload
    are the hardware's choice); infinities and signed zeros compare as they are."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    ua, ub = a.view(np.uint32).copy(), b.view(np.uint32).copy()
    ua[np.isnan(a)] = 0x7FC00000
    ub[np.isnan(b)] = 0x7FC00000
    return ua == ub


# (member, pairs) a reference-semantics comparison leaves out because a float intermediate leaves the
# float range, as the model predicts it (all above mu R = 85: K0 underflows past 85.2, exp(-mu R) past
# 87.3, I0 overflows past 91.9, 1 / (2 exp(-mu R)) past 88.0), and the pairs whose bound is infinite
# (the 3D float I32 = cosh - sinh / x below mu R ~ 5e-3 cancels completely: B1, hence gradient_norm,
# gradient and poisson_kernel_gradient, carry no information)
_RANGE_2D = {"A1": (288, 0), "B1": (288, 0), "poisson_kernel": (288, 0), "norm": (288, 0), "evaluate": (288, 0),
             "gradient_norm": (288, 0), "dir_sampled_poisson_kernel": (288, 0), "evaluate_xy": (288, 0),
             "gradient": (576, 0), "poisson_kernel_gradient": (824, 0)}
_RANGE_3D = {"A1": (384, 0), "B1": (384, 0), "poisson_kernel": (384, 0), "norm": (384, 0), "evaluate": (384, 0),
             "gradient_norm": (384, 480), "dir_sampled_poisson_kernel": (384, 0), "evaluate_xy": (384, 0),
             "gradient": (998, 1044), "poisson_kernel_gradient": (998, 1048)}
LEFT_OUT = {(2, 1): _RANGE_2D, (3, 1): _RANGE_3D,
            (3, 2): {"gradient_norm": (0, 480), "gradient": (0, 1044), "poisson_kernel_gradient": (0, 1048)}}


def check_report(d, mode, rep):
    for name, e in rep.items():
        print(f"gfn d={d} mode={mode} {name}: max err/tol {e['max']:.4g} at item {e['item']}, {e['n']} pairs, "
              f"{e['skipped']} out of range (mu R >= {e['skipped_min_muR']}), {e['unbounded']} unbounded")
    for name, e in rep.items():
        assert e["max"] <= 1.0, (d, mode, name, e)
        if mode != 1:
            assert e["skipped"] == 0, (d, mode, name, e)
        elif e["skipped"]:
            assert e["skipped_min_muR"] > 85.0, (d, mode, name, e)
        if e["unbounded"]:
            assert d == 3 and mode != 0 and name in ("gradient_norm", "gradient", "poisson_kernel_gradient"), (d, mode, name, e)
    got = {name: (e["skipped"], e["unbounded"]) for name, e in rep.items() if e["skipped"] or e["unbounded"]}
    assert got == LEFT_OUT.get((d, mode), {}), (d, mode, got)
