"""Writes tests/golden/gfn_truth.npz: the items of the Green's-function probe and, per item,
the 50-digit model's values (tests/gfn_model.py) with the derived error bound of every member
under each mode.  Deterministic (no random draws); python tests/golden/make_gfn_truth.py [--jobs N].

Per dimension d (2, 3):
  items{d}   float32 [n, 20]  the probe's items (include/wos.h WOS_GFN_ITEM); rows [0, nA) are the
                             reference grid (modes 0, 1, 2), [nA, nAB) the robust grid (mode 2),
                             [nAB, n) the free-space sweep (every mode; only fsG fsg fsc are pinned)
  kind{d}    int8 [n]         0, 1, 2 for the three row ranges
  th{d}      float64 [nA + nF, S]  harmonic truth of rows kind 0 and 2, S = len(SLOTS)
  ty{d}      float64 [n, S]   Yukawa truth; NaN: not pinned (slot does not apply to the row)
  tys{d}     float64 [n, 4]   2D: the scaled members ke0 ie0 ke1 ie1 where mu R > 80 (NaN elsewhere)
  eh{d}, e1{d}, e2{d}  float32, same shapes as th / ty / ty: the bounds under mode 0, 1, 2
                             (rounded up; inf: the expression carries no information); e2 holds
                             rows with mu R > 80 only (idx2{d}), at or below it mode 2 is mode 1
  out1{d}    bool, shape of e1: a float intermediate of the member leaves the float range
"""
import argparse
import os
import sys
from multiprocessing import Pool

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gfn_model as M  # noqa: E402

SLOTS = M.BALL_SLOTS + M.ITEM_SLOTS
HERE = os.path.dirname(os.path.abspath(__file__))
LAMBDAS = (1e-2, 1.0, 50.0, 350.0, 1e4)
RATIOS = ("clamp", 1e-3, 1e-2, 0.1, 0.3, 0.5, 0.7, 0.9, 0.99, 0.999, 1.0 - 2.0 ** -20, 1.0)
FAR = (37.25, -11.5, 3.125)
f32 = np.float32


def mur_reference():
    grid = list(np.exp(np.linspace(np.log(2e-4), np.log(200.0), 40)))
    # the robust threshold, K0's underflow (85.2), exp(-mu R)'s (87.3), I0's overflow (91.9), exp's flush (103.3)
    return grid + [79.9, 80.0, 80.1, 85.0, 86.0, 87.2, 87.5, 88.5, 90.0, 91.5, 92.5, 103.0, 104.5]


def mur_robust():
    return list(np.exp(np.linspace(np.log(80.0), np.log(700.0), 20)))


def radius_for(mur, lam):
    """R with fl(R fl(sqrt(lam))) as close to mur as a float R gets (exactly mur where one exists)."""
    sl = np.sqrt(f32(lam), dtype=np.float32)
    R = f32(f32(mur) / sl)
    best = R
    for k in range(-3, 4):
        Rk = R
        for _ in range(abs(k)):
            Rk = np.nextafter(Rk, f32(np.inf if k > 0 else 0), dtype=np.float32)
        if abs(float(f32(Rk * sl)) - float(f32(mur))) < abs(float(f32(best * sl)) - float(f32(mur))):
            best = Rk
    return best


def unit_dirs(d):
    if d == 2:
        v = [(1.0, 0.0, 0.0), (0.6, 0.8, 0.0), (-0.28, 0.96, 0.0), (0.0, -1.0, 0.0), (-0.8, -0.6, 0.0)]
    else:
        v = [(1.0, 0.0, 0.0), (2 / 3, -2 / 3, 1 / 3), (0.36, 0.48, -0.8), (0.0, 0.0, -1.0), (-3 / 7, 6 / 7, 2 / 7)]
    return np.asarray(v, np.float32)


def ball_rows(d, murs, lam_per_pair, offset):
    dirs = unit_dirs(d)
    rows = []
    j = offset
    for mi, mur in enumerate(murs):
        for ri, ratio in enumerate(RATIOS):
            for li in range(lam_per_pair):
                lam = LAMBDAS[(mi + ri + li) % len(LAMBDAS)]
                R = radius_for(mur, lam)
                r = M.RCLAMP if ratio == "clamp" else max(M.RCLAMP, f32(R * f32(ratio)))
                if r > R:
                    r = f32(R / f32(2))  # sample_volume's own fallback
                c = np.asarray(FAR if j % 2 else (0, 0, 0), np.float32)
                u, v = dirs[j % 5], dirs[(j + 2) % 5]
                it = np.zeros(20, np.float32)
                it[0], it[1], it[2] = R, lam, r
                it[3:6], it[6:9] = c, dirs[(j + 1) % 5]
                # x, y inside the ball with |y - x| <= R and (x - c).(y - c) >= 0, so that evaluate_xy's two
                # arguments stay at or below mu R as in the solve (which calls it with x = c): x at the
                # centre, both off it (w bisects u and v), and |y - x| below rClamp
                w = (u + v) / np.sqrt(np.sum((u + v) ** 2, dtype=np.float32), dtype=np.float32)
                case = j % 4
                if case == 0:
                    x, y = c, c + f32(0.5) * R * u
                elif case == 1:
                    x, y = c + f32(0.3) * R * u, c + f32(0.5) * R * w
                elif case == 2:
                    x = c + f32(0.2) * R * u
                    y = x + min(f32(3e-5), f32(0.3) * R) * w  # (still inside balls smaller than rClamp)
                else:
                    x, y = c + f32(0.6) * R * u, c + f32(0.8) * R * w
                it[9:12], it[12:15] = x, y
                it[15:17] = dirs[(j + 3) % 5][:2] if d == 2 else (1.0, 0.0)
                it[17] = 1e-3
                if d == 2:
                    it[[5, 8, 11, 14]] = 0.0
                rows.append(it)
                j += 1
    return rows


def freespace_rows(d):
    """mu r from 1e-6 to 700 across bessel_ik's branch points 2 and 3.75, the radius clamp above and
    below |y - x|, the normal parallel, orthogonal, opposite and oblique to x - y; benign unit ball."""
    murs = list(np.exp(np.linspace(np.log(1e-6), np.log(700.0), 36))) + [1.99, 2.0, 2.01, 3.74, 3.75, 3.76]
    rows = []
    j = 0
    for mur in murs:
        for ni, ang in enumerate((0.0, np.pi / 2, np.pi, 0.7)):
            lam = LAMBDAS[(j + ni) % 5]
            dist = mur / np.sqrt(lam)
            phi = 0.37 * j
            e = np.asarray((np.cos(phi), np.sin(phi)))
            y = np.asarray((0.125, -0.25)) if j % 2 else np.asarray((21.5, -7.75))
            x = y + dist * e  # x - y = dist e
            it = np.zeros(20, np.float32)
            it[0], it[1], it[2] = 1.0, lam, 0.5
            it[6] = 1.0
            it[9:11], it[12:14] = x, y
            it[15:17] = (np.cos(phi + ang), np.sin(phi + ang))
            it[17] = (1e-3, 1e-3, 2.0 * dist, 1e-2)[(j // 2) % 4]  # every third pair clamped
            rows.append(it)
            j += 1
    return rows


def make_items(d):
    A = ball_rows(d, mur_reference(), 4, 0)
    B = ball_rows(d, mur_robust(), 2, 1)
    F = freespace_rows(d)
    items = np.asarray(A + B + F, np.float32)
    kind = np.asarray([0] * len(A) + [1] * len(B) + [2] * len(F), np.int8)
    return items, kind


def _up32(v):
    """float32 not below the mpf v."""
    if not M.mp.isfinite(v):
        return f32(np.inf)
    with np.errstate(over="ignore"):
        x = f32(float(v))
    return x if M.mpf(float(x)) >= v else np.nextafter(x, f32(np.inf), dtype=np.float32)


def row_values(args):
    """(truth [S], bound [S], out [S]) of one item under one mode."""
    d, mode, it, kind = args
    t = M.truth(d, mode != 0, it, fs_only=kind == 2)
    b = M.bounds(d, mode, it)
    tv = np.full(len(SLOTS), np.nan)
    ev = np.full(len(SLOTS), np.nan, np.float32)
    ov = np.zeros(len(SLOTS), bool)
    ts = np.full(4, np.nan)
    scaled = mode == 2 and M.float_args(d, it)["X"] > M.ROBUST_MUR
    for k, s in enumerate(SLOTS):
        tk = t.get(s, M.mp.nan)
        if scaled and d == 2 and s + "s" in t:
            ts[k] = float(t[s + "s"])
            tk = t[s + "s"]
        if s not in b or M.mp.isnan(tk):
            continue
        if s in ("A0", "A1", "B0", "B1") and (mode == 0 or (scaled and d == 3)):
            continue
        tv[k] = float(tk)
        tol, out = M.tolerance(b[s], tk)
        ev[k], ov[k] = _up32(tol), out
    return tv, ev, ov, ts


def table(pool, d, mode, items, kind, rows):
    res = pool.map(row_values, [(d, mode, items[i], int(kind[i])) for i in rows], chunksize=16)
    return (np.asarray([r[0] for r in res]), np.asarray([r[1] for r in res]), np.asarray([r[2] for r in res]),
            np.asarray([r[3] for r in res]))


def build(jobs):
    out = {"slots": np.asarray(SLOTS)}
    with Pool(jobs) as pool:
        for d in (2, 3):
            items, kind = make_items(d)
            n = len(items)
            X = np.asarray([M.float_args(d, it)["X"] for it in items])
            rows_h = np.flatnonzero(kind != 1)
            rows_1 = np.arange(n)
            idx2 = np.flatnonzero(X > M.ROBUST_MUR)
            th, eh, _, _ = table(pool, d, 0, items, kind, rows_h)
            ty, e1, o1, _ = table(pool, d, 1, items, kind, rows_1)
            t2, e2, _, ts = table(pool, d, 2, items, kind, idx2)
            tys = np.full((n, 4), np.nan)
            tys[idx2] = ts
            # at a scaled 2D ball the members' truth is tys; every other slot's truth is mode 1's
            out.update({f"items{d}": items, f"kind{d}": kind, f"th{d}": th, f"ty{d}": ty, f"tys{d}": tys,
                        f"eh{d}": eh, f"e1{d}": e1, f"e2{d}": e2, f"idx2{d}": idx2.astype(np.int32),
                        f"out1{d}": o1})
            print(d, n, (kind == 0).sum(), (kind == 1).sum(), (kind == 2).sum(), len(idx2), flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(HERE, "gfn_truth.npz"))
    a = ap.parse_args()
    np.savez_compressed(a.out, **build(a.jobs))
    print(a.out, os.path.getsize(a.out))
