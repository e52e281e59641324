"""Host restatement of the walk tape's operator and of its transpose, in numpy, from the arrays
WalkTape.read returns (or hand-built ones): the yardstick of tests/test_tape_adjoint_cpu.py and
tests/test_gpu_tape_adjoint.py.

A segment is a dict of the tape's arrays (include/wos.h wos_tape_read): code, cnt, slot, cell0,
gnorm, thr_end, term, tneu, bdir, sdir, cell, thr, nrm, pstate.  prm holds what the kernels read
from the recorded parameters: dim, wpp (records per point), n_anti, use_cv, ignore_source.

(a) forward(): replay + fold in the kernels' operation order (wos_tape_replay_kernel,
    wos_fold4_kernel), in the dtype asked for.  In float32 it is bit for bit tape.solve()'s p,
    grad and n_est; in float64 it is the operator A of the adjoint identity.
(b) adjoint(): the transpose in float64 as include/wos.h and DESIGN "Walk tape adjoint" state
    it, with, per cell, the absolute mass M = sum |a_j| |thr nrm| + sum |c_j| |gnorm| of the
    terms added there and their count k -- what the error bound of the device's float sum is
    made of.
"""
import numpy as np

FIELDS = ("code", "cnt", "slot", "cell0", "gnorm", "thr_end", "term", "tneu", "bdir", "sdir", "cell", "thr", "nrm",
          "pstate")
EST, MASK_P, MASK_G = 1, 2, 4  # pstate bits
OWN_G = 0x80000000             # cnt bit 31


def read_segments(tape):
    """Every segment of a WalkTape as a dict of numpy arrays."""
    return [{f: tape.read(f, k) for f in FIELDS} for k in range(len(tape.segments))]


def tape_prm(dim, solver, wpp):
    """The recorded parameters the fold and the replay read, from the solver keys."""
    return {"dim": dim, "wpp": int(wpp), "n_anti": 1 if solver.get("disableGradientAntitheticVariates") else 2,
            "use_cv": not solver.get("disableGradientControlVariates", False),
            "ignore_source": bool(solver.get("ignoreSource", False))}


def _walks(seg):
    """rec [T], first slot [T], entries [T] of a segment's tasks (dropped walks: 0 entries)."""
    rec = (seg["code"] & 1) != 0
    s0 = seg["slot"][:-1].astype(np.int64)
    cap = seg["slot"][1:].astype(np.int64) - s0
    n = np.where(rec, np.minimum((seg["cnt"] & np.uint32(OWN_G - 1)).astype(np.int64), cap), 0)
    return rec, s0, n


def replay(seg, f, prm, dtype, g=None):
    """total, first [T] for the flattened source f [cells] (wos_tape_replay_kernel's order).
    g: the channel's Dirichlet constant where a walk ended on constant data (several channels)."""
    dt = np.dtype(dtype).type
    rec, s0, n = _walks(seg)
    T = rec.shape[0]
    f = np.asarray(f, dtype).ravel()
    gn, thr_end, term, tneu = (seg[k].astype(dtype) for k in ("gnorm", "thr_end", "term", "tneu"))
    thr, nrm = seg["thr"].astype(dtype), seg["nrm"].astype(dtype)
    cell = seg["cell"].astype(np.int64)
    fst, tsrc = np.zeros(T, dtype), np.zeros(T, dtype)
    if not prm["ignore_source"]:
        fst[rec] = gn[rec] * f[seg["cell0"][rec].astype(np.int64)]
        tsrc = tsrc + dt(1) * fst
        for k in range(int(n.max()) if T else 0):
            act = np.nonzero(n > k)[0]
            e = s0[act] + k
            tsrc[act] = tsrc[act] + thr[e] * (nrm[e] * f[cell[e]])
    if g is not None:
        term = np.where((seg["cnt"] & np.uint32(OWN_G)) != 0, dt(g), term)
    total = np.where(rec, (thr_end * term + tneu) + tsrc, dt(0))
    return total.astype(dtype), np.where(rec, fst, dt(0)).astype(dtype)


def fold(seg, total, first, prm, dtype):
    """p [n], grad [n, dim], n_est [n] of a segment (wos_fold4_kernel's Welford chains)."""
    dt = np.dtype(dtype).type
    dim, wpp, n_anti = prm["dim"], prm["wpp"], prm["n_anti"]
    ps = seg["pstate"]
    nb = ps.shape[0]
    est = (ps & EST) != 0
    rec = ((seg["code"] & 1) != 0).reshape(nb, wpp)
    tot, fst = total.reshape(nb, wpp), first.reshape(nb, wpp)
    bdir = seg["bdir"].astype(dtype).reshape(dim, nb, wpp)
    sdir = seg["sdir"].astype(dtype).reshape(dim, nb, wpp)
    mean = np.zeros((1 + dim, nb), dtype)
    s_first, cvb, cvs = np.zeros(nb, dtype), np.zeros(nb, dtype), np.zeros(nb, dtype)
    s_n = np.zeros(nb, np.int32)
    for j in range(wpp):
        if j % n_anti == 0 and prm["use_cv"]:
            cvb = mean[0].copy()
            cvs = s_first / np.maximum(s_n, 1).astype(dtype)
        m = est & rec[:, j]
        s_n = s_n + m
        f_n = np.maximum(s_n, 1).astype(dtype)
        t, f = tot[:, j], fst[:, j]
        vals = [t] + [((t - f) - cvb) * bdir[k, :, j] + (f - cvs) * sdir[k, :, j] for k in range(dim)]
        for c in range(1 + dim):
            delta = vals[c] - mean[c]
            mean[c] = np.where(m, mean[c] + delta / f_n, mean[c])
        s_first = np.where(m, s_first + f, s_first)
    p = np.where((ps & MASK_P) != 0, dt(0), mean[0])
    g = np.where(((ps & MASK_G) != 0)[:, None], dt(0), mean[1:].T)
    return p.astype(dtype), np.ascontiguousarray(g, dtype), s_n


def forward(segs, source, prm, dtype=np.float32, g=None):
    """p [n], grad [n, dim], n_est [n] of a one-channel source over all segments."""
    out = [fold(s, *replay(s, source, prm, dtype, g), prm, dtype) for s in segs]
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3))


def adjoint_records(seg, P, G, prm):
    """a = dL/dtotal and c = dL/dfirst + a [T] in float64, for the upstream P [n], G [n, dim] of the
    segment's points."""
    dim, wpp, n_anti = prm["dim"], prm["wpp"], prm["n_anti"]
    ps = seg["pstate"]
    nb = ps.shape[0]
    est = (ps & EST) != 0
    rec = ((seg["code"] & 1) != 0).reshape(nb, wpp) & est[:, None]
    N = rec.sum(1)
    Pm = np.where(est & ((ps & MASK_P) == 0), np.asarray(P, np.float64), 0.0)
    Gm = np.where((est & ((ps & MASK_G) == 0))[:, None], np.asarray(G, np.float64).reshape(nb, dim), 0.0)
    bdir = seg["bdir"].astype(np.float64).reshape(dim, nb, wpp)
    sdir = seg["sdir"].astype(np.float64).reshape(dim, nb, wpp)
    B = np.where(rec, np.einsum("ik,kij->ij", Gm, bdir), 0.0)
    S = np.where(rec, np.einsum("ik,kij->ij", Gm, sdir), 0.0)
    npairs = wpp // n_anti
    recq = rec.reshape(nb, npairs, n_anti).sum(2)
    nbq = np.cumsum(recq, 1) - recq  # recorded walks before the pair
    w = np.where(nbq > 0, 1.0 / np.maximum(nbq, 1), 0.0) * (1.0 if prm["use_cv"] else 0.0)

    def suffix(X):  # per record: sum over the recorded walks of later pairs of X_r / nb(r)
        xq = X.reshape(nb, npairs, n_anti).sum(2) * w
        suf = np.cumsum(xq[:, ::-1], 1)[:, ::-1] - xq
        return np.repeat(suf, n_anti, axis=1)

    inv = np.where(N > 0, 1.0 / np.maximum(N, 1), 0.0)[:, None]
    a = np.where(rec, inv * (Pm[:, None] + B - suffix(B)), 0.0)
    c = np.where(rec, inv * (S - suffix(S)) + (a - B * inv), 0.0)
    return a.ravel(), c.ravel()


def adjoint(segs, P, G, prm, cells):
    """The transpose for one channel: (grad_source [cells] float64, M [cells], k [cells]).
    Zero with ignore_source."""
    out, M, k = np.zeros(cells), np.zeros(cells), np.zeros(cells, np.int64)
    if prm["ignore_source"]:
        return out, M, k
    P = np.zeros(sum(s["pstate"].shape[0] for s in segs)) if P is None else np.asarray(P, np.float64)
    G = np.zeros((P.shape[0], prm["dim"])) if G is None else np.asarray(G, np.float64)
    b0 = 0
    for seg in segs:
        nb = seg["pstate"].shape[0]
        a, c = adjoint_records(seg, P[b0:b0 + nb], G[b0:b0 + nb], prm)
        b0 += nb
        rec, s0, n = _walks(seg)
        live = np.repeat((seg["pstate"] & EST) != 0, prm["wpp"]) & rec
        t = np.nonzero(live)[0]
        cell0 = seg["cell0"][t].astype(np.int64)
        gn = seg["gnorm"][t].astype(np.float64)
        np.add.at(out, cell0, c[t] * gn)
        np.add.at(M, cell0, np.abs(c[t]) * np.abs(gn))
        np.add.at(k, cell0, 1)
        nt = n[t]
        task = np.repeat(t, nt)
        start = np.cumsum(nt) - nt
        e = s0[task] + (np.arange(int(nt.sum())) - np.repeat(start, nt))
        w = seg["thr"][e].astype(np.float64) * seg["nrm"][e].astype(np.float64)
        ce = seg["cell"][e].astype(np.int64)
        np.add.at(out, ce, a[task] * w)
        np.add.at(M, ce, np.abs(a[task]) * np.abs(w))
        np.add.at(k, ce, 1)
    return out, M, k


def tolerance(M, k, wpp):
    """Per cell, the bound of |device float32 sum - float64 adjoint|: (k + 2 wpp + 16) 2^-24 M."""
    return (k + 2 * wpp + 16) * 2.0 ** -24 * M


def synthetic_segment(rng, dim, nb, wpp, cells, max_entries=5, drop=0.25):
    """A hand-built segment: random factors and cells, dropped walks, one point that is not
    estimated, one with p masked, one with the gradient masked, slots with unused tails."""
    T = nb * wpp
    rec = rng.random(T) > drop
    steps = rng.integers(1, max_entries + 2, T)
    code = ((steps << 1) | rec).astype(np.uint32)
    cap = np.where(rec, steps - 1, 0)
    slot = np.concatenate([[0], np.cumsum(cap)]).astype(np.uint32)
    used = np.where(rec, rng.integers(0, max_entries + 2, T) % (cap + 1), 0)  # entries written <= cap
    own_g = rng.random(T) < 0.3
    slots = int(slot[-1])
    ps = np.full(nb, EST, np.int32)
    ps[0], ps[1 % nb], ps[2 % nb] = 0, EST | MASK_P, EST | MASK_G
    f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    return {"code": code, "cnt": (used.astype(np.uint32) | np.where(own_g, np.uint32(OWN_G), np.uint32(0))),
            "slot": slot, "cell0": rng.integers(0, cells, T).astype(np.uint32), "gnorm": f32(T), "thr_end": f32(T),
            "term": f32(T), "tneu": f32(T), "bdir": f32(dim, T), "sdir": f32(dim, T),
            "cell": rng.integers(0, cells, max(slots, 1)).astype(np.uint32)[:slots], "thr": f32(slots),
            "nrm": f32(slots), "pstate": ps}
