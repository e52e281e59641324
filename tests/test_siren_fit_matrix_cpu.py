"""The matrix form of the fit step's scale without a GPU (include/wos.h WOS_FIT_SCALE_MATRIX;
wos_amd.siren.affine_wrap, wos_amd.projection.slip_wrap): the flag is declared within ABI 10 and
refused with a NULL scale by every entry point before any device work; the Python layer names both
forms of `scale` when it refuses a shape; the float64 restatement equals torch float64 autograd and
the f32 chains on a diagonal matrix equal the diagonal step's; affine_wrap classifies the karman wrap
as diagonal with diagonal_wrap's bits and a slip wrap as mixing, refuses a nonlinear one by name and
handles d_out = 3; the time-stepper layer classifies a wrap once; divergence_with_wrap through
slip_wrap equals float64 autograd."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import siren_fit_matrix_model as mm
import siren_fit_model as fm
import siren_model as sm
import siren_vjp_model as vm
from wos_amd import _lib, siren
from wos_amd import projection as pj

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "wos.h")


# ---- ABI ---------------------------------------------------------------------------------------------
def test_the_flag_is_declared_within_abi_10_and_bound():
    txt = open(HEADER).read()
    assert re.search(r"#define WOS_FIT_SCALE_MATRIX 0x4u\b", txt) and _lib.WOS_FIT_SCALE_MATRIX == 0x4
    assert _lib.WOS_FIT_SCALE_MATRIX & (_lib.WOS_PTRS_DEVICE | _lib.WOS_ASYNC) == 0
    assert re.search(r"#define WOS_ABI_VERSION 10\b", txt) and _lib.load().wos_abi_version() == 10
    assert "older than this flag ignores the bit" in txt


# ---- refusals that need no device --------------------------------------------------------------------
def _net_struct(d=2, H=32, Lh=1, d_out=2, seed=0):
    p = siren.pack(sm.make_net(d, H, Lh, d_out, seed=seed))
    ws, bs = [t.numpy() for t in p.weights], [t.numpy() for t in p.biases]
    w = (C.c_void_p * (Lh + 2))(*[a.ctypes.data for a in ws])
    b = (C.c_void_p * (Lh + 2))(*[a.ctypes.data for a in bs])
    return _lib.SirenNet(p.d_in, p.d_out, p.hidden, p.n_hidden_layers, p.omega, w, b), (ws, bs, w, b)


def test_the_flag_with_a_null_scale_is_refused_by_every_entry_point_before_any_device_work():
    """Host memory throughout: a call that got as far as a launch would fail otherwise, not with -1 and this text."""
    L = _lib.load()
    n, K = 5, 2
    net, keep = _net_struct()
    x, t = sm.points(2, n), np.zeros((n, 2), np.float32)
    loss, losses, status = np.full(1, 7.0, np.float32), np.full(2 * K, 7.0, np.float32), np.full(4, 7, np.int64)
    m, v = np.zeros(4096, np.float32), np.zeros(4096, np.float32)
    idx = np.zeros((K, n), np.int64)
    offsets = (C.c_int64 * (K + 1))(0, 2, 5)
    opt = _lib.AdamParams(1e-4, 0.9, 0.999, 1e-8, -1.0)
    flag = _lib.WOS_FIT_SCALE_MATRIX
    rc = L.wos_siren_fit(C.byref(net), x.ctypes.data, n, t.ctypes.data, None, loss.ctypes.data, None, None, 0, flag, 0, None)
    assert rc == -1 and L.wos_last_error().startswith(b"wos_siren_fit: null scale with WOS_FIT_SCALE_MATRIX")
    tail = (0, C.byref(opt), -1.0, 0, losses.ctypes.data, status.ctypes.data, 0, _lib.WOS_PTRS_DEVICE | flag, 0, None)
    rc = L.wos_siren_fit_run(C.byref(net), x.ctypes.data, t.ctypes.data, None, n, idx.ctypes.data, K, n, m.ctypes.data,
                             v.ctypes.data, *tail)
    assert rc == -1 and L.wos_last_error().startswith(b"wos_siren_fit_run: null pool_scale with WOS_FIT_SCALE_MATRIX")
    rc = L.wos_siren_fit_run_batches(C.byref(net), x.ctypes.data, t.ctypes.data, None, offsets, K, m.ctypes.data,
                                     v.ctypes.data, *tail)
    assert rc == -1 and L.wos_last_error().startswith(b"wos_siren_fit_run_batches: null scale with WOS_FIT_SCALE_MATRIX")
    # the ensemble forms: a NULL array, and an array whose every entry is NULL
    other, keep2 = _net_struct(seed=1)
    nets = (_lib.SirenNet * 2)(net, other)
    ts = (C.c_void_p * 2)(t.ctypes.data, t.ctypes.data)
    ms, vs = (C.c_void_p * 2)(m.ctypes.data, m[2048:].ctypes.data), (C.c_void_p * 2)(v.ctypes.data, v[2048:].ctypes.data)
    for scales in (None, (C.c_void_p * 2)(None, None)):
        rc = L.wos_siren_fit_run_ensemble(2, nets, x.ctypes.data, ts, scales, n, idx.ctypes.data, K, n, ms, vs, *tail)
        assert rc == -1 and L.wos_last_error().startswith(b"wos_siren_fit_run_ensemble: null pool_scale with WOS_FIT_SCALE_MATRIX")
        rc = L.wos_siren_fit_run_batches_ensemble(2, nets, x.ctypes.data, ts, scales, offsets, K, ms, vs, *tail)
        assert rc == -1 and L.wos_last_error().startswith(b"wos_siren_fit_run_batches_ensemble: null scale with "
                                                           b"WOS_FIT_SCALE_MATRIX")
    assert loss[0] == 7.0 and np.all(losses == 7.0) and np.all(status == 7), "a refused call wrote nothing"
    del keep, keep2


def test_python_layer_names_both_forms_of_scale():
    net = sm.make_net(2, 32, 1)
    x, t = sm.points(2, 5), np.zeros((5, 2), np.float32)
    both = r"scale must have shape \(5, 2\) \(a factor per component\) or \(5, 2, 2\) \(a matrix per point\), got "
    for bad in (np.ones((5, 1), np.float32), np.ones((5, 2, 1), np.float32), np.ones((5, 3, 3), np.float32),
                np.ones((5, 2, 2, 2), np.float32), np.ones((4, 2, 2), np.float32), np.ones((2, 2), np.float32)):
        with pytest.raises(ValueError, match=both + re.escape(str(bad.shape))):
            siren.fit(net, x, t, bad)
        with pytest.raises(ValueError, match=both + re.escape(str(bad.shape))):
            siren.fit(net, x, t, bad, grads=False)
    one = sm.make_net(3, 32, 1, 1)  # d_out = 1: (5, 1) and (5, 1, 1) are the two forms, (5,) is neither
    with pytest.raises(ValueError, match=r"\(5, 1\) \(a factor per component\) or \(5, 1, 1\) \(a matrix per point\), got \(5,\)"):
        siren.fit(one, sm.points(3, 5), np.zeros((5, 1), np.float32), np.ones(5, np.float32))
    with pytest.raises(ValueError, match="scale.requires_grad"):
        siren.fit_loss(net, torch.from_numpy(x), torch.from_numpy(t), torch.ones(5, 2, 2).requires_grad_(True))


# ---- the model ---------------------------------------------------------------------------------------
MODEL_SHAPES = [(2, 32, 1, 2), (3, 64, 2, 3), (2, 64, 0, 3), (3, 32, 1, 2), (3, 32, 1, 1)]


@pytest.mark.parametrize("d,H,L,d_out", MODEL_SHAPES, ids=[f"d{d}_H{H}_L{L}_o{o}" for d, H, L, o in MODEL_SHAPES])
def test_float64_model_equals_float64_autograd(d, H, L, d_out):
    """Float64 identities: 1e-9 of each tensor's largest entry."""
    net = sm.make_net(d, H, L, d_out)
    x = sm.points(d, 37, seed=3)
    target, S = mm.problem(37, d_out, seed=5)
    assert np.any(S == 0) and np.any(np.all(S == 0, axis=(1, 2))) and np.all(np.any(S != 0, axis=0)), "the case"
    loss, got, ub = mm.model64(net, x, target, S)
    want_loss, want = mm.autograd(vm.net64(net), torch.from_numpy(x.astype(np.float64)), target, S)
    assert abs(loss - want_loss) <= 1e-12 * want_loss and loss > 0
    for kind, G, W in (("w", got[0], want[0]), ("b", got[1], want[1])):
        for l, (a, b) in enumerate(zip(G, W)):
            top = np.abs(b).max()
            assert a.shape == b.shape and top > 0 and np.abs(a - b).max() <= 1e-9 * top, (kind, l)


def test_the_f32_chains_on_a_diagonal_matrix_are_the_diagonal_steps():
    """fmaf(0, u, r) = r: with exact zeros off the diagonal the restated chains give r = fmaf(s, u, -t) and
    ub = (s (r + r)) / N, the diagonal step's values (the sign of an exact zero aside)."""
    rng = np.random.default_rng(3)
    for d_out in (1, 2, 3):
        n = 101
        u = rng.standard_normal((n, d_out)).astype(np.float32)
        target, scale = fm.problem(n, d_out, True, seed=d_out)
        S = mm.diagonal(scale)
        r = mm.residual32(u, target, S)
        want_r = mm._fma32(scale, u, -target)
        assert np.array_equal(r, want_r)
        inv = np.float32(1.0) / np.float32(n * d_out)
        assert np.array_equal(mm.seed32(r, S, n * d_out), (scale * (want_r + want_r)) * inv)
        r64, ub64, _ = mm.seeds64(u, target, S)
        want64 = fm.seeds64(u, target, scale)
        assert np.array_equal(r64, want64[0]) and np.array_equal(ub64, want64[1])


# ---- affine_wrap -------------------------------------------------------------------------------------
SIZE = [0.0, 2.2, 0.0, 1.0]


def circle_normal(centre):
    def normal(x):
        r = x - torch.as_tensor(centre, dtype=x.dtype, device=x.device)
        return r / torch.sqrt((r * r).sum(-1, keepdim=True))
    return normal


def circle_weight(centre, radius, eps):
    def weight(x):
        r = x - torch.as_tensor(centre, dtype=x.dtype, device=x.device)
        return ((torch.sqrt((r * r).sum(-1)) - radius) / eps).clamp(min=0, max=1)
    return weight


def _slip(dim=2):
    centre = [0.7, 0.5, 0.4][:dim]
    return pj.slip_wrap(circle_normal(centre), circle_weight(centre, 0.2, 0.25))


def tanh_wrap(x, u):
    return torch.tanh(u)


def _points64(dim=2, n=301):
    x = torch.from_numpy(sm.points(dim, n, seed=9).astype(np.float64))
    x[:40, 0] = torch.linspace(0.0, 0.125, 40, dtype=torch.float64)  # the inlet strip, both ends included
    return x


def test_affine_wrap_returns_the_karman_wrap_diagonal_with_diagonal_wraps_bits():
    x = _points64()
    for wrap in (sm.karman_wrap(SIZE, eps=0.125), sm.karman_wrap(SIZE, eps=0.125, detach_weight=False)):
        scale, offset, mixes = siren.affine_wrap(wrap, x, 2)
        want_scale, want_offset = siren.diagonal_wrap(wrap, x, 2)
        assert mixes is False and scale.shape == (301, 2) and scale.dtype == torch.float64
        assert torch.equal(scale, want_scale) and torch.equal(offset, want_offset)
        assert not scale.requires_grad and not offset.requires_grad
    x32 = x.float()
    scale, offset, mixes = siren.affine_wrap(sm.karman_wrap(SIZE, eps=0.125), x32, 2)
    want_scale, want_offset = siren.diagonal_wrap(sm.karman_wrap(SIZE, eps=0.125), x32, 2)
    assert not mixes and scale.dtype == torch.float32 and torch.equal(scale, want_scale) and torch.equal(offset, want_offset)


@pytest.mark.parametrize("dim", [2, 3])
def test_affine_wrap_returns_the_matrix_of_a_slip_wrap(dim):
    x = _points64(dim)
    slip = _slip(dim)
    S, offset, mixes = siren.affine_wrap(slip, x, dim)
    assert mixes is True and S.shape == (301, dim, dim) and offset.shape == (301, dim) and not S.requires_grad
    assert bool((offset == 0).all())
    n, w = circle_normal([0.7, 0.5, 0.4][:dim])(x), circle_weight([0.7, 0.5, 0.4][:dim], 0.2, 0.25)(x)
    assert 0 < int((w == 0).sum()) and 0 < int((w == 1).sum()) and 0 < int(((w > 0) & (w < 1)).sum()), "the case"
    want = torch.eye(dim, dtype=x.dtype) - (1 - w)[:, None, None] * n[:, :, None] * n[:, None, :]
    assert float((S - want).abs().max()) <= 1e-15
    N = torch.from_numpy(np.random.default_rng(1).standard_normal((301, dim)))
    got = (S @ N.unsqueeze(-1)).squeeze(-1) + offset
    assert float((got - slip(x, N)).abs().max()) <= 1e-14
    # where the weight is 1 the wrap is the identity, where it is 0 the velocity is tangential
    assert torch.equal(slip(x, N)[w == 1], N[w == 1])
    assert float((slip(x, N) * n).sum(-1)[w == 0].abs().max()) <= 1e-14
    # masks composed around it: an inlet clamp after the slip keeps the form affine, with an offset
    karman = sm.karman_wrap(SIZE, eps=0.125)

    def composed(x_, u):
        return karman(x_, slip(x_, u))
    S2, offset2, mixes2 = siren.affine_wrap(composed, x, dim)
    assert mixes2 and bool((offset2[:40, 0] == 0.5).all()) and bool((S2[:40, 0] == 0).all())
    assert float(((S2 @ N.unsqueeze(-1)).squeeze(-1) + offset2 - composed(x, N)).abs().max()) <= 1e-14


def test_affine_wrap_refuses_a_nonlinear_wrap_by_name():
    x = _points64()
    with pytest.raises(ValueError, match="siren.affine_wrap: wrap 'tanh_wrap' is not affine in the network's output"):
        siren.affine_wrap(tanh_wrap, x, 2)
    S, offset, mixes = siren.affine_wrap(tanh_wrap, x, 2, check=False)  # unchecked: the caller's risk
    assert not mixes and S.shape == (301, 2)
    with pytest.raises(ValueError, match=r"wrap returned shape \(301, 3\) for an output of \(301, 2\)"):
        siren.affine_wrap(lambda x_, u: torch.cat([u, u[..., :1]], -1), x, 2)
    with pytest.raises(ValueError, match="slip_wrap.*not diagonal-affine.*affine_wrap"):
        siren.diagonal_wrap(_slip(), x, 2)  # diagonal_wrap stays as it is, and names the other route


# ---- the time-stepper layer --------------------------------------------------------------------------
def test_a_wrap_is_classified_once(monkeypatch):
    x = _points64().float()
    calls = []
    real = siren.affine_wrap

    def counting(wrap, *a, **kw):
        calls.append(wrap)
        return real(wrap, *a, **kw)
    monkeypatch.setattr(siren, "affine_wrap", counting)
    slip, karman = _slip(), sm.karman_wrap(SIZE, eps=0.125)
    first = pj._affine(slip, x, 2)
    again = pj._affine(slip, x[:100], 2)
    assert calls == [slip] and first[0].shape == (301, 2, 2) and again[0].shape == (100, 2, 2)
    assert torch.equal(again[0], first[0][:100]) and torch.equal(again[1], first[1][:100])
    first = pj._affine(karman, x, 2)
    again = pj._affine(karman, x[:100], 2)
    assert calls == [slip, karman] and first[0].shape == (301, 2) and again[0].shape == (100, 2)
    want = siren.diagonal_wrap(karman, x, 2)
    assert torch.equal(first[0], want[0]) and torch.equal(first[1], want[1]) and torch.equal(again[0], want[0][:100])
    with pytest.raises(ValueError, match="tanh_wrap.*not affine"):
        pj._affine(tanh_wrap, x, 2)
    with pytest.raises(ValueError, match="tanh_wrap.*not affine"):
        pj._affine(tanh_wrap, x, 2)  # a refusal is not cached as a verdict
    assert calls == [slip, karman, tanh_wrap, tanh_wrap]


def test_projection_fit_loss_hands_a_slip_wrap_over_as_a_matrix(monkeypatch):
    n, n_samples = 50, 64
    proj = pj.PressureProjector.__new__(pj.PressureProjector)
    proj.dim, proj.device = 2, torch.device("cpu")
    proj.samples = torch.from_numpy(sm.points(2, n, seed=4))
    grad_p = torch.from_numpy(np.random.default_rng(2).standard_normal((n, 2)).astype(np.float32))
    u_prev = torch.from_numpy(np.random.default_rng(3).standard_normal((n, 2)).astype(np.float32))
    seen = {}
    idx = torch.randint(0, n - 1, (n_samples,), generator=torch.Generator().manual_seed(123))
    monkeypatch.setattr(siren, "eval", lambda net, x, **kw: u_prev[idx] if x.shape[0] == n_samples else u_prev)

    def fake_fit_loss(module, x, target, scale=None):
        seen["fit"], seen["target"], seen["scale"] = x.clone(), target.clone(), scale
        return torch.zeros(())
    monkeypatch.setattr(siren, "fit_loss", fake_fit_loss)
    slip = _slip()
    proj.projection_fit_loss(object(), object(), grad_p, n_samples, wrap=slip, generator=torch.Generator().manual_seed(123))
    x = proj.samples[idx]
    S, offset, mixes = siren.affine_wrap(slip, x, 2)
    assert mixes and torch.equal(seen["fit"], x) and torch.equal(seen["scale"], S) and seen["scale"].shape == (n_samples, 2, 2)
    assert torch.equal(seen["target"], slip(x, u_prev[idx]) - grad_p[idx] - offset)


# ---- divergence_with_wrap through slip_wrap -----------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_divergence_with_wrap_through_a_slip_wrap_equals_float64_autograd(dim):
    net64 = vm.net64(sm.make_net(dim, 32, 1))
    x = torch.from_numpy(sm.points(dim, 97, seed=2).astype(np.float64))
    slip = _slip(dim)
    xa = x.clone().requires_grad_(True)
    want = pj.divergence(slip(xa, net64(xa)), xa)[..., 0].detach()
    u, jac, _ = sm.autograd_eval(net64, x)
    got = siren.divergence_with_wrap(x, u, jac, slip)
    assert got.shape == (97,) and not got.requires_grad
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    plain = jac.diagonal(dim1=-2, dim2=-1).sum(-1)
    assert float((got - plain).abs().max()) > 1e-3, "the wrap's own derivative and its mixing enter the divergence"
