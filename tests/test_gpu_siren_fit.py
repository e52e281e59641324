"""Fused SIREN fit step on the GPU (wos_siren_fit, csrc/wos_siren_fit.hip): accuracy of every
parameter gradient against the float64 model with float32 autograd of the same loss as the
yardstick, the loss against float64 of siren.eval's own u bits within the derived bound, tail
tiles, the weight-gradient kernel's second slice, chunks, determinism, the C ABI's pointer and
refusal rules, siren.fit_loss, and the time-stepper's two losses end to end.

Measured on the MI355X (ratios of the fit step's error to float32 autograd's, RMS / max, against
float64; the caps are 2.5 / 4): see profiles/siren_fit_accuracy.json."""
import copy
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import siren_fit_model as fm
import siren_model as sm
import siren_vjp_model as vm
from wos_amd import _lib, siren, workloads
from wos_amd import projection as pj

pytestmark = pytest.mark.gpu


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def host(out):
    """fit()'s (loss, gw, gb) on the host: (loss float32 scalar, ([w], [b]))."""
    loss, gw, gb = out
    return np.float32(loss.cpu().numpy()), ([t.cpu().numpy() for t in gw], [t.cpu().numpy() for t in gb])


def same_bits(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and all(
        np.array_equal(bits(s), bits(t)) for s, t in zip(a[1][0] + a[1][1], b[1][0] + b[1][1]))


def _cuda_net(d, H, L, d_out=None):
    return copy.deepcopy(sm.make_net(d, H, L, d_out)).cuda()


def _dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


SHAPES = [(2, 32, 1, None), (2, 128, 2, None), (2, 256, 3, None), (3, 256, 3, None), (3, 96, 2, None), (2, 64, 0, None),
          (3, 64, 1, 1),
          # H / 32 = 5, 6, 7: two row tiles per wave with a dropped duplicate, and a partial second 128-tile of dW
          (2, 160, 1, None), (3, 192, 2, None), (2, 224, 3, None),
          # the reference's depth, and L = 8 (12 reduce segments) at the smallest and the largest width
          (2, 256, 5, None), (3, 32, 8, None), (3, 256, 8, None),
          # d_out != d_in
          (2, 64, 1, 3), (3, 64, 1, 2), (2, 64, 1, 1)]


@functools.lru_cache(maxsize=None)
def _reference(d, H, L, d_out, with_scale, n=193):
    """(x, target, scale, float64 (loss, grads, ub), float32 autograd on the GPU) of one case, computed once."""
    net, x = sm.make_net(d, H, L, d_out), sm.points(d, n, seed=0)
    target, scale = fm.problem(n, d_out or d, with_scale)
    ref = fm.model64(net, x, target, scale)
    t32 = fm.autograd(_cuda_net(d, H, L, d_out), torch.from_numpy(x).cuda(), target, scale)
    return x, target, scale, ref, t32


def _fit(net, x, target, scale, **kw):
    return host(siren.fit(net, _dev(x), _dev(target), _dev(scale), **kw))


def _check(got, case, what, record=None):
    """Loss within the derived bound of float64 on eval's own u; gradients by the project's yardstick."""
    x, target, scale, (_, ref, ub), (_, t32) = case
    vm.assert_grads_as_accurate(got[1], t32, ref, ub, what, record=record)


def _loss64_from_eval(net, x, target, scale):
    u = siren.eval(net, _dev(x)).cpu().numpy()
    return fm.seeds64(u, target, scale)[2]


# ---- 1. accuracy against float64 -------------------------------------------------------------------------
CASES = [(s, w) for s in SHAPES for w in (False, True)]


@pytest.mark.parametrize("shape,with_scale", CASES,
                         ids=[f"d{s[0]}_H{s[1]}_L{s[2]}_o{s[3] or s[0]}_{'scale' if w else 'plain'}" for s, w in CASES])
def test_loss_and_gradients_against_float64(gpu, shape, with_scale):
    d, H, L, d_out = shape
    case = _reference(d, H, L, d_out, with_scale)
    x, target, scale = case[:3]
    net = _cuda_net(d, H, L, d_out)
    got = _fit(net, x, target, scale)
    L64 = _loss64_from_eval(net, x, target, scale)
    bound = fm.loss_bound(target.size, L64)
    print(f"loss {got[0]:.9e} float64 of eval's u {L64:.9e} error {abs(float(got[0]) - L64):.3e} bound {bound:.3e}")
    rec = {"loss_error": abs(float(got[0]) - L64), "loss_bound": bound}
    try:
        assert L64 > 0 and abs(float(got[0]) - L64) <= bound
        if with_scale:
            assert np.any(scale == 0)
        _check(got, case, f"({d},{H},{L},{d_out or d}) {'scale' if with_scale else 'plain'}", record=rec)
    finally:
        out = os.environ.get("WOS_SIREN_FIT_ACCURACY_OUT")  # a measuring run keeps the figures; the suite writes nothing
        if out:
            with open(out, "a") as f:
                f.write(json.dumps({"d": d, "hidden": H, "hidden_layers": L, "d_out": d_out or d, "points": 193,
                                    "scale": with_scale, **rec}) + "\n")


# ---- 2. point counts ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 32, 33, 65, 545])
def test_point_counts(gpu, n):
    """Tail tiles, and 545 = 17 tiles + 1 point: with one column per point the weight-gradient kernel's
    slice of 16 column blocks is 512 points, so the 17th tile is a second, one-block slice."""
    d, H, L = 2, 64, 1
    case = _reference(d, H, L, None, True, n)
    x, target, scale = case[:3]
    net = _cuda_net(d, H, L)
    got = _fit(net, x, target, scale)
    L64 = _loss64_from_eval(net, x, target, scale)
    assert abs(float(got[0]) - L64) <= fm.loss_bound(target.size, L64)
    if n == 1:
        # One point: nothing is summed, dbo is the seed itself, and assert_grads_as_accurate's bound for it,
        # (n - 1) 2^-24 sum |ub|, is zero.  The seed's own roundings remain -- r, scale (r + r), 1 / N and the
        # product with it -- so dbo is held to 4 * 2^-24 |ub| against float64 of eval's own u bits; every other
        # tensor by the yardstick.
        u = siren.eval(net, _dev(x)).cpu().numpy()
        ub = fm.seeds64(u, target, scale)[1]
        assert np.all(np.abs(got[1][1][-1] - ub[0]) <= 4 * 2.0 ** -24 * np.abs(ub[0]))
        (_, ref, _), (_, t32) = case[3], case[4]
        for kind in (0, 1):
            for l in range(L + 2):
                if kind == 1 and l == L + 1:
                    continue
                sm.assert_as_accurate_as_torch(got[1][kind][l], t32[kind][l], ref[kind][l], f"n = 1 d{'wb'[kind]}[{l}]")
        return
    _check(got, case, f"n = {n}")


def test_no_hidden_layer_host_pointers_equal_device_pointers(gpu):
    """L = 0: no packed copies, the temporary is the H zeros and the plan's work, for the loss alone the tiles'
    sums (accuracy at L = 0: SHAPES above)."""
    net, n = _cuda_net(2, 32, 0), 33  # one full tile and one point
    x = sm.points(2, n)
    target, scale = fm.problem(n, 2, True, seed=3)
    dev = siren.fit(net, *[torch.from_numpy(a).cuda() for a in (x, target, scale)])
    host = siren.fit(net, x, target, scale)
    assert np.array_equal(bits(host[0]), bits(dev[0])) and np.isfinite(host[0]) and host[0] > 0
    for kind in (1, 2):
        assert len(host[kind]) == 2
        for l, (a, b) in enumerate(zip(host[kind], dev[kind])):
            assert isinstance(a, np.ndarray) and np.array_equal(bits(a), bits(b)), (kind, l)
            assert np.isfinite(a).all() and np.abs(a).max() > 0, (kind, l)
    only_dev = siren.fit(net, *[torch.from_numpy(a).cuda() for a in (x, target, scale)], grads=False)
    only_host = siren.fit(net, x, target, scale, grads=False)
    assert np.array_equal(bits(only_dev), bits(host[0])) and np.array_equal(bits(only_host), bits(host[0]))


# ---- 3. chunks ---------------------------------------------------------------------------------------------
def _tile_bytes(H, L):
    return (2 * L + 1) * H * 4 * 32


@pytest.mark.parametrize("tiles", [1, 2])
def test_chunks_of_one_and_two_tiles(gpu, tiles):
    d, H, L = 2, 64, 1
    case = _reference(d, H, L, None, True)
    x, target, scale = case[:3]
    net = _cuda_net(d, H, L)
    ws = tiles * _tile_bytes(H, L) + 100  # 7 tiles in chunks of `tiles`; the slack must not buy another tile
    got = _fit(net, x, target, scale, workspace_bytes=ws)
    L64 = _loss64_from_eval(net, x, target, scale)
    assert abs(float(got[0]) - L64) <= fm.loss_bound(target.size, L64), "the call's n, not the chunk's"
    _check(got, case, f"chunks of {tiles}")
    assert same_bits(got, _fit(net, x, target, scale, workspace_bytes=ws))
    only = siren.fit(net, _dev(x), _dev(target), _dev(scale), grads=False, workspace_bytes=ws)
    assert np.array_equal(bits(only), bits(got[0])), "loss only, chunked alike: the same bits"


def test_workspace_below_one_tile_is_refused(gpu):
    x, target, scale = _reference(2, 64, 1, None, True)[:3]
    with pytest.raises(_lib.WosError, match="workspace_bytes"):
        _fit(_cuda_net(2, 64, 1), x, target, scale, workspace_bytes=_tile_bytes(64, 1) - 1)
    assert b"cannot hold one tile" in _lib.load().wos_last_error()


# ---- 4. determinism ----------------------------------------------------------------------------------------
def _c_net(p, ws, bs, ptr):
    n = p.n_hidden_layers + 2
    w = (C.c_void_p * n)(*[ptr(t) for t in ws])
    b = (C.c_void_p * n)(*[ptr(t) for t in bs])
    return _lib.SirenNet(p.d_in, p.d_out, p.hidden, p.n_hidden_layers, p.omega, w, b), (w, b)


@pytest.mark.parametrize("side", [False, True], ids=["current_stream", "side_stream"])
def test_determinism_loss_only_and_written_not_accumulated(gpu, side):
    d, H, L, n = 3, 256, 3, 193
    net = _cuda_net(d, H, L)
    x = _dev(sm.points(d, n))
    target, scale = [_dev(a) for a in fm.problem(n, d, True)]
    stream = torch.cuda.Stream() if side else None

    def run(**kw):
        out = siren.fit(net, x, target, scale, stream=stream, **kw)
        if side:
            stream.synchronize()
        return out
    first = host(run())
    assert same_bits(first, host(run())), "two calls, the same bits"
    assert np.isfinite(first[0]) and first[0] > 0
    assert all(np.isfinite(a).all() and np.any(a) for a in first[1][0] + first[1][1])
    before = dict(siren.fit_calls)
    only = run(grads=False)
    assert torch.is_tensor(only) and only.shape == () and only.is_cuda
    assert np.array_equal(bits(only), bits(first[0])), "the loss-only call returns the full call's loss bits"
    assert siren.fit_calls["loss_only"] == before.get("loss_only", 0) + 1 and siren.fit_calls["grads"] == before["grads"]
    # the C ABI on buffers full of NaN: written, not accumulated; and loss only with both arrays NULL
    p = siren.pack(net)
    nl = L + 2
    gw = [torch.full_like(t, float("nan")) for t in p.weights]
    gb = [torch.full_like(t, float("nan")) for t in p.biases]
    loss = torch.full((1,), float("nan"), device="cuda")
    st, keep = _c_net(p, p.weights, p.biases, lambda t: t.data_ptr())
    pw = (C.c_void_p * nl)(*[t.data_ptr() for t in gw])
    pb = (C.c_void_p * nl)(*[t.data_ptr() for t in gb])
    torch.cuda.synchronize()
    s = stream.cuda_stream if side else None
    flags = _lib.WOS_PTRS_DEVICE | _lib.WOS_ASYNC
    lib = _lib.load()
    rc = lib.wos_siren_fit(C.byref(st), x.data_ptr(), n, target.data_ptr(), scale.data_ptr(), loss.data_ptr(), pw, pb, 0,
                           flags, gpu, s)
    assert rc == 0, lib.wos_last_error()
    torch.cuda.synchronize()
    assert same_bits(first, host((loss[0], gw, gb))), "NaN-filled buffers come back as the first call's bits"
    for t in gw + gb:
        t.fill_(5.0)
    loss.fill_(float("nan"))
    torch.cuda.synchronize()
    rc = lib.wos_siren_fit(C.byref(st), x.data_ptr(), n, target.data_ptr(), scale.data_ptr(), loss.data_ptr(), None, None,
                           0, flags, gpu, s)
    assert rc == 0, lib.wos_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(bits(loss[0]), bits(first[0])) and all(bool((t == 5.0).all()) for t in gw + gb)


# ---- 5. C ABI ----------------------------------------------------------------------------------------------
def test_c_abi_pointers_and_refusals(gpu):
    lib = _lib.load()
    net = _cuda_net(2, 64, 1)
    p = siren.pack(net)
    n, nl = 45, 3
    x = sm.points(2, n)
    target, scale = fm.problem(n, 2, True)
    xd, td, sd = _dev(x), _dev(target), _dev(scale)
    want = host(siren.fit(net, xd, td, sd))
    want_plain = host(siren.fit(net, xd, td))
    # host pointers, blocking: weights, points, target, scale, loss and gradients all on the host
    hw, hb = [t.cpu().numpy() for t in p.weights], [t.cpu().numpy() for t in p.biases]
    hnet, keep_h = _c_net(p, hw, hb, lambda a: a.ctypes.data)
    ow, ob = [np.full(a.shape, np.nan, np.float32) for a in hw], [np.full(a.shape, np.nan, np.float32) for a in hb]
    hl = np.full(1, np.nan, np.float32)
    pw = (C.c_void_p * nl)(*[a.ctypes.data for a in ow])
    pb = (C.c_void_p * nl)(*[a.ctypes.data for a in ob])
    rc = lib.wos_siren_fit(C.byref(hnet), x.ctypes.data, n, target.ctypes.data, scale.ctypes.data, hl.ctypes.data, pw, pb,
                           0, 0, gpu, None)
    assert rc == 0, lib.wos_last_error()
    assert same_bits((hl[0], (ow, ob)), want), "host pointers equal device pointers"
    rc = lib.wos_siren_fit(C.byref(hnet), x.ctypes.data, n, target.ctypes.data, None, hl.ctypes.data, pw, pb, 0, 0, gpu, None)
    assert rc == 0, lib.wos_last_error()
    assert same_bits((hl[0], (ow, ob)), want_plain), "scale NULL is scale 1"
    ones = np.ones_like(scale)
    rc = lib.wos_siren_fit(C.byref(hnet), x.ctypes.data, n, target.ctypes.data, ones.ctypes.data, hl.ctypes.data, pw, pb, 0,
                           0, gpu, None)
    assert rc == 0 and same_bits((hl[0], (ow, ob)), want_plain), "scale of ones: the same bits as none"
    for a in ow + ob:
        a.fill(3.0)
    hl.fill(np.nan)
    rc = lib.wos_siren_fit(C.byref(hnet), x.ctypes.data, n, target.ctypes.data, scale.ctypes.data, hl.ctypes.data, None,
                           None, 0, 0, gpu, None)
    assert rc == 0, lib.wos_last_error()
    assert np.array_equal(bits(hl[0]), bits(want[0])) and all(np.all(a == 3.0) for a in ow + ob), "loss only, host pointers"
    # numpy in, numpy out through the python layer
    l_np, gw_np, gb_np = siren.fit(net, x, target, scale)
    assert isinstance(l_np, np.float32) and same_bits((l_np, (gw_np, gb_np)), want)
    assert np.array_equal(bits(siren.fit(net, x, target, scale, grads=False)), bits(want[0]))
    # refusals, on the device
    dnet, keep_d = _c_net(p, p.weights, p.biases, lambda t: t.data_ptr())
    dw, db = [torch.full_like(t, 7.0) for t in p.weights], [torch.full_like(t, 7.0) for t in p.biases]
    dl = torch.full((1,), 7.0, device="cuda")
    qw = (C.c_void_p * nl)(*[t.data_ptr() for t in dw])
    qb = (C.c_void_p * nl)(*[t.data_ptr() for t in db])
    flags = _lib.WOS_PTRS_DEVICE
    torch.cuda.synchronize()

    def call(net_=dnet, n_=n, t_=td.data_ptr(), l_=dl.data_ptr(), w_=qw, b_=qb, ws=0):
        return lib.wos_siren_fit(C.byref(net_), xd.data_ptr(), n_, t_, sd.data_ptr(), l_, w_, b_, ws, flags, gpu, None)
    assert call(n_=0) == -1 and b"n must be positive" in lib.wos_last_error()
    assert call(n_=-1) == -1 and b"n must be positive" in lib.wos_last_error()
    assert call(t_=None) == -1 and b"null target" in lib.wos_last_error()
    assert call(l_=None) == -1 and b"null loss" in lib.wos_last_error()
    assert call(w_=None) == -1 and b"exactly one of grad_weights and grad_biases" in lib.wos_last_error()
    assert call(b_=None) == -1 and b"exactly one of grad_weights and grad_biases" in lib.wos_last_error()
    hole = (C.c_void_p * nl)(qw[0], None, qw[2])
    assert call(w_=hole) == -1 and b"grad_weights" in lib.wos_last_error() and b"layer 1" in lib.wos_last_error()
    assert call(ws=100) == _lib.WOS_E_CAPACITY and b"workspace_bytes" in lib.wos_last_error()
    for field, value in (("hidden", 100), ("d_in", 4), ("d_out", 0), ("n_hidden_layers", 9), ("omega", float("inf"))):
        bad, keep_b = _c_net(p, p.weights, p.biases, lambda t: t.data_ptr())
        setattr(bad, field, value)
        assert call(net_=bad) == -1 and field.encode() in lib.wos_last_error(), field
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in dw + db + [dl]), "a refused call wrote nothing"


# ---- 6. siren.fit_loss ---------------------------------------------------------------------------------------
def _params(net):
    lin = [m for m in net.net if isinstance(m, torch.nn.Linear)]
    return [m.weight for m in lin] + [m.bias for m in lin]


def test_fit_loss_is_fit_forward_and_scaled_gradients_backward(gpu):
    net = _cuda_net(2, 128, 2).requires_grad_(True)
    params = _params(net)
    n = 130
    x = _dev(sm.points(2, n))
    target, scale = [_dev(a) for a in fm.problem(n, 2, True)]
    want_loss, gw, gb = siren.fit(net, x, target, scale)
    before = dict(siren.fit_calls)
    loss = siren.fit_loss(net, x, target, scale)
    assert loss.requires_grad and loss.shape == () and np.array_equal(bits(loss), bits(want_loss))
    (3.0 * loss).backward(retain_graph=True)  # update_network's call
    for t, g in zip(params, gw + gb):
        assert np.array_equal(bits(t.grad), bits(3.0 * g))
    (3.0 * loss).backward()  # the retained graph: .grad accumulates, nothing is recomputed
    for t, g in zip(params, gw + gb):
        assert np.array_equal(bits(t.grad), bits(3.0 * g + 3.0 * g))
    assert siren.fit_calls["grads"] == before["grads"] + 1 and siren.fit_calls["loss_only"] == before.get("loss_only", 0)
    # a second-order request
    loss = siren.fit_loss(net, x, target, scale)
    first = torch.autograd.grad(loss, params, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiated twice|does not require grad"):
        torch.autograd.grad(sum((t * t).sum() for t in first), params)
    # under no_grad, and with no parameter that requires grad, only the loss-only path runs
    before = dict(siren.fit_calls)
    with torch.no_grad():
        quiet = siren.fit_loss(net, x, target, scale)
    frozen = siren.fit_loss(copy.deepcopy(net).requires_grad_(False), x, target, scale)
    for t in (quiet, frozen):
        assert not t.requires_grad and t.grad_fn is None and np.array_equal(bits(t), bits(want_loss))
    assert siren.fit_calls["loss_only"] == before.get("loss_only", 0) + 2 and siren.fit_calls["grads"] == before["grads"]


# ---- 7. end to end -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _karman():
    cfg = workloads.karman_config(n_walks=16, n_points=200)
    scene_cfg = dict(workloads.SCENE_BASE, boundary=workloads.KARMAN_OBJ)
    samples = torch.from_numpy(cfg["points"]).cuda()
    proj = pj.PressureProjector(scene_cfg, cfg["solver"], cfg["output"], samples)
    size = workloads.scene_size(workloads.KARMAN_OBJ)
    return proj, samples, [float(v) for v in size]


def _box(samples):
    return [samples[:, 0].min().item(), samples[:, 0].max().item(), samples[:, 1].min().item(), samples[:, 1].max().item()]


def _end_to_end(net, net_prev, x, wrap, target32, run_fit, run_torch, what):
    """The fit route against a float64 evaluation of the same formula at the same points x:
    target64 = the float64 twin of target32 (given as a function of the float64 nets)."""
    params = _params(net)

    def grads_of(run):
        for t in params:
            t.grad = None
        loss = run()
        loss.backward()
        return float(loss.detach()), [t.grad.detach().cpu().numpy().copy() for t in params]
    loss_c, g_c = grads_of(run_fit)
    loss_a, g_a = grads_of(run_torch)
    net64, x64 = vm.net64(net).requires_grad_(True), x.detach().cpu().double()
    t64 = target32["float64"](x64)
    u64 = net64(x64)
    w64 = wrap(x64, u64) if wrap else u64
    L64 = torch.mean((w64 - t64) ** 2)
    ref = [g.numpy() for g in torch.autograd.grad(L64, _params(net64))]
    L64 = float(L64.detach())
    # the forward's measured error, propagated: the wrapped value's and the target's, against float64
    with torch.no_grad():
        u32 = siren.eval(net, x)
        w32 = wrap(x, u32) if wrap else u32
        du = float((w32.cpu().double() - w64.detach()).abs().max())
        dt = float((target32["float32"]().cpu().double() - t64).abs().max())
    bound = fm.loss_bound(t64.numel(), L64) + 2.0 * np.sqrt(L64) * (du + dt)
    print(f"{what}: loss {loss_c:.9e} torch f32 {loss_a:.9e} float64 {L64:.9e} error {abs(loss_c - L64):.3e} "
          f"bound {bound:.3e} (du {du:.3e} dt {dt:.3e})")
    assert abs(loss_c - L64) <= bound
    nl = len(params) // 2
    s64 = torch.ones_like(u64) if wrap is None else siren.diagonal_wrap(wrap, x64, 2)[0]
    ub = (2.0 * s64 * (w64.detach() - t64) / t64.numel()).numpy()
    vm.assert_grads_as_accurate((g_c[:nl], g_c[nl:]), (g_a[:nl], g_a[nl:]), (ref[:nl], ref[nl:]), ub, what)
    return g_c


@pytest.mark.parametrize("wrapped", [False, True], ids=["plain", "karman_wrap"])
def test_projection_fit_loss_end_to_end(gpu, wrapped):
    proj, samples, size = _karman()
    net, net_prev = _cuda_net(2, 128, 2).requires_grad_(True), copy.deepcopy(sm.make_net(2, 128, 2, seed=1)).cuda()
    wrap = sm.karman_wrap(_box(samples), eps=0.125) if wrapped else None
    grad_p = torch.from_numpy(np.random.default_rng(11).standard_normal((200, 2)).astype(np.float32) * 0.1).cuda()
    n_samples = 256
    gen = lambda: torch.Generator(device="cuda").manual_seed(77)  # noqa: E731
    idx = torch.randint(0, 199, (n_samples,), device="cuda", generator=gen())
    x = samples[idx]
    prev64 = vm.net64(net_prev)

    def target64(x64):
        with torch.no_grad():
            u = prev64(x64)
            return (wrap(x64, u) if wrap else u) - grad_p[idx].cpu().double()

    def target32():
        u = siren.eval(net_prev, x)
        return (wrap(x, u) if wrap else u) - grad_p[idx]
    velocity = (lambda q: wrap(q, net(q))) if wrapped else net
    velocity_prev = (lambda q: wrap(q, net_prev(q))) if wrapped else net_prev
    g = _end_to_end(net, net_prev, x, wrap, {"float64": target64, "float32": target32},
                    lambda: proj.projection_fit_loss(net, net_prev, grad_p, n_samples, wrap=wrap, generator=gen()),
                    lambda: proj.projection_loss(velocity, velocity_prev, grad_p, n_samples, generator=gen()),
                    f"projection ({'wrap' if wrapped else 'plain'})")
    assert all(np.any(a) for a in g)
    g1, g2 = gen(), gen()
    proj.projection_fit_loss(net, net_prev, grad_p, n_samples, wrap=wrap, generator=g1)
    proj.projection_loss(velocity, velocity_prev, grad_p, n_samples, generator=g2)
    assert torch.equal(g1.get_state(), g2.get_state())


@pytest.mark.parametrize("tilde", [False, True], ids=["prev", "two_prev_minus_tilde"])
@pytest.mark.parametrize("wrapped", [False, True], ids=["plain", "karman_wrap"])
def test_advection_fit_loss_end_to_end(gpu, wrapped, tilde):
    proj, samples, size = _karman()
    net, net_prev = _cuda_net(2, 128, 2).requires_grad_(True), copy.deepcopy(sm.make_net(2, 128, 2, seed=1)).cuda()
    net_tilde = copy.deepcopy(sm.make_net(2, 128, 2, seed=2)).cuda() if tilde else None
    wrap = sm.karman_wrap(size, eps=0.125) if wrapped else None
    x, dt = samples, 0.05
    query = lambda n_, q: wrap(q, n_(q)) if wrap else n_(q)  # noqa: E731

    def formula(nets, q):  # _advect_velocity's target, in q's dtype
        with torch.no_grad():
            back = q - query(nets[0], q) * dt
            back = torch.stack([back[..., 0].clamp(min=size[0], max=size[1]), back[..., 1].clamp(min=size[2], max=size[3])], -1)
            t = query(nets[0], back)
            return 2 * t - query(nets[1], back) if tilde else t
    nets64 = (vm.net64(net_prev), vm.net64(net_tilde) if tilde else None)
    g = _end_to_end(net, net_prev, x, wrap,
                    {"float64": lambda x64: formula(nets64, x64),
                     "float32": lambda: formula((lambda q: siren.eval(net_prev, q), lambda q: siren.eval(net_tilde, q)), x)},
                    lambda: pj.advection_fit_loss(net, net_prev, x, dt, size, network_tilde=net_tilde, wrap=wrap),
                    lambda: torch.mean((query(net, x) - formula((net_prev, net_tilde), x)) ** 2),
                    f"advection ({'wrap' if wrapped else 'plain'}, {'tilde' if tilde else 'prev'})")
    assert all(np.any(a) for a in g)
