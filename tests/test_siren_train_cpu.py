"""Fused Adam step and the device-resident fit loop without a GPU (include/wos.h "Fused Adam step",
"Device-resident fit loop"): both entry points are declared, exported and bound within ABI 10; each
names what it refuses before any device work and writes nothing; the float64 model of the step
equals torch.optim.Adam(foreach=False) in float64, the float32 model torch's float32 CPU Adam within
2 B per element (siren_adam_model.bound); PressureProjector.fit_projection draws what
projection_fit_loss draws and builds the pool's target and scale as it does."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import siren_adam_model as am
import siren_model as sm
import wos_amd
from wos_amd import _lib, siren
from wos_amd import projection as pj

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "wos.h")

ADAM_ARGS = ["n_tensors", "counts", "params", "grads", "exp_avg", "exp_avg_sq", "step", "opt", "grad_norm", "flags",
             "device", "stream"]
RUN_ARGS = ["net", "pool_pts", "pool_target", "pool_scale", "n_pool", "idx", "n_iters", "batch", "exp_avg", "exp_avg_sq",
            "step0", "opt", "stop_loss", "check_every", "losses", "status", "workspace_bytes", "flags", "device", "stream"]


# ---- ABI ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,want", [("wos_adam_step", ADAM_ARGS), ("wos_siren_fit_run", RUN_ARGS)])
def test_entry_points_declared_exported_and_bound(name, want):
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S)
    assert m, f"{name} is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [re.search(r"(\w+)$", a).group(1) for a in args] == want
    L = wos_amd.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (wos_[a-z0-9_]+)$", out, flags=re.M))
    assert name in exported and name in _lib.EXPORTS and hasattr(L, name)
    assert len(getattr(L, name).argtypes) == len(want)
    assert L.wos_abi_version() == _lib.ABI_VERSION == 10
    assert re.search(r"#define WOS_ABI_VERSION 10\b", raw)
    assert re.search(r"typedef struct wos_adam_params\s*\{\s*double lr, beta1, beta2, eps;\s*double max_grad_norm;", txt)
    assert [f[0] for f in _lib.AdamParams._fields_] == ["lr", "beta1", "beta2", "eps", "max_grad_norm"]
    assert all(f[1] is C.c_double for f in _lib.AdamParams._fields_)
    if name == "wos_siren_fit_run":
        assert "WRITES THROUGH net->weights[l] AND net->biases[l]" in raw, "the header says that the net is written"


# ---- refusals that need no device --------------------------------------------------------------------
def _adam_call(**over):
    """A complete host-pointer call of wos_adam_step as keyword arguments a test can break one at a time."""
    shapes = [(3, 2), (5,)]
    p, g, m, v = am.problem(shapes, seed=1)
    k = {"p": p, "g": g, "m": m, "v": v, "norm": np.full(1, 7.0, np.float32)}
    k["before"] = [a.copy() for a in p + [m, v]]
    a = dict(n=2, counts=(C.c_int64 * 2)(6, 5), params=(C.c_void_p * 2)(*[x.ctypes.data for x in p]),
             grads=(C.c_void_p * 2)(*[x.ctypes.data for x in g]), m=m.ctypes.data, v=v.ctypes.data, step=1,
             opt=_lib.AdamParams(1e-4, 0.9, 0.999, 1e-8, 0.5), norm=k["norm"].ctypes.data, flags=0)
    a.update(over)
    L = _lib.load()
    rc = L.wos_adam_step(a["n"], a["counts"], a["params"], a["grads"], a["m"], a["v"], a["step"],
                         None if a["opt"] is None else C.byref(a["opt"]), a["norm"], a["flags"], 0, None)
    unchanged = all(np.array_equal(x, y) for x, y in zip(k["before"], p + [m, v])) and k["norm"][0] == 7.0
    return rc, L.wos_last_error(), unchanged


def _opt(**over):
    f = dict(lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=-1.0)
    f.update(over)
    return _lib.AdamParams(f["lr"], f["beta1"], f["beta2"], f["eps"], f["max_grad_norm"])


BAD_OPTS = [({"lr": float("nan")}, b"lr"), ({"lr": float("inf")}, b"lr"), ({"beta1": 1.0}, b"beta1"), ({"beta1": -0.1}, b"beta1"),
            ({"beta2": 1.0}, b"beta2"), ({"beta2": -1e-3}, b"beta2"), ({"beta2": float("nan")}, b"beta2"),
            ({"eps": -1e-8}, b"eps"), ({"eps": float("nan")}, b"eps"), ({"max_grad_norm": float("inf")}, b"max_grad_norm"),
            ({"max_grad_norm": float("nan")}, b"max_grad_norm")]


def test_adam_step_refusals_name_the_field_before_any_device_work():
    nul = C.c_void_p(None)
    x = np.zeros(8, np.float32).ctypes.data
    cases = [({"n": 0}, b"n_tensors"), ({"n": 21}, b"n_tensors"), ({"n": -1}, b"n_tensors"),
             ({"counts": None}, b"counts"), ({"params": None}, b"params"), ({"grads": None}, b"grads"),
             ({"m": None}, b"exp_avg"), ({"v": None}, b"exp_avg_sq"), ({"opt": None}, b"opt"),
             ({"params": (C.c_void_p * 2)(x, nul)}, b"params pointer of tensor 1"),
             ({"grads": (C.c_void_p * 2)(nul, x)}, b"grads pointer of tensor 0"),
             ({"counts": (C.c_int64 * 2)(6, 0)}, b"counts[1]"), ({"counts": (C.c_int64 * 2)(-6, 5)}, b"counts[0]"),
             ({"step": 0}, b"step"), ({"step": -4}, b"step")]
    cases += [({"opt": _opt(**f)}, word) for f, word in BAD_OPTS]
    for flags in (0, _lib.WOS_PTRS_DEVICE, _lib.WOS_PTRS_DEVICE | _lib.WOS_ASYNC):
        for over, word in cases:
            rc, msg, unchanged = _adam_call(flags=flags, **over)
            assert rc == -1 and msg.startswith(b"wos_adam_step") and word in msg, (over, msg)
            assert unchanged, "a refused call wrote nothing"


def _run_call(**over):
    """wos_siren_fit_run on host memory passed as device pointers: every refusal comes before any device work."""
    net = sm.make_net(2, 64, 1)
    p = siren.pack(net)
    ws, bs = [t.numpy() for t in p.weights], [t.numpy() for t in p.biases]
    total = sum(a.size for a in ws + bs)
    k = {"x": sm.points(2, 9), "t": np.zeros((9, 2), np.float32), "idx": np.zeros((2, 4), np.int64),
         "m": np.zeros(total, np.float32), "v": np.zeros(total, np.float32), "losses": np.full(2, 7.0, np.float32),
         "status": np.full(2, 7, np.int64), "ws": ws, "bs": bs}
    w = (C.c_void_p * 3)(*[a.ctypes.data for a in ws])
    b = (C.c_void_p * 3)(*[a.ctypes.data for a in bs])
    net_c = _lib.SirenNet(p.d_in, p.d_out, p.hidden, p.n_hidden_layers, p.omega, w, b)
    for field, value in over.pop("net_fields", {}).items():
        setattr(net_c, field, value)
    a = dict(pts=k["x"].ctypes.data, target=k["t"].ctypes.data, scale=None, n_pool=9, idx=k["idx"].ctypes.data, n_iters=2,
             batch=4, m=k["m"].ctypes.data, v=k["v"].ctypes.data, step0=0, opt=_opt(), stop_loss=-1.0, check_every=0,
             losses=k["losses"].ctypes.data, status=k["status"].ctypes.data, ws=0, flags=_lib.WOS_PTRS_DEVICE)
    a.update(over)
    before = [x.copy() for x in ws + bs]
    L = _lib.load()
    rc = L.wos_siren_fit_run(C.byref(net_c), a["pts"], a["target"], a["scale"], a["n_pool"], a["idx"], a["n_iters"],
                             a["batch"], a["m"], a["v"], a["step0"], None if a["opt"] is None else C.byref(a["opt"]),
                             a["stop_loss"], a["check_every"], a["losses"], a["status"], a["ws"], a["flags"], 0, None)
    unchanged = (np.all(k["losses"] == 7.0) and np.all(k["status"] == 7) and not k["m"].any() and not k["v"].any()
                 and all(np.array_equal(x, y) for x, y in zip(before, ws + bs)))
    return rc, L.wos_last_error(), unchanged


def test_fit_run_refusals_name_the_field_before_any_device_work():
    cases = [({"flags": 0}, b"WOS_PTRS_DEVICE"), ({"flags": _lib.WOS_ASYNC}, b"WOS_PTRS_DEVICE"),
             ({"flags": _lib.WOS_PTRS_DEVICE | _lib.WOS_ASYNC, "check_every": 1}, b"check_every"),
             ({"check_every": -1}, b"check_every"),
             ({"n_iters": 0}, b"n_iters"), ({"n_iters": -2}, b"n_iters"), ({"batch": 0}, b"batch"), ({"batch": -1}, b"batch"),
             ({"n_pool": 0}, b"n_pool"), ({"n_pool": -9}, b"n_pool"), ({"step0": -1}, b"step0"),
             ({"idx": None}, b"idx"), ({"losses": None}, b"losses"), ({"status": None}, b"status"),
             ({"pts": None}, b"pool_pts"), ({"target": None}, b"pool_target"), ({"m": None}, b"exp_avg"),
             ({"v": None}, b"exp_avg_sq"), ({"stop_loss": float("nan")}, b"stop_loss"), ({"opt": None}, b"opt"),
             ({"net_fields": {"d_in": 4}}, b"d_in"), ({"net_fields": {"d_out": 0}}, b"d_out"),
             ({"net_fields": {"hidden": 100}}, b"hidden"), ({"net_fields": {"n_hidden_layers": 9}}, b"n_hidden_layers"),
             ({"net_fields": {"omega": float("inf")}}, b"omega")]
    cases += [({"opt": _opt(**f)}, word) for f, word in BAD_OPTS]
    for over, word in cases:
        rc, msg, unchanged = _run_call(**over)
        assert rc == -1 and msg.startswith(b"wos_siren_fit_run") and word in msg, (over, msg)
        assert unchanged, "a refused call wrote nothing"
    tile = (2 * 1 + 1) * 64 * 4 * 32
    rc, msg, unchanged = _run_call(ws=tile - 1)
    assert rc == _lib.WOS_E_CAPACITY and b"workspace_bytes" in msg and b"cannot hold one tile" in msg and unchanged


def test_python_layer_names_what_it_refuses():
    net = sm.make_net(2, 32, 1)
    state = siren.AdamState(net)
    assert state.step == 0 and state.exp_avg.shape == (2 * 32 + 32 * 32 + 2 * 32 + 32 + 32 + 2,) and not state.exp_avg.any()
    assert state.exp_avg.dtype == torch.float32 and state.exp_avg_sq.shape == state.exp_avg.shape
    assert state.params().max_grad_norm <= 0 and siren.AdamState(net, max_grad_norm=0.5).params().max_grad_norm == 0.5
    o = siren.AdamState(net, lr=3e-4, betas=(0.8, 0.99), eps=1e-7).params()
    assert (o.lr, o.beta1, o.beta2, o.eps) == (3e-4, 0.8, 0.99, 1e-7)
    p = siren.pack(net)
    gw, gb = [np.zeros(t.shape, np.float32) for t in p.weights], [np.zeros(t.shape, np.float32) for t in p.biases]
    with pytest.raises(ValueError, match="grads must be"):
        siren.adam_step(net, (gw[:2], gb), state)
    with pytest.raises(ValueError, match="gradient 1 has shape"):
        siren.adam_step(net, ([gw[0], gw[1][:3], gw[2]], gb), state)
    with pytest.raises(ValueError, match="another shape"):
        siren.adam_step(net, (gw, gb), siren.AdamState(sm.make_net(2, 64, 1)))
    x = torch.from_numpy(sm.points(2, 5))
    with pytest.raises(ValueError, match="pool_x must be a CUDA tensor"):
        siren.fit_run(net, state, x, x, None, torch.zeros((1, 2), dtype=torch.int64))
    assert state.step == 0


# ---- the model against torch -------------------------------------------------------------------------
SHAPES = [(30, 20), (17,), (383,)]  # 1000 elements
STEPS = [1, 2, 7, 1000]
CLIPS = [None, 0.1, 1e3]  # off, active, inactive


def _torch_step(dtype, params, grads, m, v, step, clip, **kw):
    """torch.optim.Adam(foreach=False) on the CPU with the state (m, v, step - 1) injected through opt.state."""
    ps = [torch.from_numpy(np.asarray(a, dtype).copy()).requires_grad_(True) for a in params]
    opt = torch.optim.Adam(ps, foreach=False, **kw)
    at = 0
    for t, g in zip(ps, grads):
        n = t.numel()
        t.grad = torch.from_numpy(np.asarray(g, dtype).copy())
        opt.state[t] = {"step": torch.tensor(float(step - 1)),
                        "exp_avg": torch.from_numpy(np.asarray(m[at:at + n], dtype).reshape(t.shape).copy()),
                        "exp_avg_sq": torch.from_numpy(np.asarray(v[at:at + n], dtype).reshape(t.shape).copy())}
        at += n
    norm = None
    if clip is not None:
        norm = float(torch.nn.utils.clip_grad_norm_(ps, clip))
    opt.step()
    return ([t.detach().numpy() for t in ps], np.concatenate([opt.state[t]["exp_avg"].numpy().reshape(-1) for t in ps]),
            np.concatenate([opt.state[t]["exp_avg_sq"].numpy().reshape(-1) for t in ps]), norm)


def _flat(arrays):
    return np.concatenate([np.asarray(a).reshape(-1) for a in arrays])


@pytest.mark.parametrize("clip", CLIPS, ids=["noclip", "clip_active", "clip_inactive"])
@pytest.mark.parametrize("step", STEPS)
def test_float64_model_equals_torch_float64(step, clip):
    kw = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8)
    params, grads, m, v = am.problem(SHAPES, seed=step, state=step > 1)
    got = am.step64(params, grads, m, v, step, max_grad_norm=clip, **kw)
    want = _torch_step(np.float64, params, grads, m, v, step, clip, **kw)
    assert got[4]["clip_active"] == (clip == 0.1)
    for a, b in zip(got[0], want[0]):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    for a, b in ((got[1], want[1]), (got[2], want[2])):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    if clip is not None:
        assert abs(got[3] - want[3]) <= 1e-12 * want[3]


@pytest.mark.parametrize("clip", CLIPS, ids=["noclip", "clip_active", "clip_inactive"])
@pytest.mark.parametrize("step", STEPS)
def test_float32_model_against_torch_float32_within_two_bounds(step, clip):
    kw = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8)
    params, grads, m, v = am.problem(SHAPES, seed=step, state=step > 1)
    assert np.any(_flat(grads) == 0) and (step == 1 or np.any((m == 0) & (v == 0) & (_flat(grads) == 0)))
    p32, m32, v32, norm = am.step32(params, grads, m, v, step, max_grad_norm=clip, **kw)
    assert all(a.dtype == np.float32 for a in p32 + [m32, v32])
    ref = am.step64(params, grads, m, v, step, max_grad_norm=clip, **kw)
    B = am.bound(ref[4])
    want = _torch_step(np.float32, params, grads, m, v, step, clip, **kw)
    diff = np.abs(_flat(p32).astype(np.float64) - _flat(want[0]).astype(np.float64))
    e_model = np.abs(_flat(p32).astype(np.float64) - ref[4]["p"])
    e_torch = np.abs(_flat(want[0]).astype(np.float64) - ref[4]["p"])
    same = np.mean(_flat(p32) == _flat(want[0]))
    print(f"step {step} clip {clip}: bit-equal {same:.4f}; model / B {np.max(e_model / B):.3f}, torch / B {np.max(e_torch / B):.3f}, "
          f"difference / 2B {np.max(diff / (2 * B)):.3f}")
    assert np.all(B > 0) and np.all(diff <= 2 * B)
    if clip is not None:
        assert abs(float(norm) - ref[3]) <= (len(diff) / 2 + 4) * am.U * ref[3]


def _non_finite_problem(bad):
    """am.problem(SHAPES, step 2) with one gradient element, in the middle tensor, set to `bad`.
    Returns (params, grads, m, v, the element's flat index)."""
    params, grads, m, v = am.problem(SHAPES, seed=2, state=True)
    grads[1][5] = bad
    return params, grads, m, v, params[0].size + 5


@pytest.mark.parametrize("clip", [None, 0.1], ids=["noclip", "clip"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_float32_model_follows_torch_float32_on_a_non_finite_gradient(bad, clip):
    """clip_grad_norm_ clamps its coefficient with torch.clamp(max=1), which keeps a NaN: with a NaN
    gradient and clipping on, every parameter and both moments go NaN.  An infinite gradient gives a
    norm of inf and a coefficient of 0: NaN at that element, a zero gradient everywhere else.
    Without clipping only the element itself is touched."""
    kw = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8)
    params, grads, m, v, at = _non_finite_problem(bad)
    with np.errstate(invalid="ignore", over="ignore"):
        p32, m32, v32, norm = am.step32(params, grads, m, v, 2, max_grad_norm=clip, **kw)
        ref = am.step64(params, grads, m, v, 2, max_grad_norm=clip, **kw)
        B = am.bound(ref[4])
    want = _torch_step(np.float32, params, grads, m, v, 2, clip, **kw)
    total = m.size
    for name, a, b in (("parameters", _flat(p32), _flat(want[0])), ("exp_avg", m32, want[1]), ("exp_avg_sq", v32, want[2])):
        assert np.array_equal(np.isnan(a), np.isnan(b)), f"{name}: NaN at {np.flatnonzero(np.isnan(a) != np.isnan(b))[:8]}"
        assert np.array_equal(np.isinf(a), np.isinf(b)) and np.array_equal(a[np.isinf(a)], b[np.isinf(b)]), name
    ok = np.isfinite(_flat(p32))
    diff = np.abs(_flat(p32).astype(np.float64) - _flat(want[0]).astype(np.float64))
    assert np.all(B[ok] > 0) and np.all(diff[ok] <= 2 * B[ok])
    # what reading torch says must happen
    nan_p = np.isnan(_flat(p32))
    if clip is not None and np.isnan(bad):
        assert nan_p.all() and np.isnan(m32).all() and np.isnan(v32).all() and np.isnan(norm)
    else:
        only = np.zeros(total, bool)
        only[at] = True
        assert np.array_equal(nan_p, only) and np.array_equal(~np.isfinite(m32), only) and np.array_equal(~np.isfinite(v32), only)
        if clip is not None:  # inf: the coefficient is 0, the step is that of a zero gradient
            assert np.isinf(norm) and am.clip32(norm, clip) == 0
            with np.errstate(invalid="ignore"):
                zero = am.step32(params, [np.zeros_like(g) for g in grads], m, v, 2, **kw)
            assert np.array_equal(_flat(zero[0])[~only], _flat(p32)[~only])


def test_norm32_is_the_chain_then_pairwise_order():
    """Against a literal scalar restatement of the kernel's loops, at a size below, at and above 256."""
    rng = np.random.default_rng(3)
    for n in (1, 129, 256, 257, 1000):
        g = rng.standard_normal(n).astype(np.float32)
        acc = [np.float32(0)] * 256
        for t in range(256):
            for e in range(t, n, 256):
                acc[t] = np.float32(acc[t] + np.float32(g[e] * g[e]))
        w = 128
        while w >= 1:
            for t in range(w):
                acc[t] = np.float32(acc[t] + acc[t + w])
            w >>= 1
        assert am.norm32(g).view(np.uint32) == np.sqrt(acc[0]).view(np.uint32)


# ---- fit_projection draws what projection_fit_loss draws ---------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
def test_fit_projection_draws_the_samples_of_projection_fit_loss(monkeypatch, dim):
    n, n_samples, K = 50, 16, 5
    proj = pj.PressureProjector.__new__(pj.PressureProjector)
    proj.dim, proj.device = dim, torch.device("cpu")
    proj.samples = torch.from_numpy(sm.points(dim, n, seed=4))
    grad_p = torch.from_numpy(np.random.default_rng(2).standard_normal((n, dim)).astype(np.float32))
    net = sm.make_net(dim, 32, 1)
    calls = []

    def fake_eval(net_, x, **kw):
        return 0.5 * x

    def fake_fit_loss(module, x, target, scale=None):
        return torch.zeros(())

    def fake_fit_run(net_, state, pool_x, pool_target, pool_scale, idx, *, stop_loss=None, **kw):
        calls.append({"x": pool_x, "target": pool_target.clone(), "scale": pool_scale, "idx": idx.clone(), "stop": stop_loss,
                      "step": state.step})
        state.step += idx.shape[0]
        return torch.arange(idx.shape[0], dtype=torch.float32), torch.tensor([idx.shape[0], 0])
    monkeypatch.setattr(siren, "eval", fake_eval)
    monkeypatch.setattr(siren, "fit_loss", fake_fit_loss)
    monkeypatch.setattr(siren, "fit_run", fake_fit_run)
    g1 = torch.Generator().manual_seed(123)
    for _ in range(K):
        proj.projection_fit_loss(net, object(), grad_p, n_samples, generator=g1)
    g0 = torch.Generator().manual_seed(123)
    hi = n - 1 if dim == 2 else n
    rows = torch.stack([torch.randint(0, hi, (n_samples,), generator=g0) for _ in range(K)])
    assert torch.equal(g0.get_state(), g1.get_state())
    for per_call in (2, 5, 8, 1):  # not dividing, equal to, larger than n_iters, and one at a time
        calls.clear()
        g2 = torch.Generator().manual_seed(123)
        losses, state = proj.fit_projection(net, object(), grad_p, n_samples, K, generator=g2, iters_per_call=per_call)
        assert torch.equal(g1.get_state(), g2.get_state()), "the same generator consumption"
        assert len(calls) == -(-K // per_call) and [c["step"] for c in calls] == list(range(0, K, per_call))
        got = torch.cat([c["idx"] for c in calls])
        assert got.dtype == torch.int64 and got.is_contiguous() and torch.equal(got, rows), "the index rows are those draws"
        assert losses.shape == (K,) and state.step == K and isinstance(state, siren.AdamState)
        for c in calls:
            assert c["x"] is proj.samples and c["scale"] is None and c["stop"] is None
            assert torch.equal(c["target"], 0.5 * proj.samples - grad_p)
    # with a wrap: the pool's scale and target are diagonal_wrap's over the whole pool
    wrap = sm.karman_wrap([0.0, 2.2, 0.0, 1.0], eps=0.125)
    calls.clear()
    given = siren.AdamState(net, lr=3e-4)
    g3 = torch.Generator().manual_seed(123)
    _, state = proj.fit_projection(net, object(), grad_p, n_samples, K, state=given, wrap=wrap, generator=g3, early_stop=True,
                                   iters_per_call=4)
    assert state is given and torch.equal(g1.get_state(), g3.get_state())
    scale, offset = siren.diagonal_wrap(wrap, proj.samples, dim)
    for c in calls:
        assert torch.equal(c["scale"], scale) and c["stop"] == 1.1e-10
        assert torch.equal(c["target"], wrap(proj.samples, 0.5 * proj.samples) - grad_p - offset)
    # early stop inside the first block: no further block is drawn, the rest is NaN
    def stopping_fit_run(net_, state, pool_x, pool_target, pool_scale, idx, *, stop_loss=None, **kw):
        calls.append(idx.shape[0])
        out = torch.full((idx.shape[0],), float("nan"))
        out[0] = 0.0
        state.step += 1
        return out, torch.tensor([1, 0])
    monkeypatch.setattr(siren, "fit_run", stopping_fit_run)
    calls.clear()
    losses, state = proj.fit_projection(net, object(), grad_p, n_samples, K, early_stop=1e-3, iters_per_call=2)
    assert calls == [2] and state.step == 1 and losses.shape == (K,) and losses[0] == 0 and bool(torch.isnan(losses[1:]).all())


@pytest.mark.parametrize("per_call,stop_at", [(2, 1), (2, 3), (1, 0), (1, 2), (4, 3), (5, 4)])
def test_fit_projection_sees_a_stop_on_the_last_iteration_of_a_block(monkeypatch, per_call, stop_at):
    """The stopping iteration is applied and counted, so a stop at a block's last iteration returns
    status[0] == the block's length: fit_projection must still draw no further block, and the tail
    of the losses is NaN.  The fake fit_run behaves as wos_siren_fit_run does: losses of 1 - i / 10
    until the first one at or below stop_loss, NaN after it, status[0] the iterations applied."""
    n, n_samples, K, stop = 50, 8, 5, np.float32(1.0 - stop_at / 10.0)
    assert (stop_at + 1) % per_call == 0 or stop_at == K - 1, "the case: the stop is a block's last iteration"
    proj = pj.PressureProjector.__new__(pj.PressureProjector)
    proj.dim, proj.device = 2, torch.device("cpu")
    proj.samples = torch.from_numpy(sm.points(2, n, seed=4))
    grad_p = torch.zeros((n, 2))
    net = sm.make_net(2, 32, 1)
    blocks = []

    def fake_fit_run(net_, state, pool_x, pool_target, pool_scale, idx, *, stop_loss=None, **kw):
        k = idx.shape[0]
        blocks.append(k)
        out = torch.full((k,), float("nan"))
        applied = 0
        for j in range(k):
            out[j] = float(np.float32(1.0 - (state.step + j) / 10.0))
            applied = j + 1
            if np.float32(out[j]) <= np.float32(stop_loss):
                break
        state.step += applied
        return out, torch.tensor([applied, 0])
    monkeypatch.setattr(siren, "eval", lambda net_, x, **kw: torch.zeros_like(x))
    monkeypatch.setattr(siren, "fit_run", fake_fit_run)
    gen = torch.Generator().manual_seed(1)
    losses, state = proj.fit_projection(net, object(), grad_p, n_samples, K, generator=gen, early_stop=float(stop),
                                        iters_per_call=per_call)
    assert blocks == [min(per_call, K - f) for f in range(0, stop_at + 1, per_call)], "no further block is drawn"
    assert state.step == stop_at + 1 and losses.shape == (K,)
    assert bool(torch.isfinite(losses[:stop_at + 1]).all()) and bool(torch.isnan(losses[stop_at + 1:]).all())
    want = torch.Generator().manual_seed(1)
    for _ in range(sum(blocks)):
        torch.randint(0, n - 1, (n_samples,), generator=want)
    assert torch.equal(gen.get_state(), want.get_state()), "only the blocks that ran consumed the generator"
