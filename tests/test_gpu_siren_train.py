"""Fused Adam step and the device-resident fit loop on the GPU (wos_adam_step, wos_siren_fit_run,
csrc/wos_siren_train.hip): the step bit for bit against the float32 model (siren_adam_model.step32)
and within 2 B of torch.optim.Adam on the GPU; host against device pointers, determinism, a side
stream; siren.fit_run bit for bit against the loop of gather, siren.fit and siren.adam_step made
separately -- chunked, continued, stopped early, with a clamped index -- and
PressureProjector.fit_projection end to end on the karman scene."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import siren_adam_model as am
import siren_fit_model as fm
import siren_model as sm
from wos_amd import _lib, siren, workloads
from wos_amd import projection as pj

pytestmark = pytest.mark.gpu

KW = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8)


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def _cuda_net(d, H, L, d_out=None, seed=0):
    return copy.deepcopy(sm.make_net(d, H, L, d_out, seed=seed)).cuda()


def _tensors(net):
    p = siren.pack(net)
    return p.weights + p.biases


# ---- 1. the Adam step against the float32 model, bit for bit -----------------------------------------------
def _adam_c(params, grads, m, v, step, clip, device, stream=None, want_norm=True, kw=KW):
    """wos_adam_step through the C ABI on copies of the numpy inputs, with host pointers or device
    pointers (blocking; on `stream` asynchronously, then synchronised) and the hyper-parameters kw.
    Returns (params, m, v, norm)."""
    lib = _lib.load()
    n = len(params)
    counts = (C.c_int64 * n)(*[a.size for a in params])
    opt = _lib.AdamParams(kw["lr"], kw["betas"][0], kw["betas"][1], kw["eps"], -1.0 if clip is None else clip)
    if device:
        to = lambda a: torch.from_numpy(np.array(a, np.float32)).cuda()  # noqa: E731
        ptr = lambda t: t.data_ptr()  # noqa: E731
        norm = torch.full((1,), 7.0, device="cuda")
    else:
        to = lambda a: np.array(a, np.float32)  # noqa: E731
        ptr = lambda a: a.ctypes.data  # noqa: E731
        norm = np.full(1, 7.0, np.float32)
    P, G, M, V = [to(a) for a in params], [to(a) for a in grads], to(m), to(v)
    g_before = [a.cpu().numpy() if device else a.copy() for a in G]
    flags = (_lib.WOS_PTRS_DEVICE if device else 0) | (_lib.WOS_ASYNC if stream is not None else 0)
    if device:
        torch.cuda.synchronize()
    rc = lib.wos_adam_step(n, counts, (C.c_void_p * n)(*[ptr(a) for a in P]), (C.c_void_p * n)(*[ptr(a) for a in G]),
                           ptr(M), ptr(V), step, C.byref(opt), ptr(norm) if want_norm else None, flags, 0,
                           None if stream is None else stream.cuda_stream)
    assert rc == 0, lib.wos_last_error()
    if device:
        torch.cuda.synchronize()
    host = lambda a: a.cpu().numpy() if device else a  # noqa: E731
    assert all(np.array_equal(bits(host(a)), bits(b)) for a, b in zip(G, g_before)), "the gradients are read, never written"
    return [host(a) for a in P], host(M), host(V), host(norm)[0]


NETS = [(2, 32, 0, 1), (3, 96, 2, 3), (2, 256, 3, 2), (3, 32, 8, 3), (2, 160, 1, 2)]
CLIPS = [None, 0.1, 1e3]
KW_OTHER = dict(lr=1e-3, betas=(0.5, 0.9), eps=1e-6)
TINY = np.finfo(np.float32).tiny  # the least normal float32


@functools.lru_cache(maxsize=None)
def _problem(net, step):
    shapes = am.net_shapes(*net)
    return am.problem(shapes, seed=step + 10 * net[1], state=step > 1, top=0)


def _step_equals_the_model(net, step, clip, kw):
    params, grads, m, v = _problem(net, step)
    total = sum(a.size for a in params)
    if net == NETS[0]:
        assert total == 129 and params[-1].size == 1 and any(a.size % 4 for a in params)
    if net == (3, 32, 8, 3):  # the most tensors a call takes, the last one ending off a multiple of 4
        assert len(params) == 20 and total == 8675
    g = np.concatenate([a.reshape(-1) for a in grads])
    assert np.any(g == 0)
    want = am.step32(params, grads, m, v, step, max_grad_norm=clip, **kw)
    assert np.any(want[2] == 0), "v' = 0 somewhere: den = eps"
    got = _adam_c(params, grads, m, v, step, clip, device=True, kw=kw)
    for k, (a, b) in enumerate(zip(got[0], want[0])):
        assert a.shape == b.shape and same(a, b), f"parameter tensor {k}: {np.sum(bits(a) != bits(b))} of {a.size} differ"
    assert same(got[1], want[1]), "exp_avg"
    assert same(got[2], want[2]), "exp_avg_sq"
    if clip is None:
        assert got[3] == 7.0, "without clipping grad_norm is not written"
    else:
        assert same(got[3], want[3]), f"grad_norm {got[3]!r} model {want[3]!r}"
        active = am.clip32(want[3], clip) < 1
        assert active == (clip == 0.1)
    assert any(not same(a, b) for a, b in zip(got[0], params)), "the step moved the parameters"


@pytest.mark.parametrize("clip", CLIPS, ids=["noclip", "clip_active", "clip_inactive"])
@pytest.mark.parametrize("step", [1, 2, 1000, 40000])
@pytest.mark.parametrize("net", NETS, ids=[f"d{n[0]}_H{n[1]}_L{n[2]}_o{n[3]}" for n in NETS])
def test_adam_step_equals_the_float32_model_bit_for_bit(gpu, net, step, clip):
    """Step 40000 is the reference's iteration count: sqrt(1 - beta2^step) is exactly 1 and
    lr / (1 - beta1^step) exactly lr."""
    if step == 40000:
        s = am.scalars(step=step, **KW)
        assert s["bc2"] == 1.0 and s["ss"] == KW["lr"]
    _step_equals_the_model(net, step, clip, KW)


@pytest.mark.parametrize("clip", [None, 0.1], ids=["noclip", "clip_active"])
@pytest.mark.parametrize("step", [1, 40000])
@pytest.mark.parametrize("net", [NETS[0], NETS[3]], ids=[f"d{n[0]}_H{n[1]}_L{n[2]}_o{n[3]}" for n in (NETS[0], NETS[3])])
def test_adam_step_with_other_hyper_parameters_bit_for_bit(gpu, net, step, clip):
    """lr = 1e-3, betas = (0.5, 0.9), eps = 1e-6: none of the five step scalars is the default's."""
    _step_equals_the_model(net, step, clip, KW_OTHER)


@pytest.mark.parametrize("clip", [None, 0.1], ids=["noclip", "clip_active"])
def test_adam_step_keeps_subnormals_bit_for_bit(gpu, clip):
    """Gradual underflow, as numpy's float32 has it: (1 - beta2) g g and v' subnormal or zero from
    a non-zero gradient, subnormal v and m on input."""
    net, step = NETS[0], 2
    params, grads, m, v = am.problem(am.net_shapes(*net), seed=step + 10 * net[1], state=True, top=0, subnormal=True)
    g = np.concatenate([a.reshape(-1) for a in grads])
    want = am.step32(params, grads, m, v, step, max_grad_norm=clip, **KW)
    assert np.any((v > 0) & (v < TINY)) and np.any((m != 0) & (np.abs(m) < TINY)), "subnormal moments on input"
    assert np.any((want[2] > 0) & (want[2] < TINY)), "a subnormal v'"
    assert np.any((want[2] == 0) & (g != 0)), "(1 - beta2) g g underflowed to zero"
    got = _adam_c(params, grads, m, v, step, clip, device=True)
    for k, (a, b) in enumerate(zip(got[0], want[0])):
        assert same(a, b), f"parameter tensor {k}: {np.sum(bits(a) != bits(b))} of {a.size} differ"
    assert same(got[1], want[1]), f"exp_avg: {np.flatnonzero(bits(got[1]) != bits(want[1]))[:8]}"
    assert same(got[2], want[2]), f"exp_avg_sq: {np.flatnonzero(bits(got[2]) != bits(want[2]))[:8]}"
    if clip is not None:
        assert same(got[3], want[3])


def test_adam_step_pointers_determinism_and_side_stream(gpu):
    net, step = NETS[1], 2
    params, grads, m, v = _problem(net, step)
    for clip in (None, 0.1):
        dev = _adam_c(params, grads, m, v, step, clip, device=True)
        hst = _adam_c(params, grads, m, v, step, clip, device=False)
        again = _adam_c(params, grads, m, v, step, clip, device=True)
        side = _adam_c(params, grads, m, v, step, clip, device=True, stream=torch.cuda.Stream())
        quiet = _adam_c(params, grads, m, v, step, clip, device=True, want_norm=False)  # grad_norm NULL
        for what, other in (("host pointers", hst), ("a second call", again), ("a side stream", side)):
            assert all(same(a, b) for a, b in zip(dev[0], other[0])) and same(dev[1], other[1]) and same(dev[2], other[2]), what
            assert same(dev[3], other[3]), what
        assert all(same(a, b) for a, b in zip(dev[0], quiet[0])) and same(dev[1], quiet[1]) and quiet[3] == 7.0


@pytest.mark.parametrize("clip", [None, 0.1], ids=["noclip", "clip"])
def test_three_consecutive_steps_from_zero_state_through_the_python_layer(gpu, clip):
    d, H, L, d_out = 3, 96, 2, 3
    net = _cuda_net(d, H, L, d_out)
    state = siren.AdamState(net, max_grad_norm=clip, **KW)
    params = [t.cpu().numpy().copy() for t in _tensors(net)]
    m, v = np.zeros(state.exp_avg.numel(), np.float32), np.zeros(state.exp_avg.numel(), np.float32)
    nl = L + 2
    for i in range(3):
        grads = am.problem(am.net_shapes(d, H, L, d_out), seed=40 + i)[1]
        norm = siren.adam_step(net, ([torch.from_numpy(a).cuda() for a in grads[:nl]],
                                     [torch.from_numpy(a).cuda() for a in grads[nl:]]), state)
        params, m, v, want_norm = am.step32(params, grads, m, v, i + 1, max_grad_norm=clip, **KW)
        assert state.step == i + 1
        assert all(same(t, a) for t, a in zip(_tensors(net), params)), f"step {i + 1}"
        assert same(state.exp_avg, m) and same(state.exp_avg_sq, v)
        assert (norm is None) == (clip is None) and (clip is None or (norm.is_cuda and same(norm, want_norm)))
    # numpy gradients: the host-pointer path leaves the network alone and returns the updated copies
    grads = am.problem(am.net_shapes(d, H, L, d_out), seed=50)[1]
    before = [t.clone() for t in _tensors(net)]
    w, b, norm = siren.adam_step(net, (grads[:nl], grads[nl:]), state)
    params, m, v, want_norm = am.step32(params, grads, m, v, 4, max_grad_norm=clip, **KW)
    assert state.step == 4 and all(same(a, c) for a, c in zip(w + b, params)) and same(state.exp_avg, m)
    assert all(torch.equal(t, c) for t, c in zip(_tensors(net), before))
    assert (norm is None) == (clip is None) and (clip is None or same(norm, want_norm))


# ---- 2. against the reference optimiser ------------------------------------------------------------------
def _torch_adam_on_the_gpu(params, grads, m, v, step, clip):
    """clip_grad_norm_ and torch.optim.Adam(**KW).step() on the GPU with the state (m, v, step - 1) injected.
    Returns (the stepped parameter tensors, the optimiser)."""
    ps = [torch.from_numpy(a.copy()).cuda().requires_grad_(True) for a in params]
    opt = torch.optim.Adam(ps, **KW)
    at = 0
    for t, g in zip(ps, grads):
        n = t.numel()
        t.grad = torch.from_numpy(g.copy()).cuda()
        opt.state[t] = {"step": torch.tensor(float(step - 1)),
                        "exp_avg": torch.from_numpy(m[at:at + n].reshape(t.shape).copy()).cuda(),
                        "exp_avg_sq": torch.from_numpy(v[at:at + n].reshape(t.shape).copy()).cuda()}
        at += n
    if clip is not None:
        torch.nn.utils.clip_grad_norm_(ps, clip)
    opt.step()
    return ps, opt


@pytest.mark.parametrize("clip", CLIPS, ids=["noclip", "clip_active", "clip_inactive"])
def test_adam_step_against_torch_adam_on_the_gpu(gpu, clip):
    net, step = NETS[2], 7
    params, grads, m, v = _problem(net, step)
    got = _adam_c(params, grads, m, v, step, clip, device=True)
    ps, opt = _torch_adam_on_the_gpu(params, grads, m, v, step, clip)
    d = opt.defaults
    print(f"torch.optim.Adam on the GPU: foreach={d.get('foreach')} fused={d.get('fused')} capturable={d.get('capturable')} "
          f"(foreach None: torch's default, the foreach implementation on CUDA tensors)")
    ref = am.step64(params, grads, m, v, step, max_grad_norm=clip, **KW)
    B = am.bound(ref[4])
    want = np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in ps]).astype(np.float64)
    have = np.concatenate([a.reshape(-1) for a in got[0]]).astype(np.float64)
    diff = np.abs(have - want)
    print(f"clip {clip}: bit-equal {np.mean(have == want):.4f}; ours / B {np.max(np.abs(have - ref[4]['p']) / B):.3f}, "
          f"torch / B {np.max(np.abs(want - ref[4]['p']) / B):.3f}, difference / 2B {np.max(diff / (2 * B)):.3f}")
    assert np.all(diff <= 2 * B)


def _flat(arrays):
    return np.concatenate([(a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)).reshape(-1) for a in arrays])


def _same_nans_and_bits(a, b, what):
    """NaN in the same places, and every other element -- an infinity included -- the same bits."""
    a, b = _flat([a]), _flat([b])
    assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: NaN differs at {np.flatnonzero(np.isnan(a) != np.isnan(b))[:8]}"
    ok = ~np.isnan(a)
    assert np.array_equal(bits(a)[ok], bits(b)[ok]), f"{what}: {np.sum(bits(a)[ok] != bits(b)[ok])} finite elements differ"


@pytest.mark.parametrize("clip", [None, 0.1], ids=["noclip", "clip"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_adam_step_on_a_non_finite_gradient(gpu, bad, clip):
    """clip_grad_norm_ + Adam.step() on one NaN or +inf gradient element: with clipping a NaN norm
    gives a NaN coefficient and every element goes NaN; an infinite norm gives a coefficient of 0,
    NaN at the element and a zero gradient elsewhere; without clipping only the element is touched.
    The device against the float32 model -- NaN in the same places, every other bit equal -- and
    against torch's Adam on the GPU, NaN in the same places."""
    net, step = NETS[1], 2
    params, grads, m, v = _problem(net, step)
    grads = [a.copy() for a in grads]
    grads[1][5, 7] = bad  # the second tensor, past a tensor boundary
    at = params[0].size + 5 * grads[1].shape[1] + 7
    with np.errstate(invalid="ignore", over="ignore"):
        want = am.step32(params, grads, m, v, step, max_grad_norm=clip, **KW)
    got = _adam_c(params, grads, m, v, step, clip, device=True)
    _same_nans_and_bits(_flat(got[0]), _flat(want[0]), "parameters")
    _same_nans_and_bits(got[1], want[1], "exp_avg")
    _same_nans_and_bits(got[2], want[2], "exp_avg_sq")
    if clip is not None:
        _same_nans_and_bits(got[3], want[3], "grad_norm")
    ps, opt = _torch_adam_on_the_gpu(params, grads, m, v, step, clip)
    for what, a, b in (("parameters", _flat(got[0]), _flat(ps)), ("exp_avg", got[1], _flat([opt.state[t]["exp_avg"] for t in ps])),
                       ("exp_avg_sq", got[2], _flat([opt.state[t]["exp_avg_sq"] for t in ps]))):
        assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what} against torch: NaN differs at {np.flatnonzero(np.isnan(a) != np.isnan(b))[:8]}"
    nan_p = np.isnan(_flat(got[0]))
    if clip is not None and np.isnan(bad):
        assert nan_p.all() and np.isnan(got[1]).all() and np.isnan(got[2]).all() and np.isnan(got[3])
    else:
        only = np.zeros(nan_p.size, bool)
        only[at] = True
        assert np.array_equal(nan_p, only) and np.array_equal(~np.isfinite(got[1]), only)
        assert np.array_equal(~np.isfinite(got[2]), only)


# ---- 3. run = separate calls, bit for bit ------------------------------------------------------------------
N_POOL, K = 211, 4


def _pool(d, d_out, with_scale):
    x = torch.from_numpy(sm.points(d, N_POOL, seed=6)).cuda()
    target, scale = fm.problem(N_POOL, d_out, with_scale, seed=3)
    return x, torch.from_numpy(target).cuda(), None if scale is None else torch.from_numpy(scale).cuda()


def _idx(batch, k=K, seed=0):
    """[k, batch] indices into the pool: both ends of it, and a duplicate in every row that has room."""
    idx = torch.from_numpy(np.random.default_rng(100 + seed + batch).integers(0, N_POOL, (k, batch))).to(torch.int64)
    idx[0, 0], idx[-1, -1] = 0, N_POOL - 1
    if batch >= 3:
        idx[:, 0], idx[:, 1], idx[:, -1] = 0, 0, N_POOL - 1
    return idx.contiguous().cuda()


def _loop(net, state, pool, idx, n=None, ws=None):
    """The three existing calls made separately, n iterations: gather, siren.fit, siren.adam_step."""
    x, target, scale = pool
    losses = []
    for i in range(idx.shape[0] if n is None else n):
        row = idx[i]
        loss, gw, gb = siren.fit(net, x[row], target[row], None if scale is None else scale[row], workspace_bytes=ws)
        siren.adam_step(net, (gw, gb), state)
        losses.append(loss)
    return torch.stack(losses)


def _same_run(net_a, state_a, net_b, state_b, what):
    for k, (a, b) in enumerate(zip(_tensors(net_a), _tensors(net_b))):
        assert same(a, b), f"{what}: parameter tensor {k}, {np.sum(bits(a) != bits(b))} of {a.numel()} differ"
    assert same(state_a.exp_avg, state_b.exp_avg), f"{what}: exp_avg"
    assert same(state_a.exp_avg_sq, state_b.exp_avg_sq), f"{what}: exp_avg_sq"
    assert state_a.step == state_b.step, what


RUNS = [((2, 64, 1, 2), True, b, 0.1) for b in (1, 32, 65, 545)] + [((3, 96, 2, 3), False, b, None) for b in (1, 32, 65, 545)] + [
    ((2, 256, 3, 2), True, 65, None),
    ((3, 32, 8, 3), True, 65, 0.1),      # L = 8: 12 reduce segments in the fit step, 20 tensors in the Adam step
    ((2, 160, 1, 2), False, 65, None)]   # H / 32 = 5: a dropped row tile and a partial second 128-tile of dW


@pytest.mark.parametrize("shape,with_scale,batch,clip", RUNS,
                         ids=[f"d{s[0]}_H{s[1]}_L{s[2]}_{'scale' if w else 'plain'}_b{b}" for s, w, b, c in RUNS])
def test_fit_run_equals_the_separate_calls(gpu, shape, with_scale, batch, clip):
    pool, idx = _pool(shape[0], shape[3], with_scale), _idx(batch)
    assert int(idx.min()) == 0 and int(idx.max()) == N_POOL - 1
    net_a, net_b = _cuda_net(*shape), _cuda_net(*shape)
    state_a, state_b = siren.AdamState(net_a, max_grad_norm=clip, **KW), siren.AdamState(net_b, max_grad_norm=clip, **KW)
    want = _loop(net_a, state_a, pool, idx)
    losses, status = siren.fit_run(net_b, state_b, *pool, idx)
    assert losses.is_cuda and losses.shape == (K,) and status.dtype == torch.int64 and status.tolist() == [K, 0]
    assert same(losses, want), f"losses {losses.tolist()} separate calls {want.tolist()}"
    assert bool(torch.isfinite(losses).all()) and state_b.step == K
    _same_run(net_a, state_a, net_b, state_b, "fit_run")
    assert any(not same(a, b) for a, b in zip(_tensors(net_b), _tensors(_cuda_net(*shape)))), "the run moved the network"


def test_fit_run_without_a_hidden_layer_equals_the_separate_calls(gpu):
    """L = 0: no packed copies in the run's temporary, which starts with the H zeros."""
    shape, k = (2, 32, 0, 2), 2
    pool, idx = _pool(2, 2, True), _idx(33, k=k)  # one full tile and one point
    net_a, net_b = _cuda_net(*shape), _cuda_net(*shape)
    state_a, state_b = siren.AdamState(net_a, max_grad_norm=0.1, **KW), siren.AdamState(net_b, max_grad_norm=0.1, **KW)
    want = _loop(net_a, state_a, pool, idx)
    losses, status = siren.fit_run(net_b, state_b, *pool, idx)
    assert status.tolist() == [k, 0] and same(losses, want), f"losses {losses.tolist()} separate calls {want.tolist()}"
    assert bool(torch.isfinite(losses).all()) and state_b.step == k
    _same_run(net_a, state_a, net_b, state_b, "fit_run, L = 0")
    assert any(not same(a, b) for a, b in zip(_tensors(net_b), _tensors(_cuda_net(*shape)))), "the run moved the network"


def test_fit_run_chunked_and_continued(gpu):
    shape, batch = (2, 64, 1, 2), 65
    pool, idx = _pool(2, 2, True), _idx(batch)
    ws = (2 * 1 + 1) * 64 * 4 * 32  # one tile: three chunks per step
    net_a, net_b = _cuda_net(*shape), _cuda_net(*shape)
    state_a, state_b = siren.AdamState(net_a, **KW), siren.AdamState(net_b, **KW)
    want = _loop(net_a, state_a, pool, idx, ws=ws)
    losses, _ = siren.fit_run(net_b, state_b, *pool, idx, workspace_bytes=ws)
    assert same(losses, want)
    _same_run(net_a, state_a, net_b, state_b, "one-tile workspace")
    # step0 = 5 with a non-zero state: two runs of 2 equal one run of 4
    base, base_state = _cuda_net(*shape), siren.AdamState(_cuda_net(*shape), **KW)
    siren.fit_run(base, base_state, *pool, _idx(batch, k=5, seed=9))
    assert base_state.step == 5 and bool(base_state.exp_avg.any()) and bool(base_state.exp_avg_sq.any())
    net_1, state_1, net_2, state_2 = copy.deepcopy(base), copy.deepcopy(base_state), copy.deepcopy(base), copy.deepcopy(base_state)
    whole, _ = siren.fit_run(net_1, state_1, *pool, idx)
    first, _ = siren.fit_run(net_2, state_2, *pool, idx[:2].contiguous())
    assert state_2.step == 7
    second, _ = siren.fit_run(net_2, state_2, *pool, idx[2:].contiguous())
    assert same(whole, torch.cat([first, second])) and state_1.step == 9
    _same_run(net_1, state_1, net_2, state_2, "two runs of 2 against one run of 4")


# ---- 4. early stop -------------------------------------------------------------------------------------------
def test_early_stop(gpu):
    shape, batch = (2, 64, 1, 2), 65
    pool = _pool(2, 2, True)
    idx = _idx(batch)[:1].repeat(K, 1).contiguous()  # the same batch every iteration: the loss goes down
    free_net, free_state = _cuda_net(*shape), siren.AdamState(_cuda_net(*shape), **KW)
    free, status = siren.fit_run(free_net, free_state, *pool, idx)
    assert status.tolist() == [K, 0] and bool(torch.isfinite(free).all())
    assert float(free[0]) > float(free[1]), f"the test's premise, a falling loss: {free.tolist()}"
    stop = float(free[1])  # the run is deterministic: the bits are known
    two_net, two_state = _cuda_net(*shape), siren.AdamState(_cuda_net(*shape), **KW)
    _loop(two_net, two_state, pool, idx, n=2)
    results = []
    for check_every in (0, 1):
        net, state = _cuda_net(*shape), siren.AdamState(_cuda_net(*shape), **KW)
        losses, status = siren.fit_run(net, state, *pool, idx, stop_loss=stop, check_every=check_every)
        assert status.tolist() == [2, 0] and state.step == 2, (check_every, status.tolist())
        assert same(losses[:2], free[:2]) and bool(torch.isnan(losses[2:]).all()), losses.tolist()
        _same_run(two_net, two_state, net, state, f"stopped after two steps (check_every {check_every})")
        results.append(losses)
    assert same(results[0], results[1])
    # a threshold nothing reaches: never stops, and equals the free run; one that the first loss meets: one step
    net, state = _cuda_net(*shape), siren.AdamState(_cuda_net(*shape), **KW)
    losses, status = siren.fit_run(net, state, *pool, idx, stop_loss=0.0, check_every=3)
    assert status.tolist() == [K, 0] and same(losses, free) and state.step == K
    _same_run(free_net, free_state, net, state, "stop_loss 0")
    net, state = _cuda_net(*shape), siren.AdamState(_cuda_net(*shape), **KW)
    losses, status = siren.fit_run(net, state, *pool, idx, stop_loss=float(free[0]))
    assert status.tolist() == [1, 0] and same(losses[:1], free[:1]) and bool(torch.isnan(losses[1:]).all()) and state.step == 1


def test_stop_loss_minus_one_never_stops_through_the_c_abi(gpu):
    shape, batch = (2, 64, 1, 2), 32
    pool, idx = _pool(2, 2, False), _idx(batch)
    net_a, net_b = _cuda_net(*shape), _cuda_net(*shape)
    state_a, state_b = siren.AdamState(net_a, **KW), siren.AdamState(net_b, **KW)
    want, _ = siren.fit_run(net_a, state_a, *pool, idx)
    p = siren.pack(net_b)
    w = (C.c_void_p * 3)(*[t.data_ptr() for t in p.weights])
    b = (C.c_void_p * 3)(*[t.data_ptr() for t in p.biases])
    st = _lib.SirenNet(p.d_in, p.d_out, p.hidden, p.n_hidden_layers, p.omega, w, b)
    losses, status = torch.zeros(K, device="cuda"), torch.full((2,), 9, dtype=torch.int64, device="cuda")
    opt = state_b.params()
    torch.cuda.synchronize()
    lib = _lib.load()
    rc = lib.wos_siren_fit_run(C.byref(st), pool[0].data_ptr(), pool[1].data_ptr(), None, N_POOL, idx.data_ptr(), K, batch,
                               state_b.exp_avg.data_ptr(), state_b.exp_avg_sq.data_ptr(), 0, C.byref(opt), -1.0, 2,
                               losses.data_ptr(), status.data_ptr(), 0, _lib.WOS_PTRS_DEVICE, 0, None)
    assert rc == 0, lib.wos_last_error()
    state_b.step = K
    assert status.tolist() == [K, 0] and same(losses, want)
    _same_run(net_a, state_a, net_b, state_b, "blocking, check_every 2, stop_loss -1")


# ---- 4b. a NaN target ------------------------------------------------------------------------------------------
def _nan_row_case(idx):
    """A pool whose target row `row` is NaN, with idx[2, 0] = row and the row drawn nowhere before
    iteration 2.  Returns (clean pool, poisoned pool, idx)."""
    pool = _pool(2, 2, True)
    early = set(idx[:2].reshape(-1).tolist())
    row = next(r for r in range(1, N_POOL - 1) if r not in early)
    idx = idx.clone()
    idx[2, 0] = row
    target = pool[1].clone()
    target[row] = float("nan")
    return pool, (pool[0], target, pool[2]), idx.contiguous()


def test_fit_run_with_a_nan_target_poisons_the_network_as_the_separate_calls_do(gpu):
    """Clipping on: the NaN loss of iteration 2 gives a NaN norm, a NaN clip coefficient and a network
    that is NaN throughout, as clip_grad_norm_ + Adam.step() leave it -- not a half-poisoned one."""
    shape, batch, clip = (2, 64, 1, 2), 32, 0.1
    clean_pool, pool, idx = _nan_row_case(_idx(batch))
    net_c, net_a, net_b = _cuda_net(*shape), _cuda_net(*shape), _cuda_net(*shape)
    state_c, state_a, state_b = [siren.AdamState(n, max_grad_norm=clip, **KW) for n in (net_c, net_a, net_b)]
    clean, status = siren.fit_run(net_c, state_c, *clean_pool, idx)
    assert status.tolist() == [K, 0] and bool(torch.isfinite(clean).all())
    want = _loop(net_a, state_a, pool, idx)
    losses, status = siren.fit_run(net_b, state_b, *pool, idx)
    assert status.tolist() == [K, 0] and state_b.step == K
    assert bool(torch.isfinite(losses[:2]).all()) and same(losses[:2], clean[:2]), losses.tolist()
    assert bool(torch.isnan(losses[2:]).all()), losses.tolist()
    for k, t in enumerate(_tensors(net_b)):
        assert bool(torch.isnan(t).all()), f"parameter tensor {k}: {int((~torch.isnan(t)).sum())} of {t.numel()} are not NaN"
    assert bool(torch.isnan(state_b.exp_avg).all()) and bool(torch.isnan(state_b.exp_avg_sq).all())
    _same_nans_and_bits(losses, want, "losses")
    for k, (a, b) in enumerate(zip(_tensors(net_b), _tensors(net_a))):
        _same_nans_and_bits(a, b, f"parameter tensor {k}")
    _same_nans_and_bits(state_b.exp_avg, state_a.exp_avg, "exp_avg")
    _same_nans_and_bits(state_b.exp_avg_sq, state_a.exp_avg_sq, "exp_avg_sq")


@pytest.mark.parametrize("check_every", [0, 1])
def test_a_nan_loss_never_stops_the_run(gpu, check_every):
    """stop_loss one ulp below the clean run's second loss: not met by iterations 0 and 1, and a NaN
    loss is not <= stop_loss, as with the Python loop's `loss < threshold`."""
    shape, batch, clip = (2, 64, 1, 2), 32, 0.1
    clean_pool, pool, idx = _nan_row_case(_idx(batch)[:1].repeat(K, 1))  # the same batch: the clean loss falls
    net_c, state_c = _cuda_net(*shape), siren.AdamState(_cuda_net(*shape), max_grad_norm=clip, **KW)
    clean, _ = siren.fit_run(net_c, state_c, *clean_pool, idx)
    assert float(clean[0]) > float(clean[1]), f"the test's premise, a falling loss: {clean.tolist()}"
    stop = float(np.nextafter(np.float32(clean[1].item()), np.float32(0)))
    assert 0 <= stop < float(clean[1])
    net, state = _cuda_net(*shape), siren.AdamState(_cuda_net(*shape), max_grad_norm=clip, **KW)
    losses, status = siren.fit_run(net, state, *pool, idx, stop_loss=stop, check_every=check_every)
    assert status.tolist() == [K, 0] and state.step == K
    assert same(losses[:2], clean[:2]) and bool(torch.isnan(losses[2:]).all()), losses.tolist()
    assert all(bool(torch.isnan(t).all()) for t in _tensors(net))


# ---- 5. a bad index ------------------------------------------------------------------------------------------
def test_an_index_past_the_pool_is_clamped_counted_and_refused(gpu):
    """No fault is provoked: the kernel clamps the row, and that clamp is what this pins."""
    shape, batch = (2, 64, 1, 2), 32
    pool = _pool(2, 2, True)
    good = _idx(batch)
    good[1, 5] = N_POOL - 1
    bad = good.clone()
    bad[1, 5] = N_POOL
    net_a, net_b, net_c = _cuda_net(*shape), _cuda_net(*shape), _cuda_net(*shape)
    state_a, state_b, state_c = [siren.AdamState(n, **KW) for n in (net_a, net_b, net_c)]
    want, status = siren.fit_run(net_a, state_a, *pool, good)
    assert status.tolist() == [K, 0]
    losses, status = siren.fit_run(net_b, state_b, *pool, bad)  # enqueued without a host wait: the count tells
    assert status.tolist() == [K, 1] and same(losses, want), "the row was clamped to the pool's last"
    _same_run(net_a, state_a, net_b, state_b, "clamped")
    with pytest.raises(_lib.WosError, match=r"\(-1\).*idx.*outside \[0, n_pool\)"):
        siren.fit_run(net_c, state_c, *pool, bad, check_every=2)  # the blocking call
    assert state_c.step == K, "the refused run was applied: the state's step follows it"
    _same_run(net_a, state_a, net_c, state_c, "clamped, blocking")


# ---- 6. end to end -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _karman():
    cfg = workloads.karman_config(n_walks=16, n_points=200)
    scene_cfg = dict(workloads.SCENE_BASE, boundary=workloads.KARMAN_OBJ)
    samples = torch.from_numpy(cfg["points"]).cuda()
    return pj.PressureProjector(scene_cfg, cfg["solver"], cfg["output"], samples), samples


@pytest.mark.parametrize("wrapped", [False, True], ids=["plain", "karman_wrap"])
def test_fit_projection_end_to_end(gpu, wrapped):
    proj, samples = _karman()
    box = [samples[:, 0].min().item(), samples[:, 0].max().item(), samples[:, 1].min().item(), samples[:, 1].max().item()]
    wrap = sm.karman_wrap(box, eps=0.125) if wrapped else None
    net_prev = _cuda_net(2, 128, 2, seed=1)
    grad_p = torch.from_numpy(np.random.default_rng(11).standard_normal((200, 2)).astype(np.float32) * 0.1).cuda()
    n_samples, n_iters = 193, 3
    gen = lambda: torch.Generator(device="cuda").manual_seed(77)  # noqa: E731
    net = _cuda_net(2, 128, 2)
    first = proj.projection_fit_loss(net, net_prev, grad_p, n_samples, wrap=wrap, generator=gen())
    g1, g2 = gen(), gen()
    losses, state = proj.fit_projection(net, net_prev, grad_p, n_samples, n_iters, wrap=wrap, generator=g1, iters_per_call=2)
    assert losses.shape == (n_iters,) and bool(torch.isfinite(losses).all()) and state.step == n_iters
    assert same(losses[0], first), f"iteration 0 {float(losses[0])!r} projection_fit_loss {float(first)!r}"
    for _ in range(n_iters):
        proj.projection_fit_loss(net, net_prev, grad_p, n_samples, wrap=wrap, generator=g2)
    assert torch.equal(g1.get_state(), g2.get_state())
    # the same run on a pool built by hand
    with torch.no_grad():
        u_prev = siren.eval(net_prev, samples)
        if wrapped:
            scale, offset = siren.diagonal_wrap(wrap, samples, 2)
            target = wrap(samples, u_prev) - grad_p - offset
        else:
            scale, target = None, u_prev - grad_p
    g3 = gen()
    idx = torch.stack([torch.randint(0, 199, (n_samples,), device="cuda", generator=g3) for _ in range(n_iters)])
    hand, hand_state = _cuda_net(2, 128, 2), siren.AdamState(_cuda_net(2, 128, 2), lr=1e-4)
    by_hand, _ = siren.fit_run(hand, hand_state, samples, target, scale, idx)
    assert same(losses, by_hand)
    _same_run(hand, hand_state, net, state, "fit_projection against fit_run on a pool built by hand")


@pytest.mark.parametrize("per_call", [1, 2])
def test_fit_projection_stops_on_the_last_iteration_of_a_block(gpu, per_call):
    """The threshold is the free run's loss of iteration per_call - 1, the first block's last.  The
    run is deterministic, so where it stops is known from the free run's losses; a stop there leaves
    status[0] equal to the block's length."""
    proj, samples = _karman()
    net_prev = _cuda_net(2, 64, 1, 2, seed=1)
    grad_p = torch.from_numpy(np.random.default_rng(11).standard_normal((200, 2)).astype(np.float32) * 0.1).cuda()
    gen = lambda: torch.Generator(device="cuda").manual_seed(31)  # noqa: E731
    n_samples, n_iters = 65, 4
    free, _ = proj.fit_projection(_cuda_net(2, 64, 1, 2), net_prev, grad_p, n_samples, n_iters, generator=gen(),
                                  iters_per_call=per_call)
    thr = float(free[per_call - 1])
    at = int(np.flatnonzero(free.cpu().numpy() <= np.float32(thr))[0])  # per_call - 1, or an earlier one
    assert at <= per_call - 1
    net, g1 = _cuda_net(2, 64, 1, 2), gen()
    losses, state = proj.fit_projection(net, net_prev, grad_p, n_samples, n_iters, generator=g1, early_stop=thr,
                                        iters_per_call=per_call)
    assert state.step == at + 1, f"stopped after {state.step} steps, the free run's losses {free.tolist()} say {at + 1}"
    assert same(losses[:at + 1], free[:at + 1]) and bool(torch.isnan(losses[at + 1:]).all()), losses.tolist()
    g2 = gen()
    for _ in range(per_call):  # one block was drawn, and no further one
        torch.randint(0, 199, (n_samples,), device="cuda", generator=g2)
    assert torch.equal(g1.get_state(), g2.get_state())
    want, want_state = _cuda_net(2, 64, 1, 2), siren.AdamState(_cuda_net(2, 64, 1, 2), lr=1e-4)
    proj.fit_projection(want, net_prev, grad_p, n_samples, at + 1, state=want_state, generator=gen(), iters_per_call=per_call)
    _same_run(want, want_state, net, state, "stopped on a block's last iteration")


def test_two_hundred_iterations_lower_the_loss_over_the_pool(gpu):
    """Smoke level only: the correctness claims rest on the tests above."""
    proj, samples = _karman()
    net, net_prev = _cuda_net(2, 64, 1, 2), _cuda_net(2, 64, 1, 2, seed=1)
    grad_p = torch.from_numpy(np.random.default_rng(11).standard_normal((200, 2)).astype(np.float32) * 0.1).cuda()
    target = siren.eval(net_prev, samples) - grad_p
    before = float(siren.fit(net, samples, target, grads=False))
    losses, state = proj.fit_projection(net, net_prev, grad_p, 193, 200, generator=torch.Generator(device="cuda").manual_seed(5))
    after = float(siren.fit(net, samples, target, grads=False))
    print(f"loss over the pool before {before:.6e} after 200 iterations {after:.6e}")
    assert state.step == 200 and bool(torch.isfinite(losses).all()) and after < before
