"""The fit step and the fit loops through a wrap that mixes the velocity's components, on the GPU
(WOS_FIT_SCALE_MATRIX: csrc/wos_siren_fit.hip, csrc/wos_siren_train.hip, wos_amd.siren,
wos_amd.projection): every parameter gradient against the float64 model with float32 autograd of
mean((S net(x) - t)^2) as the yardstick and the loss against float64 of siren.eval's own u bits
within the derived bound; a diagonal matrix against the diagonal call, value for value; chunks,
pointer kinds, determinism, a side stream; the loops against the separate calls, bit for bit; the
refusals; and the time-stepper's two losses and two loops through a slip wrap end to end.

Measured on the MI355X (loss error / bound and the gradients' ratios to float32 autograd's error,
caps 2.5 RMS / 4 max): see profiles/siren_fit_matrix_accuracy.json."""
import copy
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import siren_fit_matrix_model as mm
import siren_fit_model as fm
import siren_model as sm
import siren_vjp_model as vm
from wos_amd import _lib, siren, workloads
from wos_amd import projection as pj

pytestmark = pytest.mark.gpu

KW = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8)


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def host(out):
    """fit()'s (loss, gw, gb) on the host: (loss float32 scalar, ([w], [b]))."""
    loss, gw, gb = out
    return np.float32(loss.cpu().numpy()), ([t.cpu().numpy() for t in gw], [t.cpu().numpy() for t in gb])


def same_bits(a, b):
    return same(a[0], b[0]) and all(same(s, t) for s, t in zip(a[1][0] + a[1][1], b[1][0] + b[1][1]))


def same_values(a, b):
    """np.array_equal on the values: -0.0 equals 0.0, which is all a diagonal matrix may change."""
    return np.array_equal(a[0], b[0]) and all(np.array_equal(s, t) for s, t in zip(a[1][0] + a[1][1], b[1][0] + b[1][1]))


def _cuda_net(d, H, L, d_out=None, seed=0):
    return copy.deepcopy(sm.make_net(d, H, L, d_out, seed=seed)).cuda()


def _dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


def _fit(net, x, target, S, **kw):
    return host(siren.fit(net, _dev(x), _dev(target), _dev(S), **kw))


def _tensors(net):
    p = siren.pack(net)
    return p.weights + p.biases


def _same_run(net_a, state_a, net_b, state_b, what):
    for k, (a, b) in enumerate(zip(_tensors(net_a), _tensors(net_b))):
        assert same(a, b), f"{what}: parameter tensor {k}, {np.sum(bits(a) != bits(b))} of {a.numel()} differ"
    assert same(state_a.exp_avg, state_b.exp_avg), f"{what}: exp_avg"
    assert same(state_a.exp_avg_sq, state_b.exp_avg_sq), f"{what}: exp_avg_sq"
    assert state_a.step == state_b.step, what


# ---- 1. accuracy against float64 -------------------------------------------------------------------------
SHAPES = [(2, 32, 1, 2), (3, 64, 1, 3), (2, 256, 3, 2), (3, 256, 3, 3), (2, 64, 1, 3), (3, 64, 1, 2), (3, 64, 1, 1)]


@functools.lru_cache(maxsize=None)
def _reference(d, H, L, d_out, n=193):
    """(x, target, S, float64 (loss, grads, ub), float32 autograd on the GPU) of one case, computed once."""
    net, x = sm.make_net(d, H, L, d_out), sm.points(d, n, seed=0)
    target, S = mm.problem(n, d_out)
    ref = mm.model64(net, x, target, S)
    t32 = mm.autograd(_cuda_net(d, H, L, d_out), torch.from_numpy(x).cuda(), target, S)
    return x, target, S, ref, t32


@pytest.mark.parametrize("shape", SHAPES, ids=[f"d{s[0]}_H{s[1]}_L{s[2]}_o{s[3]}" for s in SHAPES])
def test_loss_and_gradients_against_float64(gpu, shape):
    d, H, L, d_out = shape
    x, target, S, (_, ref, ub), (_, t32) = _reference(*shape)
    assert np.any(S == 0) and np.any(np.all(S == 0, axis=(1, 2))), "the case: exact zeros, and an inlet"
    net = _cuda_net(*shape)
    got = _fit(net, x, target, S)
    u = siren.eval(net, _dev(x)).cpu().numpy()
    bound, L64 = mm.loss_bound(u, target, S)
    error = abs(float(got[0]) - L64)
    print(f"loss {got[0]:.9e} float64 of eval's u {L64:.9e} error {error:.3e} bound {bound:.3e}")
    rec = {"loss_error": error, "loss_bound": bound}
    try:
        assert L64 > 0 and error <= bound
        vm.assert_grads_as_accurate(got[1], t32, ref, ub, f"({d},{H},{L},{d_out}) matrix", record=rec)
    finally:
        out = os.environ.get("WOS_SIREN_FIT_MATRIX_ACCURACY_OUT")  # a measuring run keeps the figures; the suite writes nothing
        if out:
            with open(out, "a") as f:
                f.write(json.dumps({"d": d, "hidden": H, "hidden_layers": L, "d_out": d_out, "points": 193, **rec}) + "\n")


# ---- 2. the diagonal twin ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 32, 33, 65, 545])
@pytest.mark.parametrize("shape", [(2, 64, 1, 2), (3, 64, 1, 3)], ids=["2to2", "3to3"])
def test_a_diagonal_matrix_equals_the_diagonal_call(gpu, shape, n):
    """fmaf(0, u, r) = r: S = diag(s) gives the values of scale = s, and S = I those of scale = None, in the
    loss and in every gradient -- the new path pinned against the tested one."""
    d, H, L, d_out = shape
    net = _cuda_net(*shape)
    x = sm.points(d, n, seed=1)
    target, scale = fm.problem(n, d_out, True, seed=n)
    assert np.any(scale == 0)
    want = _fit(net, x, target, scale)
    got = _fit(net, x, target, mm.diagonal(scale))
    assert np.isfinite(want[0]) and want[0] > 0 and all(np.any(a) for a in want[1][0] + want[1][1])
    assert same_values(got, want), f"loss {got[0]!r} the diagonal call's {want[0]!r}"
    eye = np.broadcast_to(np.eye(d_out, dtype=np.float32), (n, d_out, d_out)).copy()
    assert same_values(_fit(net, x, target, eye), _fit(net, x, target, None)), "S = I against scale = None"
    assert np.array_equal(siren.fit(net, _dev(x), _dev(target), _dev(eye), grads=False).cpu().numpy(),
                          siren.fit(net, _dev(x), _dev(target), grads=False).cpu().numpy())


# ---- 3. execution variants -------------------------------------------------------------------------------------
def _tile_bytes(H, L):
    return (2 * L + 1) * H * 4 * 32


@pytest.mark.parametrize("tiles", [1, 2])
def test_chunks_of_one_and_two_tiles(gpu, tiles):
    shape = (2, 32, 1, 2)
    x, target, S, (_, ref, ub), (_, t32) = _reference(*shape)
    net = _cuda_net(*shape)
    ws = tiles * _tile_bytes(32, 1) + 100  # 7 tiles in chunks of `tiles`; the slack must not buy another tile
    got = _fit(net, x, target, S, workspace_bytes=ws)
    bound, L64 = mm.loss_bound(siren.eval(net, _dev(x)).cpu().numpy(), target, S)
    assert abs(float(got[0]) - L64) <= bound, "the call's n, not the chunk's"
    vm.assert_grads_as_accurate(got[1], t32, ref, ub, f"chunks of {tiles}")
    assert same_bits(got, _fit(net, x, target, S, workspace_bytes=ws))
    only = siren.fit(net, _dev(x), _dev(target), _dev(S), grads=False, workspace_bytes=ws)
    assert same(only, got[0]), "loss only, chunked alike: the same bits"


def _c_net(p, ws, bs, ptr):
    n = p.n_hidden_layers + 2
    w = (C.c_void_p * n)(*[ptr(t) for t in ws])
    b = (C.c_void_p * n)(*[ptr(t) for t in bs])
    return _lib.SirenNet(p.d_in, p.d_out, p.hidden, p.n_hidden_layers, p.omega, w, b), (w, b)


def test_host_pointers_equal_device_pointers(gpu):
    shape, n = (3, 64, 1, 3), 45
    net = _cuda_net(*shape)
    x = sm.points(3, n)
    target, S = mm.problem(n, 3, seed=2)
    dev = host(siren.fit(net, _dev(x), _dev(target), _dev(S)))
    l_np, gw_np, gb_np = siren.fit(net, x, target, S)  # numpy in: the staged, blocking path
    assert isinstance(l_np, np.float32) and all(isinstance(a, np.ndarray) for a in gw_np + gb_np)
    assert same_bits((l_np, (gw_np, gb_np)), dev) and np.isfinite(l_np) and l_np > 0
    assert same(siren.fit(net, x, target, S, grads=False), dev[0])
    assert same(siren.fit(net, _dev(x), _dev(target), _dev(S), grads=False), dev[0])


@pytest.mark.parametrize("side", [False, True], ids=["current_stream", "side_stream"])
def test_determinism_loss_only_and_written_not_accumulated(gpu, side):
    shape, n = (3, 256, 3, 3), 193
    net = _cuda_net(*shape)
    x = _dev(sm.points(3, n))
    target, S = [_dev(a) for a in mm.problem(n, 3)]
    stream = torch.cuda.Stream() if side else None

    def run(**kw):
        out = siren.fit(net, x, target, S, stream=stream, **kw)
        if side:
            stream.synchronize()
        return out
    first = host(run())
    assert same_bits(first, host(run())), "two calls, the same bits"
    assert np.isfinite(first[0]) and first[0] > 0
    assert all(np.isfinite(a).all() and np.any(a) for a in first[1][0] + first[1][1])
    only = run(grads=False)
    assert torch.is_tensor(only) and only.shape == () and only.is_cuda
    assert same(only, first[0]), "the loss-only call returns the full call's loss bits"
    # the C ABI on buffers full of NaN: written, not accumulated; and loss only with both arrays NULL
    p = siren.pack(net)
    nl = shape[2] + 2
    gw = [torch.full_like(t, float("nan")) for t in p.weights]
    gb = [torch.full_like(t, float("nan")) for t in p.biases]
    loss = torch.full((1,), float("nan"), device="cuda")
    st, keep = _c_net(p, p.weights, p.biases, lambda t: t.data_ptr())
    pw = (C.c_void_p * nl)(*[t.data_ptr() for t in gw])
    pb = (C.c_void_p * nl)(*[t.data_ptr() for t in gb])
    torch.cuda.synchronize()
    s = stream.cuda_stream if side else None
    flags = _lib.WOS_PTRS_DEVICE | _lib.WOS_ASYNC | _lib.WOS_FIT_SCALE_MATRIX
    lib = _lib.load()
    rc = lib.wos_siren_fit(C.byref(st), x.data_ptr(), n, target.data_ptr(), S.data_ptr(), loss.data_ptr(), pw, pb, 0,
                           flags, gpu, s)
    assert rc == 0, lib.wos_last_error()
    torch.cuda.synchronize()
    assert same_bits(first, host((loss[0], gw, gb))), "NaN-filled buffers come back as the first call's bits"
    for t in gw + gb:
        t.fill_(5.0)
    loss.fill_(float("nan"))
    torch.cuda.synchronize()
    rc = lib.wos_siren_fit(C.byref(st), x.data_ptr(), n, target.data_ptr(), S.data_ptr(), loss.data_ptr(), None, None, 0,
                           flags, gpu, s)
    assert rc == 0, lib.wos_last_error()
    torch.cuda.synchronize()
    assert same(loss[0], first[0]) and all(bool((t == 5.0).all()) for t in gw + gb)


def test_fit_loss_takes_a_matrix(gpu):
    net = _cuda_net(2, 32, 1, 2).requires_grad_(True)
    lin = [m for m in net.net if isinstance(m, torch.nn.Linear)]
    params = [m.weight for m in lin] + [m.bias for m in lin]
    n = 70
    x = _dev(sm.points(2, n))
    target, S = [_dev(a) for a in mm.problem(n, 2, seed=1)]
    want_loss, gw, gb = siren.fit(net, x, target, S)
    loss = siren.fit_loss(net, x, target, S)
    assert loss.requires_grad and same(loss, want_loss)
    (3.0 * loss).backward()
    for t, g in zip(params, gw + gb):
        assert same(t.grad, 3.0 * g)
    with torch.no_grad():
        assert same(siren.fit_loss(net, x, target, S), want_loss)


# ---- 4. the loops ------------------------------------------------------------------------------------------------
SHAPE, N_POOL, BATCH, K = (2, 32, 1, 2), 100, 33, 3
COUNTS = [33, 1, 64]


def _pool(seed=3, n=N_POOL):
    x = torch.from_numpy(sm.points(2, n, seed=6)).cuda()
    target, S = mm.problem(n, 2, seed=seed)
    return x, torch.from_numpy(target).cuda(), torch.from_numpy(S).cuda()


def _idx(k=K, batch=BATCH):
    idx = torch.from_numpy(np.random.default_rng(100).integers(0, N_POOL, (k, batch))).to(torch.int64)
    idx[0, 0], idx[0, 1], idx[-1, -1] = 0, 0, N_POOL - 1  # both ends of the pool, and a duplicate
    return idx.contiguous().cuda()


def _separate_pool(net, state, pool, idx):
    """Gather, siren.fit and siren.adam_step made separately."""
    x, target, scale = pool
    losses = []
    for row in idx:
        loss, gw, gb = siren.fit(net, x[row], target[row], None if scale is None else scale[row])
        siren.adam_step(net, (gw, gb), state)
        losses.append(loss)
    return torch.stack(losses)


def _separate_rows(net, state, rows, counts):
    x, target, scale = rows
    losses, o = [], 0
    for c in counts:
        loss, gw, gb = siren.fit(net, x[o:o + c], target[o:o + c], None if scale is None else scale[o:o + c])
        siren.adam_step(net, (gw, gb), state)
        losses.append(loss)
        o += c
    return torch.stack(losses)


@pytest.mark.parametrize("clip", [None, 0.1], ids=["no_clip", "clip"])
def test_fit_run_equals_the_separate_calls(gpu, clip):
    pool, idx = _pool(), _idx()
    net_a, net_b = _cuda_net(*SHAPE), _cuda_net(*SHAPE)
    state_a, state_b = siren.AdamState(net_a, max_grad_norm=clip, **KW), siren.AdamState(net_b, max_grad_norm=clip, **KW)
    want = _separate_pool(net_a, state_a, pool, idx)
    losses, status = siren.fit_run(net_b, state_b, *pool, idx)
    assert losses.shape == (K,) and status.tolist() == [K, 0] and bool(torch.isfinite(losses).all())
    assert same(losses, want), f"losses {losses.tolist()} separate calls {want.tolist()}"
    _same_run(net_a, state_a, net_b, state_b, "fit_run with a matrix per point")
    assert any(not same(a, b) for a, b in zip(_tensors(net_b), _tensors(_cuda_net(*SHAPE)))), "the run moved the network"
    # not the diagonal of the matrices: the off-diagonal entries count
    net_c = _cuda_net(*SHAPE)
    diag = torch.diagonal(pool[2], dim1=-2, dim2=-1).contiguous()
    other, _ = siren.fit_run(net_c, siren.AdamState(net_c, max_grad_norm=clip, **KW), pool[0], pool[1], diag, idx)
    assert not same(other, losses)


@pytest.mark.parametrize("clip", [None, 0.1], ids=["no_clip", "clip"])
def test_fit_run_batches_equals_the_separate_calls_on_ragged_counts(gpu, clip):
    rows = _pool(seed=4, n=sum(COUNTS))
    net_a, net_b = _cuda_net(*SHAPE), _cuda_net(*SHAPE)
    state_a, state_b = siren.AdamState(net_a, max_grad_norm=clip, **KW), siren.AdamState(net_b, max_grad_norm=clip, **KW)
    want = _separate_rows(net_a, state_a, rows, COUNTS)
    losses, status = siren.fit_run_batches(net_b, state_b, *rows, COUNTS)
    assert losses.shape == (K,) and status.tolist() == [K, 0] and bool(torch.isfinite(losses).all())
    assert same(losses, want), f"losses {losses.tolist()} separate calls {want.tolist()}"
    _same_run(net_a, state_a, net_b, state_b, "fit_run_batches with a matrix per point")


def _ensemble_case(second):
    """Two members on one pool: member 0 has a matrix per point, member 1 no scale (`none`) or factors per
    component (`diagonal`).  Returns (x, targets, scales)."""
    x, t0, S0 = _pool(seed=5, n=max(N_POOL, sum(COUNTS)))
    t1, s1 = fm.problem(x.shape[0], 2, second == "diagonal", seed=9)
    return x, [t0, _dev(t1)], [S0, _dev(s1)]


@pytest.mark.parametrize("second", ["none", "diagonal"])
def test_the_ensemble_loops_equal_the_single_runs(gpu, second):
    x, targets, scales = _ensemble_case(second)
    idx = _idx()
    for form in ("pool", "rows"):
        nets_a, nets_b = [_cuda_net(*SHAPE, seed=e) for e in range(2)], [_cuda_net(*SHAPE, seed=e) for e in range(2)]
        states_a, states_b = [siren.AdamState(n, **KW) for n in nets_a], [siren.AdamState(n, **KW) for n in nets_b]
        if form == "pool":
            want = [siren.fit_run(nets_a[e], states_a[e], x[:N_POOL], targets[e][:N_POOL],
                                  None if scales[e] is None else scales[e][:N_POOL], idx)[0] for e in range(2)]
            losses, status = siren.fit_run_ensemble(nets_b, states_b, x[:N_POOL], [t[:N_POOL] for t in targets],
                                                    [None if s is None else s[:N_POOL] for s in scales], idx)
        else:
            total = sum(COUNTS)
            want = [siren.fit_run_batches(nets_a[e], states_a[e], x[:total], targets[e][:total],
                                          None if scales[e] is None else scales[e][:total], COUNTS)[0] for e in range(2)]
            losses, status = siren.fit_run_batches_ensemble(nets_b, states_b, x[:total], [t[:total] for t in targets],
                                                            [None if s is None else s[:total] for s in scales], COUNTS)
        assert losses.shape == (2, K) and status.tolist() == [[K, 0]] * 2, form
        for e in range(2):
            # member 1's single run takes the unscaled or the diagonal kernel, its ensemble run the matrix
            # kernel: without a scale the same code, as a diagonal matrix the same values
            assert np.array_equal(losses[e].cpu().numpy(), want[e].cpu().numpy()), (form, e, losses[e].tolist(), want[e].tolist())
            assert bool(torch.isfinite(losses[e]).all())
            if e == 0 or second == "none":
                assert same(losses[e], want[e])
                _same_run(nets_a[e], states_a[e], nets_b[e], states_b[e], f"{form}: member {e}")
            else:
                for a, b in zip(_tensors(nets_a[e]) + [states_a[e].exp_avg, states_a[e].exp_avg_sq],
                                _tensors(nets_b[e]) + [states_b[e].exp_avg, states_b[e].exp_avg_sq]):
                    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), f"{form}: member {e}"


def test_full_and_unscaled_members_through_the_c_abi(gpu):
    """The flag covers the member that has a scale; the NULL entry is still the identity."""
    x, targets, scales = _ensemble_case("none")
    x, targets, S0 = x[:N_POOL].contiguous(), [t[:N_POOL].contiguous() for t in targets], scales[0][:N_POOL].contiguous()
    idx = _idx()
    nets_a, nets_b = [_cuda_net(*SHAPE, seed=e) for e in range(2)], [_cuda_net(*SHAPE, seed=e) for e in range(2)]
    states_a, states_b = [siren.AdamState(n, **KW) for n in nets_a], [siren.AdamState(n, **KW) for n in nets_b]
    want = [siren.fit_run(nets_a[0], states_a[0], x, targets[0], S0, idx)[0],
            siren.fit_run(nets_a[1], states_a[1], x, targets[1], None, idx)[0]]
    lib = _lib.load()
    structs = [_c_net(siren.pack(n), siren.pack(n).weights, siren.pack(n).biases, lambda t: t.data_ptr()) for n in nets_b]
    nets = (_lib.SirenNet * 2)(*[s for s, _ in structs])
    ts = (C.c_void_p * 2)(*[t.data_ptr() for t in targets])
    ss = (C.c_void_p * 2)(S0.data_ptr(), None)
    ms = (C.c_void_p * 2)(*[s.exp_avg.data_ptr() for s in states_b])
    vs = (C.c_void_p * 2)(*[s.exp_avg_sq.data_ptr() for s in states_b])
    losses = torch.zeros(2, K, device="cuda")
    status = torch.full((2, 2), 9, dtype=torch.int64, device="cuda")
    opt = states_b[0].params()
    torch.cuda.synchronize()
    rc = lib.wos_siren_fit_run_ensemble(2, nets, x.data_ptr(), ts, ss, N_POOL, idx.data_ptr(), K, BATCH, ms, vs, 0, C.byref(opt),
                                        -1.0, 0, losses.data_ptr(), status.data_ptr(), 0,
                                        _lib.WOS_PTRS_DEVICE | _lib.WOS_FIT_SCALE_MATRIX, gpu, None)
    assert rc == 0, lib.wos_last_error()
    assert status.tolist() == [[K, 0]] * 2
    for e in range(2):
        states_b[e].step = K
        assert same(losses[e], want[e]), (e, losses[e].tolist(), want[e].tolist())
        _same_run(nets_a[e], states_a[e], nets_b[e], states_b[e], f"member {e}")


def test_early_stop_with_one_member_frozen(gpu):
    x, targets, scales = _ensemble_case("none")
    x, targets, scales = x[:N_POOL], [targets[0][:N_POOL], 0.01 * targets[1][:N_POOL]], [scales[0][:N_POOL], None]
    idx = _idx()
    nets_a, nets_b = [_cuda_net(*SHAPE, seed=e) for e in range(2)], [_cuda_net(*SHAPE, seed=e) for e in range(2)]
    states_a, states_b = [siren.AdamState(n, **KW) for n in nets_a], [siren.AdamState(n, **KW) for n in nets_b]
    free = [siren.fit_run(_cuda_net(*SHAPE, seed=e), siren.AdamState(nets_a[e], **KW), x, targets[e], scales[e], idx)[0]
            for e in range(2)]
    stop = float(np.sqrt(float(free[0].min()) * float(free[1][0])))
    assert float(free[1][0]) < stop < float(free[0].min()), "the case: member 1 stops at once, member 0 never"
    want = [siren.fit_run(nets_a[e], states_a[e], x, targets[e], scales[e], idx, stop_loss=stop) for e in range(2)]
    losses, status = siren.fit_run_ensemble(nets_b, states_b, x, targets, scales, idx, stop_loss=stop)
    assert status.tolist() == [[K, 0], [1, 0]] and [s.step for s in states_b] == [K, 1]
    assert bool(torch.isfinite(losses[0]).all()) and bool(torch.isnan(losses[1, 1:]).all())
    for e in range(2):
        assert want[e][1].tolist() == status[e].tolist()
        assert same(losses[e], want[e][0]), (e, losses[e].tolist(), want[e][0].tolist())
        _same_run(nets_a[e], states_a[e], nets_b[e], states_b[e], f"member {e}")


# ---- 5. refusals ---------------------------------------------------------------------------------------------------
def test_bad_scale_shapes_are_named_before_any_device_work(gpu):
    net = _cuda_net(*SHAPE)
    before = [t.clone() for t in _tensors(net)]
    state = siren.AdamState(net, **KW)
    x, target, S = _pool()
    idx = _idx()
    both = r"must have shape \(100, 2\) \(a factor per component\) or \(100, 2, 2\) \(a matrix per point\), got "
    for bad in (S[:, :, :1], S[:, :1], S[:99], S.reshape(N_POOL, 4), torch.ones(N_POOL, 2, 2, 2, device="cuda")):
        got = str(tuple(bad.shape)).replace("(", r"\(").replace(")", r"\)")
        with pytest.raises(ValueError, match="siren.fit: scale " + both + got):
            siren.fit(net, x, target, bad)
        with pytest.raises(ValueError, match="siren.fit_run: pool_scale " + both + got):
            siren.fit_run(net, state, x, target, bad, idx)
        with pytest.raises(ValueError, match="siren.fit_run_batches: scale " + both + got):
            siren.fit_run_batches(net, state, x, target, bad, [33, 67])
        with pytest.raises(ValueError, match=r"siren.fit_run_ensemble: pool_scales\[1\] " + both + got):
            siren.fit_run_ensemble([net, _cuda_net(*SHAPE, seed=1)], [state, siren.AdamState(net, **KW)], x, [target, target],
                                   [S, bad], idx)
        with pytest.raises(ValueError, match=r"siren.fit_run_batches_ensemble: scales\[0\] " + both + got):
            siren.fit_run_batches_ensemble([net, _cuda_net(*SHAPE, seed=1)], [state, siren.AdamState(net, **KW)], x,
                                           [target, target], [bad, None], [33, 67])
    with pytest.raises(ValueError, match="scale must be a tensor on cuda"):
        siren.fit(net, x, target, S.cpu())
    assert state.step == 0 and all(same(a, b) for a, b in zip(before, _tensors(net))), "a refused call moved nothing"
    # the flag with a NULL scale, device pointers
    lib = _lib.load()
    p = siren.pack(net)
    st, keep = _c_net(p, p.weights, p.biases, lambda t: t.data_ptr())
    loss = torch.full((1,), 7.0, device="cuda")
    torch.cuda.synchronize()
    rc = lib.wos_siren_fit(C.byref(st), x.data_ptr(), N_POOL, target.data_ptr(), None, loss.data_ptr(), None, None, 0,
                           _lib.WOS_PTRS_DEVICE | _lib.WOS_FIT_SCALE_MATRIX, gpu, None)
    assert rc == -1 and b"null scale with WOS_FIT_SCALE_MATRIX" in lib.wos_last_error()
    torch.cuda.synchronize()
    assert float(loss) == 7.0, "a refused call wrote nothing"


# ---- 7. end to end ---------------------------------------------------------------------------------------------------
CENTRE, RADIUS, EPS = (0.7, 0.5), 0.2, 0.25


def circle_normal(x):
    r = x - torch.as_tensor(CENTRE, dtype=x.dtype, device=x.device)
    return r / torch.sqrt((r * r).sum(-1, keepdim=True))


def circle_weight(x):
    r = x - torch.as_tensor(CENTRE, dtype=x.dtype, device=x.device)
    return ((torch.sqrt((r * r).sum(-1)) - RADIUS) / EPS).clamp(min=0, max=1)


@functools.lru_cache(maxsize=None)
def _karman():
    cfg = workloads.karman_config(n_walks=16, n_points=200)
    scene_cfg = dict(workloads.SCENE_BASE, boundary=workloads.KARMAN_OBJ)
    samples = torch.from_numpy(cfg["points"]).cuda()
    proj = pj.PressureProjector(scene_cfg, cfg["solver"], cfg["output"], samples)
    return proj, samples, [float(v) for v in workloads.scene_size(workloads.KARMAN_OBJ)]


def _params(net):
    lin = [m for m in net.net if isinstance(m, torch.nn.Linear)]
    return [m.weight for m in lin] + [m.bias for m in lin]


def _end_to_end(net, x, wrap, target64, target32, run_fit, run_torch, what):
    """The fit route against a float64 evaluation of the same formula at the same points x, as
    tests/test_gpu_siren_fit.py does for the diagonal wraps: the loss within the fit step's bound plus the
    forward's and the target's measured errors propagated, the gradients by the project's yardstick with
    the seed S^T (2 r) / N."""
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
    t64 = target64(x64)
    u64 = net64(x64)
    w64 = wrap(x64, u64)
    L64 = torch.mean((w64 - t64) ** 2)
    ref = [g.numpy() for g in torch.autograd.grad(L64, _params(net64))]
    L64 = float(L64.detach())
    with torch.no_grad():
        w32 = wrap(x, siren.eval(net, x))
        du = float((w32.cpu().double() - w64.detach()).abs().max())
        dt = float((target32().cpu().double() - t64).abs().max())
    bound = fm.loss_bound(t64.numel(), L64) + 2.0 * np.sqrt(L64) * (du + dt)
    print(f"{what}: loss {loss_c:.9e} torch f32 {loss_a:.9e} float64 {L64:.9e} error {abs(loss_c - L64):.3e} "
          f"bound {bound:.3e} (du {du:.3e} dt {dt:.3e})")
    assert abs(loss_c - L64) <= bound
    nl = len(params) // 2
    S64, _, mixes = siren.affine_wrap(wrap, x64, 2)
    assert mixes
    ub = (S64.transpose(-1, -2) @ (2.0 * (w64.detach() - t64) / t64.numel()).unsqueeze(-1)).squeeze(-1).numpy()
    vm.assert_grads_as_accurate((g_c[:nl], g_c[nl:]), (g_a[:nl], g_a[nl:]), (ref[:nl], ref[nl:]), ub, what)
    assert all(np.any(a) for a in g_c)


def test_projection_fit_loss_through_a_slip_wrap(gpu):
    proj, samples, size = _karman()
    net, net_prev = _cuda_net(2, 128, 2).requires_grad_(True), _cuda_net(2, 128, 2, seed=1)
    wrap = pj.slip_wrap(circle_normal, circle_weight)
    w = circle_weight(samples)
    assert int((w == 0).sum()) > 0 and int((w == 1).sum()) > 0 and int(((w > 0) & (w < 1)).sum()) > 0, "the case"
    grad_p = torch.from_numpy(np.random.default_rng(11).standard_normal((200, 2)).astype(np.float32) * 0.1).cuda()
    n_samples = 256
    gen = lambda: torch.Generator(device="cuda").manual_seed(77)  # noqa: E731
    idx = torch.randint(0, 199, (n_samples,), device="cuda", generator=gen())
    x = samples[idx]
    prev64 = vm.net64(net_prev)

    def target64(x64):
        with torch.no_grad():
            return wrap(x64, prev64(x64)) - grad_p[idx].cpu().double()
    _end_to_end(net, x, wrap, target64, lambda: wrap(x, siren.eval(net_prev, x)) - grad_p[idx],
                lambda: proj.projection_fit_loss(net, net_prev, grad_p, n_samples, wrap=wrap, generator=gen()),
                lambda: proj.projection_loss(lambda q: wrap(q, net(q)), lambda q: wrap(q, net_prev(q)), grad_p, n_samples,
                                             generator=gen()),
                "projection (slip wrap)")


@pytest.mark.parametrize("tilde", [False, True], ids=["prev", "two_prev_minus_tilde"])
def test_advection_fit_loss_through_a_slip_wrap(gpu, tilde):
    proj, samples, size = _karman()
    net, net_prev = _cuda_net(2, 128, 2).requires_grad_(True), _cuda_net(2, 128, 2, seed=1)
    net_tilde = _cuda_net(2, 128, 2, seed=2) if tilde else None
    wrap = pj.slip_wrap(circle_normal, circle_weight)
    x, dt = samples, 0.05

    def formula(nets, q):  # _advect_velocity's target, in q's dtype
        with torch.no_grad():
            back = q - wrap(q, nets[0](q)) * dt
            back = torch.stack([back[..., 0].clamp(min=size[0], max=size[1]), back[..., 1].clamp(min=size[2], max=size[3])], -1)
            t = wrap(back, nets[0](back))
            return 2 * t - wrap(back, nets[1](back)) if tilde else t
    nets64 = (vm.net64(net_prev), vm.net64(net_tilde) if tilde else None)
    _end_to_end(net, x, wrap, lambda x64: formula(nets64, x64),
                lambda: formula((lambda q: siren.eval(net_prev, q), lambda q: siren.eval(net_tilde, q)), x),
                lambda: pj.advection_fit_loss(net, net_prev, x, dt, size, network_tilde=net_tilde, wrap=wrap),
                lambda: torch.mean((wrap(x, net(x)) - formula((net_prev, net_tilde), x)) ** 2),
                f"advection (slip wrap, {'tilde' if tilde else 'prev'})")


def _step_from_grad(net, state):
    """siren.adam_step on the gradients a backward left in .grad, which are then cleared."""
    params = _params(net)
    nl = len(params) // 2
    grads = [t.grad for t in params]
    siren.adam_step(net, (grads[:nl], grads[nl:]), state)
    for t in params:
        t.grad = None


def test_fit_projection_through_a_slip_wrap_equals_the_per_iteration_calls(gpu):
    proj, samples, size = _karman()
    wrap = pj.slip_wrap(circle_normal, circle_weight)
    net_prev = _cuda_net(2, 64, 1, seed=1)
    grad_p = torch.from_numpy(np.random.default_rng(11).standard_normal((200, 2)).astype(np.float32) * 0.1).cuda()
    n_samples, n_iters = 193, 3
    g1, g2 = [torch.Generator(device="cuda").manual_seed(77) for _ in range(2)]
    net_a, net_b = _cuda_net(2, 64, 1).requires_grad_(True), _cuda_net(2, 64, 1)
    state_a = siren.AdamState(net_a, lr=1e-4)
    want = []
    for _ in range(n_iters):
        loss = proj.projection_fit_loss(net_a, net_prev, grad_p, n_samples, wrap=wrap, generator=g1)
        loss.backward()
        _step_from_grad(net_a, state_a)
        want.append(loss.detach())
    losses, state_b = proj.fit_projection(net_b, net_prev, grad_p, n_samples, n_iters, wrap=wrap, generator=g2, iters_per_call=2)
    assert losses.shape == (n_iters,) and bool(torch.isfinite(losses).all()) and state_b.step == n_iters
    assert torch.equal(g1.get_state(), g2.get_state()), "the generator consumption of the loop"
    assert same(losses, torch.stack(want)), f"losses {losses.tolist()} per-iteration {[float(v) for v in want]}"
    _same_run(net_a, state_a, net_b, state_b, "fit_projection against projection_fit_loss, backward and adam_step")


def test_fit_advection_through_a_slip_wrap_equals_the_per_iteration_calls(gpu):
    proj, samples, size = _karman()
    wrap = pj.slip_wrap(circle_normal, circle_weight)
    net_prev = _cuda_net(2, 64, 1, seed=1)
    keep = lambda q: circle_weight(q) > 0  # noqa: E731 (the points outside the circle: ragged counts)
    n_samples, n_iters, dt = 193, 3, 0.05
    g1, g2 = [torch.Generator(device="cuda").manual_seed(77) for _ in range(2)]
    net_a, net_b = _cuda_net(2, 64, 1).requires_grad_(True), _cuda_net(2, 64, 1)
    state_a = siren.AdamState(net_a, lr=1e-4)
    want, counts = [], []
    for _ in range(n_iters):
        x = torch.rand(n_samples, 2, device="cuda", generator=g1)
        for c in range(2):
            x[..., c] = x[..., c] * (size[2 * c + 1] - size[2 * c]) + size[2 * c]
        x = x[keep(x)]
        loss = pj.advection_fit_loss(net_a, net_prev, x, dt, size, wrap=wrap)
        loss.backward()
        _step_from_grad(net_a, state_a)
        want.append(loss.detach())
        counts.append(int(x.shape[0]))
    assert len(set(counts)) >= 2 and all(0 < c < n_samples for c in counts), f"the case: ragged counts, got {counts}"
    losses, state_b = pj.fit_advection(net_b, net_prev, dt, size, n_iters, n_samples=n_samples, wrap=wrap, keep=keep,
                                       generator=g2, iters_per_call=2)
    assert losses.shape == (n_iters,) and bool(torch.isfinite(losses).all()) and state_b.step == n_iters
    assert torch.equal(g1.get_state(), g2.get_state()), "the generator consumption of the loop"
    assert same(losses, torch.stack(want)), f"losses {losses.tolist()} per-iteration {[float(v) for v in want]}"
    _same_run(net_a, state_a, net_b, state_b, "fit_advection against advection_fit_loss, backward and adam_step")


def test_the_ensemble_time_stepper_loops_take_a_slip_wrap_beside_a_diagonal_one(gpu):
    proj, samples, size = _karman()
    box = [samples[:, 0].min().item(), samples[:, 0].max().item(), samples[:, 1].min().item(), samples[:, 1].max().item()]
    wraps = [pj.slip_wrap(circle_normal, circle_weight), sm.karman_wrap(box, eps=0.125)]
    prevs = [_cuda_net(2, 64, 1, seed=3 + e) for e in range(2)]
    grad_p = torch.from_numpy(np.random.default_rng(12).standard_normal((2, 200, 2)).astype(np.float32) * 0.1).cuda()
    gen = lambda: torch.Generator(device="cuda").manual_seed(5)  # noqa: E731
    nets_a, nets_b = [_cuda_net(2, 64, 1, seed=e) for e in range(2)], [_cuda_net(2, 64, 1, seed=e) for e in range(2)]
    want = [proj.fit_projection(nets_a[e], prevs[e], grad_p[e], 65, 3, wrap=wraps[e], generator=gen())[0] for e in range(2)]
    losses, _ = proj.fit_projection_ensemble(nets_b, prevs, grad_p, 65, 3, wraps=wraps, generator=gen())
    for e in range(2):
        assert np.array_equal(losses[e].cpu().numpy(), want[e].cpu().numpy()), (e, losses[e].tolist(), want[e].tolist())
        for a, b in zip(_tensors(nets_a[e]), _tensors(nets_b[e])):
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), f"projection: member {e}"
    nets_a, nets_b = [_cuda_net(2, 64, 1, seed=e) for e in range(2)], [_cuda_net(2, 64, 1, seed=e) for e in range(2)]
    want = [pj.fit_advection(nets_a[e], prevs[e], 0.05, size, 3, n_samples=65, wrap=wraps[e], generator=gen())[0]
            for e in range(2)]
    losses, _ = pj.fit_advection_ensemble(nets_b, prevs, 0.05, size, 3, n_samples=65, wraps=wraps, generator=gen())
    for e in range(2):
        assert np.array_equal(losses[e].cpu().numpy(), want[e].cpu().numpy()), (e, losses[e].tolist(), want[e].tolist())
        for a, b in zip(_tensors(nets_a[e]), _tensors(nets_b[e])):
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), f"advection: member {e}"
