"""Device-resident pressure projection: the callers on either side of the walk-on-stars
path, kept on the GPU.

The reference's projection step, per time step (src/2d/models/model_split.py:185-283;
3D: src/3d/models/model_split.py:190-316):
  * get_divergence: grid = sample_uniform_2D(vis_resolution, with_boundary=True)
    (src/2d/utils/model_utils.py:3-20), u = query_velocity(grid) (the SIREN,
    src/2d/models/networks.py:14-68), div = divergence(u, grid)
    (src/2d/utils/diff_ops.py:45-51), then -div[..., 0].detach().cpu().numpy();
  * wost_pressure: Scene(sceneConfig, div) + wost(scene, solver, output,
    pressure_samples.detach().cpu().numpy()) -> nested lists -> numpy;
  * _project_velocity: grad_p = torch.Tensor(grad_p).to(device), then on random
    samples target = u_prev - grad_p[idx], loss = mean((u - target)^2).
Here the divergence grid stays a CUDA tensor and reaches the engine by device
pointer (wos_scene_set_source: one device-to-device copy, the geometry stays
resident), the pressure samples stay a CUDA tensor, and grad p comes back as a CUDA
tensor that the loss indexes in place -- no host round trip anywhere.  The SIREN runs
in PyTorch-ROCm: its Linear layers are the dense contractions (hipBLASLt / MFMA).  For the
source alone there is a second path without autograd: source_from_network evaluates the
network and its divergence in the fused forward-mode kernel of wos_amd.siren.
"""
import weakref

import numpy as np
import torch
import torch.nn as nn

from . import engine as _engine
from . import siren as _siren


class Sine(nn.Module):
    """sin(30 x) (networks.py:15-21)."""

    def forward(self, x):
        return torch.sin(30.0 * x)


class Siren(nn.Module):
    """The reference's MLP with sine nonlinearity (networks.py:25-68) and its
    initialisation (sine_init / first_layer_sine_init, networks.py:78-90)."""

    def __init__(self, in_features, out_features, num_hidden_layers, hidden_features):
        super().__init__()
        layers = [nn.Linear(in_features, hidden_features), Sine()]
        for _ in range(num_hidden_layers):
            layers += [nn.Linear(hidden_features, hidden_features), Sine()]
        layers.append(nn.Linear(hidden_features, out_features))
        self.net = nn.Sequential(*layers)
        with torch.no_grad():
            for m in self.net:
                if isinstance(m, nn.Linear):
                    n = m.weight.size(-1)
                    m.weight.uniform_(-np.sqrt(6 / n) / 30, np.sqrt(6 / n) / 30)
            first = self.net[0]
            first.weight.uniform_(-1 / in_features, 1 / in_features)

    def forward(self, coords):
        return self.net(coords)


def sample_uniform_2d(resolution, size, with_boundary=True, device="cpu"):
    """sample_uniform_2D (src/2d/utils/model_utils.py:3-20): cell centres of a grid
    over size = (x0, x1, y0, y1) with `resolution` cells along the longer side, plus
    the boundary rows/columns; meshgrid 'xy' -> shape (res_y [+2], res_x [+2], 2)."""
    if (size[1] - size[0]) > (size[3] - size[2]):
        res_x, res_y = resolution, int(resolution * (size[3] - size[2]) / (size[1] - size[0]))
    else:
        res_x, res_y = int(resolution * (size[1] - size[0]) / (size[3] - size[2])), resolution
    x = torch.linspace(0.5, res_x - 0.5, res_x, device=device)
    y = torch.linspace(0.5, res_y - 0.5, res_y, device=device)
    if with_boundary:
        x = torch.cat([torch.zeros(1, device=device), x, torch.full((1,), float(res_x), device=device)])
        y = torch.cat([torch.zeros(1, device=device), y, torch.full((1,), float(res_y), device=device)])
    coords = torch.stack(torch.meshgrid(x, y, indexing="xy"), dim=-1)
    coords[..., 0] = coords[..., 0] / res_x * (size[1] - size[0]) + size[0]
    coords[..., 1] = coords[..., 1] / res_y * (size[3] - size[2]) + size[2]
    return coords


def sample_uniform_3d(resolution, size, with_boundary=True, device="cpu"):
    """The 3D sampler (src/3d/utils/model_utils.py:3-29, named sample_uniform_2D there):
    `resolution` cells along the shortest side, meshgrid 'ij' -> (X, Y, Z, 3).  The
    reference builds the z axis with res_y points (model_utils.py:17); kept."""
    ex, ey, ez = size[1] - size[0], size[3] - size[2], size[5] - size[4]
    if ex < ey:
        if ex < ez:
            res = (resolution, int(resolution * ey / ex), int(resolution * ez / ex))
        else:
            res = (int(resolution * ex / ez), int(resolution * ey / ez), resolution)
    else:
        if ey < ez:
            res = (int(resolution * ex / ey), resolution, int(resolution * ez / ey))
        else:
            res = (int(resolution * ex / ez), int(resolution * ey / ez), resolution)
    rx, ry, rz = res
    axes = [torch.linspace(0.5, rx - 0.5, rx, device=device), torch.linspace(0.5, ry - 0.5, ry, device=device),
            torch.linspace(0.5, rz - 0.5, ry, device=device)]
    if with_boundary:
        axes = [torch.cat([torch.zeros(1, device=device), a, torch.full((1,), float(r), device=device)])
                for a, r in zip(axes, res)]
    coords = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1)
    for k in range(3):
        coords[..., k] = coords[..., k] / res[k] * (size[2 * k + 1] - size[2 * k]) + size[2 * k]
    return coords


def divergence(y, x, create_graph=False):
    """sum_i d y_i / d x_i by autograd (diff_ops.py:45-51)."""
    div = 0.0
    for i in range(y.shape[-1]):
        g = torch.autograd.grad(y[..., i], x, torch.ones_like(y[..., i]), create_graph=create_graph,
                                retain_graph=True)[0]
        div = div + g[..., i:i + 1]
    return div


class _MeshDistance(torch.autograd.Function):
    """sign * signed_dist of WosScene.query as a once-differentiable function of the points."""

    @staticmethod
    def forward(ctx, x, scene, sign):
        xq = x.detach().to(torch.float32).contiguous()
        dist, sd, _, cp = scene.query(xq, which="neumann", closest=True)
        # a host scene (CPU tensors in) answers in numpy
        dist, sd, cp = (torch.as_tensor(a).to(xq.device) for a in (dist, sd, cp))
        out = sd if sign > 0 else -sd
        ctx.save_for_backward(xq, cp, dist, out)
        ctx.dtype = x.dtype
        return out.to(x.dtype)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        xq, cp, dist, out = ctx.saved_tensors
        r = xq - cp
        nrm = torch.sqrt((r * r).sum(-1, keepdim=True))
        on = (dist == 0)[:, None] | (nrm == 0)
        direction = torch.where(on, torch.zeros_like(r), r / torch.where(on, torch.ones_like(nrm), nrm))
        # |value| grows along (x - closest): d value / dx = sgn(value) (x - closest) / |x - closest|
        g = grad_out.to(torch.float32)[:, None] * torch.sign(out)[:, None] * direction
        return g.to(ctx.dtype), None, None


class MeshSDF:
    """The signed distance to a scene's boundary mesh as a device function with the signature of
    the reference's obs_sdf_func (src/2d/models/base.py:239-241, 352-358): samples [..., dim] ->
    distances [...], on the samples' device, with no host synchronisation.  It replaces
    obstacle_function(v, l) (src/2d/sources.py:102-119: gpytoolbox on the host per call, no
    gradient) for any OBJ outline.

        sdf = MeshSDF(scene, positive="outside")      # scene: a WosScene or a zombie_bindings.Scene
        dist = sdf(samples); samples = samples[dist > 0]

    The value is WosScene.query's signed_dist, the solver's own: negative on the domain side.
    positive="inside" returns -signed_dist (positive in the domain the solver estimates in),
    positive="outside" +signed_dist (for an obstacle mesh whose domain side is the obstacle's
    interior this is the reference's convention: positive in the fluid).
    Once differentiable: d value / dx = sgn(value) (x - closest) / |x - closest|, and 0 where the
    distance is 0, so the grad(w) . u term of divergence(query_velocity(grid), grid) behaves as
    with an analytic SDF.  Second derivatives are not provided: the backward is
    once_differentiable, and source_from_velocity(create_graph=True) through a MeshSDF raises."""

    def __init__(self, scene, positive="inside"):
        if positive not in ("inside", "outside"):
            raise ValueError(f"MeshSDF: positive must be 'inside' or 'outside', got {positive!r}")
        self.scene = getattr(scene, "_scene", scene)
        self.positive = positive
        self.dim = int(self.scene.dim)

    def __call__(self, samples):
        if samples.shape[-1] != self.dim:
            raise ValueError(f"MeshSDF: samples must be [..., {self.dim}], got shape {tuple(samples.shape)}")
        out = _MeshDistance.apply(samples.reshape(-1, self.dim), self.scene, 1 if self.positive == "outside" else -1)
        return out.reshape(samples.shape[:-1])


class _TapeProjection(torch.autograd.Function):
    """solve(div) of a PressureProjector with reuse_walks as a differentiable function of div:
    forward is the source replacement plus the replay, backward the tape's transpose
    (WalkTape.vjp; over the tape's cell-sorted index, bit for bit reproducible, with the
    projector's deterministic_backward).  The variance outputs are not differentiable."""

    @staticmethod
    def forward(ctx, div, proj, variance):
        proj._set_source(div.detach())
        *out, st = proj._replay_points(proj.samples, 0, 1, **({"variance": True} if variance else {}))
        proj.last_stats = st
        ctx.tape, ctx.shape, ctx.dtype = proj._tape, tuple(div.shape), div.dtype
        ctx.deterministic = proj.deterministic_backward
        if variance:
            ctx.mark_non_differentiable(out[2], out[3])
        return tuple(out)

    @staticmethod
    def backward(ctx, grad_p, grad_g, *unused):
        if ctx.tape._h is None:
            raise RuntimeError("the projector recorded a new tape (another source grid) before backward()")
        if tuple(ctx.tape.scene.source_shape) != ctx.shape:
            raise RuntimeError("the projector's source grid changed shape before backward()")
        return ctx.tape.vjp(grad_p, grad_g, deterministic=ctx.deterministic).to(ctx.dtype), None, None


class PressureProjector:
    """One scene for the whole simulation; each projection replaces its source in
    place and solves at the (device-resident) pressure samples.

        proj = PressureProjector(wost_json["scene"], wost_json["solver"], wost_json["output"],
                                 pressure_samples_cuda)
        div = proj.source_from_velocity(u_prev, vis_resolution, scene_size)
        p, grad_p = proj.solve(div)
        loss = proj.projection_loss(u, u_prev, grad_p, n)

    Multi-GPU (one process per GPU): pass the process group
    (`group=torch.distributed.group.WORLD` after init_process_group("nccl")).  Every
    rank holds the same pressure samples; rank r solves the stride shard r, r + W, ...
    keyed by GLOBAL sample index, and ONE all_gather_into_tensor of [p, grad p] (RCCL
    over xGMI) hands every rank the full field -- bit-identical to a one-GPU solve, so
    projection_loss draws from it unchanged.  `force_gather` runs the collective even in
    a world of one.

    reuse_walks=True: the walks do not depend on the source, so the first solve(div) records
    this rank's walks (WosScene.record, at global indices with a group) and every later one
    replays them for the new div (WalkTape.solve) -- outputs bit-identical to
    reuse_walks=False at a fraction of the time.  The noise is frozen as the fixed seed already
    freezes it; a div of another grid shape records anew.

    solve(div, differentiable=True) (reuse_walks=True, no group) returns p and grad_p attached to
    div's autograd graph: backward applies the transpose of the recorded walks' affine map
    (WalkTape.vjp), so a loss on p / grad_p reaches whatever produced div --
    source_from_velocity(..., create_graph=True) keeps that graph down to the network's weights.
    deterministic_backward=True: that backward sums in a fixed order without atomics
    (WalkTape.vjp(deterministic=True); the tape's index is built at the first backward), so two
    backward passes give the same bits and a training run can be replayed.
    """

    # class-level defaults: a subclass that builds its own scene keeps the plain path
    reuse_walks = False
    deterministic_backward = False
    _tape, _tape_grid = None, None

    def __init__(self, scene_config, solver_config, output_config, pressure_samples, device=None,
                 group=None, force_gather=False, reuse_walks=False, deterministic_backward=False):
        import zombie_bindings  # the drop-in shim parses the reference's scene keys
        self.dim = int(pressure_samples.shape[-1])
        self.device = pressure_samples.device if device is None else torch.device(device)
        placeholder = torch.zeros((2,) * self.dim, dtype=torch.float32, device=self.device)
        self.scene = zombie_bindings.Scene(dict(scene_config), placeholder, device=self.device.index or 0)
        self.params = _engine.solver_params(solver_config, output_config)
        self.samples = pressure_samples.detach().to(self.device, torch.float32).contiguous()
        self.group, self.force_gather = group, force_gather
        self.last_stats = None
        self.reuse_walks = bool(reuse_walks)
        self.deterministic_backward = bool(deterministic_backward)
        self._tape, self._tape_grid = None, None

    def source_from_velocity(self, velocity_fn, resolution, size, create_graph=False):
        """-div u on the reference's grid (get_divergence, model_split.py:230-236),
        computed and kept on the device.  create_graph=True keeps the autograd graph instead of
        detaching, so a loss behind solve(div, differentiable=True) reaches velocity_fn's weights."""
        sampler = sample_uniform_2d if self.dim == 2 else sample_uniform_3d
        grid = sampler(resolution, size, with_boundary=True, device=self.device).requires_grad_(True)
        u = velocity_fn(grid)
        if create_graph:
            return (-divergence(u, grid, create_graph=True)[..., 0]).contiguous()
        div = divergence(u, grid)
        return (-div[..., 0]).detach().contiguous()

    def source_from_network(self, network, resolution, size, wrap=None, differentiable=False):
        """source_from_velocity for a velocity that is the SIREN itself, through the fused forward-mode
        kernel (wos_amd.siren.eval) instead of autograd: the same grid, the same shape, dtype and
        sign, detached and contiguous, ready for solve(div).  `network`: a Siren, the reference's MLP
        or their .net (siren.pack).  wrap=None: div = trace J straight from the kernel.
        wrap(x, u_net) -> u: the time-stepper's pointwise masks and weights around the network
        (query_velocity, src/2d/models/base.py:158-180); the kernel returns the network's value and
        Jacobian and siren.divergence_with_wrap applies the chain rule through `wrap` alone.
        differentiable=True: the same bits, attached to the network's parameters (wos_amd.siren.apply;
        with a wrap through its elementwise graph as well), so solve(div, differentiable=True) and
        loss.backward() fill network.parameters()' .grad through the fused backward kernel
        (wos_amd.siren.vjp) with no autograd graph over the network."""
        sampler = sample_uniform_2d if self.dim == 2 else sample_uniform_3d
        grid = sampler(resolution, size, with_boundary=True, device=self.device)
        if differentiable:
            if wrap is None:
                return (-_siren.apply(network, grid, value=False, divergence=True)).contiguous()
            u, jac = _siren.apply(network, grid, value=True, jacobian=True)
            return (-_siren.divergence_with_wrap(grid, u, jac, wrap, create_graph=True)).contiguous()
        if wrap is None:
            return (-_siren.eval(network, grid, value=False, divergence=True)).contiguous()
        u, jac = _siren.eval(network, grid, value=True, jacobian=True)
        return (-_siren.divergence_with_wrap(grid, u, jac, wrap)).contiguous()

    def sample_state(self, pts=None):
        """The state words solve() will give the pressure samples, or `pts` [N, dim]
        (WosScene.query_state with this projector's scene and boundaryDistanceMask): int32 [N],
        bit 0 estimated, bit 1 p masked, bit 2 grad p masked, bit 3 inside the domain.  A masked
        sample comes back as grad_p = 0 and projection_loss then trains on target = u_prev there;
        with this a caller can draw or filter samples the solve estimates and does not mask:
        keep = (state & 5) == 1."""
        x = self.samples if pts is None else pts
        return self.scene._scene.query_state(x, self.params.boundary_distance_mask)

    def _set_source(self, div):
        self.scene._scene.set_source(div)

    def _solve_points(self, x, index_base, index_stride, variance=False):
        if not variance:
            return self.scene._scene.solve(x, self.params, index_base=index_base, index_stride=index_stride)
        return self.scene._scene.solve(x, self.params, index_base=index_base, index_stride=index_stride,
                                       variance=True)

    def _replay_points(self, x, index_base, index_stride, variance=False):
        """_solve_points through the walk tape of (x, index_base, index_stride): recorded on first use."""
        grid = tuple(self.scene._scene.source_shape[-self.dim:])
        if self._tape is not None and self._tape_grid != grid:
            self._tape.close()
            self._tape = None
        if self._tape is None:
            self._tape = self.scene._scene.record(x, self.params, index_base=index_base, index_stride=index_stride)
            self._tape_grid = grid
        return self._tape.solve(variance=variance)

    def solve(self, div, variance=False, differentiable=False):
        """wost_pressure (model_split.py:185-202) with device tensors in and out; with a
        process group, this rank's stride shard + one all-gather (wos_amd.dist).
        variance=True: (p, grad_p, p_var, grad_var) -- the per-walk sample variances of
        WosScene.solve(..., variance=True), gathered by the same collective.
        A `div` with a leading channel axis, (C, ...) with C <= 4, solves the C source fields
        on one set of walks and returns channel-major outputs, p [C, N] and grad_p [C, N, dim]
        (the variances alike) -- with a process group still through one all-gather.
        differentiable=True: p and grad_p carry div's autograd graph (the variances do not);
        needs reuse_walks=True and no process group."""
        if differentiable:
            if not self.reuse_walks:
                raise ValueError("solve(differentiable=True) needs reuse_walks=True: the backward pass is the "
                                 "walk tape's transpose")
            if self.group is not None or self.force_gather:
                raise ValueError("solve(differentiable=True) does not support a process group: the sharded "
                                 "backward is not implemented")
            return _TapeProjection.apply(div, self, bool(variance))
        self._set_source(div)
        kw = {"variance": True} if variance else {}
        solve_points = self._replay_points if self.reuse_walks else self._solve_points
        if self.group is None and not self.force_gather:
            *out, st = solve_points(self.samples, 0, 1, **kw)
            self.last_stats = st
            return tuple(out)
        import torch.distributed as tdist
        from . import dist as _dist
        group = self.group if self.group is not None else tdist.group.WORLD
        rank, world = tdist.get_rank(group), tdist.get_world_size(group)

        def solve_local(local, base, stride):
            *out, st = solve_points(local.contiguous(), base, stride, **kw)
            self.last_stats = st  # this rank's shard
            return tuple(out)

        return _dist.sharded_projection(solve_local, self.samples, rank, world, self.dim, group=group,
                                        device=self.device, force_gather=self.force_gather)

    def projection_loss(self, velocity, velocity_prev, grad_p, n_samples, generator=None):
        """_project_velocity (model_split.py:272-283): u <- u_prev - grad p on random
        pressure samples, grad p indexed on the device.  The index range is the
        reference's: the 2D caller draws randint(0, N-1) (src/2d/models/model_split.py:274,
        so the last sample is never drawn), the 3D caller randint(0, N)
        (src/3d/models/model_split.py:297)."""
        n = self.samples.shape[0]
        hi = n - 1 if self.dim == 2 else n
        idx = torch.randint(0, hi, (n_samples,), device=self.device, generator=generator)
        x = self.samples[idx]
        with torch.no_grad():
            target = velocity_prev(x) - grad_p[idx]
        return torch.mean((velocity(x) - target) ** 2)

    def projection_fit_loss(self, network, network_prev, grad_p, n_samples, wrap=None, generator=None):
        """projection_loss for velocities that are SIRENs, through the fused fit step
        (wos_amd.siren.fit_loss) instead of an autograd graph over the network: the same
        torch.randint draw (range rule and generator consumption as projection_loss, so a generator
        seeded alike selects the same samples), target = wrap(x, network_prev(x)) - grad_p[idx] with
        the previous network evaluated by wos_amd.siren.eval, and the loss
        mean((wrap(x, network(x)) - target)^2) attached to network's parameters.  wrap(x, u_net) -> u
        must be affine in u_net, wrap(x, N) = S(x) N + c(x) (wos_amd.siren.affine_wrap refuses any other):
        diagonal, as query_velocity's karman and taylorgreen branches, or mixing the components, as its
        jpipe branch and slip_wrap.  Its scale -- a factor per component, or a matrix per point -- goes
        to the kernel, its offset into the target."""
        n = self.samples.shape[0]
        hi = n - 1 if self.dim == 2 else n
        idx = torch.randint(0, hi, (n_samples,), device=self.device, generator=generator)
        x = self.samples[idx]
        with torch.no_grad():
            u_prev = _siren.eval(network_prev, x)
            if wrap is None:
                scale, target = None, u_prev - grad_p[idx]
            else:
                scale, offset = _affine(wrap, x, u_prev.shape[-1])
                target = wrap(x, u_prev) - grad_p[idx] - offset
        return _siren.fit_loss(network, x, target, scale)

    def fit_projection(self, network, network_prev, grad_p, n_samples, n_iters, *, state=None, wrap=None,
                       generator=None, early_stop=None, iters_per_call=256, lr=1e-4):
        """The whole training loop of _project_velocity (n_iters iterations of projection_fit_loss,
        backward and Adam: _training_loop, src/2d/models/base.py:130-152) on the device, through
        wos_amd.siren.fit_run.  The sample pool, grad_p and the previous network are fixed for the
        loop, so u_prev = siren.eval(network_prev, samples), the wrap's (scale, offset) and the target
        wrap(samples, u_prev) - grad_p - offset are computed once over the whole pool; an iteration is
        then gather by index, fit step, Adam step.  The indices are drawn one
        torch.randint(0, hi, (n_samples,)) per iteration -- projection_fit_loss's range rule and
        generator consumption: a generator seeded alike selects the same samples as n_iters calls of
        projection_fit_loss -- and handed over in blocks of iters_per_call iterations (256 x 16384
        indices are 33 MB).  Iteration 0's loss is projection_fit_loss's, bit for bit.
        `network` IS UPDATED IN PLACE.  state: a wos_amd.siren.AdamState to continue (None: a fresh
        one with `lr`).  early_stop: None, or the loss at or below which the loop stops after that
        iteration's update (True: the reference's 1.1e-10); it costs one host synchronisation per
        block, and the losses from the stop on are NaN; no further block is drawn after a stop, but
        the rest of the stopping block is already enqueued and still pays its gathers and fit steps
        with the update switched off -- a smaller iters_per_call bounds that cost.
        Returns (losses [n_iters], state)."""
        n_iters, per_call = int(n_iters), int(iters_per_call)
        if n_iters < 1 or per_call < 1:
            raise ValueError(f"fit_projection: n_iters and iters_per_call must be positive, got {n_iters}, {per_call}")
        if state is None:
            state = _siren.AdamState(network, lr=lr)
        stop = None if early_stop is None or early_stop is False else (1.1e-10 if early_stop is True else float(early_stop))
        n = self.samples.shape[0]
        hi = n - 1 if self.dim == 2 else n
        with torch.no_grad():
            u_prev = _siren.eval(network_prev, self.samples)
            if wrap is None:
                scale, target = None, u_prev - grad_p
            else:
                scale, offset = _affine(wrap, self.samples, u_prev.shape[-1])
                target = wrap(self.samples, u_prev) - grad_p - offset
        losses = []
        for first in range(0, n_iters, per_call):
            k = min(per_call, n_iters - first)
            idx = torch.stack([torch.randint(0, hi, (n_samples,), device=self.device, generator=generator)
                               for _ in range(k)])
            block, status = _siren.fit_run(network, state, self.samples, target, scale, idx, stop_loss=stop)
            losses.append(block)
            if stop is None:
                continue
            # fit_run has synchronised already.  The stopping iteration is applied and counted, so a stop at the
            # block's last iteration leaves status[0] == k: the last applied loss tells, by the device's own test
            # (float32 loss <= stop_loss as a float).
            applied = int(status[0])
            if applied < k or float(block[applied - 1]) <= float(np.float32(stop)):
                if first + k < n_iters:
                    losses.append(torch.full((n_iters - first - k,), float("nan"), dtype=block.dtype, device=block.device))
                break
        return torch.cat(losses), state

    def fit_projection_ensemble(self, networks, networks_prev, grad_p, n_samples, n_iters, *, states=None, wraps=None,
                                generator=None, early_stop=None, iters_per_call=256, lr=1e-4):
        """fit_projection for the E <= 4 members of an ensemble after one multi-channel solve, trained in
        one device loop (wos_amd.siren.fit_run_ensemble).  networks and networks_prev are lists of E
        networks of one shape, grad_p the (E, N, dim) of solve() on an (E, ...) source; states and wraps,
        when given, lists with one entry per member (an entry of wraps may be None).  The members share
        the sample pool and the index draw: one torch.randint(0, hi, (n_samples,)) per iteration serves
        all of them -- common random numbers, as the solve's walks are.  Member e equals fit_projection
        on (networks[e], networks_prev[e], grad_p[e]) with a generator seeded alike, bit for bit, as
        long as no member has stopped early: a stopped member leaves the later blocks (its network
        frozen, its losses NaN) while the others go on, and no further block is drawn once every member
        has stopped.  EVERY NETWORK IS UPDATED IN PLACE.  Returns (losses [E, n_iters], states)."""
        who = "fit_projection_ensemble"
        n_iters, per_call = int(n_iters), int(iters_per_call)
        if n_iters < 1 or per_call < 1:
            raise ValueError(f"{who}: n_iters and iters_per_call must be positive, got {n_iters}, {per_call}")
        networks = list(networks)
        E = len(networks)
        if not 1 <= E <= _siren.MAX_MEMBERS:
            raise ValueError(f"{who}: an ensemble has 1..{_siren.MAX_MEMBERS} members, got {E}")
        prevs, wraps = _per_member(who, "networks_prev", list(networks_prev), E), _per_member(who, "wraps", wraps, E)
        n = self.samples.shape[0]
        if tuple(grad_p.shape) != (E, n, self.dim):
            raise ValueError(f"{who}: grad_p must be {(E, n, self.dim)}, a multi-channel solve's, got {tuple(grad_p.shape)}")
        states = [_siren.AdamState(net, lr=lr) for net in networks] if states is None else _per_member(who, "states", states, E)
        stop = _stop_loss(early_stop)
        hi = n - 1 if self.dim == 2 else n
        targets, scales = [], []
        with torch.no_grad():
            for e in range(E):
                u_prev = _siren.eval(prevs[e], self.samples)
                if wraps[e] is None:
                    scale, target = None, u_prev - grad_p[e]
                else:
                    scale, offset = _affine(wraps[e], self.samples, u_prev.shape[-1])
                    target = wraps[e](self.samples, u_prev) - grad_p[e] - offset
                targets.append(target)
                scales.append(scale)

        def run_block(first, k, live):
            idx = torch.stack([torch.randint(0, hi, (n_samples,), device=self.device, generator=generator)
                               for _ in range(k)])
            return _siren.fit_run_ensemble([networks[e] for e in live], [states[e] for e in live], self.samples,
                                           [targets[e] for e in live], [scales[e] for e in live], idx, stop_loss=stop)
        return _ensemble_blocks(who, networks, states, n_iters, per_call, stop, run_block), states


_wrap_mixes = weakref.WeakKeyDictionary()  # wrap -> whether it mixes the velocity's components


def _affine(wrap, x, d_out):
    """(scale, offset) of a wrap for the two fit losses, as wos_amd.siren.fit takes them: scale
    [..., d_out] for a wrap that is diagonal in the network's output (siren.diagonal_wrap's bits),
    [..., d_out, d_out] for one that mixes its components (siren.affine_wrap).  The probe and the
    classification read their verdicts on the host, so a wrap is probed and classified at its first
    batch only -- whether it is affine, and whether it mixes components, does not depend on the points --
    and every later batch builds the cached form without a synchronisation.  A callable that cannot be
    weakly referenced is probed every time."""
    try:
        mixes = _wrap_mixes.get(wrap)
    except TypeError:
        mixes = None
    if mixes is None:
        scale, offset, mixes = _siren.affine_wrap(wrap, x, d_out)
        try:
            _wrap_mixes[wrap] = mixes
        except TypeError:
            pass
        return scale, offset
    if not mixes:
        return _siren.diagonal_wrap(wrap, x, d_out, check=False)
    with torch.no_grad():
        return _siren._affine_columns(wrap, x.detach(), d_out)


def slip_wrap(normal, weight):
    """The free-slip wrap of a curved wall, wrap(x, u) = u - (1 - weight(x)) (n(x) . u) n(x): the
    network's normal component is removed and a share weight(x) of it put back, u_t + weight u_n --
    the reference's jpipe branch around its bend (src/2d/models/base.py:191-222, with the clamped
    wall distance over eps as the weight).  normal(x) -> [..., d] unit normals, weight(x) -> [...] in
    [0, 1], both torch callables of the points; where weight is 1 the wrap is the identity, where it
    is 0 the velocity is tangential.  Affine in u but not diagonal: u = (I - (1 - w) n n^T) N, which
    siren.affine_wrap classifies as mixing and the fit losses and loops here take as a matrix per
    point.  Pure torch and differentiable in x, so source_from_network(wrap=) and
    siren.divergence_with_wrap take it as they are; compose masks around it in a function of your own,
    e.g. lambda x, u: inlet(x, slip(x, u))."""
    def wrap(x, u):
        n = normal(x)
        w = weight(x)
        un = (n * u).sum(-1, keepdim=True)
        return u - (1 - w).unsqueeze(-1) * un * n
    wrap.__name__ = "slip_wrap"  # the name a refusal gives
    return wrap


def advection_fit_loss(network, network_prev, samples, dt, size, network_tilde=None, wrap=None):
    """_advect_velocity's loss (src/2d/models/model_split.py:88-120; semi-Lagrangian) for velocities
    that are SIRENs, through the fused fit step: backtrack x_b = samples - dt * u_prev(samples) with
    the wrapped previous velocity, clamp x_b to `size` ([x0, x1, y0, y1(, z0, z1)]), take
    target = u_prev(x_b) -- or 2 u_prev(x_b) - u_tilde(x_b) when network_tilde is given (the
    reference's `flag` branch) -- and return mean((wrap(samples, network(samples)) - target)^2)
    attached to network's parameters (wos_amd.siren.fit_loss).  Every no-grad evaluation runs in
    wos_amd.siren.eval.  wrap as in PressureProjector.projection_fit_loss."""
    x = samples.detach()
    target, scale = _advection_target(network_prev, x, dt, size, network_tilde, wrap)
    return _siren.fit_loss(network, x, target, scale)


def _advection_target(network_prev, x, dt, size, network_tilde, wrap):
    """The no-grad part of the advection fit at the points x [..., d_in]: (target, scale) as
    wos_amd.siren.fit takes them (scale None without a wrap).  Every operation is pointwise --
    siren.eval gives a point the same bits in any batch -- so the rows of one call over the points of
    many iterations are, bit for bit, the rows of one call per iteration: advection_fit_loss and
    fit_advection both go through here."""
    with torch.no_grad():
        def query(net, pts):
            u = _siren.eval(net, pts)
            return u if wrap is None else wrap(pts, u)
        back = x - query(network_prev, x) * dt
        back = torch.stack([back[..., k].clamp(min=size[2 * k], max=size[2 * k + 1]) for k in range(x.shape[-1])], dim=-1)
        target = query(network_prev, back)
        if network_tilde is not None:
            target = 2 * target - query(network_tilde, back)
        scale = None
        if wrap is not None:
            scale, offset = _affine(wrap, x, target.shape[-1])
            target = target - offset
    return target, scale


def _advection_block(who, first, k, d, dev, size, n_samples, samples, keep, generator):
    """The points of iterations first .. first + k - 1 of an advection fit, flattened, and their row
    counts: (x [sum(counts), d], counts).  fit_advection's rules for n_samples, samples and keep."""
    if samples is None:
        x = torch.stack([torch.rand(int(n_samples), d, device=dev, generator=generator) for _ in range(k)])
        for c in range(d):
            x[..., c] = x[..., c] * (size[2 * c + 1] - size[2 * c]) + size[2 * c]
    else:
        x = samples(k)
        if x.dim() != 3 or x.shape[0] != k or x.shape[1] < 1 or x.shape[2] != d:
            raise ValueError(f"{who}: samples({k}) must return [{k}, n, {d}], got shape {tuple(x.shape)}")
        x = x.detach()
    n = int(x.shape[1])
    x = x.reshape(k * n, d)
    if keep is None:
        counts = [n] * k
    else:
        mask = keep(x)
        if mask.dtype != torch.bool or tuple(mask.shape) != (k * n,):
            raise ValueError(f"{who}: keep must return a bool mask of shape {(k * n,)}, got {mask.dtype} "
                             f"{tuple(mask.shape)}")
        counts = mask.reshape(k, n).sum(dim=1).tolist()  # the block's one host synchronisation
        for i, c in enumerate(counts):
            if c < 1:
                raise ValueError(f"{who}: keep left iteration {first + i} without a point (its loss is a mean "
                                 f"over nothing); the network and the state are as the {first} iterations before this "
                                 f"block left them")
        # the kept rows in their order; the size is known, so this does not wait for the device again
        x = x[torch.nonzero_static(mask, size=sum(counts)).squeeze(1)]
    return x, counts


def fit_advection(network, network_prev, dt, size, n_iters, *, n_samples=None, samples=None, network_tilde=None,
                  wrap=None, keep=None, state=None, generator=None, early_stop=None, iters_per_call=256, lr=1e-4):
    """The whole training loop of _advect_velocity (n_iters iterations of advection_fit_loss, backward
    and Adam: src/2d/models/model_split.py:88-120 in _training_loop, base.py:130-152; the 3D twin
    src/3d/models/model_split.py:89-122) on the device, through wos_amd.siren.fit_run_batches.
    network_prev and network_tilde are frozen for the loop, so the points, backtracked positions,
    targets and wrap factors of a block of k <= iters_per_call iterations are computed together, all
    rows at once, exactly as advection_fit_loss computes them per iteration; an iteration is then fit
    step and Adam step on its own rows.  Iteration i is, bit for bit in the loss, every parameter and
    both moments, advection_fit_loss's target for that iteration's points followed by siren.fit and
    siren.adam_step.  `network` IS UPDATED IN PLACE.
    Points: with n_samples, one torch.rand(n_samples, d_in) per iteration on the network's device,
    component c scaled as sample_random_2D does, x_c * (size[2c+1] - size[2c]) + size[2c] -- the
    generator consumption of the Python loop, so a generator seeded alike yields the same points;
    otherwise `samples` is a callable samples(k) -> [k, n, d_in] (the `uniform` and `random+uniform`
    patterns).  Exactly one of the two.
    keep: None, or a function of points [m, d_in] returning a bool mask [m] -- for karman
    lambda x: sdf(x) > 0 with a MeshSDF or an analytic circle, the reference's
    samples = samples[dist > 0] (base.py:239-241).  It is applied to the flattened block; rows keep
    their order, so an iteration's points stay contiguous and in draw order, and its loss is the mean
    over its own count.  The counts are read on the host: the one synchronisation per block.  An
    iteration left without a point raises ValueError, naming the iteration, before the block is
    enqueued: network and state are then as the previous block left them.
    wrap(x, u_net) -> u as in advection_fit_loss: pointwise and affine in u_net.  A wrap whose
    value at a point depends on the rest of the batch (the 3D smoke branch's per-call np.random draw,
    the jpipe branch's norm over the batch as the reference wrote it) is not covered by the block form: a block hands it the
    points of k iterations at once.  iters_per_call=1 hands such a wrap exactly one iteration's points.
    state: a wos_amd.siren.AdamState to continue (None: a fresh one with `lr`).  early_stop as in
    PressureProjector.fit_projection: None, or the loss at or below which the loop stops after that
    iteration's update (True: the reference's 1.1e-10); one host read per block, the losses from the
    stop on are NaN, no further block is drawn.  A block of 256 iterations of 16384 points holds its
    points, backtracked points, two or three network values, target and scale: about 0.3 GB at its peak.
    Returns (losses [n_iters], state)."""
    n_iters, per_call = int(n_iters), int(iters_per_call)
    if n_iters < 1 or per_call < 1:
        raise ValueError(f"fit_advection: n_iters and iters_per_call must be positive, got {n_iters}, {per_call}")
    if (n_samples is None) == (samples is None):
        raise ValueError("fit_advection: give exactly one of n_samples (torch.rand points per iteration) and samples "
                         "(a callable samples(k) -> [k, n, d_in])")
    if n_samples is not None and int(n_samples) < 1:
        raise ValueError(f"fit_advection: n_samples must be positive, got {n_samples}")
    p = _siren.pack(network)
    d, dev = p.d_in, p.weights[0].device
    if len(size) != 2 * d:
        raise ValueError(f"fit_advection: size must hold {2 * d} bounds for {d} coordinates, got {len(size)}")
    if state is None:
        state = _siren.AdamState(network, lr=lr)
    stop = None if early_stop is None or early_stop is False else (1.1e-10 if early_stop is True else float(early_stop))
    losses = []
    for first in range(0, n_iters, per_call):
        k = min(per_call, n_iters - first)
        x, counts = _advection_block("fit_advection", first, k, d, dev, size, n_samples, samples, keep, generator)
        target, scale = _advection_target(network_prev, x, dt, size, network_tilde, wrap)
        block, status = _siren.fit_run_batches(network, state, x, target, scale, counts, stop_loss=stop)
        losses.append(block)
        if stop is None:
            continue
        # as in fit_projection: a stop at the block's last iteration leaves status[0] == k, and the last applied
        # loss tells, by the device's own test
        applied = int(status[0])
        if applied < k or float(block[applied - 1]) <= float(np.float32(stop)):
            if first + k < n_iters:
                losses.append(torch.full((n_iters - first - k,), float("nan"), dtype=block.dtype, device=block.device))
            break
    return torch.cat(losses), state


def _stop_loss(early_stop):
    return None if early_stop is None or early_stop is False else (1.1e-10 if early_stop is True else float(early_stop))


def _per_member(who, name, values, E):
    """A per-member argument as a list of E entries (None: E times None)."""
    if values is None:
        return [None] * E
    values = list(values)
    if len(values) != E:
        raise ValueError(f"{who}: {name} must hold one entry per member ({E}), got {len(values)}")
    return values


def _ensemble_blocks(who, networks, states, n_iters, per_call, stop, run_block):
    """The block loop of the two ensemble fits.  run_block(first, k, live) -> (block [len(live), k],
    status [len(live), 2]) trains the members `live` (indices into networks) for iterations
    first .. first + k - 1.  A member that has stopped leaves the later blocks, so its network stays
    as the stop left it and its losses stay NaN; no block is run once every member has stopped."""
    E = len(networks)
    live = list(range(E))
    losses = None
    for first in range(0, n_iters, per_call):
        k = min(per_call, n_iters - first)
        block, status = run_block(first, k, live)
        if losses is None:
            losses = torch.full((E, n_iters), float("nan"), dtype=block.dtype, device=block.device)
        losses[live, first:first + k] = block
        if stop is None:
            continue
        # as in fit_projection: a stop at the block's last iteration leaves status[e][0] == k, and the last
        # applied loss tells, by the device's own test
        applied = status[:, 0].tolist()
        last = block[torch.arange(len(live)), torch.tensor(applied) - 1].tolist()
        live = [e for e, a, loss in zip(live, applied, last) if not (a < k or loss <= float(np.float32(stop)))]
        if not live:
            break
    return losses


def fit_advection_ensemble(networks, networks_prev, dt, size, n_iters, *, n_samples=None, samples=None, networks_tilde=None,
                           wraps=None, keep=None, states=None, generator=None, early_stop=None, iters_per_call=256, lr=1e-4):
    """fit_advection for the E <= 4 members of an ensemble on one obstacle mesh, trained in one device
    loop (wos_amd.siren.fit_run_batches_ensemble).  networks, networks_prev and, when given,
    networks_tilde, wraps and states are lists with one entry per member (an entry of wraps or of
    networks_tilde may be None).  The members share the points -- one torch.rand per iteration, or one
    samples(k), serves all of them -- and one `keep` filter, so the row counts are common; the previous
    networks and wraps are evaluated per member, each in one launch over the block's rows, as
    fit_advection does.  Member e equals fit_advection on member e with a generator seeded alike, bit
    for bit, as long as no member has stopped early: a stopped member leaves the later blocks (its
    network frozen, its losses NaN) while the others go on, and no further block is drawn once every
    member has stopped.  EVERY NETWORK IS UPDATED IN PLACE.  Returns (losses [E, n_iters], states)."""
    who = "fit_advection_ensemble"
    n_iters, per_call = int(n_iters), int(iters_per_call)
    if n_iters < 1 or per_call < 1:
        raise ValueError(f"{who}: n_iters and iters_per_call must be positive, got {n_iters}, {per_call}")
    if (n_samples is None) == (samples is None):
        raise ValueError(f"{who}: give exactly one of n_samples (torch.rand points per iteration) and samples "
                         "(a callable samples(k) -> [k, n, d_in])")
    if n_samples is not None and int(n_samples) < 1:
        raise ValueError(f"{who}: n_samples must be positive, got {n_samples}")
    networks = list(networks)
    E = len(networks)
    if not 1 <= E <= _siren.MAX_MEMBERS:
        raise ValueError(f"{who}: an ensemble has 1..{_siren.MAX_MEMBERS} members, got {E}")
    prevs, tildes = _per_member(who, "networks_prev", list(networks_prev), E), _per_member(who, "networks_tilde", networks_tilde, E)
    wraps = _per_member(who, "wraps", wraps, E)
    p = _siren.pack(networks[0])
    d, dev = p.d_in, p.weights[0].device
    if len(size) != 2 * d:
        raise ValueError(f"{who}: size must hold {2 * d} bounds for {d} coordinates, got {len(size)}")
    states = [_siren.AdamState(net, lr=lr) for net in networks] if states is None else _per_member(who, "states", states, E)
    stop = _stop_loss(early_stop)

    def run_block(first, k, live):
        x, counts = _advection_block(who, first, k, d, dev, size, n_samples, samples, keep, generator)
        rows = [_advection_target(prevs[e], x, dt, size, tildes[e], wraps[e]) for e in live]
        return _siren.fit_run_batches_ensemble([networks[e] for e in live], [states[e] for e in live], x,
                                               [t for t, _ in rows], [sc for _, sc in rows], counts, stop_loss=stop)
    return _ensemble_blocks(who, networks, states, n_iters, per_call, stop, run_block), states
