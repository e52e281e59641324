"""Host-side API of the MI355X walk-on-stars engine (thin layer over include/wos.h).

Mirrors the reference's operator interface for the pressure solve:
  Scene(config, source)   <-> bindings/zombie/demo/scene.h:54-77 (2D),
                              bindings/zombie3d/demo/scene_3d.h:22-40 (3D)
  solve(points)           <-> runWalkOnStars_sampled, demo.cpp:119-205 /
                              runWalkOnStars_3d, zombie3d/demo/demo.cpp:15-116
Inputs may be numpy arrays (host) or torch tensors already on the GPU (zero-copy:
device pointers are handed to the C ABI and the kernel runs on torch's current
stream).
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import BvcParams, SceneDesc, SceneInfo, SolverParams, Stats, WosError, check

_DEFAULT_SEED = 0x5EED0001


def load_obj(path, dim, flip_orientation=False, normalize=False):
    """OBJ -> (vertices [V,dim] f32, prims [P,dim] i32) with the reference's parsing rules."""
    L = _lib.load()
    m = _lib.Mesh()
    check(L.wos_load_obj(os.fsencode(path), dim, int(flip_orientation), int(normalize), C.byref(m)),
          f"wos_load_obj({path})")
    try:
        v = np.ctypeslib.as_array(m.vertices, shape=(m.n_vertices * dim,)).copy().reshape(-1, dim)
        ix = np.ctypeslib.as_array(m.prims, shape=(m.n_prims * dim,)).copy().reshape(-1, dim)
    finally:
        L.wos_mesh_free(C.byref(m))
    return v.astype(np.float32), ix.astype(np.int32)


def _get_opt(d, key, default, typ):
    v = d.get(key, default) if d is not None else default
    return typ(v)


def solver_params(solver=None, output=None, seed=None, schedule=0):
    """Parse the reference's wost.json "solver" / "output" sections (demo.cpp:121-137,
    grid.h:159), same keys (including the misspelled `setps...`) and defaults."""
    s = dict(solver or {})
    o = dict(output or {})
    p = SolverParams()
    _lib.load().wos_default_params(C.byref(p))
    p.n_walks = _get_opt(s, "nWalks", 128, int)
    p.max_walk_length = _get_opt(s, "maxWalkLength", 1024, int)
    p.steps_before_tikhonov = _get_opt(s, "setpsBeforeApplyingTikhonov", p.max_walk_length, int)
    p.steps_before_maximal_spheres = _get_opt(s, "setpsBeforeUsingMaximalSpheres", p.max_walk_length, int)
    p.epsilon_shell = _get_opt(s, "epsilonShell", 1e-3, float)
    p.min_star_radius = _get_opt(s, "minStarRadius", 1e-3, float)
    p.silhouette_precision = _get_opt(s, "silhouettePrecision", 1e-3, float)
    p.russian_roulette_threshold = _get_opt(s, "russianRouletteThreshold", 0.0, float)
    p.boundary_distance_mask = _get_opt(o, "boundaryDistanceMask", 0.0, float)
    p.disable_gradient_control_variates = int(bool(s.get("disableGradientControlVariates", False)))
    p.disable_gradient_antithetic_variates = int(bool(s.get("disableGradientAntitheticVariates", False)))
    p.use_cosine_sampling = int(bool(s.get("useCosineSamplingForDirectionalDerivatives", False)))
    p.ignore_dirichlet = int(bool(s.get("ignoreDirichlet", False)))
    p.ignore_neumann = int(bool(s.get("ignoreNeumann", False)))
    p.ignore_source = int(bool(s.get("ignoreSource", False)))
    p.seed = int(seed if seed is not None else s.get("seed", _DEFAULT_SEED)) & 0xFFFFFFFFFFFFFFFF
    # extension key (no reference analogue): robust float semantics, SURVEY.md 7.2 hard part 4
    p.robust_float = int(bool(s.get("robustFloatSemantics", False)))
    # GPU scheduling switches (_lib.SCHED_*): never change a result
    p.schedule = int(schedule)
    return p


def bvc_params(solver=None, output=None, grid_box=None):
    """The boundary-value-caching keys runBoundaryValueCaching reads (demo.cpp:269-290):
    same names and defaults; output.gridRes is required.  grid_box = (x0, y0, ex, ey): the
    rectangle of the evaluation grid (None: the scene's bounding box, demo.cpp:311)."""
    s = dict(solver or {})
    o = dict(output or {})
    if "gridRes" not in o:
        raise KeyError("Missing required setting: gridRes")
    b = BvcParams()
    _lib.load().wos_default_bvc_params(C.byref(b))
    eps = _get_opt(s, "epsilonShell", 1e-3, float)
    b.n_walks_solution = _get_opt(s, "nWalksForCachedSolutionEstimates", 128, int)
    b.n_walks_gradient = _get_opt(s, "nWalksForCachedGradientEstimates", 640, int)
    b.boundary_cache_size = _get_opt(s, "boundaryCacheSize", 1024, int)
    b.domain_cache_size = _get_opt(s, "domainCacheSize", 1024, int)
    b.grid_res = int(o["gridRes"])
    b.use_finite_differences = int(bool(s.get("useFiniteDifferencesForBoundaryDerivatives", False)))
    b.normal_offset = _get_opt(s, "normalOffsetForCachedDirichletSamples", 5.0 * eps, float)
    b.radius_clamp = _get_opt(s, "radiusClampForKernels", 1e-3, float)
    b.kernel_regularization = _get_opt(s, "regularizationForKernels", 0.0, float)
    if grid_box is not None:
        for k in range(4):
            b.grid_box[k] = float(grid_box[k])
    return b


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _check_source_shape(shape, dim):
    """(has a channel axis, channels) of a source of this shape; WosError if it fits neither form."""
    shape = tuple(int(s) for s in shape)
    if len(shape) == dim:
        return False, 1
    if len(shape) == dim + 1:
        if not 1 <= shape[0] <= _lib.MAX_CHANNELS:
            raise WosError(f"a source with a channel axis holds 1..{_lib.MAX_CHANNELS} channels, got shape {shape}")
        return True, shape[0]
    raise WosError(f"source grid must be {dim}-D, or {dim + 1}-D with a leading channel axis, got shape {shape}")


class WosScene:
    """Geometry + source field resident on one GPU."""

    def __init__(self, vertices, prims, source=None, absorption=0.0, *, dvertices=None, dprims=None,
                 dirichlet_value=0.0, dirichlet_image=None, dirichlet_image_box=None, neumann_image=None,
                 neumann_image_box=None, watertight=True, double_sided=False, device=0, dirichlet_values=None):
        """source: the grid [H, W] / [X, Y, Z], or several source fields on one set of walks,
        [C, H, W] / [C, X, Y, Z] with C <= 4 (wos_scene_set_source_channels): solve() then returns
        every output with the same leading channel axis (for C = 1 too), channel c bit for bit
        the solve of source c alone.  dirichlet_values (optional, with a channel axis): the
        constant g_c of every channel instead of dirichlet_value.
        dirichlet_image (2D, optional): g as an image [H, W] (row ~ y) over the rectangle
        dirichlet_image_box = (x0, y0, ex, ey), evaluated at each walk's projection onto the
        Dirichlet boundary (the upstream demo's pde.dirichlet, scene.h:202-207); replaces the
        constant dirichlet_value.  neumann_image (2D, optional): the Neumann data h as an image
        [H, W] over neumann_image_box, evaluated at the walks' stochastic boundary samples and at
        BVC's Neumann samples (the upstream demo's pde.neumann, scene.h:175-181); default h = 0."""
        L = _lib.load()
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        ix = np.ascontiguousarray(prims, dtype=np.int32)
        self.dim = int(v.shape[1])
        if self.dim not in (2, 3) or ix.ndim != 2 or ix.shape[1] != self.dim:
            raise WosError("vertices must be [V,2|3] and prims [P,dim]")
        d = SceneDesc()
        d.dim = self.dim
        d.vertices = v.ctypes.data_as(C.POINTER(C.c_float))
        d.prims = ix.ctypes.data_as(C.POINTER(C.c_int32))
        d.n_vertices, d.n_prims = v.shape[0], ix.shape[0]
        keep = [v, ix]
        if dprims is not None and len(dprims):
            dv = np.ascontiguousarray(dvertices, dtype=np.float32)
            dix = np.ascontiguousarray(dprims, dtype=np.int32)
            d.dvertices = dv.ctypes.data_as(C.POINTER(C.c_float))
            d.dprims = dix.ctypes.data_as(C.POINTER(C.c_int32))
            d.n_dvertices, d.n_dprims = dv.shape[0], dix.shape[0]
            keep += [dv, dix]
        d.dirichlet_value = float(dirichlet_value)
        if dirichlet_image is not None:
            if dirichlet_image_box is None or len(dirichlet_image_box) != 4:
                raise WosError("dirichlet_image needs dirichlet_image_box = (x0, y0, ex, ey)")
            if _is_torch(dirichlet_image) and dirichlet_image.is_cuda:
                dimg = dirichlet_image.detach().to(dtype=__import__("torch").float32).contiguous()
                d.dirichlet_image, d.dirichlet_image_on_device = dimg.data_ptr(), 1
            else:
                if _is_torch(dirichlet_image):
                    dirichlet_image = dirichlet_image.detach().cpu().numpy()
                dimg = np.ascontiguousarray(dirichlet_image, dtype=np.float32)
                d.dirichlet_image = dimg.ctypes.data
            if len(dimg.shape) != 2:
                raise WosError(f"dirichlet_image must be 2-D, got shape {tuple(dimg.shape)}")
            d.dirichlet_image_dims[0], d.dirichlet_image_dims[1] = int(dimg.shape[0]), int(dimg.shape[1])
            for k in range(4):
                d.dirichlet_image_box[k] = float(dirichlet_image_box[k])
            keep.append(dimg)
        if neumann_image is not None:
            nimg, on_dev = self._image(neumann_image, neumann_image_box, "neumann_image")
            d.neumann_image, d.neumann_image_on_device = (nimg.data_ptr() if on_dev else nimg.ctypes.data), on_dev
            d.neumann_image_dims[0], d.neumann_image_dims[1] = int(nimg.shape[0]), int(nimg.shape[1])
            for k in range(4):
                d.neumann_image_box[k] = float(neumann_image_box[k])
            keep.append(nimg)
        d.absorption = float(absorption)
        d.is_watertight = int(bool(watertight))
        d.is_double_sided = int(bool(double_sided))
        self.source_shape = None
        self._channel_axis = False
        chan_source = None
        if source is not None and _check_source_shape(tuple(source.shape), self.dim)[0]:
            chan_source, source = source, None  # set after the scene exists (set_source)
        elif dirichlet_values is not None:
            raise WosError("dirichlet_values needs a source with a leading channel axis")
        if source is not None:
            if _is_torch(source) and source.is_cuda:
                src = source.detach().to(dtype=__import__("torch").float32).contiguous()
                d.source = src.data_ptr()
                d.source_on_device = 1
                keep.append(src)
                shape = tuple(src.shape)
            else:
                if _is_torch(source):
                    source = source.detach().cpu().numpy()
                src = np.ascontiguousarray(source, dtype=np.float32)
                d.source = src.ctypes.data
                keep.append(src)
                shape = src.shape
            if len(shape) != self.dim:
                raise WosError(f"source grid must be {self.dim}-D, got shape {shape}")
            for k in range(3):
                d.source_dims[k] = shape[k] if k < len(shape) else 0
            self.source_shape = tuple(int(s) for s in shape)
        self.device = int(device)
        h = C.c_void_p()
        check(L.wos_scene_create(C.byref(d), self.device, C.byref(h)), "wos_scene_create")
        self._h = h
        del keep
        if chan_source is not None:
            self.set_source(chan_source, dirichlet_values=dirichlet_values)
            if _is_torch(chan_source) and chan_source.is_cuda:
                # like wos_scene_create's copy: done when the constructor returns
                __import__("torch").cuda.current_stream(chan_source.device).synchronize()

    @staticmethod
    def _image(img, box, name):
        """A 2-D float32 image for the C ABI: (contiguous array or CUDA tensor, on_device)."""
        if box is None or len(box) != 4:
            raise WosError(f"{name} needs {name}_box = (x0, y0, ex, ey)")
        if _is_torch(img) and img.is_cuda:
            out, on_dev = img.detach().to(dtype=__import__("torch").float32).contiguous(), 1
        else:
            if _is_torch(img):
                img = img.detach().cpu().numpy()
            out, on_dev = np.ascontiguousarray(img, dtype=np.float32), 0
        if len(out.shape) != 2:
            raise WosError(f"{name} must be 2-D, got shape {tuple(out.shape)}")
        return out, on_dev

    @property
    def channels(self):
        """Source channels the scene holds (1 for a source without a channel axis)."""
        return int(_lib.load().wos_scene_channels(self._h))

    def set_source(self, source, stream=None, *, dirichlet_values=None):
        """Replace the source grid (-div u) in place: the geometry stays resident.
        `source` is a numpy array or a torch tensor (a CUDA tensor is copied
        device-to-device on torch's current stream, no host round trip).  Replaces
        the reference's per-step Scene(sceneConfig, div) (model_split.py:191).
        A source with one extra leading axis, [C, ...] with C <= 4, makes the scene
        multi-channel (see __init__); dirichlet_values: C constants g_c, or None for the
        scene's own Dirichlet data.  A source without the axis returns it to one channel."""
        L = _lib.load()
        dims = (C.c_int32 * 3)(0, 0, 0)
        axis, nch = _check_source_shape(tuple(source.shape), self.dim)
        if dirichlet_values is not None:
            if not axis:
                raise WosError("dirichlet_values needs a source with a leading channel axis")
            gv = np.ascontiguousarray(dirichlet_values, dtype=np.float32).reshape(-1)
            if gv.shape[0] != nch:
                raise WosError(f"dirichlet_values must hold one constant per channel ({nch}), got {gv.shape[0]}")
        if _is_torch(source) and source.is_cuda:
            import torch
            src = source.detach().to(dtype=torch.float32).contiguous()
            shape = tuple(src.shape)
            ptr, on_dev = src.data_ptr(), 1
            if stream is None:
                stream = torch.cuda.current_stream(src.device).cuda_stream
        else:
            if _is_torch(source):
                source = source.detach().cpu().numpy()
            src = np.ascontiguousarray(source, dtype=np.float32)
            shape = src.shape
            ptr, on_dev = src.ctypes.data, 0
        grid = shape[1:] if axis else shape
        for k in range(len(grid)):
            dims[k] = int(grid[k])
        if axis:
            gp = gv.ctypes.data_as(C.POINTER(C.c_float)) if dirichlet_values is not None else None
            check(L.wos_scene_set_source_channels(self._h, ptr, nch, dims, gp, on_dev, stream),
                  "wos_scene_set_source_channels")
        else:
            check(L.wos_scene_set_source(self._h, ptr, dims, on_dev, stream), "wos_scene_set_source")
        # the copy is ordered on `stream`: keep the buffer alive until the next replacement
        self._src_keep = src
        self.source_shape = tuple(int(x) for x in shape)
        self._channel_axis = axis

    @classmethod
    def from_obj(cls, path, dim, source=None, absorption=0.0, flip_orientation=False, normalize=False, **kw):
        v, ix = load_obj(path, dim, flip_orientation, normalize)
        return cls(v, ix, source, absorption, **kw)

    def info(self):
        i = SceneInfo()
        check(_lib.load().wos_scene_get_info(self._h, C.byref(i)), "wos_scene_get_info")
        return {"dim": i.dim, "n_prims": i.n_prims, "n_silhouettes": i.n_silhouettes,
                "n_dprims": i.n_dprims, "device": i.device,
                "bbox_min": list(i.bbox_min)[:i.dim], "bbox_max": list(i.bbox_max)[:i.dim]}

    def solve(self, pts, params=None, *, index_base=0, index_stride=1, counts=False, stream=None,
              sync=True, variance=False):
        """Solve at query points.  Returns (p [N], grad [N,dim], stats dict[, n_est, steps])
        as numpy arrays for host input, torch tensors for GPU tensor input.  With variance=True
        the tuple is (p, grad, p_var [N], grad_var [N,dim], stats dict[, n_est, steps]): the
        reference's per-walk sample variances M2 / max(1, n_est - 1) (wos_solve_var,
        walk_on_stars.h:811-831), masked like their means.  With GPU tensors
        and sync=False the solve is only enqueued on the stream: the stats dict then holds
        just "ticket"; solve_stats(ticket) waits for that solve and returns the full dict.
        A scene whose source has a channel axis [C, ...] returns p [C, N], grad [C, N, dim] and
        the variances alike (wos_solve_channels); n_est and steps stay [N], shared by the channels.
        `stream`: a torch.cuda.Stream or a raw hipStream_t handle (default: torch's current
        stream)."""
        L = _lib.load()
        params = params if params is not None else solver_params()
        st = Stats()
        nch = self.channels if self._channel_axis else 0
        lead = (nch,) if self._channel_axis else ()
        if _is_torch(pts) and pts.is_cuda:
            import torch
            x = pts.detach().to(torch.float32).contiguous()
            n = x.shape[0]
            if x.ndim != 2 or x.shape[1] != self.dim:
                raise WosError(f"points must be [N,{self.dim}]")
            p = torch.empty(lead + (n,), dtype=torch.float32, device=x.device)
            g = torch.empty(lead + (n, self.dim), dtype=torch.float32, device=x.device)
            ne = torch.empty(n, dtype=torch.int32, device=x.device) if counts else None
            sp = torch.empty(n, dtype=torch.int32, device=x.device) if counts else None
            pv = torch.empty(lead + (n,), dtype=torch.float32, device=x.device) if variance else None
            gv = torch.empty(lead + (n, self.dim), dtype=torch.float32, device=x.device) if variance else None
            cur = torch.cuda.current_stream(x.device)
            ts = None
            if stream is None:
                s = cur.cuda_stream
            else:
                ts = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream),
                                                                                                    device=x.device)
                s = ts.cuda_stream
                # the points and the fresh output buffers belong to torch's current stream:
                # the solve on `stream` starts after the work queued there (the kernel that
                # produced x, the allocator's last user of p / g)
                ts.wait_stream(cur)
            flags = _lib.WOS_PTRS_DEVICE | (0 if sync else _lib.WOS_ASYNC)
            if self._channel_axis:
                check(L.wos_solve_channels(self._h, C.byref(params), x.data_ptr(), n, index_base, index_stride, nch,
                                           p.data_ptr(), g.data_ptr(), pv.data_ptr() if variance else None,
                                           gv.data_ptr() if variance else None, ne.data_ptr() if counts else None,
                                           sp.data_ptr() if counts else None, C.byref(st), s, flags),
                      "wos_solve_channels")
            elif variance:
                check(L.wos_solve_var(self._h, C.byref(params), x.data_ptr(), n, index_base, index_stride,
                                      p.data_ptr(), g.data_ptr(), pv.data_ptr(), gv.data_ptr(),
                                      ne.data_ptr() if counts else None, sp.data_ptr() if counts else None,
                                      C.byref(st), s, flags), "wos_solve_var")
            else:
                check(L.wos_solve(self._h, C.byref(params), x.data_ptr(), n, index_base, index_stride,
                                  p.data_ptr(), g.data_ptr(), ne.data_ptr() if counts else None,
                                  sp.data_ptr() if counts else None, C.byref(st), s, flags), "wos_solve")
            if not sync and ts is not None:
                # the buffers were allocated on torch's current stream but the enqueued
                # solve uses them on `stream`: keep the caching allocator from handing
                # their memory out again before that stream has finished with them
                for t in (x, p, g, ne, sp, pv, gv):
                    if t is not None:
                        t.record_stream(ts)
        else:
            if _is_torch(pts):
                pts = pts.detach().cpu().numpy()
            x = np.ascontiguousarray(pts, dtype=np.float32)
            if x.ndim != 2 or x.shape[1] != self.dim:
                raise WosError(f"points must be [N,{self.dim}]")
            n = x.shape[0]
            p = np.empty(lead + (n,), np.float32)
            g = np.empty(lead + (n, self.dim), np.float32)
            ne = np.empty(n, np.int32) if counts else None
            sp = np.empty(n, np.int32) if counts else None
            pv = np.empty(lead + (n,), np.float32) if variance else None
            gv = np.empty(lead + (n, self.dim), np.float32) if variance else None
            if self._channel_axis:
                check(L.wos_solve_channels(self._h, C.byref(params), x.ctypes.data, n, index_base, index_stride, nch,
                                           p.ctypes.data, g.ctypes.data, pv.ctypes.data if variance else None,
                                           gv.ctypes.data if variance else None, ne.ctypes.data if counts else None,
                                           sp.ctypes.data if counts else None, C.byref(st), stream, 0),
                      "wos_solve_channels")
            elif variance:
                check(L.wos_solve_var(self._h, C.byref(params), x.ctypes.data, n, index_base, index_stride,
                                      p.ctypes.data, g.ctypes.data, pv.ctypes.data, gv.ctypes.data,
                                      ne.ctypes.data if counts else None, sp.ctypes.data if counts else None,
                                      C.byref(st), stream, 0), "wos_solve_var")
            else:
                check(L.wos_solve(self._h, C.byref(params), x.ctypes.data, n, index_base, index_stride,
                                  p.ctypes.data, g.ctypes.data, ne.ctypes.data if counts else None,
                                  sp.ctypes.data if counts else None, C.byref(st), stream, 0), "wos_solve")
        out = (p, g, pv, gv, st.as_dict()) if variance else (p, g, st.as_dict())
        if counts:
            out = out + (ne, sp)
        return out

    def query(self, pts, *, which="neumann", boundary_distance_mask=0.0, closest=False, stream=None):
        """Distance, side and solve state of points [N, dim] (wos_scene_query), computed by the
        solve's own device code: (dist [N], signed_dist [N], state [N] int32[, closest [N, dim]]).
        which: "neumann" (the boundary mesh) or "dirichlet" (the optional Dirichlet mesh) -- the
        boundary dist, signed_dist and closest describe.  signed_dist is the solver's: negative on
        the domain side.  state: bit 0 estimated, bit 1 p masked, bit 2 grad masked -- what a solve
        with output.boundaryDistanceMask = boundary_distance_mask gives the point -- and bit 3
        inside the domain (_lib.STATE_*); it takes both boundaries into account whatever `which`.
        numpy in, numpy out (blocking); a torch CUDA tensor in, torch tensors on its device out,
        enqueued on `stream` (a torch.cuda.Stream or a raw hipStream_t; default: torch's current
        stream) without a host synchronisation."""
        w = {"neumann": _lib.QUERY_NEUMANN, "dirichlet": _lib.QUERY_DIRICHLET}.get(which, which)
        if w not in (_lib.QUERY_NEUMANN, _lib.QUERY_DIRICHLET):
            raise WosError(f"WosScene.query: which must be 'neumann' or 'dirichlet', got {which!r}")
        d, sd, cp, state = self._query(pts, w, boundary_distance_mask, (True, True, bool(closest), True), stream)
        return (d, sd, state, cp) if closest else (d, sd, state)

    def query_state(self, pts, boundary_distance_mask=0.0, *, stream=None):
        """query()'s state words alone: needs neither boundary to exist and scans nothing else."""
        return self._query(pts, _lib.QUERY_NEUMANN, boundary_distance_mask, (False, False, False, True), stream)[3]

    def _query(self, pts, which, mask, want, stream):
        """wos_scene_query for the outputs `want` = (dist, signed_dist, closest, state) asks for:
        those four, None where not asked."""
        L = _lib.load()
        mask = float(mask)
        dtypes = ("float32", "float32", "float32", "int32")
        if _is_torch(pts) and pts.is_cuda:
            import torch
            x = pts.detach().to(torch.float32).contiguous()
            if x.ndim != 2 or x.shape[1] != self.dim:
                raise WosError(f"points must be [N,{self.dim}]")
            n = x.shape[0]
            out = [torch.empty((n, self.dim) if k == 2 else (n,), dtype=getattr(torch, dtypes[k]), device=x.device)
                   if want[k] else None for k in range(4)]
            if n == 0:  # empty tensors have null data pointers, which the C ABI reads as "not asked for"
                return tuple(out)
            cur = torch.cuda.current_stream(x.device)
            if stream is None:
                s = cur.cuda_stream
            else:
                ts = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream),
                                                                                                    device=x.device)
                s = ts.cuda_stream
                ts.wait_stream(cur)  # the points and the fresh outputs belong to torch's current stream
                for t in [x] + out:
                    if t is not None:
                        t.record_stream(ts)  # ... and are used on `stream`: the allocator must wait for it
            ptr = [t.data_ptr() if t is not None else None for t in out]
            check(L.wos_scene_query(self._h, which, mask, x.data_ptr(), n, *ptr, s,
                                    _lib.WOS_PTRS_DEVICE | _lib.WOS_ASYNC), "wos_scene_query")
        else:
            if _is_torch(pts):
                pts = pts.detach().cpu().numpy()
            x = np.ascontiguousarray(pts, dtype=np.float32)
            if x.ndim != 2 or x.shape[1] != self.dim:
                raise WosError(f"points must be [N,{self.dim}]")
            n = x.shape[0]
            out = [np.empty((n, self.dim) if k == 2 else (n,), dtypes[k]) if want[k] else None for k in range(4)]
            if n == 0:
                return tuple(out)
            ptr = [a.ctypes.data if a is not None else None for a in out]
            s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
            check(L.wos_scene_query(self._h, which, mask, x.ctypes.data, n, *ptr, s, 0), "wos_scene_query")
        return tuple(out)

    def selftest_geometry(self, kind, items, masks, *, schedule=0, min_star_radius=1e-3, silhouette_precision=1e-3):
        """The walk step's geometry queries on `items`, run by the kernels' own device code on the
        scene planned as a solve under `schedule` plans it (wos_selftest_geometry).  kind: "ray"
        (items [n, 2 dim + 1] = origin, direction, tmax), "star" ([n, dim + 2] = x, maxR, flip) or
        "dirichlet" ([n, dim] = x); masks: one 64-bit lane mask per wave, whose set bits take the
        items in order.  Returns a dict: out float32 [n, 3, 8] (exact scan, per-lane culled form,
        wave-cooperative form), tags int32 [n], sound uint32 [n], counts uint32 [n, 16] (_lib.GEO_*)
        and plan = a dict of how the scene was planned (geom_global, star_grid, dir_grid, lds_bytes,
        ptree / stree / dtree levels, n_silhouettes)."""
        k = {"ray": _lib.GEO_RAY, "star": _lib.GEO_STAR, "dirichlet": _lib.GEO_DIRICHLET}.get(kind, kind)
        width = {_lib.GEO_RAY: 2 * self.dim + 1, _lib.GEO_STAR: self.dim + 2, _lib.GEO_DIRICHLET: self.dim}.get(k, 1)
        x = np.ascontiguousarray(items, dtype=np.float32).reshape(-1, width)
        m = np.ascontiguousarray(masks, dtype=np.uint64).reshape(-1)
        n = x.shape[0]
        out = np.zeros((n, 3, _lib.GEO_OUT), np.float32)
        tags = np.zeros(n, np.int32)
        sound = np.zeros(n, np.uint32)
        counts = np.zeros((n, _lib.GEO_COUNTS), np.uint32)
        plan = np.zeros(8, np.int32)
        check(_lib.load().wos_selftest_geometry(self._h, int(schedule), float(min_star_radius),
                                                float(silhouette_precision), int(k), x.ctypes.data, n, m.ctypes.data,
                                                m.size, out.ctypes.data, tags.ctypes.data, sound.ctypes.data,
                                                counts.ctypes.data, plan.ctypes.data), "wos_selftest_geometry")
        names = ("geom_global", "star_grid", "dir_grid", "lds_bytes", "ptree", "stree", "dtree", "n_silhouettes")
        return {"out": out, "tags": tags, "sound": sound, "counts": counts,
                "plan": {k: int(p) for k, p in zip(names, plan)}}

    def record(self, pts, params=None, *, index_base=0, index_stride=1, max_bytes=None):
        """Record the walks of solve(pts, params, index_base=..., index_stride=...) once
        (wos_tape_record; blocking, about two solves).  The returned WalkTape replays them for
        whatever source this scene holds later, bit for bit the full solve, at the cost of
        streaming the tape.  max_bytes: refuse (WOS_E_CAPACITY) a tape larger than that."""
        L = _lib.load()
        params = params if params is not None else solver_params()
        st = Stats()
        on_dev = _is_torch(pts) and pts.is_cuda
        if on_dev:
            import torch
            x = pts.detach().to(torch.float32).contiguous()
            ptr, flags = x.data_ptr(), _lib.WOS_PTRS_DEVICE
            stream = torch.cuda.current_stream(x.device).cuda_stream
        else:
            if _is_torch(pts):
                pts = pts.detach().cpu().numpy()
            x = np.ascontiguousarray(pts, dtype=np.float32)
            ptr, flags, stream = x.ctypes.data, 0, None
        if x.ndim != 2 or x.shape[1] != self.dim:
            raise WosError(f"points must be [N,{self.dim}]")
        h = C.c_void_p()
        check(L.wos_tape_record(self._h, C.byref(params), ptr, x.shape[0], index_base, index_stride,
                                int(max_bytes) if max_bytes is not None else 0, C.byref(h), C.byref(st), stream,
                                flags), "wos_tape_record")
        return WalkTape(self, h, x.shape[0], x.device if on_dev else None, st.as_dict())

    def bvc(self, params=None, bvc=None, samples=True):
        """Boundary value caching (wos_bvc; the reference's bvc, demo.cpp:265-363) on this
        2D scene (Neumann and Dirichlet boundaries).  Returns (solution [g, g], grad [g, g, 2],
        info) on the evaluation grid (index [i, j] = point (i/g, j/g) of the grid box, masked as
        saveEvaluationGrid masks); info holds the sample counts, the cached samples
        ([k, 8]: x y nx ny pdf value normalDerivative kind, include/wos.h) and the stats."""
        L = _lib.load()
        params = params if params is not None else solver_params()
        if bvc is None:
            raise WosError("bvc parameters required (engine.bvc_params(solver, output))")
        g = int(bvc.grid_res)
        sol = np.empty(g * g, np.float32)
        grad = np.empty(g * g * 2, np.float32)
        counts = np.zeros(4, np.int64)
        st = Stats()
        cap = 0
        buf = None
        if samples:
            cap = 2 * int(bvc.boundary_cache_size) + 4 * int(bvc.domain_cache_size) + 16
            buf = np.empty(cap * 8, np.float32)
        rc = L.wos_bvc(self._h, C.byref(params), C.byref(bvc), sol.ctypes.data, grad.ctypes.data,
                       buf.ctypes.data if samples else None, cap, counts.ctypes.data, C.byref(st))
        if rc == _lib.WOS_E_CAPACITY and samples and int(counts[3]) > cap:
            # the domain sampler keeps more candidates than the first guess (non-watertight
            # scenes, small |signedVolume|): wos_bvc failed before the walks with the exact
            # count in counts[3] -- retry once with a buffer of that size
            cap = int(counts[3])
            buf = np.empty(cap * 8, np.float32)
            rc = L.wos_bvc(self._h, C.byref(params), C.byref(bvc), sol.ctypes.data, grad.ctypes.data,
                           buf.ctypes.data, cap, counts.ctypes.data, C.byref(st))
        check(rc, "wos_bvc")
        info = {"counts": {"boundary": int(counts[0]), "boundary_aligned": int(counts[1]), "domain": int(counts[2]),
                           "total": int(counts[3])}, "stats": st.as_dict()}
        if samples:
            info["samples"] = buf[:int(counts[3]) * 8].reshape(-1, 8).copy()
        return sol.reshape(g, g), grad.reshape(g, g, 2), info

    def solve_stats(self, ticket):
        """Statistics of an enqueued solve (wos_solve_stats); blocks until it has finished."""
        st = Stats()
        check(_lib.load().wos_solve_stats(self._h, int(ticket), C.byref(st)), "wos_solve_stats")
        return st.as_dict()

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().wos_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WalkTape:
    """The recorded walks of one (scene, params, points, indices): WosScene.record.  solve()
    replays them for the scene's current source."""

    def __init__(self, scene, handle, n, torch_device, record_stats):
        self.scene = scene
        self._h = handle
        self._n = int(n)
        self._torch_device = torch_device  # outputs follow the recorded points: torch-CUDA in, torch-CUDA out
        self.record_stats = record_stats

    @property
    def info(self):
        """wos_tape_info as a dict (bytes, n_entries, max_entries_per_walk, replay_chunk_entries, ...)."""
        i = _lib.TapeInfo()
        check(_lib.load().wos_tape_get_info(self._h, C.byref(i)), "wos_tape_get_info")
        out = {n: getattr(i, n) for n, _ in i._fields_ if n != "source_dims"}
        out["source_dims"] = list(i.source_dims)
        return out

    def solve(self, *, variance=False, counts=False, stream=None):
        """The solve of the recorded points for the scene's current source (wos_tape_solve):
        the tuple WosScene.solve(pts, params, variance=..., counts=...) would return now, bit
        for bit, with the recorded walks' counters and this call's times in the stats dict."""
        L = _lib.load()
        sc = self.scene
        st = Stats()
        n, dim = self._n, sc.dim
        nch = sc.channels
        lead = (nch,) if sc._channel_axis else ()
        if self._torch_device is not None:
            import torch
            dev = self._torch_device
            p = torch.empty(lead + (n,), dtype=torch.float32, device=dev)
            g = torch.empty(lead + (n, dim), dtype=torch.float32, device=dev)
            ne = torch.empty(n, dtype=torch.int32, device=dev) if counts else None
            sp = torch.empty(n, dtype=torch.int32, device=dev) if counts else None
            pv = torch.empty(lead + (n,), dtype=torch.float32, device=dev) if variance else None
            gv = torch.empty(lead + (n, dim), dtype=torch.float32, device=dev) if variance else None
            cur = torch.cuda.current_stream(dev)
            if stream is None:
                s = cur.cuda_stream
            else:
                ts = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream),
                                                                                                    device=dev)
                s = ts.cuda_stream
                ts.wait_stream(cur)  # the fresh output buffers belong to torch's current stream
            ptr = lambda t: t.data_ptr() if t is not None else None
            flags = _lib.WOS_PTRS_DEVICE
        else:
            p = np.empty(lead + (n,), np.float32)
            g = np.empty(lead + (n, dim), np.float32)
            ne = np.empty(n, np.int32) if counts else None
            sp = np.empty(n, np.int32) if counts else None
            pv = np.empty(lead + (n,), np.float32) if variance else None
            gv = np.empty(lead + (n, dim), np.float32) if variance else None
            ptr = lambda a: a.ctypes.data if a is not None else None
            s, flags = stream, 0
        check(L.wos_tape_solve(self._h, sc._h, nch, ptr(p), ptr(g), ptr(pv), ptr(gv), ptr(ne), ptr(sp), C.byref(st),
                               s, flags), "wos_tape_solve")
        out = (p, g, pv, gv, st.as_dict()) if variance else (p, g, st.as_dict())
        if counts:
            out = out + (ne, sp)
        return out

    def build_index(self, max_bytes=None):
        """Build the tape's cell-sorted index (wos_tape_index_build; blocking, once per tape: a
        second call does nothing), which vjp(..., deterministic=True) sums over.  max_bytes:
        refuse (WOS_E_CAPACITY) a build whose index and sort scratch need more device memory;
        the tape then stays as it was."""
        check(_lib.load().wos_tape_index_build(self._h, int(max_bytes) if max_bytes else 0), "wos_tape_index_build")

    @property
    def index_info(self):
        """wos_tape_index_info as a dict: built, n_segments, n_terms, n_cells, max_terms_per_cell,
        bytes, tile_terms."""
        i = _lib.TapeIndexInfo()
        check(_lib.load().wos_tape_index_get_info(self._h, C.byref(i)), "wos_tape_index_get_info")
        return {n: int(getattr(i, n)) for n, _ in i._fields_}

    def read_index(self, field, segment=0):
        """One array of one segment's index as numpy (wos_tape_index_read): row [cells + 1], and
        per term, sorted stably by cell, id (task | bit 31: the first-ball term), w and cell."""
        L = _lib.load()
        if field not in _lib.TAPE_INDEX_FIELDS:
            raise WosError(f"WalkTape.read_index: unknown field {field!r} (one of {', '.join(_lib.TAPE_INDEX_FIELDS)})")
        fid, dtype = _lib.TAPE_INDEX_FIELDS[field]
        cells = self.index_info["n_cells"]
        row = np.empty(cells + 1, "u4")
        check(L.wos_tape_index_read(self._h, segment, _lib.TAPE_INDEX_FIELDS["row"][0], 0, row.size, row.ctypes.data),
              "wos_tape_index_read")
        if field == "row":
            return row
        out = np.empty(int(row[-1]), dtype)
        check(L.wos_tape_index_read(self._h, segment, fid, 0, out.size, out.ctypes.data), "wos_tape_index_read")
        return out

    def vjp(self, grad_p=None, grad_grad=None, *, stream=None, deterministic=False):
        """The transpose of solve() applied to an upstream (wos_tape_vjp): the gradient with
        respect to the scene's source grid of a loss whose derivatives by solve()'s p and grad
        are grad_p and grad_grad (shaped like them; one may be None: zeros).  Returns an array
        of the scene's source_shape -- numpy for numpy input, a torch-CUDA tensor for torch-CUDA
        input.  It depends neither on the current source values nor on dirichlet_values;
        upstream values of masked outputs and of points without an estimate are ignored.
        deterministic=False: the sums are float atomics (wos_tape_vjp), two calls may differ in
        the last bits.  deterministic=True: the sums run over the tape's cell-sorted index in a
        fixed order, without atomics (wos_tape_vjp_indexed): every call on this tape, and on a
        tape recorded from the same inputs in the same batches, returns the same bits; the
        index is built on first use (build_index).  last_vjp_stats holds the call's statistics
        (fold_ms: the adjoint fold, walk_ms: the scatter or the sum kernels)."""
        L = _lib.load()
        sc = self.scene
        if grad_p is None and grad_grad is None:
            raise WosError("WalkTape.vjp: grad_p and grad_grad are both None")
        n, dim = self._n, sc.dim
        nch = sc.channels
        lead = (nch,) if sc._channel_axis else ()
        shapes = (lead + (n,), lead + (n, dim))
        for u, shp, name in ((grad_p, shapes[0], "grad_p"), (grad_grad, shapes[1], "grad_grad")):
            if u is not None and tuple(u.shape) != shp:
                raise WosError(f"WalkTape.vjp: {name} must have shape {shp}, got {tuple(u.shape)}")
        if sc.source_shape is None:
            raise WosError("WalkTape.vjp: the scene has no source grid")
        on_dev = any(_is_torch(u) and u.is_cuda for u in (grad_p, grad_grad))
        st = Stats()
        if on_dev:
            import torch
            dev = next(u.device for u in (grad_p, grad_grad) if _is_torch(u) and u.is_cuda)
            up = [None if u is None else torch.as_tensor(u).detach().to(dev, torch.float32).contiguous()
                  for u in (grad_p, grad_grad)]
            out = torch.empty(sc.source_shape, dtype=torch.float32, device=dev)
            cur = torch.cuda.current_stream(dev)
            if stream is None:
                s = cur.cuda_stream
            else:
                ts = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(int(stream),
                                                                                                    device=dev)
                s = ts.cuda_stream
                ts.wait_stream(cur)  # the upstream and the fresh output belong to torch's current stream
            ptr = lambda t: t.data_ptr() if t is not None else None
            flags = _lib.WOS_PTRS_DEVICE
        else:
            up = [None if u is None else np.ascontiguousarray(u.detach().cpu().numpy() if _is_torch(u) else u,
                                                              dtype=np.float32) for u in (grad_p, grad_grad)]
            out = np.empty(sc.source_shape, np.float32)
            ptr = lambda a: a.ctypes.data if a is not None else None
            s, flags = stream, 0
        if deterministic:
            self.build_index()
        fn = "wos_tape_vjp_indexed" if deterministic else "wos_tape_vjp"
        check(getattr(L, fn)(self._h, sc._h, nch, ptr(up[0]), ptr(up[1]), ptr(out), C.byref(st), s, flags), fn)
        self.last_vjp_stats = st.as_dict()
        return out

    def read(self, field, segment=0):
        """One array of one segment of the tape as numpy (wos_tape_read; one segment per recorded
        batch): per task code, cnt, cell0, gnorm, thr_end, term, tneu [T], slot [T + 1], bdir,
        sdir [dim, T]; per entry slot cell, thr, nrm [slot[T]]; per point pstate.  A diagnostic:
        with it the replay, the fold and their transpose can be restated on the host."""
        L = _lib.load()
        if field not in _lib.TAPE_FIELDS:
            raise WosError(f"WalkTape.read: unknown field {field!r} (one of {', '.join(_lib.TAPE_FIELDS)})")
        fid, dtype = _lib.TAPE_FIELDS[field]
        npts = np.zeros(1, np.int64)
        check(L.wos_tape_read(self._h, segment, _lib.TAPE_SEGMENT_POINTS, 0, 1, npts.ctypes.data), "wos_tape_read")
        info = self.info
        T = int(npts[0]) * (info["n_tasks"] // max(1, info["n_points"]))
        dim = info["dim"]
        if field in ("cell", "thr", "nrm"):
            last = np.zeros(1, np.uint32)
            check(L.wos_tape_read(self._h, segment, _lib.TAPE_FIELDS["slot"][0], T, 1, last.ctypes.data), "wos_tape_read")
            shape = (int(last[0]),)
        else:
            shape = {"slot": (T + 1,), "bdir": (dim, T), "sdir": (dim, T), "pstate": (int(npts[0]),)}.get(field, (T,))
        out = np.empty(shape, dtype)
        check(L.wos_tape_read(self._h, segment, fid, 0, out.size, out.ctypes.data), "wos_tape_read")
        return out

    @property
    def segments(self):
        """Point counts of the tape's segments (one per recorded batch), in order."""
        L = _lib.load()
        out, npts = [], np.zeros(1, np.int64)
        while sum(out) < self._n:
            check(L.wos_tape_read(self._h, len(out), _lib.TAPE_SEGMENT_POINTS, 0, 1, npts.ctypes.data), "wos_tape_read")
            out.append(int(npts[0]))
        return out

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().wos_tape_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def release_caches(device=-1):
    """Free the per-device solve workspace and the cached prepared geometries
    (wos_release_caches); live scenes stay valid."""
    check(_lib.load().wos_release_caches(int(device)), "wos_release_caches")


def set_max_batch_tasks(n):
    """Walk tasks per batch (wos_set_max_batch_tasks; n <= 0: the default 2^28).  Returns the
    previous value.  Results do not depend on it; it bounds the per-device workspace."""
    return int(_lib.load().wos_set_max_batch_tasks(int(n)))


def set_length_hints(hint_min=-1, express_min=-1, express_per_wave=-1, capacity=-1, priority=-1):
    """Tunables of the length hints (wos_set_length_hints; a negative value: that one's default).  Scheduling
    only: results never depend on them."""
    _lib.load().wos_set_length_hints(int(hint_min), int(express_min), int(express_per_wave), int(capacity),
                                     int(priority))


def length_hint_stats(device=0):
    """Of the last solve on `device` (waits for it): express walks started, walks the list had no room for,
    walks listed, entries of the express list it ran with (wos_length_hint_stats)."""
    out = (C.c_int64 * 4)()
    check(_lib.load().wos_length_hint_stats(int(device), out), "wos_length_hint_stats")
    return {"claimed": int(out[0]), "overflow": int(out[1]), "listed": int(out[2]), "express": int(out[3])}


def set_express_layout(solo_min=-1, stripe=-1, placement=-1):
    """Which wave starts which express walk (wos_set_express_layout; a negative value: that one's default): walks
    of >= solo_min steps a wave each (0: none), the others striped over the waves (1) or in blocks of the sorted
    list (0), the express wave of a workgroup rotating (0) or pinned to its lowest SIMD (1).  Scheduling only."""
    _lib.load().wos_set_express_layout(int(solo_min), int(stripe), int(placement))


def express_layout():
    """The express layout in force (wos_get_express_layout)."""
    out = (C.c_int32 * 3)()
    _lib.load().wos_get_express_layout(out)
    return {"solo_min": int(out[0]), "stripe": int(out[1]), "placement": int(out[2])}


def express_layout_stats(device=0):
    """Of the last solve on `device` (waits for it): the entries of its solo tier and the claims its other express
    entries went to (wos_express_layout_stats)."""
    out = (C.c_int64 * 2)()
    check(_lib.load().wos_express_layout_stats(int(device), out), "wos_express_layout_stats")
    return {"solo": int(out[0]), "claims_below": int(out[1])}


def selftest_express_slot(nx, express_per_wave, stripe):
    """The layout's table for a list of nx entries (host only; wos_selftest_express_slot): rows (n_solo, claim, j,
    entry) over every solo tier 0..nx, every claim 0..nx+1 and j 0..express_per_wave+1 that holds an entry."""
    L = _lib.load()
    rows = int(L.wos_selftest_express_slot(int(nx), int(express_per_wave), int(stripe), None, 0))
    out = np.empty((rows, 4), np.uint32)
    got = int(L.wos_selftest_express_slot(int(nx), int(express_per_wave), int(stripe), out.ctypes.data, rows))
    assert got == rows
    return out


def selftest_simd_ids(device=0):
    """Of one 256-thread workgroup: the SIMD of each wave as the walk kernel reads it, and each wave's whole
    hardware id register (wos_selftest_simd_ids)."""
    out = (C.c_uint32 * 8)()
    check(_lib.load().wos_selftest_simd_ids(int(device), out), "wos_selftest_simd_ids")
    return [int(v) for v in out[:4]], [int(v) for v in out[4:]]


def selftest_hint_key():
    """Per field of the hint key (host only): does a difference in it alone make two keys unequal?"""
    res = []
    while True:
        r = int(_lib.load().wos_selftest_hint_key(len(res)))
        if r < 0:
            return res
        res.append(bool(r))


def selftest_math(which, x, device=0):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    check(_lib.load().wos_selftest_math(which, x.ctypes.data, out.ctypes.data, x.size, device),
          "wos_selftest_math")
    return out


def selftest_rejection(dim, R, lam, x, device=0):
    """The rejection sampler's decision functions on the balls (R, lam) at the radius draws
    x R, run by the kernels' own device code (wos_selftest_rejection).  Returns the edges
    int32 [n, 6] = (a, r0, e, e3, q, xr) over the draws u_k = k 2^-23, vals float32 [n, 3] =
    (norm, bound, 1 / (norm bound)) and the shape flags int32 [n]."""
    R = np.ascontiguousarray(R, dtype=np.float32).reshape(-1)
    lam = np.ascontiguousarray(lam, dtype=np.float32).reshape(-1)
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    if not (R.size == lam.size == x.size):
        raise WosError("R, lam and x must have one length")
    edges = np.empty((R.size, 6), np.int32)
    vals = np.empty((R.size, 3), np.float32)
    flags = np.empty(R.size, np.int32)
    check(_lib.load().wos_selftest_rejection(int(dim), R.ctypes.data, lam.ctypes.data, x.ctypes.data, R.size,
                                             edges.ctypes.data, vals.ctypes.data, flags.ctypes.data, device),
          "wos_selftest_rejection")
    return edges, vals, flags


def selftest_gfn(dim, mode, items, device=0):
    """The Green's-function members of the ball and the 2D free-space functions on items
    float32 [n, GFN_ITEM], run by the kernels' own device code (wos_selftest_gfn; layouts in
    include/wos.h).  mode 0 harmonic, 1 Yukawa, 2 Yukawa robust.  Returns float32 [n, GFN_OUT]."""
    items = np.ascontiguousarray(items, dtype=np.float32).reshape(-1, _lib.GFN_ITEM)
    out = np.zeros((items.shape[0], _lib.GFN_OUT), np.float32)
    check(_lib.load().wos_selftest_gfn(int(dim), int(mode), items.ctypes.data, items.shape[0], out.ctypes.data,
                                       device), "wos_selftest_gfn")
    return out


def selftest_sample_volume(dim, items, seeds, masks, *, fb=False, rb=False, need_pdf=False, device=0):
    """The source sample on items float32 [n, SV_ITEM] with stream seeds uint32 [n], wave w of the probe
    under lane mask masks[w] (uint64), run by the kernels' own device code (wos_selftest_sample_volume;
    layouts in include/wos.h): sample_volume_wave<dim, rb, fb> as shipped (form 0) beside the sequential
    sample_volume (form 1).  Returns a dict: r, pdf float32 [n, 2], out float32 [n, 2, 3], state uint64
    [n, 2], iters uint32 [n, 2], tags int32 [n], canary uint32 [len(masks), 64] and plan (SV_PLAN)."""
    items = np.ascontiguousarray(items, dtype=np.float32).reshape(-1, _lib.SV_ITEM)
    seeds = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
    masks = np.ascontiguousarray(masks, dtype=np.uint64).reshape(-1)
    n = items.shape[0]
    if seeds.size != n:
        raise WosError("items and seeds must have one length")
    out = np.zeros((n, 2, _lib.SV_OUT), np.float32)
    state = np.zeros((n, 2), np.uint64)
    iters = np.zeros((n, 2), np.uint32)
    tags = np.zeros(n, np.int32)
    canary = np.zeros((masks.size, 64), np.uint32)
    plan = np.zeros(8, np.int32)
    variant = (_lib.SV_FB if fb else 0) | (_lib.SV_RB if rb else 0)
    check(_lib.load().wos_selftest_sample_volume(int(dim), variant, int(bool(need_pdf)), items.ctypes.data,
                                                 seeds.ctypes.data, n, masks.ctypes.data, masks.size,
                                                 out.ctypes.data, state.ctypes.data, iters.ctypes.data,
                                                 tags.ctypes.data, canary.ctypes.data, plan.ctypes.data, device),
          "wos_selftest_sample_volume")
    return {"r": out[:, :, 0], "pdf": out[:, :, 1], "out": out[:, :, 2:5], "state": state, "iters": iters,
            "tags": tags, "canary": canary, "plan": dict(zip(_lib.SV_PLAN, (int(v) for v in plan)))}


def selftest_lhs(key, gidx, n_pairs, dim, jump_lds=True, device=0):
    """The first-ball kernel's stratified samples of the point indices gidx, built by the
    kernel's own device code (wos_selftest_lhs): float32 [n, 2 n_pairs, dim - 1]."""
    gidx = np.ascontiguousarray(gidx, dtype=np.int64).reshape(-1)
    out = np.empty((gidx.size, 2 * int(n_pairs), int(dim) - 1), np.float32)
    check(_lib.load().wos_selftest_lhs(int(key), gidx.ctypes.data, gidx.size, int(n_pairs), int(dim),
                                       int(bool(jump_lds)), out.ctypes.data, device), "wos_selftest_lhs")
    return out


def selftest_lhs_permute_slots(impl):
    """Slots a table of wos_selftest_lhs_permute holds for shuffle implementation impl."""
    return 2 if impl == _lib.LHS_PACK_R1 else 1


def selftest_lhs_permute(impl, partner, values, slots=1, device=0):
    """One shuffle implementation (_lib.LHS_*) of the stratified sampler on caller-supplied
    tables (wos_selftest_lhs_permute).  partner: int32 [count, cap, sd, nstrat], values: float32
    [count, cap, nstrat, sd] with cap = selftest_lhs_permute_slots(impl); the first `slots`
    slots of every table are shuffled.  Returns the values after `for i: for j: swap(a[j, i],
    a[partner[i][j], i])`, shaped like values."""
    partner = np.ascontiguousarray(partner, dtype=np.int32)
    values = np.ascontiguousarray(values, dtype=np.float32)
    cap = selftest_lhs_permute_slots(impl)
    if partner.ndim != 4 or values.ndim != 4 or partner.shape[1] != cap or \
            values.shape != (partner.shape[0], cap, partner.shape[3], partner.shape[2]):
        raise WosError(f"partner must be [count, {cap}, sd, nstrat] and values [count, {cap}, nstrat, sd]")
    count, _, sd, nstrat = partner.shape
    out = np.empty_like(values)
    check(_lib.load().wos_selftest_lhs_permute(int(impl), partner.ctypes.data, values.ctypes.data, nstrat, sd,
                                               int(slots), count, out.ctypes.data, device),
          "wos_selftest_lhs_permute")
    return out


def selftest_lhs_plan(n_pairs, dim):
    """What the kernels' constants select for the stratified samples of n_pairs pairs
    (wos_selftest_lhs_plan; host only): a dict."""
    out = np.zeros(9, np.int32)
    check(_lib.load().wos_selftest_lhs_plan(int(n_pairs), int(dim), out.ctypes.data), "wos_selftest_lhs_plan")
    keys = ("points_per_wave", "one_pass", "shuffle", "pair_passes", "jump_mixed", "wave_lds_bytes", "lds_budget",
            "point_grab", "shuffle_chunks")
    return {k: int(v) for k, v in zip(keys, out)}


def selftest_tape_rowsum(row, id, w, a, c, device=0):
    """The indexed adjoint's sum kernels on a hand-built index (wos_selftest_tape_rowsum): row
    [n_rows + 1] offsets, id / w per term, a / c [C, T] (or [T]: one channel).  Returns
    (out float32 [C, n_rows] or [n_rows], the tile constant)."""
    row = np.ascontiguousarray(row, dtype=np.uint32)
    id = np.ascontiguousarray(id, dtype=np.uint32)
    w = np.ascontiguousarray(w, dtype=np.float32)
    a = np.ascontiguousarray(a, dtype=np.float32)
    c = np.ascontiguousarray(c, dtype=np.float32)
    if a.shape != c.shape or a.ndim not in (1, 2) or id.shape != w.shape or row.ndim != 1 or row.size < 2:
        raise WosError("selftest_tape_rowsum: row [n_rows + 1], id / w [n_terms], a / c [C, T] or [T]")
    nch = 1 if a.ndim == 1 else a.shape[0]
    if id.size != int(row[-1]):
        raise WosError(f"selftest_tape_rowsum: {id.size} terms, row[-1] = {int(row[-1])}")
    out = np.empty((nch, row.size - 1), np.float32)
    tile = C.c_int32(0)
    check(_lib.load().wos_selftest_tape_rowsum(row.ctypes.data, row.size - 1, id.ctypes.data, w.ctypes.data,
                                               a.ctypes.data, c.ctypes.data, a.shape[-1], nch, out.ctypes.data,
                                               C.byref(tile), device), "wos_selftest_tape_rowsum")
    return (out[0] if a.ndim == 1 else out), int(tile.value)


def device_count():
    return int(_lib.load().wos_device_count())
