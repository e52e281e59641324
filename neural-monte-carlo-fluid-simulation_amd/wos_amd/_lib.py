"""ctypes binding of the C ABI in include/wos.h (lib/libwos_hip.so).

The product path: every solve goes through libwos_hip.so's HIP kernel.  There is
no CPU fallback -- if the library cannot be loaded the import fails loudly.
"""
import ctypes as C
import os

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("WOS_LIB_PATH") or os.path.join(PKG_DIR, "lib", "libwos_hip.so")

ABI_VERSION = 10  # include/wos.h WOS_ABI_VERSION this binding's structs mirror
WOS_OK = 0
WOS_E_CAPACITY = -4
WOS_PTRS_DEVICE = 0x1
WOS_ASYNC = 0x2
WOS_FIT_SCALE_MATRIX = 0x4  # wos_siren_fit and the fit loops: scale is [rows][d_out][d_out]
MAX_CHANNELS = 4  # include/wos.h WOS_MAX_CHANNELS
# include/wos.h WOS_LHS_*: the stratified sampler's shuffles (wos_selftest_lhs_permute, wos_selftest_lhs_plan)
LHS_REG1, LHS_REG2, LHS_LDS, LHS_PACK_R1, LHS_PACK_R2, LHS_SERIAL = range(6)


class WosError(RuntimeError):
    pass


class Mesh(C.Structure):
    _fields_ = [("dim", C.c_int32), ("n_vertices", C.c_int32), ("n_prims", C.c_int32),
                ("vertices", C.POINTER(C.c_float)), ("prims", C.POINTER(C.c_int32))]


class SceneDesc(C.Structure):
    _fields_ = [
        ("dim", C.c_int32),
        ("vertices", C.POINTER(C.c_float)), ("prims", C.POINTER(C.c_int32)),
        ("n_vertices", C.c_int32), ("n_prims", C.c_int32),
        ("dvertices", C.POINTER(C.c_float)), ("dprims", C.POINTER(C.c_int32)),
        ("n_dvertices", C.c_int32), ("n_dprims", C.c_int32),
        ("dirichlet_value", C.c_float), ("absorption", C.c_float),
        ("is_watertight", C.c_int32), ("is_double_sided", C.c_int32),
        ("source", C.c_void_p), ("source_dims", C.c_int32 * 3), ("source_on_device", C.c_int32),
        ("dirichlet_image", C.c_void_p), ("dirichlet_image_dims", C.c_int32 * 2),
        ("dirichlet_image_box", C.c_float * 4), ("dirichlet_image_on_device", C.c_int32),
        ("neumann_image", C.c_void_p), ("neumann_image_dims", C.c_int32 * 2),
        ("neumann_image_box", C.c_float * 4), ("neumann_image_on_device", C.c_int32),
    ]


class SceneInfo(C.Structure):
    _fields_ = [("dim", C.c_int32), ("n_prims", C.c_int32), ("n_silhouettes", C.c_int32),
                ("n_dprims", C.c_int32), ("device", C.c_int32),
                ("bbox_min", C.c_float * 3), ("bbox_max", C.c_float * 3)]


class SolverParams(C.Structure):
    _fields_ = [
        ("n_walks", C.c_int32), ("max_walk_length", C.c_int32),
        ("steps_before_tikhonov", C.c_int32), ("steps_before_maximal_spheres", C.c_int32),
        ("epsilon_shell", C.c_float), ("min_star_radius", C.c_float),
        ("silhouette_precision", C.c_float), ("russian_roulette_threshold", C.c_float),
        ("boundary_distance_mask", C.c_float),
        ("disable_gradient_control_variates", C.c_int32),
        ("disable_gradient_antithetic_variates", C.c_int32),
        ("use_cosine_sampling", C.c_int32), ("ignore_dirichlet", C.c_int32),
        ("ignore_neumann", C.c_int32), ("ignore_source", C.c_int32),
        ("seed", C.c_uint64),
        ("robust_float", C.c_int32),
        ("schedule", C.c_uint32),
    ]


# wos_solver_params.schedule bits (include/wos.h): scheduling only, results bit-identical
SCHED_GEOM_GLOBAL = 0x1
SCHED_FULL_NEUMANN = 0x2
SCHED_NO_STAR_GRID = 0x4
SCHED_NO_DIR_GRID = 0x8
SCHED_NO_TAIL_SPREAD = 0x10
SCHED_NO_GRID_SPREAD = 0x20  # reserved: no effect (include/wos.h)
SCHED_NO_LENGTH_HINTS = 0x40


class BvcParams(C.Structure):
    _fields_ = [("n_walks_solution", C.c_int32), ("n_walks_gradient", C.c_int32),
                ("boundary_cache_size", C.c_int32), ("domain_cache_size", C.c_int32),
                ("grid_res", C.c_int32), ("use_finite_differences", C.c_int32),
                ("normal_offset", C.c_float), ("radius_clamp", C.c_float),
                ("kernel_regularization", C.c_float), ("grid_box", C.c_float * 4)]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "walk_steps", "wasted_steps", "walks_recorded", "walks_escaped", "walks_max_length",
        "walks_rr", "walks_dirichlet", "points_estimated", "rejection_iters")] + [
        (n, C.c_double) for n in ("kernel_ms", "first_ball_ms", "walk_ms", "fold_ms")] + [("walk_launches", C.c_uint64)] + [
        (n, C.c_int32) for n in ("first_ball_blocks_per_cu", "walk_blocks_per_cu", "walk_lds_bytes", "star_grid",
                                 "geom_global", "dir_grid")] + [("ticket", C.c_uint64)]

    def as_dict(self):
        return {n: (float(getattr(self, n)) if t is C.c_double else int(getattr(self, n))) for n, t in self._fields_}


class TapeInfo(C.Structure):
    _fields_ = [("dim", C.c_int32), ("n_walks", C.c_int32), ("source_dims", C.c_int32 * 3), ("device", C.c_int32),
                ("n_points", C.c_int64), ("n_tasks", C.c_int64), ("n_entries", C.c_int64),
                ("max_entries_per_walk", C.c_int64), ("bytes", C.c_int64), ("replay_chunk_entries", C.c_int32)]


class TapeIndexInfo(C.Structure):
    _fields_ = [("built", C.c_int32), ("n_segments", C.c_int32), ("n_terms", C.c_int64), ("n_cells", C.c_int64),
                ("max_terms_per_cell", C.c_int64), ("bytes", C.c_int64), ("tile_terms", C.c_int32)]


class SirenNet(C.Structure):
    """wos_siren_net: weights / biases are host arrays of n_hidden_layers + 2 pointers."""
    _fields_ = [("d_in", C.c_int32), ("d_out", C.c_int32), ("hidden", C.c_int32), ("n_hidden_layers", C.c_int32),
                ("omega", C.c_float), ("weights", C.POINTER(C.c_void_p)), ("biases", C.POINTER(C.c_void_p))]


class AdamParams(C.Structure):
    """wos_adam_params: doubles, as torch.optim.Adam holds them; max_grad_norm <= 0: no clipping."""
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double),
                ("max_grad_norm", C.c_double)]


# exported symbols, exactly those declared in include/wos.h
EXPORTS = (
    "wos_load_obj", "wos_mesh_free", "wos_scene_create", "wos_scene_destroy",
    "wos_scene_get_info", "wos_scene_set_source", "wos_release_caches", "wos_default_params", "wos_solve", "wos_solve_var",
    "wos_solve_stats", "wos_default_bvc_params", "wos_bvc",
    "wos_selftest_math", "wos_selftest_lhs", "wos_selftest_lhs_permute", "wos_selftest_lhs_plan", "wos_last_error", "wos_abi_version", "wos_device_count", "wos_set_max_batch_tasks",
    "wos_scene_set_source_channels", "wos_scene_channels", "wos_solve_channels",
    "wos_tape_record", "wos_tape_solve", "wos_tape_get_info", "wos_tape_destroy",
    "wos_tape_vjp", "wos_tape_read",
    "wos_tape_index_build", "wos_tape_index_get_info", "wos_tape_index_read", "wos_tape_vjp_indexed",
    "wos_selftest_tape_rowsum", "wos_selftest_rejection", "wos_selftest_geometry", "wos_selftest_gfn",
    "wos_selftest_sample_volume",
    "wos_scene_query",
    "wos_siren_eval", "wos_selftest_siren_layer",
    "wos_siren_vjp", "wos_selftest_siren_vjp_layer",
    "wos_siren_fit",
    "wos_adam_step", "wos_siren_fit_run", "wos_siren_fit_run_batches",
    "wos_siren_fit_run_ensemble", "wos_siren_fit_run_batches_ensemble",
    "wos_set_length_hints", "wos_length_hint_stats", "wos_selftest_hint_key",
    "wos_set_express_layout", "wos_get_express_layout", "wos_express_layout_stats", "wos_selftest_express_slot", "wos_selftest_simd_ids",
)

# include/wos.h WOS_GFN_*: wos_selftest_gfn's modes and its item and result widths
GFN_HARMONIC, GFN_YUKAWA, GFN_ROBUST = 0, 1, 2
GFN_ITEM, GFN_OUT = 20, 32

# include/wos.h WOS_SV_*: wos_selftest_sample_volume's variant bits, widths, regime tags and canary bits
SV_FB, SV_RB = 1, 2
SV_ITEM, SV_OUT = 9, 5
SV_FALLBACK, SV_SOLO, SV_SPARSE, SV_DENSE_OWN, SV_DENSE_COOP = range(5)
SV_PUBLISHED = 0x100
SV_CANARY = {"ball": 0x1, "stream": 0x2, "pdf": 0x4, "out": 0x8, "iters": 0x10}
# plan[k] of wos_selftest_sample_volume
SV_PLAN = ("wave", "bmin", "bcap", "own", "own_min", "jump_lds", "limit", "block")

# include/wos.h WOS_GEO_*: wos_selftest_geometry's kinds, regime tags, soundness bits and count slots
GEO_RAY, GEO_STAR, GEO_DIRICHLET = 0, 1, 2
GEO_OUT, GEO_COUNTS = 8, 16
GEO_RAY_NONE, GEO_RAY_LANE_SCAN, GEO_RAY_SOLO, GEO_RAY_LIST, GEO_RAY_TREE = range(5)
GEO_STAR_NONE, GEO_STAR_SOLO_CELL, GEO_STAR_CELL_LISTS, GEO_STAR_GROUPS, GEO_STAR_TREE = range(5)
GEO_STAR_MIXED = 0x100
GEO_DIR_NONE, GEO_DIR_GRID, GEO_DIR_GRID_MISS, GEO_DIR_SOLO, GEO_DIR_CULLED, GEO_DIR_TREE = range(6)
GEO_SOUND = {"ray_box": 0x1, "ray_prefilter": 0x2, "ball_box": 0x4, "cone": 0x8, "class2": 0x10,
             "star_early": 0x20, "star_cell": 0x40, "dir_box": 0x80, "dir_cell": 0x100}
# counts[:, slot] fired, counts[:, slot + 1] declined
GEO_COUNT = {"ray_box": 0, "ray_prefilter": 2, "ball_box": 4, "cone": 6, "star_early": 8, "dir_box": 10}
GEO_C_CLASS, GEO_C_CELL_LEN = 12, 15

# include/wos.h WOS_QUERY_*: the boundary wos_scene_query's dist / signed_dist / closest describe
QUERY_NEUMANN, QUERY_DIRICHLET = 0, 1
# wos_scene_query's state word: WOS_TAPE_PSTATE's bits 0-2, bit 3 insideDomain
STATE_ESTIMATED, STATE_MASK_P, STATE_MASK_GRAD, STATE_INSIDE = 1, 2, 4, 8

# wos_tape_field (include/wos.h): the arrays wos_tape_read copies out, with their element types
TAPE_FIELDS = {"code": (0, "u4"), "cnt": (1, "u4"), "slot": (2, "u4"), "cell0": (3, "u4"), "gnorm": (4, "f4"),
               "thr_end": (5, "f4"), "term": (6, "f4"), "tneu": (7, "f4"), "bdir": (8, "f4"), "sdir": (9, "f4"),
               "cell": (10, "u4"), "thr": (11, "f4"), "nrm": (12, "f4"), "pstate": (13, "i4")}
TAPE_SEGMENT_POINTS = 14
# wos_tape_index_field (include/wos.h): the arrays wos_tape_index_read copies out
TAPE_INDEX_FIELDS = {"row": (0, "u4"), "id": (1, "u4"), "w": (2, "f4"), "cell": (3, "u4")}

_lib = None


def load():
    """Load libwos_hip.so (raises if it is missing -- no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise WosError(f"{LIB_PATH} not built: run `make -C {PKG_DIR}` or __graft_entry__.build()")
    L = C.CDLL(LIB_PATH)
    L.wos_load_obj.restype = C.c_int
    L.wos_load_obj.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Mesh)]
    L.wos_mesh_free.restype = None
    L.wos_mesh_free.argtypes = [C.POINTER(Mesh)]
    L.wos_scene_create.restype = C.c_int
    L.wos_scene_create.argtypes = [C.POINTER(SceneDesc), C.c_int32, C.POINTER(C.c_void_p)]
    L.wos_scene_destroy.restype = C.c_int
    L.wos_scene_destroy.argtypes = [C.c_void_p]
    L.wos_scene_get_info.restype = C.c_int
    L.wos_scene_get_info.argtypes = [C.c_void_p, C.POINTER(SceneInfo)]
    L.wos_scene_set_source.restype = C.c_int
    L.wos_scene_set_source.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_void_p]
    L.wos_scene_query.restype = C.c_int
    L.wos_scene_query.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.wos_release_caches.restype = C.c_int
    L.wos_release_caches.argtypes = [C.c_int32]
    L.wos_set_max_batch_tasks.restype = C.c_int64
    L.wos_set_max_batch_tasks.argtypes = [C.c_int64]
    # additive within ABI 10: a library built before the length hints (an A/B against WOS_LIB_PATH) lacks them
    if hasattr(L, "wos_set_length_hints"):
        L.wos_set_length_hints.restype = None
        L.wos_set_length_hints.argtypes = [C.c_int32] * 5
        L.wos_length_hint_stats.restype = C.c_int
        L.wos_length_hint_stats.argtypes = [C.c_int32, C.POINTER(C.c_int64)]
        L.wos_selftest_hint_key.restype = C.c_int32
        L.wos_selftest_hint_key.argtypes = [C.c_int32]
    # ... and one built before the express layout
    if hasattr(L, "wos_set_express_layout"):
        L.wos_set_express_layout.restype = None
        L.wos_set_express_layout.argtypes = [C.c_int32] * 3
        L.wos_get_express_layout.restype = None
        L.wos_get_express_layout.argtypes = [C.POINTER(C.c_int32)]
        L.wos_express_layout_stats.restype = C.c_int
        L.wos_express_layout_stats.argtypes = [C.c_int32, C.POINTER(C.c_int64)]
        L.wos_selftest_express_slot.restype = C.c_int64
        L.wos_selftest_express_slot.argtypes = [C.c_uint32, C.c_uint32, C.c_int32, C.c_void_p, C.c_int64]
        L.wos_selftest_simd_ids.restype = C.c_int
        L.wos_selftest_simd_ids.argtypes = [C.c_int32, C.POINTER(C.c_uint32)]
    L.wos_default_params.restype = None
    L.wos_default_params.argtypes = [C.POINTER(SolverParams)]
    L.wos_solve.restype = C.c_int
    L.wos_solve.argtypes = [C.c_void_p, C.POINTER(SolverParams), C.c_void_p, C.c_int64, C.c_int64,
                            C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                            C.POINTER(Stats), C.c_void_p, C.c_uint32]
    L.wos_solve_var.restype = C.c_int
    L.wos_solve_var.argtypes = [C.c_void_p, C.POINTER(SolverParams), C.c_void_p, C.c_int64, C.c_int64,
                                C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.POINTER(Stats), C.c_void_p, C.c_uint32]
    L.wos_scene_set_source_channels.restype = C.c_int
    L.wos_scene_set_source_channels.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32),
                                                C.POINTER(C.c_float), C.c_int32, C.c_void_p]
    L.wos_scene_channels.restype = C.c_int32
    L.wos_scene_channels.argtypes = [C.c_void_p]
    L.wos_solve_channels.restype = C.c_int
    L.wos_solve_channels.argtypes = [C.c_void_p, C.POINTER(SolverParams), C.c_void_p, C.c_int64, C.c_int64,
                                     C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.POINTER(Stats), C.c_void_p, C.c_uint32]
    L.wos_solve_stats.restype = C.c_int
    L.wos_solve_stats.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(Stats)]
    L.wos_tape_record.restype = C.c_int
    L.wos_tape_record.argtypes = [C.c_void_p, C.POINTER(SolverParams), C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                  C.c_int64, C.POINTER(C.c_void_p), C.POINTER(Stats), C.c_void_p, C.c_uint32]
    L.wos_tape_solve.restype = C.c_int
    L.wos_tape_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.POINTER(Stats), C.c_void_p, C.c_uint32]
    L.wos_tape_get_info.restype = C.c_int
    L.wos_tape_get_info.argtypes = [C.c_void_p, C.POINTER(TapeInfo)]
    L.wos_tape_destroy.restype = C.c_int
    L.wos_tape_destroy.argtypes = [C.c_void_p]
    L.wos_tape_vjp.restype = C.c_int
    L.wos_tape_vjp.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.POINTER(Stats), C.c_void_p, C.c_uint32]
    L.wos_tape_read.restype = C.c_int
    L.wos_tape_read.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_void_p]
    L.wos_tape_index_build.restype = C.c_int
    L.wos_tape_index_build.argtypes = [C.c_void_p, C.c_int64]
    L.wos_tape_index_get_info.restype = C.c_int
    L.wos_tape_index_get_info.argtypes = [C.c_void_p, C.POINTER(TapeIndexInfo)]
    L.wos_tape_index_read.restype = C.c_int
    L.wos_tape_index_read.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_void_p]
    L.wos_tape_vjp_indexed.restype = C.c_int
    L.wos_tape_vjp_indexed.argtypes = L.wos_tape_vjp.argtypes
    L.wos_selftest_tape_rowsum.restype = C.c_int
    L.wos_selftest_tape_rowsum.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_int64, C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.c_int32]
    L.wos_siren_eval.restype = C.c_int
    L.wos_siren_eval.argtypes = [C.POINTER(SirenNet), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_uint32, C.c_int32, C.c_void_p]
    L.wos_selftest_siren_layer.restype = C.c_int
    L.wos_selftest_siren_layer.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_int32]
    L.wos_siren_vjp.restype = C.c_int
    L.wos_siren_vjp.argtypes = [C.POINTER(SirenNet), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_size_t, C.c_uint32, C.c_int32,
                                C.c_void_p]
    L.wos_siren_fit.restype = C.c_int
    L.wos_siren_fit.argtypes = [C.POINTER(SirenNet), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_size_t, C.c_uint32, C.c_int32,
                                C.c_void_p]
    L.wos_adam_step.restype = C.c_int
    L.wos_adam_step.argtypes = [C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(AdamParams), C.c_void_p, C.c_uint32,
                                C.c_int32, C.c_void_p]
    L.wos_siren_fit_run.restype = C.c_int
    L.wos_siren_fit_run.argtypes = [C.POINTER(SirenNet), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                    C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(AdamParams),
                                    C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_int32,
                                    C.c_void_p]
    if hasattr(L, "wos_siren_fit_run_batches"):  # additive within ABI 10, as the length hints above
        L.wos_siren_fit_run_batches.restype = C.c_int
        L.wos_siren_fit_run_batches.argtypes = [C.POINTER(SirenNet), C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(C.c_int64), C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                                C.POINTER(AdamParams), C.c_float, C.c_int32, C.c_void_p, C.c_void_p,
                                                C.c_size_t, C.c_uint32, C.c_int32, C.c_void_p]
    if hasattr(L, "wos_siren_fit_run_ensemble"):  # additive within ABI 10 as well
        ptrs = C.POINTER(C.c_void_p)  # a host array of device pointers, one per member
        L.wos_siren_fit_run_ensemble.restype = C.c_int
        L.wos_siren_fit_run_ensemble.argtypes = [C.c_int32, C.POINTER(SirenNet), C.c_void_p, ptrs, ptrs, C.c_int64,
                                                 C.c_void_p, C.c_int64, C.c_int64, ptrs, ptrs, C.c_int64,
                                                 C.POINTER(AdamParams), C.c_float, C.c_int32, C.c_void_p, C.c_void_p,
                                                 C.c_size_t, C.c_uint32, C.c_int32, C.c_void_p]
        L.wos_siren_fit_run_batches_ensemble.restype = C.c_int
        L.wos_siren_fit_run_batches_ensemble.argtypes = [C.c_int32, C.POINTER(SirenNet), C.c_void_p, ptrs, ptrs,
                                                         C.POINTER(C.c_int64), C.c_int64, ptrs, ptrs, C.c_int64,
                                                         C.POINTER(AdamParams), C.c_float, C.c_int32, C.c_void_p,
                                                         C.c_void_p, C.c_size_t, C.c_uint32, C.c_int32, C.c_void_p]
    L.wos_selftest_siren_vjp_layer.restype = C.c_int
    L.wos_selftest_siren_vjp_layer.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_int32]
    L.wos_default_bvc_params.restype = None
    L.wos_default_bvc_params.argtypes = [C.POINTER(BvcParams)]
    L.wos_bvc.restype = C.c_int
    L.wos_bvc.argtypes = [C.c_void_p, C.POINTER(SolverParams), C.POINTER(BvcParams), C.c_void_p, C.c_void_p,
                          C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(Stats)]
    L.wos_selftest_math.restype = C.c_int
    L.wos_selftest_math.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
    L.wos_selftest_lhs.restype = C.c_int
    L.wos_selftest_lhs.argtypes = [C.c_uint64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                   C.c_int32]
    L.wos_selftest_lhs_permute.restype = C.c_int
    L.wos_selftest_lhs_permute.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_void_p, C.c_int32]
    L.wos_selftest_lhs_plan.restype = C.c_int
    L.wos_selftest_lhs_plan.argtypes = [C.c_int32, C.c_int32, C.c_void_p]
    L.wos_selftest_rejection.restype = C.c_int
    L.wos_selftest_rejection.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_int32]
    if hasattr(L, "wos_selftest_geometry"):  # additive within ABI 10 as well
        L.wos_selftest_geometry.restype = C.c_int
        L.wos_selftest_geometry.argtypes = [C.c_void_p, C.c_uint32, C.c_float, C.c_float, C.c_int32, C.c_void_p,
                                            C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]
    L.wos_selftest_sample_volume.restype = C.c_int
    L.wos_selftest_sample_volume.argtypes = [C.c_int32, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                             C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_int32]
    L.wos_last_error.restype = C.c_char_p
    L.wos_last_error.argtypes = []
    L.wos_selftest_gfn.restype = C.c_int
    L.wos_selftest_gfn.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32]
    L.wos_abi_version.restype = C.c_int32
    L.wos_device_count.restype = C.c_int32
    if L.wos_abi_version() != ABI_VERSION:
        raise WosError(f"{LIB_PATH}: ABI {L.wos_abi_version()} != binding ABI {ABI_VERSION}; rebuild the library")
    _lib = L
    return L


def check(rc, what=""):
    if rc != WOS_OK:
        msg = load().wos_last_error().decode(errors="replace")
        raise WosError(f"{what} failed ({rc}): {msg}")
