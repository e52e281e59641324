"""wos_amd -- MI355X-native walk-on-stars pressure-projection engine (host side).

The compute path is the HIP kernel in ../csrc (built into ../lib/libwos_hip.so);
this package only marshals arguments across the C ABI (include/wos.h).
"""
from ._lib import WosError, load as load_library  # noqa: F401
from . import siren  # noqa: F401
from .engine import WalkTape, WosScene, bvc_params, load_obj, solver_params, selftest_math, selftest_lhs, selftest_lhs_permute, selftest_lhs_permute_slots, selftest_lhs_plan, selftest_tape_rowsum, selftest_rejection, selftest_gfn, selftest_sample_volume, device_count, release_caches, set_max_batch_tasks, set_length_hints, length_hint_stats, selftest_hint_key, set_express_layout, express_layout, express_layout_stats, selftest_express_slot, selftest_simd_ids  # noqa: F401

__all__ = ["WalkTape", "WosScene", "WosError", "bvc_params", "load_obj", "solver_params", "selftest_math", "selftest_lhs", "selftest_lhs_permute",
           "selftest_lhs_permute_slots", "selftest_lhs_plan", "selftest_tape_rowsum", "selftest_rejection", "selftest_gfn", "selftest_sample_volume", "device_count", "set_max_batch_tasks",
           "load_library", "release_caches", "siren", "set_length_hints", "length_hint_stats", "selftest_hint_key",
           "set_express_layout", "express_layout", "express_layout_stats", "selftest_express_slot", "selftest_simd_ids"]
