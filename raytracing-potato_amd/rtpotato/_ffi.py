"""ctypes bindings of include/rp.h (librp.so, the HIP hot path) and include/rp_host.h (librp_host.so).

librp.so must share the HIP runtime with PyTorch when both live in one process: torch's own
libamdhip64.so is loaded under the NEEDED name "libamdhip64.so" and would not be recognised as the
same library if librp.so (NEEDED "libamdhip64.so.7") pulled /opt/rocm's copy in first.  So `import
torch` happens before librp.so is opened (SONAMEs match, the loader then reuses torch's runtime).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import (POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int64, c_uint8, c_uint32,
                    c_uint64, c_void_p)

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(PKG_DIR, "lib")

RP_OK, RP_EINVAL, RP_EHIP, RP_ENOMEM, RP_ENODEV, RP_EINTERNAL, RP_ERCCL = 0, -1, -2, -3, -4, -5, -6
RP_HITTABLE_SPHERE, RP_HITTABLE_TRIANGLE = 0, 1
RP_SCATTER_NONE, RP_SCATTER_LAMBERT, RP_SCATTER_METAL, RP_SCATTER_DIELECTRIC = 0, 1, 2, 3
RP_ABSORB_BLACK_BODY, RP_ABSORB_WHITE_BODY, RP_ABSORB_ALBEDO, RP_ABSORB_ALBEDO_MAP = 0, 1, 2, 3
(RP_EMIT_NONE, RP_EMIT_DEBUG_NORMALS, RP_EMIT_COLOR, RP_EMIT_SKY_GRADIENT, RP_EMIT_SKY_SPHERE) = range(5)
(RP_TEXTURE_MISSING, RP_TEXTURE_DEBUG_UVS, RP_TEXTURE_SOLID, RP_TEXTURE_IMAGE, RP_TEXTURE_CHECKER,
 RP_TEXTURE_NOISE, RP_TEXTURE_PERLIN) = range(7)
RP_ROOT_BVH, RP_ROOT_LIST = 0, 1
RP_COUNTERS_LEN = 4  # device counter block: rays, samples, pixels, status (include/rp.h)
RP_SAMPLES_PER_STREAM = 32
RP_COMM_ID_BYTES = 128
RP_BUILDER_AUTO, RP_BUILDER_HOST, RP_BUILDER_DEVICE, RP_BUILDER_PLOC = 0, 1, 2, 3
RP_NODES_AUTO, RP_NODES_F32, RP_NODES_Q8, RP_NODES_W8 = 0, 1, 2, 3
RP_TILES_AUTO, RP_TILES_PLAIN, RP_TILES_COST, RP_TILES_MORTON, RP_TILES_PROBE = 0, 1, 2, 3, 4
RP_QUEUES_AUTO, RP_QUEUES_SINGLE, RP_QUEUES_XCD_TILES, RP_QUEUES_XCD_REGIONS = 0, 1, 2, 3
RP_COLLAPSE_AUTO, RP_COLLAPSE_GREEDY, RP_COLLAPSE_SAH = 0, 1, 2
RP_LAYOUT_AUTO, RP_LAYOUT_DFS, RP_LAYOUT_DFS_LINE = 0, 1, 2
RP_UNITS_AUTO, RP_UNITS_TILES, RP_UNITS_LEARNED = 0, 1, 2
RP_FRAME_LEARNED_ORDER, RP_FRAME_PROBED, RP_FRAME_UNIT_ORDER = 2, 4, 8
RP_SHARD_INTERLEAVE, RP_SHARD_BALANCED = 0, 1
RP_STATUS_STACK_OVERFLOW, RP_STATUS_PLAN_MISMATCH = 1, 2
RP_ABI_VERSION = 9
RP_MAX_FRAMES = 64
RP_ERROR_STATS_LEN = 4  # rp_accum_error_device_ws: pixels counted, pixels over, bits of the largest finite e2, non-finite
RP_REPROJECT_STATS_LEN = 4  # rp_reproject_device: pixels, pixels with count >= 1, the sum of the counts, off pixels
RP_FRAME_ORDER_AUTO, RP_FRAME_ORDER_SEQUENTIAL, RP_FRAME_ORDER_INTERLEAVED, RP_FRAME_ORDER_PIXEL = 0, 1, 2, 3
RP_REFIT_OUT_OF_BOUND = 1  # rp_scene_refit_device's status word: a primitive's box beyond the coordinate bound


class rp_hittable(Structure):
    _fields_ = [("kind", c_uint32), ("material", c_uint32), ("mesh", c_uint32), ("triangle", c_uint32),
                ("center", c_double * 3), ("radius", c_double)]


class rp_mesh(Structure):
    _fields_ = [("n_vertices", c_uint32), ("n_indices", c_uint32), ("positions", c_void_p),
                ("normals", c_void_p), ("uvs", c_void_p), ("indices", c_void_p), ("material", c_uint32),
                ("reserved", c_uint32)]


class rp_scatter(Structure):
    _fields_ = [("kind", c_uint32), ("reserved", c_uint32), ("param", c_double)]


class rp_absorb(Structure):
    _fields_ = [("kind", c_uint32), ("texture", c_uint32), ("color", c_double * 3)]


class rp_emit(Structure):
    _fields_ = [("kind", c_uint32), ("texture", c_uint32), ("color", c_double * 3)]


class rp_material(Structure):
    _fields_ = [("scatter", rp_scatter), ("absorb", rp_absorb), ("emit", rp_emit)]


class rp_texture(Structure):
    _fields_ = [("kind", c_uint32), ("odd", c_uint32), ("even", c_uint32), ("width", c_uint32),
                ("height", c_uint32), ("reserved", c_uint32), ("seed", c_int64), ("color", c_double * 3),
                ("rgba", c_void_p)]


class rp_scene_desc(Structure):
    _fields_ = [("root_kind", c_uint32), ("n_hittables", c_uint32), ("hittables", c_void_p),
                ("n_meshes", c_uint32), ("meshes", POINTER(rp_mesh)), ("n_materials", c_uint32),
                ("materials", POINTER(rp_material)), ("n_textures", c_uint32),
                ("textures", POINTER(rp_texture)), ("background", rp_emit)]


class rp_camera(Structure):
    _fields_ = [("aspect_ratio", c_double), ("fov", c_double), ("focal_dist", c_double),
                ("lens_radius", c_double), ("orientation", c_double * 9), ("position", c_double * 3)]


class rp_render_params(Structure):
    _fields_ = [("width", c_uint32), ("height", c_uint32), ("spp", c_uint32), ("max_bounce", c_uint32),
                ("seed", c_uint64), ("tile_w", c_uint32), ("tile_h", c_uint32), ("shard", c_uint32),
                ("num_shards", c_uint32), ("samples_per_stream", c_uint32), ("shard_map", c_uint32)]


class rp_scene_options(Structure):
    _fields_ = [("builder", c_uint32), ("max_leaf", c_uint32), ("cost_traverse", c_double),
                ("always_max", ctypes.c_int32), ("lds_depth", c_uint32), ("self_check", c_uint32),
                ("trav_threshold", c_uint32), ("tile_order", c_uint32), ("probe_n", c_uint32),
                ("node_format", c_uint32), ("leaf_break", c_uint32),
                ("unit_queues", c_uint32), ("queue_chunk", c_uint32), ("debug_stack_depth", c_uint32),
                ("collapse", c_uint32), ("node_layout", c_uint32), ("unit_order", c_uint32)]


class rp_stats(Structure):
    _fields_ = [("rays", c_uint64), ("samples", c_uint64), ("pixels", c_uint64), ("seconds", c_double)]


class rp_denoise_params(Structure):  # include/rp.h: a zero field takes its default (rp_denoise_params_init)
    _fields_ = [("iterations", c_uint32), ("normal_power", c_uint32), ("sigma_depth", c_double),
                ("sigma_albedo", c_double), ("sigma_color", c_double), ("albedo_eps", c_double)]


class rp_denoise_var_params(Structure):  # include/rp.h: base.sigma_color is ignored; a zero field takes its default
    _fields_ = [("base", rp_denoise_params), ("sigma_var", c_double), ("var_eps", c_double)]


class rp_error_params(Structure):  # include/rp.h: a zero field takes its default (tol 0.05, eps 1e-4)
    _fields_ = [("tol", c_double), ("eps", c_double)]


class rp_reproject_params(Structure):  # include/rp.h: a zero field takes its default (0.05, 0.9, 32)
    _fields_ = [("sigma_depth", c_double), ("normal_cos", c_double), ("max_history", c_uint32), ("reserved", c_uint32)]


class rph_mesh(Structure):
    _fields_ = [("n_vertices", c_uint32), ("n_indices", c_uint32), ("positions", POINTER(c_double)),
                ("normals", POINTER(c_double)), ("uvs", POINTER(c_double)), ("indices", POINTER(c_uint32))]


# numpy dtype with exactly rp_hittable's layout (48 B), so large meshes never become Python objects
def hittable_dtype():
    import numpy as np
    return np.dtype({"names": ["kind", "material", "mesh", "triangle", "center", "radius"],
                     "formats": ["<u4", "<u4", "<u4", "<u4", ("<f8", (3,)), "<f8"],
                     "offsets": [0, 4, 8, 12, 16, 40], "itemsize": 48})


# numpy dtypes with exactly the layouts of csrc/rp_layout.h's records (rp_scene_tree; DeviceScene.tree())
def node4_dtype():
    import numpy as np
    names = ["lo_x", "hi_x", "lo_y", "hi_y", "lo_z", "hi_z"]
    return np.dtype({"names": names + ["child", "pad"], "formats": [("<f4", (4,))] * 6 + [("<u4", (4,))] * 2,
                     "offsets": [16 * k for k in range(8)], "itemsize": 128})


def node4q_dtype():
    import numpy as np
    names = ["lo_x", "hi_x", "lo_y", "hi_y", "lo_z", "hi_z"]
    return np.dtype({"names": ["o", "s"] + names + ["child"],
                     "formats": [("<f4", (3,))] * 2 + [("u1", (4,))] * 6 + [("<u4", (4,))],
                     "offsets": [0, 12] + [24 + 4 * k for k in range(6)] + [48], "itemsize": 64})


def node8q_dtype():
    import numpy as np
    names = ["lo_x", "hi_x", "lo_y", "hi_y", "lo_z", "hi_z"]
    return np.dtype({"names": ["o", "s", "inner", "prim"] + names + ["pmask", "pad"],
                     "formats": [("<f4", (3,))] * 2 + ["<u4", "<u4"] + [("u1", (8,))] * 6 + [("<u4", (8,)), ("<u4", (4,))],
                     "offsets": [0, 12, 24, 28] + [32 + 8 * k for k in range(6)] + [80, 112], "itemsize": 128})


def prim_dtype():
    import numpy as np
    return np.dtype({"names": ["g", "kind", "material"], "formats": [("<f8", (9,)), "<u4", "<u4"],
                     "offsets": [0, 72, 76], "itemsize": 80})


def tri_normals_dtype():
    import numpy as np
    return np.dtype({"names": ["n"], "formats": [("<f8", (3, 3))], "offsets": [0], "itemsize": 72})


def prim_ref_dtype():
    import numpy as np
    return np.dtype({"names": ["v", "src"], "formats": [("<u4", (3,)), "<u4"], "offsets": [0, 12], "itemsize": 16})


def node_dtype(node_format: int):
    return {RP_NODES_F32: node4_dtype, RP_NODES_Q8: node4q_dtype, RP_NODES_W8: node8q_dtype}[node_format]()


class RPError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"rp error {code}: {message}")
        self.code = code


_rp = None
_host = None

RP_SYMBOLS = ["rp_abi_version", "rp_last_error", "rp_device_count", "rp_scene_create", "rp_scene_destroy",
              "rp_scene_info", "rp_shard_pixel_count", "rp_shard_unpack", "rp_render", "rp_render_device",
              "rp_intersect", "rp_diagnostics", "rp_workspace_create", "rp_workspace_destroy",
              "rp_render_device_ws", "rp_shard_to_bgra8", "rp_srgb_thresholds", "rp_scene_options_init",
              "rp_scene_create_ex", "rp_workspace_reserve", "rp_comm_unique_id", "rp_comm_create", "rp_comm_destroy",
              "rp_comm_info", "rp_frame_gather", "rp_gather_stride", "rp_frame_assemble", "rp_render_gather", "rp_multi_create", "rp_multi_destroy",
              "rp_render_multi", "rp_shard_unpack_map", "rp_workspace_tile_map", "rp_frame_assemble_ws", "rp_build_id",
              "rp_workspace_tile_costs", "rp_workspace_set_tile_costs", "rp_scene_build_times",
              "rp_workspace_frame_info", "rp_workspace_reserve_frames", "rp_render_frames_device_ws", "rp_frames_gather",
              "rp_workspace_unit_order", "rp_frames_block_words", "rp_frames_pack", "rp_frames_unpack",
              "rp_render_aov_device_ws", "rp_render_aov", "rp_denoise_params_init", "rp_denoise_scratch_bytes",
              "rp_denoise_device", "rp_denoise", "rp_render_variance_device_ws", "rp_denoise_var_params_init",
              "rp_denoise_var_scratch_bytes", "rp_denoise_var_device", "rp_denoise_var", "rp_accum_frames_device",
              "rp_accum_error_device_ws", "rp_render_tiles_device_ws", "rp_accum_tiles_select_device",
              "rp_accum_frames_tiles_device", "rp_scene_tree", "rp_reproject_params_init", "rp_reproject_device",
              "rp_reproject", "rp_accum_frames_counts_device", "rp_refit_create", "rp_refit_destroy", "rp_refit_info",
              "rp_scene_refit_device", "rp_scene_refit"]
class rph_launch_plan(Structure):  # include/rp_host.h (test hook rph_plan_launch)
    _fields_ = [("n_shard_tiles", c_uint32), ("nbatch", c_uint32), ("plan_block", c_uint32), ("n_slots", c_uint64),
                ("gather_stride", c_uint64), ("block_words", c_uint64), ("queue_groups", c_uint32),
                ("queue_chunk", c_uint32), ("frames_inter", c_uint32), ("sortable", c_uint32), ("measure", c_uint32),
                ("grid", c_uint32), ("n_queue", c_uint64), ("out_stride", c_uint64), ("dv_units", c_uint32 * 2),
                ("dv_tiles_x", c_uint32 * 2), ("dv_chunk", c_uint32 * 2)]


HOST_SYMBOLS = ["rph_obj_load", "rph_mesh_free", "rph_tga_load", "rph_tga_save", "rph_free", "rph_to_srgb_u8",
                "rph_lookat", "rph_sky_panorama", "rph_bvh_selfcheck", "rph_bvh_traversal_stats", "rph_bvh_selfcheck_ex", "rph_bvh_traversal_stats_ex", "rph_bvh_tree_hash", "rph_last_error",
                "rph_bvh_selfcheck_opt", "rph_bvh_traversal_stats_opt", "rph_bvh_tree_hash_opt",
                "rph_stdrng_u64", "rph_make_div32", "rph_plan_launch", "rph_draw_round", "rph_ray_setup", "rph_prim_test",
                "rph_unit_walk", "rph_denoise", "rph_denoise_var", "rph_batch_variance", "rph_accum_frames",
                "rph_accum_error", "rph_accum_frames_tiles", "rph_accum_tiles_select", "rph_plan_tiles_launch",
                "rph_tiles_unit_walk", "rph_material_head", "rph_scene_materials", "rph_reproject",
                "rph_accum_frames_counts", "rph_draw_values", "rph_tri_normals", "rph_refit_records", "rph_refit_plan",
                "rph_bvh_refit_check"]


def rp_lib_path() -> str:
    return os.path.join(LIB_DIR, "librp.so")


def host_lib_path() -> str:
    return os.path.join(LIB_DIR, "librp_host.so")


def rp() -> ctypes.CDLL:
    """librp.so (the HIP hot path).  Raises if it is missing: there is no CPU fallback."""
    global _rp
    if _rp is not None:
        return _rp
    path = os.environ.get("RP_LIB") or rp_lib_path()  # RP_LIB: lib/librp_diag.so (diagnostic counters)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `make -C raytracing-potato_amd` "
                           "(or __graft_entry__.build()); there is no CPU fallback for the render path")
    try:
        import torch  # noqa: F401  (share torch's HIP runtime, see module docstring)
    except Exception:
        pass
    lib = ctypes.CDLL(path)
    lib.rp_abi_version.restype = c_int
    lib.rp_last_error.restype = c_char_p
    lib.rp_build_id.restype = c_char_p
    lib.rp_device_count.argtypes = [POINTER(c_int)]
    lib.rp_scene_create.argtypes = [POINTER(rp_scene_desc), c_int, POINTER(c_void_p)]
    lib.rp_scene_destroy.argtypes = [c_void_p]
    lib.rp_scene_destroy.restype = None
    lib.rp_scene_info.argtypes = [c_void_p, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint32),
                                  POINTER(c_uint64), POINTER(c_uint64)]
    lib.rp_shard_pixel_count.argtypes = [POINTER(rp_render_params), POINTER(c_uint64)]
    lib.rp_shard_unpack.argtypes = [POINTER(rp_render_params), c_void_p, c_uint32, c_void_p]
    lib.rp_render.argtypes = [c_void_p, POINTER(rp_camera), POINTER(rp_render_params), c_void_p, c_void_p,
                              POINTER(rp_stats)]
    lib.rp_render_device.argtypes = [c_void_p, POINTER(rp_camera), POINTER(rp_render_params), c_void_p, c_void_p,
                                     c_void_p, c_void_p]
    lib.rp_workspace_create.argtypes = [c_void_p, POINTER(c_void_p)]
    lib.rp_workspace_destroy.argtypes = [c_void_p]
    lib.rp_workspace_destroy.restype = None
    lib.rp_render_device_ws.argtypes = [c_void_p, c_void_p, POINTER(rp_camera), POINTER(rp_render_params), c_void_p,
                                        c_void_p, c_void_p, c_void_p]
    lib.rp_shard_to_bgra8.argtypes = [c_void_p, POINTER(rp_render_params), c_void_p, c_void_p, c_void_p]
    lib.rp_srgb_thresholds.argtypes = [c_void_p]
    lib.rp_intersect.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_void_p]
    lib.rp_diagnostics.argtypes = [c_void_p, c_void_p, c_uint32, c_int]
    lib.rp_scene_options_init.argtypes = [POINTER(rp_scene_options)]
    lib.rp_scene_create_ex.argtypes = [POINTER(rp_scene_desc), c_int, POINTER(rp_scene_options), POINTER(c_void_p)]
    lib.rp_workspace_reserve.argtypes = [c_void_p, c_void_p, POINTER(rp_render_params)]
    lib.rp_comm_unique_id.argtypes = [c_void_p]
    lib.rp_comm_create.argtypes = [c_void_p, c_int, c_int, c_int, POINTER(c_void_p)]
    lib.rp_comm_destroy.argtypes = [c_void_p]
    lib.rp_comm_destroy.restype = None
    lib.rp_comm_info.argtypes = [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int)]
    lib.rp_frame_gather.argtypes = [c_void_p, c_void_p, c_void_p, POINTER(rp_render_params), c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p]
    lib.rp_gather_stride.argtypes = [POINTER(rp_render_params), POINTER(c_uint64)]
    lib.rp_frame_assemble.argtypes = [POINTER(rp_render_params), c_void_p, c_uint32, c_void_p, c_void_p]
    lib.rp_render_gather.argtypes = [c_void_p, c_void_p, c_void_p, POINTER(rp_camera), POINTER(rp_render_params),
                                     c_void_p, c_void_p, c_void_p, c_void_p]
    lib.rp_multi_create.argtypes = [POINTER(rp_scene_desc), c_void_p, c_int, POINTER(rp_scene_options),
                                    POINTER(c_void_p)]
    lib.rp_multi_destroy.argtypes = [c_void_p]
    lib.rp_multi_destroy.restype = None
    lib.rp_render_multi.argtypes = [c_void_p, POINTER(rp_camera), POINTER(rp_render_params), c_void_p, c_void_p,
                                    POINTER(rp_stats)]
    lib.rp_shard_unpack_map.argtypes = [POINTER(rp_render_params), c_void_p, c_void_p, c_uint32, c_void_p]
    lib.rp_workspace_tile_map.argtypes = [c_void_p, c_void_p, POINTER(rp_render_params), c_void_p, c_uint32]
    lib.rp_scene_build_times.argtypes = [c_void_p, c_void_p, c_uint32]
    lib.rp_workspace_tile_costs.argtypes = [c_void_p, c_void_p, POINTER(rp_render_params), c_void_p, c_uint32]
    lib.rp_workspace_frame_info.argtypes = [c_void_p, c_void_p, POINTER(c_uint32)]
    lib.rp_workspace_unit_order.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_uint64]
    lib.rp_frames_block_words.argtypes = [POINTER(rp_render_params), c_uint32, POINTER(c_uint64)]
    lib.rp_frames_pack.argtypes = [c_void_p, c_void_p, POINTER(rp_render_params), c_uint32, c_void_p, c_void_p, c_void_p,
                                   c_void_p]
    lib.rp_frames_unpack.argtypes = [c_void_p, c_void_p, POINTER(rp_render_params), c_uint32, c_void_p, c_void_p, c_void_p,
                                     c_void_p]
    lib.rp_workspace_reserve_frames.argtypes = [c_void_p, c_void_p, POINTER(rp_render_params), c_uint32]
    lib.rp_frames_gather.argtypes = [c_void_p, c_void_p, c_void_p, POINTER(rp_render_params), c_uint32, c_void_p, c_void_p,
                                     c_void_p, c_void_p]
    lib.rp_render_frames_device_ws.argtypes = [c_void_p, c_void_p, POINTER(rp_camera), POINTER(rp_render_params),
                                               c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.rp_workspace_set_tile_costs.argtypes = [c_void_p, c_void_p, POINTER(rp_render_params), c_void_p, c_uint32]
    lib.rp_frame_assemble_ws.argtypes = [c_void_p, c_void_p, POINTER(rp_render_params), c_void_p, c_uint32, c_void_p,
                                         c_void_p]
    lib.rp_render_aov_device_ws.argtypes = [c_void_p, c_void_p, POINTER(rp_camera), POINTER(rp_render_params), c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.rp_render_aov.argtypes = [c_void_p, POINTER(rp_camera), POINTER(rp_render_params), c_void_p, c_void_p, c_void_p,
                                  c_void_p, POINTER(rp_stats)]
    lib.rp_denoise_params_init.argtypes = [POINTER(rp_denoise_params)]
    lib.rp_denoise_scratch_bytes.argtypes = [c_uint32, c_uint32, POINTER(c_uint64)]
    lib.rp_denoise_device.argtypes = [POINTER(rp_denoise_params), c_uint32, c_uint32, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p]
    lib.rp_denoise.argtypes = [POINTER(rp_denoise_params), c_int, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, POINTER(c_double)]
    lib.rp_render_variance_device_ws.argtypes = [c_void_p, c_void_p, POINTER(rp_render_params), c_void_p, c_void_p]
    lib.rp_denoise_var_params_init.argtypes = [POINTER(rp_denoise_var_params)]
    lib.rp_denoise_var_scratch_bytes.argtypes = [c_uint32, c_uint32, POINTER(c_uint64)]
    lib.rp_denoise_var_device.argtypes = [POINTER(rp_denoise_var_params), c_uint32, c_uint32, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.rp_denoise_var.argtypes = [POINTER(rp_denoise_var_params), c_int, c_uint32, c_uint32, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_double)]
    lib.rp_accum_frames_device.argtypes = [c_uint64, c_uint32, c_uint32, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p,
                                           c_void_p]
    lib.rp_accum_error_device_ws.argtypes = [c_void_p, c_void_p, POINTER(rp_render_params), POINTER(rp_error_params),
                                             c_void_p, c_void_p, c_void_p, c_void_p]
    lib.rp_render_tiles_device_ws.argtypes = [c_void_p, c_void_p, POINTER(rp_camera), POINTER(rp_render_params), c_void_p,
                                              c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.rp_accum_tiles_select_device.argtypes = [POINTER(rp_render_params), POINTER(rp_error_params), c_double, c_void_p,
                                                 c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.rp_accum_frames_tiles_device.argtypes = [c_uint64, c_uint32, c_void_p, c_uint32, c_uint32, c_uint32, c_void_p,
                                                 c_uint64, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.rp_scene_tree.argtypes = [c_void_p, c_void_p, c_uint64, c_void_p, c_uint64, c_void_p, c_uint64, POINTER(c_uint32),
                                  POINTER(c_uint32)]
    lib.rp_reproject_params_init.argtypes = [POINTER(rp_reproject_params)]
    lib.rp_reproject_device.argtypes = [POINTER(rp_reproject_params), c_uint32, c_uint32, POINTER(rp_camera),
                                        POINTER(rp_camera)] + [c_void_p] * 12
    lib.rp_reproject.argtypes = [POINTER(rp_reproject_params), c_int, c_uint32, c_uint32, POINTER(rp_camera),
                                 POINTER(rp_camera)] + [c_void_p] * 11 + [POINTER(c_double)]
    lib.rp_accum_frames_counts_device.argtypes = [c_uint64, c_uint32, c_uint32, c_void_p, c_uint64, c_void_p, c_void_p,
                                                  c_void_p, c_void_p, c_double, c_void_p]
    if hasattr(lib, "rp_refit_create"):  # added without an ABI bump: an older library serves every other call
        lib.rp_refit_create.argtypes = [c_void_p, c_double, POINTER(c_void_p)]
        lib.rp_refit_destroy.argtypes = [c_void_p]
        lib.rp_refit_destroy.restype = None
        lib.rp_refit_info.argtypes = [c_void_p, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint32), POINTER(c_double)]
        lib.rp_scene_refit_device.argtypes = [c_void_p] * 6
        lib.rp_scene_refit.argtypes = [c_void_p] * 5 + [POINTER(c_double)]
    if lib.rp_abi_version() != RP_ABI_VERSION:
        raise RuntimeError(f"{path}: ABI version {lib.rp_abi_version()}, bindings expect {RP_ABI_VERSION} (rebuild)")
    _rp = lib
    return lib


def host() -> ctypes.CDLL:
    global _host
    if _host is not None:
        return _host
    path = os.environ.get("RP_HOST_LIB") or host_lib_path()  # RP_HOST_LIB: the sanitizer build (tools/sanitize.sh)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `make -C raytracing-potato_amd`")
    lib = ctypes.CDLL(path)
    lib.rph_obj_load.argtypes = [c_char_p, POINTER(rph_mesh)]
    lib.rph_mesh_free.argtypes = [POINTER(rph_mesh)]
    lib.rph_mesh_free.restype = None
    lib.rph_tga_load.argtypes = [c_char_p, POINTER(c_uint32), POINTER(c_uint32), POINTER(POINTER(c_uint8))]
    lib.rph_tga_save.argtypes = [c_char_p, c_uint32, c_uint32, c_void_p]
    lib.rph_free.argtypes = [c_void_p]
    lib.rph_free.restype = None
    lib.rph_to_srgb_u8.argtypes = [c_void_p, c_uint64, c_void_p]
    lib.rph_to_srgb_u8.restype = None
    lib.rph_lookat.argtypes = [c_double * 3, c_double * 3, c_double * 3, c_double * 9]
    lib.rph_lookat.restype = None
    lib.rph_sky_panorama.argtypes = [c_uint32, c_uint32, c_void_p]
    lib.rph_bvh_selfcheck.argtypes = [POINTER(rp_scene_desc), c_uint32, POINTER(c_uint64)]
    lib.rph_bvh_traversal_stats.argtypes = [POINTER(rp_scene_desc), c_void_p, c_uint64, c_uint32, c_void_p]
    lib.rph_bvh_selfcheck_ex.argtypes = [POINTER(rp_scene_desc), c_uint32, c_uint32, POINTER(c_uint64)]
    lib.rph_bvh_traversal_stats_ex.argtypes = [POINTER(rp_scene_desc), c_void_p, c_uint64, c_uint32, c_uint32, c_void_p]
    lib.rph_bvh_tree_hash.argtypes = [POINTER(rp_scene_desc), c_uint32, c_uint32, POINTER(c_uint64)]
    lib.rph_bvh_selfcheck_opt.argtypes = [POINTER(rp_scene_desc), c_uint32, c_uint32, ctypes.c_int32, c_uint32, POINTER(c_uint64)]
    lib.rph_bvh_traversal_stats_opt.argtypes = [POINTER(rp_scene_desc), c_void_p, c_uint64, c_uint32, c_uint32, ctypes.c_int32,
                                                c_uint32, c_void_p]
    lib.rph_bvh_tree_hash_opt.argtypes = [POINTER(rp_scene_desc), c_uint32, c_uint32, ctypes.c_int32, c_uint32, POINTER(c_uint64)]
    lib.rph_last_error.restype = c_char_p
    lib.rph_stdrng_u64.argtypes = [c_void_p, c_uint64, c_uint64, c_void_p]
    lib.rph_make_div32.argtypes = [c_uint32, POINTER(c_uint32), POINTER(c_uint32)]
    lib.rph_draw_round.argtypes = [c_uint32, c_uint32, c_void_p, c_uint32, c_void_p, POINTER(c_uint32),
                                   POINTER(c_uint32)]
    lib.rph_draw_values.argtypes = [c_void_p, c_uint64, c_void_p, c_void_p]
    lib.rph_ray_setup.argtypes = [c_uint32, c_double, c_void_p, c_uint64, c_void_p]
    lib.rph_prim_test.argtypes = [c_uint32, c_void_p, c_void_p, c_uint64, c_void_p]
    lib.rph_plan_launch.argtypes = [c_uint32] * 14 + [c_uint64, POINTER(rph_launch_plan)]
    lib.rph_unit_walk.argtypes = [c_uint32] * 14 + [c_void_p] * 3 + [c_uint32] * 4 + [c_void_p, c_uint64,
                                  POINTER(c_uint64), c_void_p, c_void_p, POINTER(c_uint64)]
    lib.rph_denoise.argtypes = [POINTER(rp_denoise_params), c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p]
    lib.rph_denoise_var.argtypes = [POINTER(rp_denoise_var_params), c_uint32, c_uint32, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p]
    lib.rph_batch_variance.argtypes = [c_uint32, c_uint32, c_uint64, c_void_p, c_void_p]
    lib.rph_accum_frames.argtypes = [c_uint64, c_uint32, c_uint32, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p]
    lib.rph_accum_error.argtypes = [POINTER(rp_error_params), c_uint64, c_void_p, c_void_p, c_void_p]
    lib.rph_accum_frames_tiles.argtypes = [c_uint64, c_uint32, c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_uint64,
                                           c_void_p, c_void_p, c_void_p]
    lib.rph_accum_tiles_select.argtypes = [POINTER(rp_render_params), POINTER(rp_error_params), c_double, c_void_p,
                                           c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_void_p]
    lib.rph_plan_tiles_launch.argtypes = [c_uint32] * 12 + [c_uint64, POINTER(rph_launch_plan)]
    lib.rph_tiles_unit_walk.argtypes = [c_uint32] * 11 + [c_void_p, c_uint32, c_uint32, c_void_p, c_uint64,
                                        POINTER(c_uint64), c_void_p, c_void_p]
    lib.rph_material_head.argtypes = [c_void_p, c_void_p, c_void_p]
    lib.rph_scene_materials.argtypes = [POINTER(rp_scene_desc), c_uint64, c_void_p, POINTER(c_uint64)]
    lib.rph_tri_normals.argtypes = [POINTER(rp_scene_desc), c_uint32, ctypes.c_int32, c_uint32, c_uint64, c_void_p, c_void_p,
                                    c_void_p, POINTER(c_uint64)]
    lib.rph_reproject.argtypes = [POINTER(rp_reproject_params), c_uint32, c_uint32, POINTER(rp_camera),
                                  POINTER(rp_camera)] + [c_void_p] * 11
    lib.rph_accum_frames_counts.argtypes = [c_uint64, c_uint32, c_uint32, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_double]
    lib.rph_refit_records.argtypes = [c_uint32, c_void_p, c_uint64, c_uint32, c_void_p, c_void_p, c_void_p, c_uint64,
                                      c_void_p, c_void_p, c_void_p, c_uint64, c_uint64, c_double, POINTER(c_uint32)]
    lib.rph_refit_plan.argtypes = [c_uint32, c_void_p, c_uint64, c_uint32, c_void_p, c_void_p, POINTER(c_uint32)]
    lib.rph_bvh_refit_check.argtypes = [POINTER(rp_scene_desc), POINTER(rp_scene_desc), c_uint32, ctypes.c_int32, c_uint32,
                                        c_void_p, POINTER(c_uint32)]
    _host = lib
    return lib


def check(code: int, lib: ctypes.CDLL | None = None) -> None:
    if code != RP_OK:
        lib = lib or rp()
        fn = lib.rp_last_error if hasattr(lib, "rp_last_error") else lib.rph_last_error
        raise RPError(code, (fn() or b"").decode(errors="replace"))


def check_host(code: int) -> None:
    if code != RP_OK:
        raise RPError(code, (host().rph_last_error() or b"").decode(errors="replace"))


__all__ = [n for n in dir() if not n.startswith("__")]
