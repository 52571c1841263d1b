"""render(): the drop-in for the reference's per-pixel worker loop (main.rs:61-92 calling
render.rs:94 trace_path), on MI355X through librp.so.  No CPU fallback: a missing or failing HIP
library raises.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _ffi as F
from .scene import RenderParams, Scene, shard_slot_count


# scene_options' named values, by field
_OPTION_NAMES = {
    "builder": {"auto": F.RP_BUILDER_AUTO, "host": F.RP_BUILDER_HOST, "gpu": F.RP_BUILDER_DEVICE,
                "ploc": F.RP_BUILDER_PLOC},
    "tile_order": {"auto": F.RP_TILES_AUTO, "plain": F.RP_TILES_PLAIN, "cost": F.RP_TILES_COST,
                   "morton": F.RP_TILES_MORTON, "probe": F.RP_TILES_PROBE},
    "node_format": {"auto": F.RP_NODES_AUTO, "f32": F.RP_NODES_F32, "q8": F.RP_NODES_Q8, "w8": F.RP_NODES_W8},
    "unit_queues": {"auto": F.RP_QUEUES_AUTO, "single": F.RP_QUEUES_SINGLE, "xcd_tiles": F.RP_QUEUES_XCD_TILES,
                    "xcd_regions": F.RP_QUEUES_XCD_REGIONS},
    "collapse": {"auto": F.RP_COLLAPSE_AUTO, "greedy": F.RP_COLLAPSE_GREEDY, "sah": F.RP_COLLAPSE_SAH},
    "node_layout": {"auto": F.RP_LAYOUT_AUTO, "dfs": F.RP_LAYOUT_DFS, "dfs_line": F.RP_LAYOUT_DFS_LINE},
    "unit_order": {"auto": F.RP_UNITS_AUTO, "tiles": F.RP_UNITS_TILES, "learned": F.RP_UNITS_LEARNED},
}
# the `order` argument of the multi-frame launches (RP_FRAME_ORDER_*); any other value is passed through
_FRAME_ORDER = {"auto": F.RP_FRAME_ORDER_AUTO, "sequential": F.RP_FRAME_ORDER_SEQUENTIAL,
                "interleaved": F.RP_FRAME_ORDER_INTERLEAVED, "pixel": F.RP_FRAME_ORDER_PIXEL}


def scene_options(**kw) -> F.rp_scene_options:
    """rp_scene_options with the library defaults (rp_scene_options_init), fields overridden by keyword:
    builder ("auto" | "host" | "gpu" (LBVH) | "ploc" or RP_BUILDER_*), max_leaf, cost_traverse, always_max, lds_depth,
    self_check, trav_threshold, probe_n,
    node_format ("auto" | "f32" | "q8" | "w8" or RP_NODES_*), tile_order ("auto" | "plain" | "cost" | "morton" | "probe"), leaf_break,
    unit_queues ("auto" | "single" | "xcd_tiles" | "xcd_regions" or RP_QUEUES_*), collapse ("auto" | "greedy" | "sah" or
    RP_COLLAPSE_*), node_layout ("auto" | "dfs" | "dfs_line" or RP_LAYOUT_*), unit_order ("auto" | "tiles" | "learned" or
    RP_UNITS_*)."""
    o = F.rp_scene_options()
    F.check(F.rp().rp_scene_options_init(ctypes.byref(o)))
    for k, v in kw.items():
        if isinstance(v, str) and k in _OPTION_NAMES:
            v = _OPTION_NAMES[k][v]
        if not hasattr(o, k):
            raise KeyError(f"unknown scene option {k!r}")
        setattr(o, k, v)
    return o


def _stream(stream, device):
    """`stream` (a torch stream), or torch's current one on `device`."""
    import torch
    return stream if stream is not None else torch.cuda.current_stream(device)


def _stream_ptr(stream, device=None):
    """_stream(stream, device) as the library takes it."""
    return ctypes.c_void_p(_stream(stream, device).cuda_stream)


def _ws_handle(workspace, scene=None):
    """The handle of `workspace` (None: the scene's own workspace); with `scene`, a live workspace of that scene."""
    if workspace is None:
        return None
    assert scene is None or (workspace.scene is scene and workspace.handle)
    return workspace.handle


def _stats_dict(st) -> dict:
    return {"rays": st.rays, "samples": st.samples, "pixels": st.pixels, "seconds": st.seconds}


def _check_tensor(t, dtype, numel: int, device=None, contiguous: bool = True) -> None:
    """`t` is a torch tensor on a GPU (on `device`, if given) of `dtype` and at least `numel` elements."""
    assert t.dtype == dtype and t.is_cuda and t.numel() >= numel
    assert not contiguous or t.is_contiguous()
    assert device is None or t.device == device


def _whole_frame(params, who: str) -> None:
    if params.num_shards != 1 or params.shard_map != F.RP_SHARD_INTERLEAVE:
        raise ValueError(f"{who} renders the whole frame on one device (num_shards = 1, interleave)")


def _assemble(params, shard: dict, frame: dict, sp) -> None:
    """rp_frame_assemble at num_shards = 1: every compact shard buffer of `shard` (torch f64) into frame order in the
    tensor of `frame` under the same key, on the stream `sp` (_stream_ptr)."""
    p, n = params.to_c(), shard_slot_count(params)
    for k, t in shard.items():  # 32-bit words per slot: 6 for 3 doubles, 2 for one
        F.check(F.rp().rp_frame_assemble(ctypes.byref(p), t.data_ptr(), 2 * (t.numel() // n), frame[k].data_ptr(), sp))


def _progressive_args(params, who: str, frames_per_launch: int, max_frames: int, tol: float, share: float) -> None:
    """What render_progressive and render_adaptive refuse alike."""
    _whole_frame(params, who)
    if not 1 <= frames_per_launch <= F.RP_MAX_FRAMES:
        raise ValueError(f"frames_per_launch must be 1..{F.RP_MAX_FRAMES}, got {frames_per_launch}")
    if min(frames_per_launch, max_frames) < 2:
        raise ValueError("the variance needs two frames: frames_per_launch and max_frames must be >= 2")
    if not (tol > 0.0 and 0.0 <= share <= 1.0):
        raise ValueError(f"tol must be > 0 and share in [0, 1], got {tol}, {share}")


def _progressive_state(params, frames_per_launch: int, dev) -> tuple:
    """The device state of a progressive loop (allocated on torch's current stream): the launches' frames buffer, the
    running mean, m2 and variance (compact shard buffers), the counters and the error statistics."""
    import torch
    n = shard_slot_count(params)
    frames = torch.empty(frames_per_launch * 3 * n, dtype=torch.float64, device=dev)
    mean, m2, var = (torch.empty(3 * n, dtype=torch.float64, device=dev) for _ in range(3))
    ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device=dev)
    stats = torch.zeros(F.RP_ERROR_STATS_LEN, dtype=torch.int64, device=dev)
    return frames, mean, m2, var, ctr, stats


class DeviceScene:
    """rp_scene: the scene's acceleration structure and tables resident in one GPU's HBM.  `options`: a dict of
    rp_scene_options fields (scene_options())."""

    def __init__(self, scene: Scene, device: int = 0, options: dict | None = None):
        self.scene = scene
        self.device = device
        self._desc = scene.desc()
        h = ctypes.c_void_p()
        opt = scene_options(**(options or {}))
        F.check(F.rp().rp_scene_create_ex(self._desc.ptr(), device, ctypes.byref(opt), ctypes.byref(h)))
        self.handle = h

    def info(self) -> dict:
        nn, nl, np_, nb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        md = ctypes.c_uint32()
        F.check(F.rp().rp_scene_info(self.handle, ctypes.byref(nn), ctypes.byref(nl), ctypes.byref(md),
                                     ctypes.byref(np_), ctypes.byref(nb)))
        return {"nodes": nn.value, "leaves": nl.value, "max_depth": md.value, "prims": np_.value,
                "device_bytes": nb.value}

    def tree(self) -> dict:
        """rp_scene_tree (a test hook): the packed tree as it lies in device memory.  "nodes": a structured array of
        Node4, Node4Q or Node8Q records by "node_format" (RP_NODES_*; _ffi.node_dtype), "prims" and "prim_refs" in leaf
        order (_ffi.prim_dtype, prim_ref_dtype), "root": the root's node index."""
        fmt, root = ctypes.c_uint32(), ctypes.c_uint32()
        F.check(F.rp().rp_scene_tree(self.handle, None, 0, None, 0, None, 0, ctypes.byref(fmt), ctypes.byref(root)))
        info = self.info()
        nodes = np.zeros(info["nodes"], dtype=F.node_dtype(fmt.value))
        prims = np.zeros(info["prims"], dtype=F.prim_dtype())
        refs = np.zeros(info["prims"], dtype=F.prim_ref_dtype())
        F.check(F.rp().rp_scene_tree(self.handle, nodes.ctypes.data, nodes.nbytes, prims.ctypes.data, prims.nbytes,
                                     refs.ctypes.data, refs.nbytes, None, None))
        return {"node_format": fmt.value, "root": root.value, "nodes": nodes, "prims": prims, "prim_refs": refs}

    def geometry(self) -> dict:
        """The geometry a refit moves, in rp_scene_refit_device's numbering, from the host scene (copies): "positions"
        and "normals" (n_vertices, 3) -- the meshes' vertices concatenated in mesh order --, "spheres" (n_spheres, 4)
        {center, radius} -- the sphere hittables in hittable order.  The starting point of a deformation."""
        return scene_geometry(self.scene)

    def refit_handle(self, coord_max: float = 0.0) -> "Refit":
        """rp_refit_create: the plan and scratch that move this scene's geometry without building it again.  coord_max:
        the largest |coordinate| later updates may reach (0 keeps the build's bound).  `self.scene`, the host
        description, is never updated by a refit: it stays what the scene was created from."""
        r = Refit(self, coord_max)
        self.__dict__.setdefault("_refits", []).append(r)
        return r

    def build_times(self) -> dict:
        """rp_scene_build_times: host seconds of the scene_create phases."""
        t = np.zeros(6)
        F.check(F.rp().rp_scene_build_times(self.handle, t.ctypes.data, 6))
        return dict(zip(("validate", "host_tree", "device_input", "device_build_or_upload", "tables_upload",
                         "workspace"), t.round(4).tolist()))

    def close(self) -> None:
        for w in list(getattr(self, "_workspaces", ())) + list(getattr(self, "_refits", ())):
            w.close()
        if getattr(self, "handle", None):
            F.rp().rp_scene_destroy(self.handle)
            self.handle = None

    def workspace(self) -> "Workspace":
        """A second (third, ...) per-frame workspace: frames rendered with different workspaces may run
        concurrently on different streams (rp_workspace_create)."""
        w = Workspace(self)
        self.__dict__.setdefault("_workspaces", []).append(w)
        return w

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def reserve(self, params: RenderParams, workspace: "Workspace | None" = None) -> None:
        """rp_workspace_reserve: device memory the asynchronous renders (and frame gathers) of `params`' shape
        need, in `workspace` (default: the scene's own)."""
        p = params.to_c()
        F.check(F.rp().rp_workspace_reserve(self.handle, _ws_handle(workspace), ctypes.byref(p)))

    def reserve_frames(self, params: RenderParams, n_frames: int, workspace: "Workspace | None" = None) -> None:
        """rp_workspace_reserve_frames: rp_workspace_reserve, plus the batch sums of n_frames frames per launch."""
        p = params.to_c()
        F.check(F.rp().rp_workspace_reserve_frames(self.handle, _ws_handle(workspace),
                                                   ctypes.byref(p), n_frames))

    def tile_map(self, params: RenderParams, workspace: "Workspace | None" = None) -> np.ndarray:
        """rp_workspace_tile_map: the frame's deal order (shard s's k-th tile = map[s + k * num_shards]) -- the
        balanced plan the last render of this frame in `workspace` made, or the interleave's identity."""
        tiles = -(-params.width // params.tile_w) * -(-params.height // params.tile_h)
        out = np.empty(tiles, dtype=np.uint32)
        p = params.to_c()
        F.check(F.rp().rp_workspace_tile_map(self.handle, _ws_handle(workspace), ctypes.byref(p),
                                             out.ctypes.data, tiles))
        return out

    def tile_costs(self, params: RenderParams, workspace: "Workspace | None" = None) -> np.ndarray:
        """rp_workspace_tile_costs: (2, shard tiles) measured costs of the last render in `workspace` -- summed unit
        durations per shard tile, then the longest unit."""
        n = shard_slot_count(params) // (params.tile_w * params.tile_h)
        out = np.zeros(2 * max(n, 1), dtype=np.uint32)
        p = params.to_c()
        F.check(F.rp().rp_workspace_tile_costs(self.handle, _ws_handle(workspace), ctypes.byref(p),
                                               out.ctypes.data, len(out)))
        return out[:2 * n].reshape(2, n)

    def frame_info(self, workspace: "Workspace | None" = None) -> int:
        """rp_workspace_frame_info: RP_FRAME_* bits of the last render enqueued with `workspace` (None = the scene's)."""
        f = ctypes.c_uint32()
        F.check(F.rp().rp_workspace_frame_info(self.handle, _ws_handle(workspace), ctypes.byref(f)))
        return f.value

    def unit_order(self, n: int, workspace: "Workspace | None" = None) -> tuple:
        """rp_workspace_unit_order: (durations, order) of the last render's n units (uint32 arrays; order valid when
        frame_info has RP_FRAME_UNIT_ORDER)."""
        dur = np.zeros(n, dtype=np.uint32)
        order = np.zeros(n, dtype=np.uint32)
        F.check(F.rp().rp_workspace_unit_order(self.handle, _ws_handle(workspace), dur.ctypes.data,
                                               order.ctypes.data, n))
        return dur, order

    def set_tile_costs(self, params: RenderParams, costs: np.ndarray, ranks: int,
                       workspace: "Workspace | None" = None) -> None:
        """rp_workspace_set_tile_costs: install a frame's learned cost table, (2, frame tiles) by frame tile."""
        c = np.ascontiguousarray(costs, dtype=np.uint32).reshape(-1)
        p = params.to_c()
        F.check(F.rp().rp_workspace_set_tile_costs(self.handle, _ws_handle(workspace),
                                                   ctypes.byref(p), c.ctypes.data, ranks))

    # ---- synchronous host-buffer render -----------------------------------------------------------
    def render(self, params: RenderParams, camera=None, foreground: bool = False):
        """Full frame (only the shard's pixels written, others zero): (rgb (h, w, 3) f64,
        foreground (h, w) f32 or None, stats dict)."""
        cam = (camera or self.scene.camera).to_c()
        p = params.to_c()
        rgb = np.zeros((params.height, params.width, 3), dtype=np.float64)
        fg = np.zeros((params.height, params.width), dtype=np.float32) if foreground else None
        st = F.rp_stats()
        F.check(F.rp().rp_render(self.handle, ctypes.byref(cam), ctypes.byref(p), rgb.ctypes.data,
                                 fg.ctypes.data if fg is not None else None, ctypes.byref(st)))
        return rgb, fg, _stats_dict(st)

    # ---- asynchronous device render (torch tensors, torch's current stream) ------------------------
    def render_device(self, params: RenderParams, out, counters, fg=None, camera=None, stream=None,
                      workspace: "Workspace | None" = None) -> None:
        """Render the shard into `out` (torch f64 tensor, >= shard_slot_count*3 elements) on `stream`
        (torch stream; default: current).  counters: torch int64 tensor of RP_COUNTERS_LEN elements.
        workspace: one from self.workspace() (default: the scene's own, rp_render_device); frames of more
        than one sample batch need self.reserve(params, workspace) first."""
        import torch
        cam = (camera or self.scene.camera).to_c()
        p = params.to_c()
        _check_tensor(out, torch.float64, 3 * shard_slot_count(params), contiguous=False)
        assert counters.dtype == torch.int64 and counters.numel() >= F.RP_COUNTERS_LEN
        sp = _stream_ptr(stream, out.device)
        fgp = fg.data_ptr() if fg is not None else None
        if workspace is None:
            F.check(F.rp().rp_render_device(self.handle, ctypes.byref(cam), ctypes.byref(p), out.data_ptr(), fgp,
                                            counters.data_ptr(), sp))
        else:
            F.check(F.rp().rp_render_device_ws(self.handle, _ws_handle(workspace, self), ctypes.byref(cam),
                                               ctypes.byref(p), out.data_ptr(), fgp, counters.data_ptr(), sp))

    def render_frames_device(self, params: RenderParams, n_frames: int, out, counters, fg=None, camera=None,
                             stream=None, workspace: "Workspace | None" = None, order="auto") -> None:
        """rp_render_frames_device_ws: n_frames frames in one launch -- frame f is render_device's frame of `params` with
        seed + f * ceil(spp / samples_per_stream) * width * height.  out: torch f64, >= n_frames * 3 * shard_slot_count
        elements (frame f at f * 3 * slots); fg: n_frames * slots floats or None; counters: the frames' sums.  The
        workspace needs reserve_frames(params, n_frames) when the frame has more than one sample batch.  order: "auto" |
        "sequential" | "interleaved" (RP_FRAME_ORDER_*)."""
        import torch
        cam = (camera or self.scene.camera).to_c()
        p = params.to_c()
        n = shard_slot_count(params)
        _check_tensor(out, torch.float64, 3 * n * n_frames, contiguous=False)
        assert fg is None or fg.numel() >= n * n_frames
        assert counters.dtype == torch.int64 and counters.numel() >= F.RP_COUNTERS_LEN
        F.check(F.rp().rp_render_frames_device_ws(self.handle, _ws_handle(workspace), ctypes.byref(cam), ctypes.byref(p),
                                                  n_frames, _FRAME_ORDER.get(order, order), out.data_ptr(),
                                                  fg.data_ptr() if fg is not None else None, counters.data_ptr(),
                                                  _stream_ptr(stream, out.device)))

    # ---- first-hit feature pass (rp_render_aov*): normal, albedo, depth, foreground ------------------
    def render_aov(self, params: RenderParams, camera=None, normal: bool = True, albedo: bool = True,
                   depth: bool = True, foreground: bool = True) -> dict:
        """rp_render_aov: the guide buffers of the camera rays' first hits, full frames (only the shard's pixels
        written, others zero): {"normal": (h, w, 3) f64, "albedo": (h, w, 3) f64, "depth": (h, w) f64,
        "fg": (h, w) f32, "stats": dict}; a buffer that is not asked for is None."""
        cam = (camera or self.scene.camera).to_c()
        p = params.to_c()
        h, w = params.height, params.width
        out = {"normal": np.zeros((h, w, 3), dtype=np.float64) if normal else None,
               "albedo": np.zeros((h, w, 3), dtype=np.float64) if albedo else None,
               "depth": np.zeros((h, w), dtype=np.float64) if depth else None,
               "fg": np.zeros((h, w), dtype=np.float32) if foreground else None}
        ptr = {k: (v.ctypes.data if v is not None else None) for k, v in out.items()}
        st = F.rp_stats()
        F.check(F.rp().rp_render_aov(self.handle, ctypes.byref(cam), ctypes.byref(p), ptr["normal"], ptr["albedo"],
                                     ptr["depth"], ptr["fg"], ctypes.byref(st)))
        out["stats"] = _stats_dict(st)
        return out

    def render_aov_device(self, params: RenderParams, normal=None, albedo=None, depth=None, fg=None, counters=None,
                          camera=None, stream=None, workspace: "Workspace | None" = None) -> None:
        """rp_render_aov_device_ws: the shard's guide buffers into torch tensors on `stream` (torch stream; default:
        current), compact shard order -- normal, albedo: f64, >= 3 * shard_slot_count elements; depth: f64, fg: f32,
        >= shard_slot_count; counters: int64, RP_COUNTERS_LEN.  Each is optional, at least one output is needed.  A
        balanced shard (params.shard_map) takes the plan of the beauty render done before on `workspace`."""
        import torch
        cam = (camera or self.scene.camera).to_c()
        p = params.to_c()
        n = shard_slot_count(params)
        dev = None
        for t, dt, m in ((normal, torch.float64, 3 * n), (albedo, torch.float64, 3 * n), (depth, torch.float64, n),
                         (fg, torch.float32, n), (counters, torch.int64, F.RP_COUNTERS_LEN)):
            if t is not None:
                _check_tensor(t, dt, m)
                dev = t.device
        assert dev is not None, "render_aov_device needs at least one output tensor"
        ptr = [t.data_ptr() if t is not None else None for t in (normal, albedo, depth, fg, counters)]
        F.check(F.rp().rp_render_aov_device_ws(self.handle, _ws_handle(workspace, self), ctypes.byref(cam),
                                               ctypes.byref(p), *ptr, _stream_ptr(stream, dev)))

    # ---- per-pixel variance from the batch sums (rp_render_variance_device_ws) -------------------------
    def render_variance_device(self, params: RenderParams, var, workspace: "Workspace | None" = None,
                               stream=None) -> None:
        """rp_render_variance_device_ws: the variance of every pixel's mean, from the batch sums the last render of
        `params` left in `workspace` (None = the scene's), into `var` (torch f64, >= 3 * shard_slot_count elements,
        compact shard order like the render's rgb) on `stream` (torch stream; default: current).  Needs more than one
        sample batch per pixel (spp > samples_per_stream); order it after that render and before the workspace's next."""
        import torch
        _check_tensor(var, torch.float64, 3 * shard_slot_count(params))
        p = params.to_c()
        F.check(F.rp().rp_render_variance_device_ws(self.handle, _ws_handle(workspace, self), ctypes.byref(p),
                                                    var.data_ptr(), _stream_ptr(stream, var.device)))

    # ---- beauty + guides + denoiser, device-resident ---------------------------------------------------
    def render_denoised(self, params: RenderParams, denoise=None, bgra: bool = False, camera=None, stream=None,
                        variance: bool = False):
        """A denoised frame without a host round trip: the beauty render and the feature pass into shard buffers,
        rp_frame_assemble at num_shards = 1 into frame order, then rp_denoise_device (`denoise`: rp_denoise_params, a
        dict of its fields or None = the defaults), all on `stream` (torch stream; default: current).  Returns the frame
        as a torch f64 tensor (h, w, 3) on the scene's device and, with bgra=True, also its to_srgb_u8 bytes (h, w, 4)
        uint8 in TGA order B, G, R, A (rp_shard_to_bgra8: a frame-order buffer is the shard buffer of the frame tiled
        tile_w = width, tile_h = height).  One device holds the whole frame (multi-GPU frames assemble with
        rp_frame_assemble_ws and denoise_device).  variance=True: the variance pass (render_variance_device) follows the
        beauty render and the filter is the variance-guided one (rp_denoise_var_device; `denoise`: as
        denoise_var_params takes it); `params` must give more than one sample batch per pixel."""
        import torch
        from dataclasses import replace
        _whole_frame(params, "render_denoised")
        if variance and params.spp <= (params.samples_per_stream or F.RP_SAMPLES_PER_STREAM):
            raise ValueError("render_denoised(variance=True) needs at least two sample batches per pixel "
                             f"(spp > samples_per_stream): spp = {params.spp}, samples_per_stream = "
                             f"{params.samples_per_stream or F.RP_SAMPLES_PER_STREAM}")
        dev = torch.device("cuda", self.device)
        s = _stream(stream, dev)
        w, h, n = params.width, params.height, shard_slot_count(params)
        self.reserve(params)
        with torch.cuda.stream(s):
            bufs = (("rgb", 3), ("normal", 3), ("albedo", 3), ("depth", 1)) + ((("var", 3),) if variance else ())
            shard = {k: torch.empty(c * n, dtype=torch.float64, device=dev) for k, c in bufs}
            frame = {k: torch.empty(c * w * h, dtype=torch.float64, device=dev) for k, c in bufs}
            ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device=dev)
            out = torch.empty((h, w, 3), dtype=torch.float64, device=dev)
            self.render_device(params, shard["rgb"], ctr, camera=camera, stream=s)
            if variance:
                self.render_variance_device(params, shard["var"], stream=s)
            self.render_aov_device(params, normal=shard["normal"], albedo=shard["albedo"], depth=shard["depth"],
                                   camera=camera, stream=s)
            _assemble(params, shard, frame, _stream_ptr(s))
            denoise_device(frame["rgb"], frame["normal"], frame["albedo"], frame["depth"], out, params=denoise,
                           stream=s, variance=frame.get("var"))
            if not bgra:
                return out
            bytes_ = torch.empty((h, w, 4), dtype=torch.uint8, device=dev)
            self.to_bgra8(replace(params, tile_w=w, tile_h=h), out, bytes_, stream=s)
            return out, bytes_

    # ---- progressive rendering: running mean and variance over frames (rp_accum_*) ------
    def accum_error_device(self, params: RenderParams, mean, var, stats, tol: float = 0.0, eps: float = 0.0,
                           workspace: "Workspace | None" = None, stream=None) -> None:
        """rp_accum_error_device_ws: the error statistics of the shard's pixels from `mean` and `var` (torch f64,
        >= 3 * shard_slot_count elements, compact shard order) into `stats` (torch int64, RP_ERROR_STATS_LEN: pixels
        counted, pixels with e2 > tol^2, the bits of the largest finite e2 -- error_stats() decodes them --, pixels whose
        e2 is not finite) on `stream` (torch stream; default: current).  tol, eps: 0 takes the default (0.05, 1e-4).  A
        balanced shard takes the plan of the beauty render done before on `workspace`."""
        import torch
        n = shard_slot_count(params)
        for t in (mean, var):
            _check_tensor(t, torch.float64, 3 * n)
        _check_tensor(stats, torch.int64, F.RP_ERROR_STATS_LEN)
        p = params.to_c()
        e = F.rp_error_params(tol, eps)
        F.check(F.rp().rp_accum_error_device_ws(self.handle, _ws_handle(workspace, self), ctypes.byref(p),
                                                ctypes.byref(e), mean.data_ptr(), var.data_ptr(), stats.data_ptr(),
                                                _stream_ptr(stream, mean.device)))

    def render_progressive(self, params: RenderParams, frames_per_launch: int = 4, max_frames: int = 64,
                           tol: float = 0.05, share: float = 0.01, denoise=None, camera=None, stream=None) -> dict:
        """Progressive rendering: launches of `frames_per_launch` frames (render_frames_device, launch number l at
        seed + done * B * W * H with B = ceil(spp / samples_per_stream), so no stream repeats) folded on the device into
        a running mean and the variance of that mean (accum_frames_device), until at most `share` of the pixels have a
        relative standard error above `tol` (accum_error_device) or `max_frames` frames are in; the last launch is
        shortened so that max_frames is met exactly.  Everything runs on `stream` (torch stream; default: current).
        After every launch the four statistics words and the counters are read back: ONE HOST SYNCHRONISATION PER
        LAUNCH, the price of deciding on the host whether to go on.
        Returns {"mean", "variance": (h, w, 3) torch f64 in frame order, "frames": n, "stats": one tuple per launch
        (frames so far, pixels, over, largest finite e2, non-finite pixels)} and, unless denoise is False, "denoised":
        the guides of render_aov_device at spp = min(n * spp, 64), then denoise_device(variance=...) (`denoise`: as
        denoise_var_params takes it).  One device holds the whole frame (num_shards = 1, interleave)."""
        import torch
        from dataclasses import replace
        _progressive_args(params, "render_progressive", frames_per_launch, max_frames, tol, share)
        dev = torch.device("cuda", self.device)
        s = _stream(stream, dev)
        w, h, n = params.width, params.height, shard_slot_count(params)
        nbatch = -(-params.spp // (params.samples_per_stream or F.RP_SAMPLES_PER_STREAM))
        self.reserve_frames(params, frames_per_launch)
        done, log = 0, []
        with torch.cuda.stream(s):
            frames, mean, m2, var, ctr, stats = _progressive_state(params, frames_per_launch, dev)
            while done < max_frames:
                k = min(frames_per_launch, max_frames - done)
                q = replace(params, seed=(params.seed + done * nbatch * w * h) & 0xFFFFFFFFFFFFFFFF)
                self.render_frames_device(q, k, frames, ctr, camera=camera, stream=s)
                accum_frames_device(frames, k, mean, m2, n_prior=done, var=var, n_words=3 * n, stream=s)
                self.accum_error_device(params, mean, var, stats, tol=tol, stream=s)
                done += k
                s.synchronize()  # the one host synchronisation of the launch: the loop's decision needs the counts
                st, status = error_stats(stats.cpu().numpy()), int(ctr[3])
                if status:
                    raise RuntimeError(f"render_progressive: device status {status:#x} after {done} frames")
                log.append((done,) + st)
                if st[1] <= share * st[0]:
                    break
            return self._progressive_result(params, mean, var, done, {"frames": done, "stats": log}, denoise, camera, s)

    def _progressive_result(self, params: RenderParams, mean, var, frames: int, out: dict, denoise, camera, s) -> dict:
        """What render_progressive and render_adaptive return from their state (compact shard buffers, on stream s,
        which is current): "mean" and "variance" in frame order (rp_frame_assemble) and, unless denoise is False,
        "denoised" with the guides at min(frames * spp, 64) spp."""
        import torch
        from dataclasses import replace
        dev = mean.device
        w, h, n = params.width, params.height, shard_slot_count(params)
        for key in ("mean", "variance"):
            out[key] = torch.empty((h, w, 3), dtype=torch.float64, device=dev)
        _assemble(params, {"mean": mean, "variance": var}, out, _stream_ptr(s))
        if denoise is False:
            return out
        ga = replace(params, spp=min(frames * params.spp, 64))
        bufs = (("normal", 3), ("albedo", 3), ("depth", 1))
        shard = {k_: torch.empty(c * n, dtype=torch.float64, device=dev) for k_, c in bufs}
        self.render_aov_device(ga, normal=shard["normal"], albedo=shard["albedo"], depth=shard["depth"],
                               camera=camera, stream=s)
        guide = {k_: torch.empty(c * w * h, dtype=torch.float64, device=dev) for k_, c in bufs}
        _assemble(ga, shard, guide, _stream_ptr(s))
        out["denoised"] = torch.empty((h, w, 3), dtype=torch.float64, device=dev)
        denoise_device(out["mean"], guide["normal"], guide["albedo"], guide["depth"], out["denoised"],
                       params=denoise, stream=s, variance=out["variance"])
        return out

    # ---- a camera sequence with reprojected history (rp_reproject_device) ----------------------
    def render_sequence(self, params: RenderParams, cameras, frames_per_pose: int = 2, max_history: int = 32,
                        var_one: float = 1.0, reproject=None, denoise=None, stream=None):
        """An animation that keeps its accumulated history across camera moves: a generator over `cameras` (Camera
        objects), one dict per pose.  Pose t renders `frames_per_pose` frames (render_frames_device at
        seed + t * frames_per_pose * B * W * H, B = ceil(spp / samples_per_stream), so no stream repeats) and the guides
        (render_aov_device) at its camera, assembles them to frame order, carries pose t - 1's mean, m2 and per-pixel
        frame count to the new pixels (reproject_device with reproject_prev_camera(pose t - 1's camera), so a tilted
        lookat camera reprojects exactly; pose 0 starts from zero counts), folds the new frames in with
        the frame number taken per pixel (accum_frames_counts_device; a pixel with one frame gets the variance
        `var_one`) and, unless denoise is False, filters the mean with that variance (denoise_device(variance=...);
        `denoise`: as denoise_var_params takes it).  reproject: as reproject_params takes it; max_history overrides
        its field.  Everything runs on `stream` (torch stream; default: current) with no host synchronisation inside a
        pose.  Yields {"mean", "variance": (h, w, 3) f64, "count": (h, w) int32, "denoised": (h, w, 3) f64 or None,
        "stats": int64[RP_REPROJECT_STATS_LEN] (reproject_stats decodes them; pose 0: every pixel, nothing kept)},
        torch tensors on the scene's device, valid once the stream has drained.  One device holds the whole frame."""
        import torch
        from dataclasses import replace
        _whole_frame(params, "render_sequence")
        if not 1 <= frames_per_pose <= F.RP_MAX_FRAMES:
            raise ValueError(f"frames_per_pose must be 1..{F.RP_MAX_FRAMES}, got {frames_per_pose}")
        if not 1 <= max_history < 2 ** 31:
            raise ValueError(f"max_history must be 1 .. 2^31 - 1, got {max_history}")
        rp = reproject_params(reproject, max_history=max_history)
        dev = torch.device("cuda", self.device)
        s = _stream(stream, dev)
        w, h, n = params.width, params.height, shard_slot_count(params)
        nbatch = -(-params.spp // (params.samples_per_stream or F.RP_SAMPLES_PER_STREAM))
        self.reserve_frames(params, frames_per_pose)
        f64 = {"dtype": torch.float64, "device": dev}
        prev = None
        for t, cam in enumerate(cameras):
            with torch.cuda.stream(s):
                q = replace(params, seed=(params.seed + t * frames_per_pose * nbatch * w * h) & 0xFFFFFFFFFFFFFFFF)
                shard_frames = torch.empty(frames_per_pose * 3 * n, **f64)
                ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device=dev)
                self.render_frames_device(q, frames_per_pose, shard_frames, ctr, camera=cam, stream=s)
                shard = {k: torch.empty(c * n, **f64) for k, c in (("normal", 3), ("albedo", 3), ("depth", 1))}
                self.render_aov_device(params, normal=shard["normal"], albedo=shard["albedo"], depth=shard["depth"],
                                       camera=cam, stream=s)
                cur = {"normal": torch.empty((h, w, 3), **f64), "albedo": torch.empty((h, w, 3), **f64),
                       "depth": torch.empty((h, w), **f64), "camera": cam}
                frames = torch.empty((frames_per_pose, h, w, 3), **f64)
                _assemble(params, shard, cur, _stream_ptr(s))
                _assemble(params, {f: shard_frames[f * 3 * n:(f + 1) * 3 * n] for f in range(frames_per_pose)}, frames,
                          _stream_ptr(s))
                cur.update(mean=torch.empty((h, w, 3), **f64), m2=torch.empty((h, w, 3), **f64))
                var = torch.empty((h, w, 3), **f64)
                stats = torch.zeros(F.RP_REPROJECT_STATS_LEN, dtype=torch.int64, device=dev)
                if prev is None:
                    cur["count"] = torch.zeros((h, w), dtype=torch.int32, device=dev)
                    stats[:1].fill_(w * h)
                else:
                    cur["count"] = torch.empty((h, w), dtype=torch.int32, device=dev)
                    reproject_device(cam, reproject_prev_camera(prev["camera"]), cur["depth"], cur["normal"],
                                     prev["depth"], prev["normal"],
                                     prev["mean"], prev["m2"], prev["count"], cur["mean"], cur["m2"], cur["count"],
                                     stats, params=rp, stream=s)
                accum_frames_counts_device(frames, frames_per_pose, cur["count"], cur["mean"], cur["m2"], var=var,
                                           var_one=var_one, stream=s)
                out = None
                if denoise is not False:
                    out = torch.empty((h, w, 3), **f64)
                    denoise_device(cur["mean"], cur["normal"], cur["albedo"], cur["depth"], out, params=denoise,
                                   stream=s, variance=var)
                prev = cur
            yield {"mean": cur["mean"], "variance": var, "count": cur["count"], "denoised": out, "stats": stats}

    # ---- tile-adaptive progressive rendering (rp_render_tiles_device_ws, rp_accum_tiles_*) ------
    def render_tiles_device(self, params: RenderParams, tiles, n_listed: int, n_frames: int, out, counters, fg=None,
                            camera=None, stream=None, workspace: "Workspace | None" = None, order="auto") -> None:
        """rp_render_tiles_device_ws: n_frames frames of the n_listed frame tiles `tiles` names (torch int32 on the
        scene's device, row-major tile indices of the whole frame `params` describes), frame f at seed + f * W * H.
        out: torch f64, listed tile k at slot k * tw * th, frame f at f * 3 * n_listed * tw * th; fg likewise in floats or
        None; counters: int64, RP_COUNTERS_LEN, zeroed and filled by the launch.  One stream per pixel only."""
        import torch
        cam = (camera or self.scene.camera).to_c()
        p = params.to_c()
        slots = n_listed * (params.tile_w or 32) * (params.tile_h or 32)
        if tiles is not None:
            _check_tensor(tiles, torch.int32, n_listed)
        _check_tensor(out, torch.float64, 3 * slots * n_frames, contiguous=False)
        assert fg is None or (fg.dtype == torch.float32 and fg.numel() >= slots * n_frames)
        _check_tensor(counters, torch.int64, F.RP_COUNTERS_LEN, contiguous=False)
        F.check(F.rp().rp_render_tiles_device_ws(
            self.handle, _ws_handle(workspace, self), ctypes.byref(cam), ctypes.byref(p),
            tiles.data_ptr() if tiles is not None else None, n_listed, n_frames, _FRAME_ORDER.get(order, order),
            out.data_ptr(), fg.data_ptr() if fg is not None else None, counters.data_ptr(),
            _stream_ptr(stream, out.device)))

    def render_adaptive(self, params: RenderParams, frames_per_launch: int = 4, max_frames: int = 64,
                        max_launch_frames: int = 16, tol: float = 0.05, share: float = 0.01, tile_share=None,
                        denoise=None, camera=None, stream=None) -> dict:
        """Tile-adaptive progressive rendering: render_progressive's first launch over the whole frame, then launches
        over the tiles still over the tolerance only.  After every launch accum_tiles_select_device keeps, of the current
        list, the tiles with more than `tile_share` (default: share) of their pixels over `tol`; the loop stops when the
        list is empty, when at most `share` of all pixels are over, or at max_frames.  With A of T tiles active a launch
        renders k = min(max_launch_frames, max_frames - done, frames_per_launch * (T // A)) frames of them
        (render_tiles_device at seed + done * W * H) and folds them with accum_frames_tiles_device: about the first
        launch's unit count, always inside its frames buffer.  ONE HOST SYNCHRONISATION PER LAUNCH, as
        render_progressive.  One stream per pixel (samples_per_stream >= spp), one device, at most 16384 tiles.
        Returns {"mean", "variance": (h, w, 3) torch f64 in frame order -- each pixel the progressive mean of its own
        tile's first n_t frames, and the variance of that mean --, "tile_frames": (tiles_y, tiles_x) int32 numpy, n_t,
        "frames": the largest n_t, "samples", "rays": the counters' sums, "log": per launch (frames done before it, its
        tiles, its frames) + error_stats after it, "launch_ms": per launch the device time of its render, fold, error
        pass and select (events on the stream)} and, unless denoise is False, "denoised" as render_progressive's."""
        import torch
        from dataclasses import replace
        _progressive_args(params, "render_adaptive", frames_per_launch, max_frames, tol, share)
        if not 1 <= max_launch_frames <= F.RP_MAX_FRAMES:
            raise ValueError(f"max_launch_frames must be 1..{F.RP_MAX_FRAMES}, got {max_launch_frames}")
        tile_share = share if tile_share is None else tile_share
        if not 0.0 <= tile_share < 1.0:
            raise ValueError(f"tile_share must be in [0, 1), got {tile_share}")
        if params.spp < 1 or (params.samples_per_stream or F.RP_SAMPLES_PER_STREAM) < params.spp:
            raise ValueError("render_adaptive needs one stream per pixel: 1 <= spp <= samples_per_stream")
        dev = torch.device("cuda", self.device)
        s = _stream(stream, dev)
        w, h, n = params.width, params.height, shard_slot_count(params)
        tw, th = params.tile_w or 32, params.tile_h or 32
        tiles_x, tiles_y = -(-w // tw), -(-h // th)
        T, tile_words = tiles_x * tiles_y, 3 * tw * th
        if T > 16384:
            raise ValueError(f"render_adaptive selects among at most 16384 tiles, the frame has {T}")
        self.reserve_frames(params, frames_per_launch)
        tile_frames = np.zeros(T, dtype=np.int32)
        done, log, samples, rays = 0, [], 0, 0
        with torch.cuda.stream(s):
            frames, mean, m2, var, ctr, stats = _progressive_state(params, frames_per_launch, dev)
            lists = [torch.empty(T, dtype=torch.int32, device=dev) for _ in range(2)]
            count = torch.zeros(1, dtype=torch.int32, device=dev)
            cur, active, listed = None, T, np.arange(T)  # the list the next select reads: None = identity
            k = min(frames_per_launch, max_frames)
            marks = [torch.cuda.Event(enable_timing=True)]  # one before the first launch, one after every select
            marks[0].record(s)
            self.render_frames_device(params, k, frames, ctr, camera=camera, stream=s)
            accum_frames_device(frames, k, mean, m2, n_prior=0, var=var, n_words=3 * n, stream=s)
            while True:
                self.accum_error_device(params, mean, var, stats, tol=tol, stream=s)
                nxt = lists[1] if cur is lists[0] else lists[0]
                accum_tiles_select_device(params, mean, var, nxt, count, tiles_in=cur, n_in=active, tol=tol,
                                          tile_share=tile_share, stream=s)
                marks.append(torch.cuda.Event(enable_timing=True))
                marks[-1].record(s)
                s.synchronize()  # the one host synchronisation of the launch: the loop's decision needs the counts
                c = ctr.cpu().numpy()
                st, n_next = error_stats(stats.cpu().numpy()), int(count[0])
                if int(c[3]):
                    raise RuntimeError(f"render_adaptive: device status {int(c[3]):#x} after {done + k} frames")
                rays, samples = rays + int(c[0]), samples + int(c[1])
                tile_frames[listed] += k
                log.append((done, active, k) + st)
                done += k
                if n_next == 0 or st[1] <= share * st[0] or done == max_frames:
                    break
                cur, active, listed = nxt, n_next, nxt[:n_next].cpu().numpy()
                k = min(max_launch_frames, max_frames - done, frames_per_launch * (T // active))
                q = replace(params, seed=(params.seed + done * w * h) & 0xFFFFFFFFFFFFFFFF)
                self.render_tiles_device(q, cur, active, k, frames, ctr, camera=camera, stream=s)
                accum_frames_tiles_device(frames, k, cur, active, tile_words, mean, m2, n_prior=done, var=var,
                                          n_state_tiles=T, stream=s)
            out = {"frames": done, "tile_frames": tile_frames.reshape(tiles_y, tiles_x), "samples": samples,
                   "rays": rays, "log": log, "launch_ms": [a.elapsed_time(b) for a, b in zip(marks, marks[1:])]}
            return self._progressive_result(params, mean, var, done, out, denoise, camera, s)

    def to_bgra8(self, params: RenderParams, shard_rgb, out, stream=None) -> None:
        """Output stage on the device (rp_shard_to_bgra8): the shard's linear f64 RGB (`shard_rgb`, torch
        f64) -> to_srgb_u8 bytes in TGA order B, G, R, A into `out` (torch uint8, >= 4 * slots)."""
        import torch
        n = shard_slot_count(params)
        _check_tensor(shard_rgb, torch.float64, 3 * n, contiguous=False)
        _check_tensor(out, torch.uint8, 4 * n, contiguous=False)
        p = params.to_c()
        F.check(F.rp().rp_shard_to_bgra8(self.handle, ctypes.byref(p), shard_rgb.data_ptr(), out.data_ptr(),
                                         _stream_ptr(stream, out.device)))

    def frame_gather(self, comm: "Comm", params: RenderParams, shard_rgb, frame_bgra=None, frame_rgb=None,
                     counters=None, stream=None, workspace: "Workspace | None" = None) -> None:
        """rp_frame_gather: this rank's finished shard (`shard_rgb`, torch f64) all-gathered over RCCL with the
        other ranks' and de-interleaved into frame order: `frame_bgra` (torch uint8, W*H*4: to_srgb_u8 in
        tga::save order) and/or `frame_rgb` (torch f64, W*H*3); `counters` (int64, 4) summed over ranks."""
        import torch
        n = params.width * params.height
        if frame_bgra is not None:
            _check_tensor(frame_bgra, torch.uint8, 4 * n, contiguous=False)
        if frame_rgb is not None:
            _check_tensor(frame_rgb, torch.float64, 3 * n, contiguous=False)
        p = params.to_c()
        F.check(F.rp().rp_frame_gather(comm.handle, self.handle, _ws_handle(workspace),
                                       ctypes.byref(p), shard_rgb.data_ptr(),
                                       frame_bgra.data_ptr() if frame_bgra is not None else None,
                                       frame_rgb.data_ptr() if frame_rgb is not None else None,
                                       counters.data_ptr() if counters is not None else None,
                                       _stream_ptr(stream, shard_rgb.device)))

    def frames_gather(self, comm: "Comm", params: RenderParams, n_frames: int, shard_rgb, frames_bgra=None,
                      counters=None, stream=None, workspace: "Workspace | None" = None) -> None:
        """rp_frames_gather: the n_frames shards of one render_frames_device launch (`shard_rgb`, back to back) in one
        all-gather; `frames_bgra` (torch uint8, n_frames * W*H*4) receives the assembled frames back to back."""
        import torch
        n = params.width * params.height
        if frames_bgra is not None:
            _check_tensor(frames_bgra, torch.uint8, 4 * n * n_frames, contiguous=False)
        assert shard_rgb.dtype == torch.float64 and shard_rgb.numel() >= 3 * shard_slot_count(params) * n_frames
        p = params.to_c()
        F.check(F.rp().rp_frames_gather(comm.handle, self.handle, _ws_handle(workspace),
                                        ctypes.byref(p), n_frames, shard_rgb.data_ptr(),
                                        frames_bgra.data_ptr() if frames_bgra is not None else None,
                                        counters.data_ptr() if counters is not None else None,
                                        _stream_ptr(stream, shard_rgb.device)))

    def frames_block_words(self, params: RenderParams, n_frames: int) -> int:
        """rp_frames_block_words: 32-bit words of one rank's packed block for a launch of n_frames frames (the same on
        every rank of the job)."""
        p = params.to_c()
        w = ctypes.c_uint64()
        F.check(F.rp().rp_frames_block_words(ctypes.byref(p), n_frames, ctypes.byref(w)))
        return w.value

    def frames_pack(self, params: RenderParams, n_frames: int, shard_rgb, counters, send, stream=None,
                    workspace: "Workspace | None" = None) -> None:
        """rp_frames_pack: this rank's half of rp_frames_gather without the collective -- the launch's n_frames shards
        (output stage to BGRA8) and its counters into `send` (torch int32, frames_block_words words), for a caller's
        own all-gather."""
        import torch
        _check_tensor(send, torch.int32, self.frames_block_words(params, n_frames), contiguous=False)
        p = params.to_c()
        F.check(F.rp().rp_frames_pack(self.handle, _ws_handle(workspace), ctypes.byref(p), n_frames,
                                      shard_rgb.data_ptr(), counters.data_ptr(), send.data_ptr(),
                                      _stream_ptr(stream, shard_rgb.device)))

    def frames_unpack(self, params: RenderParams, n_frames: int, recv, frames_bgra, counters=None, stream=None,
                      workspace: "Workspace | None" = None) -> None:
        """rp_frames_unpack: the all-gathered blocks of every rank (`recv`, rank-major) de-interleaved into the n_frames
        assembled BGRA8 frames and the counters summed over the ranks."""
        n = params.width * params.height
        assert frames_bgra.is_cuda and frames_bgra.numel() * frames_bgra.element_size() >= 4 * n * n_frames
        p = params.to_c()
        F.check(F.rp().rp_frames_unpack(self.handle, _ws_handle(workspace), ctypes.byref(p), n_frames,
                                        recv.data_ptr(), frames_bgra.data_ptr(),
                                        counters.data_ptr() if counters is not None else None,
                                        _stream_ptr(stream, recv.device)))

    def render_gather(self, comm: "Comm", params: RenderParams, frame_bgra=None, frame_rgb=None, counters=None,
                      camera=None, stream=None, workspace: "Workspace | None" = None) -> None:
        """rp_render_gather: render this rank's shard and gather the frame (see frame_gather)."""
        dev = (frame_bgra if frame_bgra is not None else frame_rgb).device
        cam = (camera or self.scene.camera).to_c()
        p = params.to_c()
        F.check(F.rp().rp_render_gather(comm.handle, self.handle, _ws_handle(workspace),
                                        ctypes.byref(cam), ctypes.byref(p),
                                        frame_bgra.data_ptr() if frame_bgra is not None else None,
                                        frame_rgb.data_ptr() if frame_rgb is not None else None,
                                        counters.data_ptr() if counters is not None else None,
                                        _stream_ptr(stream, dev)))

    def intersect(self, rays: np.ndarray):
        """Hittable::hit on the root for (n, 8) rays -> ((n, 9) hits, (n,) material ids)."""
        r = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 8)
        hits = np.empty((len(r), 9), dtype=np.float64)
        mats = np.empty(len(r), dtype=np.uint32)
        F.check(F.rp().rp_intersect(self.handle, r.ctypes.data, len(r), hits.ctypes.data, mats.ctypes.data))
        return hits, mats


class Refit:
    """rp_refit: new vertex positions, vertex normals and sphere records for a DeviceScene, its tree refit in place
    (include/rp.h).  Arrays as DeviceScene.geometry() numbers them; None means unchanged.  An update of the geometry names
    all of it: positions when the scene has triangles, spheres when it has spheres.  The caller orders updates against
    renders of the scene (streams); the scene's host description is not touched."""

    def __init__(self, scene: DeviceScene, coord_max: float = 0.0):
        h = ctypes.c_void_p()
        F.check(F.rp().rp_refit_create(scene.handle, float(coord_max), ctypes.byref(h)))
        self.scene = scene
        self.handle = h

    def info(self) -> dict:
        """rp_refit_info: {"vertices", "spheres", "levels", "bound"}."""
        nv, ns, nl, b = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_double()
        F.check(F.rp().rp_refit_info(self.handle, ctypes.byref(nv), ctypes.byref(ns), ctypes.byref(nl), ctypes.byref(b)))
        return {"vertices": nv.value, "spheres": ns.value, "levels": nl.value, "bound": b.value}

    def update_device(self, positions=None, normals=None, spheres=None, status=None, stream=None):
        """rp_scene_refit_device on `stream` (torch stream; default: current): torch f64 tensors on the scene's device,
        positions and normals of 3 * vertices elements, spheres of 4 * spheres.  status: a torch int32 tensor of one
        element (allocated when None).  Returns the status tensor: RP_REFIT_OUT_OF_BOUND or 0 once the stream got there."""
        import torch
        info = self.info()
        dev = torch.device("cuda", self.scene.device)
        for t, m in ((positions, 3 * info["vertices"]), (normals, 3 * info["vertices"]), (spheres, 4 * info["spheres"])):
            if t is not None:
                _check_tensor(t, torch.float64, m, dev)
        if status is None:
            status = torch.zeros(1, dtype=torch.int32, device=dev)
        _check_tensor(status, torch.int32, 1, dev)
        ptr = [t.data_ptr() if t is not None else None for t in (positions, normals, spheres)]
        F.check(F.rp().rp_scene_refit_device(self.handle, ptr[0], ptr[1], ptr[2], status.data_ptr(), _stream_ptr(stream, dev)))
        return status

    def update(self, positions=None, normals=None, spheres=None) -> tuple:
        """rp_scene_refit: the same from numpy arrays, synchronous.  -> (status, seconds of the kernels)."""
        info = self.info()
        arrs = []
        for a, m in ((positions, 3 * info["vertices"]), (normals, 3 * info["vertices"]), (spheres, 4 * info["spheres"])):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
                if a.size != m:
                    raise ValueError(f"a refit array of {a.size} doubles, the scene takes {m}")
            arrs.append(a)
        st, sec = ctypes.c_uint32(), ctypes.c_double()
        F.check(F.rp().rp_scene_refit(self.handle, *[a.ctypes.data if a is not None else None for a in arrs],
                                      ctypes.byref(st), ctypes.byref(sec)))
        return st.value, sec.value

    def close(self) -> None:
        if getattr(self, "handle", None):
            F.rp().rp_refit_destroy(self.handle)
            self.handle = None
            rs = self.scene.__dict__.get("_refits", [])
            if self in rs:
                rs.remove(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def scene_geometry(scene: Scene) -> dict:
    """DeviceScene.geometry() of a host scene."""
    meshes = scene.scene_data.mesh_table
    pos = np.concatenate([m.positions for m in meshes]) if meshes else np.zeros((0, 3))
    nrm = np.concatenate([m.normals for m in meshes]) if meshes else np.zeros((0, 3))
    root = np.asarray(scene.root, dtype=F.hittable_dtype())
    sph = root[root["kind"] == F.RP_HITTABLE_SPHERE]
    spheres = np.concatenate([sph["center"], sph["radius"][:, None]], axis=1) if len(sph) else np.zeros((0, 4))
    return {"positions": np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3),
            "normals": np.ascontiguousarray(nrm, dtype=np.float64).reshape(-1, 3),
            "spheres": np.ascontiguousarray(spheres, dtype=np.float64).reshape(-1, 4)}


def with_geometry(scene: Scene, positions=None, normals=None, spheres=None) -> Scene:
    """A copy of a host scene with its geometry replaced (arrays as scene_geometry numbers them; None: kept): the
    description a refit scene is compared with."""
    from .scene import Mesh, SceneData
    meshes, vb = [], 0
    for m in scene.scene_data.mesh_table:
        nv = len(m.positions)
        meshes.append(Mesh(np.array(positions[vb:vb + nv]) if positions is not None else m.positions.copy(),
                           np.array(normals[vb:vb + nv]) if normals is not None else m.normals.copy(),
                           m.uvs, m.indices, m.material))
        vb += nv
    root = np.array(scene.root, dtype=F.hittable_dtype())
    if spheres is not None:
        rows = np.nonzero(root["kind"] == F.RP_HITTABLE_SPHERE)[0]
        sp = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
        root["center"][rows] = sp[:, :3]
        root["radius"][rows] = sp[:, 3]
    sd = SceneData(scene.scene_data.material_table, scene.scene_data.texture_table, meshes)
    return Scene(scene.camera, sd, root, scene.background, scene.root_kind, scene.name)


def refit_records_host(tree: dict, positions=None, normals=None, spheres=None, bound: float = 2.0 ** 54,
                       tri_normals=None, n_vertices=None, n_spheres=None) -> int:
    """rph_refit_records, the CPU model of Refit.update: refits `tree` (DeviceScene.tree()'s dict: "node_format", "root",
    "nodes", "prims", "prim_refs") IN PLACE; tri_normals: the per-primitive normals (_ffi.tri_normals_dtype, rewritten
    when normals are given).  bound: finite.  n_vertices, n_spheres default to the arrays' lengths.  -> the status."""
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (positions, normals, spheres)]
    nv = n_vertices if n_vertices is not None else max([a.size // 3 for a in arrs[:2] if a is not None], default=0)
    ns = n_spheres if n_spheres is not None else (arrs[2].size // 4 if arrs[2] is not None else 0)
    ptr = [a.ctypes.data if a is not None and a.size else None for a in arrs]
    for k in ("nodes", "prims", "prim_refs"):
        assert tree[k].flags["C_CONTIGUOUS"]
    st = ctypes.c_uint32()
    F.check_host(F.host().rph_refit_records(tree["node_format"], tree["nodes"].ctypes.data, len(tree["nodes"]), tree["root"],
                                            tree["prims"].ctypes.data, tree["prim_refs"].ctypes.data,
                                            tri_normals.ctypes.data if tri_normals is not None else None,
                                            len(tree["prims"]), ptr[0], ptr[1], ptr[2], nv, ns, bound, ctypes.byref(st)))
    return st.value


class Workspace:
    """rp_workspace: per-frame device state (keystream cache, queue counters, probe buffers, batch sums)."""

    def __init__(self, scene: DeviceScene):
        h = ctypes.c_void_p()
        F.check(F.rp().rp_workspace_create(scene.handle, ctypes.byref(h)))
        self.scene = scene
        self.handle = h

    def close(self) -> None:
        if getattr(self, "handle", None):
            F.rp().rp_workspace_destroy(self.handle)
            self.handle = None
            ws = self.scene.__dict__.get("_workspaces", [])
            if self in ws:
                ws.remove(self)


def comm_unique_id() -> bytes:
    """rp_comm_unique_id: the RCCL id rank 0 makes and shares with the other ranks out of band."""
    buf = (ctypes.c_uint8 * F.RP_COMM_ID_BYTES)()
    F.check(F.rp().rp_comm_unique_id(buf))
    return bytes(buf)


class Comm:
    """rp_comm: this rank's RCCL communicator (one process per GPU)."""

    def __init__(self, unique_id: bytes, nranks: int, rank: int, device: int):
        assert len(unique_id) == F.RP_COMM_ID_BYTES
        h = ctypes.c_void_p()
        buf = (ctypes.c_uint8 * F.RP_COMM_ID_BYTES).from_buffer_copy(unique_id)
        F.check(F.rp().rp_comm_create(buf, nranks, rank, device, ctypes.byref(h)))
        self.handle = h
        self.nranks, self.rank, self.device = nranks, rank, device

    def close(self) -> None:
        if getattr(self, "handle", None):
            F.rp().rp_comm_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class MultiScene:
    """rp_multi: one process driving several GPUs (a scene copy per device, one RCCL communicator)."""

    def __init__(self, scene: Scene, devices, options: dict | None = None):
        self.scene = scene
        self._desc = scene.desc()
        devs = (ctypes.c_int * len(devices))(*devices)
        opt = scene_options(**(options or {}))
        h = ctypes.c_void_p()
        F.check(F.rp().rp_multi_create(self._desc.ptr(), devs, len(devices), ctypes.byref(opt), ctypes.byref(h)))
        self.handle = h
        self.devices = list(devices)

    def render(self, params: RenderParams, camera=None, rgb: bool = True, bgra: bool = False):
        """rp_render_multi: (rgb (h, w, 3) f64 or None, bgra (h, w, 4) u8 or None, stats)."""
        cam = (camera or self.scene.camera).to_c()
        p = params.to_c()
        out = np.zeros((params.height, params.width, 3)) if rgb else None
        ob = np.zeros((params.height, params.width, 4), dtype=np.uint8) if bgra else None
        st = F.rp_stats()
        F.check(F.rp().rp_render_multi(self.handle, ctypes.byref(cam), ctypes.byref(p),
                                       out.ctypes.data if out is not None else None,
                                       ob.ctypes.data if ob is not None else None, ctypes.byref(st)))
        return out, ob, _stats_dict(st)

    def close(self) -> None:
        if getattr(self, "handle", None):
            F.rp().rp_multi_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def unpack_shard(params: RenderParams, shard_buf: np.ndarray, channels: int = 3,
                 frame: np.ndarray | None = None, tile_map=None) -> np.ndarray:
    """Scatter a compact shard buffer into a full (h, w, channels) frame (rp_shard_unpack; with `tile_map`, the
    deal order of a balanced frame, rp_shard_unpack_map)."""
    if frame is None:
        frame = np.zeros((params.height, params.width, channels), dtype=np.float64)
    src = np.ascontiguousarray(shard_buf, dtype=np.float64)
    p = params.to_c()
    if tile_map is None:
        F.check(F.rp().rp_shard_unpack(ctypes.byref(p), src.ctypes.data, channels, frame.ctypes.data))
    else:
        m = np.ascontiguousarray(tile_map, dtype=np.uint32)
        F.check(F.rp().rp_shard_unpack_map(ctypes.byref(p), m.ctypes.data, src.ctypes.data, channels,
                                           frame.ctypes.data))
    return frame


def srgb_thresholds() -> np.ndarray:
    """The 256-entry threshold table of the device output stage (rp_srgb_thresholds; host only)."""
    t = np.empty(256, dtype=np.float64)
    F.check(F.rp().rp_srgb_thresholds(t.ctypes.data))
    return t


# ---- guided denoiser (rp_denoise*, include/rp.h) --------------------------------------
def denoise_params(params=None, **kw) -> F.rp_denoise_params:
    """rp_denoise_params: `params` (an rp_denoise_params, a dict of its fields or None) with fields overridden by
    keyword.  Fields left at zero take the library's defaults (iterations 3, normal_power 6, sigma_depth 0.05,
    sigma_albedo 0.1, sigma_color 1.0 -- negative disables the colour term --, albedo_eps 1e-2)."""
    p = F.rp_denoise_params()
    if isinstance(params, F.rp_denoise_params):
        ctypes.memmove(ctypes.byref(p), ctypes.byref(params), ctypes.sizeof(p))
    elif params:
        kw = {**params, **kw}
    for k, v in kw.items():
        if not hasattr(p, k):
            raise KeyError(f"unknown denoise parameter {k!r}")
        setattr(p, k, v)
    return p


def denoise_defaults() -> F.rp_denoise_params:
    """rp_denoise_params_init: every field at its default (host only)."""
    p = F.rp_denoise_params()
    F.check(F.rp().rp_denoise_params_init(ctypes.byref(p)))
    return p


def denoise_scratch_bytes(width: int, height: int) -> int:
    """rp_denoise_scratch_bytes: device bytes denoise_device needs beside its buffers (host only)."""
    b = ctypes.c_uint64()
    F.check(F.rp().rp_denoise_scratch_bytes(width, height, ctypes.byref(b)))
    return b.value


def denoise_var_params(params=None, **kw) -> F.rp_denoise_var_params:
    """rp_denoise_var_params: `params` (an rp_denoise_var_params, an rp_denoise_params taken as its base, a dict or
    None) with fields overridden by keyword; sigma_var and var_eps beside the base's fields, all at one level.  Fields
    left at zero take the library's defaults (sigma_var 3.0, var_eps 1e-6, the base as denoise_params; base.sigma_color
    is ignored)."""
    p = F.rp_denoise_var_params()
    if isinstance(params, F.rp_denoise_var_params):
        ctypes.memmove(ctypes.byref(p), ctypes.byref(params), ctypes.sizeof(p))
    elif isinstance(params, F.rp_denoise_params):
        ctypes.memmove(ctypes.byref(p.base), ctypes.byref(params), ctypes.sizeof(params))
    elif params:
        kw = {**params, **kw}
    for k, v in kw.items():
        if k in ("sigma_var", "var_eps"):
            setattr(p, k, v)
        elif hasattr(p.base, k):
            setattr(p.base, k, v)
        else:
            raise KeyError(f"unknown denoise parameter {k!r}")
    return p


def denoise_var_defaults() -> F.rp_denoise_var_params:
    """rp_denoise_var_params_init: every field at its default (host only)."""
    p = F.rp_denoise_var_params()
    F.check(F.rp().rp_denoise_var_params_init(ctypes.byref(p)))
    return p


def denoise_var_scratch_bytes(width: int, height: int) -> int:
    """rp_denoise_var_scratch_bytes: device bytes denoise_device(variance=...) needs beside its buffers (host only)."""
    b = ctypes.c_uint64()
    F.check(F.rp().rp_denoise_var_scratch_bytes(width, height, ctypes.byref(b)))
    return b.value


def _host_frames(rgb, normal, albedo, depth, variance=None):
    rgb = np.ascontiguousarray(rgb, dtype=np.float64)
    assert rgb.ndim == 3 and rgb.shape[2] == 3, "rgb: (h, w, 3)"
    h, w = rgb.shape[:2]
    guides = []
    for name, g, shape in (("normal", normal, (h, w, 3)), ("albedo", albedo, (h, w, 3)), ("depth", depth, (h, w)),
                           ("variance", variance, (h, w, 3))):
        if g is not None:
            g = np.ascontiguousarray(g, dtype=np.float64)
            assert g.shape == shape, f"{name}: {shape}, got {g.shape}"
        guides.append(g)
    return rgb, guides[:3], h, w, guides[3]


def denoise(rgb, normal=None, albedo=None, depth=None, params=None, device: int = 0, variance=None):
    """rp_denoise on host arrays in frame order -- rgb, normal, albedo (h, w, 3), depth (h, w), each guide optional --
    through the device kernel: (denoised (h, w, 3) f64, device seconds of the levels).  variance (h, w, 3): the
    variance-guided filter (rp_denoise_var; params as denoise_var_params takes them)."""
    rgb, guides, h, w, var = _host_frames(rgb, normal, albedo, depth, variance)
    out = np.empty_like(rgb)
    sec = ctypes.c_double()
    gp = [g.ctypes.data if g is not None else None for g in guides]
    if var is None:
        p = denoise_params(params)
        F.check(F.rp().rp_denoise(ctypes.byref(p), device, w, h, rgb.ctypes.data, *gp, out.ctypes.data,
                                  ctypes.byref(sec)))
    else:
        p = denoise_var_params(params)
        F.check(F.rp().rp_denoise_var(ctypes.byref(p), device, w, h, rgb.ctypes.data, var.ctypes.data, *gp,
                                      out.ctypes.data, ctypes.byref(sec)))
    return out, sec.value


def denoise_host(rgb, normal=None, albedo=None, depth=None, params=None, variance=None) -> np.ndarray:
    """rph_denoise: the same filter on the CPU (librp_host.so; the same arithmetic header as the kernel, equal bits).
    variance (h, w, 3): rph_denoise_var, the variance-guided filter."""
    rgb, guides, h, w, var = _host_frames(rgb, normal, albedo, depth, variance)
    out = np.empty_like(rgb)
    gp = [g.ctypes.data if g is not None else None for g in guides]
    if var is None:
        p = denoise_params(params)
        F.check_host(F.host().rph_denoise(ctypes.byref(p), w, h, rgb.ctypes.data, *gp, out.ctypes.data))
    else:
        p = denoise_var_params(params)
        F.check_host(F.host().rph_denoise_var(ctypes.byref(p), w, h, rgb.ctypes.data, var.ctypes.data, *gp,
                                              out.ctypes.data))
    return out


def batch_variance_host(sums, spp: int, samples_per_stream: int = 0) -> np.ndarray:
    """rph_batch_variance: the variance pass's arithmetic on the CPU.  sums (..., B, 3): every pixel's batch sums,
    B = ceil(spp / samples_per_stream); returns (..., 3)."""
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    sps = samples_per_stream or F.RP_SAMPLES_PER_STREAM
    assert sums.ndim >= 2 and sums.shape[-1] == 3 and sums.shape[-2] == (spp + sps - 1) // sps, sums.shape
    var = np.empty(sums.shape[:-2] + (3,), dtype=np.float64)
    F.check_host(F.host().rph_batch_variance(spp, samples_per_stream, var.size // 3, sums.ctypes.data, var.ctypes.data))
    return var


# ---- progressive accumulation (rp_accum_*, include/rp.h) --------------------------------
def _accum_shape(n_frames: int, n_words, stride, mean_len: int, frames_len: int):
    n_words = mean_len if n_words is None else int(n_words)
    stride = n_words if stride is None else int(stride)
    # what the library would read and write must lie inside the buffers; its own refusals stay the library's
    assert n_words <= mean_len, f"mean, m2 and var hold {mean_len} words, n_words = {n_words}"
    if n_frames >= 1 and stride >= n_words:
        assert frames_len >= (n_frames - 1) * stride + n_words, "frames: (n_frames - 1) * stride + n_words words"
    return n_words, stride


def accum_frames_device(frames, n_frames: int, mean, m2, n_prior: int = 0, var=None, n_words=None, stride=None,
                        stream=None) -> None:
    """rp_accum_frames_device on torch f64 tensors of one device, asynchronously on `stream` (torch stream; default:
    current): the n_frames blocks of `frames` (block f at f * stride; stride default n_words, n_words default
    mean.numel()) folded in order into the running `mean` and `m2`, which hold n_prior frames already (0: they are only
    written); `var` (optional) receives the variance of the mean after n_prior + n_frames frames.  Elementwise: shard
    buffers, full frames, anything."""
    import torch
    for t in (frames, mean, m2, var):
        if t is not None:
            _check_tensor(t, torch.float64, 0, device=mean.device)
    small = min(t.numel() for t in (mean, m2, var) if t is not None)
    n_words, stride = _accum_shape(n_frames, n_words, stride, small, frames.numel())
    with torch.cuda.device(mean.device):
        F.check(F.rp().rp_accum_frames_device(n_words, n_prior, n_frames, frames.data_ptr(), stride, mean.data_ptr(),
                                              m2.data_ptr(), var.data_ptr() if var is not None else None,
                                              _stream_ptr(stream, mean.device)))


def accum_frames_host(frames, n_frames: int, mean, m2, n_prior: int = 0, var=None, n_words=None, stride=None) -> None:
    """rph_accum_frames: the same fold on the CPU (librp_host.so; the same arithmetic header as the kernel, equal
    bits), in place on contiguous numpy f64 arrays."""
    for a in (frames, mean, m2, var):
        if a is not None:
            assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous
    for a in (mean, m2, var):
        assert a is None or a.flags.writeable
    small = min(a.size for a in (mean, m2, var) if a is not None)
    n_words, stride = _accum_shape(n_frames, n_words, stride, small, frames.size)
    F.check_host(F.host().rph_accum_frames(n_words, n_prior, n_frames, frames.ctypes.data, stride, mean.ctypes.data,
                                           m2.ctypes.data, var.ctypes.data if var is not None else None))


def error_stats(stats) -> tuple:
    """The RP_ERROR_STATS_LEN words of an error pass as (pixels, over, largest finite e2 as a float, non-finite)."""
    w = np.asarray(stats).reshape(-1)[:F.RP_ERROR_STATS_LEN].astype(np.uint64)
    return int(w[0]), int(w[1]), float(w[2:3].view(np.float64)[0]), int(w[3])


def accum_error_host(mean, var, tol: float = 0.0, eps: float = 0.0) -> np.ndarray:
    """rph_accum_error: the error statistics of full frames mean and var ((h, w, 3) or (pixels, 3) f64) on the CPU:
    uint64[RP_ERROR_STATS_LEN], as rp_accum_error_device_ws defines them (error_stats() decodes them)."""
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    var = np.ascontiguousarray(var, dtype=np.float64)
    assert mean.shape == var.shape and mean.shape[-1] == 3, (mean.shape, var.shape)
    stats = np.zeros(F.RP_ERROR_STATS_LEN, dtype=np.uint64)
    e = F.rp_error_params(tol, eps)
    F.check_host(F.host().rph_accum_error(ctypes.byref(e), mean.size // 3, mean.ctypes.data, var.ctypes.data,
                                          stats.ctypes.data))
    return stats


# ---- tile-adaptive progressive rendering (rp_accum_tiles_*, include/rp.h) ----------------
def accum_tiles_select_device(params: RenderParams, mean, var, tiles_out, count, tiles_in=None, n_in=None, over=None,
                              tol: float = 0.0, eps: float = 0.0, tile_share: float = 0.0, stream=None) -> None:
    """rp_accum_tiles_select_device on torch tensors of one device, asynchronously on `stream` (torch stream; default:
    current): of the n_in tiles `tiles_in` lists (int32; None = the identity list 0 .. n_in - 1, n_in default: the
    list's length or the frame's tile count), those with more than tile_share of their in-frame pixels over the
    tolerance go, in list order, to `tiles_out` (int32, >= n_in) and their number to count[0] (int32); `over` (int32,
    >= n_in, optional) receives every listed tile's count.  mean, var: the whole frame's compact shard buffers (f64)."""
    import torch
    n = shard_slot_count(params)
    for t in (mean, var):
        _check_tensor(t, torch.float64, 3 * n)
    if n_in is None:
        n_in = tiles_in.numel() if tiles_in is not None else n // ((params.tile_w or 32) * (params.tile_h or 32))
    for t, m in ((tiles_in, n_in), (over, n_in), (tiles_out, n_in), (count, 1)):
        if t is not None:
            _check_tensor(t, torch.int32, m, device=mean.device)
    p = params.to_c()
    e = F.rp_error_params(tol, eps)
    with torch.cuda.device(mean.device):
        F.check(F.rp().rp_accum_tiles_select_device(
            ctypes.byref(p), ctypes.byref(e), tile_share, mean.data_ptr(), var.data_ptr(),
            tiles_in.data_ptr() if tiles_in is not None else None, n_in, over.data_ptr() if over is not None else None,
            tiles_out.data_ptr(), count.data_ptr(), _stream_ptr(stream, mean.device)))


def accum_tiles_select_host(params: RenderParams, mean, var, tiles_in=None, n_in=None, tol: float = 0.0,
                            eps: float = 0.0, tile_share: float = 0.0) -> tuple:
    """rph_accum_tiles_select: the same selection on the CPU (librp_host.so; the same arithmetic header as the kernels).
    mean, var: contiguous numpy f64, the whole frame's compact shard buffers.  Returns (active tiles in list order,
    every listed tile's over count), both uint32."""
    for a in (mean, var):
        assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous
        assert a.size >= 3 * shard_slot_count(params)
    if tiles_in is not None:
        tiles_in = np.ascontiguousarray(tiles_in, dtype=np.uint32)
    if n_in is None:
        n_in = tiles_in.size if tiles_in is not None else (
            shard_slot_count(params) // ((params.tile_w or 32) * (params.tile_h or 32)))
    assert tiles_in is None or tiles_in.size >= n_in
    over = np.zeros(max(n_in, 1), dtype=np.uint32)
    out = np.zeros(max(n_in, 1), dtype=np.uint32)
    count = np.zeros(1, dtype=np.uint32)
    p = params.to_c()
    e = F.rp_error_params(tol, eps)
    F.check_host(F.host().rph_accum_tiles_select(
        ctypes.byref(p), ctypes.byref(e), tile_share, mean.ctypes.data, var.ctypes.data,
        tiles_in.ctypes.data if tiles_in is not None else None, n_in, over.ctypes.data, out.ctypes.data,
        count.ctypes.data))
    return out[:int(count[0])].copy(), over[:n_in].copy()


def _tiles_shape(n_frames: int, n_listed: int, tile_words: int, stride, n_state_tiles, state_len: int, frames_len: int):
    stride = n_listed * tile_words if stride is None else int(stride)
    n_state_tiles = state_len // tile_words if n_state_tiles is None and tile_words > 0 else int(n_state_tiles or 0)
    # what the library would read and write must lie inside the buffers; its own refusals stay the library's
    assert n_state_tiles * tile_words <= state_len, f"mean, m2 and var hold {state_len} words"
    if n_frames >= 1 and stride >= n_listed * tile_words:
        assert frames_len >= (n_frames - 1) * stride + n_listed * tile_words, "frames: too short for the listed blocks"
    return stride, n_state_tiles


def accum_frames_tiles_device(frames, n_frames: int, tiles, n_listed: int, tile_words: int, mean, m2, n_prior: int = 0,
                              var=None, stride=None, n_state_tiles=None, stream=None) -> None:
    """rp_accum_frames_tiles_device on torch tensors of one device, asynchronously on `stream` (torch stream; default:
    current): listed block k (tile_words doubles at f * stride + k * tile_words of `frames`; stride default n_listed *
    tile_words) of the n_frames frames folded in order into block tiles[k] (int32) of the running `mean` and `m2`
    (n_state_tiles blocks, default what they hold), which hold n_prior frames already; `var` (optional) is written for
    the listed blocks.  Every other block is untouched; an entry >= n_state_tiles is skipped."""
    import torch
    for t in (frames, mean, m2, var):
        if t is not None:
            _check_tensor(t, torch.float64, 0, device=mean.device)
    if tiles is not None:
        _check_tensor(tiles, torch.int32, n_listed, device=mean.device)
    small = min(t.numel() for t in (mean, m2, var) if t is not None)
    stride, n_state_tiles = _tiles_shape(n_frames, n_listed, tile_words, stride, n_state_tiles, small, frames.numel())
    with torch.cuda.device(mean.device):
        F.check(F.rp().rp_accum_frames_tiles_device(
            tile_words, n_state_tiles, tiles.data_ptr() if tiles is not None else None, n_listed, n_prior, n_frames,
            frames.data_ptr(), stride, mean.data_ptr(), m2.data_ptr(), var.data_ptr() if var is not None else None,
            _stream_ptr(stream, mean.device)))


def accum_frames_tiles_host(frames, n_frames: int, tiles, n_listed: int, tile_words: int, mean, m2, n_prior: int = 0,
                            var=None, stride=None, n_state_tiles=None) -> None:
    """rph_accum_frames_tiles: the same fold on the CPU (librp_host.so; equal bits), in place on contiguous numpy f64
    arrays; tiles: uint32 (or anything np.ascontiguousarray converts)."""
    for a in (frames, mean, m2, var):
        if a is not None:
            assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous
    for a in (mean, m2, var):
        assert a is None or a.flags.writeable
    tiles = np.ascontiguousarray(tiles if tiles is not None else [], dtype=np.uint32)
    assert tiles.size >= n_listed
    small = min(a.size for a in (mean, m2, var) if a is not None)
    stride, n_state_tiles = _tiles_shape(n_frames, n_listed, tile_words, stride, n_state_tiles, small, frames.size)
    F.check_host(F.host().rph_accum_frames_tiles(
        tile_words, n_state_tiles, tiles.ctypes.data if tiles.size else None, n_listed, n_prior, n_frames,
        frames.ctypes.data, stride, mean.ctypes.data, m2.ctypes.data, var.ctypes.data if var is not None else None))


# ---- temporal reprojection (rp_reproject*, rp_accum_frames_counts_device, include/rp.h) ----
def reproject_params(params=None, **kw) -> F.rp_reproject_params:
    """rp_reproject_params: `params` (an rp_reproject_params, a dict of its fields or None) with fields overridden by
    keyword.  Fields left at zero take the library's defaults (sigma_depth 0.05, normal_cos 0.9, max_history 32)."""
    p = F.rp_reproject_params()
    if isinstance(params, F.rp_reproject_params):
        ctypes.memmove(ctypes.byref(p), ctypes.byref(params), ctypes.sizeof(p))
    elif params:
        kw = {**params, **kw}
    for k, v in kw.items():
        if not hasattr(p, k):
            raise KeyError(f"unknown reproject parameter {k!r}")
        setattr(p, k, v)
    return p


def _camera_c(camera) -> F.rp_camera:
    return camera if isinstance(camera, F.rp_camera) else camera.to_c()


def reproject_prev_camera(camera) -> F.rp_camera:
    """`camera` (Camera or rp_camera) as the `prev` argument of the reprojection calls: the same camera with its
    orientation replaced by the inverse transpose, columns (c1 x c2, c2 x c0, c0 x c1) / det.  The pass takes the
    transpose of prev's orientation for its inverse, which holds for orthonormal columns only, and
    Transformation.lookat's x and y columns are shorter than 1 whenever the camera looks up or down (x = up x z is not
    normalised); the transpose of what this returns IS the inverse, so the reprojection is exact for any camera.  An
    orthonormal orientation comes back unchanged up to rounding."""
    c = _camera_c(camera)
    o = list(c.orientation)
    col = [o[0:3], o[3:6], o[6:9]]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    dual = [cross(col[1], col[2]), cross(col[2], col[0]), cross(col[0], col[1])]
    det = (col[0][0] * dual[0][0] + col[0][1] * dual[0][1]) + col[0][2] * dual[0][2]
    if not det != 0.0:
        raise ValueError("the camera's orientation is singular")
    out = F.rp_camera()
    ctypes.memmove(ctypes.byref(out), ctypes.byref(c), ctypes.sizeof(out))
    out.orientation[:] = [x / det for v in dual for x in v]
    return out


def reproject_stats(stats) -> dict:
    """The RP_REPROJECT_STATS_LEN words of a reprojection: pixels, those that kept history (count >= 1), the sum of the
    counts and the pixels that fell off the previous frame."""
    w = [int(x) for x in np.asarray(stats).reshape(-1)[:F.RP_REPROJECT_STATS_LEN]]
    return {"pixels": w[0], "kept": w[1], "count_sum": w[2], "off": w[3]}


def reproject_device(cur, prev, depth, normal, depth_prev, normal_prev, mean_prev, m2_prev, count_prev, mean, m2, count,
                     stats, params=None, stream=None) -> None:
    """rp_reproject_device on torch tensors of one device, asynchronously on `stream` (torch stream; default: current):
    the state of the previous pose (mean_prev, m2_prev (h, w, 3) f64, count_prev (h, w) int32, frame order) carried to
    the current pose's pixels into mean, m2, count, guided by both poses' depth (h, w) and normal (h, w, 3) from
    render_aov; cur, prev: Camera or rp_camera -- prev as reproject_prev_camera gives it unless its orientation is
    orthonormal.  stats: int64, RP_REPROJECT_STATS_LEN (reproject_stats decodes them).
    The frame's size is `count`'s shape; no output may alias an input.  params: as reproject_params takes them."""
    import torch
    assert count.dtype == torch.int32 and count.is_cuda and count.is_contiguous() and count.dim() == 2
    h, w = count.shape
    dev = count.device
    for t, dt, m in ((depth, torch.float64, w * h), (normal, torch.float64, 3 * w * h), (depth_prev, torch.float64, w * h),
                     (normal_prev, torch.float64, 3 * w * h), (mean_prev, torch.float64, 3 * w * h),
                     (m2_prev, torch.float64, 3 * w * h), (count_prev, torch.int32, w * h), (mean, torch.float64, 3 * w * h),
                     (m2, torch.float64, 3 * w * h), (stats, torch.int64, F.RP_REPROJECT_STATS_LEN)):
        _check_tensor(t, dt, m, device=dev)
        assert t.numel() == m
    p, cc, cp = reproject_params(params), _camera_c(cur), _camera_c(prev)
    with torch.cuda.device(dev):
        F.check(F.rp().rp_reproject_device(ctypes.byref(p), w, h, ctypes.byref(cc), ctypes.byref(cp), depth.data_ptr(),
                                           normal.data_ptr(), depth_prev.data_ptr(), normal_prev.data_ptr(),
                                           mean_prev.data_ptr(), m2_prev.data_ptr(), count_prev.data_ptr(),
                                           mean.data_ptr(), m2.data_ptr(), count.data_ptr(), stats.data_ptr(),
                                           _stream_ptr(stream, dev)))


def _reproject_host_frames(depth, normal, depth_prev, normal_prev, mean_prev, m2_prev, count_prev):
    depth = np.ascontiguousarray(depth, dtype=np.float64)
    assert depth.ndim == 2, "depth: (h, w)"
    h, w = depth.shape
    f3 = [np.ascontiguousarray(a, dtype=np.float64) for a in (normal, normal_prev, mean_prev, m2_prev)]
    depth_prev = np.ascontiguousarray(depth_prev, dtype=np.float64)
    count_prev = np.ascontiguousarray(count_prev, dtype=np.uint32)
    assert all(a.shape == (h, w, 3) for a in f3) and depth_prev.shape == (h, w) and count_prev.shape == (h, w)
    out = (np.empty((h, w, 3)), np.empty((h, w, 3)), np.empty((h, w), dtype=np.uint32),
           np.zeros(F.RP_REPROJECT_STATS_LEN, dtype=np.uint64))
    ptrs = [a.ctypes.data for a in (depth, f3[0], depth_prev, f3[1], f3[2], f3[3], count_prev) + out]
    return w, h, ptrs, out


def reproject_host(cur, prev, depth, normal, depth_prev, normal_prev, mean_prev, m2_prev, count_prev, params=None) -> tuple:
    """rph_reproject: the same pass on the CPU (librp_host.so; the same arithmetic header as the kernel, equal bits) on
    numpy frames: (mean (h, w, 3), m2 (h, w, 3), count (h, w) uint32, stats uint64[RP_REPROJECT_STATS_LEN])."""
    w, h, ptrs, out = _reproject_host_frames(depth, normal, depth_prev, normal_prev, mean_prev, m2_prev, count_prev)
    p, cc, cp = reproject_params(params), _camera_c(cur), _camera_c(prev)
    F.check_host(F.host().rph_reproject(ctypes.byref(p), w, h, ctypes.byref(cc), ctypes.byref(cp), *ptrs))
    return out


def reproject(cur, prev, depth, normal, depth_prev, normal_prev, mean_prev, m2_prev, count_prev, params=None,
              device: int = 0) -> tuple:
    """rp_reproject: reproject_host's arguments and results through the device kernel, and the device seconds."""
    w, h, ptrs, out = _reproject_host_frames(depth, normal, depth_prev, normal_prev, mean_prev, m2_prev, count_prev)
    p, cc, cp = reproject_params(params), _camera_c(cur), _camera_c(prev)
    sec = ctypes.c_double()
    F.check(F.rp().rp_reproject(ctypes.byref(p), device, w, h, ctypes.byref(cc), ctypes.byref(cp), *ptrs,
                                ctypes.byref(sec)))
    return out + (sec.value,)


def _counts_shape(n_frames: int, n_pixels, wpp: int, stride, count_len: int, state_len: int, frames_len: int):
    n_pixels = count_len if n_pixels is None else int(n_pixels)
    stride = n_pixels * wpp if stride is None else int(stride)
    # what the library would read and write must lie inside the buffers; its own refusals stay the library's
    assert n_pixels <= count_len and n_pixels * wpp <= state_len, "count, mean, m2 and var: too short for n_pixels"
    if n_frames >= 1 and stride >= n_pixels * wpp:
        assert frames_len >= (n_frames - 1) * stride + n_pixels * wpp, "frames: (n_frames - 1) * stride + words"
    return n_pixels, stride


def accum_frames_counts_device(frames, n_frames: int, count, mean, m2, var=None, var_one: float = 1.0,
                               words_per_pixel: int = 3, n_pixels=None, stride=None, stream=None) -> None:
    """rp_accum_frames_counts_device on torch tensors of one device, asynchronously on `stream` (torch stream; default:
    current): accum_frames_device with the frame number taken per pixel -- pixel p, which holds count[p] (int32) frames
    already (0: its state is only written), folds its words_per_pixel words of the n_frames blocks of `frames` (block f
    at f * stride; default n_pixels * words_per_pixel) and count[p] grows by n_frames; `var` (optional) receives the
    variance of the mean, var_one where a pixel has one frame.  n_pixels default: count.numel()."""
    import torch
    for t in (frames, mean, m2, var):
        if t is not None:
            _check_tensor(t, torch.float64, 0, device=mean.device)
    _check_tensor(count, torch.int32, 0, device=mean.device)
    small = min(t.numel() for t in (mean, m2, var) if t is not None)
    n_pixels, stride = _counts_shape(n_frames, n_pixels, words_per_pixel, stride, count.numel(), small, frames.numel())
    with torch.cuda.device(mean.device):
        F.check(F.rp().rp_accum_frames_counts_device(n_pixels, words_per_pixel, n_frames, frames.data_ptr(), stride,
                                                     count.data_ptr(), mean.data_ptr(), m2.data_ptr(),
                                                     var.data_ptr() if var is not None else None, var_one,
                                                     _stream_ptr(stream, mean.device)))


def accum_frames_counts_host(frames, n_frames: int, count, mean, m2, var=None, var_one: float = 1.0,
                             words_per_pixel: int = 3, n_pixels=None, stride=None) -> None:
    """rph_accum_frames_counts: the same fold on the CPU (librp_host.so; equal bits), in place on contiguous numpy
    arrays (f64; count uint32)."""
    for a in (frames, mean, m2, var):
        if a is not None:
            assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous
    assert isinstance(count, np.ndarray) and count.dtype == np.uint32 and count.flags.c_contiguous
    for a in (count, mean, m2, var):
        assert a is None or a.flags.writeable
    small = min(a.size for a in (mean, m2, var) if a is not None)
    n_pixels, stride = _counts_shape(n_frames, n_pixels, words_per_pixel, stride, count.size, small, frames.size)
    F.check_host(F.host().rph_accum_frames_counts(n_pixels, words_per_pixel, n_frames, frames.ctypes.data, stride,
                                                  count.ctypes.data, mean.ctypes.data, m2.ctypes.data,
                                                  var.ctypes.data if var is not None else None, var_one))


def denoise_device(rgb, normal, albedo, depth, out, scratch=None, params=None, stream=None, variance=None) -> None:
    """rp_denoise_device on torch tensors of one device, asynchronously on `stream` (torch stream; default: current):
    rgb (h, w, 3) f64 and the optional guides normal, albedo (h, w, 3), depth (h, w) in frame order (flat tensors of
    the same sizes are taken with `out`'s shape), `out` (h, w, 3) f64, which must not alias an input.  scratch: a
    tensor of >= denoise_scratch_bytes(w, h) bytes (default: allocated here on `stream`).  variance (h, w, 3) f64:
    rp_denoise_var_device, the variance-guided filter (params as denoise_var_params takes them, scratch of
    denoise_var_scratch_bytes(w, h) bytes)."""
    import torch
    assert out.dtype == torch.float64 and out.is_cuda and out.is_contiguous() and out.dim() == 3 and out.shape[2] == 3
    h, w = out.shape[:2]
    for t, m in ((rgb, 3 * w * h), (normal, 3 * w * h), (albedo, 3 * w * h), (depth, w * h), (variance, 3 * w * h)):
        if t is not None:
            assert t.dtype == torch.float64 and t.device == out.device and t.is_contiguous() and t.numel() == m
    assert rgb is not None
    s = _stream(stream, out.device)
    need = denoise_scratch_bytes(w, h) if variance is None else denoise_var_scratch_bytes(w, h)
    if scratch is None:
        with torch.cuda.stream(s):
            scratch = torch.empty(need // 8, dtype=torch.float64, device=out.device)
    assert scratch.is_cuda and scratch.device == out.device and scratch.numel() * scratch.element_size() >= need
    gp = [t.data_ptr() if t is not None else None for t in (normal, albedo, depth)]
    with torch.cuda.device(out.device):
        if variance is None:
            p = denoise_params(params)
            F.check(F.rp().rp_denoise_device(ctypes.byref(p), w, h, rgb.data_ptr(), *gp, out.data_ptr(),
                                             scratch.data_ptr(), _stream_ptr(s)))
        else:
            p = denoise_var_params(params)
            F.check(F.rp().rp_denoise_var_device(ctypes.byref(p), w, h, rgb.data_ptr(), variance.data_ptr(), *gp,
                                                 out.data_ptr(), scratch.data_ptr(), _stream_ptr(s)))


def tga_bytes(width: int, height: int, bgra) -> bytes:
    """tga::save (image.rs:116-137): 18-byte header (uncompressed true colour, 32 bpp) + the frame's
    B, G, R, A bytes in row order, row 0 = bottom -- the file rph_tga_save writes."""
    hd = bytearray(18)
    hd[2] = 2
    hd[12:14] = int(width).to_bytes(2, "little")
    hd[14:16] = int(height).to_bytes(2, "little")
    hd[16] = 32
    body = np.ascontiguousarray(bgra, dtype=np.uint8).reshape(-1)
    assert body.size == 4 * width * height
    return bytes(hd) + body.tobytes()


def device_count() -> int:
    n = ctypes.c_int()
    rc = F.rp().rp_device_count(ctypes.byref(n))
    return n.value if rc == F.RP_OK else 0


def render(scene: Scene, params: RenderParams, device: int = 0, foreground: bool = False,
           options: dict | None = None):
    """One-shot: upload the scene, render the frame, return (rgb, fg, stats)."""
    with DeviceScene(scene, device, options) as ds:
        return ds.render(params, foreground=foreground)
