"""References of the first-hit feature pass (include/rp.h rp_render_aov), built from the CPU oracle alone.

(a) normal: the scene with every material replaced by (Scatter.None_, Absorb.BlackBody, Emit.DebugNormals) and an
    Emit.None_ background, rendered by the oracle at samples_per_stream = 1 -- each sample is then the first camera
    sample of its own stream, the path ends at the first hit, and its colour is hit.normal (zero on a miss): the
    colour frame is the normal buffer and the foreground the fg buffer.
(b) albedo: the same with Emit chosen from each material's Absorb: BlackBody -> None_, WhiteBody -> Color(1, 1, 1),
    Albedo(c) -> Color(c), AlbedoMap(t) -> SkySphere(t), which samples the texture at the hit record
    (material.rs:58) and draws no random number.
(c) depth (pinhole cameras): each sample's primary ray rebuilt in numpy from the first two draws of its stream,
    in Camera::shoot's operation order with a zero lens offset, and traced by the oracle's closest-hit query.
    tests/test_aov_ref.py checks (c) against (a) -- hit flags and normals bit for bit -- before (c) judges the GPU.
"""
from __future__ import annotations

import math
from dataclasses import replace

import numpy as np

from parity import oracle_render

SEED = 0xA0F1
# (scene, width, height): the frames the references were checked on; every one has pixels of partial coverage at 4 spp
FRAMES = {"variants": (64, 48), "earth": (64, 48), "variants_sky": (64, 48), "three_balls": (64, 48),
          "bunny_full": (96, 64)}
PINHOLE = ("variants", "earth", "variants_sky", "bunny_full")


def add_frame(name: str, scene, width: int, height: int) -> None:
    """Enter a scene object (not of the catalogue) into the frame table under `name`."""
    FRAMES[name] = (width, height, scene)


def _pinhole(name: str) -> bool:
    return name in PINHOLE or (len(FRAMES[name]) == 3 and FRAMES[name][2].camera.lens_radius == 0.0)


def scene_params(name: str, spp: int, **kw):
    from rtpotato import scenes
    from rtpotato.scene import RenderParams
    w, h = FRAMES[name][:2]
    sc = scenes.configure(FRAMES[name][2] if len(FRAMES[name]) == 3 else scenes.CATALOGUE[name](), w, h)
    return sc, RenderParams(w, h, spp, 8, SEED, 32, 32, **kw)


def _with_materials(scene, materials):
    from rtpotato.scene import Emit
    return replace(scene, scene_data=replace(scene.scene_data, material_table=list(materials)), background=Emit.None_)


def normals_scene(scene):
    from rtpotato.scene import Absorb, Emit, Material, Scatter
    m = Material.new(Scatter.None_, Absorb.BlackBody, Emit.DebugNormals)
    return _with_materials(scene, [m] * len(scene.scene_data.material_table))


def albedo_scene(scene):
    from rtpotato import _ffi as F
    from rtpotato.scene import Absorb, Emit, Material, Scatter

    def emit_of(a):
        if a.kind == F.RP_ABSORB_WHITE_BODY:
            return Emit.Color((1.0, 1.0, 1.0))
        if a.kind == F.RP_ABSORB_ALBEDO:
            return Emit.Color(a.color)
        if a.kind == F.RP_ABSORB_ALBEDO_MAP:
            return Emit.SkySphere(a.texture)
        return Emit.None_

    return _with_materials(scene, [Material.new(Scatter.None_, Absorb.BlackBody, emit_of(m.absorb))
                                   for m in scene.scene_data.material_table])


def _first_hit_render(scene, params):
    rgb, fg, _ = oracle_render(scene, replace(params, samples_per_stream=1), threads=8, foreground=True)
    return rgb, fg


def normal_ref(scene, params):
    """(a): (normal (h, w, 3) f64, fg (h, w) f32)."""
    return _first_hit_render(normals_scene(scene), params)


def albedo_ref(scene, params):
    """(b): (albedo (h, w, 3) f64, fg (h, w) f32)."""
    return _first_hit_render(albedo_scene(scene), params)


def primary_rays(scene, params, k: int) -> np.ndarray:
    """Sample k's camera rays of a pinhole frame, (h * w, 8) {origin, direction, t_min, t_max}: the uv jitter from
    the first two draws of stream seed + k W H + j W + i, then Camera::shoot (render.rs:32-52) with a zero lens
    offset, every product and sum in the reference's order."""
    from oracle import oracle_py as O
    cam = scene.camera
    assert cam.lens_radius == 0.0, "the depth reference is for pinhole cameras"
    W, H = params.width, params.height
    jit = np.empty((H, W, 2), dtype=np.uint64)
    for j in range(H):
        for i in range(W):
            jit[j, i] = O.stream_u64(params.seed + k * W * H + j * W + i, 2)
    r = (jit >> np.uint64(11)).astype(np.float64) * 2.0 ** -53  # rand 0.8 Standard f64
    ii, jj = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ju = (ii + r[..., 0]) / float(W)
    jv = (jj + r[..., 1]) / float(H)
    tanf = math.tan(0.5 * cam.fov)
    x = (2.0 * ju - 1.0) * tanf * cam.focal_dist * cam.aspect_ratio
    y = (2.0 * jv - 1.0) * tanf * cam.focal_dist
    z = np.full_like(x, -cam.focal_dist)
    n = np.sqrt((x * x + y * y) + z * z)
    x, y, z = x / n, y / n, z / n
    m = cam.transformation.orientation  # column-major
    d = np.stack([(x * m[0] + y * m[3]) + z * m[6], (x * m[1] + y * m[4]) + z * m[7],
                  (x * m[2] + y * m[5]) + z * m[8]], axis=-1)
    rays = np.empty((H * W, 8))
    rays[:, 0:3] = cam.transformation.position
    rays[:, 3:6] = d.reshape(-1, 3)
    rays[:, 6] = 1e-3
    rays[:, 7] = np.inf
    return rays


def depth_ref(scene, params):
    """(c): (depth (h, w) f64, fg (h, w) f32, normal (h, w, 3) f64) of the reconstructed rays: per pixel the hits' t
    (and normals) summed from 0.0 in sample order, / spp."""
    from oracle import oracle_py as O
    W, H = params.width, params.height
    d = scene.desc()
    osc = O.OracleScene(d.addr(), d)
    depth = np.zeros(H * W)
    nrm = np.zeros((H * W, 3))
    hits = np.zeros(H * W, dtype=np.int64)
    try:
        for k in range(params.spp):
            h, _, _ = osc.intersect(primary_rays(scene, params, k))
            hit = np.isfinite(h[:, 0])
            depth = depth + np.where(hit, h[:, 0], 0.0)
            nrm = nrm + np.where(hit[:, None], h[:, 4:7], 0.0)
            hits += hit
    finally:
        osc.close()
    spp = float(params.spp)
    fg = (hits.astype(np.float64) / spp).astype(np.float32)
    return (depth / spp).reshape(H, W), fg.reshape(H, W), (nrm / spp).reshape(H, W, 3)


_cache: dict = {}


def refs(name: str, spp: int) -> dict:
    """The references of frame `name` at `spp`, computed once per session and shared (read-only) by the tests:
    {"scene", "params", "normal", "albedo", "fg", and for pinhole frames "depth", "depth_fg", "depth_normal"}."""
    key = (name, spp)
    if key not in _cache:
        sc, p = scene_params(name, spp)
        normal, fg = normal_ref(sc, p)
        albedo, fg_b = albedo_ref(sc, p)
        assert np.array_equal(fg, fg_b)
        out = {"scene": sc, "params": p, "normal": normal, "albedo": albedo, "fg": fg}
        if _pinhole(name):
            out["depth"], out["depth_fg"], out["depth_normal"] = depth_ref(sc, p)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = out
    return _cache[key]
