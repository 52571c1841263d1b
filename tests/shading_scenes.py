"""Scenes aimed at the shading branches no catalogue scene reaches (test infrastructure, not the product's catalogue).

Each builder returns an rtpotato.scene.Scene made of small numpy meshes and images; no asset files.  No two surfaces
coincide, so a closest hit is never an exact-t tie.  OWNS names, per scene, the events of the oracle's shading census
(oracle_py.EVENT_NAMES) that the scene exists for: tests/test_shading_census.py holds every one of them to at least
FLOOR distinct pixels of the W x H x SPP frame the GPU parity tests render.
"""
from __future__ import annotations

import math
from dataclasses import replace

import numpy as np

from rtpotato import _ffi as F
from rtpotato.scene import (Absorb, Camera, Emit, Hittable, Material, Mesh, RenderParams, Scatter, Scene, SceneData,
                            Texture, Transformation, hittables, rgb)

W, H, SPP, TILE = 48, 32, 8, 16
SEED = 0x5AD1E5
FLOOR = 16  # distinct pixels on which an owned event must appear


def _image(h: int, w: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 4), dtype=np.uint8)


def _cam(fov, focal, lens, pos, target, up=(0.0, 1.0, 0.0)) -> Camera:
    return Camera(float(W) / float(H), fov, focal, lens, Transformation.lookat(pos, target, up))


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def _interleave(meshes) -> np.ndarray:
    """Root rows of every triangle of every mesh, round-robin over the meshes."""
    ids = [list(m.iter_triangles()) for m in meshes]
    rows = []
    for k in range(max(len(i) for i in ids)):
        for mi, i in enumerate(ids):
            if k < len(i):
                rows.append(Hittable.Triangle(int(i[k]), mi))
    return hittables(*rows)


def _quad_mesh(material: int) -> Mesh:
    """Ground quad of 4 shared vertices; uv runs from -0.25 to 1.25, so an Image on it takes all four clamps."""
    pos = np.array([[-2.6, 0.0, -2.2], [2.6, 0.0, -2.2], [2.6, 0.0, 2.4], [-2.6, 0.0, 2.4]])
    uv = np.array([[-0.25, 1.25], [1.25, 1.25], [1.25, -0.25], [-0.25, -0.25]])
    return Mesh(pos, np.array([[0.0, 1.0, 0.0]] * 4), uv, np.array([0, 1, 2, 0, 2, 3], dtype=np.uint32), material)


def _prism_mesh(material: int) -> Mesh:
    """Closed triangular prism, flat normals (every face has its own vertices, shared by the face's triangles)."""
    base = np.array([[-1.9, -0.3], [-0.5, 0.1], [-1.3, 1.0]])  # (x, z) of a scalene cross-section
    y0, y1 = 0.07, 1.35
    centre = np.array([base[:, 0].mean(), 0.5 * (y0 + y1), base[:, 1].mean()])
    pos, nrm, uv, idx = [], [], [], []

    def face(pts):
        pts = np.array(pts)
        n = _unit(np.cross(pts[1] - pts[0], pts[2] - pts[0]))
        if np.dot(n, pts.mean(axis=0) - centre) < 0.0:
            pts, n = pts[::-1], -n
        b = len(pos)
        for k, p in enumerate(pts):
            pos.append(p)
            nrm.append(n)
            uv.append([0.13 * (b + k) % 1.0, 0.29 * (b + 2 * k) % 1.0])
        for k in range(1, len(pts) - 1):
            idx.extend([b, b + k, b + k + 1])

    lo = [[x, y0, z] for x, z in base]
    hi = [[x, y1, z] for x, z in base]
    face(lo)
    face(hi)
    for a in range(3):
        b = (a + 1) % 3
        face([lo[a], lo[b], hi[b], hi[a]])
    return Mesh(np.array(pos), np.array(nrm), np.array(uv), np.array(idx, dtype=np.uint32), material)


def _fan_mesh(material: int) -> Mesh:
    """Five smooth-shaded triangles around a shared hub; the vertex normals lean apart, so the interpolated normal
    turns across each triangle."""
    hub = [1.3, 0.75, 0.2]
    rim = [[0.55, 0.15, 0.5], [2.05, 0.12, 0.1], [2.3, 1.0, -0.2], [1.45, 1.6, -0.1], [0.5, 1.15, 0.3]]
    pos = np.array([hub] + rim)
    nrm = _unit([[0.1, 0.1, 1.0], [-0.7, -0.5, 0.6], [0.6, -0.6, 0.7], [0.8, 0.3, 0.5], [0.1, 0.8, 0.5],
                 [-0.8, 0.4, 0.6]])
    uv = np.array([[0.5, 0.5], [0.05, 0.1], [0.95, 0.05], [1.1, 0.7], [0.6, 1.05], [-0.1, 0.8]])
    idx = []
    for k in range(5):
        idx.extend([0, 1 + k, 1 + (k + 1) % 5])
    return Mesh(pos, nrm, uv, np.array(idx, dtype=np.uint32), material)


def meshes() -> Scene:
    """Three meshes of 4, 18 and 6 vertices, their triangles interleaved in root order."""
    textures = [Texture.Image(_image(5, 7, 1)), Texture.Image(_image(4, 6, 2)), Texture.Image(_image(3, 5, 3))]
    materials = [
        Material.new(Scatter.Dielectric(1.5), Absorb.Albedo(rgb(0.9, 0.95, 0.9)), Emit.None_),  # prism (mesh 1)
        Material.new(Scatter.Metal(0.2), Absorb.AlbedoMap(1), Emit.SkySphere(2)),                # fan (mesh 2)
        Material.new(Scatter.Lambert, Absorb.AlbedoMap(0), Emit.None_),                          # quad (mesh 0)
    ]
    table = [_quad_mesh(2), _prism_mesh(0), _fan_mesh(1)]
    cam = _cam(math.pi / 3.0, 1.0, 0.0, (0.1, 1.7, 4.2), (0.05, 0.55, 0.0))
    return Scene(cam, SceneData(materials, textures, table), _interleave(table), Emit.SkyGradient, F.RP_ROOT_BVH,
                 "meshes")


def checkers() -> Scene:
    """Checkers of Checkers over an Image and DebugUVs on spheres whose centres straddle negative coordinates; the
    background walks a Checker at p = d.  A nested Checker decides on the same point as its parent, so the outer odd
    cell always reaches the inner odd texture and the outer even cell the inner even one."""
    textures = [
        Texture.Image(_image(4, 6, 4)), Texture.Solid(rgb(0.9, 0.2, 0.1)), Texture.DebugUVs, Texture.Noise(5),
        Texture.Checker(0, 1),   # 4: odd Image, even Solid
        Texture.Checker(3, 2),   # 5: odd Noise, even DebugUVs
        Texture.Checker(4, 5),   # 6: odd -> 4 -> Image, even -> 5 -> DebugUVs
        Texture.Perlin(3), Texture.Image(_image(3, 1, 5)),
        Texture.Checker(7, 8),   # 9: odd Perlin, even Image
    ]
    materials = [Material.new(Scatter.Lambert, Absorb.AlbedoMap(6), Emit.None_),
                 Material.new(Scatter.Lambert, Absorb.AlbedoMap(4), Emit.None_),
                 Material.new(Scatter.Metal(0.1), Absorb.AlbedoMap(5), Emit.None_)]
    root = hittables(Hittable.Sphere((0.3, -20.4, -0.7), 20.0, 0), Hittable.Sphere((-0.9, 0.35, -0.6), 0.75, 1),
                     Hittable.Sphere((0.95, 0.3, -0.2), 0.7, 2))
    cam = _cam(math.pi / 2.0, 1.0, 0.0, (0.15, 1.3, 2.4), (0.0, 0.1, -0.6))
    return Scene(cam, SceneData(materials, textures, []), root, Emit.SkySphere(9), F.RP_ROOT_BVH, "checkers")


def sky_offset() -> Scene:
    """The background image is the third texture, behind another image: its texel offset is not zero."""
    textures = [Texture.Image(_image(5, 7, 6)), Texture.Solid(rgb(0.6, 0.7, 0.5)), Texture.Image(_image(4, 6, 7))]
    materials = [
        Material.new(Scatter.Lambert, Absorb.AlbedoMap(0), Emit.None_),
        Material.new(Scatter.Metal(0.0), Absorb.Albedo(rgb(0.9, 0.8, 0.7)), Emit.None_),
        Material.new(Scatter.Metal(1.0), Absorb.AlbedoMap(1), Emit.None_),
        Material.new(Scatter.Dielectric(0.67), Absorb.WhiteBody, Emit.None_),
        Material.new(Scatter.Dielectric(1.0), Absorb.Albedo(rgb(0.8, 0.9, 1.0)), Emit.None_),
    ]
    root = hittables(Hittable.Sphere((0.0, -30.5, -1.0), 30.0, 0), Hittable.Sphere((-1.65, 0.05, -0.9), 0.55, 1),
                     Hittable.Sphere((-0.55, 0.0, -1.0), 0.5, 2), Hittable.Sphere((0.55, 0.02, -0.8), 0.52, 3),
                     Hittable.Sphere((1.65, 0.0, -1.1), 0.5, 4))
    cam = _cam(math.pi / 2.0, 1.0, 0.0, (0.0, 0.7, 1.6), (0.0, 0.0, -1.0))
    return Scene(cam, SceneData(materials, textures, []), root, Emit.SkySphere(2), F.RP_ROOT_BVH, "sky_offset")


EMITTER_BACKGROUNDS = {"color": Emit.Color(rgb(0.3, 0.5, 0.9)), "debug_normals": Emit.DebugNormals,
                       "sky_solid": Emit.SkySphere(0), "sky_noise": Emit.SkySphere(1)}


def emitters(background: str = "color") -> Scene:
    """Emitting surfaces that also scatter, under each background the catalogue does not have."""
    textures = [Texture.Solid(rgb(0.7, 0.6, 0.9)), Texture.Noise(-9)]
    materials = [
        Material.new(Scatter.Lambert, Absorb.Albedo(rgb(0.5, 0.5, 0.5)), Emit.None_),
        Material.new(Scatter.Lambert, Absorb.Albedo(rgb(0.6, 0.3, 0.2)), Emit.SkyGradient),
        Material.new(Scatter.Metal(0.05), Absorb.Albedo(rgb(0.8, 0.8, 0.3)), Emit.DebugNormals),
        Material.new(Scatter.Dielectric(1.5), Absorb.WhiteBody, Emit.Color(rgb(0.05, 0.1, 0.02))),
    ]
    root = hittables(Hittable.Sphere((0.0, -40.5, -1.0), 40.0, 0), Hittable.Sphere((-1.15, 0.05, -1.0), 0.55, 1),
                     Hittable.Sphere((0.0, 0.0, -1.2), 0.5, 2), Hittable.Sphere((1.1, 0.03, -0.9), 0.53, 3))
    cam = _cam(math.pi / 2.0, 1.0, 0.0, (0.0, 0.6, 1.3), (0.0, 0.0, -1.0))
    return Scene(cam, SceneData(materials, textures, []), root, EMITTER_BACKGROUNDS[background], F.RP_ROOT_BVH,
                 "emitters_" + background)


def inside() -> Scene:
    """The camera is inside a Lambert sphere and inside a Metal one (each the nearer wall on one side), so primary
    hits are back faces; a thin lens; two bounces, so paths off the small spheres run out of depth."""
    materials = [
        Material.new(Scatter.Lambert, Absorb.Albedo(rgb(0.7, 0.7, 0.7)), Emit.Color(rgb(0.9, 0.8, 0.6))),
        Material.new(Scatter.Metal(0.3), Absorb.Albedo(rgb(0.8, 0.8, 0.8)), Emit.Color(rgb(0.2, 0.3, 0.5))),
        Material.new(Scatter.Lambert, Absorb.Albedo(rgb(0.3, 0.6, 0.4)), Emit.None_),
        Material.new(Scatter.Metal(0.6), Absorb.Albedo(rgb(0.9, 0.6, 0.5)), Emit.None_),
        Material.new(Scatter.Dielectric(1.5), Absorb.WhiteBody, Emit.None_),
    ]
    root = hittables(Hittable.Sphere((0.0, 0.0, 0.0), 5.0, 0), Hittable.Sphere((6.0, 0.0, 0.0), 6.5, 1),
                     Hittable.Sphere((1.0, -0.45, -1.6), 0.4, 2), Hittable.Sphere((0.2, 0.1, -1.4), 0.35, 3),
                     Hittable.Sphere((1.7, 0.3, -1.5), 0.38, 4))
    cam = _cam(math.pi / 1.8, 1.5, 0.05, (1.0, 0.0, 0.0), (1.0, 0.0, -1.0))
    return Scene(cam, SceneData(materials, [], []), root, Emit.None_, F.RP_ROOT_BVH, "inside")


SCENES = {"meshes": meshes, "checkers": checkers, "sky_offset": sky_offset, "inside": inside}
SCENES.update({"emitters_" + b: (lambda b=b: emitters(b)) for b in EMITTER_BACKGROUNDS})
MAX_BOUNCE = {"inside": 2}

# scene -> the census events it exists for
OWNS = {
    "meshes": ["hit_tri", "hit_tri_mesh1", "tx_on_tri", "tx_clamp_x_lo", "tx_clamp_x_hi", "tx_clamp_y_lo",
               "tx_clamp_y_hi", "hit_two_tex", "hit_two_img", "ems_sky_sphere", "em_sky_sphere", "sc_diel_inside",
               "sc_diel_tir", "sc_diel_refract", "sc_diel_reflect", "sc_metal", "sc_lambert", "ab_albedo_map",
               "tx_image"],
    "checkers": ["tx_checker_in_checker", "tx_image_in_checker", "tx_checker_even", "tx_checker_odd", "tx_perlin",
                 "tx_debug_uvs", "tx_noise", "tx_solid", "tx_on_miss", "tx_on_sph", "bg_sky_sphere"],
    "sky_offset": ["bg_sky_sphere", "tx_on_miss", "tx_image", "sc_metal", "sc_metal_below", "sc_diel_tir",
                   "sc_diel_inside", "sc_diel_refract", "sc_diel_reflect", "ab_white_body"],
    "emitters_color": ["bg_color", "ems_sky_gradient", "ems_debug_normals", "ems_color", "em_sky_gradient",
                       "em_debug_normals", "em_color"],
    "emitters_debug_normals": ["bg_debug_normals"],
    "emitters_sky_solid": ["bg_sky_sphere", "tx_solid", "tx_on_miss"],
    "emitters_sky_noise": ["bg_sky_sphere", "tx_noise", "tx_on_miss"],
    "inside": ["sc_lambert_back", "sc_metal_back", "depth_out", "hit_sph"],
}


def scene(name: str) -> Scene:
    return SCENES[name]()


def params(name: str, **kw) -> RenderParams:
    return RenderParams(W, H, SPP, MAX_BOUNCE.get(name, 8), SEED, TILE, TILE, **kw)


# ---- table permutations (the table-order tests) and deliberately wrong scenes (the sensitivity check) ----------

def permuted(sc: Scene, tex=None, mat=None, mesh=None) -> Scene:
    """The same scene with its texture / material / mesh table reordered and every reference renumbered.  Each
    argument lists, per new index, the old index it holds (None: unchanged)."""
    sd = sc.scene_data
    nt, nm, nh = len(sd.texture_table), len(sd.material_table), len(sd.mesh_table)
    tex = list(range(nt)) if tex is None else list(tex)
    mat = list(range(nm)) if mat is None else list(mat)
    mesh = list(range(nh)) if mesh is None else list(mesh)
    assert sorted(tex) == list(range(nt)) and sorted(mat) == list(range(nm)) and sorted(mesh) == list(range(nh))
    tnew = {old: new for new, old in enumerate(tex)}
    mnew = {old: new for new, old in enumerate(mat)}
    hnew = {old: new for new, old in enumerate(mesh)}

    def retex(t):
        return replace(t, odd=tnew[t.odd], even=tnew[t.even]) if t.kind == F.RP_TEXTURE_CHECKER else t

    def reemit(e):
        return replace(e, texture=tnew[e.texture]) if e.kind == F.RP_EMIT_SKY_SPHERE else e

    def remat(m):
        a = m.absorb
        if a.kind == F.RP_ABSORB_ALBEDO_MAP:
            a = replace(a, texture=tnew[a.texture])
        return Material.new(m.scatter, a, reemit(m.emit))

    textures = [retex(sd.texture_table[o]) for o in tex]
    materials = [remat(sd.material_table[o]) for o in mat]
    table = [replace(sd.mesh_table[o], material=mnew[sd.mesh_table[o].material]) for o in mesh]
    root = sc.root.copy()
    tri = root["kind"] == F.RP_HITTABLE_TRIANGLE
    root["mesh"][tri] = [hnew[int(m)] for m in root["mesh"][tri]]
    root["material"][~tri] = [mnew[int(m)] for m in root["material"][~tri]]
    return replace(sc, scene_data=SceneData(materials, textures, table), root=root, background=reemit(sc.background))


PERMUTATIONS = {
    # per new index the old one; sky_offset's background image is texture 2: to index 0, and to index 1
    "meshes": [{"tex": [2, 0, 1]}, {"mat": [1, 2, 0]}, {"mesh": [2, 0, 1]},
               {"tex": [1, 2, 0], "mat": [2, 0, 1], "mesh": [1, 2, 0]}],
    "sky_offset": [{"tex": [2, 1, 0]}, {"tex": [1, 2, 0]}, {"mat": [4, 3, 2, 1, 0]},
                   {"tex": [2, 0, 1], "mat": [1, 0, 3, 4, 2]}],
}


def wrong_scenes() -> dict:
    """name -> (aimed scene name, a scene with one mistake of the kind the aimed scene exists to catch)."""
    out = {}
    s = sky_offset()  # the sky read at texel offset 0: background moved to texture 0 without renumbering
    out["sky_at_texture_0"] = ("sky_offset", replace(s, background=Emit.SkySphere(0)))
    m = meshes()      # vertex base of mesh 2 wrong: its normals and uvs read at mesh 1's base in the packed arrays
    sd = m.scene_data
    n2 = len(sd.mesh_table[2].positions)
    fan = replace(sd.mesh_table[2], normals=sd.mesh_table[1].normals[:n2].copy(), uvs=sd.mesh_table[1].uvs[:n2].copy())
    out["mesh2_vertex_base"] = ("meshes", replace(m, scene_data=replace(sd, mesh_table=sd.mesh_table[:2] + [fan])))
    c = checkers()    # uv not delivered through the Checkers: the hit's uv reads 0, as an Image at uv = (0, 0) and DebugUVs at 0
    tx = list(c.scene_data.texture_table)
    img = tx[0].image
    tx[0] = Texture.Solid(tuple(float(v) / 255.0 for v in img[0, 0, :3]))
    tx[2] = Texture.Solid(rgb(0.0, 0.0, 0.0))
    out["checker_uv_zero"] = ("checkers", replace(c, scene_data=replace(c.scene_data, texture_table=tx)))
    return out


# ---- rays for the closest-hit tests on `meshes` ------------------------------------------------------------

def mesh_rays():
    """Rays at the `meshes` scene: its camera's pixel centres and random rays among the meshes, read-only."""
    sc = meshes()
    cam = sc.camera
    rng = np.random.default_rng(0x3E5)
    n = 1500
    o = rng.uniform(-3.0, 3.0, size=(n, 3))
    o[:, 1] = rng.uniform(0.02, 2.5, size=n)
    d = rng.uniform(-2.4, 2.4, size=(n, 3)) * np.array([1.0, 0.0, 0.8]) + np.array([0.0, 1.0, 0.0]) * rng.uniform(
        -0.2, 1.5, size=(n, 1)) - o
    m = np.array(cam.transformation.orientation).reshape(3, 3)  # columns
    ii, jj = np.meshgrid((np.arange(40) + 0.5) / 40.0, (np.arange(25) + 0.5) / 25.0)
    t = np.tan(0.5 * cam.fov)
    loc = np.stack([(2.0 * ii - 1.0) * t * cam.aspect_ratio, (2.0 * jj - 1.0) * t, -np.ones_like(ii)], axis=-1)
    dc = loc.reshape(-1, 3) @ m
    oc = np.broadcast_to(np.array(cam.transformation.position), dc.shape)
    o, d = np.concatenate([o, oc]), np.concatenate([d, dc])
    rays = np.ascontiguousarray(np.concatenate([o, d, np.full((len(o), 1), 1e-3), np.full((len(o), 1), np.inf)],
                                               axis=1))
    rays.setflags(write=False)
    return sc, rays


# ---- the census itself -----------------------------------------------------------------------------------------

CATALOGUE_FRAMES = ["three_balls", "more_balls", "more_balls_optimized", "two_balls", "earth", "one_triangle",
                    "glass_bunny", "bunny", "bunny_lambert", "bunny_full", "variants", "variants_sky"]
CATALOGUE_SIZE = (64, 36, 4)  # tests/test_gpu_parity.py test_catalogue_scenes


def catalogue(name: str):
    """(scene, params) of a catalogue scene as test_catalogue_scenes renders it."""
    from rtpotato import scenes
    w, h, spp = CATALOGUE_SIZE
    return scenes.configure(scenes.CATALOGUE[name](), w, h), RenderParams(w, h, spp, 8, scenes.DEFAULT_SEED)


def census(sc: Scene, p: RenderParams, threads: int = 8):
    """The oracle's frame with its shading census: (rgb, counters by name, per-pixel event mask)."""
    import ctypes
    from oracle import oracle_py as O
    d = sc.desc()
    osc = O.OracleScene(d.addr(), d)
    cam, pc = sc.camera.to_c(), p.to_c()
    try:
        return osc.render_events(ctypes.addressof(cam), ctypes.addressof(pc), p.width, p.height, threads)
    finally:
        osc.close()


def event_pixels(mask: np.ndarray) -> dict:
    """event name -> number of pixels whose samples produced it."""
    from oracle import oracle_py as O
    return {e: int(((mask >> np.uint64(k)) & np.uint64(1)).sum()) for k, e in enumerate(O.EVENT_NAMES)}


def pixel_events(mask_value) -> list:
    """The names of the events in one pixel's mask (what a parity failure prints)."""
    from oracle import oracle_py as O
    return [e for k, e in enumerate(O.EVENT_NAMES) if (int(mask_value) >> k) & 1]


# ---- the feature pass's frames (tests/aov_ref.py) ----------------------------------------------------------------

AOV_FRAMES = {"aimed_meshes": "meshes", "aimed_checkers": "checkers", "aimed_sky_offset": "sky_offset"}


def add_aov_frames() -> None:
    """Enter the aimed scenes the feature pass is checked on into aov_ref's frame table (W x H, pinhole cameras)."""
    import aov_ref
    for frame, name in AOV_FRAMES.items():
        if frame not in aov_ref.FRAMES:
            aov_ref.add_frame(frame, scene(name), W, H)
