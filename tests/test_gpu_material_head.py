"""GPU: shading through the material record's packed head (rp_layout.h material_head_pack; rp_device.h shade_ray reads
a hit's kinds, needs_uv and texture ids from it with one load, at a 32-bit offset from the table's base).

One 64 x 48 frame at 4 spp against the oracle.  The scene packs, within a few pixels of each other and behind one
another's reflections, Lambert, Metal and Dielectric hits and misses, a material with an absorb map and a SkySphere
emit at once, a three-level Checker ending in an Image, a sphere with an Image map and a uv-mapped quad; the
materials used are the last ones of a table of 300 whose other entries are bright emitters of other kinds, so a head
read from the wrong record, or a field of it from the wrong bits, shows.  A second frame maps a sphere to texture
65,536 of a table of 65,537 Solid textures: its id does not fit the head's 16 bits and the kernel must take it from
the record's u32 field.

"Equal" is the parity tests' per-pixel exactness (parity.TOL_EXACT, with the same ray and sample counts): the kernel
adds each bounce's emission into the pixel sum as it goes and the oracle adds the sample's total, which differs in the
last ulp (rp_device.h shade_ray), so the frames are not the same bits with or without this change.
"""
import math

import numpy as np
import pytest

import shading_scenes as S
from parity import TOL_EXACT, compare
from rtpotato import _ffi as F
from rtpotato.scene import (Absorb, Camera, Emit, Hittable, Material, RenderParams, Scatter, Scene, SceneData, Texture,
                            Transformation, hittables, rgb)

pytestmark = pytest.mark.gpu

W, H, SPP, TILE = 64, 48, 4, 16
N_MATERIALS = 300


def _camera(pos, target) -> Camera:
    return Camera(float(W) / float(H), math.pi / 2.5, 1.0, 0.0, Transformation.lookat(pos, target, (0.0, 1.0, 0.0)))


def _fillers(n: int, n_textures: int):
    """Records nobody is mapped to: every kind, bright colours, texture ids in range."""
    out = []
    for i in range(n):
        scatter = [Scatter.None_, Scatter.Lambert, Scatter.Metal(0.5), Scatter.Dielectric(1.3)][i % 4]
        absorb = [Absorb.BlackBody, Absorb.WhiteBody, Absorb.Albedo(rgb(0.9, 0.1, 0.9)),
                  Absorb.AlbedoMap(i % n_textures)][(i // 4) % 4]
        emit = [Emit.Color(rgb(9.0, 7.0, 5.0)), Emit.DebugNormals, Emit.SkyGradient, Emit.SkySphere(i % n_textures),
                Emit.Color(rgb(3.0, 8.0, 1.0))][(i // 16) % 5]
        out.append(Material.new(scatter, absorb, emit))
    return out


def packed_scene() -> Scene:
    textures = [
        Texture.Image(S._image(6, 9, 11)),   # 0: the sphere's map
        Texture.Image(S._image(5, 4, 12)),   # 1: under the Checkers
        Texture.Solid(rgb(0.2, 0.7, 0.9)), Texture.DebugUVs, Texture.Noise(7),
        Texture.Checker(1, 2),               # 5: odd Image, even Solid
        Texture.Checker(5, 3),               # 6: odd -> 5, even DebugUVs
        Texture.Checker(6, 4),               # 7: odd -> 6 -> 5 -> Image: three levels; even Noise
        Texture.Image(S._image(3, 5, 13)),   # 8: the quad's map and an emitter's sky
    ]
    used = [
        Material.new(Scatter.Lambert, Absorb.AlbedoMap(7), Emit.None_),                     # ground: three-level Checker
        Material.new(Scatter.Lambert, Absorb.AlbedoMap(0), Emit.None_),                     # sphere with an Image map
        Material.new(Scatter.Metal(0.15), Absorb.Albedo(rgb(0.85, 0.8, 0.7)), Emit.None_),
        Material.new(Scatter.Dielectric(1.5), Absorb.WhiteBody, Emit.None_),
        Material.new(Scatter.Metal(0.3), Absorb.AlbedoMap(2), Emit.SkySphere(8)),           # absorb map and sky emit
        Material.new(Scatter.Lambert, Absorb.AlbedoMap(8), Emit.Color(rgb(0.05, 0.02, 0.1))),  # the quad
    ]
    materials = _fillers(N_MATERIALS - len(used), len(textures)) + used
    b = N_MATERIALS - len(used)
    quad = S._quad_mesh(b + 5)
    quad = type(quad)(quad.positions * 0.3 + np.array([0.0, -0.25, 0.1]), quad.normals, quad.uvs, quad.indices, b + 5)
    root = hittables(Hittable.Sphere((0.2, -25.3, -0.6), 25.0, b + 0),
                     Hittable.Sphere((-0.62, 0.12, -0.9), 0.4, b + 1), Hittable.Sphere((0.0, 0.05, -0.55), 0.33, b + 2),
                     Hittable.Sphere((0.58, 0.1, -0.85), 0.38, b + 3), Hittable.Sphere((0.05, 0.62, -1.0), 0.27, b + 4),
                     Hittable.Triangle(0, 0), Hittable.Triangle(3, 0))
    return Scene(_camera((0.05, 0.55, 1.15), (0.0, 0.2, -0.8)), SceneData(materials, textures, [quad]), root,
                 Emit.SkySphere(7), F.RP_ROOT_BVH, "packed_heads")


def wide_id_scene() -> Scene:
    textures = [Texture.Solid(rgb(0.5, 0.5, 0.5))] * 65536 + [Texture.Solid(rgb(0.9, 0.3, 0.1))]
    materials = [Material.new(Scatter.Lambert, Absorb.AlbedoMap(65535), Emit.None_),
                 Material.new(Scatter.Lambert, Absorb.AlbedoMap(65536), Emit.None_),
                 Material.new(Scatter.Metal(0.1), Absorb.AlbedoMap(3), Emit.SkySphere(65536))]
    root = hittables(Hittable.Sphere((0.0, -30.4, -1.0), 30.0, 0), Hittable.Sphere((-0.5, 0.1, -1.0), 0.45, 1),
                     Hittable.Sphere((0.55, 0.1, -0.9), 0.45, 2))
    return Scene(_camera((0.0, 0.5, 0.9), (0.0, 0.1, -1.0)), SceneData(materials, textures, []), root,
                 Emit.SkyGradient, F.RP_ROOT_BVH, "wide_ids")


def _check(gpu, sc: Scene, options, owns):
    p = RenderParams(W, H, SPP, 8, S.SEED, TILE, TILE)
    ref, ctr, mask = S.census(sc, p)
    pixels = S.event_pixels(mask)
    for e in owns:  # the oracle's census: the frame does hold what it was built for
        assert pixels.get(e, 0) >= 8, (e, pixels)
    rgb, _, st = gpu.render(sc, p, options=options)
    c = compare(rgb, ref)
    same_bits = int((rgb.view(np.uint64) == ref.view(np.uint64)).all(axis=-1).sum())
    err = np.where(np.isnan(rgb) & np.isnan(ref), 0.0, np.abs(rgb - ref)).max(axis=-1)
    print(sc.name, options, c, "pixels of equal bits", same_bits, "of", W * H, "rays", st["rays"], ctr["rays"])
    for j, i in np.argwhere(~(err <= TOL_EXACT))[:12]:
        print(f"  pixel ({i}, {j}): gpu {rgb[j, i]} oracle {ref[j, i]} events {S.pixel_events(mask[j, i])}")
    assert c["nan_mismatch"] == 0 and c["not_exact"] == 0, c
    assert (st["rays"], st["samples"], st["pixels"]) == (ctr["rays"], ctr["samples"], W * H), (st, ctr)


@pytest.mark.parametrize("fmt", ["f32", "q8"])  # the material from the traversal, and re-read from the primitive
def test_heads_at_the_end_of_a_long_table(gpu, oracle, fmt):
    _check(gpu, packed_scene(), {"builder": "host", "node_format": fmt},
           ["sc_lambert", "sc_metal", "sc_diel_refract", "sc_diel_reflect", "hit_two_tex", "tx_checker_in_checker",
            "tx_image_in_checker", "tx_on_sph", "tx_on_tri", "tx_on_miss", "tx_image", "ab_albedo_map", "ems_sky_sphere",
            "ems_color", "bg_sky_sphere"])


def test_texture_id_beyond_the_head(gpu, oracle):
    _check(gpu, wide_id_scene(), {"builder": "host", "node_format": "f32"}, ["tx_solid", "ab_albedo_map", "hit_two_tex"])
