"""GPU: a triangle hit's normals from the per-primitive table (rp_layout.h TriNormals; rp_device.h surface_at).

Shading reads the three vertex normals of a hit triangle as one 72 B record at the primitive's index -- five loads
that go out with the material head's -- instead of the PrimRef's ids and then three rows of a vertex table, which is no
longer on the device.  The table is uploaded from the host builder's copy, or filled by a gather kernel behind a
device build.  16 x 8 frames against the oracle within parity.py's bound, with ray, sample and pixel counters equal
(a wrong normal changes a path and its rays): the bunny with Lambert alone and with all its materials, on both 4-wide
node formats (the hit's material from the traversal, and re-read from the primitive); both device builders; the
feature pass's normal buffer, which shares surface_at; and the aimed mesh scene, whose quad and fan read an Image
through the triangle's uv -- the path that still takes the PrimRef and the vertex uvs, behind the normals.
"""
import numpy as np
import pytest

import aov_ref
import shading_scenes as S
from parity import assert_parity, compare, oracle_render

pytestmark = pytest.mark.gpu

W, H, SPP = 16, 8, 6
_refs = {}


def _scene(name):
    from rtpotato import scenes
    return scenes.configure(S.meshes() if name == "meshes" else scenes.CATALOGUE[name](), W, H)


def _params():
    from rtpotato import scenes
    from rtpotato.scene import RenderParams
    return RenderParams(W, H, SPP, 8, scenes.DEFAULT_SEED)


def _check(gpu, name, options):
    sc, p = _scene(name), _params()
    if name not in _refs:  # one oracle render per scene, shared by the formats and builders
        _refs[name] = oracle_render(sc, p, threads=8)
    ref, _, ctr = _refs[name]
    rgb, _, st = gpu.render(sc, p, options=options)
    c = compare(rgb, ref)
    print(name, options, c, st["rays"], ctr["rays"])
    assert_parity(c)
    assert st["rays"] == ctr["rays"] and st["samples"] == ctr["samples"] == W * H * SPP, (st, ctr)
    assert st["pixels"] == W * H


@pytest.mark.parametrize("fmt", ["f32", "q8"])
@pytest.mark.parametrize("name", ["bunny_lambert", "bunny_full"])
def test_host_built_table(gpu, name, fmt):
    _check(gpu, name, {"builder": "host", "node_format": fmt})


@pytest.mark.parametrize("builder,fmt", [("ploc", "q8"), ("gpu", "f32")])
def test_gathered_table(gpu, builder, fmt):
    """The device builders: the table is filled by the gather kernel from the finished tree's PrimRefs."""
    _check(gpu, "bunny_full", {"builder": builder, "node_format": fmt})


@pytest.mark.parametrize("builder", ["host", "ploc"])
def test_textured_mesh_reads_uv_behind_the_normals(gpu, builder):
    sc, p = _scene("meshes"), _params()
    _, _, mask = S.census(sc, p)
    assert S.event_pixels(mask).get("tx_on_tri", 0) >= 8  # the frame does sample textures on triangles
    _check(gpu, "meshes", {"builder": builder, "node_format": "f32"})


@pytest.mark.parametrize("options", [{"builder": "host"}, {"builder": "ploc"}])
def test_feature_pass_normals(gpu, options):
    """The first-hit normal buffer of bunny_lambert at the feature pass's own bound (tests/test_gpu_aov.py), and the
    frame does show interpolated bunny normals, not the ground's alone."""
    from rtpotato.scene import RenderParams
    sc = _scene("bunny_lambert")
    p = RenderParams(W, H, SPP, 8, aov_ref.SEED, 32, 32)
    if "aov" not in _refs:
        _refs["aov"] = aov_ref.normal_ref(sc, p)
    normal, fg = _refs["aov"]
    with gpu.DeviceScene(sc, options=options) as ds:
        out = ds.render_aov(p, albedo=False, depth=False)
    c = compare(out["normal"], normal)
    print(options, c)
    assert_parity(c)
    assert np.array_equal(out["fg"], fg)
    assert (np.abs(normal[..., 1]) < 0.9).sum() >= 8
