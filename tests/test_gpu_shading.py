"""GPU: the render kernel's shading on the aimed scenes of tests/shading_scenes.py -- several meshes, an Image on a
triangle with uv outside [0, 1], Checkers over Checkers over an Image, a background image that is not texture 0, two
Images in one hit, every background and surface Emit, Dielectric below and at index 1, Metal at fuzziness 1, back faces
on primary hits, paths that run out of depth.  tests/test_shading_census.py holds each scene's oracle frame to at
least 16 pixels of every branch the scene owns; here the device's 48 x 32 x 8 spp frame (16 x 16 tiles) equals that
oracle frame on every pixel to parity.TOL_EXACT, with the same ray, sample and pixel counts.  The scenes have no
coincident surfaces, so there is no exact-t tie to excuse.  Besides: rp_intersect on three meshes against brute force,
the feature pass against aov_ref's references, and the order of the texture, material and mesh tables (renumbering
them must not change a bit of the frame).
"""
import numpy as np
import pytest

import aov_ref
import shading_scenes as S
from brute import Brute
from parity import TOL_EXACT, assert_parity, compare

pytestmark = pytest.mark.gpu

_oracle = {}


def _reference(name):
    """The oracle's frame, counters and per-pixel event mask of an aimed scene: rendered once, read-only."""
    if name not in _oracle:
        rgb, ctr, mask = S.census(S.scene(name), S.params(name))
        rgb.setflags(write=False)
        mask.setflags(write=False)
        _oracle[name] = (rgb, ctr, mask)
    return _oracle[name]


def _check(gpu, name, options):
    sc, p = S.scene(name), S.params(name)
    ref, ctr, mask = _reference(name)
    rgb, _, st = gpu.render(sc, p, options=options)
    c = compare(rgb, ref)
    err = np.where(np.isnan(rgb) & np.isnan(ref), 0.0, np.abs(rgb - ref)).max(axis=-1)
    print(name, options, c, "rays", st["rays"], ctr["rays"])
    for j, i in np.argwhere(~(err <= TOL_EXACT))[:12]:  # a pixel that differs is a finding: which branches it took
        print(f"  pixel ({i}, {j}): gpu {rgb[j, i]} oracle {ref[j, i]} events {S.pixel_events(mask[j, i])}")
    assert c["nan_mismatch"] == 0 and c["not_exact"] == 0, c
    assert (st["rays"], st["samples"], st["pixels"]) == (ctr["rays"], ctr["samples"], p.width * p.height), (st, ctr)


@pytest.mark.parametrize("fmt", ["f32", "q8", "w8"])
@pytest.mark.parametrize("name", list(S.SCENES))
def test_parity_with_oracle(gpu, oracle, name, fmt):
    _check(gpu, name, {"builder": "host", "node_format": fmt})


@pytest.mark.parametrize("fmt", ["f32", "q8"])
@pytest.mark.parametrize("builder", ["gpu", "ploc"])
def test_meshes_on_the_device_builders(gpu, oracle, builder, fmt):
    _check(gpu, "meshes", {"builder": builder, "node_format": fmt})


@pytest.mark.parametrize("always_max", [0, 4])
def test_sky_offset_inside_and_outside_the_tree(gpu, oracle, always_max):
    _check(gpu, "sky_offset", {"always_max": always_max})


# ---- closest hits on three meshes ------------------------------------------------------------------------------------

_mesh_hits = []


def _brute_force_hits():
    """(scene, rays, brute-force Hit records, materials, the hits' mesh): made once, read-only."""
    if _mesh_hits:
        return _mesh_hits[0]
    sc, rays = S.mesh_rays()
    bf = Brute(sc)
    ref = bf.closest(rays)
    assert not ref["tie"].any()
    rec, mats, is_tri = bf.records(rays, ref)
    mesh = np.full(len(rays), -1, dtype=np.int64)
    mesh[is_tri] = bf.tri_mesh[np.searchsorted(bf.tri_id, ref["id"][is_tri])]
    for a in (rec, mats, mesh):
        a.setflags(write=False)
    _mesh_hits.append((sc, rays, rec, mats, mesh))
    return _mesh_hits[0]


@pytest.mark.parametrize("builder,fmt", [("host", "f32"), ("host", "q8"), ("host", "w8"), ("gpu", "f32"), ("gpu", "q8"),
                                         ("ploc", "f32"), ("ploc", "q8")])
def test_intersect_on_three_meshes(gpu, builder, fmt):
    """t, position, normal and material bit for bit, uv within the 1e-12 of the other intersect tests; every mesh is
    hit (vertex base offsets of meshes 1 and 2, each mesh's own normals, uvs and material)."""
    sc, rays, rec, mats, mesh = _brute_force_hits()
    with gpu.DeviceScene(sc, options={"builder": builder, "node_format": fmt}) as ds:
        hits, got = ds.intersect(rays)
    assert (np.bincount(mesh[mesh >= 0], minlength=3) >= 100).all() and (mesh < 0).sum() >= 100
    assert np.array_equal(hits[:, 0], rec[:, 0]), np.nonzero(hits[:, 0] != rec[:, 0])[0][:10]
    assert np.array_equal(got, mats), np.nonzero(got != mats)[0][:10]
    bad = np.nonzero((hits[:, 1:7] != rec[:, 1:7]).any(axis=1))[0]
    assert len(bad) == 0, (bad[:10], mesh[bad[:10]])
    assert np.max(np.abs(hits[:, 7:9] - rec[:, 7:9])) < 1e-12


# ---- the feature pass ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", list(S.AOV_FRAMES))
def test_feature_pass(gpu, frame):
    """rp_render_aov normal, albedo and foreground at 4 spp and depth at 1 spp, asserted as tests/test_gpu_aov.py
    asserts them on the catalogue frames."""
    S.add_aov_frames()
    r = aov_ref.refs(frame, 4)
    with gpu.DeviceScene(r["scene"]) as ds:
        out = ds.render_aov(r["params"])
        for k in ("normal", "albedo"):
            c = compare(out[k], r[k])
            print(frame, k, c)
            assert_parity(c)
        assert np.array_equal(out["fg"], r["fg"])
        n = r["params"].width * r["params"].height
        assert (out["stats"]["rays"], out["stats"]["samples"], out["stats"]["pixels"]) == (4 * n, 4 * n, n)
        r1 = aov_ref.refs(frame, 1)
        d = ds.render_aov(r1["params"], normal=False, albedo=False)
    assert np.array_equal(d["fg"], r1["depth_fg"])
    assert np.array_equal(d["depth"] > 0, r1["depth"] > 0)
    err = np.abs(d["depth"] - r1["depth"]) / np.maximum(1.0, r1["depth"])
    print(frame, "max relative depth error", float(err.max()), "hit pixels", int((r1["depth"] > 0).sum()))
    assert err.max() <= TOL_EXACT


# ---- table order --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(S.PERMUTATIONS))
def test_table_order(gpu, name):
    """The texture, material and mesh tables reordered with every reference renumbered: the same frame bit for bit
    and the same counters.  No oracle: the device against itself."""
    sc, p = S.scene(name), S.params(name)
    rgb, _, st = gpu.render(sc, p)
    assert np.isfinite(rgb).all() and rgb.max() > 0.1
    for perm in S.PERMUTATIONS[name]:
        q = S.permuted(sc, **perm)
        if name == "sky_offset" and "tex" in perm:
            assert q.background.texture == perm["tex"].index(2)
        got, _, gst = gpu.render(q, p)
        assert np.array_equal(got, rgb), (perm, int((got != rgb).any(axis=-1).sum()))
        assert (gst["rays"], gst["samples"], gst["pixels"]) == (st["rays"], st["samples"], st["pixels"]), perm
