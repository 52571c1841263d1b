"""The refit on the device (rp_refit.hip): a scene's records read back with rp_scene_tree before and after an update
and held to tests/refit_ref.py, the refit written out in numpy, bit for bit; the refit scene's queries against the
oracle on the deformed description; its frames against a freshly created scene of that description.  Every comparison
is exact: the closest hit does not depend on the tree, and a refit node stores what the builders would store.

The deformation is refit_ref.deform: p' = p + a sin(3 p.yzx), a = 0.05 of the extent; normals n.yzx; radii x 1.1.
"""
import functools

import numpy as np
import pytest

import bvh_scenes as S
import refit_ref as RR
from rtpotato import _ffi as F
from rtpotato import scenes
from rtpotato.render import scene_geometry, unpack_shard, with_geometry
from rtpotato.scene import RenderParams, shard_slot_count

pytestmark = pytest.mark.gpu

# builder, node format, node layout
TREES = [(b, f, "auto") for b in ("host", "gpu", "ploc") for f in ("f32", "q8")] + [("ploc", "q8", "dfs_line")]
INPUTS = ["uniform_5", "uniform_257", "mixed", "clustered"]
CASES = [(n,) + t for n in INPUTS for t in TREES]
IDS = ["-".join(c) for c in CASES]


def _options(builder, fmt, layout="auto"):
    return {"builder": builder, "node_format": fmt, "node_layout": layout}


@functools.lru_cache(maxsize=None)
def _scene(name):
    return scenes.CATALOGUE[name]() if name in scenes.CATALOGUE else S.scene(name)


@functools.lru_cache(maxsize=None)
def _deformed(name):
    """(the deformed geometry, the deformed description), computed once and shared."""
    g = RR.deform(scene_geometry(_scene(name)))
    for a in g.values():
        a.setflags(write=False)
    return g, with_geometry(_scene(name), g["positions"], g["normals"], g["spheres"])


def _args(g):
    return g["positions"], g["normals"], g["spheres"]


def _same_tree(a, b, what):
    for k in ("nodes", "prims", "prim_refs"):
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("name,builder,fmt,layout", CASES, ids=IDS)
def test_records(gpu, name, builder, fmt, layout):
    """Identity: a refit with the scene's own geometry() changes no byte of the nodes, prims and refs, status 0.
    Deformed: the read-back nodes are refit_ref applied to the read-back "before" records, and the prims are those of a
    scene freshly created from the deformed description, matched through PrimRef.src.  Back: the original bytes."""
    sc = _scene(name)
    g1, sc1 = _deformed(name)
    with gpu.DeviceScene(sc, options=_options(builder, fmt, layout)) as ds:
        before = ds.tree()
        g0 = ds.geometry()
        with ds.refit_handle(coord_max=2.0 ** 12) as rf:
            info = rf.info()
            assert (info["vertices"], info["spheres"]) == (len(g0["positions"]), len(g0["spheres"]))
            assert info["levels"] >= 1 and info["bound"] == 2.0 ** 12
            st, sec = rf.update(*_args(g0))
            assert st == 0 and sec >= 0.0
            _same_tree(ds.tree(), before, "identity")
            assert rf.update(*_args(g1))[0] == 0
            after = ds.tree()
            assert rf.update(*_args(g0))[0] == 0
            _same_tree(ds.tree(), before, "there and back")
    want = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in before.items()}
    assert RR.refit(want, None, g1["positions"], None, g1["spheres"], 2.0 ** 12) == 0
    _same_tree(after, want, "deformed")
    assert after["prims"].tobytes() != before["prims"].tobytes()
    with gpu.DeviceScene(sc1, options=_options(builder, fmt, layout)) as fresh:
        ft = fresh.tree()
    by_src = np.argsort(ft["prim_refs"]["src"])
    assert after["prims"].tobytes() == ft["prims"][by_src][after["prim_refs"]["src"]].tobytes()


def _rays(sc, n_random=1024, w=64, h=48):
    """The pinhole camera's rays through the pixel centres of a w x h frame, then random rays aimed at the geometry."""
    cam = sc.camera
    ii, jj = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    t = np.tan(0.5 * cam.fov) * cam.focal_dist
    x, y = (2.0 * ii / w - 1.0) * t * cam.aspect_ratio, (2.0 * jj / h - 1.0) * t
    z = np.full_like(x, -cam.focal_dist)
    m = np.array(cam.transformation.orientation).reshape(3, 3)  # column-major: rows of this array are the columns
    d = np.stack([x, y, z], axis=-1).reshape(-1, 3) @ m
    o = np.tile(np.array(cam.transformation.position), (len(d), 1))
    # targets strictly inside a triangle (random barycentric weights) or at a small sphere's centre: a ray through a
    # vertex or an edge lies on the boundary of the triangle test, and of all the triangles that share it -- ties
    rng = np.random.default_rng(0xF17)
    g = scene_geometry(sc)
    tris = [m.positions[m.indices.reshape(-1, 3).astype(np.int64)] for m in sc.scene_data.mesh_table]
    tris = np.concatenate(tris) if tris else np.zeros((0, 3, 3))
    centres = g["spheres"][g["spheres"][:, 3] < 100.0, :3]
    pick = rng.integers(0, len(tris) + len(centres), size=n_random)
    wts = rng.dirichlet(np.ones(3), size=n_random)
    target = np.empty((n_random, 3))
    on_tri = pick < len(tris)
    target[on_tri] = np.einsum("kv,kvc->kc", wts[on_tri], tris[pick[on_tri]])
    target[~on_tri] = centres[pick[~on_tri] - len(tris)]
    dirs = rng.normal(size=(n_random, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    ext = float(np.abs(target - target.mean(axis=0)).max()) + 1.0
    o2 = target - dirs * ext * rng.uniform(2.0, 3.0, size=(n_random, 1))
    rays = np.concatenate([np.concatenate([o, o2]), np.concatenate([d, target - o2])], axis=1)
    return np.concatenate([rays, np.full((len(rays), 1), 1e-3), np.full((len(rays), 1), np.inf)], axis=1)


@pytest.mark.parametrize("opts", [{}, _options("ploc", "q8")], ids=["default", "ploc-q8"])
@pytest.mark.parametrize("name", ["mixed", "three_balls", "bunny_lambert"])
def test_queries(gpu, oracle, name, opts):
    """rp_intersect on the refit scene against the oracle's intersect on the deformed description: 4,096 rays, the hit
    records -- t, position, NORMAL (the per-primitive normals moved with the refit) -- bit for bit, the materials
    equal."""
    sc = _scene(name)
    g1, sc1 = _deformed(name)
    rays = _rays(sc1)
    assert len(rays) == 4096
    with gpu.DeviceScene(sc, options=opts) as ds, ds.refit_handle(coord_max=2.0 ** 12) as rf:
        assert rf.update(*_args(g1))[0] == 0
        hits, mats = ds.intersect(rays)
    d = sc1.desc()
    osc = oracle.OracleScene(d.addr(), d)
    ref, ref_mats, _ = osc.intersect(rays)
    osc.close()
    hit = np.isfinite(ref[:, 0])
    assert hit.sum() > 1024
    assert np.array_equal(np.isfinite(hits[:, 0]), hit)
    np.testing.assert_array_equal(hits[hit, :7], ref[hit, :7])
    assert np.array_equal(mats[hit], ref_mats[hit])
    assert np.max(np.abs(hits[hit, 7:] - ref[hit, 7:])) < 1e-12  # uv, as test_intersect_rays


FRAMES = [("bunny_lambert", 96, 64), ("three_balls", 64, 48), ("variants", 64, 48)]


@pytest.mark.parametrize("fmt", ["f32", "q8"])
@pytest.mark.parametrize("name,w,h", FRAMES, ids=[f[0] for f in FRAMES])
def test_frames(gpu, name, w, h, fmt):
    """render and render_aov after the refit are those of a freshly created scene of the deformed description, bit for
    bit; q8 with twice the build's bound.  Widening the bound alone, without an update, leaves the frame as it was."""
    sc = scenes.configure(_scene(name), w, h)
    g1, sc1 = _deformed(name)
    sc1 = scenes.configure(sc1, w, h)
    p = RenderParams(w, h, 4, 8, scenes.DEFAULT_SEED)
    opts = {"node_format": fmt}
    with gpu.DeviceScene(sc, options=opts) as ds:
        first = ds.render(p)[0]
        with ds.refit_handle() as rf0:
            build_bound = rf0.info()["bound"]
        with ds.refit_handle(coord_max=2.0 * build_bound) as rf:
            assert rf.info()["bound"] == 2.0 * build_bound
            assert np.array_equal(ds.render(p)[0], first)  # the bound alone
            assert rf.update(*_args(g1))[0] == 0
            rgb = ds.render(p)[0]
            aov = ds.render_aov(p)
    with gpu.DeviceScene(sc1, options=opts) as fresh:
        want = fresh.render(p)[0]
        want_aov = fresh.render_aov(p)
    assert not np.array_equal(rgb, first)
    assert np.array_equal(rgb, want)
    for k in ("normal", "albedo", "depth", "fg"):
        assert np.array_equal(aov[k], want_aov[k]), k


@pytest.mark.parametrize("fmt", ["f32", "q8"])
def test_normals_alone(gpu, oracle, fmt):
    """A refit of the normals only changes no node or prim byte; the hit records' normals are the new ones."""
    name = "uniform_257"
    sc = _scene(name)
    g1, _ = _deformed(name)
    sc_n = with_geometry(sc, normals=g1["normals"])
    rays = _rays(sc, 1024, 32, 32)
    with gpu.DeviceScene(sc, options=_options("ploc", fmt)) as ds, ds.refit_handle() as rf:
        before = ds.tree()
        assert rf.update(normals=g1["normals"])[0] == 0
        _same_tree(ds.tree(), before, "normals only")
        hits, _ = ds.intersect(rays)
    d = sc_n.desc()
    osc = oracle.OracleScene(d.addr(), d)
    ref, _, _ = osc.intersect(rays)
    osc.close()
    hit = np.isfinite(ref[:, 0])
    assert hit.sum() >= 256
    np.testing.assert_array_equal(hits[hit, :7], ref[hit, :7])


def test_refusals(gpu):
    """What needs a scene: an 8-wide tree, coord_max out of range, an update that names nothing or the geometry in
    part, a NULL status."""
    import ctypes
    L = F.rp()
    h = ctypes.c_void_p()
    sc = _scene("mixed")
    g = scene_geometry(sc)
    with gpu.DeviceScene(_scene("uniform_257"), options={"node_format": "w8"}) as ds:
        assert L.rp_refit_create(ds.handle, 0.0, ctypes.byref(h)) == F.RP_EINVAL and not h.value
        assert b"8-wide" in L.rp_last_error()
    with gpu.DeviceScene(sc) as ds:
        for bad in (-1.0, float("nan"), float("inf"), 2.0 ** 55):
            assert L.rp_refit_create(ds.handle, bad, ctypes.byref(h)) == F.RP_EINVAL and not h.value
        before = ds.tree()
        with ds.refit_handle() as rf:
            for args in ((None, None, None), (g["positions"], None, None), (None, None, g["spheres"])):
                with pytest.raises(F.RPError) as e:
                    rf.update(*args)
                assert e.value.code == F.RP_EINVAL
            with pytest.raises(ValueError):
                rf.update(g["positions"][:-1], None, g["spheres"])
            pos = np.ascontiguousarray(g["positions"])
            assert L.rp_scene_refit(rf.handle, pos.ctypes.data, None, g["spheres"].ctypes.data, None, None) == F.RP_EINVAL
            _same_tree(ds.tree(), before, "refused calls write nothing")


def test_async_form(gpu):
    """update_device on a side stream followed by render_device on the same stream is the synchronous path, its status
    tensor 0.  A vertex beyond the bound on an f32 scene sets the bit, and the frame is still the fresh scene's."""
    import torch
    name = "uniform_257"
    sc = _scene(name)
    g1, sc1 = _deformed(name)
    p = RenderParams(64, 48, 4, 8, scenes.DEFAULT_SEED)
    n = shard_slot_count(p)
    far = {k: np.array(v) for k, v in g1.items()}
    with gpu.DeviceScene(sc, options=_options("ploc", "f32")) as ds, ds.refit_handle(coord_max=2.0) as rf:
        bound = rf.info()["bound"]
        assert bound == 2.0  # covers the deformation (the mesh lies in [-1.005, 1.005], a = 0.1)
        far["positions"][100] = [2.5 * bound, 0.25, -0.5]
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            pos, nrm = (torch.from_numpy(np.array(g1[k])).cuda() for k in ("positions", "normals"))
            pos_far = torch.from_numpy(far["positions"]).cuda()
            out, out_far = (torch.zeros(3 * n, dtype=torch.float64, device="cuda") for _ in range(2))
            ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device="cuda")
            status = rf.update_device(pos, nrm, stream=st)
            ds.render_device(p, out, ctr, stream=st)
            status_far = rf.update_device(pos_far, nrm, stream=st)
            ds.render_device(p, out_far, ctr, stream=st)
        st.synchronize()
        assert status.tolist() == [0] and status_far.tolist() == [F.RP_REFIT_OUT_OF_BOUND]
        frame, frame_far = (unpack_shard(p, t.cpu().numpy()) for t in (out, out_far))
        assert rf.update(g1["positions"], g1["normals"])[0] == 0
        assert np.array_equal(frame, ds.render(p)[0])
    for want_sc, got in ((sc1, frame), (with_geometry(sc, far["positions"], far["normals"]), frame_far)):
        with gpu.DeviceScene(want_sc, options=_options("ploc", "f32")) as fresh:
            assert np.array_equal(got, fresh.render(p)[0])
