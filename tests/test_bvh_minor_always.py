"""The host builder's minor rule (rp_bvh.h BuildOptions::always_minor, on for every tree librp.so builds on the host):
a mesh scene's few non-triangle hittables join the always-tested list, so the tree's leaves hold triangles only.
Through the option-taking hooks of librp_host.so (rph_bvh_*_opt), CPU only: the tree the renderer uses is valid,
finds the default tree's closest hittables, costs fewer node visits, and scenes the rule does not apply to keep
their trees bit for bit."""
import ctypes
import math

import numpy as np
import pytest

from test_bvh import _rays_for

F32, Q8, W8 = 1, 2, 3  # RP_NODES_*
MISS = np.uint64(2**64 - 1)


def _stats(scene, fmt, always_max, minor):
    from rtpotato import _ffi as F
    d = scene.desc()
    st = (ctypes.c_uint64 * 6)()
    rc = F.host().rph_bvh_selfcheck_opt(d.ptr(), fmt, F.RP_COLLAPSE_AUTO, always_max, minor, st)
    assert rc == 0, (F.host().rph_last_error() or b"").decode()
    return list(st)


def _trace(scene, rays, fmt, always_max, minor):
    from rtpotato import _ffi as F
    d = scene.desc()
    out = np.zeros((len(rays), 3), dtype=np.uint64)
    F.check_host(F.host().rph_bvh_traversal_stats_opt(d.ptr(), rays.ctypes.data, len(rays), fmt, F.RP_COLLAPSE_AUTO,
                                                      always_max, minor, out.ctypes.data))
    return out


def _hash(scene, fmt, always_max, minor):
    from rtpotato import _ffi as F
    d = scene.desc()
    h = ctypes.c_uint64()
    F.check_host(F.host().rph_bvh_tree_hash_opt(d.ptr(), fmt, 0, always_max, minor, ctypes.byref(h)))
    return h.value


def _camera_rays(scene, w, h, seed):
    """One ray per pixel of a w x h frame through the scene's camera as a pinhole (Camera::shoot, render.rs:32-52,
    without the lens offset), at a random position inside the pixel."""
    cam = scene.camera
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    u = (ii + rng.uniform(size=ii.shape)) / w
    v = (jj + rng.uniform(size=ii.shape)) / h
    tanf = math.tan(0.5 * cam.fov)
    x = (2.0 * u - 1.0) * tanf * cam.focal_dist * (w / h)
    y = (2.0 * v - 1.0) * tanf * cam.focal_dist
    z = np.full_like(x, -cam.focal_dist)
    m = cam.transformation.orientation  # column-major
    d = np.stack([x * m[0] + y * m[3] + z * m[6], x * m[1] + y * m[4] + z * m[7], x * m[2] + y * m[5] + z * m[8]], axis=-1)
    rays = np.empty((h * w, 8))
    rays[:, 0:3] = cam.transformation.position
    rays[:, 3:6] = d.reshape(-1, 3)
    rays[:, 6] = 1e-3
    rays[:, 7] = np.inf
    return rays


def _box_rays(n, seed):
    """Random rays in the box of bunny_full without its ground: origins uniform in the box, directions uniform on
    the sphere."""
    rng = np.random.default_rng(seed)
    o = rng.uniform([-1.6, 0.0, -1.3], [1.7, 1.0, 0.5], size=(n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d, np.full((n, 1), 1e-3), np.full((n, 1), np.inf)], axis=1)


@pytest.fixture(scope="module")
def bunny_full():
    from rtpotato import scenes
    return scenes.bunny_full()


@pytest.mark.parametrize("fmt", [F32, Q8, W8])
def test_bunny_full_tree_holds_triangles_only(bunny_full, fmt):
    """The ground (the size rule) and the two balls (the minor rule) are always tested, no sphere is left inside the
    tree, and the structural self-check passes; without the rule the two balls are in the tree."""
    nodes, leaves, depth, prims, n_always, inside = _stats(bunny_full, fmt, -1, 1)
    assert (prims, n_always, inside) == (4971, 3, 0)
    assert leaves >= 4968 // 8 and nodes >= 1
    assert _stats(bunny_full, fmt, -1, 0)[4:] == [1, 2]
    assert _stats(bunny_full, fmt, 0, 1)[4:] == [0, 3]  # always_max = 0: every hittable in the tree, rule or not


@pytest.mark.parametrize("fmt", [F32, Q8])
def test_same_closest_hittable_on_random_and_adversarial_rays(bunny_full, fmt):
    """tests/test_bvh.py's rays, adversarial ones included.  The closest hittable is the default tree's on every ray
    but exact-t ties: a ray made to run along a mesh edge ([4k, 5k)) meets the triangles around a vertex at one and the
    same t, and among equal t the one tested last wins (hittable.rs:52,99), which any change of a tree's shape reorders
    (SURVEY.md 8a A9).  Where the ids differ, both must be such triangles and their exact tests (rph_prim_test) must
    accept this ray at bitwise the same t: the closest hit is the same distance, only the tie's winner moved."""
    from rtpotato import _ffi as F
    rays = _rays_for(bunny_full, 40000, 3)
    a, b = _trace(bunny_full, rays, fmt, -1, 0), _trace(bunny_full, rays, fmt, -1, 1)
    diff = np.nonzero(a[:, 2] != b[:, 2])[0]
    k = len(rays) // 10
    print(f"fmt {fmt}: {len(diff)} of {len(rays)} rays name another hittable")
    assert np.all((diff >= 4 * k) & (diff < 5 * k)), diff[:10]
    assert len(diff) <= k // 20, len(diff)
    mesh = bunny_full.scene_data.mesh_table[0]
    tri = mesh.indices.reshape(-1, 3)
    for r in diff:
        ts = []
        for hid in (int(a[r, 2]), int(b[r, 2])):
            assert hid < len(tri), (r, hid)  # a triangle of the bunny, not a miss and not a sphere
            p0, p1, p2 = (mesh.positions[i] for i in tri[hid])
            g = np.concatenate([p0, p0 - p1, p0 - p2])
            out = np.zeros(4)
            ray = np.ascontiguousarray(rays[r])
            F.check_host(F.host().rph_prim_test(1, g.ctypes.data, ray.ctypes.data, 1, out.ctypes.data))
            assert out[0] == 1.0, (r, hid)
            ts.append(out[1])
        assert ts[0] == ts[1], (r, ts)
    assert (a[:, 2] != MISS).sum() > 1000
    assert (b[:, 1] >= 3).all()  # every ray tests the three always-tested spheres


def test_same_closest_hittable_and_fewer_visits_on_camera_and_box_rays(bunny_full):
    """Mean node visits at most 0.92 of the default tree's (200 k rays each: 0.85 on C3's camera rays, 0.83 on random
    rays in the scene's box; the slack is for these smaller samples)."""
    from rtpotato import scenes
    cam = _camera_rays(scenes.config_scene("C3")[0], 240, 135, 5)
    box = _box_rays(30000, 6)
    for what, rays in (("camera", cam), ("box", box)):
        a, b = _trace(bunny_full, rays, F32, -1, 0), _trace(bunny_full, rays, F32, -1, 1)
        assert (a[:, 2] == b[:, 2]).all(), what
        ratio = b[:, 0].mean() / a[:, 0].mean()
        print(f"{what}: visits per ray {a[:, 0].mean():.3f} -> {b[:, 0].mean():.3f} ({ratio:.3f}), "
              f"tests per ray {a[:, 1].mean():.3f} -> {b[:, 1].mean():.3f}")
        assert ratio <= 0.92, (what, ratio)
        # hits on the balls, the ground, the bunny and misses are all in the sample
        ids = a[:, 2]
        assert (ids == 4969).any() and (ids == 4970).any() and (ids == 4968).any() and (ids < 4968).any()
        assert what == "box" or (ids == MISS).any()


@pytest.mark.parametrize("fmt", [F32, Q8, W8])
@pytest.mark.parametrize("name,arg,always_max", [
    ("three_balls", None, -1), ("more_balls", None, -1), ("earth", None, -1),  # spheres only
    ("variants", None, -1),        # five spheres and a triangle: over the cap, and under the triangle floor
    ("one_triangle", None, -1),    # one triangle: under the floor
    ("random_mesh", 20000, -1),    # triangles only
    ("bunny_full", None, 0),       # always_max = 0 puts every hittable in the tree
])
def test_other_trees_unchanged(name, arg, always_max, fmt):
    from rtpotato import scenes
    scene = scenes.CATALOGUE[name](arg) if arg else scenes.CATALOGUE[name]()
    assert _hash(scene, fmt, always_max, 1) == _hash(scene, fmt, always_max, 0)


def test_rule_off_is_the_default_hooks_tree(bunny_full):
    """The hooks without the options build what they built: rph_bvh_tree_hash is rph_bvh_tree_hash_opt(-1, 0)."""
    from rtpotato import _ffi as F
    d = bunny_full.desc()
    h = ctypes.c_uint64()
    F.check_host(F.host().rph_bvh_tree_hash(d.ptr(), F32, 0, ctypes.byref(h)))
    assert h.value == _hash(bunny_full, F32, -1, 0) != _hash(bunny_full, F32, -1, 1)


def test_cap_and_floor():
    """The rule's conditions on a mesh of 20 triangles: four spheres with the ground are over always_max = 4, three
    spheres with it are not; 15 triangles are under the floor of 16 (rp_bvh.h ALWAYS_MINOR_MIN_TRIS)."""
    from rtpotato.scene import (Absorb, Camera, Emit, Hittable, Material, Mesh, Scatter, Scene, SceneData,
                                Transformation, hittables)
    cam = Camera(1.0, 1.0, 1.0, 0.0, Transformation.lookat((0, 0, 3), (0, 0, 0), (0, 1, 0)))
    mat = [Material.new(Scatter.Lambert, Absorb.Albedo((0.5, 0.5, 0.5)), Emit.None_)]

    def scene(n_tri, n_small):
        rng = np.random.default_rng(n_tri)
        pos = (rng.uniform(-1, 1, size=(n_tri, 1, 3)) + rng.uniform(-0.1, 0.1, size=(n_tri, 3, 3))).reshape(-1, 3)
        mesh = Mesh(pos, np.zeros_like(pos), np.zeros((3 * n_tri, 2)), np.arange(3 * n_tri, dtype=np.uint32))
        balls = [Hittable.Sphere((0.3 * k, 0.0, 0.0), 0.2, 0) for k in range(n_small)]
        root = hittables(Hittable.Triangle(mesh.iter_triangles(), 0), Hittable.Sphere((0.0, -1000.0, 0.0), 999.0, 0), *balls)
        return Scene(cam, SceneData(mat, [], [mesh]), root, Emit.SkyGradient)

    assert _stats(scene(20, 3), F32, -1, 1)[4:] == [4, 0]
    assert _stats(scene(20, 4), F32, -1, 1)[4:] == [1, 4]
    assert _stats(scene(20, 3), F32, 3, 1)[4:] == [1, 3]  # the cap is always_max
    assert _stats(scene(16, 3), F32, -1, 1)[4:] == [4, 0]
    assert _stats(scene(15, 3), F32, -1, 1)[4:] == [1, 3]
