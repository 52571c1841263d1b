"""GPU parity with a mesh scene's few spheres on the always-tested list (rp_bvh.h BuildOptions::always_minor, on for
every host-built tree): the render kernel tests them once per ray at its per-round site instead of in the tree's
leaves.  Against the CPU oracle at 64 x 40, 6 spp, max_bounce 8, in both node formats whose always site the rule feeds
(f32 nodes, and q8 nodes over the host builder's tree): every pixel exact (parity.py: to 1e-12) and the ray count the
oracle's."""
import numpy as np
import pytest

from parity import compare, oracle_render

pytestmark = pytest.mark.gpu

FORMATS = {"f32": {}, "q8": {"node_format": "q8", "builder": "host"}}


def _params():
    from rtpotato import scenes
    from rtpotato.scene import RenderParams
    return RenderParams(64, 40, 6, 8, scenes.DEFAULT_SEED)


def wall_scene():
    """48 triangles scattered in a slab around z = 0, a metal sphere that overlaps their box (parts of it in front of
    triangles, parts behind), a glass sphere behind them along the camera axis (seen through the gaps, hidden behind the
    triangles elsewhere) and the ground: a sphere hit at the always site must win against some triangle hits and lose
    against others, for camera rays and for scattered ones."""
    from rtpotato import scenes
    from rtpotato.scene import (Absorb, Camera, Emit, Hittable, Material, Mesh, Scatter, Scene, SceneData,
                                Transformation, hittables)
    rng = np.random.default_rng(22)
    n = 48
    c = rng.uniform([-0.9, 0.1, -0.25], [0.9, 1.1, 0.25], size=(n, 1, 3))
    v = c + rng.uniform(-0.2, 0.2, size=(n, 3, 3))
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    pos = v.reshape(-1, 3)
    mesh = Mesh(pos, np.repeat(nrm, 3, axis=0), np.zeros((len(pos), 2)), np.arange(3 * n, dtype=np.uint32), material=0)
    materials = [Material.new(Scatter.Lambert, Absorb.Albedo((0.7, 0.3, 0.3)), Emit.None_),
                 Material.new(Scatter.Metal(0.05), Absorb.Albedo((0.8, 0.8, 0.8)), Emit.None_),
                 Material.new(Scatter.Dielectric(1.5), Absorb.Albedo((0.9, 0.9, 1.0)), Emit.None_),
                 Material.new(Scatter.Lambert, Absorb.Albedo((0.5, 0.5, 0.5)), Emit.None_)]
    root = hittables(Hittable.Triangle(mesh.iter_triangles(), 0),
                     Hittable.Sphere((0.0, -1000.0, 0.0), 1000.0, 3),
                     Hittable.Sphere((0.35, 0.55, -0.2), 0.35, 1),   # overlaps the triangles' box
                     Hittable.Sphere((-0.2, 0.6, -1.3), 0.55, 2))    # behind them along the camera axis
    cam = Camera(1.0, 0.9, 1.0, 0.0, Transformation.lookat((0.0, 0.6, 3.0), (0.0, 0.6, 0.0), (0.0, 1.0, 0.0)))
    return scenes.configure(Scene(cam, SceneData(materials, [], [mesh]), root, Emit.SkyGradient), 64, 40)


@pytest.fixture(scope="module")
def refs():
    """name -> (scene, oracle image, oracle foreground, oracle counters): rendered once, read by every case."""
    from rtpotato import scenes
    out = {}
    for name, sc in (("bunny_full", scenes.configure(scenes.bunny_full(), 64, 40)), ("wall", wall_scene())):
        ref, fg, ctr = oracle_render(sc, _params(), threads=8, foreground=True)
        out[name] = (sc, ref, fg, ctr)
    return out


def _exact(gpu, refs, name, options):
    sc, ref, ref_fg, ctr = refs[name]
    rgb, fg, st = gpu.render(sc, _params(), foreground=True, options=options)
    c = compare(rgb, ref)
    print(f"{name} {options}: rays {st['rays']} (oracle {ctr['rays']}), linf {c['linf']:.3g}, not exact {c['not_exact']}")
    assert c["nan_mismatch"] == 0 and c["not_exact"] == 0, c
    assert (st["rays"], st["samples"]) == (ctr["rays"], ctr["samples"]), (st, ctr)
    assert np.array_equal(fg, ref_fg)
    return rgb


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_bunny_full_default_options(gpu, refs, fmt):
    _exact(gpu, refs, "bunny_full", dict(FORMATS[fmt]))


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_wall_scene_spheres_at_the_always_site_and_in_the_tree(gpu, refs, fmt):
    """The defaults (ground and both spheres always tested, a triangle-only tree) and always_max = 0 (all four in the
    tree): both the oracle's frame, and each other's bit for bit."""
    a = _exact(gpu, refs, "wall", dict(FORMATS[fmt]))
    b = _exact(gpu, refs, "wall", dict(FORMATS[fmt], always_max=0))
    assert np.array_equal(a, b)


def test_wall_scene_is_what_it_says(refs, oracle):
    """The scene's premise, on the oracle's closest hits of the frame's pixel-centre rays: both spheres are seen,
    triangles are seen in front of each of them, and the overlapping sphere is seen in front of triangles."""
    sc = refs["wall"][0]
    cam = sc.camera
    w, h = 64, 40
    ii, jj = np.meshgrid((np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h)
    tanf = np.tan(0.5 * cam.fov)
    x, y = (2 * ii - 1) * tanf * cam.focal_dist * cam.aspect_ratio, (2 * jj - 1) * tanf * cam.focal_dist
    m = cam.transformation.orientation
    z = np.full_like(x, -cam.focal_dist)
    d = np.stack([x * m[0] + y * m[3] + z * m[6], x * m[1] + y * m[4] + z * m[7], x * m[2] + y * m[5] + z * m[8]], -1)
    rays = np.empty((w * h, 8))
    rays[:, 0:3] = cam.transformation.position
    rays[:, 3:6] = d.reshape(-1, 3)
    rays[:, 6], rays[:, 7] = 1e-3, np.inf
    desc = sc.desc()
    hits, mats, _ = oracle.OracleScene(desc.addr(), desc).intersect(rays)
    seen = {k: int((mats == k).sum()) for k in range(4)}
    assert all(seen[k] >= 20 for k in range(4)), seen
    # a triangle in front of each sphere: the ray's closest hit is a triangle and the sphere's own test hits further on
    o, dd = rays[:, 0:3], rays[:, 3:6]
    for centre, r, mat in (((0.35, 0.55, -0.2), 0.35, 1), ((-0.2, 0.6, -1.3), 0.55, 2)):
        tc = o - np.array(centre)
        a_, hb, cq = (dd * dd).sum(1), (dd * tc).sum(1), (tc * tc).sum(1) - r * r
        disc = hb * hb - a_ * cq
        t_s = np.where(disc > 0, (-hb - np.sqrt(np.maximum(disc, 0))) / a_, np.inf)
        on_line = np.isfinite(t_s)
        assert ((mats == 0) & on_line & (hits[:, 0] < t_s)).sum() >= 5, (mat, "never hidden by a triangle")
        assert ((mats == mat) & on_line).sum() >= 20, (mat, "never seen")
    # the overlapping sphere in front of a triangle: some ray whose closest hit is that sphere also meets a triangle
    # further on -- with the sphere out of the scene its closest hit is a triangle
    from dataclasses import replace
    no_ball = replace(sc, root=np.delete(sc.root, 49))
    d2 = no_ball.desc()
    _, mats2, _ = oracle.OracleScene(d2.addr(), d2).intersect(rays)
    assert ((mats == 1) & (mats2 == 0)).sum() >= 5
