"""The device's ray setup and box test (rp_ray.h through setup_ray32 / trav_step, rp_device.h) on the GPU: closest hits
of hand-picked ray families through rp_intersect against brute force over every hittable (tests/brute.py), in the
three node formats, and one small frame of the full-materials scene against the oracle -- with the whole stack in LDS
and with the stack split so that the SPILL kernel's global run is used (options.lds_depth = 8, the option that forces
the split; debug_stack_depth would make the stack overflow instead, which gives wrong frames by design).

rp_intersect returns the reference's Hit record (t, position, normal, uv, material), not the primitive index and the
barycentrics: the record is recomputed here from the brute-force (hittable, t, u, v) in the reference's expression
order, so equal records mean equal primitive, t, u and v.  Everything is compared bit for bit except a sphere's uv
(atan2 / asin: OCML against numpy's libm, 1e-12 as in tests/test_gpu_parity.py), and except, for rays with an exact-t
tie between two hittables (rays through a shared vertex or along a shared edge), everything but t: which of the tied
hittables a tree returns is free.
"""
import numpy as np
import pytest

from brute import Brute
from parity import compare, oracle_render, shard_mask

pytestmark = pytest.mark.gpu

GRID = 30  # 30 x 30 quads: 1,800 triangles sharing vertices and edges


def _scene():
    from rtpotato.scene import (Absorb, Camera, Emit, Hittable, Material, Mesh, Scatter, Scene, SceneData,
                                Transformation, hittables)
    g = np.linspace(-1.0, 1.0, GRID + 1) * 1.0371  # not f32 values
    x, z = np.meshgrid(g, g, indexing="ij")
    y = 0.3 * np.sin(3.0 * x) * np.cos(2.0 * z) + 0.1
    pos = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    nrm = np.stack([-0.9 * np.cos(3.0 * x), np.ones_like(x), 0.6 * np.sin(2.0 * z)], axis=-1).reshape(-1, 3)
    nrm = nrm / np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])[:, None]
    uv = np.stack([(x + 1.1) / 2.2, (z + 1.1) / 2.2], axis=-1).reshape(-1, 2)
    i, j = np.meshgrid(np.arange(GRID), np.arange(GRID), indexing="ij")
    v00 = (i * (GRID + 1) + j).reshape(-1)
    v01, v10, v11 = v00 + 1, v00 + GRID + 1, v00 + GRID + 2
    idx = np.stack([v00, v10, v11, v00, v11, v01], axis=-1).reshape(-1).astype(np.uint32)
    mesh = Mesh(pos, nrm, uv, idx, material=0)
    mats = [Material.new(Scatter.Lambert, Absorb.Albedo((0.7, 0.7, 0.7)), Emit.None_),
            Material.new(Scatter.Metal(0.1), Absorb.Albedo((0.8, 0.6, 0.2)), Emit.None_)]
    root = hittables(Hittable.Triangle(mesh.iter_triangles(), 0), Hittable.Sphere((0.31, 0.93, -0.22), 0.35, 1),
                     Hittable.Sphere((-0.52, -0.81, 0.43), 0.5, 1))
    cam = Camera(1.0, 1.0, 1.0, 0.0, Transformation.lookat((0, 2, 3), (0, 0, 0), (0, 1, 0)))
    from rtpotato import _ffi as F
    return Scene(cam, SceneData(mats, [], [mesh]), root, Emit.SkyGradient, F.RP_ROOT_BVH, "ray_setup_grid")


def _rays(scene):
    rng = np.random.default_rng(0xbeef)
    m = scene.scene_data.mesh_table[0]
    tri = m.indices.reshape(-1, 3)
    fam = []

    def add(o, d, tmin=1e-3, tmax=np.inf):
        n = len(o)
        fam.append(np.concatenate([o, d, np.broadcast_to(np.asarray(tmin, float), (n,)).reshape(n, 1),
                                   np.broadcast_to(np.asarray(tmax, float), (n,)).reshape(n, 1)], axis=1))

    def origins(n):
        o = rng.uniform(-2.0, 2.0, size=(n, 3))
        o[:, 1] = rng.uniform(-1.8, 2.2, size=n)
        return o

    def towards(o):
        return rng.uniform(-0.9, 0.9, size=(len(o), 3)) * np.array([1.0, 0.4, 1.0]) - o

    o = origins(900)
    add(o, towards(o))                                           # random
    for z in (0.0, -0.0):                                         # axis-parallel, a zero component of either sign
        o = origins(250)
        d = towards(o)
        d[np.arange(250), rng.integers(0, 3, size=250)] = z
        d[:80, 0] = z
        d[:80, 2] = z                                             # straight up / down
        add(o, d)
    o = origins(200)
    d = towards(o)
    d[np.arange(200), rng.integers(0, 3, size=200)] = rng.choice([-1.0, 1.0], size=200) * 2.0 ** rng.uniform(-62, -58, size=200)
    add(o, d)                                                     # a component near 2^-60
    o = origins(200)
    add(o, towards(o) * 2.0 ** rng.uniform(58, 62, size=(200, 1)), tmin=0.0)  # components near 2^60 (t near 2^-60)
    o = origins(300).astype(np.float32).astype(np.float64)
    add(o, towards(o))                                            # origins that are f32 values
    o = np.round(origins(100))
    add(o, towards(o))
    far = towards(np.zeros((200, 3)))
    far = far / np.sqrt((far * far).sum(axis=1))[:, None]
    tgt = rng.uniform(-0.9, 0.9, size=(200, 3)) * np.array([1.0, 0.3, 1.0])
    add(tgt - far * 2.0 ** rng.uniform(10, 20, size=(200, 1)), far)  # large |o|: the origin's f32 rounding is ~1
    v = m.positions[rng.integers(0, len(m.positions), size=300)]
    o = origins(300)
    o[np.arange(300), rng.integers(0, 3, size=300)] = v[np.arange(300), rng.integers(0, 3, size=300)]
    add(o, towards(o))                                            # a coordinate shared with a vertex (a box plane)
    o = v.copy()
    o[:, 1] += rng.integers(0, 2, size=300) * 1.0
    add(o, rng.normal(size=(300, 3)))                             # starting on a vertex, or straight above one
    o = origins(200)
    add(o, m.positions[rng.integers(0, len(m.positions), size=200)] - o)   # through a vertex
    e = tri[rng.integers(0, len(tri), size=300)]
    a, b = m.positions[e[:, 0]], m.positions[e[:, 1]]
    add(a - 2.0 * (b - a), b - a)                                 # along an edge
    o = origins(400)
    add(o, towards(o), tmax=rng.uniform(0.05, 4.0, size=400))     # finite t_max
    rays = np.ascontiguousarray(np.concatenate(fam))
    assert len(rays) <= 4096
    return rays


@pytest.fixture(scope="module")
def reference():
    """(scene, rays, brute-force closest hits and the Hit records they imply): made once, read-only."""
    scene = _scene()
    rays = _rays(scene)
    bf = Brute(scene)
    ref = bf.closest(rays)
    rec, mats, is_tri = bf.records(rays, ref)
    hit = ref["id"] >= 0
    out = {"rec": rec, "mats": mats, "hit": hit, "tri": is_tri, "tie": ref["tie"].copy()}
    for a in out.values():
        a.setflags(write=False)
    rays.setflags(write=False)
    return scene, rays, out


@pytest.mark.parametrize("fmt", ["f32", "q8", "w8"])
def test_intersect_equals_brute_force(gpu, reference, fmt):
    scene, rays, ref = reference
    assert len(scene.root) <= 2002
    with gpu.DeviceScene(scene, options={"builder": "host", "node_format": fmt}) as ds:
        hits, mats = ds.intersect(rays)  # raises on a stack-overflow status
    hit, tie = ref["hit"], ref["tie"]
    assert hit.sum() > len(rays) // 3 and (~hit).sum() > 100 and ref["tri"].sum() > 500 and (hit & ~ref["tri"]).sum() > 100
    assert 0 < tie.sum() < len(rays) // 8
    assert np.array_equal(np.isfinite(hits[:, 0]), hit)
    assert np.array_equal(hits[:, 0], ref["rec"][:, 0]), np.nonzero(hits[:, 0] != ref["rec"][:, 0])[0][:10]
    u = ~tie
    assert np.array_equal(mats[u], ref["mats"][u])
    bad = np.nonzero(u & (hits[:, 1:7] != ref["rec"][:, 1:7]).any(axis=1))[0]
    assert len(bad) == 0, bad[:10]
    t = u & ref["tri"]
    assert np.array_equal(hits[t, 7:9], ref["rec"][t, 7:9])
    s = u & hit & ~ref["tri"]
    assert np.max(np.abs(hits[s, 7:9] - ref["rec"][s, 7:9])) < 1e-12


@pytest.mark.parametrize("options", [{}, {"lds_depth": 8}], ids=["lds", "spill"])
def test_frame_with_resumed_traversals(gpu, options):
    """64 x 64 x 4 spp of the full-materials scene (Lambert, Metal, Dielectric; textured spheres): the smallest frame
    with several shading rounds per wave and traversals resumed across them (best32 remade from the closest hit so
    far at every step).  Every pixel equal to the oracle's to parity.TOL_EXACT, the same ray and sample counts."""
    from rtpotato import scenes
    from rtpotato.scene import RenderParams
    sc = scenes.configure(scenes.bunny_full(), 64, 64)
    params = RenderParams(64, 64, 4, 8, scenes.DEFAULT_SEED)
    rgb, fg, st = gpu.render(sc, params, foreground=True, options=options)
    ref, ref_fg, ctr = oracle_render(sc, params, threads=8, foreground=True)
    mask = shard_mask(params)
    c = compare(rgb, ref, mask)
    print(c, st["rays"], ctr["rays"])
    assert c["nan_mismatch"] == 0 and c["not_exact"] == 0, c
    assert (st["rays"], st["samples"]) == (ctr["rays"], ctr["samples"]), (st, ctr)
    assert np.array_equal(fg[mask], ref_fg[mask])
