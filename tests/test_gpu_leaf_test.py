"""The device's exact primitive tests and leaf loop (prim_test, trav_step / trav_step_w8, rp_device.h) on the GPU:
closest hits of ray families aimed at every rejection of the two tests, through rp_intersect against brute force over
every hittable (tests/brute.py), bit for bit, in the three node formats.

The scene is a 30 x 30 grid of quads (1,800 triangles sharing vertices and edges) with twelve small spheres sitting on
the surface and two larger ones, all inside the tree (always_max = 0) and built with the largest leaves a format takes
(max_leaf 8; the 8-wide nodes: 4), so a leaf holds up to eight primitives and a sphere shares its leaf with the
triangles around it.  The families:

  plane    rays through the inside of a triangle, nearly in its plane: |det| from SMOL / 4 to 4 SMOL, both signs, and
           rays along an edge (det = 0 up to rounding); a rejected one passes through the triangle it is aimed at
  edge     vertical rays whose origin lies exactly on a grid line, so v (or u) of the edge's triangles is exactly +-0,
           and one ulp to either side of it; rays aimed at points of edges and at vertices from anywhere (u, v or w
           within rounding of 0), on the mesh's border (one triangle) and inside it (two to six)
  tmin     t_min equal to the closest hit's t (kept: the test is t < t_min), one ulp above it (the next hit wins) and
           one ulp below
  tmax     a finite t_max halfway between the closest and the second hit, equal to the closest hit's t (kept: the test
           is t > t_max) and one ulp below it (then both are out of range)
  sphere   origins inside a sphere (the second root) and on its surface (a root within rounding of 0; t_min 0 and
           1e-3), outward and inward, and rays tangent to a sphere (delta within rounding of 0)
  miss     rays that hit nothing: pointing away, passing outside, or with a t_max in front of the scene
  random   rays from anywhere towards the scene

Each family is 282 rays, shuffled and sent as batches of 5, 13, 64 and 200: rp_intersect's kernel runs one ray per lane,
so the leaf loop's wave-level break (at most PRIM_BREAK = 12 lanes still testing) is taken at once, after a few tests,
and late.  Rays for which brute force finds an exact-t tie between two hittables are compared on t only (which of the
tied hittables a tree returns is free); the families keep them under 2 % of all rays, which the CPU
test checks together with what each family is meant to reach.
"""
import numpy as np
import pytest

from brute import SMOL, Brute

GRID = 30
BATCHES = (5, 13, 64, 200)
N_FAM = sum(BATCHES)
FORMATS = {"f32": 8, "q8": 8, "w8": 4}  # node format: the largest max_leaf it takes


def _scene():
    from rtpotato.scene import (Absorb, Camera, Emit, Hittable, Material, Mesh, Scatter, Scene, SceneData,
                                Transformation, hittables)
    from rtpotato import _ffi as F
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
    rng = np.random.default_rng(0x1eaf)
    small = pos[rng.choice(len(pos), size=12, replace=False)] + rng.uniform(-0.02, 0.02, size=(12, 3))
    parts = [Hittable.Triangle(mesh.iter_triangles(), 0)]
    parts += [Hittable.Sphere(tuple(c), float(r), 1) for c, r in zip(small, rng.uniform(0.04, 0.09, size=12))]
    parts += [Hittable.Sphere((0.31, 0.93, -0.22), 0.35, 1), Hittable.Sphere((-0.52, -0.81, 0.43), 0.5, 1)]
    cam = Camera(1.0, 1.0, 1.0, 0.0, Transformation.lookat((0, 2, 3), (0, 0, 0), (0, 1, 0)))
    return Scene(cam, SceneData(mats, [], [mesh]), hittables(*parts), Emit.SkyGradient, F.RP_ROOT_BVH, "leaf_test_grid")


def _det_row(bf, k):
    """The vector N with det = N . d for triangle k, in brute force's expression (hittable.rs:69-71)."""
    ba, ca = bf.ba[k], bf.ca[k]
    return np.stack([ba[:, 1] * ca[:, 2] - ba[:, 2] * ca[:, 1], ba[:, 2] * ca[:, 0] - ba[:, 0] * ca[:, 2],
                     ba[:, 0] * ca[:, 1] - ba[:, 1] * ca[:, 0]], axis=-1)


def _unit(v):
    return v / np.sqrt((v * v).sum(axis=-1))[..., None]


def _families(scene, bf):
    """name -> (282, 8) rays {o, d, t_min, t_max} and name -> per-ray labels the CPU test reads."""
    rng = np.random.default_rng(0x7e57)
    m = scene.scene_data.mesh_table[0]
    pos = m.positions
    n_tri = len(bf.tri_id)
    fam, lab = {}, {}

    def pack(o, d, tmin=1e-3, tmax=np.inf):
        n = len(o)
        col = lambda v: np.broadcast_to(np.asarray(v, float), (n,)).reshape(n, 1)
        return np.concatenate([o, d, col(tmin), col(tmax)], axis=1)

    def put(name, rays, labels=None):
        rays = np.concatenate(rays) if isinstance(rays, list) else rays
        assert len(rays) == N_FAM, (name, len(rays))
        p = rng.permutation(N_FAM)
        fam[name] = np.ascontiguousarray(rays[p])
        lab[name] = None if labels is None else np.asarray(labels)[p]

    def origins(n):
        o = rng.uniform(-2.0, 2.0, size=(n, 3))
        o[:, 1] = rng.uniform(-1.8, 2.2, size=n)
        return o

    def towards(o):
        return rng.uniform(-0.9, 0.9, size=(len(o), 3)) * np.array([1.0, 0.4, 1.0]) - o

    def inside(k):  # a point well inside triangle k
        b = rng.dirichlet((2.0, 2.0, 2.0), size=len(k))
        A, B, C = bf.A[k], bf.A[k] - bf.ba[k], bf.A[k] - bf.ca[k]
        return b[:, 0:1] * A + b[:, 1:2] * B + b[:, 2:3] * C

    # ---- plane: det = N . d around +-SMOL; the in-plane part of d is a unit vector, the rest is along N
    n = N_FAM - 30
    k = rng.integers(0, n_tri, size=n)
    N = _det_row(bf, k)
    nn = np.sqrt((N * N).sum(axis=1))
    e = _unit(bf.ba[k] * rng.uniform(-1, 1, size=(n, 1)) + bf.ca[k] * rng.uniform(-1, 1, size=(n, 1)))
    want = SMOL * 2.0 ** rng.uniform(-2.0, 2.0, size=n) * rng.choice([-1.0, 1.0], size=n)
    want[:40] = SMOL * (1.0 + rng.uniform(-1e-9, 1e-9, size=40)) * rng.choice([-1.0, 1.0], size=40)
    d = e + (want / nn / nn)[:, None] * N
    P = inside(k)
    plane = pack(P - d * rng.uniform(0.3, 1.5, size=(n, 1)), d)
    k2 = rng.integers(0, n_tri, size=30)  # along an edge: det = 0 up to rounding
    along = pack(bf.A[k2] + 2.0 * bf.ba[k2], -bf.ba[k2])
    put("plane", [plane, along], np.concatenate([k, np.full(30, -1)]))

    # ---- edge: exact zeros of v and u from vertical rays on grid lines, then points of edges and vertices
    g = pos.reshape(GRID + 1, GRID + 1, 3)
    rays = []
    for axis in (2, 0):  # o.z on a line z = z_j (edge A-B of the quad's first triangle: v = +-0); o.x likewise (u)
        n = 60
        line = rng.integers(0, GRID + 1, size=n)
        line[:12] = rng.choice([0, GRID], size=12)  # the mesh's border: one triangle
        o = np.zeros((n, 3))
        o[:, axis] = g[0, line, 2] if axis == 2 else g[line, 0, 0]
        o[:, 2 - axis] = rng.uniform(-1.0, 1.0, size=n)
        step = rng.integers(-1, 2, size=n)  # on the line, or one ulp to either side
        o[:, axis] = np.where(step == 0, o[:, axis], np.nextafter(o[:, axis], np.where(step > 0, np.inf, -np.inf)))
        up = rng.choice([-1.0, 1.0], size=n)
        o[:, 1] = -2.0 * up
        d = np.zeros((n, 3))
        d[:, 1] = up * rng.uniform(0.5, 2.0, size=n)
        rays.append(pack(o, d))
    n = N_FAM - 120
    k = rng.integers(0, n_tri, size=n)
    border = np.nonzero((np.abs(bf.A[:, 2] - g[0, 0, 2]) < 1e-12) & (bf.ba[:, 2] == 0.0))[0]  # first triangles, j = 0
    k[:40] = rng.choice(border, size=40)
    A, B, C = bf.A[k], bf.A[k] - bf.ba[k], bf.A[k] - bf.ca[k]
    s = rng.uniform(0.0, 1.0, size=(n, 1))
    s[40:90] = rng.choice([0.0, 1.0], size=(50, 1))  # vertices
    which = rng.integers(0, 3, size=n)
    which[:40] = 0  # the border edge A-B
    Q = np.where((which == 0)[:, None], A + s * (B - A), np.where((which == 1)[:, None], B + s * (C - B), C + s * (A - C)))
    o = origins(n)
    o[:, 1] = np.abs(o[:, 1]) + 0.6
    rays.append(pack(o, Q - o))
    put("edge", rays)

    # ---- tmin / tmax: around the closest hit's t (a first pass of brute force finds it)
    def hitters(n, grazing):
        while True:
            o = origins(4 * n)
            if grazing:  # from the side, nearly level: several crossings of the surface
                o[:, 0] = -2.0
                o[:, 1] = rng.uniform(-0.2, 0.4, size=4 * n)
                d = np.stack([np.full(4 * n, 4.0), rng.uniform(-0.3, 0.3, size=4 * n), rng.uniform(-1, 1, size=4 * n)], axis=1)
            else:
                d = towards(o)
            r = pack(o, d)
            t1 = bf.closest(r)["t"]
            r2 = r.copy()
            r2[:, 6] = np.nextafter(t1, np.inf)
            t2 = bf.closest(r2)["t"]
            ok = np.isfinite(t1) & (np.isfinite(t2) if grazing else True)
            if ok.sum() >= n:
                return r[ok][:n], t1[ok][:n], t2[ok][:n]

    r, t1, _ = hitters(N_FAM, False)
    case = rng.integers(0, 3, size=N_FAM)
    r[:, 6] = np.where(case == 0, t1, np.where(case == 1, np.nextafter(t1, np.inf), np.nextafter(t1, -np.inf)))
    put("tmin", r, case)
    r, t1, t2 = hitters(N_FAM, True)
    case = rng.integers(0, 3, size=N_FAM)
    case[:150] = 0
    r[:, 7] = np.where(case == 0, 0.5 * (t1 + t2), np.where(case == 1, t1, np.nextafter(t1, -np.inf)))
    put("tmax", r, case)

    # ---- sphere: inside, on the surface, tangent
    sph = [(c, rad) for c, rad, _ in bf.sph]
    # (half of them from the two large spheres, which nothing else touches)
    pick = lambda n: [sph[i] for i in np.where(rng.random(n) < 0.5, rng.integers(12, 14, size=n), rng.integers(0, 12, size=n))]
    rays = []
    n = 100
    cs = pick(n)
    c, rad = np.array([s[0] for s in cs]), np.array([s[1] for s in cs])
    rays.append(pack(c + _unit(rng.normal(size=(n, 3))) * (rad * rng.uniform(0.0, 0.99, size=n))[:, None],
                     rng.normal(size=(n, 3)), tmin=rng.choice([0.0, 1e-3], size=n)))
    cs = pick(n)
    c, rad = np.array([s[0] for s in cs]), np.array([s[1] for s in cs])
    u = _unit(rng.normal(size=(n, 3)))
    d = rng.normal(size=(n, 3))
    d[:30] = u[:30] * rng.uniform(0.5, 2.0, size=(30, 1))    # straight out
    d[30:60] = -u[30:60] * rng.uniform(0.5, 2.0, size=(30, 1))  # straight through the centre
    rays.append(pack(c + u * rad[:, None], d, tmin=rng.choice([0.0, 1e-3], size=n)))
    n = N_FAM - 200
    cs = pick(n)
    c, rad = np.array([s[0] for s in cs]), np.array([s[1] for s in cs])
    u = _unit(rng.normal(size=(n, 3)))
    w = _unit(np.cross(u, rng.normal(size=(n, 3))))  # tangent at c + rad u
    rays.append(pack(c + u * rad[:, None] - w * rng.uniform(0.5, 3.0, size=(n, 1)), w * rng.uniform(0.5, 2.0, size=(n, 1))))
    put("sphere", rays)

    # ---- miss
    rays = []
    o = origins(100)
    o[:, 1] = rng.uniform(1.6, 2.5, size=100)
    d = rng.normal(size=(100, 3))
    d[:, 1] = np.abs(d[:, 1]) + 0.05
    rays.append(pack(o, d))                                    # above everything, going up
    o = origins(100)
    o[:, 0] = rng.uniform(1.2, 2.0, size=100)
    d = rng.normal(size=(100, 3))
    d[:, 0] = np.abs(d[:, 0]) + 0.05
    d[:, 1] = 0.2 * d[:, 1]
    rays.append(pack(o, d))                                    # beside everything, going away
    o = origins(N_FAM - 200)
    o[:, 1] = 2.2
    rays.append(pack(o, towards(o), tmax=rng.uniform(1e-3, 0.5, size=len(o))))  # t_max in front of the scene
    put("miss", rays)

    o = origins(N_FAM)
    put("random", pack(o, towards(o)))
    return fam, lab


def _records(bf, rays, ref):
    """The reference's Hit records (t, position, normal, uv) and materials of brute force's closest hits, in the
    reference's expression order (tests/brute.py Brute.records)."""
    rec, mats, is_tri = bf.records(rays, ref)
    hit = ref["id"] >= 0
    return {"rec": rec, "mats": mats, "hit": hit, "tri": is_tri, "tie": ref["tie"].copy()}


@pytest.fixture(scope="module")
def reference():
    """(scene, brute force, family -> rays, labels, records): made once, read-only."""
    scene = _scene()
    bf = Brute(scene)
    fam, lab = _families(scene, bf)
    out = {}
    for name, rays in fam.items():
        ref = bf.closest(rays)
        rec = _records(bf, rays, ref)
        rec["id"], rec["u"], rec["v"] = ref["id"], ref["u"], ref["v"]
        for a in rec.values():
            a.setflags(write=False)
        rays.setflags(write=False)
        out[name] = (rays, lab[name], rec)
    return scene, bf, out


def test_families_reach_what_they_aim_at(reference):
    """CPU only: brute force's own view of the families.  Exact-t ties stay under 2 % of all rays; each family has the
    cases it is named for, on both sides of the comparison it is aimed at."""
    scene, bf, fams = reference
    assert len(scene.root) <= 2014 and len(bf.sph) == 14
    assert set(fams) == {"plane", "edge", "tmin", "tmax", "sphere", "miss", "random"}
    ties = sum(int(r["tie"].sum()) for _, _, r in fams.values())
    total = sum(len(rays) for rays, _, _ in fams.values())
    print("ties", {k: int(r["tie"].sum()) for k, (_, _, r) in fams.items()}, "of", total)
    assert ties < 0.02 * total, (ties, total)

    rays, k, r = fams["plane"]
    aimed = k >= 0
    det = (_det_row(bf, np.where(aimed, k, 0)) * rays[:, 3:6]).sum(axis=1)
    below, above = aimed & (np.abs(det) < SMOL), aimed & (np.abs(det) > SMOL)
    assert below.sum() > 60 and above.sum() > 60 and (det[aimed] > 0).sum() > 60 and (det[aimed] < 0).sum() > 60
    near = aimed & (np.abs(np.abs(det) / SMOL - 1.0) < 1e-6)
    assert (near & below).sum() > 5 and (near & above).sum() > 5
    took = r["id"] == bf.tri_id[np.where(aimed, k, 0)]  # the aimed-at triangle is the closest hit
    assert (took & above).sum() > 30 and not (took & below).any()

    _, _, r = fams["edge"]
    on = r["tri"] & ((r["u"] == 0.0) | (r["v"] == 0.0))
    w = 1.0 - r["u"] - r["v"]
    close = r["tri"] & (np.minimum(np.minimum(np.abs(r["u"]), np.abs(r["v"])), np.abs(w)) < 1e-12)
    assert on.sum() > 20 and close.sum() > 100 and (~r["hit"]).sum() + (~close & r["hit"]).sum() > 20

    _, case, r = fams["tmin"]
    assert all((case == c).sum() > 60 for c in range(3)) and r["hit"][case != 1].all()
    rays, case, r = fams["tmax"]
    assert r["hit"][case < 2].all() and not r["hit"][case == 2].any() and (case == 1).sum() > 30
    assert (r["rec"][case == 1, 0] == rays[case == 1, 7]).all()

    rays, _, r = fams["sphere"]
    sp = r["hit"] & ~r["tri"]
    c = np.array([bf.sph[i][0] for i in np.searchsorted(bf.sph_id, np.where(sp, r["id"], bf.sph_id[0]))])
    rad = np.array([bf.sph[i][1] for i in np.searchsorted(bf.sph_id, np.where(sp, r["id"], bf.sph_id[0]))])
    from_inside = sp & (np.sqrt(((rays[:, 0:3] - c) ** 2).sum(axis=1)) < rad * (1.0 - 1e-9))
    assert sp.sum() > 150 and from_inside.sum() > 60 and (~r["hit"]).sum() > 10

    assert not fams["miss"][2]["hit"].any()
    _, _, r = fams["random"]
    assert r["hit"].sum() > 100 and (~r["hit"]).sum() > 20


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_leaf_tests_equal_brute_force(gpu, reference, fmt):
    scene, _, fams = reference
    checked = 0
    with gpu.DeviceScene(scene, options={"builder": "host", "node_format": fmt, "max_leaf": FORMATS[fmt],
                                         "always_max": 0}) as ds:
        for name, (rays, _, ref) in fams.items():
            start = 0
            for n in BATCHES:
                s = slice(start, start + n)
                start += n
                hits, mats = ds.intersect(rays[s])  # raises on a stack-overflow status
                where = (fmt, name, n)
                hit, tie, tri, rec = ref["hit"][s], ref["tie"][s], ref["tri"][s], ref["rec"][s]
                assert np.array_equal(np.isfinite(hits[:, 0]), hit), where
                assert np.array_equal(hits[:, 0], rec[:, 0]), (where, np.nonzero(hits[:, 0] != rec[:, 0])[0][:10])
                u = ~tie
                assert np.array_equal(mats[u], ref["mats"][s][u]), where
                bad = np.nonzero(u & (hits[:, 1:7] != rec[:, 1:7]).any(axis=1))[0]
                assert len(bad) == 0, (where, bad[:10])
                t = u & tri
                assert np.array_equal(hits[t, 7:9], rec[t, 7:9]), where
                sp = u & hit & ~tri
                if sp.any():
                    assert np.max(np.abs(hits[sp, 7:9] - rec[sp, 7:9])) < 1e-12, where
                checked += n
            assert start == N_FAM
    assert checked == 7 * N_FAM
