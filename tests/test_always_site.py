"""The scenes and ray families of tests/test_gpu_always_site.py, seen by brute force and the host builder (CPU only).

The always-tested site of the kernels (rp_device.h always_tests: the list's records through scalar loads, a sphere's
test with its constants in scalar operands, anything else through prim_test) is reached through the renderer's own
trees: the host builder with the minor rule on (rp_bvh.h BuildOptions::always_minor), over a 6 x 6 grid of quads (72
triangles, above the 16 the rule asks for).  The scenes and what the builder lists for them:

  none      the grid alone                                  an empty list
  ground    + the ground (r = 1000)                         one entry, by the size rule
  c3        + the ground and two balls                      three entries, config C3's shape
  cap       + the ground and three balls                    four entries, the cap
  past_cap  + the ground and four balls                     past the cap: the ground alone, four spheres in leaves
  mixed     + a huge triangle under the grid and one ball   the triangle (size rule), then the ball
  mixed2    a ball, the grid, the huge triangle, a ball     sphere, triangle, sphere in list order

and the families, 282 rays each, aimed at the scene's spheres (`targets`: the listed ones, and past_cap's four in
leaves):

  inside    origins inside a sphere, any direction, t_min 0 and 1e-3: the second root is taken
  surface   origins on a sphere's surface, t_min 0 and 1e-3, straight out, straight through the centre, anywhere
  tangent   rays tangent to a sphere: delta within rounding of 0, on both sides
  behind    a sphere behind the ray
  order     rays through two spheres, the nearer one later in the list than the farther one, and the reverse
  tmax      a finite t_max halfway between the two closest roots, equal to the closest (kept) and one ulp below it
  mesh      a mesh triangle in front of a listed primitive, and behind one
  miss      rays that hit nothing

A scene without spheres has mesh and miss only.  This module checks that each scene's list has the intended length and
kinds in the three node formats, that each family reaches what it is aimed at, and that exact-t ties (compared on t
alone on the GPU: which of two tied hittables a tree returns is free) stay under 2 % of a family.
"""
import ctypes
import functools

import numpy as np
import pytest

from brute import Brute

GRID = 6
BATCHES = (5, 13, 64, 200)
N_FAM = sum(BATCHES)
F32, Q8, W8 = 1, 2, 3  # RP_NODES_*
GROUND = ((0.0, -1000.5, 0.0), 1000.0)  # its top at y = -0.5, under the grid
BALLS = [((-0.45, 0.95, 0.1), 0.35), ((0.4, 1.0, -0.15), 0.3), ((0.05, 1.7, 0.3), 0.25), ((0.1, 0.9, 0.8), 0.2)]
HUGE = np.array([[-60.0, -0.9, -50.0], [60.0, -1.1, -50.0], [0.0, -0.7, 70.0]])
# scene -> (n_always, spheres on the list, triangles on it, spheres left inside the tree)
LISTS = {"none": (0, 0, 0, 0), "ground": (1, 1, 0, 0), "c3": (3, 3, 0, 0), "cap": (4, 4, 0, 0), "past_cap": (1, 1, 0, 4),
         "mixed": (2, 1, 1, 0), "mixed2": (3, 2, 1, 0)}


def _unit(v):
    return v / np.sqrt((v * v).sum(axis=-1))[..., None]


def _grid_mesh():
    from rtpotato.scene import Mesh
    g = np.linspace(-1.0, 1.0, GRID + 1) * 1.0371  # not f32 values
    x, z = np.meshgrid(g, g, indexing="ij")
    y = 0.3 * np.sin(3.0 * x) * np.cos(2.0 * z) + 0.1
    pos = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    nrm = _unit(np.stack([-0.9 * np.cos(3.0 * x), np.ones_like(x), 0.6 * np.sin(2.0 * z)], axis=-1).reshape(-1, 3))
    uv = np.stack([(x + 1.1) / 2.2, (z + 1.1) / 2.2], axis=-1).reshape(-1, 2)
    i, j = np.meshgrid(np.arange(GRID), np.arange(GRID), indexing="ij")
    v00 = (i * (GRID + 1) + j).reshape(-1)
    v01, v10, v11 = v00 + 1, v00 + GRID + 1, v00 + GRID + 2
    idx = np.stack([v00, v10, v11, v00, v11, v01], axis=-1).reshape(-1).astype(np.uint32)
    return Mesh(pos, nrm, uv, idx, material=0)


def _make_scene(parts, meshes, name):
    from rtpotato.scene import Absorb, Camera, Emit, Material, Scatter, Scene, SceneData, Transformation, hittables
    from rtpotato import _ffi as F
    mats = [Material.new(Scatter.Lambert, Absorb.Albedo((0.7, 0.7, 0.7)), Emit.None_),
            Material.new(Scatter.Metal(0.1), Absorb.Albedo((0.8, 0.6, 0.2)), Emit.None_),
            Material.new(Scatter.Lambert, Absorb.Albedo((0.2, 0.6, 0.3)), Emit.None_)]
    cam = Camera(1.0, 1.0, 1.0, 0.0, Transformation.lookat((0, 2, 3), (0, 0, 0), (0, 1, 0)))
    return Scene(cam, SceneData(mats, [], meshes), hittables(*parts), Emit.SkyGradient, F.RP_ROOT_BVH, name)


def _scene(name):
    """(scene, targets): targets = [(centre, radius)] of the spheres the families aim at, in hittable (= list) order."""
    from rtpotato.scene import Hittable, Mesh
    grid = _grid_mesh()
    tris = Hittable.Triangle(grid.iter_triangles(), 0)
    sph = lambda cr, mat: Hittable.Sphere(cr[0], cr[1], mat)
    huge_mesh = Mesh(HUGE, np.tile([0.0, 1.0, 0.0], (3, 1)), np.array([[0.0, 0.0], [1.0, 0.0], [0.5, 1.0]]),
                     np.arange(3, dtype=np.uint32), material=2)
    huge = Hittable.Triangle(huge_mesh.iter_triangles(), 1)
    if name == "none":
        return _make_scene([tris], [grid], name), []
    if name in ("ground", "c3", "cap", "past_cap"):
        n = {"ground": 0, "c3": 2, "cap": 3, "past_cap": 4}[name]
        t = [GROUND] + BALLS[:n]
        return _make_scene([tris, sph(GROUND, 2)] + [sph(b, 1) for b in BALLS[:n]], [grid], name), t
    if name == "mixed":  # the triangle in front of the ball in list order
        return _make_scene([tris, huge, sph(BALLS[0], 1)], [grid, huge_mesh], name), [BALLS[0]]
    if name == "mixed2":
        return _make_scene([sph(BALLS[1], 1), tris, huge, sph(BALLS[0], 1)], [grid, huge_mesh], name), [BALLS[1], BALLS[0]]
    raise KeyError(name)


def _one_sphere(cr):
    """Brute force over that sphere alone: what its own test answers a ray."""
    from rtpotato.scene import Hittable
    return Brute(_make_scene([Hittable.Sphere(cr[0], cr[1], 0)], [], "one"))


def _pack(o, d, tmin=1e-3, tmax=np.inf):
    n = len(o)
    col = lambda v: np.broadcast_to(np.asarray(v, float), (n,)).reshape(n, 1)
    return np.concatenate([o, d, col(tmin), col(tmax)], axis=1)


def _delta(rays, c, rad):
    """The sphere test's discriminant in its expression order (rp_isect.h sphere_test), to classify the tangent rays."""
    o, d = rays[:, 0:3], rays[:, 3:6]
    tc = o - np.asarray(c)[None]
    a = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    hb = (d[:, 0] * tc[:, 0] + d[:, 1] * tc[:, 1]) + d[:, 2] * tc[:, 2]
    cq = ((tc[:, 0] * tc[:, 0] + tc[:, 1] * tc[:, 1]) + tc[:, 2] * tc[:, 2]) - rad * rad
    return hb * hb - a * cq, a


def _families(name, bf, targets, seed):
    """family -> (282, 8) rays {o, d, t_min, t_max}, family -> per-ray labels (what the CPU test reads)."""
    rng = np.random.default_rng(seed)
    fam, lab = {}, {}
    C = np.array([t[0] for t in targets]).reshape(-1, 3)
    R = np.array([t[1] for t in targets])

    def put(fname, rays, labels=None):
        rays = np.concatenate(rays) if isinstance(rays, list) else rays
        assert len(rays) == N_FAM, (fname, len(rays))
        p = rng.permutation(N_FAM)
        fam[fname] = np.ascontiguousarray(rays[p])
        lab[fname] = None if labels is None else np.asarray(labels)[p]

    def pick(n):
        return rng.integers(0, len(targets), size=n)

    def out_dir(k):
        """Unit vectors from the centres of spheres k: anywhere for a ball, within 2 mrad of straight up for the
        ground (points of it under the scene)."""
        u = _unit(rng.normal(size=(len(k), 3)))
        up = _unit(np.array([0.0, 1.0, 0.0]) + rng.uniform(-2e-3, 2e-3, size=(len(k), 3)) * np.array([1.0, 0.0, 1.0]))
        return np.where((R[k] > 100.0)[:, None], up, u)

    def above(n):
        return np.stack([rng.uniform(-1.5, 1.5, size=n), rng.uniform(2.0, 3.0, size=n), rng.uniform(-1.5, 1.5, size=n)], axis=1)

    def at_grid(n):
        return np.stack([rng.uniform(-0.9, 0.9, size=n), np.full(n, 0.1), rng.uniform(-0.9, 0.9, size=n)], axis=1)

    # ---- mesh: from above through the balls and the grid to whatever lies under it; from under the grid upwards; from
    # inside the ground upwards (the ground's far root in front of the grid)
    o1 = above(120)
    d1 = at_grid(120) - o1
    balls = np.nonzero(R < 100.0)[0]
    if len(balls):  # half of them from over a ball, through it
        b = rng.choice(balls, size=60)
        o1[:60] = C[b] + np.stack([rng.uniform(-0.3, 0.3, size=60), rng.uniform(1.0, 2.0, size=60), rng.uniform(-0.3, 0.3, size=60)], axis=1)
        d1[:60] = C[b] + rng.normal(size=(60, 3)) * 0.3 * R[b][:, None] - o1[:60]
    r1 = _pack(o1, d1)
    o2 = np.stack([rng.uniform(-0.9, 0.9, size=100), np.full(100, -0.4), rng.uniform(-0.9, 0.9, size=100)], axis=1)
    aim = (C[pick(100)] if len(targets) else at_grid(100) + np.array([0.0, 1.0, 0.0])) + rng.uniform(-0.3, 0.3, size=(100, 3))
    aim[:, 1] = np.maximum(aim[:, 1], 0.5)
    r2 = _pack(o2, aim - o2)
    o3 = np.stack([rng.uniform(-0.8, 0.8, size=62), rng.uniform(-0.9, -0.6, size=62), rng.uniform(-0.8, 0.8, size=62)], axis=1)
    r3 = _pack(o3, at_grid(62) + np.array([0.0, 1.0, 0.0]) - o3)
    put("mesh", [r1, r2, r3])

    # ---- miss: above everything going up, beside everything going up and away, a t_max in front of the scene
    o = above(100)
    o[:, 1] += 0.4
    d = rng.normal(size=(100, 3))
    d[:, 1] = np.abs(d[:, 1]) + 0.05
    m1 = _pack(o, d)
    o = above(100)
    o[:, 0] = rng.uniform(1.2, 2.0, size=100)
    d = rng.normal(size=(100, 3))
    d[:, 0] = np.abs(d[:, 0]) + 0.05
    d[:, 1] = np.abs(d[:, 1]) * 0.2 + 0.01
    m2 = _pack(o, d)
    o = above(N_FAM - 200)
    o[:, 1] = 2.3
    m3 = _pack(o, _unit(at_grid(len(o)) - o), tmax=rng.uniform(1e-3, 0.3, size=len(o)))
    put("miss", [m1, m2, m3])
    if not targets:
        return fam, lab

    # ---- inside: the second root
    k = pick(N_FAM)
    depth = np.where(R[k] > 100.0, rng.uniform(0.9985, 0.99999, size=N_FAM), rng.uniform(0.0, 0.99, size=N_FAM))
    o = C[k] + out_dir(k) * (R[k] * depth)[:, None]
    put("inside", _pack(o, rng.normal(size=(N_FAM, 3)), tmin=rng.choice([0.0, 1e-3], size=N_FAM)), k)

    # ---- surface: a root within rounding of 0
    k = pick(N_FAM)
    u = out_dir(k)
    d = rng.normal(size=(N_FAM, 3))
    d[:90] = u[:90] * rng.uniform(0.5, 2.0, size=(90, 1))          # straight out
    d[90:180] = -u[90:180] * rng.uniform(0.5, 2.0, size=(90, 1))   # straight through the centre
    put("surface", _pack(C[k] + u * R[k][:, None], d, tmin=rng.choice([0.0, 1e-3], size=N_FAM)), k)

    # ---- tangent: delta within rounding of 0
    k = pick(N_FAM)
    u = out_dir(k)
    w = _unit(np.cross(u, rng.normal(size=(N_FAM, 3))))  # tangent at c + rad u
    put("tangent", _pack(C[k] + u * R[k][:, None] - w * rng.uniform(0.5, 3.0, size=(N_FAM, 1)),
                         w * rng.uniform(0.5, 2.0, size=(N_FAM, 1))), k)

    # ---- behind: the origin outside, the direction away from the centre
    k = pick(N_FAM)
    u = out_dir(k)
    o = C[k] + u * (R[k] + rng.uniform(0.05, 1.5, size=N_FAM) * np.minimum(R[k], 1.0))[:, None]
    put("behind", _pack(o, u * rng.uniform(0.5, 2.0, size=(N_FAM, 1)) + rng.normal(size=(N_FAM, 3)) * 0.2), k)

    # ---- order: through sphere i, then sphere j, i < j and i > j alike (one target: through it from anywhere)
    def through(n):
        i = pick(n)
        j = (i + rng.integers(1, max(len(targets), 2), size=n)) % len(targets)
        if len(targets) == 1:
            axis = _unit(rng.normal(size=(n, 3)))
            axis[:, 1] = -np.abs(axis[:, 1]) - 0.2  # from above
            axis = _unit(axis)
            aim = C[i] + rng.normal(size=(n, 3)) * 0.3 * R[i][:, None]
        else:
            axis = _unit(C[j] - C[i])
            aim = C[j] + rng.normal(size=(n, 3)) * 0.3 * np.minimum(R[j], 1.0)[:, None]
        o = C[i] - axis * (R[i] + rng.uniform(0.1, 1.0, size=n))[:, None] + rng.normal(size=(n, 3)) * 0.1 * np.minimum(R[i], 1.0)[:, None]
        return _pack(o, _unit(aim - o) * rng.uniform(0.5, 2.0, size=(n, 1))), np.stack([i, j], axis=1)

    rays, ij = through(N_FAM)
    put("order", rays, ij)

    # ---- tmax: around the closest root (a first pass of brute force finds it and the next one)
    while True:
        r, _ = through(4 * N_FAM)
        t1 = bf.closest(r)["t"]
        r2 = r.copy()
        r2[:, 6] = np.nextafter(t1, np.inf)
        t2 = bf.closest(r2)["t"]
        ok = np.isfinite(t1) & np.isfinite(t2)
        if ok.sum() >= N_FAM:
            r, t1, t2 = r[ok][:N_FAM], t1[ok][:N_FAM], t2[ok][:N_FAM]
            break
    case = rng.integers(0, 3, size=N_FAM)
    r[:, 7] = np.where(case == 0, 0.5 * (t1 + t2), np.where(case == 1, t1, np.nextafter(t1, -np.inf)))
    put("tmax", r, case)
    return fam, lab


SEEDS = {"none": 0xa110, "ground": 0xa111, "c3": 0xa112, "cap": 0xa113, "past_cap": 0xa114, "mixed": 0xa115,
         "mixed2": 0xa116}


@functools.lru_cache(maxsize=None)
def always_reference():
    """scene name -> (scene, targets, brute force, family -> (rays, labels, records)): made once per process,
    read-only; tests/test_gpu_always_site.py reads the same object."""
    out = {}
    for name in LISTS:
        scene, targets = _scene(name)
        bf = Brute(scene)
        fam, lab = _families(name, bf, targets, SEEDS[name])
        fams = {}
        for fname, rays in fam.items():
            ref = bf.closest(rays)
            rec, mats, is_tri = bf.records(rays, ref)
            r = {"rec": rec, "mats": mats, "hit": ref["id"] >= 0, "tri": is_tri, "tie": ref["tie"].copy(), "id": ref["id"]}
            for a in r.values():
                a.setflags(write=False)
            rays.setflags(write=False)
            fams[fname] = (rays, lab[fname], r)
        out[name] = (scene, targets, bf, fams)
    return out


@pytest.fixture(scope="module")
def reference():
    return always_reference()


@pytest.mark.parametrize("fmt", [F32, Q8, W8])
@pytest.mark.parametrize("name", list(LISTS))
def test_lists_have_the_intended_length_and_kinds(reference, name, fmt):
    """rph_bvh_selfcheck_opt with the renderer's options (always_max its default, the minor rule on): the list's length,
    and its kinds from the non-triangle primitives left inside the tree (every sphere is on the list or in a leaf)."""
    from rtpotato import _ffi as F
    scene, _, bf, _ = reference[name]
    st = (ctypes.c_uint64 * 6)()
    rc = F.host().rph_bvh_selfcheck_opt(scene.desc().ptr(), fmt, F.RP_COLLAPSE_AUTO, -1, 1, st)
    assert rc == 0, (F.host().rph_last_error() or b"").decode()
    n_always, inside = int(st[4]), int(st[5])
    spheres = len(bf.sph) - inside
    assert (n_always, spheres, n_always - spheres, inside) == LISTS[name]
    assert int(st[3]) == len(scene.root) and len(bf.tri_id) >= 72


@pytest.mark.parametrize("name", list(LISTS))
def test_families_reach_what_they_aim_at(reference, name):
    scene, targets, bf, fams = reference[name]
    assert set(fams) == ({"mesh", "miss"} if not targets else
                         {"mesh", "miss", "inside", "surface", "tangent", "behind", "order", "tmax"})
    for fname, (rays, _, r) in fams.items():
        ties = int(r["tie"].sum())
        print(name, fname, "ties", ties, "hits", int(r["hit"].sum()), "on triangles", int(r["tri"].sum()))
        assert len(rays) == N_FAM and ties <= 0.02 * N_FAM, (name, fname, ties)
    assert not fams["miss"][2]["hit"].any()

    # mesh: a grid triangle in front of a listed primitive (the next hit behind it), and behind one (the closest hit is
    # listed, and the grid alone is hit as well)
    rays, _, r = fams["mesh"]
    assert r["tri"].sum() > 60
    sph_ids = bf.sph_id
    if name != "none":
        nxt = np.array(rays)
        nxt[:, 6] = np.where(r["hit"], np.nextafter(r["rec"][:, 0], np.inf), np.inf)
        second = bf.closest(nxt)
        listed = set(int(i) for i in sph_ids[:1 if name == "past_cap" else len(sph_ids)])
        if name.startswith("mixed"):
            listed.add(int(bf.tri_id[-1]))  # the huge triangle
        on_list = lambda ids: np.isin(ids, list(listed))
        mesh_tri = lambda ids: np.isin(ids, bf.tri_id[:72])
        tri_first = mesh_tri(r["id"]) & on_list(second["id"])
        listed_first = on_list(r["id"]) & np.isfinite(reference["none"][2].closest(rays)["t"])  # the grid alone is hit
        print(name, "mesh: triangle in front of a listed primitive", int(tri_first.sum()), "behind one", int(listed_first.sum()))
        assert tri_first.sum() > 30 and listed_first.sum() > 30
    if not targets:
        return
    C = np.array([t[0] for t in targets])
    R = np.array([t[1] for t in targets])
    one = [_one_sphere(t) for t in targets]
    tid = [int(i) for i in sph_ids]  # root index of each target: both in hittable order
    assert len(tid) == len(targets)

    def own(rays, k):  # each ray's t against the sphere it was aimed at, alone
        t = np.full(len(rays), np.inf)
        for q in range(len(targets)):
            m = k == q
            if m.any():
                t[m] = one[q].closest(rays[m])["t"]
        return t

    # inside: the origin strictly inside, so the first root is negative and the accepted one is the second
    rays, k, r = fams["inside"]
    dist = np.sqrt(((rays[:, 0:3] - C[k]) ** 2).sum(axis=1))
    assert (dist < R[k] * (1.0 - 1e-9)).all()
    t_own = own(rays, k)
    assert np.isfinite(t_own).all() and (t_own > 0.0).all()
    took = r["id"] == np.array(tid)[k]
    assert took.sum() > 150 and (r["rec"][took, 0] == t_own[took]).all()
    assert all((took & (k == q)).sum() > 10 for q in range(len(targets)))

    # surface: roots within rounding of 0 at t_min 0 (kept when they round to >= 0), the far root for rays going in
    rays, k, r = fams["surface"]
    t_own = own(rays, k)
    tiny = np.isfinite(t_own) & (np.abs(t_own) < 1e-6 * np.minimum(R[k], 1.0))
    far = np.isfinite(t_own) & (t_own > 1e-3)
    assert (rays[:, 6] == 0.0).sum() > 60 and (rays[:, 6] == 1e-3).sum() > 60
    assert tiny.sum() > 10 and far.sum() > 60 and (~np.isfinite(t_own)).sum() > 10
    assert not tiny[rays[:, 6] == 1e-3].any()

    # tangent: delta on both sides of 0, within rounding of it
    rays, k, r = fams["tangent"]
    delta = np.empty(N_FAM)
    a = np.empty(N_FAM)
    for q in range(len(targets)):
        m = k == q
        if m.any():
            delta[m], a[m] = _delta(rays[m], C[q], R[q])
    assert (np.abs(delta) <= 1e-9 * a * R[k] * R[k]).all()
    assert (delta > 0.0).sum() > 40 and (delta <= 0.0).sum() > 40
    t_own = own(rays, k)
    assert not (np.isfinite(t_own) & ~(delta > 0.0)).any()

    # behind: the aimed-at sphere's own test rejects every ray
    rays, k, r = fams["behind"]
    assert not np.isfinite(own(rays, k)).any()

    # order: both spheres' own tests accept, the nearer one later in the list and earlier in it
    rays, ij, r = fams["order"]
    if len(targets) > 1:
        ti, tj = own(rays, ij[:, 0]), own(rays, ij[:, 1])
        both = np.isfinite(ti) & np.isfinite(tj)
        near_later = both & (np.where(ti < tj, ij[:, 0], ij[:, 1]) > np.where(ti < tj, ij[:, 1], ij[:, 0]))
        near_earlier = both & ~near_later
        print(name, "order: both hit", int(both.sum()), "nearer later in the list", int(near_later.sum()),
              "nearer earlier", int(near_earlier.sum()))
        assert near_later.sum() > 30 and near_earlier.sum() > 30
    else:
        assert np.isfinite(own(rays, ij[:, 0])).sum() > 150

    # tmax: halfway (hit), equal to the closest root (kept), one ulp below it (nothing left in range)
    rays, case, r = fams["tmax"]
    assert all((case == c).sum() > 60 for c in range(3))
    assert r["hit"][case < 2].all() and not r["hit"][case == 2].any()
    assert (r["rec"][case == 1, 0] == rays[case == 1, 7]).all()
    assert (~r["tri"][case < 2]).sum() > 60  # roots of spheres among them
