"""CPU: the per-primitive normals table (rp_layout.h TriNormals; hook rph_tri_normals).

The render kernel's shading reads a triangle hit's three vertex normals from the primitive's own 72 B record instead of
going through the PrimRef's vertex ids to the vertex table, so the table must hold, for every primitive k of the tree
in leaf order, exactly the doubles normals[ids[k]] -- copied, never recomputed: compared here as uint64 views.  The
ids are checked on their own against the scene (mesh base + the mesh's indices of the source hittable), so the two
halves of the old path and the new record are tied together from both ends.  Inputs: the bunny fixture; two meshes
(the second one's vertex base is not 0); a mesh whose triangles share vertices; spheres and triangles mixed (a sphere's
entry is unread, the triangles' are exact), under the renderer's tree options too (always-tested spheres sit behind
the tree's primitives).

PrimRef and the tree are not touched by the table: the tree hashes (nodes and prim_refs, rph_bvh_tree_hash_opt) of the
pinned trees below are the values of the commit before the table existed.
"""
import ctypes

import numpy as np
import pytest

import shading_scenes as S
from rtpotato import _ffi as F
from rtpotato import scenes
from rtpotato.scene import Absorb, Emit, Hittable, Material, Mesh, Scatter, Scene, SceneData, hittables, rgb

F32, Q8, W8 = 1, 2, 3  # RP_NODES_*
DEFAULT, RENDERER = (-1, 0), (4, 1)  # (always_max, always_minor): the hooks' default tree, the tree librp.so builds


def _table(sc: Scene, fmt: int, opts):
    d = sc.desc()
    n = ctypes.c_uint64(0)
    F.check_host(F.host().rph_tri_normals(d.ptr(), fmt, opts[0], opts[1], 0, None, None, None, ctypes.byref(n)))
    assert n.value == len(sc.root)
    nrm = np.full((n.value, 9), np.nan)
    refs = np.full((n.value, 4), 0xFFFFFFFF, dtype=np.uint32)
    kinds = np.full(n.value, 7, dtype=np.uint32)
    F.check_host(F.host().rph_tri_normals(d.ptr(), fmt, opts[0], opts[1], n.value, nrm.ctypes.data, refs.ctypes.data,
                                          kinds.ctypes.data, ctypes.byref(n)))
    return nrm, refs, kinds


def _expected(sc: Scene, refs: np.ndarray):
    """From the scene alone: (ids (n, 3) as the builder must number them, is_triangle (n,), the concatenated normals)."""
    table = sc.scene_data.mesh_table
    vbase = np.concatenate([[0], np.cumsum([len(m.positions) for m in table])]).astype(np.int64)
    allnrm = np.concatenate([np.ascontiguousarray(m.normals, dtype=np.float64) for m in table]) if table else np.zeros((0, 3))
    rows = sc.root[refs[:, 3]]  # the source hittables, in leaf order
    tri = rows["kind"] == F.RP_HITTABLE_TRIANGLE
    ids = np.zeros((len(rows), 3), dtype=np.int64)
    for k in np.flatnonzero(tri):
        m, t = int(rows["mesh"][k]), int(rows["triangle"][k])
        ids[k] = vbase[m] + table[m].indices[t:t + 3].astype(np.int64)
    return ids, tri, allnrm


def _check(sc: Scene, fmt: int, opts):
    nrm, refs, kinds = _table(sc, fmt, opts)
    assert sorted(refs[:, 3].tolist()) == list(range(len(sc.root)))  # every hittable once
    ids, tri, allnrm = _expected(sc, refs)
    assert np.array_equal(kinds == 1, tri) and np.array_equal(kinds == 0, ~tri)
    assert np.array_equal(refs[tri, :3].astype(np.int64), ids[tri])
    got = nrm[tri].reshape(-1, 3, 3).view(np.uint64)
    want = np.ascontiguousarray(allnrm[refs[tri, :3].astype(np.int64)]).view(np.uint64)  # normals[ids[k]]
    assert got.shape == want.shape and np.array_equal(got, want)
    return nrm, refs, tri


def two_meshes() -> Scene:
    """A quad (4 shared vertices) and the smooth fan (6 vertices, hub shared by five triangles): the fan's ids start
    at 4.  Its normals carry a NaN payload and a negative zero, which only a copy keeps."""
    quad, fan = S._quad_mesh(0), S._fan_mesh(0)
    nrm = fan.normals.copy()
    nrm[2, 1] = -0.0
    nrm.view(np.uint64)[4, 0] = 0x7FF8_0000_DEAD_BEEF
    fan = Mesh(fan.positions, nrm, fan.uvs, fan.indices, 0)
    mats = [Material.new(Scatter.Lambert, Absorb.Albedo(rgb(0.5, 0.5, 0.5)), Emit.None_)]
    return Scene(S._cam(1.0, 1.0, 0.0, (0.1, 1.7, 4.2), (0.05, 0.55, 0.0)), SceneData(mats, [], [quad, fan]),
                 S._interleave([quad, fan]), Emit.SkyGradient, F.RP_ROOT_BVH, "two_meshes")


def shared_vertices() -> Scene:
    """A 9 x 9 grid of vertices under 128 triangles: inner vertices belong to six triangles each; every vertex has a
    normal of its own."""
    g = 9
    x, z = np.meshgrid(np.linspace(-1, 1, g), np.linspace(-1, 1, g))
    pos = np.stack([x.ravel(), 0.1 * np.sin(3 * x.ravel()) * np.cos(2 * z.ravel()), z.ravel()], axis=1)
    nrm = S._unit(np.random.default_rng(5).normal(size=(g * g, 3)) + [0.0, 3.0, 0.0])
    idx = []
    for j in range(g - 1):
        for i in range(g - 1):
            a = j * g + i
            idx += [a, a + 1, a + g, a + 1, a + g + 1, a + g]
    mesh = Mesh(pos, nrm, np.zeros((g * g, 2)), np.array(idx, dtype=np.uint32), 0)
    mats = [Material.new(Scatter.Lambert, Absorb.Albedo(rgb(0.5, 0.5, 0.5)), Emit.None_)]
    return Scene(S._cam(1.0, 1.0, 0.0, (0.0, 2.0, 3.0), (0.0, 0.0, 0.0)), SceneData(mats, [], [mesh]),
                 Hittable.Triangle(mesh.iter_triangles(), 0), Emit.SkyGradient, F.RP_ROOT_BVH, "shared_vertices")


def mixed() -> Scene:
    """The shared-vertex grid among 40 small spheres, and one big one: spheres inside leaves, in front of triangles."""
    sc = shared_vertices()
    rng = np.random.default_rng(9)
    balls = [Hittable.Sphere(tuple(rng.uniform(-1, 1, 3) * [1.0, 0.2, 1.0]), 0.03, 0) for _ in range(40)]
    rows = [sc.root[i:i + 1] for i in range(len(sc.root))]
    for k, b in enumerate(balls):
        rows.insert(3 * k, b)
    root = hittables(*rows, Hittable.Sphere((0.0, -500.0, 0.0), 499.5, 0))
    return Scene(sc.camera, sc.scene_data, root, sc.background, F.RP_ROOT_BVH, "mixed")


SCENES = {"bunny_full": scenes.bunny_full, "two_meshes": two_meshes, "shared_vertices": shared_vertices, "mixed": mixed,
          "meshes": S.meshes}


@pytest.mark.parametrize("opts", [DEFAULT, RENDERER], ids=["default", "renderer"])
@pytest.mark.parametrize("fmt", [F32, Q8, W8])
@pytest.mark.parametrize("name", list(SCENES))
def test_table_is_normals_at_the_ids(name, fmt, opts):
    sc = SCENES[name]()
    nrm, refs, tri = _check(sc, fmt, opts)
    assert not nrm[~tri].view(np.uint64).any()  # a sphere's entry: zeros (unread)
    if name == "bunny_full":
        assert tri.sum() == len(sc.root) - 3 and len(sc.scene_data.mesh_table[0].positions) < tri.sum()  # shared
    if name == "two_meshes":
        assert refs[tri, :3].max() == 9 and (refs[tri, :3] >= 4).any()  # the second mesh's base is 4
        raw = nrm[tri].view(np.uint64)
        assert (raw == 0x7FF8_0000_DEAD_BEEF).any() and (raw == 0x8000_0000_0000_0000).any()
    if name == "mixed":
        assert (~tri).sum() == 41 and tri.sum() == 128
        if opts == DEFAULT:  # spheres sit inside the tree's leaf order, not only behind it
            assert (~tri)[:len(tri) - 4].any()


def test_capacity_and_null_outputs():
    sc = two_meshes()
    full, _, _ = _table(sc, F32, DEFAULT)
    d = sc.desc()
    n = ctypes.c_uint64(0)
    part = np.full((3, 9), np.nan)
    F.check_host(F.host().rph_tri_normals(d.ptr(), F32, -1, 0, 2, part.ctypes.data, None, None, ctypes.byref(n)))
    assert n.value == len(sc.root)
    assert np.array_equal(part[:2].view(np.uint64), full[:2].view(np.uint64)) and np.isnan(part[2]).all()
    assert F.host().rph_tri_normals(None, F32, -1, 0, 0, None, None, None, ctypes.byref(n)) == F.RP_EINVAL
    assert F.host().rph_tri_normals(d.ptr(), F32, -1, 0, 0, None, None, None, None) == F.RP_EINVAL


# FNV-1a over the packed node records and prim_refs (rph_bvh_tree_hash_opt) of the commit before the normals table
PINNED = {
    ("bunny_full", F32, DEFAULT): 0x76bb0a4f40c1c18f, ("bunny_full", F32, RENDERER): 0xc5cc7d8c3b971581,
    ("bunny_full", Q8, DEFAULT): 0x2670a68e81265a43, ("bunny_full", Q8, RENDERER): 0xc0bd3bff54c8fe78,
    ("bunny_full", W8, DEFAULT): 0x27e979bb10a70a13, ("bunny_full", W8, RENDERER): 0x3c172a6f5d6f812a,
    ("two_meshes", F32, DEFAULT): 0x8f75548d4a54f45f, ("two_meshes", Q8, DEFAULT): 0x70a68b65a4651fa8,
    ("mixed", F32, DEFAULT): 0x9c6beac1cab84a4a, ("mixed", Q8, RENDERER): 0x3d381e8c73611a2,
    ("mixed", W8, DEFAULT): 0xd1c214de3cc9eff1, ("meshes", F32, RENDERER): 0xfba88f911fe21967,
}


@pytest.mark.parametrize("key", list(PINNED), ids=lambda k: f"{k[0]}-{k[1]}-{k[2][0]}-{k[2][1]}")
def test_pinned_trees_keep_their_hash(key):
    name, fmt, opts = key
    h = ctypes.c_uint64()
    d = SCENES[name]().desc()
    F.check_host(F.host().rph_bvh_tree_hash_opt(d.ptr(), fmt, 0, opts[0], opts[1], ctypes.byref(h)))
    assert h.value == PINNED[key], hex(h.value)
