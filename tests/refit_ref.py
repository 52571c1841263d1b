"""The refit (raytracing-potato_amd/csrc/rp_refit.h) written out from its definition in numpy and plain
Python f64: the reference tests/test_refit.py holds the host model (rph_refit_records) to, and tests/test_gpu_refit.py
the device's read-back records, bit for bit.  The rounding and the frames are tests/bvh_ref.py's (f32_rd, f32_ru,
qframe, q_down, q_up), the restatement the device builders' trees are already pinned to.

    scene_records   the primitive table of a scene in a given leaf order: Prim, PrimRef, TriNormals (pack_prim)
    geometry        a scene's positions, normals and spheres in the refit's numbering
    deform          the tests' deformation
    plan            reachable nodes, levels, order
    prim_record     a primitive's record from its geometry;  prim_box: its exact box (hittable_box)
    node_words      a node's new box words from its children's exact boxes, both formats
    refit           the whole update, in place on a tree dict (DeviceScene.tree()'s layout)

Min and max are fmin and fmax (np.fmin / np.fmax: a NaN is ignored beside a number and stays where all are NaN).
"""
from __future__ import annotations

import math

import numpy as np

import bvh_ref as R
from rtpotato import _ffi as F

AXES = (("lo_x", "hi_x"), ("lo_y", "hi_y"), ("lo_z", "hi_z"))
OUT_OF_BOUND = 1
NOT_REACHED = 0xFFFFFFFF
INF = math.inf


# ---------------------------------------------------------------------------------------------------------------
# input

def geometry(scene) -> dict:
    """positions, normals (n_vertices, 3): the meshes' vertices concatenated in mesh order; spheres (n_spheres, 4):
    {center, radius} of the sphere hittables in hittable order."""
    meshes = scene.scene_data.mesh_table
    pos = np.concatenate([m.positions for m in meshes]) if meshes else np.zeros((0, 3))
    nrm = np.concatenate([m.normals for m in meshes]) if meshes else np.zeros((0, 3))
    sph = scene.root[scene.root["kind"] == F.RP_HITTABLE_SPHERE]
    spheres = np.concatenate([sph["center"], sph["radius"][:, None]], axis=1) if len(sph) else np.zeros((0, 4))
    return {"positions": pos.copy(), "normals": nrm.copy(), "spheres": spheres.copy()}


def amplitude(geom: dict, frac: float = 0.05) -> float:
    """frac of the scene's extent: the largest side of the vertices' bounds, or -- a scene of spheres alone, whose
    ground sphere would make its bounds meaningless -- of the median radius."""
    pos = geom["positions"]
    if len(pos):
        return frac * float((pos.max(axis=0) - pos.min(axis=0)).max())
    return frac * float(np.median(geom["spheres"][:, 3]))


def deform(geom: dict, frac: float = 0.05) -> dict:
    """p' = p + a sin(3 p.yzx) per component, a = frac of the extent, for the vertices and the spheres' centres;
    normals n' = n.yzx (a rotation of the axes); radii x 1.1."""
    a = amplitude(geom, frac)

    def move(p):
        return p + a * np.sin(3.0 * p[:, [1, 2, 0]])

    sph = geom["spheres"]
    return {"positions": move(geom["positions"]), "normals": geom["normals"][:, [1, 2, 0]].copy(),
            "spheres": np.concatenate([move(sph[:, :3]), sph[:, 3:4] * 1.1], axis=1)}


def scene_records(scene, perm) -> tuple:
    """(prims, prim_refs, tri_normals) of `scene` with source hittable perm[k] at leaf-order position k: the triangle
    {a, a - b, a - c}, the sphere {center, radius, 0...}; v = the global vertex ids, src = the hittable."""
    perm = np.asarray(perm, dtype=np.int64)
    n = len(perm)
    prims = np.zeros(n, dtype=F.prim_dtype())
    refs = np.zeros(n, dtype=F.prim_ref_dtype())
    tn = np.zeros(n, dtype=F.tri_normals_dtype())
    root = scene.root[perm]
    refs["src"] = perm
    meshes = scene.scene_data.mesh_table
    vbase = np.concatenate([[0], np.cumsum([len(m.positions) for m in meshes])]).astype(np.int64)
    geom = geometry(scene)
    sph = root["kind"] == F.RP_HITTABLE_SPHERE
    prims["kind"] = np.where(sph, 0, 1)
    prims["material"][sph] = root["material"][sph]
    prims["g"][sph, 0:3] = root["center"][sph]
    prims["g"][sph, 3] = root["radius"][sph]
    for mi, m in enumerate(meshes):
        rows = np.nonzero(~sph & (root["mesh"] == mi))[0]
        if not len(rows):
            continue
        t = root["triangle"][rows].astype(np.int64)
        v = np.stack([m.indices[t + k].astype(np.int64) + vbase[mi] for k in range(3)], axis=1)
        refs["v"][rows] = v
        prims["material"][rows] = m.material
        a, b, c = (geom["positions"][v[:, k]] for k in range(3))
        prims["g"][rows, 0:3], prims["g"][rows, 3:6], prims["g"][rows, 6:9] = a, a - b, a - c
        tn["n"][rows] = geom["normals"][v]
    return prims, refs, tn


def tree_of(scene, ref: "R.RefTree", node_format: int) -> tuple:
    """A bvh_ref tree as DeviceScene.tree() would return it, and its per-primitive normals."""
    prims, refs, tn = scene_records(scene, ref.perm)
    return ({"node_format": node_format, "root": 0, "nodes": ref.nodes.copy(), "prims": prims, "prim_refs": refs}, tn)


# ---------------------------------------------------------------------------------------------------------------
# the plan

def plan(nodes: np.ndarray, root: int) -> tuple:
    """-> (level per record or NOT_REACHED, order, n_levels): the nodes reachable from root; a node's level is 0
    without inner children, else 1 + the highest among them; order sorts them by (level, index)."""
    level = {}

    def inner(i):
        return [int(c) for c in nodes[i]["child"] if int(c) != R.ENTRY_EMPTY and not int(c) & R.ENTRY_LEAF]

    stack = [(root, False)]
    while stack:
        i, done = stack.pop()
        if done:
            level[i] = 1 + max((level[c] for c in inner(i)), default=-1)
            continue
        assert i not in level
        stack.append((i, True))
        stack += [(c, False) for c in inner(i)]
    out = np.full(len(nodes), NOT_REACHED, dtype=np.uint32)
    for i, lv in level.items():
        out[i] = lv
    order = sorted(level, key=lambda i: (level[i], i))
    return out, order, level[root] + 1


def sphere_ranks(prims: np.ndarray, refs: np.ndarray) -> np.ndarray:
    """Per primitive: a sphere's rank among the sphere hittables in hittable order, through PrimRef.src."""
    sph = prims["kind"] == 0
    rank = np.zeros(len(prims), dtype=np.int64)
    rank[sph] = np.searchsorted(np.sort(refs["src"][sph]), refs["src"][sph])
    return rank


# ---------------------------------------------------------------------------------------------------------------
# the arithmetic

def prim_record(kind: int, a, b=None, c=None) -> np.ndarray:
    """g[9]: a triangle {a, a - b, a - c}; a sphere (a = {center, radius}) {center, radius, 0...}."""
    g = np.zeros(9)
    if kind == 1:
        g[0:3], g[3:6], g[6:9] = a, np.asarray(a) - b, np.asarray(a) - c
    else:
        g[0:4] = a
    return g


def prim_box(kind: int, a, b=None, c=None) -> tuple:
    """A triangle: fmin / fmax of its three VERTICES; a sphere: center -+ radius."""
    if kind == 1:
        return np.fmin(np.fmin(a, b), c), np.fmax(np.fmax(a, b), c)
    a = np.asarray(a)
    return a[0:3] - a[3], a[0:3] + a[3]


def union(boxes) -> tuple:
    lo, hi = boxes[0]
    for l, h in boxes[1:]:
        lo, hi = np.fmin(lo, l), np.fmax(hi, h)
    return lo, hi


EMPTY = (np.full(3, INF), np.full(3, -INF))


def node_words(node_format: int, rec, kids: list) -> tuple:
    """The new box words of record `rec` (written in place; child[] untouched) from kids[c] = the exact box of slot c
    or None for an empty slot.  -> the node's own exact box: the union from (+inf, -inf)."""
    q8 = node_format == F.RP_NODES_Q8
    nb = union([EMPTY] + [k for k in kids if k is not None])
    if q8:
        for a in range(3):
            lo, hi = float(nb[0][a]), float(nb[1][a])
            ok = math.isfinite(lo) and math.isfinite(hi) and lo <= hi
            rec["o"][a], rec["s"][a] = R.qframe(lo, hi) if ok else R.qframe(0.0, 0.0)
    for c in range(4):
        for a in range(3):
            if kids[c] is None:
                rec[AXES[a][0]][c], rec[AXES[a][1]][c] = (255, 0) if q8 else (INF, -INF)
                continue
            lo, hi = float(kids[c][0][a]), float(kids[c][1][a])
            if q8:
                ok = lo == lo and hi == hi  # quantize_child: a NaN bound takes the whole frame
                rec[AXES[a][0]][c] = R.q_down(lo, rec["o"][a], rec["s"][a]) if ok else 0
                rec[AXES[a][1]][c] = R.q_up(hi, rec["o"][a], rec["s"][a]) if ok else 255
            else:
                rec[AXES[a][0]][c], rec[AXES[a][1]][c] = R.f32_rd(lo), R.f32_ru(hi)
    return nb


# ---------------------------------------------------------------------------------------------------------------
# the whole update

def refit(tree: dict, tri_normals=None, positions=None, normals=None, spheres=None, bound: float = INF) -> int:
    """Refits `tree` in place (and tri_normals, when normals are given).  -> the status word."""
    nodes, prims, refs = tree["nodes"], tree["prims"], tree["prim_refs"]
    tri = prims["kind"] == 1
    if normals is not None:
        tri_normals["n"][tri] = np.asarray(normals).reshape(-1, 3)[refs["v"][tri].astype(np.int64)]
    if positions is None and spheres is None:
        return 0
    rank = sphere_ranks(prims, refs)
    boxes, status = [], 0
    for k in range(len(prims)):
        kind = int(prims["kind"][k])
        if kind == 1:
            geo = [np.asarray(positions).reshape(-1, 3)[int(v)] for v in refs["v"][k]]
        else:
            geo = [np.asarray(spheres).reshape(-1, 4)[rank[k]]]
        prims["g"][k] = prim_record(kind, *geo)
        lo, hi = prim_box(kind, *geo)
        boxes.append((lo, hi))
        x = np.concatenate([lo, hi])
        if (np.isfinite(x) & (np.abs(x) > bound)).any():
            status |= OUT_OF_BOUND
    _, order, _ = plan(nodes, tree["root"])
    own = {}
    for i in order:
        kids = []
        for c in nodes[i]["child"]:
            c = int(c)
            if c == R.ENTRY_EMPTY:
                kids.append(None)
            elif c & R.ENTRY_LEAF:
                first, cnt = c & R.LEAF_FIRST_MASK, ((c >> R.LEAF_SHIFT) & 7) + 1
                kids.append(union(boxes[first:first + cnt]))
            else:
                kids.append(own[c])
        own[i] = node_words(tree["node_format"], nodes[i], kids)
    return status
