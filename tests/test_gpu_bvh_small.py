"""The device tree builders (rp_bvh_gpu.hip: LBVH and PLOC, then the one wide collapse) on the smallest trees.

2 triangles is the least the device builders accept (one binary node, both children of the root leaves); 3 and 4 fill
the root's wide node without opening a grandchild's family; 5 is the first scene that needs an inner wide child at
max_leaf = 1 and 9 the first at max_leaf = 8; 33 gives three levels.  Every tree passes the host's structural
self-check (options.self_check) and answers rays exactly as the host builder's tree of the same node format does:
the closest hit does not depend on the tree's shape.
"""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 4, 5, 9, 33]
# (builder, node_format, max_leaf, node_layout): both builders, both formats, the leaf sizes at either end, and the
# line-aligned families that only PLOC's quantized nodes have
GRID = [(b, f, m, "auto") for b in ("gpu", "ploc") for f in ("f32", "q8") for m in (1, 8)] + \
       [("ploc", "q8", m, "dfs_line") for m in (1, 8)]
GRID_IDS = ["-".join(map(str, g)) for g in GRID]


@functools.lru_cache(maxsize=None)
def _scene(n, duplicates=False):
    from rtpotato import scenes
    sc = scenes.random_mesh(n)
    if duplicates:  # every triangle is triangle 0: equal centroids, identical Morton codes
        pos = sc.scene_data.mesh_table[0].positions
        for i in range(1, n):
            pos[3 * i:3 * i + 3] = pos[0:3]
    return sc


@functools.lru_cache(maxsize=None)
def _rays(n, duplicates=False):
    """256 rays aimed at points inside the triangles and 256 at points of the scene's bounds, from outside them; the
    last 48: axis-parallel directions (one or two infinite inverse components) towards a triangle's centroid."""
    rng = np.random.default_rng(1000 + n)
    tri = _scene(n, duplicates).scene_data.mesh_table[0].positions.reshape(-1, 3, 3)
    lo, hi = tri.reshape(-1, 3).min(axis=0), tri.reshape(-1, 3).max(axis=0)
    k = 256
    w = rng.dirichlet(np.ones(3), size=k)
    on_tri = np.einsum("kv,kvc->kc", w, tri[rng.integers(0, len(tri), size=k)])
    in_box = rng.uniform(lo, hi, size=(k, 3))
    target = np.concatenate([on_tri, in_box])
    d = rng.normal(size=(2 * k, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    o = target - d * rng.uniform(4.0, 6.0, size=(2 * k, 1))
    rays = np.concatenate([o, target - o, np.full((2 * k, 1), 1e-3), np.full((2 * k, 1), np.inf)], axis=1)
    cen = tri.mean(axis=1)
    for j in range(48):
        axis, two = j % 3, j % 2
        r = rays[2 * k - 48 + j]
        c = cen[j % len(cen)]
        r[0:3] = c
        r[3:6] = 0.0
        r[axis] = c[axis] - 5.0
        r[3 + axis] = 1.0
        if two:  # a second non-zero component: the ray still passes through the centroid
            b = (axis + 1) % 3
            r[b] = c[b] - 5.0
            r[3 + b] = 1.0
    return rays


@functools.lru_cache(maxsize=None)
def _host_hits(n, fmt, duplicates=False):
    """The host builder's tree of the same node format: the reference of every case, computed once."""
    from rtpotato import render
    with render.DeviceScene(_scene(n, duplicates), options={"builder": "host", "node_format": fmt}) as ds:
        hits, mats = ds.intersect(_rays(n, duplicates))
    hits.setflags(write=False)
    mats.setflags(write=False)
    return hits, mats


def _options(builder, fmt, max_leaf, layout):
    return {"builder": builder, "node_format": fmt, "max_leaf": max_leaf, "node_layout": layout, "self_check": 1}


def _check_shape(info, n, max_leaf):
    assert info["prims"] == n, info
    assert math.ceil(n / max_leaf) <= info["leaves"] <= n, info
    assert info["nodes"] >= 1, info


@pytest.mark.parametrize("builder,fmt,max_leaf,layout", GRID, ids=GRID_IDS)
@pytest.mark.parametrize("n", SIZES)
def test_small_tree_matches_host_tree(gpu, n, builder, fmt, max_leaf, layout):
    with gpu.DeviceScene(_scene(n), options=_options(builder, fmt, max_leaf, layout)) as ds:
        info = ds.info()
        hits, mats = ds.intersect(_rays(n))
    _check_shape(info, n, max_leaf)
    ref, ref_mats = _host_hits(n, fmt)
    hit = np.isfinite(ref[:, 0])
    assert hit.sum() >= 256, hit.sum()  # at least the rays aimed at a triangle
    assert np.array_equal(np.isfinite(hits[:, 0]), hit)
    assert np.array_equal(hits[hit, 0:7], ref[hit, 0:7])  # t, position, normal
    assert np.array_equal(mats[hit], ref_mats[hit])
    assert np.max(np.abs(hits[hit, 7:] - ref[hit, 7:])) < 1e-12  # uv, as test_intersect_rays


@pytest.mark.parametrize("builder,fmt,max_leaf,layout", GRID, ids=GRID_IDS)
def test_identical_triangles(gpu, builder, fmt, max_leaf, layout):
    """Nine copies of one triangle: every centroid equal, every Morton code identical.  Exact-t ties may pick any of
    the copies, so only the hit mask and t are compared (all share one material)."""
    n = 9
    with gpu.DeviceScene(_scene(n, True), options=_options(builder, fmt, max_leaf, layout)) as ds:
        info = ds.info()
        hits, _ = ds.intersect(_rays(n, True))
    _check_shape(info, n, max_leaf)
    ref, _ = _host_hits(n, fmt, True)
    hit = np.isfinite(ref[:, 0])
    assert hit.sum() >= 256, hit.sum()
    assert np.array_equal(np.isfinite(hits[:, 0]), hit)
    assert np.array_equal(hits[hit, 0], ref[hit, 0])


@pytest.mark.parametrize("fmt,max_leaf,layout", [g[1:] for g in GRID if g[0] == "ploc"],
                         ids=[i for g, i in zip(GRID, GRID_IDS) if g[0] == "ploc"])
def test_ploc_build_is_deterministic(gpu, fmt, max_leaf, layout):
    """Two PLOC builds of one scene: the same tree (after the depth-first relayout nothing depends on the order of the
    collapse's atomics), so the same info() and byte-identical answers, primitive-dependent columns included.
    PLOC only: the LBVH has no relayout, its wide node ids come from the collapse's atomics and are not reproducible
    (its tree is: test_gpu_bvh_ref.py compares it with the reference by a walk from the root in child slot order)."""
    n = 33
    out = []
    for _ in range(2):
        with gpu.DeviceScene(_scene(n), options=_options("ploc", fmt, max_leaf, layout)) as ds:
            hits, mats = ds.intersect(_rays(n))
            out.append((ds.info(), hits.tobytes(), mats.tobytes()))
    assert out[0][0] == out[1][0]
    assert out[0][1] == out[1][1] and out[0][2] == out[1][2]
