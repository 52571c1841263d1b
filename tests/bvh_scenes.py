"""Inputs aimed at the places the device tree builders (rp_bvh_gpu.hip) can go wrong (test infrastructure, as
tests/shading_scenes.py): small numpy meshes and spheres, at most about 1,100 primitives, no asset files.

    uniform_N    scenes.random_mesh(N), N around PLOC's 256-cluster block, block + radius, and two to four blocks: the
                 rounds move the cluster count across the seams
    seam_N       N boxes along one axis in tight pairs (2k+1, 2k+2): the round-1 mutual pair (255, 256) straddles a
                 block seam, and the equal spacings make exact distance ties
    planar       a 16 x 16 quad grid in the plane y = 0: one Morton axis of zero extent (scale 0), the two triangles of
                 a quad share a box (the SAH leaf rule fires), the grid's exact coordinates tie everywhere
    clustered    300 triangles inside one 30-bit Morton cell beside 200 scattered ones: the LBVH's index tie-break
                 decides long runs, the radix chains are deep; 100 more within a few cells of PLOC's 63-bit code
    duplicates   33 copies of one triangle: every code identical
    mixed        spheres and triangles over four orders of magnitude around a radius-1000 ground sphere, away from the
                 origin: node frames and f32 rounding at large coordinates
"""
from __future__ import annotations

import functools
import math

import numpy as np

from rtpotato import _ffi as F
from rtpotato import scenes
from rtpotato.scene import (Absorb, Camera, Emit, Hittable, Material, Mesh, Scatter, Scene, SceneData, Transformation,
                            hittables, rgb)

UNIFORM = [2, 3, 5, 33, 255, 256, 257, 259, 515, 1031]
SEAM = [257, 258, 260, 515]
PLOC_B = 256  # clusters per block of ploc_nn_kernel


def _scene(tris: np.ndarray, spheres=(), name="") -> Scene:
    """tris: (n, 3, 3) vertices; spheres: (centre, radius) pairs, placed after the triangles in root order."""
    tris = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    pos = tris.reshape(-1, 3)
    mesh = Mesh(pos, np.tile([0.0, 0.0, 1.0], (len(pos), 1)), np.zeros((len(pos), 2)),
                np.arange(len(pos), dtype=np.uint32), material=0)
    materials = [Material.new(Scatter.Lambert, Absorb.Albedo(rgb(0.7, 0.7, 0.7)), Emit.None_)]
    root = hittables(Hittable.Triangle(mesh.iter_triangles(), 0), *[Hittable.Sphere(c, r, 0) for c, r in spheres])
    cam = Camera(1.0, math.pi / 3.0, 1.0, 0.0, Transformation.lookat((0.0, 0.0, 3.5), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)))
    return Scene(cam, SceneData(materials, [], [mesh]), root, Emit.SkyGradient, F.RP_ROOT_BVH, name)


def uniform(n: int) -> Scene:
    return scenes.random_mesh(n)


def seam(n: int) -> Scene:
    """Gaps of 1 inside a pair and 3 between pairs; the pair across each multiple of 256 is the tightest (0.25) and
    both its outer neighbours lean on it (0.5).  A search that cannot see across the seam then pairs 254 with 255, and
    256 with 257: merges the true search never makes, where a merely delayed merge would heal in the next round."""
    gap = np.where(np.arange(n - 1) % 2 == 1, 1.0, 3.0)  # gap[i]: between boxes i and i + 1
    for s in range(PLOC_B, n, PLOC_B):
        gap[s - 1], gap[s - 2] = 0.25, 0.5
        if s + 1 < n:
            gap[s] = 0.5
    x = np.concatenate([[1.0], 1.0 + np.cumsum(gap)])
    a = np.stack([x, np.zeros(n), np.zeros(n)], axis=1)
    tris = np.stack([a, a + [0.5, 0.25, 0.0], a + [0.0, 0.5, 0.25]], axis=1)
    return _scene(tris, name=f"seam_{n}")


def planar(side: int = 16) -> Scene:
    tris = []
    for j in range(side):
        for i in range(side):
            p00, p10, p11, p01 = ([float(i + di), 0.0, float(j + dj)] for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)))
            tris += [[p00, p10, p11], [p00, p11, p01]]
    return _scene(np.array(tris), name="planar")


def clustered() -> Scene:
    rng = np.random.default_rng(0xC1)
    far = rng.uniform(-1.0, 1.0, size=(200, 1, 3)) + rng.uniform(-0.01, 0.01, size=(200, 3, 3))
    near = np.array([0.3001, -0.2003, 0.1002]) + rng.uniform(-1e-4, 1e-4, size=(300, 1, 3)) + \
        rng.uniform(-2e-5, 2e-5, size=(300, 3, 3))
    # and 100 within a few cells of the 63-bit code: their order is decided by the code's last bit per axis
    tight = np.array([-0.4502, 0.6001, -0.1503]) + rng.uniform(-1.5e-6, 1.5e-6, size=(100, 1, 3)) + \
        rng.uniform(-2e-7, 2e-7, size=(100, 3, 3))
    tris = np.concatenate([far[:100], near, far[100:150], tight, far[150:]])
    return _scene(tris, name="clustered")


def duplicates(n: int = 33) -> Scene:
    sc = scenes.random_mesh(n)
    pos = sc.scene_data.mesh_table[0].positions
    for i in range(1, n):
        pos[3 * i:3 * i + 3] = pos[0:3]
    return sc


def mixed() -> Scene:
    rng = np.random.default_rng(0x51E)
    shift = np.array([300.125, 0.0, -700.375])
    size = 10.0 ** rng.uniform(-2.0, 1.0, size=120)  # 0.01 .. 10
    c = shift + rng.uniform(-1.0, 1.0, size=(120, 3)) * np.array([40.0, 0.0, 40.0]) + np.array([0.0, 1.0, 0.0]) * size[:, None]
    tris = c[:60, None, :] + rng.uniform(-1.0, 1.0, size=(60, 3, 3)) * size[:60, None, None]
    spheres = [(shift + [0.0, -1000.0, 0.0], 1000.0)] + [(c[k], float(size[k])) for k in range(60, 120)]
    return _scene(tris, spheres, name="mixed")


INPUTS = {**{f"uniform_{n}": functools.partial(uniform, n) for n in UNIFORM},
          **{f"seam_{n}": functools.partial(seam, n) for n in SEAM},
          "planar": planar, "clustered": clustered, "duplicates": duplicates, "mixed": mixed}


@functools.lru_cache(maxsize=None)
def scene(name: str) -> Scene:
    return INPUTS[name]()


# The reference (tests/bvh_ref.py) of an input, computed once per stage and shared by the tests that need it.
@functools.lru_cache(maxsize=None)
def boxes(name: str):
    import bvh_ref
    return bvh_ref.scene_boxes(scene(name))


@functools.lru_cache(maxsize=None)
def merges(name: str, rules=None):
    import bvh_ref
    return bvh_ref.ploc_merges(boxes(name), rules or bvh_ref.DEVICE)


@functools.lru_cache(maxsize=None)
def reference(name: str, builder: str, node_format: int, max_leaf: int, cost_traverse: float, dfs_line: bool = False,
              rules=None):
    import bvh_ref
    rules = rules or bvh_ref.DEVICE
    ref = bvh_ref.build(boxes(name), builder, node_format, max_leaf, cost_traverse, dfs_line, rules,
                        merges(name, rules) if builder == "ploc" else None)
    ref.nodes.setflags(write=False)
    return ref
