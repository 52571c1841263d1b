"""The CPU model of the device traversal (rph_bvh_traversal_stats: rp_ray.h's ray setup, the packed wide trees, the
f32 / quantized slab tests) against brute force over every hittable (tests/brute.py): the slopes, addends, tmin32 and
best32 the header makes never cull a primitive the exact f64 tests accept, in any of the three node formats, on the
ray families of tests/test_bvh.py (random, axis-parallel, finite t_max, origins on vertices and box planes, rays
along mesh edges)."""
import numpy as np
import pytest

from brute import Brute
from test_bvh import FORMATS, _rays_for

_cache = {}


def _reference(name):
    """(scene, rays, brute-force closest hits): computed once per scene, shared by the three formats, not modified."""
    if name not in _cache:
        from rtpotato import scenes
        scene = scenes.CATALOGUE[name]()
        rays = _rays_for(scene, 2000, 3)
        ref = Brute(scene).closest(rays)
        for a in ref.values():
            a.setflags(write=False)
        _cache[name] = (scene, rays, ref)
    return _cache[name]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", ["bunny_full", "more_balls", "one_triangle", "two_balls"])
def test_traversal_model_finds_brute_force_hits(name, fmt):
    from rtpotato import _ffi as F
    scene, rays, ref = _reference(name)
    d = scene.desc()
    out = np.zeros((len(rays), 3), dtype=np.uint64)
    F.check_host(F.host().rph_bvh_traversal_stats(d.ptr(), rays.ctypes.data, len(rays), fmt, out.ctypes.data))
    got = np.where(out[:, 2] == np.uint64(2**64 - 1), -1, out[:, 2].astype(np.int64))
    assert (ref["id"] >= 0).sum() > len(rays) // 4
    # a hit is a hit and a miss a miss for every ray; the hittable is the brute-force one wherever it is unique
    assert np.array_equal(got >= 0, ref["id"] >= 0)
    uniq = ~ref["tie"]
    assert np.array_equal(got[uniq], ref["id"][uniq]), np.nonzero(got != ref["id"])[0][:10]
    assert ref["tie"].mean() < 0.05
