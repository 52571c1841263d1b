"""The kernels' always-tested site (rp_device.h always_tests, reached through trav_begin) on the GPU: closest hits of
tests/test_always_site.py's scenes and ray families through rp_intersect against brute force over every hittable
(tests/brute.py), bit for bit on t, the hit record and the material, in the three node formats.

The scenes are built by the host builder with the renderer's options (the minor rule on): an empty list, the ground
alone, the ground and two balls (config C3's shape), four spheres (the cap), five (past it: the ground listed, four
spheres in leaves), and two lists that hold a huge triangle -- one with a sphere behind it in list order, one with a
sphere on either side -- so the scalar sphere path, the generic path and the hand-over between them all run.  Each
family is 282 rays, shuffled and sent as batches of 5, 13, 64 and 200 (rp_intersect's kernel runs one ray per lane).
Rays for which brute force finds an exact-t tie between two hittables are compared on t only; the CPU module keeps
them under 2 % of a family and checks what each family reaches.
"""
import numpy as np
import pytest

from test_always_site import BATCHES, LISTS, N_FAM, always_reference

FORMATS = ("f32", "q8", "w8")


@pytest.fixture(scope="module")
def reference():
    return always_reference()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_always_site_equals_brute_force(gpu, reference, fmt):
    checked = 0
    for name in LISTS:
        scene, _, _, fams = reference[name]
        with gpu.DeviceScene(scene, options={"builder": "host", "node_format": fmt}) as ds:
            for fname, (rays, _, ref) in fams.items():
                start = 0
                for n in BATCHES:
                    s = slice(start, start + n)
                    start += n
                    hits, mats = ds.intersect(rays[s])  # raises on a stack-overflow status
                    where = (fmt, name, fname, n)
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
                    if sp.any():  # a sphere's uv goes through atan2 and asin (the leaf test's bound)
                        assert np.max(np.abs(hits[sp, 7:9] - rec[sp, 7:9])) < 1e-12, where
                    checked += n
                assert start == N_FAM
    assert checked == (2 + 8 * (len(LISTS) - 1)) * N_FAM
