"""The exact primitive tests and the slab test on the CPU, through the source the kernels compile
(raytracing-potato_amd/csrc/rp_isect.h): the ray families of tests/test_gpu_leaf_test.py -- aimed at every rejection of
the triangle and the sphere test -- through the CPU traversal model (rph_bvh_traversal_stats) in the three node
formats, and through the test hook rph_prim_test one primitive at a time, against brute force (tests/brute.py: numpy,
every ray against every hittable, its own statement of the reference's arithmetic)."""
import numpy as np
import pytest

from brute import Brute
from test_gpu_leaf_test import _families, _scene

MISS = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def reference():
    """(scene, brute force, family -> (rays, labels, brute force's closest hits)): made once, read-only."""
    scene = _scene()
    bf = Brute(scene)
    fam, lab = _families(scene, bf)
    out = {}
    for name, rays in fam.items():
        ref = bf.closest(rays)
        for a in ref.values():
            a.setflags(write=False)
        rays.setflags(write=False)
        out[name] = (rays, lab[name], ref)
    return scene, bf, out


def test_host_model_closest_hits_equal_brute_force(reference):
    """Hit or miss equals brute force for every ray, and the hittable wherever brute force has no exact-t tie (which of
    two tied hittables a tree returns is free), in the three node formats."""
    from rtpotato import _ffi as F
    scene, _, fams = reference
    ties = sum(int(r["tie"].sum()) for _, _, r in fams.values())
    total = sum(len(rays) for rays, _, _ in fams.values())
    print("ties", ties, "of", total)
    assert total == 7 * 282 and ties < 0.02 * total, (ties, total)
    d = scene.desc()
    for fmt in (F.RP_NODES_F32, F.RP_NODES_Q8, F.RP_NODES_W8):
        for name, (rays, _, ref) in fams.items():
            out = np.zeros((len(rays), 3), dtype=np.uint64)
            F.check_host(F.host().rph_bvh_traversal_stats(d.ptr(), rays.ctypes.data, len(rays), fmt, out.ctypes.data))
            hit = out[:, 2] != MISS
            assert np.array_equal(hit, ref["id"] >= 0), (fmt, name, np.nonzero(hit != (ref["id"] >= 0))[0][:10])
            got = np.where(hit, out[:, 2], 0).astype(np.int64)
            bad = np.nonzero(hit & ~ref["tie"] & (got != ref["id"]))[0]
            assert len(bad) == 0, (fmt, name, bad[:10], got[bad[:10]], ref["id"][bad[:10]])


def _one(bf, hid):
    """Brute force over the single hittable `hid` (its own arithmetic, one primitive), and that primitive as
    rph_prim_test takes it: (kind, nine doubles)."""
    one = object.__new__(Brute)
    k = np.searchsorted(bf.tri_id, hid)
    if k < len(bf.tri_id) and bf.tri_id[k] == hid:
        one.tri_id, one.sph_id, one.sph = bf.tri_id[k:k + 1], bf.sph_id[:0], []
        one.A, one.ba, one.ca = bf.A[k:k + 1], bf.ba[k:k + 1], bf.ca[k:k + 1]
        return one, 1, np.concatenate([bf.A[k], bf.ba[k], bf.ca[k]])
    q = int(np.searchsorted(bf.sph_id, hid))
    assert bf.sph_id[q] == hid
    one.tri_id, one.sph_id, one.sph = bf.tri_id[:0], bf.sph_id[q:q + 1], [bf.sph[q]]
    c, rad, _ = bf.sph[q]
    return one, 0, np.concatenate([c, [rad], np.zeros(5)])


def test_prim_test_equals_brute_force_bit_for_bit(reference):
    """For every ray the primitive brute force names as its closest hit, and for the plane family the triangle a ray is
    aimed at, accepted or not: `accepted` is brute force's predicate, and t, u, v of an accepted test are brute
    force's bits (both evaluate the reference's expression in f64 without contraction: no tolerance)."""
    from rtpotato import _ffi as F
    _, bf, fams = reference
    pairs = []  # (hittable, rays)
    for name, (rays, lab, ref) in fams.items():
        hit = ref["id"] >= 0
        pairs.append((ref["id"][hit], rays[hit]))
        if name == "plane":
            aimed = lab >= 0
            pairs.append((bf.tri_id[lab[aimed]], rays[aimed]))
    ids = np.concatenate([p[0] for p in pairs])
    rays = np.ascontiguousarray(np.concatenate([p[1] for p in pairs]))
    accepted = rejected = spheres = 0
    for hid in np.unique(ids):
        r = np.ascontiguousarray(rays[ids == hid])
        one, kind, g = _one(bf, hid)
        ref = one.closest(r)
        out = np.full((len(r), 4), np.nan)
        F.check_host(F.host().rph_prim_test(kind, g.ctypes.data, r.ctypes.data, len(r), out.ctypes.data))
        acc = ref["id"] >= 0
        assert np.array_equal(out[:, 0], acc.astype(np.float64)), (hid, out[:, 0], acc)
        for col, key in ((1, "t"), (2, "u"), (3, "v")):
            assert np.array_equal(out[acc, col], ref[key][acc]), (hid, key, out[acc, col], ref[key][acc])
        accepted += int(acc.sum())
        rejected += int((~acc).sum())
        spheres += int(acc.sum()) if kind == 0 else 0
    print("accepted", accepted, "rejected", rejected, "sphere hits", spheres)
    # every closest hit is an accepted test; the plane family aims more than 60 rays at a triangle with |det| < SMOL and
    # the sphere family has more than 150 sphere hits (test_gpu_leaf_test.py test_families_reach_what_they_aim_at)
    n_hits = sum(int((ref["id"] >= 0).sum()) for _, _, ref in fams.values())
    assert accepted >= n_hits and rejected > 60 and spheres > 150


def test_prim_test_refuses_bad_arguments():
    from rtpotato import _ffi as F
    g, r, out = np.zeros(9), np.zeros((1, 8)), np.zeros((1, 4))
    H = F.host()
    assert H.rph_prim_test(2, g.ctypes.data, r.ctypes.data, 1, out.ctypes.data) == F.RP_EINVAL
    assert H.rph_prim_test(1, None, r.ctypes.data, 1, out.ctypes.data) == F.RP_EINVAL
    assert H.rph_prim_test(1, g.ctypes.data, None, 1, out.ctypes.data) == F.RP_EINVAL
    assert H.rph_prim_test(0, g.ctypes.data, r.ctypes.data, 1, None) == F.RP_EINVAL
