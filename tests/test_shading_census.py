"""CPU: the oracle's shading census (rp_oracle.h OR_E_*, oracle_py.EVENT_NAMES) and the aimed scenes of
tests/shading_scenes.py.

The census records which branch of the shading every path vertex of an oracle frame took, per pixel.  The GPU frames of
tests/test_gpu_shading.py are held to the oracle's pixel for pixel, so an event that the oracle's frame produces on many
pixels is a branch the device is checked on; an event no frame produces is a branch nobody checks.  Here:
  * the oracle reproduces golden_shading.npz (the pure-Python restatement's frames of the aimed scenes) bit for bit,
  * every event a scene owns appears on at least FLOOR = 16 distinct pixels of the frame the GPU tests render
    (a condition on the scenes, set before they were first rendered: one odd pixel cannot carry an event),
  * every event of the enum is owned by some scene, so an event added later without a scene fails,
  * three deliberately wrong scenes change at least 16 pixels of the aimed frame that exists to catch them.
"""
import ctypes
import os

import numpy as np
import pytest

import shading_scenes as S
from brute import Brute
from parity import oracle_render

HERE = os.path.dirname(os.path.abspath(__file__))

# catalogue scenes (at test_catalogue_scenes' 64 x 36 x 4 spp) that own the events no aimed scene is about
CATALOGUE_OWNS = {
    "variants": ["bg_none", "tx_missing", "sc_none", "ab_black_body"],
    "bunny_lambert": ["bg_sky_gradient", "ab_albedo", "em_none", "hit_miss"],
}
# events that cannot occur in any scene: none
IMPOSSIBLE = {}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "golden_shading.npz"))


_census = {}


def _aimed(name):
    if name not in _census:
        rgb, ctr, mask = S.census(S.scene(name), S.params(name))
        mask.setflags(write=False)
        _census[name] = (rgb, ctr, mask)
    return _census[name]


def test_event_names_match_the_enum(oracle):
    """EVENT_NAMES has one name per OR_E_* value and fits the 64-bit pixel mask; the seven counters keep their place."""
    import re
    src = open(os.path.join(os.path.dirname(HERE), "oracle", "rp_oracle.h")).read()
    enum = src[src.index("OR_C_RAYS = 0"):src.index("OR_C_N\n")]
    events = [e for e in re.findall(r"\bOR_E_([A-Z0-9_]+)\b", re.sub(r"/\*.*?\*/", "", enum, flags=re.S))
              if e != "FIRST"]
    assert [e.lower() for e in events] == oracle.EVENT_NAMES
    assert len(set(oracle.EVENT_NAMES)) == len(oracle.EVENT_NAMES) <= 64
    assert oracle.COUNTER_NAMES == ["rays", "box_tests", "tri_tests", "sphere_tests", "samples", "tri_hits", "texels"]
    assert oracle.N_COUNTERS == 7


@pytest.mark.parametrize("name", list(S.SCENES))
def test_oracle_equals_python_restatement(golden, name):
    from rtpotato import scenes
    from rtpotato.scene import RenderParams
    w, h, spp = (int(x) for x in golden[f"img_{name}_size"])
    sc = scenes.configure(S.scene(name), w, h)
    p = RenderParams(w, h, spp, S.params(name).max_bounce, S.SEED)
    rgb, _, ctr = oracle_render(sc, p, threads=4)
    assert np.array_equal(rgb, golden[f"img_{name}"])
    assert ctr["rays"] == int(golden[f"img_{name}_rays"][0]) and ctr["samples"] == w * h * spp


@pytest.mark.parametrize("name", list(S.SCENES))
def test_render_events_is_render(name):
    """The census entry point renders or_render's frame and counters, and or_render still writes seven counters."""
    from oracle import oracle_py as O
    sc, p = S.scene(name), S.params(name)
    rgb, ctr, mask = _aimed(name)
    ref, _, ref_ctr = oracle_render(sc, p, threads=3)
    assert np.array_equal(rgb, ref, equal_nan=True)
    assert {k: ctr[k] for k in O.COUNTER_NAMES} == ref_ctr
    d = sc.desc()
    osc = O.OracleScene(d.addr(), d)
    cam, pc = sc.camera.to_c(), p.to_c()
    out = np.zeros((p.height, p.width, 3))
    guard = np.full(O.N_COUNTERS + 4, 77, dtype=np.uint64)
    try:
        assert O.lib().or_render(osc.h, ctypes.addressof(cam), ctypes.addressof(pc), out.ctypes.data, None,
                                 guard.ctypes.data, 2) == 0
    finally:
        osc.close()
    assert guard[O.N_COUNTERS:].tolist() == [77] * 4
    # the mask is the census per pixel: an event is counted if and only if some pixel's mask has it
    px = S.event_pixels(mask)
    assert {e for e in O.EVENT_NAMES if ctr[e]} == {e for e in O.EVENT_NAMES if px[e]}
    assert ctr["hit_tri"] + ctr["hit_sph"] + ctr["hit_miss"] == ctr["rays"]
    assert ctr["tx_image"] == ctr["texels"] and ctr["hit_tri"] <= ctr["tri_hits"]


@pytest.mark.parametrize("name", list(S.SCENES))
def test_owned_events_meet_the_floor(name):
    assert (S.W, S.H, S.SPP) == (48, 32, 8) and S.FLOOR == 16
    px = S.event_pixels(_aimed(name)[2])
    print(name, {e: px[e] for e in S.OWNS[name]})
    low = {e: px[e] for e in S.OWNS[name] if px[e] < S.FLOOR}
    assert not low, low


@pytest.mark.parametrize("name", list(CATALOGUE_OWNS))
def test_catalogue_owned_events_meet_the_floor(name):
    sc, p = S.catalogue(name)
    px = S.event_pixels(S.census(sc, p)[2])
    low = {e: px[e] for e in CATALOGUE_OWNS[name] if px[e] < S.FLOOR}
    assert not low, low


def test_every_event_has_an_owner(oracle):
    owned = {e for v in S.OWNS.values() for e in v} | {e for v in CATALOGUE_OWNS.values() for e in v}
    assert owned <= set(oracle.EVENT_NAMES), owned - set(oracle.EVENT_NAMES)
    assert set(S.OWNS) == set(S.SCENES)
    missing = set(oracle.EVENT_NAMES) - owned - set(IMPOSSIBLE)
    assert not missing, f"census events no scene owns: {sorted(missing)}"


def test_completeness(oracle):
    """Over the aimed scenes and the catalogue scenes at the suite's small sizes, every event of the enum occurs."""
    seen = set()
    for name in S.SCENES:
        seen |= {e for e, n in S.event_pixels(_aimed(name)[2]).items() if n}
    for name in S.CATALOGUE_FRAMES:
        sc, p = S.catalogue(name)
        seen |= {e for e, n in S.event_pixels(S.census(sc, p)[2]).items() if n}
    missing = set(oracle.EVENT_NAMES) - seen - set(IMPOSSIBLE)
    assert not missing, f"census events no test frame produces: {sorted(missing)}"


@pytest.mark.parametrize("name", ["sky_at_texture_0", "mesh2_vertex_base", "checker_uv_zero"])
def test_aimed_frames_see_the_mistakes(name):
    """Sensitivity: a scene with one mistake of the kind an aimed scene exists to catch differs from it on at least
    16 pixels of the oracle's frame (far above parity.TOL_EXACT, at which the GPU frame is compared)."""
    aimed, wrong = S.wrong_scenes()[name]
    ref = _aimed(aimed)[0]
    rgb, _, _ = oracle_render(wrong, S.params(aimed), threads=4)
    differ = int((np.abs(rgb - ref).max(axis=-1) > 1e-6).sum())
    print(name, "pixels that differ:", differ)
    assert differ >= 16


def test_brute_force_on_several_meshes(oracle):
    """tests/brute.py on three meshes against the oracle's closest-hit query (its BVH): the same records, on all
    three meshes.  This is the yardstick test_gpu_shading.py holds rp_intersect to."""
    sc, rays = S.mesh_rays()
    bf = Brute(sc)
    ref = bf.closest(rays)
    rec, mats, is_tri = bf.records(rays, ref)
    assert not ref["tie"].any()
    d = sc.desc()
    osc = oracle.OracleScene(d.addr(), d)
    try:
        hits, omats, _ = osc.intersect(rays)
    finally:
        osc.close()
    assert np.array_equal(hits, rec) and np.array_equal(omats, mats)
    k = np.searchsorted(bf.tri_id, ref["id"][is_tri])
    per_mesh = np.bincount(bf.tri_mesh[k], minlength=3)
    print("hits per mesh", per_mesh.tolist(), "misses", int((ref["id"] < 0).sum()))
    assert (per_mesh >= 100).all() and (ref["id"] < 0).sum() >= 100


@pytest.mark.parametrize("frame", list(S.AOV_FRAMES))
@pytest.mark.parametrize("spp", [1, 4])
def test_feature_pass_references_of_the_aimed_scenes(frame, spp):
    """tests/aov_ref.py on the aimed scenes, checked as tests/test_aov_ref.py checks its catalogue frames before they
    judge the GPU: the rebuilt camera rays hit the renderer's pixels with the renderer's normals, bit for bit."""
    import aov_ref
    S.add_aov_frames()
    r = aov_ref.refs(frame, spp)
    hit = r["depth_fg"] > 0
    assert np.array_equal(r["depth_fg"], r["fg"])
    assert np.array_equal(r["depth_normal"], r["normal"])
    assert 100 < hit.sum() < hit.size - 100 and np.all(r["depth"][hit] > 1e-3) and np.all(r["depth"][~hit] == 0.0)
    assert np.all(r["albedo"][~hit] == 0.0) and np.all(r["normal"][~hit] == 0.0)
    if spp == 4:
        assert ((r["fg"] > 0) & (r["fg"] < 1)).sum() >= 20


@pytest.mark.parametrize("name", list(S.PERMUTATIONS))
def test_permuted_tables_are_the_same_scene(name):
    """S.permuted renumbers every reference: the oracle renders the permuted scenes to the same bits and census."""
    from oracle import oracle_py as O
    ref, ctr, mask = _aimed(name)
    for perm in S.PERMUTATIONS[name]:
        rgb, c, m = S.census(S.permuted(S.scene(name), **perm), S.params(name))
        keep = ~np.uint64(1 << O.EVENT_NAMES.index("hit_tri_mesh1"))  # which meshes have an index >= 1 changes
        assert np.array_equal(rgb, ref) and np.array_equal(m & keep, mask & keep), perm
        c["hit_tri_mesh1"], expect = 0, dict(ctr, hit_tri_mesh1=0)
        assert c == expect, perm
