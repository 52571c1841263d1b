"""CPU: the packed head of a device material record (rp_layout.h material_head_pack / material_head_unpack through the
host hooks rph_material_head and rph_scene_materials).  The render kernel's shading reads a hit's three kinds, needs_uv
and both texture ids from this head with one load, so: unpacking a packed head returns the fields for every
combination of the kinds and needs_uv and for texture ids on both sides of the 16-bit limit (beyond it the head says
`wide` and holds no id: the reader takes the record's u32 fields), and the head the builder wrote into every material
record of every catalogue scene and aimed scene is the head packed from that record's own fields.
"""
import ctypes
import itertools

import numpy as np
import pytest

import shading_scenes as S
from rtpotato import _ffi as F
from rtpotato import scenes
from rtpotato.scene import Absorb, Emit, Hittable, Material, Scatter, Scene, SceneData, Texture, hittables, rgb

SCATTER, ABSORB, EMIT = range(4), range(4), range(5)  # include/rp.h RP_SCATTER_*, RP_ABSORB_*, RP_EMIT_*
NEEDS_UV, WIDE = 1 << 12, 1 << 13                      # rp_layout.h MH_NEEDS_UV, MH_WIDE_TEX


def _head(fields):
    f = np.asarray(fields, dtype=np.uint32)
    packed, unpacked = np.zeros(2, dtype=np.uint32), np.zeros(7, dtype=np.uint32)
    F.check_host(F.host().rph_material_head(f.ctypes.data, packed.ctypes.data, unpacked.ctypes.data))
    return [int(x) for x in packed], [int(x) for x in unpacked]


def _records(sc: Scene) -> np.ndarray:
    """Rows {scatter_kind, absorb_kind, emit_kind, absorb_tex, emit_tex, needs_uv, head, head_tex} of a scene's
    material records as the builder fills them."""
    d = sc.desc()
    n = ctypes.c_uint64(0)
    F.check_host(F.host().rph_scene_materials(d.ptr(), 0, None, ctypes.byref(n)))
    words = np.zeros((n.value, 8), dtype=np.uint32)
    F.check_host(F.host().rph_scene_materials(d.ptr(), n.value, words.ctypes.data, ctypes.byref(n)))
    return words


@pytest.mark.parametrize("tex", [(0, 0), (1, 2), (65535, 0), (0, 65535), (65535, 65535)])
def test_pack_then_unpack_returns_every_combination(tex):
    for sk, ak, ek, uv in itertools.product(SCATTER, ABSORB, EMIT, (0, 1)):
        packed, un = _head([sk, ak, ek, uv, tex[0], tex[1]])
        assert un == [sk, ak, ek, uv, tex[0], tex[1], 0], (sk, ak, ek, uv, tex, packed, un)
        assert packed[0] == sk | ak << 4 | ek << 8 | (NEEDS_UV if uv else 0) and packed[1] == tex[0] | tex[1] << 16


@pytest.mark.parametrize("tex", [(65536, 0), (0, 65536), (65536, 65535), (0xFFFFFFFF, 7), (70000, 0xFFFFFFFF)])
def test_an_id_beyond_16_bits_sends_the_reader_to_the_fields(tex):
    for sk, ak, ek, uv in itertools.product(SCATTER, ABSORB, EMIT, (0, 1)):
        packed, un = _head([sk, ak, ek, uv, tex[0], tex[1]])
        assert un[:4] == [sk, ak, ek, uv] and un[6] == 1, (sk, ak, ek, uv, tex, packed, un)
        assert packed[0] & WIDE and packed[1] == 0


def test_needs_uv_is_a_flag_whatever_its_value():
    assert _head([1, 3, 0, 5, 2, 0])[1] == [1, 3, 0, 1, 2, 0, 0]


def _all_scenes():
    for name in S.CATALOGUE_FRAMES:
        yield name, scenes.CATALOGUE[name]()
    for name in S.SCENES:
        yield name, S.scene(name)


def test_every_scene_record_carries_the_head_of_its_own_fields():
    seen = set()
    for name, sc in _all_scenes():
        rec = _records(sc)
        assert len(rec) == len(sc.scene_data.material_table), name
        for i, (sk, ak, ek, at, et, uv, head, head_tex) in enumerate(rec.tolist()):
            packed, un = _head([sk, ak, ek, uv, at, et])
            assert [head, head_tex] == packed, (name, i, rec[i])
            assert un == [sk, ak, ek, 1 if uv else 0, at, et, 0], (name, i, rec[i])
            seen.add((sk, ak, ek, 1 if uv else 0))
    # the scenes between them use every scatter, absorb and emit kind, with and without uv
    assert {s[0] for s in seen} == set(SCATTER) and {s[1] for s in seen} == set(ABSORB)
    assert {s[2] for s in seen} == set(EMIT) and {s[3] for s in seen} == {0, 1}


def test_ids_0_65535_and_65536_in_a_built_scene():
    """A table of 65,537 Solid textures: materials mapped to ids 0 and 65,535 keep them in the head, the one mapped
    to id 65,536 is marked wide and keeps its ids in the u32 fields."""
    textures = [Texture.Solid(rgb(0.5, 0.5, 0.5))] * 65537
    materials = [Material.new(Scatter.Lambert, Absorb.AlbedoMap(0), Emit.None_),
                 Material.new(Scatter.Lambert, Absorb.AlbedoMap(65535), Emit.SkySphere(65535)),
                 Material.new(Scatter.Metal(0.1), Absorb.AlbedoMap(65536), Emit.None_),
                 Material.new(Scatter.Lambert, Absorb.AlbedoMap(3), Emit.SkySphere(65536))]
    root = hittables(*[Hittable.Sphere((float(i), 0.0, -3.0), 0.4, i) for i in range(4)])
    sc = Scene(S._cam(1.0, 1.0, 0.0, (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)), SceneData(materials, textures, []), root,
               Emit.SkyGradient, F.RP_ROOT_BVH, "wide_ids")
    rec = _records(sc).tolist()
    assert [r[3:5] for r in rec] == [[0, 0], [65535, 65535], [65536, 0], [3, 65536]]
    assert [bool(r[6] & WIDE) for r in rec] == [False, False, True, True]
    assert [r[7] for r in rec] == [0, 65535 | 65535 << 16, 0, 0]
    for r in rec:
        assert [r[6], r[7]] == _head([r[0], r[1], r[2], r[5], r[3], r[4]])[0]
