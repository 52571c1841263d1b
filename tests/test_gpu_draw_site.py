"""The kernel's keystream draws on the device (rp_device.h scatter_eval, start_sample; rp_draw.h).

A 16 x 8 frame is two waves; at 16 spp and 8 bounces a unit consumes about two hundred stream words (16 camera draws
and ~1.5 scatters per sample, 4 to 6 words a try), so its lane laps the 8-block ring (128 words) once or twice and the
q8 kernel's 4-block ring about three times, and over the 128 lanes the draw windows cross the ring's end, into the
mirror tail, at every offset.  more_balls puts Lambert, fuzzy Metal and Dielectric lanes into one wave (windows of two
and of three values, and the single draw); bunny_full is the headline's material set.  Every case is checked
against the oracle: paths are the reference's, so the image agrees within parity.py's bound and the ray, sample and
pixel counters are exactly equal -- one wrong or stale keystream word changes a path and its ray count.
"""
from dataclasses import replace

import pytest

from parity import assert_parity, compare, oracle_render
from test_gpu_frames import _assert_same, _frames_vs_singles

pytestmark = pytest.mark.gpu

W, H, SPP = 16, 8, 16
_refs = {}


def _case(name, lens=None, max_bounce=8, sps=0):
    from rtpotato import scenes
    from rtpotato.scene import RenderParams
    sc = scenes.configure(scenes.CATALOGUE[name](), W, H)
    if lens is not None:
        sc = replace(sc, camera=replace(sc.camera, lens_radius=lens))
    return sc, RenderParams(W, H, SPP, max_bounce, scenes.DEFAULT_SEED, samples_per_stream=sps)


def _check(gpu, name, fmt, **kw):
    sc, p = _case(name, **kw)
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _refs:  # one oracle render per case, shared by the node formats
        _refs[key] = oracle_render(sc, p, threads=8)
    ref, _, ctr = _refs[key]
    rgb, _, st = gpu.render(sc, p, options={"node_format": fmt})
    assert_parity(compare(rgb, ref))
    assert st["rays"] == ctr["rays"] and st["samples"] == ctr["samples"] == W * H * SPP, (st, ctr)
    assert st["pixels"] == W * H
    return st


@pytest.mark.parametrize("sps", [32, SPP])
@pytest.mark.parametrize("fmt", ["f32", "q8"])
@pytest.mark.parametrize("name", ["more_balls", "bunny_full"])
def test_draw_site_against_oracle(gpu, name, fmt, sps):
    st = _check(gpu, name, fmt, sps=sps)
    assert st["rays"] > 2 * st["samples"]  # most samples scatter: a unit's draws lap its ring


@pytest.mark.parametrize("fmt", ["f32", "q8"])
def test_draw_site_lens_camera(gpu, fmt):
    """UnitDisk with a non-zero radius: the camera's draws move the ray, through the same windows."""
    _check(gpu, "bunny_full", fmt, lens=0.3)
    _check(gpu, "more_balls", fmt, lens=0.5)


@pytest.mark.parametrize("fmt", ["f32", "q8"])
def test_draw_site_one_bounce(gpu, fmt):
    """max_bounce 1: every sample is the camera's draw and at most one scatter, then a new sample."""
    _check(gpu, "more_balls", fmt, max_bounce=1)


@pytest.mark.parametrize("fmt", ["f32", "q8"])
def test_draw_site_frames_equal_lone_renders(gpu, fmt):
    """Every frame of a 3-frame launch equals its lone render bit for bit (the lanes' rings are reused from unit to
    unit and from frame to frame: no stale block or tail may leak into a later unit)."""
    sc, p = _case("more_balls")
    with gpu.DeviceScene(sc, options={"node_format": fmt}) as ds:
        _assert_same(*_frames_vs_singles(ds, p, 3))
