"""The keystream ring holds decoded values (rp_draw.h value_store / unit_of; rp_device.h ring_values), on the device.

The refill pass stores, for every keystream u64, the double 2 r - 1 with r = (u64 >> 11) 2^-53; the rejection loops
read those doubles, and the jitter and the Bernoulli draw take (v + 1) / 2 of them.  The cases aim at what the stored
form touches besides the loops tests/test_gpu_draw_site.py already drives: a jitter block consumed in part with the
next one never made (spp 6: samples 4 and 5 of block 1, no block 2), both ring sizes (f32: 8 blocks and the mirror
tail; q8: 4 blocks, every value wrapped by itself), one stream per pixel against one stream per sample batch
(samples_per_stream 0 and spp: the fresh unit's block 0 stored into the ring and into jitter slot 0), and a camera
whose UnitDisk values move the ray (lens_radius 0.3).  Every case is a 16 x 8 frame checked against the oracle within
parity.py's bound, with ray, sample and pixel counters exactly equal: one wrong value changes a path and its rays.
"""
from dataclasses import replace

import pytest

from parity import assert_parity, compare, oracle_render

pytestmark = pytest.mark.gpu

W, H = 16, 8
_refs = {}


def _check(gpu, name, fmt, spp, sps=0, lens=None):
    from rtpotato import scenes
    from rtpotato.scene import RenderParams
    sc = scenes.configure(scenes.CATALOGUE[name](), W, H)
    if lens is not None:
        sc = replace(sc, camera=replace(sc.camera, lens_radius=lens))
    p = RenderParams(W, H, spp, 8, scenes.DEFAULT_SEED, samples_per_stream=sps)
    key = (name, spp, sps, lens)
    if key not in _refs:  # one oracle render per case, shared by the node formats
        _refs[key] = oracle_render(sc, p, threads=8)
    ref, _, ctr = _refs[key]
    rgb, _, st = gpu.render(sc, p, options={"node_format": fmt})
    assert_parity(compare(rgb, ref))
    assert st["rays"] == ctr["rays"] and st["samples"] == ctr["samples"] == W * H * spp, (st, ctr)
    assert st["pixels"] == W * H


@pytest.mark.parametrize("fmt", ["f32", "q8"])
def test_values_partial_jitter_block(gpu, fmt):
    """spp 6: jitter block 1 is used for two of its four samples and block 2 is never made."""
    _check(gpu, "more_balls", fmt, 6)


@pytest.mark.parametrize("sps", [0, 16])
def test_values_stream_contracts(gpu, sps):
    """spp 16 as one stream per pixel (samples_per_stream 0) and with samples_per_stream = spp."""
    _check(gpu, "more_balls", "f32", 16, sps=sps)


def test_values_lens_camera(gpu):
    """lens_radius 0.3: the UnitDisk's stored values move the ray's origin and direction."""
    _check(gpu, "bunny_full", "f32", 6, lens=0.3)
