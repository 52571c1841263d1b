"""The references of the first-hit feature pass agree with each other on the CPU (tests/aov_ref.py), and the pass is
part of the C-ABI.  The depth reference (c) rebuilds every camera ray in numpy; before it judges the GPU
(tests/test_gpu_aov.py) it is checked here against the reference renderer's own first hits (a): the same pixels hit,
and the same normals bit for bit -- so the rebuilt rays are the renderer's rays."""
import ctypes

import numpy as np
import pytest

import aov_ref


@pytest.mark.parametrize("name", aov_ref.PINHOLE)
def test_reconstructed_rays_are_the_renderers(name):
    r = aov_ref.refs(name, 1)
    hit = np.isfinite(r["depth"]) & (r["depth_fg"] > 0)
    assert np.array_equal(r["depth_fg"], r["fg"])            # hit flags against the renderer's foreground
    assert np.array_equal(r["depth_normal"], r["normal"])    # bit for bit (1 spp: one sample's normal / 1.0)
    assert 0 < hit.sum() and np.all(r["depth"][hit] > 1e-3) and np.all(r["depth"][~hit] == 0.0)
    assert np.all(r["albedo"][~hit] == 0.0) and np.all(r["normal"][~hit] == 0.0)


def test_references_at_4_spp_have_partial_coverage():
    """4 spp: sums in sample order; every frame has pixels some of whose samples miss (the edge case of the rule
    `a miss adds zero`), and (c) still agrees with (a)."""
    for name in ("bunny_full", "variants"):
        r = aov_ref.refs(name, 4)
        partial = (r["fg"] > 0) & (r["fg"] < 1)
        assert partial.sum() >= 20, (name, int(partial.sum()))
        assert np.array_equal(r["depth_fg"], r["fg"])
        assert np.array_equal(r["depth_normal"], r["normal"])


def test_albedo_reference_covers_every_absorb():
    """The substitution (b): Albedo colours come out exactly, AlbedoMap through the texture at the hit record."""
    r = aov_ref.refs("bunny_full", 1)
    flat = r["albedo"].reshape(-1, 3)
    for c in ((0.7, 0.8, 0.7), (0.8, 0.8, 0.8), (0.8, 0.6, 0.2)):  # glass bunny, ground, mirror ball
        assert np.any(np.all(flat == np.array(c), axis=1)), c
    # the earth ball's image texels: bytes / 255
    tex = flat[(r["fg"].reshape(-1) > 0) & ~np.any([np.all(flat == np.array(c), axis=1)
                                                    for c in ((0.7, 0.8, 0.7), (0.8, 0.8, 0.8), (0.8, 0.6, 0.2))], axis=0)]
    assert len(tex) > 0 and np.allclose(tex * 255.0, np.round(tex * 255.0), atol=1e-9)


def test_abi_has_the_feature_pass():
    """rp_render_aov refuses a NULL scene with RP_EINVAL on a host without a GPU; the export test of test_abi.py
    covers the header-to-bindings match."""
    from rtpotato import _ffi as F
    from rtpotato.scene import RenderParams
    L = F.rp()
    p = RenderParams(8, 8, 1).to_c()
    buf = np.zeros(8 * 8 * 3)
    assert L.rp_render_aov(None, None, ctypes.byref(p), buf.ctypes.data, None, None, None, None) == F.RP_EINVAL
    assert L.rp_render_aov_device_ws(None, None, None, ctypes.byref(p), None, None, None, None, None,
                                     None) == F.RP_EINVAL
    assert "rp_render_aov" in F.RP_SYMBOLS and "rp_render_aov_device_ws" in F.RP_SYMBOLS
