"""GPU: the per-pixel variance pass (rp_render_variance_device_ws, csrc/rp_variance.hip) against the host model
(rph_batch_variance: the same arithmetic header on the CPU, itself equal to the numpy model in tests/test_denoise_var.py)
fed with the device's own batch frames, bit for bit; its shards, its refusals and its stream behaviour.  The frame is
`variants` at 64 x 48 in 32 x 32 tiles -- rows 32 .. 47 lie in edge tiles with 16 rows of slots outside the frame -- at
samples_per_stream = 4: a batch's frame times 4 (or 2, the partial batch of spp 10) is the batch's sum exactly."""
from dataclasses import replace

import numpy as np
import pytest

import aov_ref
from parity import shard_mask

pytestmark = pytest.mark.gpu

SPS = 4
SENTINEL = -7.0  # a variance is never negative


def _params(spp, **kw):
    sc, p = aov_ref.scene_params("variants", spp, samples_per_stream=SPS)
    return sc, replace(p, **kw)


def _variance_shard(ds, p, workspace=None, stream=None):
    """The beauty render of p's shard on `workspace`, then the variance pass: (rgb, var) shard buffers on the host; the
    variance buffer starts at SENTINEL."""
    import torch
    from rtpotato import _ffi as F
    from rtpotato.scene import shard_slot_count
    n = shard_slot_count(p)
    ds.reserve(p, workspace)
    rgb = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
    var = torch.full((3 * n,), SENTINEL, dtype=torch.float64, device="cuda")
    ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device="cuda")
    ds.render_device(p, rgb, ctr, workspace=workspace, stream=stream)
    ds.render_variance_device(p, var, workspace=workspace, stream=stream)
    torch.cuda.synchronize()
    assert int(ctr[3]) == 0
    return rgb.cpu().numpy(), var.cpu().numpy()


_whole: dict = {}


def _whole_frame(gpu, spp):
    """(rgb, var) full frames of the one-shard render at spp, once per session and shared read-only."""
    if spp not in _whole:
        from rtpotato.render import unpack_shard
        sc, p = _params(spp)
        with gpu.DeviceScene(sc) as ds:
            rgb, var = _variance_shard(ds, p)
        _whole[spp] = (unpack_shard(p, rgb, 3), unpack_shard(p, var, 3), var)
        for a in _whole[spp]:
            a.setflags(write=False)
    return _whole[spp]


@pytest.mark.parametrize("spp", [12, 10])
def test_variance_equals_host_model_on_batch_frames(gpu, spp):
    """spp 12: three batches of 4; spp 10: 4, 4 and a partial batch of 2.  S_b = n_b x the device's frame of batch b
    alone (spp = n_b, seed + b W H); rph_batch_variance of those sums is the device's variance bit for bit, and their
    mean is the device's frame.  Slots of edge tiles outside the frame keep the buffer's old contents."""
    from rtpotato.render import batch_variance_host
    from rtpotato.scene import shard_slot_pixels
    sc, p = _params(spp)
    B = (spp + SPS - 1) // SPS
    rgb, var, var_shard = _whole_frame(gpu, spp)
    with gpu.DeviceScene(sc) as ds:
        sums = []
        for b in range(B):
            nb = min(SPS, spp - b * SPS)
            frame, _, _ = ds.render(replace(p, spp=nb, seed=p.seed + b * p.width * p.height))
            sums.append(float(nb) * frame)
    sums = np.stack(sums, axis=-2)
    x = np.zeros_like(rgb)
    for b in range(B):
        x = x + sums[..., b, :]
    assert np.array_equal(x / float(spp), rgb), "the batch frames do not rebuild the frame"
    ref = batch_variance_host(sums, spp, SPS)
    diff = np.abs(var - ref)
    print(f"spp {spp}: max |device - host| {float(diff.max())}, pixels differing {int((diff > 0).any(-1).sum())}, "
          f"mean variance {float(ref.mean()):.3g}, zero-variance pixels {int((ref == 0).all(-1).sum())}")
    assert np.array_equal(var, ref)
    assert (ref > 0.0).any() and np.isfinite(ref).all()
    idx = shard_slot_pixels(p)
    outside = np.repeat(idx < 0, 3)
    assert outside.sum() == 3 * 2 * 32 * 16
    assert (var_shard[outside] == SENTINEL).all() and (var_shard[~outside] >= 0.0).all()


def test_shards(gpu):
    """num_shards = 3 (4 tiles: shards of 2, 1 and 1), interleaved and balanced after the beauty render on that
    workspace: every shard is the whole frame's pixels bit for bit."""
    from rtpotato import _ffi as F
    from rtpotato.render import unpack_shard
    from rtpotato.scene import shard_slot_pixels
    spp = 12
    sc, p = _params(spp)
    _, whole, _ = _whole_frame(gpu, spp)
    with gpu.DeviceScene(sc) as ds:
        for s in range(3):
            q = replace(p, shard=s, num_shards=3)
            _, var = _variance_shard(ds, q)
            m = shard_mask(q)
            part = unpack_shard(q, var, 3)
            assert np.array_equal(part[m], whole[m]), s
            assert not part[~m].any(), s
        ws = ds.workspace()
        for s in range(3):
            q = replace(p, shard=s, num_shards=3, shard_map=F.RP_SHARD_BALANCED)
            _, var = _variance_shard(ds, q, workspace=ws)
            tmap = ds.tile_map(q, ws)
            idx = shard_slot_pixels(q, tmap)
            m = np.zeros(p.width * p.height, dtype=bool)
            m[idx[idx >= 0]] = True
            m = m.reshape(p.height, p.width)
            assert m.any()
            assert np.array_equal(unpack_shard(q, var, 3, tile_map=tmap)[m], whole[m]), s


def test_refusals(gpu):
    """RP_EINVAL, each with its message and nothing launched: one batch per pixel, a workspace that reserved no batch
    sums, a balanced shard on a workspace that rendered no plan, a NULL buffer."""
    import ctypes

    import torch
    from rtpotato import _ffi as F
    from rtpotato.scene import shard_slot_count
    sc, p = _params(12)
    with gpu.DeviceScene(sc) as ds:
        var = torch.full((3 * shard_slot_count(p),), SENTINEL, dtype=torch.float64, device="cuda")
        ds.reserve(p)
        for one in (replace(p, spp=4), replace(p, spp=3), replace(p, spp=12, samples_per_stream=0)):
            with pytest.raises(F.RPError) as e:
                ds.render_variance_device(one, var)
            assert e.value.code == F.RP_EINVAL and "batches" in str(e.value)
        ws = ds.workspace()
        with pytest.raises(F.RPError) as e:
            ds.render_variance_device(p, var, workspace=ws)
        assert e.value.code == F.RP_EINVAL and "reserve" in str(e.value)
        q = replace(p, shard=1, num_shards=3, shard_map=F.RP_SHARD_BALANCED)
        ds.reserve(q, ws)
        with pytest.raises(F.RPError) as e:
            ds.render_variance_device(q, var, workspace=ws)
        assert e.value.code == F.RP_EINVAL and "plan" in str(e.value)
        c = p.to_c()
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert F.rp().rp_render_variance_device_ws(ds.handle, None, ctypes.byref(c), None, s) == F.RP_EINVAL
        assert F.rp().rp_render_variance_device_ws(None, None, ctypes.byref(c), var.data_ptr(), s) == F.RP_EINVAL
        assert F.rp().rp_render_variance_device_ws(ds.handle, None, None, var.data_ptr(), s) == F.RP_EINVAL
        torch.cuda.synchronize()
        assert bool((var == SENTINEL).all())


def test_asynchronous_call(gpu):
    """On a non-default torch stream, twice into the same buffer: identical bytes, equal to the default stream's."""
    import torch
    from rtpotato import _ffi as F
    from rtpotato.scene import shard_slot_count
    spp = 10
    sc, p = _params(spp)
    _, _, ref = _whole_frame(gpu, spp)
    n = shard_slot_count(p)
    with gpu.DeviceScene(sc) as ds:
        ds.reserve(p)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            rgb = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
            var = torch.full((3 * n,), SENTINEL, dtype=torch.float64, device="cuda")
            ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device="cuda")
            ds.render_device(p, rgb, ctr, stream=st)
            ds.render_variance_device(p, var, stream=st)
            first = var.clone()
            ds.render_variance_device(p, var, stream=st)
        st.synchronize()
        assert torch.equal(first.view(torch.uint8), var.view(torch.uint8))
        assert np.array_equal(var.cpu().numpy(), ref)
