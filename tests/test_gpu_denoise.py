"""GPU: the guided denoiser's kernel (rp_denoise / rp_denoise_device, csrc/rp_denoise.hip) against the host model
(rph_denoise: the same arithmetic header on the CPU, itself equal to the numpy model in tests/test_denoise.py) bit for
bit, asynchronously, end to end behind a render, and its refusals.  The kernel works in 32 x 8 tiles of one residue
class mod 2^l with a halo of 2: 70 x 37 has tile seams and ragged edges at every level, 7 x 5 at L = 5 has classes
with no pixel at all."""
import ctypes

import numpy as np
import pytest

import denoise_ref as R

pytestmark = pytest.mark.gpu

SEED = 20260113


def _host(frame, guides, params):
    from rtpotato.render import denoise_host
    return denoise_host(frame["rgb"], params=params, **guides)


@pytest.mark.parametrize("width,height,iterations,variant",
                         [(70, 37, 5, v) for v in R.VARIANTS] + [(7, 5, 5, v) for v in R.VARIANTS] +
                         [(64, 48, 1, "defaults"), (64, 48, 3, "defaults"), (64, 48, 5, "defaults"),
                          (64, 48, 1, "no_albedo"), (64, 48, 3, "no_color"), (70, 37, 2, "defaults"),
                          (70, 37, 8, "defaults")])
def test_device_equals_host_model(gpu, width, height, iterations, variant):
    """np.array_equal, nothing looser: L = 1 goes from rgb straight to out, L = 2 uses one scratch buffer, L >= 3 both;
    L = 8 has steps up to 128, beyond either side of the frame."""
    frame = R.random_frame(width, height, SEED)
    guides, params = R.variant_inputs(frame, variant, iterations)
    out, seconds = gpu.denoise(frame["rgb"], params=params, **guides)
    ref = _host(frame, guides, params)
    diff = np.abs(out - ref)
    print(width, height, iterations, variant, "max |device - host|", float(diff.max()), "pixels differing",
          int((diff > 0).any(-1).sum()), "device seconds", seconds)
    assert seconds > 0.0
    assert np.array_equal(out, ref)
    if guides["normal"] is not None:
        assert np.array_equal(out[frame["miss"]], frame["rgb"][frame["miss"]])


def test_asynchronous_call(gpu):
    """denoise_device on a non-default torch stream, twice into the same buffers (scratch included): identical bytes,
    equal to the synchronous call."""
    import torch
    frame = R.random_frame(70, 37, SEED)
    params = {"iterations": 4}
    ref, _ = gpu.denoise(frame["rgb"], frame["normal"], frame["albedo"], frame["depth"], params=params)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t = {k: torch.from_numpy(np.array(frame[k])).cuda() for k in ("rgb", "normal", "albedo", "depth")}
        out = torch.zeros((37, 70, 3), dtype=torch.float64, device="cuda")
        scratch = torch.zeros(gpu.denoise_scratch_bytes(70, 37), dtype=torch.uint8, device="cuda")
        gpu.denoise_device(t["rgb"], t["normal"], t["albedo"], t["depth"], out, scratch, params=params, stream=st)
        first = out.clone()
        gpu.denoise_device(t["rgb"], t["normal"], t["albedo"], t["depth"], out, scratch, params=params, stream=st)
    st.synchronize()
    assert torch.equal(first.view(torch.uint8), out.view(torch.uint8))
    assert np.array_equal(out.cpu().numpy(), ref)
    for k in ("rgb", "normal", "albedo", "depth"):  # the inputs are read only
        assert np.array_equal(t[k].cpu().numpy(), frame[k])


def test_end_to_end(gpu):
    """render_denoised on variants_sky at 4 spp: the host model applied to that scene's own render and render_aov
    outputs, bit for bit (so rp_frame_assemble at num_shards = 1 leaves frame order); the 0.6 MSE cap against the
    oracle's 512-spp target; and with bgra=True the to_srgb_u8 bytes of the frame in B, G, R, A order (so
    rp_shard_to_bgra8 serves a frame-order buffer as the shard of a frame tiled width x height)."""
    from rtpotato import _ffi as F
    q = R.quality_case("variants_sky")
    p = q["params"]
    with gpu.DeviceScene(q["scene"]) as ds:
        rgb, _, _ = ds.render(p)
        aov = ds.render_aov(p, foreground=False)
        frame, bgra = ds.render_denoised(p, bgra=True)
        only = ds.render_denoised(p)
        frame, bgra, only = frame.cpu().numpy(), bgra.cpu().numpy(), only.cpu().numpy()
    ref = gpu.denoise_host(rgb, aov["normal"], aov["albedo"], aov["depth"])
    assert frame.shape == (p.height, p.width, 3) and bgra.shape == (p.height, p.width, 4)
    assert np.array_equal(frame, ref) and np.array_equal(only, ref)
    noisy, den = R.mse(rgb, q["target"]), R.mse(frame, q["target"])
    print(f"variants_sky on the device: MSE noisy {noisy:.6g}, denoised {den:.6g}, ratio {den / noisy:.4f}")
    assert den <= R.MSE_CAP * noisy
    rgba = np.empty((p.height, p.width, 4), dtype=np.uint8)
    F.host().rph_to_srgb_u8(np.ascontiguousarray(frame).ctypes.data, p.width * p.height, rgba.ctypes.data)
    assert np.array_equal(bgra, rgba[..., [2, 1, 0, 3]])


def test_refusals(gpu):
    """rp_denoise_device: RP_EINVAL for out aliasing an input, NULL rgb, out or scratch, a zero size and parameters
    out of range; nothing is launched."""
    import torch
    from rtpotato import _ffi as F
    w, h = 16, 8
    rgb = torch.ones((h, w, 3), dtype=torch.float64, device="cuda")
    nrm = torch.ones((h, w, 3), dtype=torch.float64, device="cuda")
    out = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
    scratch = torch.zeros(gpu.denoise_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
    for bad_out in (rgb, nrm):
        with pytest.raises(F.RPError) as e:
            gpu.denoise_device(rgb, nrm, None, None, bad_out, scratch)
        assert e.value.code == F.RP_EINVAL and "alias" in str(e.value)
    L = F.rp()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = [None, w, h, rgb.data_ptr(), nrm.data_ptr(), None, None, out.data_ptr(), scratch.data_ptr(), s]
    # NULL rgb, out, scratch; a zero width, height; scratch over out
    for at, value in ((3, None), (7, None), (8, None), (1, 0), (2, 0), (8, out.data_ptr())):
        args = list(ok)
        args[at] = value
        assert L.rp_denoise_device(*args) == F.RP_EINVAL, at
    bad = F.rp_denoise_params(iterations=9)
    assert L.rp_denoise_device(ctypes.byref(bad), *ok[1:]) == F.RP_EINVAL
    x = np.ones((h, w, 3))
    assert L.rp_denoise(None, 0, w, h, x.ctypes.data, None, None, None, x.ctypes.data, None) == F.RP_EINVAL
    assert L.rp_denoise(None, 0, w, h, None, None, None, None, x.ctypes.data, None) == F.RP_EINVAL
    assert L.rp_denoise_device(*ok) == F.RP_OK
    torch.cuda.synchronize()
    assert torch.equal(out, rgb)  # a constant frame with a constant normal comes back as it is
