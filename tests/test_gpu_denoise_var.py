"""GPU: the variance-guided denoiser's kernel (rp_denoise_var / rp_denoise_var_device, the VAR instantiation of
csrc/rp_denoise.hip's level kernel) against the host model (rph_denoise_var: the same arithmetic header on the CPU,
itself equal to the numpy model in tests/test_denoise_var.py) bit for bit, its refusals, end to end behind a render and
its variance pass, and captured in a graph.  70 x 37 has tile seams and ragged edges at every level, 7 x 5 at L = 5 has
residue classes with no pixel at all."""
import ctypes
from dataclasses import replace

import numpy as np
import pytest

import denoise_ref as R
import denoise_var_ref as V

pytestmark = pytest.mark.gpu

SEED = 20260113


def _inputs(width, height, variant, iterations):
    frame = R.random_frame(width, height, SEED)
    var = V.random_variance(frame, SEED + V.VAR_SEED_OFFSET)
    guides, params = V.variant_inputs(frame, variant, iterations)
    return frame, var, guides, params


@pytest.mark.parametrize("width,height,iterations,variant",
                         [(70, 37, 5, v) for v in V.VARIANTS] + [(7, 5, 5, v) for v in V.VARIANTS] +
                         [(64, 48, 1, "defaults"), (64, 48, 2, "no_albedo"), (64, 48, 3, "defaults"),
                          (70, 37, 8, "defaults")])
def test_device_equals_host_model(gpu, width, height, iterations, variant):
    """np.array_equal, nothing looser, for the synchronous call and the asynchronous one on torch tensors: L = 1 goes
    from rgb and var straight to out, L = 2 uses one colour and one variance buffer of the scratch, L >= 3 both; L = 8
    has steps up to 128, beyond either side of the frame."""
    import torch
    frame, var, guides, params = _inputs(width, height, variant, iterations)
    ref = gpu.denoise_host(frame["rgb"], params=params, variance=var, **guides)
    out, seconds = gpu.denoise(frame["rgb"], params=params, variance=var, **guides)
    diff = np.abs(out - ref)
    print(width, height, iterations, variant, "max |device - host|", float(diff.max()), "pixels differing",
          int((diff > 0).any(-1).sum()), "device seconds", seconds)
    assert seconds > 0.0
    assert np.array_equal(out, ref)
    if guides["normal"] is not None:
        assert np.array_equal(out[frame["miss"]], frame["rgb"][frame["miss"]])
    t = {k: (torch.from_numpy(np.array(g)).cuda() if g is not None else None)
         for k, g in dict(guides, rgb=frame["rgb"], var=var).items()}
    dev = torch.zeros((height, width, 3), dtype=torch.float64, device="cuda")
    gpu.denoise_device(t["rgb"], t["normal"], t["albedo"], t["depth"], dev, params=params, variance=t["var"])
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), ref)
    assert np.array_equal(t["var"].cpu().numpy(), var) and np.array_equal(t["rgb"].cpu().numpy(), frame["rgb"])


def test_refusals(gpu):
    """rp_denoise_var_device: RP_EINVAL for out aliasing an input (var included), scratch over anything -- judged at
    the variance-guided filter's own scratch size, 2 x (24 + 8) bytes per pixel --, NULL rgb, var, out or scratch, a
    zero size and parameters out of range; the wrapper refuses a scratch tensor of rp_denoise's size."""
    import torch
    from rtpotato import _ffi as F
    w, h = 16, 8
    n = w * h
    rgb = torch.ones((h, w, 3), dtype=torch.float64, device="cuda")
    var = torch.ones((h, w, 3), dtype=torch.float64, device="cuda")
    nrm = torch.ones((h, w, 3), dtype=torch.float64, device="cuda")
    out = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
    assert gpu.denoise_var_scratch_bytes(w, h) == 64 * n
    scratch = torch.zeros(gpu.denoise_var_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
    for bad_out in (rgb, nrm, var):
        with pytest.raises(F.RPError) as e:
            gpu.denoise_device(rgb, nrm, None, None, bad_out, scratch, variance=var)
        assert e.value.code == F.RP_EINVAL and "alias" in str(e.value)
    with pytest.raises(AssertionError):
        gpu.denoise_device(rgb, nrm, None, None, out, scratch[:gpu.denoise_scratch_bytes(w, h)], variance=var)
    L = F.rp()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = [None, w, h, rgb.data_ptr(), var.data_ptr(), nrm.data_ptr(), None, None, out.data_ptr(), scratch.data_ptr(), s]
    # one allocation: 6 n doubles, then a frame that the scratch covers only at the variance-guided size (8 n doubles)
    big = torch.zeros(9 * n, dtype=torch.float64, device="cuda")
    behind = big[6 * n:].data_ptr()
    assert L.rp_denoise_device(None, w, h, rgb.data_ptr(), nrm.data_ptr(), None, None, behind, big.data_ptr(), s) == F.RP_OK
    # NULL rgb, var, out, scratch; a zero width, height; scratch over out, over var; out in the scratch's variance part
    for at, value in ((3, None), (4, None), (8, None), (9, None), (1, 0), (2, 0), (9, out.data_ptr()),
                      (9, var.data_ptr()), ((8, 9), (behind, big.data_ptr())), ((4, 9), (behind, big.data_ptr()))):
        args = list(ok)
        for a, v in zip(*((at, value) if isinstance(at, tuple) else ((at,), (value,)))):
            args[a] = v
        assert L.rp_denoise_var_device(*args) == F.RP_EINVAL, at
    for bad in ({"sigma_var": -1.0}, {"var_eps": float("nan")}, {"iterations": 9}):
        assert L.rp_denoise_var_device(ctypes.byref(gpu.denoise_var_params(**bad)), *ok[1:]) == F.RP_EINVAL, bad
    x = np.ones((h, w, 3))
    y = np.ones((h, w, 3))
    assert L.rp_denoise_var(None, 0, w, h, x.ctypes.data, y.ctypes.data, None, None, None, x.ctypes.data, None) == F.RP_EINVAL
    assert L.rp_denoise_var(None, 0, w, h, x.ctypes.data, y.ctypes.data, None, None, None, y.ctypes.data, None) == F.RP_EINVAL
    assert L.rp_denoise_var(None, 0, w, h, x.ctypes.data, None, None, None, None, y.ctypes.data, None) == F.RP_EINVAL
    torch.cuda.synchronize()
    assert not out.any()  # nothing was launched
    assert L.rp_denoise_var_device(*ok) == F.RP_OK
    torch.cuda.synchronize()
    assert torch.equal(out, rgb)  # a constant frame with a constant normal comes back as it is


def _one_tile(p):
    """p with the whole frame as one tile: the compact shard order is the frame order."""
    return replace(p, tile_w=p.width, tile_h=p.height)


def _case():
    import aov_ref
    return aov_ref.scene_params("variants_sky", 8, samples_per_stream=4)


def test_end_to_end(gpu):
    """render_denoised(params, variance=True) on variants_sky at 8 spp in two batches of 4: the host model applied to
    that scene's own render, variance pass and render_aov outputs, bit for bit; one batch per pixel is a ValueError."""
    import torch
    from rtpotato import _ffi as F
    from rtpotato.render import unpack_shard
    from rtpotato.scene import shard_slot_count
    sc, p = _case()
    n = shard_slot_count(p)
    with gpu.DeviceScene(sc) as ds:
        frame = ds.render_denoised(p, variance=True).cpu().numpy()
        narrow = ds.render_denoised(p, variance=True, denoise={"sigma_var": 1.0}).cpu().numpy()
        with pytest.raises(ValueError, match="batches"):
            ds.render_denoised(replace(p, spp=4), variance=True)
        plain = ds.render_denoised(p).cpu().numpy()
        rgb_s = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
        var_s = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
        ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device="cuda")
        ds.reserve(p)
        ds.render_device(p, rgb_s, ctr)
        ds.render_variance_device(p, var_s)
        torch.cuda.synchronize()
        rgb, var = unpack_shard(p, rgb_s.cpu().numpy(), 3), unpack_shard(p, var_s.cpu().numpy(), 3)
        aov = ds.render_aov(p, foreground=False)
    g = {k: aov[k] for k in ("normal", "albedo", "depth")}
    assert frame.shape == (p.height, p.width, 3) and (var > 0.0).any()
    assert np.array_equal(frame, gpu.denoise_host(rgb, variance=var, **g))
    assert np.array_equal(narrow, gpu.denoise_host(rgb, variance=var, params={"sigma_var": 1.0}, **g))
    assert np.array_equal(plain, gpu.denoise_host(rgb, **g)) and not np.array_equal(plain, frame)


def test_graph_capture(gpu):
    """The variance pass and rp_denoise_var_device captured into a torch.cuda.graph as one chain on the capture stream
    (neither allocates or synchronises) after the beauty render left its batch sums: the replay writes the bytes of the
    eager calls.  The frame is one tile, so the pass's shard buffer is the filter's frame-order input."""
    import torch
    from rtpotato import _ffi as F
    sc, p = _case()
    p = _one_tile(p)
    w, h = p.width, p.height
    with gpu.DeviceScene(sc) as ds:
        aov = ds.render_aov(p, foreground=False)
        g = [torch.from_numpy(aov[k]).cuda() for k in ("normal", "albedo", "depth")]
        rgb = torch.zeros(3 * w * h, dtype=torch.float64, device="cuda")
        var = torch.zeros(3 * w * h, dtype=torch.float64, device="cuda")
        out = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
        scratch = torch.zeros(gpu.denoise_var_scratch_bytes(w, h) // 8, dtype=torch.float64, device="cuda")
        ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device="cuda")
        ds.reserve(p)
        ds.render_device(p, rgb, ctr)

        def chain():
            ds.render_variance_device(p, var)
            gpu.denoise_device(rgb, *g, out, scratch, params={"iterations": 4}, variance=var)

        chain()
        torch.cuda.synchronize()
        eager_var, eager_out = var.clone(), out.clone()
        assert bool((eager_var > 0).any()) and bool(eager_out.any())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            chain()
        for _ in range(2):
            var.zero_()
            out.zero_()
            scratch.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(var.view(torch.uint8), eager_var.view(torch.uint8))
            assert torch.equal(out.view(torch.uint8), eager_out.view(torch.uint8))
        del graph
    ref = gpu.denoise_host(rgb.cpu().numpy().reshape(h, w, 3), aov["normal"], aov["albedo"], aov["depth"],
                           params={"iterations": 4}, variance=eager_var.cpu().numpy().reshape(h, w, 3))
    assert np.array_equal(eager_out.cpu().numpy(), ref)
