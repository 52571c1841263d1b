"""GPU: progressive accumulation (rp_accum_frames_device, rp_accum_error_device_ws, csrc/rp_accum.hip) against the host
models (rph_accum_frames, rph_accum_error: the same arithmetic header on the CPU, themselves equal to the numpy models in
tests/test_accum.py) bit for bit, on synthetic words of every path of the kernel and on the device's own frames; the
continuation across launches, the error pass's shards and refusals, DeviceScene.render_progressive's stopping rule, streams
and graph capture.  The frame is `variants` at 64 x 48 in 32 x 32 tiles -- rows 32 .. 47 lie in edge tiles with 16 rows of
slots outside the frame -- in frames of 4 spp, one stream per pixel."""
import ctypes
from dataclasses import replace

import numpy as np
import pytest

import accum_ref as A
import aov_ref

pytestmark = pytest.mark.gpu

SPS = 4
SEED = 20260117
GUARD = 2  # words behind every output that must keep their contents


def _params(spp=4, **kw):
    sc, p = aov_ref.scene_params("variants", spp, samples_per_stream=SPS)
    return sc, replace(p, **kw)


def _host_fold(frames, n_frames, n_words, stride, mean=None, m2=None, n_prior=0, want_var=True):
    from rtpotato.render import accum_frames_host
    mean = np.full(n_words, A.PAD) if mean is None else np.array(mean)
    m2 = np.full(n_words, A.PAD) if m2 is None else np.array(m2)
    var = np.full(n_words, A.PAD) if want_var else None
    accum_frames_host(np.ascontiguousarray(frames), n_frames, mean, m2, n_prior=n_prior, var=var, n_words=n_words,
                      stride=stride)
    return mean, m2, var


def _device_fold(frames, n_frames, n_words, stride, mean=None, m2=None, n_prior=0, want_var=True, shift=0, out_shift=0,
                 stream=None):
    """rp_accum_frames_device on a copy of `frames` that starts `shift` doubles into its allocation, outputs `out_shift`
    doubles into theirs and GUARD words short of their end: (mean, m2, var) on the host."""
    import torch
    from rtpotato.render import accum_frames_device
    base = torch.full((shift + frames.size,), A.PAD, dtype=torch.float64, device="cuda")
    base[shift:] = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    outs = []
    for init in (mean, m2, None if want_var else False):
        if init is False:
            outs.append(None)
            continue
        t = torch.full((out_shift + n_words + GUARD,), A.PAD, dtype=torch.float64, device="cuda")
        if init is not None:
            t[out_shift:out_shift + n_words] = torch.from_numpy(np.ascontiguousarray(init)).cuda()
        outs.append(t)
    view = [t[out_shift:] if t is not None else None for t in outs]
    accum_frames_device(base[shift:], n_frames, view[0], view[1], n_prior=n_prior, var=view[2], n_words=n_words,
                        stride=stride, stream=stream)
    torch.cuda.synchronize()
    res = []
    for t in outs:
        if t is None:
            res.append(None)
            continue
        a = t.cpu().numpy()
        assert (a[:out_shift] == A.PAD).all() and (a[out_shift + n_words:] == A.PAD).all(), "wrote outside its words"
        res.append(a[out_shift:out_shift + n_words])
    assert bool((base[:shift] == A.PAD).all())
    return res


def _same(got, ref):
    return all((g is None and r is None) or A.same_bits(g, r) for g, r in zip(got, ref))


@pytest.mark.parametrize("n_words", [1, 2, 3, 127, 129, 2 * 64 * 256 + 1])
def test_kernel_equals_host_model(gpu, n_words):
    """n_frames 1, 2, 3, 5 (below, at and above the group of four whose loads fly together) at stride = n_words and
    n_words + 5: one of the two strides is even -- the 16-byte path, with the scalar walk for an odd last word -- and
    the other odd, the scalar path throughout.  129 words end inside a wave, 2 x 64 x 256 + 1 words take 65 blocks
    whose last has one lane with one word."""
    for n_frames in (1, 2, 3, 5):
        for pad in (0, 5):
            stride = n_words + pad
            frames = A.synthetic(n_frames, n_words, stride, SEED + 100 * n_frames + n_words)
            ref = _host_fold(frames, n_frames, n_words, stride, want_var=n_frames >= 2)
            got = _device_fold(frames, n_frames, n_words, stride, want_var=n_frames >= 2)
            assert _same(got, ref), (n_frames, pad)
            if n_frames == 1:
                assert A.same_bits(got[0], frames[:n_words])


@pytest.mark.parametrize("n_words", [2, 129, 1000])
def test_misaligned_buffers_and_continuation(gpu, n_words):
    """Frames that start one double into their allocation, outputs that do, and both, at an even stride: the scalar
    path, the same bits.  Five frames at once against two, then three with n_prior = 2."""
    stride = n_words + (n_words % 2)
    frames = A.synthetic(5, n_words, stride, SEED + 9)
    ref = _host_fold(frames, 5, n_words, stride)
    for shift, out_shift in ((0, 0), (1, 0), (0, 1), (1, 1)):
        assert _same(_device_fold(frames, 5, n_words, stride, shift=shift, out_shift=out_shift), ref), (shift, out_shift)
        mean, m2, _ = _device_fold(frames, 2, n_words, stride, want_var=False, shift=shift, out_shift=out_shift)
        part = _device_fold(frames[2 * stride:], 3, n_words, stride, mean=mean, m2=m2, n_prior=2, shift=shift,
                            out_shift=out_shift)
        assert _same(part, ref), (shift, out_shift)


def test_frames_refusals(gpu):
    """Each RP_EINVAL case of rp_accum_frames_device with its message, nothing launched."""
    import torch
    from rtpotato import _ffi as F
    L = F.rp()
    fr = torch.ones(40, dtype=torch.float64, device="cuda")
    out = torch.full((3, 8), A.PAD, dtype=torch.float64, device="cuda")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t, off=0: None if t is None else t.data_ptr() + 8 * off

    def call(n_words=4, n_prior=0, n_frames=3, frames=ptr(fr), stride=4, mean=ptr(out[0]), m2=ptr(out[1]),
             var=ptr(out[2])):
        return L.rp_accum_frames_device(n_words, n_prior, n_frames, frames, stride, mean, m2, var, s)

    for kw, msg in (({"frames": None}, b"non-NULL"), ({"mean": None}, b"non-NULL"), ({"m2": None}, b"non-NULL"),
                    ({"n_frames": 0}, b"n_frames is zero"), ({"n_words": 0}, b"n_words is zero"),
                    ({"stride": 3}, b"frame_stride"), ({"n_frames": 1}, b"at least two frames"),
                    ({"n_prior": 2 ** 31 - 3}, b"2^31 - 1"), ({"n_words": 2 ** 40, "stride": 2 ** 40}, b"2^40 - 512"),
                    ({"mean": ptr(fr, 8)}, b"alias the frames"), ({"m2": ptr(fr, 11)}, b"alias the frames"),
                    ({"var": ptr(fr, 1)}, b"alias the frames"), ({"m2": ptr(out[0])}, b"one another"),
                    ({"var": ptr(out[1], 3)}, b"one another")):
        assert call(**kw) == F.RP_EINVAL, kw
        assert msg in L.rp_last_error(), (kw, L.rp_last_error())
    torch.cuda.synchronize()
    assert bool((out == A.PAD).all()) and bool((fr == 1.0).all())
    assert call(mean=ptr(fr, 12)) == F.RP_OK  # the word after the frames does not alias them
    torch.cuda.synchronize()
    assert bool((fr[12:16] == 1.0).all()) and bool((out[1, :4] == 0.0).all()) and bool((out[2, :4] == 0.0).all())


def test_frames_refusals_are_the_host_library_s(gpu):
    """test_frames_refusals' table through both libraries, each on buffers of its own with the same layout (40 words of
    frames, three 8-word outputs; a pointer is a buffer and an offset in words): rp_accum_frames_device's message is
    rph_accum_frames' after its prefix -- rp_accum.h's check_fold, compiled into both -- and neither call writes."""
    import torch
    from rtpotato import _ffi as F
    L, H = F.rp(), F.host()
    dev = {"fr": torch.ones(40, dtype=torch.float64, device="cuda"),
           "out": torch.full((3, 8), A.PAD, dtype=torch.float64, device="cuda")}
    host = {"fr": np.ones(40), "out": np.full((3, 8), A.PAD)}
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    base = lambda bufs, name: bufs[name].data_ptr() if bufs is dev else bufs[name].ctypes.data
    ok = dict(n_words=4, n_prior=0, n_frames=3, frames=("fr", 0), stride=4, mean=("out", 0), m2=("out", 8), var=("out", 16))

    def call(bufs, **kw):
        a = {**ok, **kw}
        ptr = [None if a[k] is None else base(bufs, a[k][0]) + 8 * a[k][1] for k in ("frames", "mean", "m2", "var")]
        if bufs is dev:
            rc = L.rp_accum_frames_device(a["n_words"], a["n_prior"], a["n_frames"], ptr[0], a["stride"], *ptr[1:], s)
            return rc, L.rp_last_error()
        rc = H.rph_accum_frames(a["n_words"], a["n_prior"], a["n_frames"], ptr[0], a["stride"], *ptr[1:])
        return rc, H.rph_last_error()

    for kw in ({"frames": None}, {"mean": None}, {"m2": None}, {"n_frames": 0}, {"n_words": 0}, {"stride": 3},
               {"n_frames": 1}, {"n_prior": 2 ** 31 - 3}, {"n_words": 2 ** 40, "stride": 2 ** 40}, {"mean": ("fr", 8)},
               {"m2": ("fr", 11)}, {"var": ("fr", 1)}, {"m2": ("out", 0)}, {"var": ("out", 11)}):
        (rc_d, msg_d), (rc_h, msg_h) = call(dev, **kw), call(host, **kw)
        assert rc_d == rc_h == F.RP_EINVAL, kw
        assert msg_h == b"rph_accum_frames: " + msg_d and msg_d, (kw, msg_d, msg_h)
    torch.cuda.synchronize()
    assert bool((dev["out"] == A.PAD).all()) and bool((dev["fr"] == 1.0).all())
    assert (host["out"] == A.PAD).all() and (host["fr"] == 1.0).all()


_chain: dict = {}


def _render_chain(gpu):
    """Once per session, shared read-only: the 4-frame launch at 4 spp, its fold on the device, and the unpacked
    frames."""
    if not _chain:
        import torch
        from rtpotato import _ffi as F
        from rtpotato.render import accum_frames_device, unpack_shard
        from rtpotato.scene import shard_slot_count
        sc, p = _params()
        n = shard_slot_count(p)
        with gpu.DeviceScene(sc) as ds:
            ds.reserve_frames(p, 4)
            frames = torch.full((4 * 3 * n,), float("nan"), dtype=torch.float64, device="cuda")
            mean, m2, var = (torch.full((3 * n,), A.PAD, dtype=torch.float64, device="cuda") for _ in range(3))
            ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device="cuda")
            ds.render_frames_device(p, 4, frames, ctr)
            accum_frames_device(frames, 4, mean, m2, var=var)
            torch.cuda.synchronize()
            assert int(ctr[3]) == 0
        _chain.update(frames=frames.cpu().numpy(), **{k: t.cpu().numpy() for k, t in
                                                      (("mean", mean), ("m2", m2), ("var", var))})
        for k in ("mean", "m2", "var"):
            _chain[k + "_frame"] = unpack_shard(p, _chain[k], 3)
        for a in _chain.values():
            a.setflags(write=False)
    return _chain


def test_frames_against_a_plain_render(gpu):
    """Four frames of 4 spp are the four batches of rp_render at 16 spp and samples_per_stream = 4: the folded mean is
    its frame to rtol 1e-12 (a running mean against a sum divided once: a few ulps), the folded variance its batch
    variance under tests/test_accum.py's derived tolerance -- rtol 1e-9 where sigma / m >= 1e-6, atol 1e-12 max(frame)^2
    below.  The fold of the device's frames is the host model's, bit for bit, whatever the slots outside the frame carry."""
    import torch
    from rtpotato import _ffi as F
    from rtpotato.render import unpack_shard
    from rtpotato.scene import shard_slot_count, shard_slot_pixels
    c = _render_chain(gpu)
    sc, p = _params()
    p16 = replace(p, spp=16)
    n = shard_slot_count(p)
    assert _same(_host_fold(c["frames"], 4, 3 * n, 3 * n), (c["mean"], c["m2"], c["var"]))
    outside = np.repeat(shard_slot_pixels(p) < 0, 3)
    assert outside.sum() == 3 * 2 * 32 * 16
    assert np.isfinite(c["mean"][~outside]).all() and (c["var"][~outside] >= 0.0).all() and (c["var"] > 0.0).any()
    with gpu.DeviceScene(sc) as ds:
        rgb, _, _ = ds.render(p16)
        ds.reserve(p16)
        d_rgb = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
        d_var = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
        ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device="cuda")
        ds.render_device(p16, d_rgb, ctr)
        ds.render_variance_device(p16, d_var)
        torch.cuda.synchronize()
        var = unpack_shard(p16, d_var.cpu().numpy(), 3)
    scale = float(rgb.max())
    dm, dv = np.abs(c["mean_frame"] - rgb), np.abs(c["var_frame"] - var)
    print("mean: max relative difference", float((dm / np.maximum(np.abs(rgb), 1e-300)).max()),
          "variance: max relative", float((dv / np.maximum(var, 1e-300))[var > 0].max()), "max absolute", float(dv.max()))
    assert np.allclose(c["mean_frame"], rgb, rtol=1e-12, atol=0.0)
    assert np.allclose(c["var_frame"], var, rtol=1e-9, atol=1e-12 * scale * scale)


def test_continuation_across_launches(gpu):
    """Two launches of two frames, the second at seed + 2 W H, folded with n_prior = 2: the 4-frame launch's mean, m2
    and variance bit for bit."""
    import torch
    from rtpotato import _ffi as F
    from rtpotato.render import accum_frames_device
    from rtpotato.scene import shard_slot_count
    c = _render_chain(gpu)
    sc, p = _params()
    n = shard_slot_count(p)
    with gpu.DeviceScene(sc) as ds:
        ds.reserve_frames(p, 2)
        frames = torch.full((2 * 3 * n,), float("nan"), dtype=torch.float64, device="cuda")
        mean, m2, var = (torch.full((3 * n,), A.PAD, dtype=torch.float64, device="cuda") for _ in range(3))
        ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device="cuda")
        ds.render_frames_device(p, 2, frames, ctr)
        accum_frames_device(frames, 2, mean, m2)
        ds.render_frames_device(replace(p, seed=p.seed + 2 * p.width * p.height), 2, frames, ctr)
        accum_frames_device(frames, 2, mean, m2, n_prior=2, var=var)
        torch.cuda.synchronize()
        assert int(ctr[3]) == 0
    assert _same((mean.cpu().numpy(), m2.cpu().numpy(), var.cpu().numpy()), (c["mean"], c["m2"], c["var"]))


def _pack(whole, idx):
    """A compact shard buffer of the frame `whole` (h, w, 3) for the slot map idx: NaN in slots outside the frame."""
    buf = np.full((len(idx), 3), np.nan)
    buf[idx >= 0] = whole.reshape(-1, 3)[idx[idx >= 0]]
    return buf.reshape(-1)


def test_error_pass(gpu):
    """The whole frame's statistics are rph_accum_error's on the unpacked frames, exactly, at the default and at
    explicit parameters; 64 x 48 pixels are counted, so the 2 x 32 x 16 outside slots -- NaN here -- are not.  Shards
    0 .. 2 of 3, interleaved and balanced after a render on that workspace: each is the host model's on its pixels, their
    pixels, overs and non-finites sum to the frame's and the frame's maximum is the largest of theirs.  A balanced shard
    without a plan, NULL buffers and parameters out of range are refused."""
    import torch
    from rtpotato import _ffi as F
    from rtpotato.render import accum_error_host, error_stats
    from rtpotato.scene import shard_slot_count, shard_slot_pixels
    c = _render_chain(gpu)
    sc, p = _params()
    mean_f, var_f = c["mean_frame"], c["var_frame"]
    stats = torch.full((F.RP_ERROR_STATS_LEN,), -1, dtype=torch.int64, device="cuda")
    idx0 = shard_slot_pixels(p)
    wm, wv = _pack(mean_f, idx0), _pack(var_f, idx0)  # the whole frame's shard buffers, NaN outside the frame
    assert (idx0 < 0).sum() == 2 * 32 * 16 and A.same_bits(wm[np.repeat(idx0 >= 0, 3)], c["mean"][np.repeat(idx0 >= 0, 3)])

    def run(ds, q, mean, var, ws=None, **kw):
        ds.accum_error_device(q, torch.from_numpy(np.array(mean)).cuda(), torch.from_numpy(np.array(var)).cuda(), stats,
                              workspace=ws, **kw)
        torch.cuda.synchronize()
        return stats.cpu().numpy().astype(np.uint64)

    with gpu.DeviceScene(sc) as ds:
        for kw in ({}, {"tol": 0.02}, {"tol": 0.3, "eps": 1e-2}, {"tol": 1e-6, "eps": 1e-12}):
            got, ref = run(ds, p, wm, wv, **kw), accum_error_host(mean_f, var_f, **kw)
            print(kw, error_stats(got))
            assert got.tolist() == ref.tolist(), kw
            assert got[0] == 64 * 48 and got[3] == 0 and got[2] > 0
        whole = accum_error_host(mean_f, var_f)
        assert 0 < whole[1] < whole[0]
        # a non-finite pixel inside the frame is counted as one
        bad = np.array(wv)
        first = int(np.flatnonzero(idx0 >= 0)[0])
        bad[3 * first] = np.inf
        got = run(ds, p, wm, bad)
        assert (got[0], got[1], got[3]) == (whole[0], whole[1] + (0 if _over(mean_f, var_f, first, p) else 1), 1)
        for balanced in (False, True):
            ws = ds.workspace() if balanced else None
            parts = []
            for s in range(3):
                q = replace(p, shard=s, num_shards=3, shard_map=F.RP_SHARD_BALANCED if balanced else F.RP_SHARD_INTERLEAVE)
                tmap = None
                if balanced:  # the beauty render of this shard leaves the plan the pass decodes its slots with
                    ds.reserve(q, ws)
                    rgb = torch.zeros(3 * shard_slot_count(q), dtype=torch.float64, device="cuda")
                    ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device="cuda")
                    ds.render_device(q, rgb, ctr, workspace=ws)
                    torch.cuda.synchronize()
                    tmap = ds.tile_map(q, ws)
                idx = shard_slot_pixels(q, tmap)
                inside = idx[idx >= 0]
                got = run(ds, q, _pack(mean_f, idx), _pack(var_f, idx), ws=ws)
                ref = accum_error_host(mean_f.reshape(-1, 3)[inside], var_f.reshape(-1, 3)[inside])
                assert got.tolist() == ref.tolist(), (balanced, s)
                assert got[0] == len(inside) > 0
                parts.append(got)
            parts = np.array(parts)
            assert parts[:, 0].sum() == whole[0] == 64 * 48 and parts[:, 1].sum() == whole[1]
            assert parts[:, 2].max() == whole[2] and parts[:, 3].sum() == whole[3] == 0
        q = replace(p, shard=1, num_shards=3, shard_map=F.RP_SHARD_BALANCED)
        ws2 = ds.workspace()
        ds.reserve(q, ws2)
        idx = shard_slot_pixels(q)
        stats.fill_(-1)
        with pytest.raises(F.RPError) as e:
            run(ds, q, _pack(mean_f, idx), _pack(var_f, idx), ws=ws2)
        assert e.value.code == F.RP_EINVAL and "plan" in str(e.value)
        for kw in ({"tol": -1.0}, {"eps": -1e-4}, {"eps": float("inf")}, {"tol": float("nan")}):
            with pytest.raises(F.RPError) as e:
                run(ds, p, wm, wv, **kw)
            assert e.value.code == F.RP_EINVAL and "out of range" in str(e.value)
        pc = p.to_c()
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        d = torch.from_numpy(np.array(c["mean"])).cuda()
        L = F.rp()
        assert L.rp_accum_error_device_ws(ds.handle, None, ctypes.byref(pc), None, None, d.data_ptr(), stats.data_ptr(), s) == F.RP_EINVAL
        assert L.rp_accum_error_device_ws(ds.handle, None, ctypes.byref(pc), None, d.data_ptr(), None, stats.data_ptr(), s) == F.RP_EINVAL
        assert L.rp_accum_error_device_ws(ds.handle, None, ctypes.byref(pc), None, d.data_ptr(), d.data_ptr(), None, s) == F.RP_EINVAL
        assert L.rp_accum_error_device_ws(None, None, ctypes.byref(pc), None, d.data_ptr(), d.data_ptr(), stats.data_ptr(), s) == F.RP_EINVAL
        torch.cuda.synchronize()
        assert bool((stats == -1).all())  # a refused call does not touch the statistics


def test_error_pass_above_the_grid_cap(gpu):
    """1000 x 530 in 32 x 32 tiles is 544 tiles, 557,056 slots: more than 2048 blocks of 256, so every block walks a
    second stretch of slots and the last stretch is ragged.  Seeded frames with dark pixels, zero, negative, infinite and
    NaN variances and a NaN mean (no render: the pass reads what it is given), NaN in the 27,056 slots outside the frame;
    the statistics are the host model's, exactly."""
    import torch
    from rtpotato import _ffi as F
    from rtpotato.render import accum_error_host, error_stats
    from rtpotato.scene import shard_slot_count, shard_slot_pixels
    sc, p = _params()
    q = replace(p, width=1000, height=530)
    idx = shard_slot_pixels(q)
    assert len(idx) == shard_slot_count(q) == 544 * 1024 > 2048 * 256 and (idx < 0).sum() == 544 * 1024 - 1000 * 530
    mean, var = A.synthetic_error_frames(1000 * 530, SEED + 3)
    ref = accum_error_host(mean, var)
    stats = torch.full((F.RP_ERROR_STATS_LEN,), -1, dtype=torch.int64, device="cuda")
    with gpu.DeviceScene(sc) as ds:
        ds.accum_error_device(q, torch.from_numpy(_pack(mean, idx)).cuda(), torch.from_numpy(_pack(var, idx)).cuda(), stats)
        torch.cuda.synchronize()
    got = stats.cpu().numpy().astype(np.uint64)
    print(error_stats(got))
    assert got.tolist() == ref.tolist()
    assert got[0] == 1000 * 530 and 0 < got[1] < got[0] and got[3] == 3


def _over(mean_f, var_f, slot, p):
    """Whether the pixel of whole-frame slot `slot` is over at the defaults (host model on that one pixel)."""
    from rtpotato.render import accum_error_host
    from rtpotato.scene import shard_slot_pixels
    i = int(shard_slot_pixels(p)[slot])
    return bool(accum_error_host(mean_f.reshape(-1, 3)[i:i + 1], var_f.reshape(-1, 3)[i:i + 1])[1])


def test_render_progressive(gpu):
    """A huge tolerance stops after the first launch; a tiny one runs to max_frames = 6 at 4 frames per launch, as
    launches of 4 and 2.  Mean and variance are the hand-made chain's bit for bit, two calls give the same bytes, and
    `denoised` is denoise_device(variance=...) on the returned buffers with the guides at spp = 24."""
    import torch
    from rtpotato import _ffi as F
    from rtpotato.render import accum_error_host, accum_frames_device, denoise_device, error_stats, unpack_shard
    from rtpotato.scene import shard_slot_count
    c = _render_chain(gpu)
    sc, p = _params()
    n = shard_slot_count(p)
    with gpu.DeviceScene(sc) as ds:
        one = ds.render_progressive(p, tol=1e6, denoise=False)
        assert one["frames"] == 4 and len(one["stats"]) == 1 and "denoised" not in one
        assert one["stats"][0][:3] == (4, 64 * 48, 0) and one["stats"][0][4] == 0
        assert A.same_bits(one["mean"].cpu().numpy(), c["mean_frame"])
        assert A.same_bits(one["variance"].cpu().numpy(), c["var_frame"])
        out = ds.render_progressive(p, frames_per_launch=4, max_frames=6, tol=1e-9)
        again = ds.render_progressive(p, frames_per_launch=4, max_frames=6, tol=1e-9)
        assert out["frames"] == 6 and [s[0] for s in out["stats"]] == [4, 6]
        assert out["stats"][0] == (4,) + error_stats(accum_error_host(c["mean_frame"], c["var_frame"], tol=1e-9))
        assert out["stats"][1][2] > 0.01 * 64 * 48  # still over: max_frames ended it
        for k in ("mean", "variance", "denoised"):
            assert out[k].shape == (p.height, p.width, 3)
            assert torch.equal(out[k].view(torch.uint8), again[k].view(torch.uint8)), k
        assert out["stats"] == again["stats"]
        # the chain by hand: 4 frames at seed, 2 at seed + 4 W H
        ds.reserve_frames(p, 4)
        frames = torch.zeros(4 * 3 * n, dtype=torch.float64, device="cuda")
        mean, m2, var = (torch.zeros(3 * n, dtype=torch.float64, device="cuda") for _ in range(3))
        ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device="cuda")
        ds.render_frames_device(p, 4, frames, ctr)
        accum_frames_device(frames, 4, mean, m2)
        ds.render_frames_device(replace(p, seed=p.seed + 4 * p.width * p.height), 2, frames, ctr)
        accum_frames_device(frames, 2, mean, m2, n_prior=4, var=var, n_words=3 * n)
        torch.cuda.synchronize()
        assert np.array_equal(out["mean"].cpu().numpy(), unpack_shard(p, mean.cpu().numpy(), 3))
        assert np.array_equal(out["variance"].cpu().numpy(), unpack_shard(p, var.cpu().numpy(), 3))
        aov = ds.render_aov(replace(p, spp=24), foreground=False)
        g = [torch.from_numpy(aov[k]).cuda() for k in ("normal", "albedo", "depth")]
        ref = torch.zeros_like(out["denoised"])
        denoise_device(out["mean"], *g, ref, variance=out["variance"])
        torch.cuda.synchronize()
        assert torch.equal(out["denoised"].view(torch.uint8), ref.view(torch.uint8))
        assert not torch.equal(out["denoised"], out["mean"])
        for bad in ({"frames_per_launch": 0}, {"frames_per_launch": 1}, {"max_frames": 1}, {"tol": 0.0}):
            with pytest.raises(ValueError):
                ds.render_progressive(p, **bad)
        with pytest.raises(ValueError, match="num_shards"):
            ds.render_progressive(replace(p, num_shards=2))


def test_asynchronous_calls(gpu):
    """On a non-default torch stream, twice into the same buffers: identical bytes, equal to the default stream's."""
    import torch
    from rtpotato import _ffi as F
    from rtpotato.render import accum_error_host, accum_frames_device
    c = _render_chain(gpu)
    sc, p = _params()
    with gpu.DeviceScene(sc) as ds:
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            frames = torch.from_numpy(np.array(c["frames"])).cuda()
            mean, m2, var = (torch.full((frames.numel() // 4,), A.PAD, dtype=torch.float64, device="cuda")
                             for _ in range(3))
            stats = torch.full((F.RP_ERROR_STATS_LEN,), -1, dtype=torch.int64, device="cuda")
            runs = []
            for _ in range(2):
                accum_frames_device(frames, 4, mean, m2, var=var, stream=st)
                ds.accum_error_device(p, mean, var, stats, stream=st)
                runs.append([t.clone() for t in (mean, m2, var, stats)])
        st.synchronize()
        for a, b in zip(*runs):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        assert _same([t.cpu().numpy() for t in runs[1][:3]], (c["mean"], c["m2"], c["var"]))
        assert runs[1][3].cpu().numpy().astype(np.uint64).tolist() == \
            accum_error_host(c["mean_frame"], c["var_frame"]).tolist()


def test_graph_capture(gpu):
    """The accumulate and error calls alone, captured once into a torch.cuda.graph as one chain on the capture stream
    (neither allocates or synchronises): the replay writes the bytes of the eager calls."""
    import torch
    from rtpotato import _ffi as F
    from rtpotato.render import accum_frames_device
    c = _render_chain(gpu)
    sc, p = _params()
    with gpu.DeviceScene(sc) as ds:
        frames = torch.from_numpy(np.array(c["frames"])).cuda()
        mean, m2, var = (torch.full((frames.numel() // 4,), A.PAD, dtype=torch.float64, device="cuda") for _ in range(3))
        stats = torch.full((F.RP_ERROR_STATS_LEN,), -1, dtype=torch.int64, device="cuda")

        def chain():
            accum_frames_device(frames, 4, mean, m2, var=var)
            ds.accum_error_device(p, mean, var, stats)

        chain()
        torch.cuda.synchronize()
        eager = [t.clone() for t in (mean, m2, var, stats)]
        assert int(eager[3][0]) == 64 * 48
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            chain()
        for _ in range(2):
            for t in (mean, m2, var):
                t.fill_(A.PAD)
            stats.fill_(-1)
            graph.replay()
            torch.cuda.synchronize()
            for t, e in zip((mean, m2, var, stats), eager):
                assert torch.equal(t.view(torch.uint8), e.view(torch.uint8))
        del graph
