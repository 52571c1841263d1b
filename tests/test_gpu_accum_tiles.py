"""GPU: tile-adaptive progressive rendering (rp_render_tiles_device_ws, rp_accum_tiles_select_device,
rp_accum_frames_tiles_device, DeviceScene.render_adaptive).  The tile-list launch against
render_frames_device's frames bit for bit, the two selection kernels and the tile fold against the host models
(rph_accum_tiles_select, rph_accum_frames_tiles: equal to the numpy models in tests/test_accum_tiles.py) exactly, and the
whole loop against its replay on the host from frames rendered once.  The frame is `variants` at 80 x 48 in 32 x 32 tiles
-- 3 x 2 tiles, the right column 16 pixels wide and the bottom row 16 high -- in frames of 4 spp, one stream per pixel."""
import ctypes
from dataclasses import replace

import numpy as np
import pytest

import accum_ref as A
import accum_tiles_ref as T
import aov_ref

pytestmark = pytest.mark.gpu

W, H, TW, TH = 80, 48, 32, 32
TILE_PX, N_TILES = TW * TH, 6
SPP = 4
MAX_FRAMES = 12
SEED = 20260219
GUARD = 2
ORDERS = ("auto", "sequential", "interleaved", "pixel")

_shared = {}


def _params(**kw):
    from rtpotato import scenes
    sc, p = aov_ref.scene_params("variants", SPP, samples_per_stream=SPP)
    return scenes.configure(sc, W, H), replace(p, width=W, height=H, **kw)


def _frames(gpu):
    """Once per session, shared read-only: MAX_FRAMES whole frames in one launch (frame f at seed + f W H; compact
    buffers, slots outside the frame at PAD) and the counters of a 3-frame launch."""
    if not _shared:
        import torch
        from rtpotato import _ffi as F
        sc, p = _params()
        n = N_TILES * TILE_PX
        with gpu.DeviceScene(sc) as ds:
            frames = torch.full((MAX_FRAMES * 3 * n,), A.PAD, dtype=torch.float64, device="cuda")
            ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device="cuda")
            ds.render_frames_device(p, MAX_FRAMES, frames, ctr)
            torch.cuda.synchronize()
            assert int(ctr[3]) == 0
            three = torch.full((3 * 3 * n,), A.PAD, dtype=torch.float64, device="cuda")
            ctr3 = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device="cuda")
            ds.render_frames_device(p, 3, three, ctr3)
            torch.cuda.synchronize()
        _shared.update(frames=frames.cpu().numpy().reshape(MAX_FRAMES, N_TILES, TILE_PX, 3), ctr3=ctr3.cpu().numpy())
        assert A.same_bits(three.cpu().numpy(), _shared["frames"][:3].reshape(-1))
        for a in _shared.values():
            a.setflags(write=False)
    return _shared


# ---- the tile-list launch

def _render_tiles(ds, p, tiles, n_frames, order, ws=None):
    import torch
    from rtpotato import _ffi as F
    n = len(tiles) * TILE_PX
    out = torch.full((n_frames * 3 * n + GUARD,), A.PAD, dtype=torch.float64, device="cuda")
    ctr = torch.full((F.RP_COUNTERS_LEN,), -1, dtype=torch.int64, device="cuda")
    d_tiles = torch.from_numpy(np.array(tiles, dtype=np.uint32).view(np.int32)).cuda()
    ds.render_tiles_device(p, d_tiles, len(tiles), n_frames, out, ctr, order=order, workspace=ws)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[n_frames * 3 * n:] == A.PAD).all(), "wrote behind its frames"
    return o[:n_frames * 3 * n].reshape(n_frames, len(tiles), TILE_PX, 3), ctr.cpu().numpy()


@pytest.mark.parametrize("order", ORDERS)
def test_render_tiles_equals_the_full_launch(gpu, order):
    """[5, 0, 6, 3] over 3 frames: tiles 5, 0 and 3 bit for bit the frames' own, entry 6 (not a tile of the frame) and
    every slot outside the frame left at the guard pattern; samples = spp x in-frame pixels x frames.  Then the full
    list: the whole launch again, with its ray count."""
    c = _frames(gpu)
    sc, p = _params()
    _, _, _, inside = T.grid(W, H, TW, TH)
    tiles = [5, 0, 6, 3]
    with gpu.DeviceScene(sc) as ds:
        got, ctr = _render_tiles(ds, p, tiles, 3, order)
        assert ds.frame_info() == 0
        full, ctr_full = _render_tiles(ds, p, list(range(N_TILES)), 3, order)
    px = 0
    for k, t in enumerate(tiles):
        if t >= N_TILES:
            assert (got[:, k] == A.PAD).all(), "an entry outside the frame was written"
            continue
        assert A.same_bits(got[:, k][:, inside[t]], c["frames"][:3, t][:, inside[t]]), (order, t)
        assert (got[:, k][:, ~inside[t]] == A.PAD).all(), "a slot outside the frame was written"
        px += int(inside[t].sum())
    assert px == 256 + 1024 + 512 and int(ctr[1]) == SPP * px * 3 and int(ctr[2]) == px * 3 and int(ctr[3]) == 0
    assert A.same_bits(full, c["frames"][:3])
    assert np.array_equal(ctr_full, c["ctr3"]) and int(ctr_full[1]) == SPP * W * H * 3


def test_render_tiles_leaves_the_workspace_alone(gpu):
    """render, render against render, tile launch, render on fresh workspaces: the third frame and its frame_info are
    the second's -- the learned state survived the tile launch in between, which itself reports 0."""
    import torch
    from rtpotato import _ffi as F
    sc, p = _params()
    n = N_TILES * TILE_PX
    with gpu.DeviceScene(sc) as ds:
        res = []
        for between in (False, True):
            ws = ds.workspace()
            ds.reserve(p, ws)  # the per-unit order's buffers: the second render runs its units in their learned order
            out = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
            ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device="cuda")
            ds.render_device(p, out, ctr, workspace=ws)
            if between:
                _render_tiles(ds, replace(p, seed=p.seed + 99), [4, 1], 2, "auto", ws=ws)
                assert ds.frame_info(ws) == 0
            ds.render_device(p, out, ctr, workspace=ws)
            torch.cuda.synchronize()
            res.append((out.cpu().numpy(), ctr.cpu().numpy(), ds.frame_info(ws)))
            ws.close()
    assert res[0][2] == res[1][2] and res[0][2] & F.RP_FRAME_LEARNED_ORDER
    assert A.same_bits(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


def test_render_tiles_refusals(gpu):
    import torch
    from rtpotato import _ffi as F
    sc, p = _params()
    with gpu.DeviceScene(sc) as ds:
        out = torch.full((3 * 65 * 7 * TILE_PX,), A.PAD, dtype=torch.float64, device="cuda")  # room for every refused shape
        ctr = torch.full((F.RP_COUNTERS_LEN,), -1, dtype=torch.int64, device="cuda")
        tiles = torch.tensor([1, 2, 3, 4, 5, 0, 0], dtype=torch.int32, device="cuda")
        for q, n_listed, n_frames, order, msg in (
                (replace(p, samples_per_stream=2), 2, 1, "auto", "one stream per pixel"),
                (replace(p, spp=0), 2, 1, "auto", "spp >= 1"),
                (p, 7, 1, "auto", "above the frame's tile count"),
                (p, 2, 0, "auto", "n_frames"), (p, 2, 65, "auto", "n_frames"), (p, 2, 1, 4, "frame_order"),
                (replace(p, num_shards=2), 2, 1, "auto", "whole frame"),
                (replace(p, shard_map=1), 2, 1, "auto", "whole frame")):
            with pytest.raises(F.RPError, match=msg):
                ds.render_tiles_device(q, tiles, n_listed, n_frames, out, ctr, order=order)
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        cam, pc = sc.camera.to_c(), p.to_c()
        args = [ds.handle, None, ctypes.byref(cam), ctypes.byref(pc), tiles.data_ptr(), 2, 1, 0, out.data_ptr(), None,
                ctr.data_ptr(), s]
        for i in (2, 3, 4, 8, 10):
            bad = list(args)
            bad[i] = None
            assert F.rp().rp_render_tiles_device_ws(*bad) == F.RP_EINVAL, i
        torch.cuda.synchronize()
        assert bool((out == A.PAD).all()) and bool((ctr == -1).all())  # nothing was launched or cleared
        ds.render_tiles_device(p, None, 0, 1, out, ctr)  # an empty list: the counters zeroed, nothing else
        torch.cuda.synchronize()
        assert bool((out == A.PAD).all()) and bool((ctr == 0).all())


# ---- select and the tile fold against the host models

def _device_select(p, mean, var, tiles_in=None, n_in=None, shift=0, **kw):
    import torch
    from rtpotato.render import accum_tiles_select_device
    if n_in is None:
        n_in = len(tiles_in) if tiles_in is not None else mean.size // (3 * (p.tile_w * p.tile_h))
    d_mean, d_var = (torch.from_numpy(a).cuda() for a in (mean, var))
    d_in = None if tiles_in is None else torch.from_numpy(np.ascontiguousarray(tiles_in, np.uint32).view(np.int32)).cuda()
    d_out, d_over = (torch.full((shift + n_in + GUARD,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    count = torch.full((1 + GUARD,), -7, dtype=torch.int32, device="cuda")
    accum_tiles_select_device(p, d_mean, d_var, d_out[shift:], count, tiles_in=d_in, n_in=n_in, over=d_over[shift:], **kw)
    torch.cuda.synchronize()
    c = count.cpu().numpy()
    assert (c[1:] == -7).all()
    for t in (d_out, d_over):
        a = t.cpu().numpy()
        assert (a[:shift] == -7).all() and (a[shift + n_in:] == -7).all(), "wrote outside its entries"
    return (d_out.cpu().numpy()[shift:shift + int(c[0])].view(np.uint32),
            d_over.cpu().numpy()[shift:shift + n_in].view(np.uint32))


def test_select_kernels_equal_host_model(gpu):
    """tests/test_accum_tiles.py's cases on the device: identity, shuffled and partial lists with out-of-range entries,
    NaN and 1e300 outside the frame, several tolerances and tile shares, output lists at odd offsets."""
    from rtpotato.render import accum_tiles_select_host
    from rtpotato.scene import RenderParams
    p = RenderParams(W, H, SPP, 8, 1, TW, TH, samples_per_stream=SPP)
    mean, var = T.synthetic_state(W, H, TW, TH, SEED)
    r = np.random.default_rng(SEED)
    lists = [None, r.permutation(6), np.array([5, 0, 3]), np.array([4, 6, 1, 0xFFFFFFFF, 2]), np.array([], np.uint32)]
    for tile_share in (0.0, 0.01, 0.3):
        for tol in (0.05, 0.02):
            for i, tiles in enumerate(lists):
                ref = accum_tiles_select_host(p, mean, var, tiles_in=tiles, tol=tol, tile_share=tile_share)
                got = _device_select(p, mean, var, tiles, tol=tol, tile_share=tile_share, shift=i % 2)
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (tile_share, tol, tiles)
    # the strict threshold: exactly tile_share * px over is not active, one more is
    _, _, _, inside = T.grid(W, H, TW, TH)
    m1, v1 = np.ones((6 * TILE_PX, 3)), np.zeros((6 * TILE_PX, 3))
    slots = 2 * TILE_PX + np.flatnonzero(inside[2])
    v1[slots[:64]] = 1.0
    assert 2 not in _device_select(p, m1, v1, tile_share=0.125)[0]
    v1[slots[64]] = np.inf
    got = _device_select(p, m1, v1, tile_share=0.125)
    assert list(got[0]) == [2] and got[1][2] == 65


def test_select_16384_tiles_and_refusals(gpu):
    """128 x 128 in 1 x 1 tiles: every lane of the scan's block holds its 16 entries; a shuffled list checks the order.
    One entry more is refused, as are the other bad arguments, with nothing written."""
    import torch
    from rtpotato import _ffi as F
    from rtpotato.render import accum_tiles_select_device, accum_tiles_select_host
    from rtpotato.scene import RenderParams
    p = RenderParams(128, 128, SPP, 8, 1, 1, 1, samples_per_stream=SPP)
    mean, var = T.synthetic_state(128, 128, 1, 1, SEED + 1)
    r = np.random.default_rng(SEED + 1)
    for tiles in (None, r.permutation(16384), r.permutation(16384)[:9999]):
        ref = accum_tiles_select_host(p, mean, var, tiles_in=tiles)
        got = _device_select(p, mean, var, tiles)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and 0 < len(ref[0]) < 16384
    big = RenderParams(129, 127, SPP, 8, 1, 1, 1, samples_per_stream=SPP)
    d = torch.zeros(3 * 129 * 127, dtype=torch.float64, device="cuda")
    out = torch.full((16390,), -7, dtype=torch.int32, device="cuda")
    count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    for kw, msg in ((dict(n_in=16385), "16384"), (dict(tile_share=1.0), "tile_share"), (dict(tol=-1.0), "error params"),
                    (dict(tiles_in=out[2:]), "alias"), (dict(over=out), "alias")):
        with pytest.raises(F.RPError, match=msg):
            accum_tiles_select_device(big, d, d, out, count, **{"n_in": 100, **kw})
    with pytest.raises(F.RPError, match="whole frame"):
        accum_tiles_select_device(replace(big, num_shards=2, shard=1), d, d, out, count, n_in=10)
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and int(count[0]) == -7


def _device_tile_fold(frames, n_frames, tiles, tile_words, stride, n_state, state, n_prior, want_var, shift=0, out_shift=0):
    import torch
    from rtpotato.render import accum_frames_tiles_device
    n = n_state * tile_words
    base = torch.full((shift + frames.size,), A.PAD, dtype=torch.float64, device="cuda")
    base[shift:] = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    outs = []
    for init in state:
        t = torch.full((out_shift + n + GUARD,), A.PAD, dtype=torch.float64, device="cuda")
        t[out_shift:out_shift + n] = torch.from_numpy(np.ascontiguousarray(init)).cuda()
        outs.append(t)
    d_tiles = torch.from_numpy(np.ascontiguousarray(tiles, np.uint32).view(np.int32)).cuda() if len(tiles) else None
    accum_frames_tiles_device(base[shift:], n_frames, d_tiles, len(tiles), tile_words, outs[0][out_shift:out_shift + n],
                              outs[1][out_shift:out_shift + n], n_prior=n_prior,
                              var=outs[2][out_shift:out_shift + n] if want_var else None, stride=stride, n_state_tiles=n_state)
    torch.cuda.synchronize()
    res = []
    for t in outs:
        a = t.cpu().numpy()
        assert (a[:out_shift] == A.PAD).all() and (a[out_shift + n:] == A.PAD).all(), "wrote outside the state"
        res.append(a[out_shift:out_shift + n])
    return res


@pytest.mark.parametrize("tile_words", [3, 6, 3 * 32 * 32])
def test_tile_fold_kernel_equals_host_model(gpu, tile_words):
    """tests/test_accum_tiles.py's cases on the device: tile_words 3 (odd: the 8-byte path), 6 and 3 x 32 x 32 (the wide
    path at an even stride, the 8-byte one at an odd stride or misaligned buffers); lists of 0, 1 and all blocks, an
    out-of-range entry skipped with the guard words behind every buffer intact; with and without prior frames.  The
    whole state is compared: the unlisted blocks keep their words."""
    from rtpotato.render import accum_frames_tiles_host
    n_state = 6
    n = n_state * tile_words
    r = np.random.default_rng(SEED + tile_words)
    prior = A.synthetic(2, n, n, SEED + 3)
    state = A.accum_frames(prior, 2, n, n)
    fresh = tuple(np.full(n, v) for v in (7.0, 8.0, 9.0))
    for tiles in ([], [4], list(r.permutation(n_state)), [2, 6, 1]):
        tiles = np.array(tiles, dtype=np.uint32)
        for pad, shift, out_shift in ((0, 0, 0), (5, 0, 0), (0, 1, 0), (0, 0, 1), (2, 1, 1)):
            for n_frames, n_prior, st in ((1, 0, fresh), (5, 0, fresh), (3, 2, state)):
                stride = len(tiles) * tile_words + pad
                frames = T.synthetic_blocks(n_frames, len(tiles), tile_words, stride, SEED + 7 * n_frames + len(tiles))
                want_var = n_prior + n_frames >= 2
                ref = [np.array(s) for s in st]
                accum_frames_tiles_host(frames, n_frames, tiles, len(tiles), tile_words, ref[0], ref[1], n_prior=n_prior,
                                        var=ref[2] if want_var else None, stride=stride, n_state_tiles=n_state)
                got = _device_tile_fold(frames, n_frames, tiles, tile_words, stride, n_state, st, n_prior, want_var, shift,
                                        out_shift)
                assert all(A.same_bits(g, x) for g, x in zip(got, ref)), (tiles, pad, shift, out_shift, n_frames)


def test_tile_fold_refusals(gpu):
    import torch
    from rtpotato import _ffi as F
    L = F.rp()
    fr = torch.ones(64, dtype=torch.float64, device="cuda")
    out = torch.full((3, 16), A.PAD, dtype=torch.float64, device="cuda")
    tiles = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t, off=0: None if t is None else t.data_ptr() + 8 * off

    def call(tile_words=4, n_state=4, tl=tiles.data_ptr(), n_listed=2, n_prior=0, n_frames=3, frames=ptr(fr), stride=8,
             mean=ptr(out[0]), m2=ptr(out[1]), var=ptr(out[2])):
        return L.rp_accum_frames_tiles_device(tile_words, n_state, tl, n_listed, n_prior, n_frames, frames, stride, mean, m2,
                                              var, s)

    for kw, msg in ((dict(frames=None), "non-NULL"), (dict(mean=None), "non-NULL"), (dict(m2=None), "non-NULL"),
                    (dict(tile_words=0), "tile_words is zero"), (dict(n_frames=0), "n_frames is zero"),
                    (dict(n_listed=5), "above n_state_tiles"), (dict(tl=None), "tiles must be non-NULL"),
                    (dict(stride=7), "frame_stride is below"), (dict(n_prior=0x7fffffff), "2^31 - 1"),
                    (dict(n_frames=1), "at least two frames"), (dict(tile_words=1 << 40), "2^40 - 512"),
                    (dict(n_state=1 << 31, tile_words=1 << 10, n_listed=1), "2^40 - 512"),
                    (dict(mean=ptr(fr, 8)), "alias the frames"), (dict(m2=ptr(out[0], 4)), "alias one another"),
                    (dict(var=ptr(out[1])), "alias one another")):
        assert call(**kw) == F.RP_EINVAL, kw
        assert msg in L.rp_last_error().decode(), (kw, L.rp_last_error())
    assert call(n_listed=0, tl=None, stride=0) == F.RP_OK
    torch.cuda.synchronize()
    assert bool((out == A.PAD).all())  # nothing was launched
    assert call() == F.RP_OK
    torch.cuda.synchronize()
    assert int((out != A.PAD).sum()) == 3 * 8


# ---- the loop

ADAPT = dict(frames_per_launch=4, max_frames=MAX_FRAMES, max_launch_frames=4, tol=0.05, share=0.0, tile_share=0.05)


def test_render_adaptive_is_its_host_replay(gpu):
    """The end-to-end invariant: render_adaptive's tile_frames and log are those of the loop replayed on the host with
    the numpy models from 12 frames rendered once, its mean and variance are the replay's bit for bit -- every pixel
    the plain progressive mean of its own tile's first n_t frames -- and samples = spp x sum of n_t x px_t.

    tol and tile_share were chosen on the CPU from the oracle's frames of this scene.  Pixels over 5 % per tile (of
    1024, 1024, 512, 512, 512, 256 in-frame pixels) after 4 frames: 302, 565, 99, 0, 43, 0; after 8: 432, 735, 159, 0,
    44, 0; after 12: 529, 789, 212, 0, 44, 0 (they grow: a pixel whose first frames all missed the light has variance 0
    until a frame hits it -- DESIGN.md 4.14 on the bias).  The counts barely move with tol (0.3: 293, 509, 94, 0, 26, 0
    after 4), so the gap that matters is tile_share's: at 0.05 tile 4's threshold is 25.6 pixels against its 43, tiles
    3 and 5 have none over and stop after the first launch, tiles 0, 1, 2 and 4 are refined to 12 frames.  The test
    asserts that it is not vacuous."""
    c = _frames(gpu)
    sc, p = _params()
    ref = T.replay_adaptive(c["frames"].reshape(MAX_FRAMES, -1), W, H, TW, TH, ADAPT["frames_per_launch"], MAX_FRAMES,
                            ADAPT["max_launch_frames"], ADAPT["tol"], ADAPT["share"], ADAPT["tile_share"])
    with gpu.DeviceScene(sc) as ds:
        out = ds.render_adaptive(p, denoise=False, **ADAPT)
    nt = out["tile_frames"]
    print("tile_frames", nt.tolist(), "log", out["log"])
    assert nt.dtype == np.int32 and np.array_equal(nt, ref["tile_frames"])
    assert out["log"] == ref["log"] and out["frames"] == int(nt.max()) and "denoised" not in out
    assert A.same_bits(out["mean"].cpu().numpy(), ref["mean"])
    assert A.same_bits(out["variance"].cpu().numpy(), ref["variance"])
    _, _, _, inside = T.grid(W, H, TW, TH)
    assert out["samples"] == SPP * int((nt.reshape(-1) * inside.sum(1)).sum())
    # not vacuous: a tile stopped after the first launch, another was refined beyond it
    assert (nt == ADAPT["frames_per_launch"]).any() and (nt > ADAPT["frames_per_launch"]).any()
    assert len(out["log"]) >= 2 and out["log"][1][1] < N_TILES


def test_render_adaptive_denoised_and_refusals(gpu):
    import torch
    sc, p = _params()
    with gpu.DeviceScene(sc) as ds:
        out = ds.render_adaptive(p, frames_per_launch=2, max_frames=6, tol=0.05, share=0.01)
        for k in ("mean", "variance", "denoised"):
            assert out[k].shape == (H, W, 3) and bool(torch.isfinite(out[k]).all()), k
        assert not torch.equal(out["denoised"], out["mean"]) and out["tile_frames"].shape == (2, 3)
        assert 2 <= out["frames"] <= 6 and out["samples"] > 0 and out["rays"] >= out["samples"]
        stop = ds.render_adaptive(p, tol=1e6, denoise=False)  # nothing over: the first launch is the last
        assert stop["frames"] == 4 and len(stop["log"]) == 1 and (stop["tile_frames"] == 4).all()
        for bad in ({"frames_per_launch": 0}, {"frames_per_launch": 1}, {"max_frames": 1}, {"tol": 0.0},
                    {"max_launch_frames": 0}, {"max_launch_frames": 65}, {"tile_share": 1.0}, {"share": 1.5}):
            with pytest.raises(ValueError):
                ds.render_adaptive(p, **bad)
        with pytest.raises(ValueError, match="num_shards"):
            ds.render_adaptive(replace(p, num_shards=2))
        with pytest.raises(ValueError, match="one stream per pixel"):
            ds.render_adaptive(replace(p, samples_per_stream=2))
