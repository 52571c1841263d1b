"""GPU: temporal reprojection (rp_reproject_device, rp_reproject, rp_accum_frames_counts_device; csrc/rp_reproject.hip and
csrc/rp_accum.hip) against the host models (rph_reproject, rph_accum_frames_counts: the same arithmetic headers on the
CPU) and the numpy models of tests/reproject_ref.py, bit for bit, on the cases of tests/test_reproject.py and a frame of
several blocks; refusals, graph capture, and DeviceScene.render_sequence on a camera orbit: the chain replayed on the host
and the accumulated frame's error against the oracle at 512 spp."""
import ctypes
from dataclasses import replace

import numpy as np
import pytest

import accum_ref as A
import reproject_ref as R

pytestmark = pytest.mark.gpu

SEED = 20260311
GUARD = 2  # words behind every output that must keep their contents
KEYS = ("depth", "normal", "depth_prev", "normal_prev", "mean_prev", "m2_prev", "count_prev")


def host_reproject(cur, prev, d, **kw):
    from rtpotato.render import reproject_host
    return reproject_host(cur, prev, *(d[k] for k in KEYS), params=kw or None)


def model_reproject(cur, prev, d, **kw):
    H, W = d["depth"].shape
    return R.reproject(cur, prev, W, H, *(d[k] for k in KEYS), **kw)[:4]


def upload(d):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(d[k]).view(np.int32) if d[k].dtype == np.uint32
                                else np.ascontiguousarray(d[k])).cuda() for k in KEYS}


def device_outputs(W, H):
    """mean, m2 (PAD), count (77), stats (-1), each GUARD elements longer than the frame needs."""
    import torch
    from rtpotato import _ffi as F
    return {"mean": torch.full((3 * W * H + GUARD,), A.PAD, dtype=torch.float64, device="cuda"),
            "m2": torch.full((3 * W * H + GUARD,), A.PAD, dtype=torch.float64, device="cuda"),
            "count": torch.full((W * H + GUARD,), 77, dtype=torch.int32, device="cuda"),
            "stats": torch.full((F.RP_REPROJECT_STATS_LEN + GUARD,), -1, dtype=torch.int64, device="cuda")}


def device_reproject(cur, prev, d, stream=None, **kw):
    """rp_reproject_device on uploaded copies: (mean, m2, count, stats) on the host, the guard words checked."""
    import torch
    from rtpotato import _ffi as F
    from rtpotato.render import reproject_device
    H, W = d["depth"].shape
    t, o = upload(d), device_outputs(W, H)
    reproject_device(cur, prev, *(t[k] for k in KEYS), o["mean"][:3 * W * H].view(H, W, 3), o["m2"][:3 * W * H].view(H, W, 3),
                     o["count"][:W * H].view(H, W), o["stats"][:F.RP_REPROJECT_STATS_LEN], params=kw or None, stream=stream)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in o.items()}
    assert (h["mean"][3 * W * H:] == A.PAD).all() and (h["m2"][3 * W * H:] == A.PAD).all()
    assert (h["count"][W * H:] == 77).all() and (h["stats"][F.RP_REPROJECT_STATS_LEN:] == -1).all()
    return (h["mean"][:3 * W * H].reshape(H, W, 3), h["m2"][:3 * W * H].reshape(H, W, 3),
            h["count"][:W * H].reshape(H, W).view(np.uint32), h["stats"][:F.RP_REPROJECT_STATS_LEN].astype(np.uint64))


def assert_same(got, ref, what=""):
    assert R.same_bits(got[0], ref[0]), f"{what}: mean"
    assert R.same_bits(got[1], ref[1]), f"{what}: m2"
    assert np.array_equal(got[2], ref[2]), f"{what}: count"
    assert got[3].tolist() == ref[3].tolist(), f"{what}: stats {got[3].tolist()} {ref[3].tolist()}"


@pytest.mark.parametrize("size", R.SIZES + [(130, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_host_equals_numpy(gpu, size):
    """Every camera pair of the CPU suite at its sizes and at 130 x 70 -- three blocks across with 2 lanes in the last,
    eighteen down with 2 rows in the last: kernel, host library and numpy model, bit for bit, statistics included."""
    W, H = size
    d = R.synthetic(W, H, SEED + 13 * W + H)
    for pair, (cur, prev) in R.camera_pairs(W, H).items():
        ref = model_reproject(cur, prev, d)
        assert_same(host_reproject(cur, prev, d), ref, pair + " host")
        got = device_reproject(cur, prev, d)
        assert_same(got, ref, pair + " device")
        if pair == "away":
            assert got[3][3] == W * H and not got[2].any()
    cur, prev = R.camera_pairs(W, H)["translated"]
    kw = {"sigma_depth": 0.01, "normal_cos": 0.99, "max_history": 3}
    assert_same(device_reproject(cur, prev, d, **kw), model_reproject(cur, prev, d, **kw), "explicit params")


def test_planted_cases_and_the_synchronous_call(gpu):
    """The integer-fx frame (zero-weight taps skipped, NaN behind them), the NaN states under taps that do not count and
    the NaN under one that does; rp_reproject, the synchronous call on host buffers, gives the same bits."""
    from rtpotato.render import reproject
    cur, prev, d = R.integer_fx_case(SEED + 2)
    ref = model_reproject(cur, prev, d)
    got = device_reproject(cur, prev, d)
    assert_same(got, ref, "integer fx")
    assert np.array_equal(got[2], d["count_prev"]) and R.same_bits(got[0], d["mean_prev"])
    cur, prev, d, d2, info, t = R.nan_case(SEED + 3)
    got = device_reproject(cur, prev, d)
    assert_same(got, model_reproject(cur, prev, d), "NaN where nothing counts")
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    got = device_reproject(cur, prev, d2)
    assert_same(got, model_reproject(cur, prev, d2), "NaN where it counts")
    hit = ((info["tap_index"] == t) & info["counting"]).any(axis=2)
    assert hit.sum() >= 2 and np.array_equal(np.isnan(got[0][..., 1]), hit)
    sync = reproject(cur, prev, *(d2[k] for k in KEYS))
    assert_same(sync[:4], got, "rp_reproject")
    assert sync[4] >= 0.0


def test_on_a_stream(gpu):
    """On a non-default torch stream: the default stream's bits."""
    import torch
    W, H = 130, 70
    cur, prev = R.camera_pairs(W, H)["rotated"]
    d = R.synthetic(W, H, SEED + 5)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        got = device_reproject(cur, prev, d, stream=st)
    assert_same(got, device_reproject(cur, prev, d), "stream")


def device_counts_fold(frames, n_frames, n_pixels, wpp, stride, count, mean, m2, var_one, shift=0, want_var=True):
    """rp_accum_frames_counts_device on copies that start `shift` doubles (count: `shift` words) into their allocations
    and end GUARD short of them: (count, mean, m2, var) on the host."""
    import torch
    from rtpotato.render import accum_frames_counts_device
    n_words = n_pixels * wpp

    def dev(a, fill, dtype):
        t = torch.full((shift + a.size + GUARD,), fill, dtype=dtype, device="cuda")
        t[shift:shift + a.size] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return t

    fr = dev(frames, A.PAD, torch.float64)
    c = dev(count.view(np.int32), 77, torch.int32)
    outs = [dev(mean, A.PAD, torch.float64), dev(m2, A.PAD, torch.float64),
            dev(np.full(n_words, A.PAD), A.PAD, torch.float64) if want_var else None]
    view = [t[shift:] if t is not None else None for t in outs]
    accum_frames_counts_device(fr[shift:], n_frames, c[shift:], view[0], view[1], var=view[2], var_one=var_one,
                               words_per_pixel=wpp, n_pixels=n_pixels, stride=stride)
    torch.cuda.synchronize()
    ch = c.cpu().numpy()
    assert (ch[:shift] == 77).all() and (ch[shift + n_pixels:] == 77).all()
    res = [ch[shift:shift + n_pixels].view(np.uint32)]
    for t in outs:
        if t is None:
            res.append(None)
            continue
        a = t.cpu().numpy()
        assert (a[:shift] == A.PAD).all() and (a[shift + n_words:] == A.PAD).all(), "wrote outside its words"
        res.append(a[shift:shift + n_words])
    return res


@pytest.mark.parametrize("wpp,n_pixels", [(1, 1), (1, 257), (3, 77), (3, 1025), (2, 9)])
def test_counts_fold_equals_host_equals_numpy(gpu, wpp, n_pixels):
    """rp_accum_frames_counts_device against rph_accum_frames_counts and the numpy model: odd pixel counts (one and
    several blocks), one, two and three words per pixel, 1, 2 and 5 frames, a padded stride, buffers that start one
    double into their allocation, NaN states under the pixels with count 0, var_one where a pixel ends with one frame."""
    from rtpotato.render import accum_frames_counts_host
    n_words = n_pixels * wpp
    for n_frames in (1, 2, 5):
        for pad, shift in ((0, 0), (3, 1)):
            stride = n_words + pad
            r = np.random.default_rng(SEED + 100 * n_frames + n_pixels)
            frames = A.synthetic(n_frames, n_words, stride, SEED + n_pixels)
            count = r.choice(R.COUNTS, size=n_pixels).astype(np.uint32)
            mean, m2 = r.uniform(0.0, 3.0, size=n_words), r.uniform(0.0, 3.0, size=n_words)
            fresh = np.repeat(count == 0, wpp)
            mean[fresh] = m2[fresh] = np.nan
            ref = R.accum_frames_counts(frames, n_frames, n_pixels, wpp, stride, count, mean, m2, var_one=0.25)
            hc, hm, hq, hv = count.copy(), mean.copy(), m2.copy(), np.full(n_words, A.PAD)
            accum_frames_counts_host(frames, n_frames, hc, hm, hq, var=hv, var_one=0.25, words_per_pixel=wpp, stride=stride)
            got = device_counts_fold(frames, n_frames, n_pixels, wpp, stride, count, mean, m2, 0.25, shift=shift)
            assert np.array_equal(got[0], hc) and np.array_equal(got[0], ref[0]), (n_frames, pad, shift)
            for g, h, m in zip(got[1:], (hm, hq, hv), ref[1:]):
                assert R.same_bits(g, h) and R.same_bits(g, m), (n_frames, pad, shift)
            no_var = device_counts_fold(frames, n_frames, n_pixels, wpp, stride, count, mean, m2, 0.25, shift=shift,
                                        want_var=False)
            assert R.same_bits(no_var[1], got[1]) and R.same_bits(no_var[2], got[2]) and no_var[3] is None


@pytest.mark.parametrize("c", [0, 1, 6])
def test_uniform_count_equals_the_plain_fold_on_the_device(gpu, c):
    """The defined property on the device: every count equal to c gives rp_accum_frames_device's mean, m2 and variance
    with n_prior = c, bit for bit."""
    import torch
    from rtpotato.render import accum_frames_device
    n_pixels, wpp, n_frames = 1025, 3, 3
    n_words = n_pixels * wpp
    frames = A.synthetic(n_frames, n_words, n_words + 1, SEED + 8)
    r = np.random.default_rng(SEED + 9)
    mean, m2 = r.uniform(0.0, 3.0, size=n_words), r.uniform(0.0, 3.0, size=n_words)
    got = device_counts_fold(frames, n_frames, n_pixels, wpp, n_words + 1, np.full(n_pixels, c, dtype=np.uint32), mean,
                             m2, 1.0)
    fr, dm, dq = (torch.from_numpy(a.copy()).cuda() for a in (frames, mean, m2))
    dv = torch.empty_like(dm)
    accum_frames_device(fr, n_frames, dm, dq, n_prior=c, var=dv, stride=n_words + 1)
    torch.cuda.synchronize()
    assert (got[0] == c + n_frames).all()
    for g, t in zip(got[1:], (dm, dq, dv)):
        assert R.same_bits(g, t.cpu().numpy())


def test_refusals(gpu):
    """Each RP_EINVAL case of the two device calls with its message, nothing launched: the outputs keep their fill."""
    import torch
    from rtpotato import _ffi as F
    L = F.rp()
    W, H = 5, 4
    n = W * H
    cur, prev = R.camera_pairs(W, H)["translated"]
    t = upload(R.synthetic(W, H, SEED + 10))
    o = device_outputs(W, H)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    order = list(KEYS) + ["mean", "m2", "count", "stats"]
    ptr = {**{k: v.data_ptr() for k, v in t.items()}, **{k: v.data_ptr() for k, v in o.items()}}

    def call(params=None, width=W, height=H, cur_=cur, prev_=prev, **swap):
        cc = ctypes.byref(cur_.to_c()) if cur_ is not None else None
        cp = ctypes.byref(prev_.to_c()) if prev_ is not None else None
        return L.rp_reproject_device(ctypes.byref(params) if params is not None else None, width, height, cc, cp,
                                     *[swap.get(k, ptr[k]) for k in order], s)

    cases = [({k: None}, b"non-NULL") for k in order]
    cases += [({"cur_": None}, b"non-NULL"), ({"prev_": None}, b"non-NULL"), ({"width": 0}, b"1..65535"),
              ({"height": 0}, b"1..65535"), ({"width": 65536}, b"1..65535"), ({"height": 65536}, b"1..65535")]
    for kw in ({"sigma_depth": -0.05}, {"sigma_depth": float("nan")}, {"sigma_depth": float("inf")},
               {"normal_cos": -0.5}, {"normal_cos": 1.5}, {"max_history": 2 ** 31}):
        cases.append(({"params": F.rp_reproject_params(**kw)}, b"out of range"))
    for field, value in (("fov", float("nan")), ("fov", 0.0), ("fov", -0.9), ("aspect", float("inf"))):
        for which in ("cur_", "prev_"):
            cam = R.Cam(cur.R, cur.pos, cur.fov, cur.aspect)
            setattr(cam, field, value)
            cases.append(({which: cam}, b"camera"))
    bad = R.Cam(cur.R, cur.pos, cur.fov, cur.aspect)
    bad.R[7] = np.inf
    cases.append(({"prev_": bad}, b"camera"))
    for out in ("mean", "m2"):
        for inp in ("normal", "normal_prev", "mean_prev", "m2_prev"):
            cases.append(({out: ptr[inp]}, b"alias an input"))  # in place: refused
    cases += [({"count": ptr["count_prev"]}, b"alias an input"), ({"mean": ptr["depth"] + 8 * 3}, b"alias an input"),
              ({"stats": ptr["depth_prev"] + 8 * (n - 1)}, b"alias an input"), ({"m2": ptr["mean"]}, b"one another"),
              ({"m2": ptr["mean"] + 8 * (3 * n - 1)}, b"one another"), ({"stats": ptr["m2"] + 40}, b"one another"),
              ({"count": ptr["mean"] + 400}, b"one another")]
    for kw, msg in cases:
        assert call(**kw) == F.RP_EINVAL, kw
        assert msg in L.rp_last_error(), (kw, L.rp_last_error())
    # the fold
    fr = torch.ones(40, dtype=torch.float64, device="cuda")
    st = torch.full((3, 8), A.PAD, dtype=torch.float64, device="cuda")
    cnt = torch.full((4,), 3, dtype=torch.int32, device="cuda")
    p8 = lambda x, off=0: x.data_ptr() + 8 * off

    def fold(n_pixels=2, wpp=3, n_frames=3, frames=p8(fr), stride=6, count=cnt.data_ptr(), mean=p8(st[0]), m2=p8(st[1]),
             var=p8(st[2]), var_one=1.0):
        return L.rp_accum_frames_counts_device(n_pixels, wpp, n_frames, frames, stride, count, mean, m2, var, var_one, s)

    for kw, msg in (({"frames": None}, b"non-NULL"), ({"mean": None}, b"non-NULL"), ({"m2": None}, b"non-NULL"),
                    ({"count": None}, b"non-NULL"), ({"n_frames": 0}, b"n_frames is zero"), ({"n_pixels": 0}, b"is zero"),
                    ({"wpp": 0}, b"is zero"), ({"stride": 5}, b"frame_stride"), ({"n_frames": 2 ** 31}, b"2^31 - 1"),
                    ({"n_pixels": 2 ** 39, "stride": 2 ** 41}, b"2^40 - 512"), ({"var_one": -1.0}, b"var_one"),
                    ({"var_one": float("inf")}, b"var_one"), ({"var_one": float("nan")}, b"var_one"),
                    ({"mean": p8(fr, 8)}, b"alias the frames"), ({"var": p8(fr, 1)}, b"alias the frames"),
                    ({"m2": p8(st[0])}, b"one another"), ({"var": p8(st[1], 3)}, b"one another"),
                    ({"count": p8(fr, 3)}, b"count must not alias"), ({"count": p8(st[0], 5)}, b"count must not alias"),
                    ({"count": p8(st[2])}, b"count must not alias")):
        assert fold(**kw) == F.RP_EINVAL, kw
        assert msg in L.rp_last_error(), (kw, L.rp_last_error())
    torch.cuda.synchronize()
    assert bool((o["mean"] == A.PAD).all()) and bool((o["m2"] == A.PAD).all()) and bool((o["count"] == 77).all())
    assert bool((o["stats"] == -1).all()) and bool((st == A.PAD).all()) and bool((cnt == 3).all())
    assert call() == F.RP_OK and fold(n_frames=1, var_one=0.0) == F.RP_OK
    torch.cuda.synchronize()
    assert int(o["stats"][0]) == n and bool((cnt[:2] == 4).all()) and bool((cnt[2:] == 3).all())


def test_graph_capture(gpu):
    """Reprojection and fold captured into a torch.cuda.graph as one chain (neither allocates or synchronises): one
    replay writes the bytes of the eager calls."""
    import torch
    from rtpotato import _ffi as F
    from rtpotato.render import accum_frames_counts_device, reproject_device
    W, H = 130, 70
    cur, prev = R.camera_pairs(W, H)["translated"]
    t = upload(R.synthetic(W, H, SEED + 12))
    frames = torch.from_numpy(np.random.default_rng(SEED + 13).uniform(0.0, 3.0, size=2 * 3 * W * H)).cuda()
    mean, m2, var = (torch.full((H, W, 3), A.PAD, dtype=torch.float64, device="cuda") for _ in range(3))
    count = torch.full((H, W), 77, dtype=torch.int32, device="cuda")
    stats = torch.full((F.RP_REPROJECT_STATS_LEN,), -1, dtype=torch.int64, device="cuda")
    outs = (mean, m2, var, count, stats)

    def chain():
        reproject_device(cur, prev, *(t[k] for k in KEYS), mean, m2, count, stats)
        accum_frames_counts_device(frames, 2, count, mean, m2, var=var, var_one=0.5)

    chain()
    torch.cuda.synchronize()
    eager = [x.clone() for x in outs]
    assert int(eager[4][0]) == W * H and 0 < int(eager[4][1]) < W * H
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    for x in (mean, m2, var):
        x.fill_(A.PAD)
    count.fill_(77)
    stats.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    for x, e in zip(outs, eager):
        assert torch.equal(x.view(torch.uint8), e.view(torch.uint8))
    del graph


def test_render_sequence_on_an_orbit(gpu):
    """bunny_lambert at 96 x 64, 4 spp, six poses one degree apart, two frames per pose.  (a) The last pose of
    render_sequence equals the same chain replayed on the host -- the frames and guides rendered per pose by the same
    calls, then reproject_host (with reproject_prev_camera) and accum_frames_counts_host -- bit for bit: mean,
    variance and count.  (b) Against the oracle's 512-spp frame from the last camera, the accumulated mean has a
    smaller squared error than the last pose's own two-frame mean (ratio < 1, over every pixel: a pixel that started
    over carries the same error on both sides); the pixels that started over (count <= frames_per_pose) are under
    MASK_SHARE of the frame.  (c) More than half of the pixels kept their history at the last pose.
    Measured on an MI355X: see profiles/r26/MANIFEST.md (squared-error ratio of the mean and of the denoised frames)."""
    import torch
    from parity import oracle_render
    from rtpotato import _ffi as F
    from rtpotato.render import (accum_frames_counts_host, denoise_device, reproject_host, reproject_prev_camera,
                                 reproject_stats, unpack_shard)
    from rtpotato.scene import shard_slot_count
    sc, p, cams = R.orbit_scene()
    fpp = R.ORBIT["frames_per_pose"]
    W, H, n = p.width, p.height, shard_slot_count(p)
    with gpu.DeviceScene(sc) as ds:
        seq = list(ds.render_sequence(p, cams, frames_per_pose=fpp))
        torch.cuda.synchronize()
        last = {k: (v.cpu().numpy() if v is not None else None) for k, v in seq[-1].items()}
        stats = [reproject_stats(s["stats"].cpu().numpy()) for s in seq]
        # the same chain on the host, from the same rendered frames and guides
        state = None
        for t, cam in enumerate(cams):
            frames = torch.zeros(fpp * 3 * n, dtype=torch.float64, device="cuda")
            ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device="cuda")
            ds.render_frames_device(replace(p, seed=p.seed + t * fpp * W * H), fpp, frames, ctr, camera=cam)
            torch.cuda.synchronize()
            assert int(ctr[3]) == 0
            fh = frames.cpu().numpy()
            fr = np.stack([unpack_shard(p, fh[f * 3 * n:(f + 1) * 3 * n], 3) for f in range(fpp)])
            aov = ds.render_aov(p, camera=cam, albedo=(t == len(cams) - 1), foreground=False)
            if state is None:
                mean, m2, count = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W), dtype=np.uint32)
            else:
                mean, m2, count, hstats = reproject_host(cam, reproject_prev_camera(state["cam"]), aov["depth"],
                                                         aov["normal"], state["depth"], state["normal"], state["mean"],
                                                         state["m2"], state["count"])
                assert reproject_stats(hstats) == stats[t], t
            var = np.empty((H, W, 3))
            accum_frames_counts_host(fr.reshape(-1), fpp, count.reshape(-1), mean.reshape(-1), m2.reshape(-1),
                                     var=var.reshape(-1), var_one=1.0)
            state = {"cam": cam, "depth": aov["depth"], "normal": aov["normal"], "mean": mean, "m2": m2, "count": count}
        assert R.same_bits(last["mean"], mean) and R.same_bits(last["variance"], var)
        assert np.array_equal(last["count"].view(np.uint32), count)
        # the last pose's own frames without history, and their denoised frame
        own_c = np.zeros(W * H, dtype=np.uint32)
        own_m, own_q, own_v = np.zeros(3 * W * H), np.zeros(3 * W * H), np.zeros(3 * W * H)
        accum_frames_counts_host(fr.reshape(-1), fpp, own_c, own_m, own_q, var=own_v, var_one=1.0)
        own_den = torch.empty((H, W, 3), dtype=torch.float64, device="cuda")
        g = [torch.from_numpy(aov[k]).cuda() for k in ("normal", "albedo", "depth")]
        denoise_device(torch.from_numpy(own_m.reshape(H, W, 3)).cuda(), *g, own_den,
                       variance=torch.from_numpy(own_v.reshape(H, W, 3)).cuda())
        torch.cuda.synchronize()
        own_den = own_den.cpu().numpy()
    target, _, _ = oracle_render(replace(sc, camera=cams[-1]), replace(p, spp=512, seed=p.seed + 987654321))
    se = lambda a: float(((a.reshape(H, W, 3) - target) ** 2).sum())
    ratio, ratio_den = se(mean) / se(own_m), se(last["denoised"]) / se(own_den)
    started_over = float((count <= fpp).mean())
    keep = ((count > fpp)[..., None] & np.ones(3, dtype=bool)).reshape(-1)
    masked = float(((mean.reshape(-1) - target.reshape(-1))[keep] ** 2).sum() /
                   ((own_m - target.reshape(-1))[keep] ** 2).sum())
    print(f"orbit: squared error of the accumulated mean / of the pose's own {fpp}-frame mean = {ratio:.4f} "
          f"(pixels with history only: {masked:.4f}); denoised / denoised = {ratio_den:.4f}; "
          f"{started_over:.3%} of the pixels started over; kept per pose {[s['kept'] for s in stats]} of {W * H}; "
          f"mean count {count.mean():.2f}")
    assert stats[0] == {"pixels": W * H, "kept": 0, "count_sum": 0, "off": 0}
    assert started_over < R.MASK_SHARE
    assert stats[-1]["kept"] > 0.5 * stats[-1]["pixels"]
    assert ratio < 1.0
