"""Tile-adaptive progressive rendering (DeviceScene.render_adaptive) beside the whole-frame loop it
grew from (DeviceScene.render_progressive, unchanged code: the yardstick), at the same stopping rule.

The C3 scene at 1920 x 1080, 16 spp, one stream per pixel (samples_per_stream = spp), tol 0.05, share 0.01, max_frames
64.  For every `--fpl` (frames per launch; default 4, 8, 16) the two loops alternate for `--reps` repetitions in one
session after a warm-up of each; torch (HIP) events on one stream bracket the whole loop, host synchronisations and
read-backs included -- what a caller waits for.  Per loop the record gives device ms (median, min, max), frames, camera
samples and rays (the adaptive loop's from its counters; the progressive loop's from the same launches made again
outside the timed window, since it does not return them), the final global over-count, and the mean squared error of
`mean` and of `denoised` against the plain mean of `--ref-frames` (256) further frames at seeds no run used
(seed + 64 W H onwards).  For the adaptive loop also the tiles, frames and device ms of every launch, and
rp_accum_tiles_select_device and rp_accum_frames_tiles_device timed on their own (`--calls` back-to-back calls over the
identity list, and over the last refinement launch's list and frames).  No target ratio: the record says what ran.

    python tools/adaptive_time.py --reps 5
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "raytracing-potato_amd")]


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--fpl", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--max-frames", type=int, default=64)
    ap.add_argument("--max-launch-frames", type=int, default=16)
    ap.add_argument("--tol", type=float, default=0.05)
    ap.add_argument("--share", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--ref-frames", type=int, default=256)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r19", "adaptive_time.json"))
    a = ap.parse_args()
    assert a.reps >= 5, "at least 5 repetitions of each"
    from dataclasses import replace

    import numpy as np
    import torch

    from rtpotato import _ffi as F
    from rtpotato import render, scenes
    from rtpotato.scene import shard_slot_count
    scene, params = scenes.config_scene(a.config)
    p = replace(params, spp=a.spp, samples_per_stream=a.spp)
    w, h, n = p.width, p.height, shard_slot_count(p)
    tw, th = p.tile_w or 32, p.tile_h or 32
    n_tiles = n // (tw * th)
    dev = torch.device("cuda", 0)
    rec = {"tool": "tools/adaptive_time.py", "config": a.config, "width": w, "height": h, "spp": a.spp,
           "samples_per_stream": a.spp, "tol": a.tol, "share": a.share, "tile_share": a.share, "max_frames": a.max_frames,
           "max_launch_frames": a.max_launch_frames, "tiles": n_tiles, "build_id": F.rp().rp_build_id().decode(),
           "reps": a.reps, "ref_frames": a.ref_frames,
           "timer": "torch (HIP) events on one stream around the whole loop; the loops alternate", "runs": []}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    with render.DeviceScene(scene) as ds:
        # the reference: the plain mean of ref_frames frames past every run's (frame f at seed + f W H)
        L = 16
        ds.reserve_frames(p, L)
        frames = torch.zeros(L * 3 * n, dtype=torch.float64, device=dev)
        mean, m2 = (torch.zeros(3 * n, dtype=torch.float64, device=dev) for _ in range(2))
        ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device=dev)
        for f in range(0, a.ref_frames, L):
            k = min(L, a.ref_frames - f)
            q = replace(p, seed=(p.seed + (a.max_frames + f) * w * h) & 0xFFFFFFFFFFFFFFFF)
            ds.render_frames_device(q, k, frames, ctr)
            render.accum_frames_device(frames, k, mean, m2, n_prior=f, n_words=3 * n)
            assert int(ctr[3]) == 0
        ref = torch.empty((h, w, 3), dtype=torch.float64, device=dev)
        pc = p.to_c()
        import ctypes
        F.check(F.rp().rp_frame_assemble(ctypes.byref(pc), mean.data_ptr(), 6, ref.data_ptr(),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        del frames, mean, m2

        def mse(x):
            return float(((x - ref) ** 2).mean())

        def rays_of(n_frames, fpl):  # the progressive loop's launches again: its counters
            buf = torch.zeros(fpl * 3 * n, dtype=torch.float64, device=dev)
            rays = samples = 0
            for f in range(0, n_frames, fpl):
                k = min(fpl, n_frames - f)
                ds.render_frames_device(replace(p, seed=(p.seed + f * w * h) & 0xFFFFFFFFFFFFFFFF), k, buf, ctr)
                c = ctr.cpu().numpy()
                rays, samples = rays + int(c[0]), samples + int(c[1])
            return rays, samples

        for fpl in a.fpl:
            kw = dict(frames_per_launch=fpl, max_frames=a.max_frames, tol=a.tol, share=a.share)
            loops = {"progressive": lambda: ds.render_progressive(p, **kw),
                     "adaptive": lambda: ds.render_adaptive(p, max_launch_frames=a.max_launch_frames, **kw)}
            for fn in loops.values():  # warm-up of every shape
                fn()
            times, last = {k: [] for k in loops}, {}
            for _ in range(a.reps):  # alternating
                for k, fn in loops.items():
                    ms, out = timed(fn)
                    times[k].append(ms)
                    if k in last:  # every repetition is the same run
                        assert torch.equal(out["mean"].view(torch.uint8), last[k]["mean"].view(torch.uint8))
                    last[k] = out
            pr, ad = last["progressive"], last["adaptive"]
            rays, samples = rays_of(pr["frames"], fpl)
            run = {"frames_per_launch": fpl,
                   "progressive": {**summary(times["progressive"]), "frames": pr["frames"], "launches": len(pr["stats"]),
                                   "samples": samples, "rays": rays, "pixels": pr["stats"][-1][1],
                                   "over": pr["stats"][-1][2], "mse_mean": mse(pr["mean"]),
                                   "mse_denoised": mse(pr["denoised"])},
                   "adaptive": {**summary(times["adaptive"]), "frames": ad["frames"], "launches": len(ad["log"]),
                                "samples": ad["samples"], "rays": ad["rays"], "pixels": ad["log"][-1][3],
                                "over": ad["log"][-1][4], "mse_mean": mse(ad["mean"]),
                                "mse_denoised": mse(ad["denoised"]),
                                "tile_frames_histogram": {str(int(v)): int(c) for v, c in
                                                          zip(*np.unique(ad["tile_frames"], return_counts=True))},
                                "launch_log": [{"done_before": e[0], "tiles": e[1], "frames": e[2], "over_after": e[4],
                                                "ms": round(ms, 4)} for e, ms in zip(ad["log"], ad["launch_ms"])]}}
            run["adaptive_over_progressive_ms"] = round(run["adaptive"]["median_ms"] / run["progressive"]["median_ms"], 4)
            run["adaptive_over_progressive_rays"] = round(ad["rays"] / rays, 4)
            rec["runs"].append(run)
            print(json.dumps(run))

        # select and the tile fold on their own: over the identity list, and over a short list of a late launch's size
        fpl = a.fpl[0]
        ad = ds.render_adaptive(p, frames_per_launch=fpl, max_frames=a.max_frames, max_launch_frames=a.max_launch_frames,
                                tol=a.tol, share=a.share, denoise=False)
        A_last, k_last = (ad["log"][-1][1], ad["log"][-1][2]) if len(ad["log"]) > 1 else (n_tiles, fpl)
        tile_words = 3 * tw * th
        mean, m2, var = (torch.rand(3 * n, dtype=torch.float64, device=dev) for _ in range(3))
        var *= 1e-3
        lists = {"identity": (torch.arange(n_tiles, dtype=torch.int32, device=dev), n_tiles, fpl),
                 "last_launch": (torch.randperm(n_tiles, device=dev)[:A_last].sort().values.to(torch.int32), A_last, k_last)}
        out_list = torch.zeros(n_tiles, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        rec["passes"] = {}
        for name, (tl, n_l, k) in lists.items():
            buf = torch.rand(k * n_l * tile_words, dtype=torch.float64, device=dev)
            fns = {"select": lambda: render.accum_tiles_select_device(p, mean, var, out_list, count, tiles_in=tl, n_in=n_l,
                                                                      tol=a.tol, tile_share=a.share),
                   "tile_fold": lambda: render.accum_frames_tiles_device(buf, k, tl, n_l, tile_words, mean, m2, n_prior=4,
                                                                         var=var, n_state_tiles=n_tiles)}
            for fn in fns.values():
                fn()
            t = {key: [] for key in fns}
            for _ in range(a.reps):
                for key, fn in fns.items():
                    t[key].append(timed(lambda: [fn() for _ in range(a.calls)])[0] / a.calls)
            rec["passes"][name] = {"tiles": n_l, "frames": k, **{key: summary(v) for key, v in t.items()},
                                   "tile_fold_bytes": (8 * k + 48 + 24) * n_l * tile_words,
                                   "select_bytes": 48 * n_l * tw * th}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
