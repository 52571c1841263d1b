"""Device time of progressive accumulation (rp_accum_frames_device, rp_accum_error_device_ws) beside the launch whose
frames it folds and beside torch's own reduction of the same buffer.

The C3 scene at 1920 x 1080, 16 spp, one stream per pixel (samples_per_stream = spp), one launch of `--frames` (default
20) frames into one shard buffer.  After a warm-up of every shape, the launch, the fold of its frames
(rp_accum_frames_device with the variance), the error pass and, for scale, torch's `frames.view(n, -1).mean(0)` plus
`.var(0)` (and torch.var_mean, its one-call form) on the same buffer alternate for `--reps` repetitions in one session.
Each is timed by torch (HIP) events on one stream: the launch as one call, the others as `--calls` back-to-back calls --
the frames (1 GB) do not fit the 256 MiB Infinity Cache, so a repeated fold still streams them from HBM; the error pass's
100 MB of inputs do fit, and its figure is a cache-warm one.  Medians and ranges go to `--out` (default
profiles/r17/accum_time.json) with rp_build_id.  The fold's compulsory traffic is 8 B read per word and frame plus 24 B
written per word; the record gives bytes over time as a fraction of the 8 TB/s HBM peak -- how far from a copy the kernel
is, not a utilisation -- and the ratio to the torch route.

    python tools/accum_time.py --reps 5
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "raytracing-potato_amd")]

HBM_PEAK_BPS = 8.0e12


def summary(xs):
    ms = [1e3 * x for x in xs]
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r17", "accum_time.json"))
    a = ap.parse_args()
    assert a.reps >= 5, "at least 5 repetitions of each"
    assert a.frames >= 2
    from dataclasses import replace

    import numpy as np
    import torch

    from rtpotato import _ffi as F
    from rtpotato import render, scenes
    from rtpotato.scene import shard_slot_count
    scene, params = scenes.config_scene("C3")
    p = replace(params, spp=a.spp, samples_per_stream=a.spp)
    n, nf = shard_slot_count(p), a.frames
    words = 3 * n
    rec = {"tool": "tools/accum_time.py", "config": "C3", "width": p.width, "height": p.height, "spp": a.spp,
           "samples_per_stream": a.spp, "frames": nf, "shard_slots": n, "words": words,
           "build_id": F.rp().rp_build_id().decode(), "reps": a.reps,
           "timer": f"torch (HIP) events on one stream: the launch as one call, the others around {a.calls} "
                    "back-to-back calls",
           "hbm_peak_bytes_per_s": HBM_PEAK_BPS}
    dev = torch.device("cuda", 0)

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e-3 * e0.elapsed_time(e1) / calls

    with render.DeviceScene(scene) as ds:
        ds.reserve_frames(p, nf)
        frames = torch.zeros(nf * words, dtype=torch.float64, device=dev)
        mean, m2, var = (torch.zeros(words, dtype=torch.float64, device=dev) for _ in range(3))
        ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device=dev)
        stats = torch.zeros(F.RP_ERROR_STATS_LEN, dtype=torch.int64, device=dev)
        fv = frames.view(nf, -1)
        routes = {
            "launch": (lambda: ds.render_frames_device(p, nf, frames, ctr), 1),
            "accum_frames": (lambda: render.accum_frames_device(frames, nf, mean, m2, var=var), a.calls),
            "accum_error": (lambda: ds.accum_error_device(p, mean, var, stats), a.calls),
            "torch_mean_plus_var": (lambda: (fv.mean(0), fv.var(0)), a.calls),
            "torch_var_mean": (lambda: torch.var_mean(fv, 0), a.calls),
        }
        for fn, _ in routes.values():  # warm-up of every shape
            fn()
        torch.cuda.synchronize()
        assert int(ctr[3]) == 0
        # the two routes agree: the running mean and m2 / (n (n - 1)) against torch's mean and var / n
        tm, tv = fv.mean(0), fv.var(0) / nf
        rec["max_abs_mean_minus_torch"] = float((mean - tm).abs().max())
        rec["max_abs_var_minus_torch"] = float((var - tv).abs().max())
        assert torch.allclose(mean, tm, rtol=1e-12, atol=0.0)
        assert torch.allclose(var, tv, rtol=1e-9, atol=1e-12 * float(frames.max()) ** 2)
        first = [t.clone() for t in (mean, m2, var, stats)]
        times = {k: [] for k in routes}
        for _ in range(a.reps):  # alternating
            for k, (fn, calls) in routes.items():
                times[k].append(timed(fn, calls))
        for t, f in zip((mean, m2, var, stats), first):  # every repetition rendered and folded the same frames
            assert torch.equal(t.view(torch.uint8), f.view(torch.uint8))
        rec["error_stats"] = list(render.error_stats(stats.cpu().numpy()))
    for k, xs in times.items():
        rec[k] = summary(xs)
    nbytes = (8 * nf + 24) * words
    s = rec["accum_frames"]
    s.update({"compulsory_bytes": nbytes,
              "fraction_of_hbm_peak": round(nbytes / (s["median_ms"] * 1e-3) / HBM_PEAK_BPS, 4),
              "over_launch": round(s["median_ms"] / rec["launch"]["median_ms"], 5),
              "over_torch_mean_plus_var": round(s["median_ms"] / rec["torch_mean_plus_var"]["median_ms"], 4),
              "over_torch_var_mean": round(s["median_ms"] / rec["torch_var_mean"]["median_ms"], 4)})
    e = rec["accum_error"]
    ebytes = 48 * p.width * p.height
    e.update({"compulsory_bytes": ebytes, "cache_warm": True,
              "fraction_of_hbm_peak": round(ebytes / (e["median_ms"] * 1e-3) / HBM_PEAK_BPS, 4),
              "over_launch": round(e["median_ms"] / rec["launch"]["median_ms"], 6)})
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
