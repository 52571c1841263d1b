"""Device time of the guided denoiser (rp_denoise) beside the beauty frame (rp_render) and the feature pass
(rp_render_aov) it filters.

The C3 scene at 1920 x 1080 and 16 spp: the frame and its guides are rendered once to the host, then beauty, feature
pass and the filter at each of `--levels` (default L = 3 and 5) alternate for `--reps` repetitions after a warm-up of
each shape, every one timed by HIP events around its device work (rp_stats.seconds, rp_denoise's seconds).  Medians and
ranges go to `--out` (default profiles/r13/denoise_time.json) with rp_build_id.  The filter's compulsory traffic is 80
bytes read (rgb or the level's colour, normal, albedo, depth) and 24 written per pixel and level; the record gives that
over the filter's time as a fraction of the 8 TB/s HBM peak -- how far from a copy the kernel is, not a utilisation.

    python tools/denoise_time.py --reps 5
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "raytracing-potato_amd")]

HBM_PEAK_BPS = 8.0e12
BYTES_PER_PIXEL_LEVEL = 80 + 24


def summary(xs):
    ms = [1e3 * x for x in xs]
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--levels", default="3,5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r13", "denoise_time.json"))
    a = ap.parse_args()
    assert a.reps >= 5, "at least 5 repetitions of each"
    from dataclasses import replace

    import numpy as np

    from rtpotato import _ffi as F
    from rtpotato import render, scenes
    scene, params = scenes.config_scene("C3")
    p = replace(params, spp=a.spp)
    levels = [int(x) for x in a.levels.split(",")]
    px = p.width * p.height
    rec = {"tool": "tools/denoise_time.py", "config": "C3", "width": p.width, "height": p.height, "spp": a.spp,
           "build_id": F.rp().rp_build_id().decode(), "reps": a.reps,
           "timer": "HIP events (rp_stats.seconds, rp_denoise seconds)",
           "bytes_per_pixel_and_level": BYTES_PER_PIXEL_LEVEL, "hbm_peak_bytes_per_s": HBM_PEAK_BPS}
    with render.DeviceScene(scene) as ds:
        rgb, _, _ = ds.render(p)  # warm-up of each shape, and the filter's inputs
        aov = ds.render_aov(p, foreground=False)
        guides = (aov["normal"], aov["albedo"], aov["depth"])
        rec["miss_fraction"] = round(float((np.einsum("...k,...k", guides[0], guides[0]) == 0.0).mean()), 4)
        outs = {L: render.denoise(rgb, *guides, params={"iterations": L})[0] for L in levels}
        beauty, feature, filt = [], [], {L: [] for L in levels}
        for _ in range(a.reps):  # alternating
            beauty.append(ds.render(p)[2]["seconds"])
            feature.append(ds.render_aov(p, foreground=False)["stats"]["seconds"])
            for L in levels:
                out, sec = render.denoise(rgb, *guides, params={"iterations": L})
                assert np.array_equal(out, outs[L])  # every repetition is the same frame
                filt[L].append(sec)
    rec["beauty"], rec["aov"] = summary(beauty), summary(feature)
    rec["denoise"] = []
    for L in levels:
        s = summary(filt[L])
        nbytes = BYTES_PER_PIXEL_LEVEL * px * L
        rec["denoise"].append({"iterations": L, **s, "ms_per_level": round(s["median_ms"] / L, 3),
                               "compulsory_bytes": nbytes,
                               "fraction_of_hbm_peak": round(nbytes / (s["median_ms"] * 1e-3) / HBM_PEAK_BPS, 4),
                               "over_beauty": round(s["median_ms"] / rec["beauty"]["median_ms"], 4),
                               "finite": bool(np.isfinite(outs[L]).all())})
    rec[f"frame_ms_beauty_aov_denoise_L{levels[0]}"] = round(rec["beauty"]["median_ms"] + rec["aov"]["median_ms"] +
                                                rec["denoise"][0]["median_ms"], 3)
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
