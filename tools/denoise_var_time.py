"""Device time of the variance pass (rp_render_variance_device_ws) and the variance-guided denoiser (rp_denoise_var)
beside the guided denoiser (rp_denoise) and the beauty frame (rp_render) they follow.

The C3 scene at 1920 x 1080 and 16 spp with samples_per_stream = 4 (four batches per pixel): the frame, its batch
variance and its guides are made once, then beauty, the variance pass, the variance-guided filter and the guided filter
at each of `--levels` (default L = 3 and 5) alternate for `--reps` repetitions after a warm-up of each shape.  The
renders and the filters are timed by HIP events around their device work (rp_stats.seconds, the filters' seconds), the
variance pass -- a device call without a synchronous twin -- by torch events around `--pass-calls` back-to-back calls on
one stream (it only reads the batch sums, so it repeats).  Medians and ranges go to `--out` (default
profiles/r15/denoise_var_time.json) with rp_build_id.  Per pixel and level the variance-guided filter's compulsory
traffic is 88 bytes read (colour and variance -- the first level reads rgb and var, 48 --, normal, albedo, depth) and 32
written, the guided filter's 80 and 24; the variance pass reads 24 B per pixel and batch and writes 24.  The record
gives bytes over time as a fraction of the 8 TB/s HBM peak -- how far from a copy a kernel is, not a utilisation.

    python tools/denoise_var_time.py --reps 5
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "raytracing-potato_amd")]

HBM_PEAK_BPS = 8.0e12
BYTES_VAR = 88 + 32    # per pixel and level, variance-guided
BYTES_PLAIN = 80 + 24  # per pixel and level, guided


def summary(xs):
    ms = [1e3 * x for x in xs]
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--samples-per-stream", type=int, default=4)
    ap.add_argument("--levels", default="3,5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pass-calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r15", "denoise_var_time.json"))
    a = ap.parse_args()
    assert a.reps >= 5, "at least 5 repetitions of each"
    from dataclasses import replace

    import numpy as np
    import torch

    from rtpotato import _ffi as F
    from rtpotato import render, scenes
    from rtpotato.scene import shard_slot_count
    scene, params = scenes.config_scene("C3")
    p = replace(params, spp=a.spp, samples_per_stream=a.samples_per_stream)
    nbatch = -(-a.spp // a.samples_per_stream)
    levels = [int(x) for x in a.levels.split(",")]
    px = p.width * p.height
    n = shard_slot_count(p)
    rec = {"tool": "tools/denoise_var_time.py", "config": "C3", "width": p.width, "height": p.height, "spp": a.spp,
           "samples_per_stream": a.samples_per_stream, "batches": nbatch,
           "build_id": F.rp().rp_build_id().decode(), "reps": a.reps,
           "timer": "HIP events (rp_stats.seconds, rp_denoise / rp_denoise_var seconds); the variance pass: torch events "
                    f"around {a.pass_calls} calls on one stream",
           "bytes_per_pixel_and_level": {"variance_guided": BYTES_VAR, "guided": BYTES_PLAIN},
           "hbm_peak_bytes_per_s": HBM_PEAK_BPS}
    with render.DeviceScene(scene) as ds:
        rgb, _, _ = ds.render(p)  # warm-up of each shape, and the filters' inputs
        aov = ds.render_aov(p, foreground=False)
        guides = (aov["normal"], aov["albedo"], aov["depth"])
        ds.reserve(p)
        d_rgb = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
        d_var = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
        ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device="cuda")
        ds.render_device(p, d_rgb, ctr)
        ds.render_variance_device(p, d_var)
        torch.cuda.synchronize()
        assert np.array_equal(render.unpack_shard(p, d_rgb.cpu().numpy(), 3), rgb)
        var = render.unpack_shard(p, d_var.cpu().numpy(), 3)
        rec["miss_fraction"] = round(float((np.einsum("...k,...k", guides[0], guides[0]) == 0.0).mean()), 4)
        rec["zero_variance_fraction"] = round(float((var == 0.0).all(-1).mean()), 4)
        outs = {L: (render.denoise(rgb, *guides, params={"iterations": L}, variance=var)[0],
                    render.denoise(rgb, *guides, params={"iterations": L})[0]) for L in levels}
        beauty, vpass, filt, plain = [], [], {L: [] for L in levels}, {L: [] for L in levels}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(a.reps):  # alternating
            beauty.append(ds.render(p)[2]["seconds"])
            ds.render_device(p, d_rgb, ctr)  # the sums the pass reads
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.pass_calls):
                ds.render_variance_device(p, d_var)
            e1.record()
            torch.cuda.synchronize()
            vpass.append(1e-3 * e0.elapsed_time(e1) / a.pass_calls)
            for L in levels:
                out, sec = render.denoise(rgb, *guides, params={"iterations": L}, variance=var)
                assert np.array_equal(out, outs[L][0])  # every repetition is the same frame
                filt[L].append(sec)
                out, sec = render.denoise(rgb, *guides, params={"iterations": L})
                assert np.array_equal(out, outs[L][1])
                plain[L].append(sec)
        assert np.array_equal(render.unpack_shard(p, d_var.cpu().numpy(), 3), var)
    rec["beauty"] = summary(beauty)
    s = summary(vpass)
    nbytes = (24 * nbatch + 24) * px
    rec["variance_pass"] = {**s, "compulsory_bytes": nbytes,
                            "fraction_of_hbm_peak": round(nbytes / (s["median_ms"] * 1e-3) / HBM_PEAK_BPS, 4),
                            "over_beauty": round(s["median_ms"] / rec["beauty"]["median_ms"], 5)}
    rec["denoise_var"], rec["denoise"] = [], []
    for L in levels:
        for key, xs, per, o in (("denoise_var", filt[L], BYTES_VAR, outs[L][0]), ("denoise", plain[L], BYTES_PLAIN, outs[L][1])):
            s = summary(xs)
            nbytes = per * px * L
            rec[key].append({"iterations": L, **s, "ms_per_level": round(s["median_ms"] / L, 3),
                             "compulsory_bytes": nbytes,
                             "fraction_of_hbm_peak": round(nbytes / (s["median_ms"] * 1e-3) / HBM_PEAK_BPS, 4),
                             "over_beauty": round(s["median_ms"] / rec["beauty"]["median_ms"], 4),
                             "finite": bool(np.isfinite(o).all())})
        rec["denoise_var"][-1]["over_denoise"] = round(rec["denoise_var"][-1]["median_ms"] / rec["denoise"][-1]["median_ms"], 4)
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
