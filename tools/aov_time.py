"""Device time of the first-hit feature pass (rp_render_aov) against the beauty frame (rp_render) at the same spp.

The C3 scene at 1920 x 1080, at 16 and at 256 spp, both timed by rp_stats.seconds (HIP events around the device
work), in one process: a warm-up of each shape, then the two alternating for `--reps` repetitions each.  Medians and
ranges go to `--out` (default profiles/r11/aov_time.json) with rp_build_id.  The pass traces one ray per sample and
pays a stream key and a keystream block for each; a beauty sample traces ~2.7 rays and amortises its stream over 32
samples -- the record says which effect wins.

    python tools/aov_time.py --reps 5
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "raytracing-potato_amd")]


def summary(xs):
    ms = [1e3 * x for x in xs]
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", default="16,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r11", "aov_time.json"))
    a = ap.parse_args()
    assert a.reps >= 5, "at least 5 repetitions of each"
    from dataclasses import replace

    from rtpotato import _ffi as F
    from rtpotato import render, scenes
    scene, params = scenes.config_scene("C3")
    rec = {"tool": "tools/aov_time.py", "config": "C3", "width": params.width, "height": params.height,
           "build_id": F.rp().rp_build_id().decode(), "reps": a.reps, "timer": "rp_stats.seconds (HIP events)",
           "cases": []}
    with render.DeviceScene(scene) as ds:
        for spp in (int(s) for s in a.spp.split(",")):
            p = replace(params, spp=spp)
            ds.render(p)       # warm-up of each shape
            ds.render_aov(p)
            beauty, aov, aov_guides = [], [], []
            for _ in range(a.reps):  # alternating
                _, _, st = ds.render(p)
                beauty.append(st["seconds"])
                out = ds.render_aov(p)
                aov.append(out["stats"]["seconds"])
                rays_b, rays_a = st["rays"], out["stats"]["rays"]
                aov_guides.append(ds.render_aov(p, depth=False, foreground=False)["stats"]["seconds"])
            b, v = summary(beauty), summary(aov)
            case = {"spp": spp, "beauty": b, "aov": v, "aov_normal_albedo_only": summary(aov_guides),
                    "beauty_rays": rays_b, "aov_rays": rays_a,
                    "aov_over_beauty": round(v["median_ms"] / b["median_ms"], 4),
                    "aov_mrays_per_s": round(rays_a / (v["median_ms"] * 1e-3) / 1e6, 1),
                    "beauty_mrays_per_s": round(rays_b / (b["median_ms"] * 1e-3) / 1e6, 1)}
            print(json.dumps(case))
            rec["cases"].append(case)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
