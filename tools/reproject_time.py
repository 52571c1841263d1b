"""Device time of temporal reprojection (rp_reproject_device) and the per-pixel fold (rp_accum_frames_counts_device)
beside the plain fold (rp_accum_frames_device, tools/accum_time.py's) and a beauty frame.

The C3 scene at 1920 x 1080, 16 spp, one stream per pixel (samples_per_stream = spp).  Two poses: the catalogue camera and
the same camera stepped sideways by `--step` (default 0.05 scene units), each with its guides (render_aov_device) and
`--frames` (default 2) frames, assembled to frame order; pose 0's frames folded from zero counts give the state that is
reprojected.  After a warm-up of every shape, a 16-spp beauty frame, the reprojection, the per-pixel fold of pose 1's
frames, the plain fold of the same frames and the reprojection + fold chain alternate for `--reps` repetitions in one
session.  Each is timed by torch (HIP) events on one stream: the frame as one call, the others as `--calls` back-to-back
calls.  The reprojection's 350 MB and the fold's 370 MB of compulsory traffic exceed the 256 MiB Infinity Cache, so a
repeated call still streams most of its bytes from HBM.  Medians and ranges go to `--out` (default
profiles/r26/reproject_time.json) with rp_build_id and the pass's statistics.  Compulsory bytes per pixel -- the
reprojection: 32 of current guides, 84 of one previous pixel (depth, normal, mean, m2, count; the other taps are
neighbours' own pixels and come from cache) and 52 written; the fold: 24 per frame, 52 of state read, 76 written -- over
the time, as a fraction of the 8 TB/s HBM peak: how far from a copy a kernel is, not a utilisation.

    python tools/reproject_time.py --reps 5
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
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--step", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r26", "reproject_time.json"))
    a = ap.parse_args()
    assert a.reps >= 5, "at least 5 repetitions of each"
    assert a.frames >= 2
    from dataclasses import replace

    import torch

    from rtpotato import _ffi as F
    from rtpotato import render, scenes
    from rtpotato.scene import Transformation, shard_slot_count
    scene, params = scenes.config_scene("C3")
    p = replace(params, spp=a.spp, samples_per_stream=a.spp)
    w, h, n, nf = p.width, p.height, shard_slot_count(p), a.frames
    cam0 = scene.camera
    pos = cam0.transformation.position
    cam1 = replace(cam0, transformation=Transformation(cam0.transformation.orientation,
                                                       (pos[0] + a.step, pos[1], pos[2])))
    rec = {"tool": "tools/reproject_time.py", "config": "C3", "width": w, "height": h, "spp": a.spp,
           "samples_per_stream": a.spp, "frames_per_pose": nf, "camera_step": a.step,
           "build_id": F.rp().rp_build_id().decode(), "reps": a.reps,
           "timer": f"torch (HIP) events on one stream: the frame as one call, the others around {a.calls} "
                    "back-to-back calls",
           "hbm_peak_bytes_per_s": HBM_PEAK_BPS}
    dev = torch.device("cuda", 0)
    f64 = {"dtype": torch.float64, "device": dev}

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
        sp = render._stream_ptr(None, dev)
        ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device=dev)
        shard_rgb = torch.zeros(3 * n, **f64)
        pose = []
        for t, cam in enumerate((cam0, cam1)):
            shard_frames = torch.zeros(nf * 3 * n, **f64)
            ds.render_frames_device(replace(p, seed=p.seed + t * nf * w * h), nf, shard_frames, ctr, camera=cam)
            shard = {k: torch.zeros(c * n, **f64) for k, c in (("normal", 3), ("depth", 1))}
            ds.render_aov_device(p, normal=shard["normal"], depth=shard["depth"], camera=cam)
            g = {"normal": torch.zeros((h, w, 3), **f64), "depth": torch.zeros((h, w), **f64)}
            render._assemble(p, shard, g, sp)
            g["frames"] = torch.zeros((nf, h, w, 3), **f64)
            render._assemble(p, {f: shard_frames[f * 3 * n:(f + 1) * 3 * n] for f in range(nf)}, g["frames"], sp)
            pose.append(g)
        torch.cuda.synchronize()
        assert int(ctr[3]) == 0
        del shard_frames, shard
        mean0, m20 = torch.zeros((h, w, 3), **f64), torch.zeros((h, w, 3), **f64)
        count0 = torch.zeros((h, w), dtype=torch.int32, device=dev)
        render.accum_frames_counts_device(pose[0]["frames"], nf, count0, mean0, m20)
        mean, m2, var = (torch.zeros((h, w, 3), **f64) for _ in range(3))
        count = torch.zeros((h, w), dtype=torch.int32, device=dev)
        stats = torch.zeros(F.RP_REPROJECT_STATS_LEN, dtype=torch.int64, device=dev)
        pm, pq, pv = (torch.zeros(3 * w * h, **f64) for _ in range(3))  # the plain fold's state
        render.accum_frames_device(pose[0]["frames"], nf, pm, pq)
        prev_cam = render.reproject_prev_camera(cam0)

        def reproject():
            render.reproject_device(cam1, prev_cam, pose[1]["depth"], pose[1]["normal"], pose[0]["depth"],
                                    pose[0]["normal"], mean0, m20, count0, mean, m2, count, stats)

        def fold():
            render.accum_frames_counts_device(pose[1]["frames"], nf, count, mean, m2, var=var)

        def chain():
            reproject()
            fold()

        routes = {
            "beauty_frame": (lambda: ds.render_device(p, shard_rgb, ctr, camera=cam1), 1),
            "reproject": (reproject, a.calls),
            "accum_frames_counts": (fold, a.calls),  # the counts grow by nf per call: the same work every time
            "accum_frames": (lambda: render.accum_frames_device(pose[1]["frames"], nf, pm, pq, n_prior=nf, var=pv),
                             a.calls),
            "reproject_then_fold": (chain, a.calls),
        }
        for fn, _ in routes.values():  # warm-up of every shape
            fn()
        chain()
        torch.cuda.synchronize()
        rec["reproject_stats"] = render.reproject_stats(stats.cpu().numpy())
        rec["mean_count_after_fold"] = float(count.double().mean())
        first = [t.clone() for t in (mean, m2, var, count)]
        times = {k: [] for k in routes}
        for _ in range(a.reps):  # alternating
            for k, (fn, calls) in routes.items():
                times[k].append(timed(fn, calls))
        for t, f in zip((mean, m2, var, count), first):  # the last route left the chain's result: the same every time
            assert torch.equal(t.view(torch.uint8), f.view(torch.uint8))
    for k, xs in times.items():
        rec[k] = summary(xs)
    px = w * h
    for key, nbytes in (("reproject", (32 + 84 + 52) * px), ("accum_frames_counts", (24 * nf + 52 + 76) * px),
                        ("accum_frames", (24 * nf + 48 + 72) * px)):
        s = rec[key]
        s.update({"compulsory_bytes": nbytes,
                  "fraction_of_hbm_peak": round(nbytes / (s["median_ms"] * 1e-3) / HBM_PEAK_BPS, 4),
                  "over_beauty_frame": round(s["median_ms"] / rec["beauty_frame"]["median_ms"], 5)})
    rec["reproject"]["over_accum_frames"] = round(rec["reproject"]["median_ms"] / rec["accum_frames"]["median_ms"], 4)
    rec["accum_frames_counts"]["over_accum_frames"] = round(
        rec["accum_frames_counts"]["median_ms"] / rec["accum_frames"]["median_ms"], 4)
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
