"""Device time of a refit (rp_scene_refit_device) beside what it replaces, a fresh rp_scene_create, and what it loses:
the speed of a frame on the refit tree against a freshly built tree of the same geometry.

Part 1, per scene -- bunny_full (C3's), and `--sizes` (default 1 M and 10 M) random triangles (C5's generator) -- and per
node format (f32, q8), with the PLOC builder: rp_scene_build_times of the create; rp_refit_create's host time; the
refit to the tests' deformation (tests/refit_ref.py: p + a sin(3 p.yzx), a = 0.05 of the extent, radii x 1.1) from
device arrays, timed by torch (HIP) events around `--calls` back-to-back calls, `--reps` repetitions alternating between
the deformed and the original geometry (so every call moves every box).  Compulsory bytes per triangle -- 72 of
positions and 72 of normals gathered, 16 of PrimRef and 8 of the record's tail read, 80 + 72 + 48 written; per node its
record and up to four 48 B boxes read, the box words and 48 B written -- are not summed into a rate here: the vertex
gather's reuse decides the traffic.

Part 2, the quality a refit loses: C3's scene at 1920 x 1080, 16 spp, one stream per pixel, the default tree.  For
deformations of growing amplitude (`--amps`, fractions of the extent) one frame on the refit scene and on a scene
created from the deformed description, alternating, `--reps` each; the two frames are compared bit for bit.  Here the
radii are kept (the ground sphere grown by a tenth would enclose the camera and change the workload, not the tree).

These are records, not thresholds.  Written to `--out` (default profiles/r32/refit_time.json) with rp_build_id.

    python tools/refit_time.py --reps 5
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "raytracing-potato_amd"), os.path.join(REPO, "tests")]


def summary(xs):
    ms = [1e3 * x for x in xs]
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1_000_000, 10_000_000])
    ap.add_argument("--amps", type=float, nargs="*", default=[0.0, 0.01, 0.05, 0.2])
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "r32", "refit_time.json"))
    a = ap.parse_args()
    assert a.reps >= 3
    from dataclasses import replace

    import numpy as np
    import torch

    import refit_ref as RR
    from rtpotato import _ffi as F
    from rtpotato import render, scenes
    from rtpotato.scene import shard_slot_count

    dev = torch.device("cuda", 0)
    rec = {"tool": "tools/refit_time.py", "build_id": F.rp().rp_build_id().decode(), "reps": a.reps,
           "timer": f"torch (HIP) events on one stream around {a.calls} back-to-back refits; a frame as one call",
           "deformation": "p + a sin(3 p.yzx), normals n.yzx, radii x 1.1 (tests/refit_ref.py deform)", "scenes": []}

    def timed(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e-3 * e0.elapsed_time(e1) / calls

    def to_dev(g):
        return [torch.from_numpy(np.ascontiguousarray(g[k])).to(dev) if len(g[k]) else None
                for k in ("positions", "normals", "spheres")]

    # ---- part 1: the refit beside the create
    cases = [("bunny_full", scenes.bunny_full)] + [(f"random_mesh_{n}", lambda n=n: scenes.random_mesh(n)) for n in a.sizes]
    for name, make in cases:
        sc = make()
        g0 = render.scene_geometry(sc)
        g1 = RR.deform(g0, 0.05)
        amax = max(float(np.abs(g[k]).max()) for g in (g0, g1) for k in ("positions",) if len(g[k]))
        for fmt in ("f32", "q8"):
            t0 = time.perf_counter()
            with render.DeviceScene(sc, options={"builder": "ploc", "node_format": fmt}) as ds:
                create_s = time.perf_counter() - t0
                t0 = time.perf_counter()
                with ds.refit_handle(coord_max=4.0 * amax + 2200.0) as rf:
                    plan_s = time.perf_counter() - t0
                    d0, d1 = to_dev(g0), to_dev(g1)
                    status = torch.zeros(1, dtype=torch.int32, device=dev)
                    flip = [0]

                    def refit():
                        flip[0] ^= 1
                        rf.update_device(*(d1 if flip[0] else d0), status=status)

                    refit(), refit()
                    torch.cuda.synchronize()
                    assert int(status[0]) == 0
                    times = [timed(refit, a.calls) for _ in range(a.reps)]
                    assert int(status[0]) == 0
                    row = {"scene": name, "node_format": fmt, "builder": "ploc", **ds.info(), "refit_info": rf.info(),
                           "build_times_s": ds.build_times(), "scene_create_wall_s": round(create_s, 4),
                           "refit_create_wall_s": round(plan_s, 4), "refit": summary(times)}
            bt = row["build_times_s"]
            row["tree_build_s"] = round(bt["device_input"] + bt["device_build_or_upload"], 4)
            row["refit_over_tree_build"] = round(row["refit"]["median_ms"] * 1e-3 / max(row["tree_build_s"], 1e-9), 5)
            row["refit_over_scene_create"] = round(row["refit"]["median_ms"] * 1e-3 / create_s, 6)
            print(json.dumps(row), flush=True)
            rec["scenes"].append(row)
            del d0, d1
        del sc, g0, g1

    # ---- part 2: a frame on the refit tree against a fresh tree
    scene, params = scenes.config_scene("C3")
    p = replace(params, spp=a.spp, samples_per_stream=a.spp)
    n = shard_slot_count(p)
    g0 = render.scene_geometry(scene)
    rec["quality"] = {"config": "C3", "width": p.width, "height": p.height, "spp": a.spp, "rows": []}
    out = [torch.zeros(3 * n, dtype=torch.float64, device=dev) for _ in range(2)]
    ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device=dev)
    with render.DeviceScene(scene) as ds, ds.refit_handle(coord_max=4096.0) as rf:
        for amp in a.amps:
            g = RR.deform(g0, amp) if amp else {k: v.copy() for k, v in g0.items()}
            g["spheres"][:, 3] = g0["spheres"][:, 3]  # radii kept: the ground sphere x 1.1 would swallow the camera
            assert rf.update(g["positions"], g["normals"], g["spheres"])[0] == 0
            with render.DeviceScene(render.with_geometry(scene, g["positions"], g["normals"], g["spheres"])) as fresh:
                routes = {"refit_tree": lambda: ds.render_device(p, out[0], ctr),
                          "fresh_tree": lambda: fresh.render_device(p, out[1], ctr)}
                for fn in routes.values():
                    fn(), fn()
                times = {k: [] for k in routes}
                for _ in range(a.reps):
                    for k, fn in routes.items():
                        times[k].append(timed(fn, 1))
                same = bool(torch.equal(out[0].view(torch.uint8), out[1].view(torch.uint8)))
            row = {"amplitude_of_extent": amp, "frames_equal": same, **{k: summary(v) for k, v in times.items()}}
            row["refit_over_fresh"] = round(row["refit_tree"]["median_ms"] / row["fresh_tree"]["median_ms"], 4)
            print(json.dumps(row), flush=True)
            rec["quality"]["rows"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
