"""The launch plans pinned: every field rph_plan_launch and rph_plan_tiles_launch report (rp_schedule.h's plan_launch
and plan_tiles_launch through librp_host.so), compared with tests/golden/launch_plans.json -- written out from the build
before plan_launch was split into a frame step and a tile-count step, so the split launches what the one function did.

Inputs: frames 1 x 1, 72 x 40 and 1920 x 1080; tiles 16 and 32; shard 0 of 1, 0 of 3 and 2 of 3; 1 and 3 sample batches
per pixel; 1, 4 and 20 frames per launch; the four frame orders; every queue mode, the chunk 0, 1 and 5 where the mode
reads it (per-XCD tiles); for the tile list, 0, 1, half and all of the frame's tiles.  The full product is a few thousand
plans, so the fixture holds a diagonal slice of it: shape i (frame, tiles, shard or list, batches) meets schedule j
(frames per launch, order, queues, chunk) when (i + j) % 7 == 0.  The queue settings repeat with period 6 along j and
the (shard, batches) pairs with period 6 along i; 7 is coprime to both, so every pair meets every queue setting, every
queue setting every frame count and order, and every shape 10 or 11 schedules: 371 and 205 plans.

`python tests/test_launch_plans.py` writes the fixture from the library in use (RP_HOST_LIB names another)."""
import ctypes
import itertools
import json
import os

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_plans.json")
LANES = 262_144  # 256 CUs x 16 one-wave blocks x 64 lanes
FRAMES = ((1, 1), (72, 40), (1920, 1080))
TILES = (16, 32)
SHARDS = ((0, 1), (0, 3), (2, 3))
BATCHES = ((4, 4), (5, 2))  # (spp, samples_per_stream): 1 and 3 batches
# (n_frames, frame_order, unit_queues, queue_chunk): RP_FRAME_ORDER_* 0..3; RP_QUEUES_* auto, single, xcd_tiles, xcd_regions
SCHEDULES = list(itertools.product((1, 4, 20), range(4), ((0, 0), (1, 0), (2, 0), (2, 1), (2, 5), (3, 0))))
STRIDE = 7


def _slice(shapes):
    return [(s, (nf, order, q, chunk)) for i, s in enumerate(shapes) for j, (nf, order, (q, chunk)) in enumerate(SCHEDULES)
            if (i + j) % STRIDE == 0]


def cases():
    """(rph_plan_launch's arguments, rph_plan_tiles_launch's arguments): lists of tuples, without the out pointer."""
    shapes = list(itertools.product(FRAMES, TILES, SHARDS, BATCHES))
    full = [(w, h, spp, 8, t, t, shard, n, sps, 0, nf, order, q, chunk, LANES)
            for ((w, h), t, (shard, n), (spp, sps)), (nf, order, q, chunk) in _slice(shapes)]
    lists = []
    for (w, h), t in itertools.product(FRAMES, TILES):
        n_tiles = -(-w // t) * -(-h // t)
        lists += [(w, h, t, n) for n in sorted({0, 1, n_tiles // 2, n_tiles})]
    tiles = [(w, h, 4, 8, t, t, 4, n_listed, nf, order, q, chunk, LANES)
             for (w, h, t, n_listed), (nf, order, q, chunk) in _slice(lists)]
    return full, tiles


def _fields():
    from rtpotato import _ffi as F
    return [f for f, _ in F.rph_launch_plan._fields_]


def plans():
    """What the library in use plans for cases(): per call [its arguments, its return code, every field of the plan]."""
    from rtpotato import _ffi as F
    out = {}
    for name, args in zip(("rph_plan_launch", "rph_plan_tiles_launch"), cases()):
        fn, rows = getattr(F.host(), name), []
        for a in args:
            p = F.rph_launch_plan()
            rc = fn(*a, ctypes.byref(p))
            vals = [getattr(p, f) for f in _fields()]
            rows.append([list(a), rc, [list(v) if hasattr(v, "__len__") else v for v in vals]])
        out[name] = rows
    return {"fields": _fields(), **out}


def test_launch_plans_are_the_pinned_ones():
    with open(FIXTURE) as f:
        want = json.load(f)
    got = plans()
    assert got["fields"] == want["fields"]
    for name in ("rph_plan_launch", "rph_plan_tiles_launch"):
        assert len(got[name]) == len(want[name]) >= 200, name  # 36 and 20 shapes with 10 or 11 schedules each
        for g, w in zip(got[name], want[name]):
            assert g[0] == w[0], (name, "the cases moved: the fixture is of other inputs", g[0], w[0])
            assert g[1] == w[1], (name, g[0], "return code")
            for f, a, b in zip(want["fields"], g[2], w[2]):
                assert a == b, (name, g[0], f, a, b)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(FIXTURE), "..", "..", "raytracing-potato_amd"))
    got = plans()
    with open(FIXTURE, "w") as f:
        f.write('{"fields": ' + json.dumps(got["fields"]))
        for name in ("rph_plan_launch", "rph_plan_tiles_launch"):
            f.write(',\n"' + name + '": [\n' + ",\n".join(json.dumps(r, separators=(",", ":")) for r in got[name]) + "\n]")
        f.write("}\n")
    print({k: len(v) for k, v in got.items()})
