"""What a render decides before its first launch (raytracing-potato_amd/csrc/rp_schedule.h rps::plan_launch, called by
rp_render.cpp's render_shard), checked on the header's own code through the librp_host.so test hook rph_plan_launch:
the per-XCD queue and chunk choice, the frame order of multi-frame launches, the refusals, the unit decode's division
constants, the balanced plan's block size and the gather block sizes.  The expected queue choices are the ones DESIGN.md
4.3 / 4.9 measured; the GPU tests exercise the kernel's use of the numbers."""
import ctypes

import pytest

from test_udiv import make_div32

LANES = 262_144  # 256 CUs x 16 one-wave blocks x 64 lanes


def plan(p, n_frames=1, frame_order=0, unit_queues=0, queue_chunk=0, lanes=LANES, check=True):
    """rph_plan_launch for RenderParams p -> (code, rph_launch_plan); check: raise on a refusal."""
    from rtpotato import _ffi as F
    out = F.rph_launch_plan()
    rc = F.host().rph_plan_launch(p.width, p.height, p.spp, p.max_bounce, p.tile_w, p.tile_h, p.shard, p.num_shards,
                                  p.samples_per_stream, p.shard_map, n_frames, frame_order, unit_queues, queue_chunk,
                                  lanes, ctypes.byref(out))
    if check:
        F.check_host(rc)
    return rc, out


def plan_block(n_tiles_params, world):
    """rps::plan_block for the frame of params on `world` ranks."""
    from dataclasses import replace
    return plan(replace(n_tiles_params, shard=0, num_shards=world))[1].plan_block


def _frame(**kw):
    from rtpotato.scene import RenderParams
    return RenderParams(1920, 1080, 256, 8, 3, **kw)


def _cases():
    from rtpotato import _ffi as F
    PIXEL, SEQ = F.RP_FRAME_ORDER_PIXEL, F.RP_FRAME_ORDER_SEQUENTIAL
    # (params kw, hook kw) -> (queue_groups, queue_chunk, frames_inter); None: not stated
    return [
        ({}, {}, (8, 8, 0)),                                               # whole frame, 2,040 tiles
        ({"shard": 0, "num_shards": 8}, {}, (None, 1, None)),              # 255 tiles
        ({}, {"n_frames": 20, "frame_order": PIXEL}, (None, 20, 2)),
        ({}, {"n_frames": 16, "frame_order": PIXEL}, (None, 16, 2)),
        ({}, {"n_frames": 20, "frame_order": SEQ}, (None, 8, 0)),
        ({}, {"n_frames": 20, "frame_order": PIXEL, "queue_chunk": 3}, (None, 3, 1)),
        ({}, {"n_frames": 20, "frame_order": PIXEL, "unit_queues": F.RP_QUEUES_SINGLE}, (1, 1, 2)),
        ({}, {"unit_queues": F.RP_QUEUES_XCD_REGIONS}, (None, 255, None)),
    ]


@pytest.mark.parametrize("case", range(8))
def test_queue_and_chunk_choice(case):
    pkw, hkw, want = _cases()[case]
    _, o = plan(_frame(**pkw), **hkw)
    got = (o.queue_groups, o.queue_chunk, o.frames_inter)
    assert all(w is None or w == g for w, g in zip(want, got)), (case, got, want)
    assert o.n_shard_tiles == (255 if pkw else 2040) and o.sortable == 1 and o.measure == 1
    nf = hkw.get("n_frames", 1)
    assert o.n_queue == o.n_slots * 8 * nf and o.out_stride == 3 * o.n_slots
    assert o.grid == min(-(-o.n_queue // 64), LANES // 64)


def test_refusals():
    from rtpotato import _ffi as F
    from rtpotato.scene import RenderParams
    # tests/test_gpu_configs.py test_shards_of_2_31_units_are_refused: 8192 x 8192 pixels x 32 batches on one queue
    big = RenderParams(8192, 8192, 1024, 8, 3)
    rc, o = plan(big, unit_queues=F.RP_QUEUES_SINGLE, check=False)
    assert rc == F.RP_EINVAL and "2^31" in F.host().rph_last_error().decode() and o.n_queue == 1 << 31
    rc, _ = plan(big, check=False)  # per-XCD queues: the queue word's bound comes first
    assert rc == F.RP_EINVAL and "2^32" in F.host().rph_last_error().decode()
    assert plan(RenderParams(8192, 8192, 1024 - 32, 8, 3), unit_queues=F.RP_QUEUES_SINGLE)[1].n_queue == 31 << 26
    for nf in (0, F.RP_MAX_FRAMES + 1):
        rc, _ = plan(_frame(), n_frames=nf, check=False)
        assert rc == F.RP_EINVAL and "n_frames" in F.host().rph_last_error().decode()
    assert plan(_frame(), n_frames=F.RP_MAX_FRAMES, frame_order=F.RP_FRAME_ORDER_SEQUENTIAL)[0] == F.RP_OK
    rc, _ = plan(RenderParams(1920, 1080, 256, 0, 3), check=False)
    assert rc == F.RP_EINVAL and "max_bounce" in F.host().rph_last_error().decode()
    rc, _ = plan(_frame(), frame_order=4, check=False)
    assert rc == F.RP_EINVAL


def test_division_constants():
    for pkw, hkw, _ in _cases():
        _, o = plan(_frame(**pkw), **hkw)
        assert tuple(o.dv_units) == make_div32(32 * 32 * 8)
        assert tuple(o.dv_tiles_x) == make_div32(60)
        assert tuple(o.dv_chunk) == make_div32(o.queue_chunk)
    from rtpotato.scene import RenderParams
    _, o = plan(RenderParams(75, 41, 70, 8, 3, tile_w=16, tile_h=8, samples_per_stream=32))
    assert tuple(o.dv_units) == make_div32(16 * 8 * 3) and tuple(o.dv_tiles_x) == make_div32(5)


def test_plan_block_is_the_restatement():
    from rtpotato.scene import RenderParams
    for (W, H, tile) in ((4096, 4096, 32), (1920, 1080, 32), (512, 512, 8), (520, 488, 8), (64, 36, 16)):
        p = RenderParams(W, H, 1, 8, 0, tile_w=tile, tile_h=tile)
        n = -(-W // tile) * -(-H // tile)
        for world in (1, 2, 3, 8):
            assert plan_block(p, world) == next((b for b in (4, 2) if n >= 32 * world * b * b), 1), (W, H, world)


@pytest.mark.parametrize("W,H,tile,world", [(75, 41, 16, 3), (1920, 1080, 32, 8)])
def test_gather_sizes_match_the_library(W, H, tile, world):
    """rps::pack_words / stage_slots through the hook = rp_frames_block_words / rp_gather_stride (host-only calls of
    librp.so: they load and answer without a GPU)."""
    from rtpotato import _ffi as F
    from rtpotato.scene import RenderParams
    for shard in (0, world - 1):
        p = RenderParams(W, H, 4, 8, 3, tile_w=tile, tile_h=tile, shard=shard, num_shards=world)
        c = p.to_c()
        stride = ctypes.c_uint64()
        F.check(F.rp().rp_gather_stride(ctypes.byref(c), ctypes.byref(stride)))
        for nf in (1, 20):
            words = ctypes.c_uint64()
            F.check(F.rp().rp_frames_block_words(ctypes.byref(c), nf, ctypes.byref(words)))
            _, o = plan(p, n_frames=nf)
            assert (o.block_words, o.gather_stride) == (words.value, stride.value), (shard, nf)
    tiles0 = -(-(-(-W // tile) * -(-H // tile)) // world)
    assert stride.value == tiles0 * tile * tile
