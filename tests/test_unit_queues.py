"""The render kernel's unit fetch, walked on the CPU: raytracing-potato_amd/csrc/rp_units.h fetch_pixel (with unit_frame
and unit_spp) is the text the kernel compiles, and the librp_host.so test hook rph_unit_walk runs it in a host
environment -- blocks of one lane fetching in rounds from real queue words, on a launch planned by rp_schedule.h
plan_launch (tests/test_schedule.py checks its choices).  Every unit of every frame must come out exactly once, at the
right pixel, whatever the queues, the frame order and the tile, map and unit orders; a unit that went missing or was
handed out twice shows here and not as a wrong pixel on a GPU (the GPU test test_unit_queues_bitwise checks the kernel
renders identical frames)."""
import ctypes
import itertools
from types import SimpleNamespace

import numpy as np
import pytest

QUEUE_STRIDE, QUEUE_PROBE, QUEUE_WORDS = 32, 256, 288  # rp_kernel.h
SEQUENTIAL, INTERLEAVED, PIXEL = 1, 2, 3               # rp.h RP_FRAME_ORDER_*
SINGLE, XCD_TILES, XCD_REGIONS = 1, 2, 3               # rp.h RP_QUEUES_*
SLOT, PI, PJ, BATCH, BLOCK, QUEUE, FRAME, SPP = range(8)


def walk(width, height, tw, th, spp=1, sps=32, shard=0, shards=1, n_frames=1, frame_order=SEQUENTIAL,
         unit_queues=XCD_TILES, queue_chunk=0, tile_order=None, tile_map=None, unit_order=None, probe=0, groups=0,
         n_blocks=1, any_every=0, check=True):
    """rph_unit_walk -> units (n x 8, fetch order), final queue words, entries per word, forced votes."""
    from rtpotato import _ffi as F
    nbatch = -(-spp // sps)
    tiles = -(-width // tw) * -(-height // th)
    cap = len(range(shard, tiles, shards)) * tw * th * max(nbatch, 1) * n_frames + 1
    units = np.zeros((cap, 8), np.uint32)
    words, entries = np.zeros(QUEUE_WORDS, np.uint32), np.zeros(QUEUE_WORDS, np.uint32)
    n, forced = ctypes.c_uint64(), ctypes.c_uint64()
    arrays = [None if a is None else np.ascontiguousarray(a, np.uint32) for a in (tile_order, tile_map, unit_order)]
    rc = F.host().rph_unit_walk(width, height, spp, 8, tw, th, shard, shards, sps, 1 if tile_map is not None else 0,
                                n_frames, frame_order, unit_queues, queue_chunk,
                                *[None if a is None else a.ctypes.data for a in arrays], probe, groups, n_blocks,
                                any_every, units.ctypes.data, cap, ctypes.byref(n), words.ctypes.data,
                                entries.ctypes.data, ctypes.byref(forced))
    if check:
        F.check_host(rc)
    return SimpleNamespace(rc=rc, units=units[:n.value].astype(np.int64), words=words.astype(np.int64),
                           entries=entries.astype(np.int64), forced=forced.value)


# ---- the partition of the order's tiles among the queues: K tiles of one pixel and one unit each, slot = tile

def queue_tiles(K, G, C, regions=False):
    """Per queue, the tiles it handed out, in its order -- read from a walk by G blocks."""
    w = walk(K, 1, 1, 1, unit_queues=SINGLE if G == 1 else XCD_REGIONS if regions else XCD_TILES, queue_chunk=C,
             groups=0 if G in (1, 8) else G, n_blocks=G)
    assert len(w.units) == K
    return [list(w.units[w.units[:, QUEUE] == g, SLOT]) for g in range(G)]


@pytest.mark.parametrize("K", [1, 2, 7, 8, 9, 63, 64, 65, 255, 2040])
@pytest.mark.parametrize("G,C", [(1, 1), (8, 1), (8, 2), (8, 3), (8, 16), (3, 5)])
def test_queues_partition_the_tiles(K, G, C):
    seen = []
    for tiles in queue_tiles(K, G, C):
        assert tiles == sorted(tiles)  # each queue keeps the order's sequence
        seen += tiles
    assert sorted(seen) == list(range(K))


@pytest.mark.parametrize("K", [1, 6, 8, 2040, 4999])
def test_regions_mode_is_one_chunk_per_queue(K):
    """XCD_REGIONS = chunk ceil(K / G): queue g serves one contiguous run of the order."""
    G = 8
    C = (K + G - 1) // G
    for g, tiles in enumerate(queue_tiles(K, G, C, regions=True)):
        assert tiles == list(range(min(g * C, K), min((g + 1) * C, K)))


# ---- every unit of every frame exactly once, at the right pixel

def geometry(W, H, tw, th, shard, shards, tile_map=None):
    """rp_shard_unpack's geometry, stated once: the frame's tiles row-major, dealt to the shards position by position
    (position shard + k * shards of the deal order -- the tile index itself, or tile_map's entry -- is shard tile k);
    shard tile k's pixels are the slots k * tw * th + row-major offset inside the tile.  -> per slot pi, pj, and
    whether the pixel lies in the frame."""
    tiles_x, tiles_y = -(-W // tw), -(-H // th)
    pos = np.arange(shard, tiles_x * tiles_y, shards)
    t = pos if tile_map is None else np.asarray(tile_map)[pos]
    k, lj, li = np.meshgrid(np.arange(len(pos)), np.arange(th), np.arange(tw), indexing="ij")
    pi, pj = (t[k] % tiles_x) * tw + li, (t[k] // tiles_x) * th + lj
    return SimpleNamespace(pi=pi.ravel(), pj=pj.ravel(), inside=((pi < W) & (pj < H)).ravel(), n_tiles=tiles_x * tiles_y,
                           n_shard_tiles=len(pos), tiles_x=tiles_x)


def check_walk(w, c, g, frames_inter):
    """What every walk of a render must satisfy (c: the case, g: its geometry)."""
    u = w.units
    nbatch = -(-c.spp // c.sps)
    slots = np.flatnonzero(g.inside)
    # the multiset of (slot, global batch): the in-frame slots x 0 .. n_frames * nbatch - 1, each once
    got = np.sort(u[:, SLOT] * (c.n_frames * nbatch) + u[:, BATCH])
    want = (slots[:, None] * (c.n_frames * nbatch) + np.arange(c.n_frames * nbatch)[None, :]).ravel()
    assert np.array_equal(got, want)
    if len(want) == 0:  # (a shard without tiles: every lane retires on its first fetch)
        assert not w.entries.any()
        return
    assert np.array_equal(u[:, PI], g.pi[u[:, SLOT]]) and np.array_equal(u[:, PJ], g.pj[u[:, SLOT]])
    # frame and batch within the frame; a unit's samples; spp per pixel and frame
    b = u[:, BATCH] - u[:, FRAME] * nbatch
    assert np.array_equal(u[:, FRAME], u[:, BATCH] // nbatch) and b.min() >= 0 and b.max() < nbatch
    assert np.array_equal(u[:, SPP], np.minimum(c.sps, c.spp - b * c.sps))
    per_pixel = np.zeros((len(g.inside), c.n_frames), np.int64)
    np.add.at(per_pixel, (u[:, SLOT], u[:, FRAME]), u[:, SPP])
    assert (per_pixel[slots] == c.spp).all()
    assert u[:, BLOCK].max() < c.n_blocks
    # the queue words: only the launch's own, each at most the launch's entries plus one failed fetch per lane --
    # a failed fetch on a drained queue is followed, in the same fetch, by an entry from another queue or by the lane's
    # retirement (rp_schedule.h launch_limits' premise; with one queue: its entries plus the lanes)
    G = 1 if c.unit_queues == SINGLE else 8
    own = np.arange(G) * QUEUE_STRIDE
    assert w.entries.sum() == w.entries[own].sum() == g.n_shard_tiles * c.tw * c.th * nbatch * c.n_frames
    assert (w.words >= w.entries).all() and w.words.sum() == w.words[own].sum()
    assert (w.words[own] <= w.entries.sum() + c.n_blocks).all()
    if G == 1:
        assert w.words[0] <= w.entries[0] + c.n_blocks
    local = u[:, SLOT] % (c.tw * c.th)
    if (frames_inter == 2 and c.unit_order is None) or (G == 1 and c.unit_order is not None):
        # RP_FRAME_ORDER_PIXEL: a queue hands out a unit's frames one after the other (so does a unit order, position by
        # position -- its chunks of positions may part a unit's frames between two queues)
        for q in range(G):
            f = u[u[:, QUEUE] == q][:, [SLOT, BATCH, FRAME]]
            assert len(f) % c.n_frames == 0
            f = f.reshape(-1, c.n_frames, 3)
            assert (f[:, :, 0] == f[:, :1, 0]).all() and (f[:, :, 1] - f[:, :, 2] * nbatch == f[:, :1, 1]).all()
            assert (f[:, :, 2] == np.arange(c.n_frames)).all()
    if G == 1 and c.unit_order is None and c.tile_order is None:
        # one queue, no order: tile-major, then pixel-major, a pixel's batches consecutive (rp_units.h "queue order") --
        # frame by frame, or a tile's frames together, or (PIXEL) a unit's frames together
        k = u[:, SLOT] // (c.tw * c.th)
        key = {0: (u[:, FRAME], k, local, b), 1: (k, u[:, FRAME], local, b), 2: (k, local, b, u[:, FRAME])}[frames_inter]
        rank = np.lexsort(key[::-1])
        assert np.array_equal(rank, np.arange(len(u)))


SHAPES = [(37, 21, 8, 4), (8, 4, 8, 4), (1, 1, 8, 4)]  # ragged edges on both axes; one tile; one pixel
SHARDS = [(0, 1), (1, 3)]
SAMPLING = [(5, 2), (1, 32)]  # 3 batches, the last one short; one batch
QUEUES = [(SINGLE, 0), (XCD_TILES, 1), (XCD_TILES, 2), (XCD_TILES, 3), (XCD_REGIONS, 0)]
BLOCKS = [1, 3, 8, 11]
ORDERS = ["", "T", "M", "U", "TMU"]  # random tile_order, balanced tile_map, unit_order


def frame_cases():
    """Not the full product: with every frame order and with every queue mode, every value of every other axis."""
    out = []
    for ci, (fo, (qm, qc)) in enumerate(itertools.product([SEQUENTIAL, INTERLEAVED, PIXEL], QUEUES)):
        for i in range(5):
            j = i + ci
            (W, H, tw, th), (shard, shards), (spp, sps) = SHAPES[i % 3], SHARDS[j % 2], SAMPLING[(i + j // 2) % 2]
            out.append(SimpleNamespace(W=W, H=H, tw=tw, th=th, shard=shard, shards=shards, spp=spp, sps=sps,
                                       n_frames=1 + (i + ci // 5) % 3, frame_order=fo, unit_queues=qm, queue_chunk=qc,
                                       n_blocks=BLOCKS[j % 4], orders=ORDERS[i], seed=ci * 5 + i))
    return out


def run_case(c, any_every=0):
    from test_schedule import plan
    from rtpotato.scene import RenderParams
    rng = np.random.default_rng(c.seed)
    tiles = -(-c.W // c.tw) * -(-c.H // c.th)
    c.tile_map = rng.permutation(tiles) if "M" in c.orders else None
    g = geometry(c.W, c.H, c.tw, c.th, c.shard, c.shards, c.tile_map)
    c.tile_order = rng.permutation(g.n_shard_tiles) if "T" in c.orders else None
    c.unit_order = rng.permutation(g.n_shard_tiles * c.tw * c.th * -(-c.spp // c.sps)) if "U" in c.orders else None
    p = RenderParams(c.W, c.H, c.spp, 8, 3, tile_w=c.tw, tile_h=c.th, shard=c.shard, num_shards=c.shards,
                     samples_per_stream=c.sps)
    frames_inter = plan(p, c.n_frames, c.frame_order, c.unit_queues, c.queue_chunk)[1].frames_inter
    w = walk(c.W, c.H, c.tw, c.th, c.spp, c.sps, c.shard, c.shards, c.n_frames, c.frame_order, c.unit_queues,
             c.queue_chunk, c.tile_order, c.tile_map, c.unit_order, n_blocks=c.n_blocks, any_every=any_every)
    check_walk(w, c, g, frames_inter)
    return w


def test_frame_cases_cover_every_value():
    cs = frame_cases()
    for axis, values in [("frame_order", 3), ("n_frames", 3), ("n_blocks", 4), ("orders", 5), ("W", 3), ("shards", 2),
                         ("spp", 2)]:
        for fixed in ("frame_order", "unit_queues", "queue_chunk"):
            for v in {getattr(c, fixed) for c in cs}:
                if axis == fixed or fixed == "queue_chunk" and v == 0:
                    continue  # (SINGLE and XCD_REGIONS take no chunk: covered under unit_queues)
                assert len({getattr(c, axis) for c in cs if getattr(c, fixed) == v}) == values, (axis, fixed, v)


@pytest.mark.parametrize("i", range(75))
def test_every_unit_of_every_frame_once(i):
    run_case(frame_cases()[i])


@pytest.mark.parametrize("any_every", [1, 2, 3])
@pytest.mark.parametrize("i", range(0, 75, 5))  # the ragged frame of every frame order x queue mode
def test_wave_mate_finds_the_queue_drained(i, any_every):
    """A vote forced true -- a wave-mate found the queue drained, this lane took its last entry -- moves the lane's
    `tries` on although it holds a unit; where that unit is an edge tile's slot outside the frame the lane goes on to
    the next queue from there.  The same units come out, and the environment saw no queue index out of range (that
    would be an error of the walk: g = home + tries < 2 G, rp_units.h)."""
    c = frame_cases()[i]
    assert (c.W, c.H) == (37, 21)
    w = run_case(c, any_every)
    if any_every == 1:
        assert w.forced >= 1


def test_walk_refuses():
    from rtpotato import _ffi as F
    assert walk(37, 21, 8, 4, tile_order=[30] * 30, check=False).rc == F.RP_EINVAL      # an order entry out of range
    assert walk(37, 21, 8, 4, n_blocks=0, check=False).rc == F.RP_EINVAL
    assert walk(37, 21, 8, 4, groups=9, check=False).rc == F.RP_EINVAL
    assert walk(0, 21, 8, 4, check=False).rc == F.RP_EINVAL                             # the render's own refusal


# ---- the cost probe's lattice

@pytest.mark.parametrize("lattice", [1, 3, 16])
@pytest.mark.parametrize("shard,shards,n_blocks", [(0, 1, 1), (1, 3, 11)])
def test_probe_lattice(lattice, shard, shards, n_blocks):
    """Each (tile, lattice cell) once, batch 0, at the cell's centre clamped into the tile and the frame; the side is
    the lattice's, at most the tile's shorter side."""
    W, H, tw, th = 37, 21, 8, 4
    w = walk(W, H, tw, th, spp=5, sps=2, shard=shard, shards=shards, probe=lattice, n_blocks=n_blocks)
    g = geometry(W, H, tw, th, shard, shards)
    n = min(lattice, tw, th)
    u = w.units
    assert np.array_equal(np.sort(u[:, SLOT]), np.arange(g.n_shard_tiles * n * n))
    assert not u[:, BATCH].any() and not u[:, FRAME].any() and (u[:, SPP] == 1).all()
    t = shard + (u[:, SLOT] // (n * n)) * shards
    cx, cy = u[:, SLOT] % n, u[:, SLOT] % (n * n) // n
    centre_x = np.minimum(cx * tw // n + tw // (2 * n), tw - 1)
    centre_y = np.minimum(cy * th // n + th // (2 * n), th - 1)
    assert np.array_equal(u[:, PI], np.minimum((t % g.tiles_x) * tw + centre_x, W - 1))
    assert np.array_equal(u[:, PJ], np.minimum((t // g.tiles_x) * th + centre_y, H - 1))
    # the probe's own queue word, and no other
    assert w.entries[QUEUE_PROBE] == len(u) == w.entries.sum()
    assert w.words[QUEUE_PROBE] == len(u) + n_blocks == w.words.sum()
