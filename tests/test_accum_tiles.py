"""Tile-adaptive progressive rendering on the CPU: the host models rph_accum_tiles_select and
rph_accum_frames_tiles (plain loops over csrc/rp_accum.h, the header the kernels compile) against the numpy models of
tests/accum_tiles_ref.py -- values bit for bit, counts and lists exact --, the launch arithmetic of a tile-list launch
(csrc/rp_schedule.h plan_tiles_launch) against rps::plan_launch, and the render kernel's own unit fetch (csrc/rp_units.h) walked on the
CPU with a foreign tile list as its tile map: every (listed tile, in-frame pixel, frame) exactly once, at the slot
rp_render_tiles_device_ws's layout gives it, and nothing else."""
import ctypes

import numpy as np
import pytest

import accum_ref as A
import accum_tiles_ref as T

W, H, TW, TH = 80, 48, 32, 32  # 3 x 2 tiles, edge tiles in both directions: 16 columns and 16 rows outside the frame
SEED = 20260219
SLOT, PI, PJ, BATCH, BLOCK, QUEUE, FRAME, SPP = range(8)
SEQUENTIAL, INTERLEAVED, PIXEL = 1, 2, 3


def _params(w=W, h=H, tw=TW, th=TH, spp=4, **kw):
    from rtpotato.scene import RenderParams
    return RenderParams(w, h, spp, 8, 1, tw, th, samples_per_stream=spp, **kw)


def _select(params, mean, var, **kw):
    from rtpotato.render import accum_tiles_select_host
    return accum_tiles_select_host(params, mean, var, **kw)


# ---- select

@pytest.mark.parametrize("tile_share", [0.0, 0.01, 0.3, 0.9])
def test_select_equals_numpy_model(tile_share):
    """Identity, shuffled and partial lists with an out-of-range entry; the slots outside the frame hold NaN means and
    1e300 variances (over, were they counted) and must never count."""
    mean, var = T.synthetic_state(W, H, TW, TH, SEED)
    r = np.random.default_rng(SEED)
    lists = [None, np.arange(6), r.permutation(6), np.array([5, 0, 3]), np.array([4, 6, 1, 0xFFFFFFFF, 2]), np.array([], int)]
    for tol in (0.05, 0.02):
        for tiles in lists:
            got = _select(_params(), mean, var, tiles_in=tiles, tol=tol, tile_share=tile_share)
            ref = T.select(mean, var, W, H, TW, TH, tiles, tol=tol, tile_share=tile_share)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (tol, tiles)
    # the counts are the in-frame pixels' alone: the same state with benign slots outside gives the same answer
    clean = T.synthetic_state(W, H, TW, TH, SEED, outside=(1.0, 0.0))
    a, b = _select(_params(), mean, var, tile_share=tile_share), _select(_params(), *clean, tile_share=tile_share)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].sum() > 0
    # an out-of-range entry: over 0, never selected
    got = _select(_params(), mean, var, tiles_in=np.array([6, 7, 1 << 31]), tile_share=0.0)
    assert len(got[0]) == 0 and not got[1].any()


def test_select_threshold_is_strict():
    """over == tile_share * px exactly is not active, one more pixel over is: tile 2 (16 x 32 = 512 in-frame pixels) and
    tile 5 (16 x 16 = 256) at tile_share = 1 / 8."""
    _, _, tile_px, inside = T.grid(W, H, TW, TH)
    mean = np.ones((6 * tile_px, 3))
    var = np.zeros((6 * tile_px, 3))
    var[~inside.reshape(-1)] = 1e300
    for tile, px in ((2, 512), (5, 256)):
        slots = tile * tile_px + np.flatnonzero(inside[tile])
        assert len(slots) == px
        var[slots[:px // 8]] = 1.0
        tiles, over = _select(_params(), mean, var, tile_share=0.125)
        assert over[tile] == px // 8 and tile not in tiles
        var[slots[px // 8]] = np.inf  # +inf is over
        tiles, over = _select(_params(), mean, var, tile_share=0.125)
        assert over[tile] == px // 8 + 1 and tile in tiles
        var[slots[px // 8]] = np.nan  # NaN never is
        tiles, over = _select(_params(), mean, var, tile_share=0.125)
        assert over[tile] == px // 8 and tile not in tiles
        var[slots] = 0.0


def test_select_16384_tiles_and_refusals():
    """A 128 x 128 frame in 1 x 1 tiles: the limit's 16384 tiles; one more is refused, as is every bad argument."""
    from rtpotato._ffi import RPError
    p = _params(128, 128, 1, 1)
    mean, var = T.synthetic_state(128, 128, 1, 1, SEED + 1)
    r = np.random.default_rng(SEED + 1)
    for tiles in (None, r.permutation(16384)):
        got = _select(p, mean, var, tiles_in=tiles, tile_share=0.0)
        ref = T.select(mean, var, 128, 128, 1, 1, tiles, tile_share=0.0)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and 0 < len(ref[0]) < 16384
    big = _params(129, 127, 1, 1)
    m2, v2 = T.synthetic_state(129, 127, 1, 1, SEED + 2)
    assert len(_select(big, m2, v2, n_in=16384)[1]) == 16384
    for kw, msg in ((dict(n_in=16385), "16384"), (dict(tile_share=1.0), "tile_share"), (dict(tile_share=-0.1), "tile_share"),
                    (dict(tile_share=float("nan")), "tile_share"), (dict(tol=-1.0), "error params")):
        with pytest.raises(RPError, match=msg):
            _select(big, m2, v2, **kw)
    for bad in (_params(num_shards=2), _params(shard_map=1)):
        with pytest.raises(RPError, match="whole frame"):
            _select(bad, np.zeros((6 * 1024, 3)), np.zeros((6 * 1024, 3)))


# ---- the tile fold

def _host_tile_fold(frames, n_frames, tiles, tile_words, stride, n_state, state=None, n_prior=0, want_var=True):
    from rtpotato.render import accum_frames_tiles_host
    n = n_state * tile_words
    bufs = [np.full(n + 2, A.PAD) for _ in range(3)]  # two guard words behind every buffer
    if state is not None:
        for b, s in zip(bufs, state):
            if s is not None:
                b[:n] = s
    accum_frames_tiles_host(np.ascontiguousarray(frames), n_frames, tiles, len(tiles), tile_words, bufs[0][:n], bufs[1][:n],
                            n_prior=n_prior, var=bufs[2][:n] if want_var else None, stride=stride, n_state_tiles=n_state)
    assert all((b[n:] == A.PAD).all() for b in bufs), "wrote behind a buffer"
    return bufs[0][:n], bufs[1][:n], bufs[2][:n] if want_var else None


@pytest.mark.parametrize("tile_words", [3, 6, 3 * 32 * 32])
def test_tile_fold_equals_numpy_model(tile_words):
    """Lists of 0, 1 and all blocks, shuffled, with an out-of-range entry, at stride = n_listed * tile_words and 5 more,
    with and without prior frames: the listed blocks bit for bit, every other word of the state untouched."""
    n_state = 6
    r = np.random.default_rng(SEED + tile_words)
    prior = A.synthetic(2, n_state * tile_words, n_state * tile_words, SEED + 3)
    state = A.accum_frames(prior, 2, n_state * tile_words, n_state * tile_words)
    for tiles in ([], [4], list(r.permutation(n_state)), [5, 0, 3], [2, 6, 1]):
        tiles = np.array(tiles, dtype=np.uint32)
        for pad in (0, 5):
            for n_frames in (1, 3, 5):
                stride = len(tiles) * tile_words + pad
                frames = T.synthetic_blocks(n_frames, len(tiles), tile_words, stride, SEED + 7 * n_frames + len(tiles))
                for n_prior, st in ((0, (np.full_like(state[0], 7.0), np.full_like(state[0], 8.0), np.full_like(state[0], 9.0))),
                                    (2, state)):
                    want_var = n_prior + n_frames >= 2
                    got = _host_tile_fold(frames, n_frames, tiles, tile_words, stride, n_state, st, n_prior, want_var)
                    ref = T.fold_tiles(frames, n_frames, tiles, tile_words, stride, st[0], st[1], st[2] if want_var else None,
                                       n_prior, n_state)
                    assert all((g is None and x is None) or A.same_bits(g, x) for g, x in zip(got, ref)), (tiles, pad, n_frames)
                    untouched = np.ones(n_state, bool)
                    untouched[tiles[tiles < n_state]] = False
                    keep = np.repeat(untouched, tile_words)
                    assert A.same_bits(got[0][keep], st[0][keep]) and A.same_bits(got[1][keep], st[1][keep])


@pytest.mark.parametrize("tile_words", [3, 6])
def test_tile_fold_over_identity_is_the_plain_fold(tile_words):
    from rtpotato.render import accum_frames_host
    n_state = 7
    n = n_state * tile_words
    frames = A.synthetic(5, n, n + 1, SEED + 11)
    mean, m2, var = (np.full(n, A.PAD) for _ in range(3))
    accum_frames_host(frames, 5, mean, m2, var=var, n_words=n, stride=n + 1)
    got = _host_tile_fold(frames, 5, np.arange(n_state, dtype=np.uint32), tile_words, n + 1, n_state)
    assert A.same_bits(got[0], mean) and A.same_bits(got[1], m2) and A.same_bits(got[2], var)
    # continuation: two frames, then three with n_prior = 2
    part = _host_tile_fold(frames, 2, np.arange(n_state, dtype=np.uint32), tile_words, n + 1, n_state, want_var=False)
    part = _host_tile_fold(frames[2 * (n + 1):], 3, np.arange(n_state, dtype=np.uint32), tile_words, n + 1, n_state,
                           (part[0], part[1], None), n_prior=2)
    assert A.same_bits(part[0], mean) and A.same_bits(part[1], m2) and A.same_bits(part[2], var)


def test_tile_fold_refusals():
    from rtpotato import _ffi as F
    L = F.host()
    fr = np.ones(64)
    out = np.full((3, 16), A.PAD)
    tiles = np.array([1, 0], dtype=np.uint32)
    ptr = lambda a, off=0: None if a is None else a.ctypes.data + 8 * off

    def call(tile_words=4, n_state=4, tl=tiles.ctypes.data, n_listed=2, n_prior=0, n_frames=3, frames=ptr(fr), stride=8,
             mean=ptr(out[0]), m2=ptr(out[1]), var=ptr(out[2])):
        return L.rph_accum_frames_tiles(tile_words, n_state, tl, n_listed, n_prior, n_frames, frames, stride, mean, m2, var)

    assert call() == F.RP_OK
    for kw, msg in ((dict(frames=None), "non-NULL"), (dict(mean=None), "non-NULL"), (dict(m2=None), "non-NULL"),
                    (dict(tile_words=0), "tile_words is zero"), (dict(n_frames=0), "n_frames is zero"),
                    (dict(n_listed=5), "above n_state_tiles"), (dict(tl=None), "tiles must be non-NULL"),
                    (dict(stride=7), "frame_stride is below"), (dict(n_prior=0x7fffffff), "2^31 - 1"),
                    (dict(n_frames=1), "at least two frames"), (dict(tile_words=1 << 40), "2^40 - 512"),
                    (dict(n_state=1 << 31, tile_words=1 << 10, n_listed=1), "2^40 - 512"),
                    (dict(mean=ptr(fr, 8)), "alias the frames"), (dict(m2=ptr(out[0], 4)), "alias one another"),
                    (dict(var=ptr(out[1])), "alias one another")):
        assert call(**kw) == F.RP_EINVAL, kw
        assert msg in L.rph_last_error().decode(), (kw, L.rph_last_error())
    assert (out[:, :] != A.PAD).sum() == 3 * 8  # only the accepted call wrote, and only its two blocks
    assert call(n_listed=0, tl=None, stride=0) == F.RP_OK  # nothing listed: nothing to do


# ---- the launch arithmetic and the unit fetch over a foreign list

def _plan(fn, *args):
    from rtpotato import _ffi as F
    out = F.rph_launch_plan()
    rc = fn(*args, ctypes.byref(out))
    return rc, out


@pytest.mark.parametrize("shape", [(80, 48, 32, 32), (1920, 1080, 32, 32), (640, 360, 8, 8), (33, 7, 4, 4)])
def test_plan_over_the_full_list_is_plan_launch(shape):
    """rp_tiles_plan.h restates plan_launch's queue-chunk rule for n_listed tiles: over the full list every field it
    reports equals the whole frame's plan, for every frame order, queue mode and chunk."""
    from rtpotato import _ffi as F
    w, h, tw, th = shape
    n_tiles = -(-w // tw) * -(-h // th)
    same = [f for f, _ in F.rph_launch_plan._fields_ if f not in ("plan_block", "gather_stride", "block_words", "sortable", "measure")]
    for n_frames in (1, 3, 8, 16):
        for order in (0, SEQUENTIAL, INTERLEAVED, PIXEL):
            for queues, chunk in ((0, 0), (1, 0), (2, 0), (2, 3), (3, 0)):
                rc0, a = _plan(F.host().rph_plan_launch, w, h, 4, 8, tw, th, 0, 1, 4, 0, n_frames, order, queues, chunk, 65536)
                rc1, b = _plan(F.host().rph_plan_tiles_launch, w, h, 4, 8, tw, th, 4, n_tiles, n_frames, order, queues, chunk, 65536)
                assert rc0 == rc1 == F.RP_OK
                for f in same:
                    va, vb = getattr(a, f), getattr(b, f)
                    assert (list(va) == list(vb)) if hasattr(va, "__len__") else va == vb, (f, n_frames, order, queues, chunk)
                assert b.sortable == 0 and b.measure == 0


def test_plan_of_a_short_list_and_refusals():
    from rtpotato import _ffi as F
    P = F.host().rph_plan_tiles_launch
    rc, p = _plan(P, W, H, 4, 8, TW, TH, 4, 3, 5, INTERLEAVED, 0, 0, 65536)
    assert rc == F.RP_OK and p.n_shard_tiles == 3 and p.n_slots == 3 * 1024 and p.n_queue == 5 * 3 * 1024
    assert p.out_stride == 3 * 3 * 1024 and p.nbatch == 1 and p.queue_chunk % 5 == 0 and p.frames_inter == 1
    assert p.grid == min(-(-p.n_queue // 64), 65536 // 64)
    for args, msg in (((W, H, 4, 8, TW, TH, 2, 3, 1, 0, 0, 0, 65536), "one stream per pixel"),
                      ((W, H, 0, 8, TW, TH, 4, 3, 1, 0, 0, 0, 65536), "spp >= 1"),
                      ((W, H, 4, 8, TW, TH, 4, 7, 1, 0, 0, 0, 65536), "above the frame's tile count"),
                      ((W, H, 4, 8, TW, TH, 4, 3, 0, 0, 0, 0, 65536), "n_frames"),
                      ((W, H, 4, 8, TW, TH, 4, 3, 65, 0, 0, 0, 65536), "n_frames"),
                      ((W, H, 4, 8, TW, TH, 4, 3, 1, 4, 0, 0, 65536), "frame_order"),
                      ((W, H, 4, 0, TW, TH, 4, 3, 1, 0, 0, 0, 65536), "max_bounce")):
        rc, _ = _plan(P, *args)
        assert rc == F.RP_EINVAL and msg in F.host().rph_last_error().decode(), (args, F.host().rph_last_error())
    rc, p = _plan(P, W, H, 4, 8, TW, TH, 4, 0, 1, 0, 0, 0, 65536)  # an empty list plans an empty launch
    assert rc == F.RP_OK and p.n_queue == 0 and p.n_slots == 0


def _walk(tiles, n_frames, order, queues=0, chunk=0, n_blocks=5, w=W, h=H, tw=TW, th=TH):
    from rtpotato import _ffi as F
    tiles = np.ascontiguousarray(tiles, dtype=np.uint32)
    cap = len(tiles) * tw * th * n_frames + 1
    units = np.zeros((cap, 8), np.uint32)
    words, entries = np.zeros(288, np.uint32), np.zeros(288, np.uint32)
    n = ctypes.c_uint64()
    rc = F.host().rph_tiles_unit_walk(w, h, 4, 8, tw, th, 4, n_frames, order, queues, chunk,
                                      tiles.ctypes.data if len(tiles) else None, len(tiles), n_blocks, units.ctypes.data,
                                      cap, ctypes.byref(n), words.ctypes.data, entries.ctypes.data)
    return rc, units[:n.value].astype(np.int64)


@pytest.mark.parametrize("tiles", [[5, 0, 3], [0, 1, 2, 3, 4, 5], [3], [4, 6, 1, 77, 2]])
@pytest.mark.parametrize("n_frames", [1, 3])
def test_unit_walk_serves_the_list(tiles, n_frames):
    """The kernel's unchanged fetch with the list as its tile map: every (listed tile, in-frame pixel, frame) exactly
    once, at slot k * tw * th + the row-major offset in the tile, frame f in the unit's batch; nothing else -- no slot
    outside the frame and none of an entry at or above the frame's 6 tiles."""
    from rtpotato import _ffi as F
    tiles_x, _, tile_px, inside = T.grid(W, H, TW, TH)
    want = set()
    for k, t in enumerate(tiles):
        if t >= len(inside):
            continue
        for local in np.flatnonzero(inside[t]):
            pi, pj = (t % tiles_x) * TW + local % TW, (t // tiles_x) * TH + local // TW
            want |= {(k * tile_px + int(local), int(pi), int(pj), f) for f in range(n_frames)}
    for order in (0, SEQUENTIAL, INTERLEAVED, PIXEL):
        for queues, chunk, n_blocks in ((0, 0, 5), (1, 0, 1), (2, 1, 8), (2, 3, 11), (3, 0, 8)):
            rc, u = _walk(tiles, n_frames, order, queues, chunk, n_blocks)
            assert rc == F.RP_OK, F.host().rph_last_error()
            got = list(zip(u[:, SLOT].tolist(), u[:, PI].tolist(), u[:, PJ].tolist(), u[:, BATCH].tolist()))
            assert len(got) == len(set(got)) == len(want) and set(got) == want, (order, queues, chunk)
            assert (u[:, FRAME] == u[:, BATCH]).all() and (u[:, SPP] == 4).all()


def test_unit_walk_empty_and_huge_entries():
    from rtpotato import _ffi as F
    rc, u = _walk([], 2, 0)
    assert rc == F.RP_OK and len(u) == 0
    rc, u = _walk([1 << 31], 1, 0)  # beyond the fetch's division: the walk's environment reports it
    assert rc == F.RP_EINVAL and "numerator" in F.host().rph_last_error().decode()


def test_replay_model_is_the_plain_mean_per_tile():
    """The loop's defining property, on synthetic frames: every tile's result is the plain progressive fold of its own
    first n_t frames, and tiles stop at different counts."""
    r = np.random.default_rng(SEED + 5)
    _, _, tile_px, inside = T.grid(W, H, TW, TH)
    noise = np.repeat(np.array([0.01, 0.3, 0.01, 0.08, 0.3, 0.01]), tile_px)  # per-tile relative noise
    frames = 1.0 + noise[None, :, None] * r.standard_normal((12, 6 * tile_px, 3))
    out = T.replay_adaptive(frames.reshape(12, -1), W, H, TW, TH, 4, 12, 4, 0.05, 0.0, 0.05)
    nt = out["tile_frames"].reshape(-1)
    assert nt.min() == 4 and nt.max() == 12 and len(set(nt.tolist())) >= 2, nt
    assert [e[:3] for e in out["log"]] == [(0, 6, 4)] + [(4 * i, int((nt > 4 * i).sum()), 4) for i in (1, 2) if (nt > 4 * i).any()]
    for t in range(6):
        at = slice(t * 3 * tile_px, (t + 1) * 3 * tile_px)
        mean, _, var = A.accum_frames(frames.reshape(12, -1)[:, at].reshape(-1), int(nt[t]), 3 * tile_px, 3 * tile_px)
        assert A.same_bits(out["mean_compact"][at], mean) and A.same_bits(out["var_compact"][at], var)
