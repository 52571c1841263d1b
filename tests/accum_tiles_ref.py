"""Numpy models of tile-adaptive progressive rendering, written from the definitions (include/rp.h
rp_accum_tiles_select_device, rp_accum_frames_tiles_device and DeviceScene.render_adaptive's loop) and
not from the C sources: the tile selection, the fold of a tile-list launch into whole-frame state, and the whole loop
replayed on the host from frames rendered once.  The arithmetic is accum_ref's (every IEEE operation in the definition's
order), so the models, the host library and the device agree to the last bit.  Also the frames the CPU and GPU tests
share.
"""
from __future__ import annotations

import numpy as np

import accum_ref as A


def grid(W: int, H: int, tw: int, th: int):
    """(tiles_x, tiles_y, tile_px, inside): inside[t] the row-major in-frame mask of frame tile t's tw * th slots."""
    tiles_x, tiles_y = -(-W // tw), -(-H // th)
    lj, li = np.divmod(np.arange(tw * th), tw)
    inside = np.zeros((tiles_x * tiles_y, tw * th), dtype=bool)
    for t in range(tiles_x * tiles_y):
        inside[t] = ((t % tiles_x) * tw + li < W) & ((t // tiles_x) * th + lj < H)
    return tiles_x, tiles_y, tw * th, inside


def to_compact(frame, tw: int, th: int, fill=0.0) -> np.ndarray:
    """A frame (H, W, C) as the compact buffer of the whole frame on one shard: tile t at slot t * tw * th, row-major
    inside the tile; slots outside the frame hold `fill`.  -> (tiles * tw * th, C)."""
    frame = np.asarray(frame, dtype=np.float64)
    H, W, C = frame.shape
    tiles_x, tiles_y, tile_px, _ = grid(W, H, tw, th)
    pad = np.full((tiles_y * th, tiles_x * tw, C), fill)
    pad[:H, :W] = frame
    return pad.reshape(tiles_y, th, tiles_x, tw, C).transpose(0, 2, 1, 3, 4).reshape(-1, C)


def from_compact(buf, W: int, H: int, tw: int, th: int) -> np.ndarray:
    """to_compact's inverse: (H, W, C) from (tiles * tw * th, C)."""
    buf = np.asarray(buf)
    tiles_x, tiles_y, _, _ = grid(W, H, tw, th)
    C = buf.shape[-1]
    return buf.reshape(tiles_y, tiles_x, th, tw, C).transpose(0, 2, 1, 3, 4).reshape(tiles_y * th, tiles_x * tw, C)[:H, :W]


def pixel_over(mean, var, tol: float = 0.05, eps: float = 1e-4) -> np.ndarray:
    """Per slot (..., 3): e2 > tol * tol with e2 = ((v.r + v.g) + v.b) / (((m.r m.r + m.g m.g) + m.b m.b) + eps): NaN
    is never over, +inf is."""
    m = np.asarray(mean, dtype=np.float64).reshape(-1, 3)
    v = np.asarray(var, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        s = (v[:, 0] + v[:, 1]) + v[:, 2]
        q = ((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]) + np.float64(eps)
        return (s / q) > np.float64(tol) * np.float64(tol)


def select(mean, var, W: int, H: int, tw: int, th: int, tiles_in=None, n_in=None, tol: float = 0.05, eps: float = 1e-4,
           tile_share: float = 0.0):
    """-> (the active tiles in list order, every listed entry's over count), uint32.  mean, var: compact buffers."""
    _, _, tile_px, inside = grid(W, H, tw, th)
    n_tiles = len(inside)
    if n_in is None:
        n_in = n_tiles if tiles_in is None else len(tiles_in)
    listed = np.arange(n_in) if tiles_in is None else np.asarray(tiles_in, dtype=np.int64)[:n_in]
    over_px = pixel_over(mean, var, tol, eps).reshape(n_tiles, tile_px) & inside
    over, active = np.zeros(n_in, dtype=np.uint32), []
    for k, t in enumerate(listed):
        if t >= n_tiles:
            continue  # over 0, never active
        over[k] = int(over_px[t].sum())
        if np.float64(over[k]) > np.float64(tile_share) * np.float64(inside[t].sum()):
            active.append(t)
    return np.array(active, dtype=np.uint32), over


def fold_tiles(frames, n_frames: int, tiles, tile_words: int, stride: int, mean, m2, var, n_prior: int,
               n_state_tiles: int):
    """Listed block k (word w of frame f at f * stride + k * tile_words + w of the flat `frames`) folded in frame order
    into block tiles[k] of copies of the state; var (or None) written for the listed blocks, n = n_prior + n_frames.
    An entry >= n_state_tiles is skipped.  -> (mean, m2, var)."""
    frames = np.asarray(frames, dtype=np.float64).reshape(-1)
    mean, m2 = np.array(mean, dtype=np.float64), np.array(m2, dtype=np.float64)
    var = None if var is None else np.array(var, dtype=np.float64)
    for k, t in enumerate(np.asarray(tiles, dtype=np.int64)):
        if t >= n_state_tiles:
            continue
        at = slice(t * tile_words, (t + 1) * tile_words)
        mk, qk, vk = A.accum_frames(frames[k * tile_words:], n_frames, tile_words, stride, mean[at], m2[at], n_prior)
        mean[at], m2[at] = mk, qk
        if var is not None:
            var[at] = vk
    return mean, m2, var


def replay_adaptive(frames, W: int, H: int, tw: int, th: int, frames_per_launch: int, max_frames: int,
                    max_launch_frames: int, tol: float, share: float, tile_share: float, eps: float = 1e-4) -> dict:
    """DeviceScene.render_adaptive's loop on the host.  frames: (>= max_frames, tiles * tw * th * 3), frame f the compact
    whole frame of seed + f * W * H.  -> {"mean", "variance": (H, W, 3), "tile_frames": (tiles_y, tiles_x) int32,
    "log": per launch (frames before it, its tiles, its frames, pixels, over, largest finite e2, non-finite)}."""
    from rtpotato.render import error_stats
    frames = np.asarray(frames, dtype=np.float64)
    tiles_x, tiles_y, tile_px, inside = grid(W, H, tw, th)
    T, tile_words = tiles_x * tiles_y, 3 * tile_px
    k = min(frames_per_launch, max_frames)
    mean, m2, var = A.accum_frames(frames[:k].reshape(-1), k, T * tile_words, T * tile_words)
    listed, done, log = np.arange(T), 0, []
    tile_frames = np.zeros(T, dtype=np.int32)
    while True:
        st = error_stats(A.accum_error(mean.reshape(-1, 3)[inside.reshape(-1)], var.reshape(-1, 3)[inside.reshape(-1)],
                                       tol, eps))
        nxt, _ = select(mean, var, W, H, tw, th, listed, tol=tol, eps=eps, tile_share=tile_share)
        tile_frames[listed] += k
        log.append((done, len(listed), k) + st)
        done += k
        if len(nxt) == 0 or st[1] <= share * st[0] or done == max_frames:
            break
        listed = nxt.astype(np.int64)
        k = min(max_launch_frames, max_frames - done, frames_per_launch * (T // len(listed)))
        # the launch's frames: the listed tiles of frames done .. done + k - 1, listed tile j at block j
        launch = frames[done:done + k].reshape(k, T, tile_words)[:, listed].reshape(k, -1)
        mean, m2, var = fold_tiles(launch, k, listed, tile_words, launch.shape[1], mean, m2, var, done, T)
    return {"mean": from_compact(mean.reshape(-1, 3), W, H, tw, th), "variance": from_compact(var.reshape(-1, 3), W, H, tw, th),
            "tile_frames": tile_frames.reshape(tiles_y, tiles_x), "log": log, "mean_compact": mean, "var_compact": var}


def synthetic_blocks(n_frames: int, n_listed: int, tile_words: int, stride: int, seed: int) -> np.ndarray:
    """accum_ref.synthetic's frames for n_listed blocks of tile_words words (an empty list: padding alone)."""
    if n_listed == 0:
        return np.full(max(1, n_frames * stride), A.PAD)
    return A.synthetic(n_frames, n_listed * tile_words, stride, seed)


def synthetic_state(W: int, H: int, tw: int, th: int, seed: int, outside=(np.nan, 1e300)):
    """(mean, var) compact buffers (slots, 3) of accum_ref.synthetic_error_frames' pixels, with the slots outside the
    frame filled with outside[0] (mean) and outside[1] (variance): they must never count."""
    _, _, _, inside = grid(W, H, tw, th)
    m, v = A.synthetic_error_frames(inside.size, seed)
    m[~inside.reshape(-1)] = outside[0]
    v[~inside.reshape(-1)] = outside[1]
    return np.ascontiguousarray(m), np.ascontiguousarray(v)
