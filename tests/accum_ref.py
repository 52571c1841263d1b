"""Numpy models of progressive accumulation, written from the definitions (include/rp.h rp_accum_frames_device and
rp_accum_error_device_ws) and not from csrc/rp_accum.h: every word at once, one frame after the other,
each IEEE binary64 operation in the definition's order (numpy's elementwise + - * / round once each and never fuse), so
the models, the host library and the device agree to the last bit.  Also the seeded synthetic frames the CPU and GPU
tests share.
"""
from __future__ import annotations

import numpy as np

PAD = -12345.0  # what lies between the frames of a strided buffer: never read


def accum_frames(frames, n_frames: int, n_words: int, stride: int, mean=None, m2=None, n_prior: int = 0):
    """Frames f = 0 .. n_frames - 1 (frame f's words at f * stride of the flat `frames`) folded in order into the state
    (mean, m2) of n_prior frames (None with n_prior = 0): (mean, m2, var), var None while n_prior + n_frames < 2."""
    frames = np.asarray(frames, dtype=np.float64).reshape(-1)
    if n_prior == 0:
        mean, m2 = np.zeros(n_words), np.zeros(n_words)
    else:
        mean, m2 = np.array(mean, dtype=np.float64), np.array(m2, dtype=np.float64)
    with np.errstate(all="ignore"):
        for f in range(n_frames):
            k = n_prior + f + 1
            r = np.float64(1.0) / np.float64(k)
            x = frames[f * stride:f * stride + n_words]
            d = x - mean
            mean = mean + d * r
            m2 = m2 + d * (x - mean)
        n = n_prior + n_frames
        var = m2 / (np.float64(n) * np.float64(n - 1)) if n >= 2 else None
    return mean, m2, var


def accum_error(mean, var, tol: float = 0.05, eps: float = 1e-4) -> np.ndarray:
    """The four statistics of full frames mean and var (..., 3): uint64 {pixels, pixels with e2 > tol * tol, the bit
    pattern of the largest finite positive e2 (0: none), pixels whose e2 is not finite}."""
    m = np.asarray(mean, dtype=np.float64).reshape(-1, 3)
    v = np.asarray(var, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        s = (v[:, 0] + v[:, 1]) + v[:, 2]
        q = ((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]) + np.float64(eps)
        e2 = s / q
        over = e2 > np.float64(tol) * np.float64(tol)
        fin = np.isfinite(e2)
        pos = fin & (e2 > 0.0)
    bits = int(np.ascontiguousarray(e2[pos]).view(np.uint64).max()) if pos.any() else 0
    return np.array([len(e2), int(over.sum()), bits, int((~fin).sum())], dtype=np.uint64)


def same_bits(a, b) -> bool:
    """Equal bit for bit, NaN matching NaN whatever its payload (an invalid operation's NaN differs between CPU and
    GPU in its sign bit): stricter than np.array_equal, which takes -0.0 for 0.0."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


def synthetic(n_frames: int, n_words: int, stride: int, seed: int) -> np.ndarray:
    """n_frames frames of n_words words at `stride` in one flat array, the gaps at PAD: values in (0, 3) with, as far
    as there is room, word 0 the same in every frame (m2 == 0 exactly), and from 8 words on a tenth zeros, a tenth
    denormals, word 5 with one +inf (frame 0) and word 6 with one NaN (the last frame)."""
    r = np.random.default_rng(seed)
    buf = np.full(n_frames * stride, PAD)
    fr = buf.reshape(n_frames, stride)[:, :n_words]
    fr[:] = r.uniform(0.0, 3.0, size=(n_frames, n_words))
    if n_words >= 8:
        u = r.uniform(size=(n_frames, n_words))
        fr[u < 0.1] = 0.0
        den = (u >= 0.1) & (u < 0.2)
        fr[den] = r.integers(1, 1 << 40, size=int(den.sum())) * 5e-324
        fr[0, 5] = np.inf
        fr[n_frames - 1, 6] = np.nan
    fr[:, 0] = 0.7
    return buf


def synthetic_error_frames(n_pixels: int, seed: int):
    """(mean, var) (n_pixels, 3): means in (0, 2) with a fifth of the pixels dark (~1e-3), variances of relative size
    0 .. 0.1 with a tenth exactly zero, and one pixel each with a NaN mean, an infinite variance, a NaN variance and a
    negative variance."""
    r = np.random.default_rng(seed)
    mean = r.uniform(0.0, 2.0, size=(n_pixels, 3))
    mean[r.uniform(size=n_pixels) < 0.2] *= 1e-3
    var = (mean * r.uniform(0.0, 0.1, size=(n_pixels, 3))) ** 2
    var[r.uniform(size=n_pixels) < 0.1] = 0.0
    if n_pixels >= 8:
        mean[1, 0] = np.nan
        var[2, 1] = np.inf
        var[3, 2] = np.nan
        var[4] = -1e-3
    return mean, var
