"""Numpy models of the per-pixel variance pass and the variance-guided denoiser, written from their definitions
(include/rp.h rp_render_variance_device_ws and rp_denoise_var) and not from csrc/rp_variance.h or
csrc/rp_denoise.h: every pixel at once, one batch or one tap after the other, each IEEE binary64 operation in the
definition's order (numpy's elementwise + - * / round once each and never fuse), so the models, the host library and the
device agree to the last bit.  Also the seeded frames and the oracle-built quality cases the CPU and GPU tests share.
"""
from __future__ import annotations

from dataclasses import replace

import numpy as np

import denoise_ref as R
from denoise_ref import K, _len2, _rat, _sum3

DEFAULTS = dict(R.DEFAULTS, sigma_var=3.0, var_eps=1e-6)
KG = (1.0 / 2.0, 1.0 / 4.0)


def batch_variance(sums, spp: int, sps: int) -> np.ndarray:
    """sums (..., B, 3), B = ceil(spp / sps) >= 2: the variance of the pixel's mean, (..., 3)."""
    sums = np.asarray(sums, dtype=np.float64)
    B = (spp + sps - 1) // sps
    assert B >= 2 and sums.shape[-2] == B
    n = float(spp)
    x = np.zeros(sums.shape[:-2] + (3,))
    for b in range(B):
        x = x + sums[..., b, :]
    x = x / n
    acc = np.zeros_like(x)
    for b in range(B):
        nb = min(sps, spp - b * sps)
        e = sums[..., b, :] / n - x * (float(nb) / n)
        acc = acc + e * e
    return acc * (float(B) / float(B - 1))


def denoise_var(rgb, var, normal=None, albedo=None, depth=None, **params) -> np.ndarray:
    """The variance-guided filter on (h, w, 3) rgb and var with optional guides normal, albedo (h, w, 3) and depth
    (h, w); params as rp_denoise_var_params' fields, the base's beside sigma_var and var_eps (a zero or missing one
    takes its default; sigma_color is ignored)."""
    P = dict(DEFAULTS)
    P.update({k: v for k, v in params.items() if v != 0})
    L, en = int(P["iterations"]), int(P["normal_power"])
    sz, sa, eps, sv, veps = (float(P[k]) for k in ("sigma_depth", "sigma_albedo", "albedo_eps", "sigma_var", "var_eps"))
    rgb = np.asarray(rgb, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    H, W = rgb.shape[:2]
    with np.errstate(all="ignore"):
        nn = _len2(normal) if normal is not None else None
        keep = (nn == 0.0) if nn is not None else np.zeros((H, W), dtype=bool)
        if albedo is not None:
            c = rgb / (albedo + eps)
            dv = var / ((albedo + eps) * (albedo + eps))
        else:
            c = rgb.copy()
            dv = var
        v = _sum3(dv[..., 0], dv[..., 1], dv[..., 2])
        for lvl in range(L):
            s = 1 << lvl

            def taps(r):
                for dy in range(-r, r + 1):
                    for dx in range(-r, r + 1):
                        # pixels p whose tap q = p + s (dx, dy) lies inside the frame
                        j0, j1 = max(0, -s * dy), min(H, H - s * dy)
                        i0, i1 = max(0, -s * dx), min(W, W - s * dx)
                        if j0 < j1 and i0 < i1:
                            yield (dx, dy, (slice(j0, j1), slice(i0, i1)),
                                   (slice(j0 + s * dy, j1 + s * dy), slice(i0 + s * dx, i1 + s * dx)))

            # the prefilter of v: 3 x 3 taps at the level's step, pass-through pixels do not count
            g = np.zeros((H, W))
            gw = np.zeros((H, W))
            for dx, dy, p, q in taps(1):
                k = KG[abs(dx)] * KG[abs(dy)]
                counts = nn[q] > 0.0 if nn is not None else np.ones(v[q].shape, dtype=bool)
                g[p] = np.where(counts, g[p] + k * v[q], g[p])
                gw[p] = np.where(counts, gw[p] + k, gw[p])
            vf = g / gw
            sw = np.zeros((H, W))
            acc = np.zeros((H, W, 3))
            vacc = np.zeros((H, W))
            for dx, dy, p, q in taps(2):
                w = np.full(sw[p].shape, K[abs(dx)] * K[abs(dy)])
                if normal is not None and (dx or dy):
                    d = _sum3(normal[p][..., 0] * normal[q][..., 0], normal[p][..., 1] * normal[q][..., 1],
                              normal[p][..., 2] * normal[q][..., 2])
                    ab = nn[p] * nn[q]
                    ok = (ab > 0.0) & (d > 0.0)
                    wn = np.where(ok, (d * d) / np.where(ok, ab, 1.0), 0.0)
                    for _ in range(en - 1):
                        wn = wn * wn
                    w = w * wn
                else:
                    w = w * 1.0
                if depth is not None:
                    m = np.maximum(np.abs(depth[p]), np.abs(depth[q]))
                    x = np.where(m > 0.0, (depth[p] - depth[q]) / np.where(m > 0.0, sz * m, 1.0), 0.0)
                    w = w * _rat(x * x)
                if albedo is not None:
                    w = w * _rat(_len2(albedo[p] - albedo[q]) / (sa * sa))
                w = w * _rat(_len2(c[p] - c[q]) / ((sv * sv) * (vf[p] + veps)))
                sw[p] = sw[p] + w
                acc[p] = acc[p] + w[..., None] * c[q]
                vacc[p] = vacc[p] + (w * w) * v[q]
            c = np.where(keep[..., None], c, acc / sw[..., None])
            v = np.where(keep, v, vacc / (sw * sw))
        out = c * (albedo + eps) if albedo is not None else c
        return np.where(keep[..., None], rgb, out)


def random_variance(frame: dict, seed: int) -> np.ndarray:
    """A seeded non-negative per-channel variance for a denoise_ref.random_frame: of the size of the frame's own noise
    (its rgb carries +-50 %), about a tenth of the values exactly zero, and zero on the misses."""
    r = np.random.default_rng(seed)
    rgb = frame["rgb"]
    var = (0.3 * rgb) ** 2 * r.uniform(0.0, 2.0, size=rgb.shape)
    var[r.uniform(size=rgb.shape) < 0.1] = 0.0
    var[frame["miss"]] = 0.0
    var.setflags(write=False)
    return var


# The parameter variants both suites run: every guide NULL in turn and both ends of normal_power.
VARIANTS = {
    "defaults": ({}, ()),
    "no_normal": ({}, ("normal",)),
    "no_albedo": ({}, ("albedo",)),
    "no_depth": ({}, ("depth",)),
    "power_1": ({"normal_power": 1}, ()),
    "power_8": ({"normal_power": 8}, ()),
}
VAR_SEED_OFFSET = 77


def variant_inputs(frame: dict, variant: str, iterations: int):
    """(guides dict with the variant's NULLs, params dict) of VARIANTS[variant] at L = iterations."""
    params, nulls = VARIANTS[variant]
    guides = {k: (None if k in nulls else frame[k]) for k in ("normal", "albedo", "depth")}
    return guides, dict(params, iterations=iterations)


_ref_cache: dict = {}


def reference(width: int, height: int, seed: int, variant: str, iterations: int):
    """(frame, variance, guides, params, numpy result), computed once per session and shared read-only."""
    key = (width, height, seed, variant, iterations)
    if key not in _ref_cache:
        frame = R.random_frame(width, height, seed)
        var = random_variance(frame, seed + VAR_SEED_OFFSET)
        guides, params = variant_inputs(frame, variant, iterations)
        ref = denoise_var(frame["rgb"], var, **guides, **params)
        ref.setflags(write=False)
        _ref_cache[key] = (frame, var, guides, params, ref)
    return _ref_cache[key]


# ---- quality against the oracle at 512 spp
# frame: (spp, batches).  MSE_RATIO: MSE(variance-guided, L = 3, defaults) / MSE(noisy) against the oracle's 512-spp frame
# of another seed, as rph_denoise_var measured it with this formula; MSE_CAP: that plus a margin of 0.05 for the
# target's own noise and a change of compiler, and never 1 or above -- beating the noisy frame is the hard condition.
QUALITY = {"bunny_full": (16, 4), "three_balls": (16, 4), "variants": (4, 4), "variants_sky": (4, 4), "earth": (4, 2)}
MSE_RATIO = {"bunny_full": 0.8577, "three_balls": 0.8441, "variants": 0.4939, "variants_sky": 0.5260, "earth": 0.8857}
MSE_MARGIN = 0.05
MSE_CAP = {k: v + MSE_MARGIN for k, v in MSE_RATIO.items()}  # 0.9077, 0.8941, 0.5439, 0.5760, 0.9357
# the guided denoiser (rp_denoise, L = 3, defaults) on the same frames, for comparison: 1.7731, 0.7126, 0.8574, 0.4788, 0.9364

_quality: dict = {}


def quality_case(name: str) -> dict:
    """A frame of tests/aov_ref.py at QUALITY[name] = (spp, B) with the oracle's guides at that spp: {"scene", "params"
    (samples_per_stream = N = spp / B), "noisy" (the oracle's render), "var" (batch_variance of the oracle's B batch
    frames: batch b is the frame at spp = N, samples_per_stream = N, seed + b W H, and S_b = N x it -- exact, N being a
    power of two; the batch frames rebuild `noisy` bit for bit, which is asserted), "target" (the oracle at 512 spp, seed
    SEED + 12345), "normal", "albedo", "depth" (None where the camera has a lens)}; once per session."""
    if name not in _quality:
        import aov_ref
        from parity import oracle_render
        spp, B = QUALITY[name]
        N = spp // B
        assert N * B == spp and N & (N - 1) == 0
        r = aov_ref.refs(name, spp)
        p = replace(r["params"], samples_per_stream=N)
        noisy, _, _ = oracle_render(r["scene"], p)
        sums = np.stack([float(N) * oracle_render(r["scene"], replace(p, spp=N, seed=p.seed + b * p.width * p.height))[0]
                         for b in range(B)], axis=-2)
        x = np.zeros_like(noisy)
        for b in range(B):
            x = x + sums[..., b, :]
        assert np.array_equal(x / float(spp), noisy), "the batch frames do not rebuild the frame"
        target, _, _ = oracle_render(r["scene"], replace(r["params"], spp=512, seed=aov_ref.SEED + 12345))
        out = {"scene": r["scene"], "params": p, "noisy": noisy, "var": batch_variance(sums, spp, N), "target": target,
               "normal": r["normal"], "albedo": r["albedo"], "depth": r.get("depth")}
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _quality[name] = out
    return _quality[name]
