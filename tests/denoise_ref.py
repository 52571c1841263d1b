"""A numpy model of the guided denoiser, written from its definition (include/rp.h rp_denoise) and
not from csrc/rp_denoise.h: every pixel of a level at once, one tap (dy outer, dx inner) after the other, each IEEE
binary64 operation in the definition's order (numpy's elementwise + - * / round once each and never fuse), so the model,
the host library and the device agree to the last bit.  Also the seeded frames and the oracle-built quality cases the
CPU and GPU tests share.
"""
from __future__ import annotations

from dataclasses import replace

import numpy as np

DEFAULTS = {"iterations": 3, "normal_power": 6, "sigma_depth": 0.05, "sigma_albedo": 0.1, "sigma_color": 1.0,
            "albedo_eps": 1e-2}
K = (3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
MSE_CAP = 0.6  # MSE(denoised) <= MSE_CAP * MSE(noisy) against the 512-spp target


def _sum3(x, y, z):
    return (x + y) + z


def _len2(v):
    return _sum3(v[..., 0] * v[..., 0], v[..., 1] * v[..., 1], v[..., 2] * v[..., 2])


def _rat(x2):
    t = 1.0 + x2
    return 1.0 / (t * t)


def denoise(rgb, normal=None, albedo=None, depth=None, **params) -> np.ndarray:
    """The filter on (h, w, 3) rgb with optional guides normal, albedo (h, w, 3) and depth (h, w); params as
    rp_denoise_params' fields (a zero or missing one takes its default)."""
    P = dict(DEFAULTS)
    P.update({k: v for k, v in params.items() if v != 0})
    L, en = int(P["iterations"]), int(P["normal_power"])
    sz, sa, sc, eps = (float(P[k]) for k in ("sigma_depth", "sigma_albedo", "sigma_color", "albedo_eps"))
    rgb = np.asarray(rgb, dtype=np.float64)
    H, W = rgb.shape[:2]
    with np.errstate(all="ignore"):
        nn = _len2(normal) if normal is not None else None
        keep = (nn == 0.0) if nn is not None else np.zeros((H, W), dtype=bool)
        c = rgb / (albedo + eps) if albedo is not None else rgb.copy()
        for lvl in range(L):
            s = 1 << lvl
            scl = sc / float(1 << lvl)
            sw = np.zeros((H, W))
            acc = np.zeros((H, W, 3))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    # pixels p whose tap q = p + s (dx, dy) lies inside the frame
                    j0, j1 = max(0, -s * dy), min(H, H - s * dy)
                    i0, i1 = max(0, -s * dx), min(W, W - s * dx)
                    if j0 >= j1 or i0 >= i1:
                        continue
                    p = (slice(j0, j1), slice(i0, i1))
                    q = (slice(j0 + s * dy, j1 + s * dy), slice(i0 + s * dx, i1 + s * dx))
                    w = np.full((j1 - j0, i1 - i0), K[abs(dx)] * K[abs(dy)])
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
                    if sc >= 0.0:
                        w = w * _rat(_len2(c[p] - c[q]) / (scl * scl))
                    sw[p] = sw[p] + w
                    acc[p] = acc[p] + w[..., None] * c[q]
            c = np.where(keep[..., None], c, acc / sw[..., None])
        out = c * (albedo + eps) if albedo is not None else c
        return np.where(keep[..., None], rgb, out)


def random_frame(width: int, height: int, seed: int) -> dict:
    """A seeded frame with structure the weights react to: 8 x 8 regions of one normal, albedo and depth each plus a
    little noise; about a quarter of the pixels, in 4 x 4 blocks, are misses (zero normal, albedo and depth); a few
    hit pixels have depth zero as well."""
    r = np.random.default_rng(seed)
    H, W = height, width
    jj, ii = np.meshgrid(np.arange(H) // 8, np.arange(W) // 8, indexing="ij")
    region = jj * ((W + 7) // 8) + ii
    n_reg = int(region.max()) + 1
    base_n = r.normal(size=(n_reg, 3))
    normal = base_n[region] + 0.05 * r.normal(size=(H, W, 3))  # not normalised, like a triangle's
    albedo = np.clip(r.uniform(0.1, 0.9, size=(n_reg, 3))[region] + 0.02 * r.normal(size=(H, W, 3)), 0.0, 1.0)
    depth = r.uniform(1.0, 9.0, size=n_reg)[region] * (1.0 + 0.01 * r.normal(size=(H, W)))
    rgb = albedo * r.uniform(0.2, 1.5, size=(n_reg, 1))[region] * (1.0 + 0.5 * r.uniform(-1, 1, size=(H, W, 3)))
    depth[r.uniform(size=(H, W)) < 0.03] = 0.0
    bj, bi = np.meshgrid(np.arange(H) // 4, np.arange(W) // 4, indexing="ij")
    miss = (r.uniform(size=((H + 3) // 4, (W + 3) // 4)) < 0.25)[bj, bi]
    normal[miss] = 0.0
    albedo[miss] = 0.0
    depth[miss] = 0.0
    rgb[miss] = r.uniform(0.0, 1.0, size=(int(miss.sum()), 3))  # a sky
    out = {"rgb": rgb, "normal": normal, "albedo": albedo, "depth": depth, "miss": miss}
    for v in out.values():
        v.setflags(write=False)
    return out


# The parameter variants both suites run: every guide NULL in turn, the colour term disabled, both ends of normal_power.
VARIANTS = {
    "defaults": ({}, ()),
    "no_normal": ({}, ("normal",)),
    "no_albedo": ({}, ("albedo",)),
    "no_depth": ({}, ("depth",)),
    "no_color": ({"sigma_color": -1.0}, ()),
    "power_1": ({"normal_power": 1}, ()),
    "power_8": ({"normal_power": 8}, ()),
}


def variant_inputs(frame: dict, variant: str, iterations: int):
    """(guides dict with the variant's NULLs, params dict) of VARIANTS[variant] at L = iterations."""
    params, nulls = VARIANTS[variant]
    guides = {k: (None if k in nulls else frame[k]) for k in ("normal", "albedo", "depth")}
    return guides, dict(params, iterations=iterations)


_ref_cache: dict = {}


def reference(width: int, height: int, seed: int, variant: str, iterations: int):
    """(frame, guides, params, numpy result), computed once per session and shared read-only."""
    key = (width, height, seed, variant, iterations)
    if key not in _ref_cache:
        frame = random_frame(width, height, seed)
        guides, params = variant_inputs(frame, variant, iterations)
        ref = denoise(frame["rgb"], **guides, **params)
        ref.setflags(write=False)
        _ref_cache[key] = (frame, guides, params, ref)
    return _ref_cache[key]


def mse(a, b) -> float:
    return float(np.mean((np.asarray(a) - np.asarray(b)) ** 2))


_quality: dict = {}


def quality_case(name: str) -> dict:
    """A 64 x 48 frame of tests/aov_ref.py at 4 spp with the oracle's guides: {"scene", "params", "noisy" (the oracle's
    render), "target" (the oracle at 512 spp, seed SEED + 12345), "normal", "albedo", "depth"}; once per session."""
    if name not in _quality:
        import aov_ref
        from parity import oracle_render
        r = aov_ref.refs(name, 4)
        noisy, _, _ = oracle_render(r["scene"], r["params"])
        target, _, _ = oracle_render(r["scene"], replace(r["params"], spp=512, seed=aov_ref.SEED + 12345))
        out = {"scene": r["scene"], "params": r["params"], "noisy": noisy, "target": target, "normal": r["normal"],
               "albedo": r["albedo"], "depth": r["depth"]}
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _quality[name] = out
    return _quality[name]
