"""Numpy models of temporal reprojection, written from the definitions (include/rp.h rp_reproject_device and
rp_accum_frames_counts_device) and not from csrc/rp_reproject.h: every pixel at once, each IEEE binary64
operation in the definition's order (numpy's elementwise + - * /, sqrt and floor round once each and never fuse), the
two tangents from math.tan, so the models, the host library and the device agree to the last bit.  Also the seeded
synthetic frames and camera pairs the CPU and GPU tests share.
"""
from __future__ import annotations

import math

import numpy as np

from accum_ref import same_bits  # noqa: F401  (the tests' comparison)

SIZES = [(1, 1), (2, 2), (65, 3), (37, 23)]
COUNTS = np.array([0, 1, 2, 7], dtype=np.uint32)


class Cam:
    """An rp_camera's fields: orientation R[3 * col + row], position, fov, aspect_ratio."""

    def __init__(self, R, pos, fov, aspect, focal_dist=1.0, lens_radius=0.0):
        self.R = np.asarray(R, dtype=np.float64).reshape(9).copy()
        self.pos = np.asarray(pos, dtype=np.float64).reshape(3).copy()
        self.fov, self.aspect = float(fov), float(aspect)
        self.focal_dist, self.lens_radius = float(focal_dist), float(lens_radius)

    def to_c(self):
        from rtpotato import _ffi as F
        c = F.rp_camera()
        c.aspect_ratio, c.fov, c.focal_dist, c.lens_radius = self.aspect, self.fov, self.focal_dist, self.lens_radius
        c.orientation[:] = [float(x) for x in self.R]
        c.position[:] = [float(x) for x in self.pos]
        return c

    def tans(self):
        ty = np.float64(math.tan(0.5 * self.fov))
        return ty * np.float64(self.aspect), ty


def lookat(eye, target, up=(0.0, 1.0, 0.0)) -> np.ndarray:
    """Orthonormal columns x, y, z with the camera looking down -z, column-major (any such matrix serves the tests)."""
    eye, target, up = (np.asarray(a, dtype=np.float64) for a in (eye, target, up))
    z = eye - target
    z = z / np.sqrt(z @ z)
    x = np.cross(up, z)
    x = x / np.sqrt(x @ x)
    y = np.cross(z, x)
    return np.concatenate([x, y, z])


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def project(cur: Cam, prev: Cam, W: int, H: int, depth, normal):
    """Steps 1 to 6 for every pixel: a dict of (H, W) arrays -- geo, off, fx, fy, i0, j0, a, b, z_exp, nn."""
    depth = np.asarray(depth, dtype=np.float64).reshape(H, W)
    n = np.asarray(normal, dtype=np.float64).reshape(H, W, 3)
    txc, tyc = cur.tans()
    txp, typ = prev.tans()
    Wd, Hd = np.float64(W), np.float64(H)
    with np.errstate(all="ignore"):
        i = np.arange(W, dtype=np.float64)[None, :] + np.zeros((H, 1))
        j = np.arange(H, dtype=np.float64)[:, None] + np.zeros((1, W))
        u = (i + 0.5) / Wd
        v = (j + 0.5) / Hd
        sx = (2.0 * u - 1.0) * txc
        sy = (2.0 * v - 1.0) * tyc
        l = np.sqrt((sx * sx + sy * sy) + 1.0)
        nn = _dot(n[..., 0], n[..., 1], n[..., 2], n[..., 0], n[..., 1], n[..., 2])
        geo = (nn > 0.0) & (depth > 0.0)
        g = depth / l
        Lx = np.where(geo, sx * g, sx)
        Ly = np.where(geo, sy * g, sy)
        Lz = np.where(geo, -g, -1.0)
        R = cur.R
        D = [(R[0 + r] * Lx + R[3 + r] * Ly) + R[6 + r] * Lz for r in range(3)]
        E = [np.where(geo, (D[r] + cur.pos[r]) - prev.pos[r], D[r]) for r in range(3)]
        Q = prev.R
        q = [(Q[3 * c] * E[0] + Q[3 * c + 1] * E[1]) + Q[3 * c + 2] * E[2] for c in range(3)]
        m = -q[2]
        fx = ((q[0] / (m * txp) + 1.0) * 0.5) * Wd - 0.5
        fy = ((q[1] / (m * typ) + 1.0) * 0.5) * Hd - 0.5
        on = (m > 0.0) & (fx > -1.0) & (fx < Wd) & (fy > -1.0) & (fy < Hd)
        fi, fj = np.floor(fx), np.floor(fy)
        a, b = fx - fi, fy - fj
        z_exp = np.sqrt(_dot(q[0], q[1], q[2], q[0], q[1], q[2]))
    i0 = np.where(on, fi, 0.0).astype(np.int64)
    j0 = np.where(on, fj, 0.0).astype(np.int64)
    return {"geo": geo, "off": ~on, "fx": fx, "fy": fy, "i0": i0, "j0": j0, "a": a, "b": b, "z_exp": z_exp, "nn": nn}


def reproject(cur: Cam, prev: Cam, W: int, H: int, depth, normal, depth_prev, normal_prev, mean_prev, m2_prev, count_prev,
              sigma_depth: float = 0.05, normal_cos: float = 0.9, max_history: int = 32):
    """The definition's steps 1 to 9: (mean (H, W, 3), m2 (H, W, 3), count (H, W) uint32, stats uint64[4], info) with
    info = project()'s dict plus, per pixel and tap in tap order (H, W, 4): "counting", the taps that counted;
    "tap_index", the tap's pixel index (0 where it lies outside); "taps", the conditions one by one -- "eligible" (inside
    the frame with w > 0), "count", "class", "depth", "normal" (the last two hold for a sky pixel)."""
    P = project(cur, prev, W, H, depth, normal)
    n = np.asarray(normal, dtype=np.float64).reshape(H, W, 3)
    zp = np.asarray(depth_prev, dtype=np.float64).reshape(-1)
    npv = np.asarray(normal_prev, dtype=np.float64).reshape(-1, 3)
    mp = np.asarray(mean_prev, dtype=np.float64).reshape(-1, 3)
    qp = np.asarray(m2_prev, dtype=np.float64).reshape(-1, 3)
    cp = np.asarray(count_prev).astype(np.uint32).reshape(-1)
    sd, nc = np.float64(sigma_depth), np.float64(normal_cos)
    geo, on = P["geo"], ~P["off"]
    sw = np.zeros((H, W))
    best = np.zeros((H, W))
    n_best = np.zeros((H, W), dtype=np.uint32)
    acc, sacc = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    counting = np.zeros((H, W, 4), dtype=bool)
    tap_index = np.zeros((H, W, 4), dtype=np.int64)
    taps = {k: np.zeros((H, W, 4), dtype=bool) for k in ("eligible", "count", "class", "depth", "normal")}
    with np.errstate(all="ignore"):
        for dy in (0, 1):
            for dx in (0, 1):
                ti, tj = P["i0"] + dx, P["j0"] + dy
                inside = on & (ti >= 0) & (ti < W) & (tj >= 0) & (tj < H)
                w = (P["a"] if dx else 1.0 - P["a"]) * (P["b"] if dy else 1.0 - P["b"])
                t = np.where(inside, tj * W + ti, 0)
                ct = cp[t]
                nt = npv[t]
                nnt = _dot(nt[..., 0], nt[..., 1], nt[..., 2], nt[..., 0], nt[..., 1], nt[..., 2])
                d = zp[t] - P["z_exp"]
                c = _dot(n[..., 0], n[..., 1], n[..., 2], nt[..., 0], nt[..., 1], nt[..., 2])
                flags = {"eligible": inside & (w > 0.0), "count": ct >= 1, "class": np.where(geo, nnt > 0.0, nnt == 0.0),
                         "depth": ~geo | (np.where(d < 0.0, -d, d) <= sd * P["z_exp"]),
                         "normal": ~geo | ((c > 0.0) & (c * c >= (nc * nc) * (P["nn"] * nnt)))}
                ok = flags["eligible"] & flags["count"] & flags["class"] & flags["depth"] & flags["normal"]
                counting[..., 2 * dy + dx] = ok
                tap_index[..., 2 * dy + dx] = t
                for name, val in flags.items():
                    taps[name][..., 2 * dy + dx] = val
                s = np.where((ct >= 2)[..., None], qp[t] / np.maximum(ct.astype(np.float64) - 1.0, 1.0)[..., None], 0.0)
                sw = np.where(ok, sw + w, sw)
                acc = np.where(ok[..., None], acc + w[..., None] * mp[t], acc)
                sacc = np.where(ok[..., None], sacc + w[..., None] * s, sacc)
                better = ok & (w > best)
                best = np.where(better, w, best)
                n_best = np.where(better, ct, n_best)
        kept = n_best >= 1
        count = np.where(kept, np.minimum(n_best, np.uint32(max_history)), 0).astype(np.uint32)
        mean = np.where(kept[..., None], acc / sw[..., None], 0.0)
        df = (count.astype(np.float64) - 1.0)[..., None]
        m2 = np.where(kept[..., None], (sacc / sw[..., None]) * df, 0.0)
    stats = np.array([W * H, int(kept.sum()), int(count.astype(np.uint64).sum()), int(P["off"].sum())], dtype=np.uint64)
    P.update(counting=counting, tap_index=tap_index, taps=taps)
    return mean, m2, count, stats, P


def accum_frames_counts(frames, n_frames: int, n_pixels: int, wpp: int, stride: int, count, mean, m2, var_one: float = 1.0):
    """Frames folded per pixel with k = count + f + 1 (a pixel with count 0 starts at 0.0): (count, mean, m2, var)."""
    frames = np.asarray(frames, dtype=np.float64).reshape(-1)
    c = np.asarray(count).astype(np.uint32).reshape(-1)[:n_pixels]
    start = (c > 0)[:, None]
    mean = np.where(start, np.asarray(mean, dtype=np.float64).reshape(-1)[:n_pixels * wpp].reshape(n_pixels, wpp), 0.0)
    m2 = np.where(start, np.asarray(m2, dtype=np.float64).reshape(-1)[:n_pixels * wpp].reshape(n_pixels, wpp), 0.0)
    with np.errstate(all="ignore"):
        for f in range(n_frames):
            k = c.astype(np.float64) + np.float64(f + 1)
            r = (np.float64(1.0) / k)[:, None]
            x = frames[f * stride:f * stride + n_pixels * wpp].reshape(n_pixels, wpp)
            d = x - mean
            mean = mean + d * r
            m2 = m2 + d * (x - mean)
        n = c.astype(np.float64) + np.float64(n_frames)
        var = np.where((n >= 2.0)[:, None], m2 / (n * (n - 1.0))[:, None], np.float64(var_one))
    return (c + np.uint32(n_frames)).astype(np.uint32), mean.reshape(-1), m2.reshape(-1), var.reshape(-1)


# ---- the cases the CPU and GPU tests share -------------------------------------------------------------------------
def camera_pairs(W: int, H: int) -> dict:
    """(cur, prev) by name: equal, translated, rotated, the previous camera facing away (every pixel off) and a pan
    that pushes a band of pixels off the previous frame."""
    aspect, fov = W / H, 0.9
    eye, tgt = np.array([0.3, 0.4, 4.0]), np.array([0.1, 0.2, 0.0])
    base = Cam(lookat(eye, tgt), eye, fov, aspect)
    moved = Cam(lookat(eye, tgt), eye + np.array([0.11, -0.07, 0.05]), fov, aspect)
    turned = Cam(lookat(eye, tgt + np.array([0.12, -0.05, 0.0])), eye, fov, aspect)
    away = Cam(lookat(eye, 2.0 * eye - tgt), eye, fov, aspect)
    pan = Cam(lookat(eye, tgt + np.array([1.2, 0.0, 0.0])), eye, fov, aspect)
    return {"equal": (base, base), "translated": (base, moved), "rotated": (base, turned), "away": (base, away),
            "band": (base, pan)}


def synthetic(W: int, H: int, seed: int) -> dict:
    """Random frames: depths around 4, unit-ish normals that mostly agree, a fifth of the pixels of either pose sky
    (zeroed normal and depth), previous state in (0, 3) and counts from COUNTS."""
    r = np.random.default_rng(seed)

    def guides():
        depth = r.uniform(3.8, 4.2, size=(H, W))
        normal = np.array([0.1, 0.2, 1.0]) + r.uniform(-0.25, 0.25, size=(H, W, 3))
        sky = r.uniform(size=(H, W)) < 0.2
        depth[sky] = 0.0
        normal[sky] = 0.0
        return depth, normal

    depth, normal = guides()
    depth_prev, normal_prev = guides()
    return {"depth": depth, "normal": normal, "depth_prev": depth_prev, "normal_prev": normal_prev,
            "mean_prev": r.uniform(0.0, 3.0, size=(H, W, 3)), "m2_prev": r.uniform(0.0, 3.0, size=(H, W, 3)),
            "count_prev": r.choice(COUNTS, size=(H, W)).astype(np.uint32)}


def consistent_depth(cam: Cam, W: int, H: int, plane_z: float = 0.0) -> np.ndarray:
    """The distance from the camera to the plane z = plane_z along every pixel's ray, by the model's own reconstruction
    (steps 1 and 3): depth such that the pixel's world point lies on the plane."""
    tx, ty = cam.tans()
    i = np.arange(W, dtype=np.float64)[None, :] + np.zeros((H, 1))
    j = np.arange(H, dtype=np.float64)[:, None] + np.zeros((1, W))
    sx = (2.0 * ((i + 0.5) / W) - 1.0) * tx
    sy = (2.0 * ((j + 0.5) / H) - 1.0) * ty
    l = np.sqrt((sx * sx + sy * sy) + 1.0)
    R = cam.R
    dz = ((R[2] * sx + R[5] * sy) + R[8] * -1.0) / l  # the unit ray's world z
    return (plane_z - cam.pos[2]) / dz


def identity_pair(W: int, H: int):
    """An unrotated camera at the origin, twice: R.v and Rt.v are exact, so q is L itself."""
    cam = Cam([1, 0, 0, 0, 1, 0, 0, 0, 1], [0.0, 0.0, 0.0], 0.9, W / H)
    return cam, cam


def integer_fx_case(seed: int):
    """(cur, prev, buffers) of a 2 x 2 frame through identity_pair: u = 1/4, 3/4, so sx = -+tx/2 exactly and fx comes out
    as the integer i (fy as j) for geometry and sky alike -- a = b = 0 and the taps at dx = 1 and dy = 1 weigh nothing.
    Pixel (1, 0) is sky, pixel (1, 1) holds a NaN mean that only its own pixel may read."""
    cur, prev = identity_pair(2, 2)
    d = synthetic(2, 2, seed)
    d["depth"][:] = d["depth_prev"][:] = [[4.0, 0.0], [3.5, 4.5]]
    d["normal"][:] = d["normal_prev"][:] = [[[0.0, 0.0, 1.0], [0.0, 0.0, 0.0]], [[0.1, 0.2, 0.9], [0.3, 0.0, 0.8]]]
    d["count_prev"][:] = [[2, 1], [7, 2]]
    d["mean_prev"][1, 1] = np.nan
    return cur, prev, d


def nan_case(seed: int, W: int = 37, H: int = 23):
    """(cur, prev, buffers, buffers2, info, t): the translated pair with a NaN state under every pixel whose count_prev
    is 0 (such taps never count), and in buffers2 also a NaN in channel 1 of the mean of tap t, the one that counts
    for the most pixels; info is the model's of the clean buffers (the NaNs change no decision)."""
    cur, prev = camera_pairs(W, H)["translated"]
    d = synthetic(W, H, seed)
    info = reproject(cur, prev, W, H, d["depth"], d["normal"], d["depth_prev"], d["normal_prev"], d["mean_prev"],
                     d["m2_prev"], d["count_prev"])[4]
    empty = d["count_prev"] == 0
    d["mean_prev"][empty] = np.nan
    d["m2_prev"][empty] = np.nan
    counted = np.bincount(info["tap_index"][info["counting"]], minlength=W * H)
    t = int(counted.argmax())
    d2 = {k: v.copy() for k, v in d.items()}
    d2["mean_prev"].reshape(-1, 3)[t, 1] = np.nan
    return cur, prev, d, d2, info, t


# ---- the camera orbit of the end-to-end tests ----------------------------------------------------------------------
ORBIT = {"scene": "bunny_lambert", "width": 96, "height": 64, "spp": 4, "poses": 6, "frames_per_pose": 2,
         "target": (0.0, 0.5, 0.0), "step": math.radians(1.0)}
MASK_SHARE = 0.25  # the share of a pose's pixels that may start over (count <= frames_per_pose after the fold)


def orbit_scene():
    """(scene at ORBIT's size with a pinhole camera, params, cameras): the catalogue camera turned about the vertical
    axis through ORBIT["target"] by ORBIT["step"] per pose, each pose a lookat of its own."""
    from dataclasses import replace

    from rtpotato import scenes
    from rtpotato.scene import RenderParams, Transformation
    o = ORBIT
    sc = scenes.configure(scenes.CATALOGUE[o["scene"]](), o["width"], o["height"])
    sc = replace(sc, camera=replace(sc.camera, lens_radius=0.0))
    tgt = np.array(o["target"])
    p0 = np.array(sc.camera.transformation.position) - tgt
    cams = []
    for k in range(o["poses"]):
        c, s = math.cos(k * o["step"]), math.sin(k * o["step"])
        pos = tgt + np.array([c * p0[0] + s * p0[2], p0[1], -s * p0[0] + c * p0[2]])
        cams.append(replace(sc.camera, transformation=Transformation.lookat(tuple(pos), o["target"], (0.0, 1.0, 0.0))))
    return sc, RenderParams(o["width"], o["height"], o["spp"], 8, 0x5E0A, 32, 32), cams


def as_cam(camera) -> Cam:
    """A Cam of an rtpotato Camera or an rp_camera."""
    c = camera if hasattr(camera, "orientation") else camera.to_c()
    return Cam(list(c.orientation), list(c.position), c.fov, c.aspect_ratio, c.focal_dist, c.lens_radius)
