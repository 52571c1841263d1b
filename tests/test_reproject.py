"""CPU: temporal reprojection's host models (librp_host.so rph_reproject and rph_accum_frames_counts, loops over
csrc/rp_reproject.h and csrc/rp_accum.h -- the headers the device kernels compile) against the numpy models of
tests/reproject_ref.py bit for bit, the planted edge cases, the identity of an unmoved camera, the refusals, and the
fold's agreement with rph_accum_frames at a uniform count."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import accum_ref as A
import reproject_ref as R
from conftest import REPO

SEED = 20260311
PAIRS = ["equal", "translated", "rotated", "away", "band"]


def host_reproject(cur, prev, d, **kw):
    from rtpotato.render import reproject_host
    return reproject_host(cur, prev, d["depth"], d["normal"], d["depth_prev"], d["normal_prev"], d["mean_prev"],
                          d["m2_prev"], d["count_prev"], params=kw or None)


def model_reproject(cur, prev, d, **kw):
    H, W = d["depth"].shape
    return R.reproject(cur, prev, W, H, d["depth"], d["normal"], d["depth_prev"], d["normal_prev"], d["mean_prev"],
                       d["m2_prev"], d["count_prev"], **kw)


def assert_same(got, ref, what=""):
    assert R.same_bits(got[0], ref[0]), f"{what}: mean"
    assert R.same_bits(got[1], ref[1]), f"{what}: m2"
    assert np.array_equal(got[2], ref[2]), f"{what}: count"
    assert got[3].tolist() == ref[3].tolist(), f"{what}: stats {got[3].tolist()} {ref[3].tolist()}"


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("size", R.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_model_equals_numpy(size, pair):
    """rph_reproject against the numpy model on random buffers, counts in {0, 1, 2, 7}, a fifth of the pixels sky, for
    every camera pair; the previous camera facing away puts every pixel off, the pan a band of them."""
    W, H = size
    cur, prev = R.camera_pairs(W, H)[pair]
    d = R.synthetic(W, H, SEED + 13 * W + H)
    ref = model_reproject(cur, prev, d)
    got = host_reproject(cur, prev, d)
    print(pair, size, "stats", ref[3].tolist())
    assert_same(got, ref, pair)
    n, off = int(ref[3][0]), int(ref[3][3])
    assert n == W * H
    if pair == "away":
        assert off == n and not ref[2].any() and not got[0].any() and not got[1].any()
    if pair == "equal":
        assert off == 0
    if pair in ("translated", "rotated"):  # a small move: at most a border's worth of pixels leaves the frame
        assert off < n // 4 + 1
    if pair == "band" and W >= 37:
        assert 0 < off < n
    if pair != "away" and W * H >= 37 * 23:
        assert 0 < ref[3][1] < n  # some pixels keep their history, some start over


def test_defaults_and_explicit_params():
    """Zero fields and NULL take the defaults; explicit values reach the arithmetic (a count above max_history is cut)."""
    from rtpotato import _ffi as F
    W, H = 37, 23
    cur, prev = R.camera_pairs(W, H)["translated"]
    d = R.synthetic(W, H, SEED + 1)
    assert_same(host_reproject(cur, prev, d, sigma_depth=0.05, normal_cos=0.9, max_history=32), model_reproject(cur, prev, d))
    kw = {"sigma_depth": 0.01, "normal_cos": 0.99, "max_history": 3}
    ref = model_reproject(cur, prev, d, **kw)
    assert_same(host_reproject(cur, prev, d, **kw), ref)
    assert ref[2].max() == 3 and (d["count_prev"] == 7).any()
    assert ref[3][1] < model_reproject(cur, prev, d)[3][1]  # the tighter tests keep fewer pixels
    p = F.rp_reproject_params()
    assert F.rp().rp_reproject_params_init(ctypes.byref(p)) == F.RP_OK
    assert (p.sigma_depth, p.normal_cos, p.max_history, p.reserved) == (0.05, 0.9, 32, 0)


def test_integer_fx_skips_the_zero_weight_taps():
    """A 2 x 2 frame seen through an unrotated camera that has not moved: u = 1/4, 3/4, so sx = -+tx/2 exactly and fx
    comes out as the integer i (fy as j) -- a = b = 0, the taps at dx = 1 and dy = 1 weigh nothing and are skipped even
    where they hold NaN, and every pixel takes its own previous state bit for bit."""
    cur, prev, d = R.integer_fx_case(SEED + 2)
    ref = model_reproject(cur, prev, d)
    info = ref[4]
    assert not info["off"].any() and (info["a"] == 0.0).all() and (info["b"] == 0.0).all()
    assert np.array_equal(info["fx"], [[0.0, 1.0], [0.0, 1.0]]) and np.array_equal(info["fy"], [[0.0, 0.0], [1.0, 1.0]])
    assert info["geo"].tolist() == [[True, False], [True, True]]
    assert info["counting"].reshape(4, 4).tolist() == [[True, False, False, False]] * 4
    got = host_reproject(cur, prev, d)
    assert_same(got, ref)
    assert np.array_equal(got[2], d["count_prev"])
    assert R.same_bits(got[0], d["mean_prev"]) and np.isnan(got[0][1, 1]).all() and np.isfinite(got[0][:1]).all()
    # m2 = (m2_prev / (count - 1)) * (count - 1): the per-frame variance and back, 0 for a single frame
    assert (got[1][0, 1] == 0.0).all() and np.allclose(got[1][1, 0], d["m2_prev"][1, 0], rtol=4e-16, atol=0.0)


def test_each_tap_condition_fails_on_its_own_and_nan_stays_where_it_counts():
    """On the translated pair at 37 x 23 the inputs hold, for each of the count, class, depth and normal conditions, a
    tap inside the frame with w > 0 that fails that condition alone.  Every pixel with count_prev = 0 then gets a NaN
    state -- such a tap is a neighbour of pixels that keep history, which must stay finite -- and one tap that does
    count gets a NaN mean, which must show in exactly the pixels it counts for."""
    W, H = 37, 23
    cur, prev, d, d2, info, t = R.nan_case(SEED + 3)
    taps = info["taps"]
    names = ("count", "class", "depth", "normal")
    for name in names:
        alone = taps["eligible"] & ~taps[name]
        for other in names:
            if other != name:
                alone &= taps[other]
        print(name, "fails alone in", int(alone.sum()), "taps")
        assert alone.any(), name
    empty = d["count_prev"] == 0
    assert np.isnan(d["mean_prev"][empty]).all() and np.isnan(d["m2_prev"][empty]).all()
    flat_empty = empty.reshape(-1)
    # a tap without history beside one that counts, for the same pixel
    mixed = (taps["eligible"] & flat_empty[info["tap_index"]]).any(axis=2) & info["counting"].any(axis=2)
    assert mixed.any()
    ref = model_reproject(cur, prev, d)
    got = host_reproject(cur, prev, d)
    assert_same(got, ref)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    # now a NaN where it counts: the tap most pixels count
    counted = int(((info["tap_index"] == t) & info["counting"]).any(axis=2).sum())
    assert counted >= 2
    ref = model_reproject(cur, prev, d2)
    got = host_reproject(cur, prev, d2)
    assert_same(got, ref)
    hit = ((info["tap_index"] == t) & info["counting"]).any(axis=2)
    assert hit.sum() == counted and np.array_equal(np.isnan(got[0][..., 1]), hit)
    assert np.isfinite(got[0][..., 0]).all() and np.isfinite(got[1]).all()


def neighbour_spread(a):
    """The largest |a[p] - a[q]| over pixels p, q that are 8-neighbours, over all channels."""
    H, W = a.shape[:2]
    big = 0.0
    for dy in (0, 1):
        for dx in (-1, 0, 1):
            if (dy, dx) in ((0, 0), (0, -1)) or dy >= H or abs(dx) >= W:
                continue
            p = a[:H - dy, max(0, -dx):W - max(0, dx)]
            q = a[dy:, max(0, dx):W - max(0, -dx)]
            big = max(big, float(np.abs(p - q).max()))
    return big


@pytest.mark.parametrize("size", [(37, 23), (65, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_unmoved_camera_keeps_every_pixel(size):
    """Equal cameras and a depth that is the model's own reconstruction of a plane, the same at both poses: every
    pixel lands on itself up to rounding, e = max(|fx - i|, |fy - j|) < 1e-9 (asserted), so with every count_prev >= 1
    its own tap counts (equal normal: c*c = nn*nn; equal depth up to the rounding of R and its transpose, far inside
    sigma_depth) with weight w_self >= (1 - e)^2, the heaviest, hence count == count_prev.  The other taps weigh at
    most 1 - (1 - e)^2 <= 2e together and sw >= w_self, so
        |mean - mean_prev| = |sum_{t != self} w_t (mean_t - mean_self)| / sw <= 2e / (1 - 2e) * D + rounding,
    D the largest difference between 8-neighbours of mean_prev; the rounding of four products, three sums and one
    division is below 8 ulp of the largest |mean_prev|.  m2 likewise against the per-frame variance."""
    W, H = size
    cur, _ = R.camera_pairs(W, H)["equal"]
    d = R.synthetic(W, H, SEED + 4)
    depth = R.consistent_depth(cur, W, H)
    assert (depth > 0).all() and np.isfinite(depth).all()
    sky = d["normal"][..., 2] == 0.0
    assert sky.any() and not sky.all()
    d["depth"] = np.where(sky, 0.0, depth)
    d["depth_prev"], d["normal_prev"] = d["depth"].copy(), d["normal"].copy()
    d["count_prev"] = np.random.default_rng(SEED + 5).choice(R.COUNTS[1:], size=(H, W)).astype(np.uint32)
    ref = model_reproject(cur, cur, d)
    got = host_reproject(cur, cur, d)
    assert_same(got, ref)
    info = ref[4]
    ii, jj = np.meshgrid(np.arange(W), np.arange(H))
    e = max(float(np.abs(info["fx"] - ii).max()), float(np.abs(info["fy"] - jj).max()))
    D = neighbour_spread(d["mean_prev"])
    bound = 2 * e / (1 - 2 * e) * D + 8 * np.finfo(np.float64).eps * float(np.abs(d["mean_prev"]).max())
    err = float(np.abs(got[0] - d["mean_prev"]).max())
    print(f"{W}x{H}: e = {e:.3g}, D = {D:.3g}, |mean - mean_prev| max {err:.3g}, bound {bound:.3g}")
    assert e < 1e-9
    assert np.array_equal(got[2], d["count_prev"]) and info["geo"].sum() == (~sky).sum()
    assert err <= bound
    assert got[3].tolist() == [W * H, W * H, int(d["count_prev"].sum()), 0]


def test_reprojected_count_continues_the_fold():
    """A pixel reprojected with count = 5 and then folded with one frame x takes r = 1 / 6: mean + (x - mean) * (1 / 6)
    and the count 6; its variance is m2 / (6 * 5)."""
    from rtpotato.render import accum_frames_counts_host
    W = H = 2
    cur, prev = R.identity_pair(W, H)
    d = R.synthetic(W, H, SEED + 6)
    d["depth"][:] = d["depth_prev"][:] = 4.0
    d["normal"][:] = d["normal_prev"][:] = [0.0, 0.6, 0.8]
    d["count_prev"][:] = 5
    mean, m2, count, _ = host_reproject(cur, prev, d)
    assert (count == 5).all() and R.same_bits(mean, d["mean_prev"])
    x = np.random.default_rng(SEED + 7).uniform(0.0, 3.0, size=(H, W, 3))
    m0, q0 = mean.copy(), m2.copy()
    var = np.empty_like(mean)
    accum_frames_counts_host(x, 1, count.reshape(-1), mean.reshape(-1), m2.reshape(-1), var=var.reshape(-1))
    r = np.float64(1.0) / np.float64(6.0)
    dd = x - m0
    assert (count == 6).all()
    assert R.same_bits(mean, m0 + dd * r)
    assert R.same_bits(m2, q0 + dd * (x - mean)) and R.same_bits(var, m2 / (np.float64(6.0) * np.float64(5.0)))


@pytest.mark.parametrize("wpp,n_pixels,pad", [(1, 1, 0), (1, 131, 3), (3, 77, 0), (3, 130, 5), (2, 9, 1)])
@pytest.mark.parametrize("n_frames", [1, 2, 5])
def test_counts_fold_equals_numpy(n_frames, wpp, n_pixels, pad):
    """rph_accum_frames_counts against the numpy model: counts in {0, 1, 2, 7} per pixel, a NaN state under the pixels
    with count 0 (never read), var_one where a pixel ends with one frame."""
    from rtpotato.render import accum_frames_counts_host
    n_words = n_pixels * wpp
    stride = n_words + pad
    r = np.random.default_rng(SEED + 100 * n_frames + n_pixels)
    frames = A.synthetic(n_frames, n_words, stride, SEED + n_pixels)
    count = r.choice(R.COUNTS, size=n_pixels).astype(np.uint32)
    mean, m2 = r.uniform(0.0, 3.0, size=n_words), r.uniform(0.0, 3.0, size=n_words)
    fresh = np.repeat(count == 0, wpp)
    mean[fresh] = m2[fresh] = np.nan
    ref = R.accum_frames_counts(frames, n_frames, n_pixels, wpp, stride, count, mean, m2, var_one=0.25)
    c, var = count.copy(), np.full(n_words, A.PAD)
    accum_frames_counts_host(frames, n_frames, c, mean, m2, var=var, var_one=0.25, words_per_pixel=wpp, stride=stride)
    assert np.array_equal(c, ref[0]) and np.array_equal(c, count + n_frames)
    assert R.same_bits(mean, ref[1]) and R.same_bits(m2, ref[2]) and R.same_bits(var, ref[3])
    one = np.repeat(c == 1, wpp)
    assert (var[one] == 0.25).all() and one.any() == (n_frames == 1 and (count == 0).any())
    if n_frames == 1:
        assert R.same_bits(mean[fresh], frames[:n_words][fresh])


@pytest.mark.parametrize("c", [0, 1, 6])
def test_uniform_count_equals_the_plain_fold(c):
    """The defined property: with every count equal to c, mean, m2 and var equal rph_accum_frames' with n_prior = c."""
    from rtpotato.render import accum_frames_counts_host, accum_frames_host
    n_pixels, wpp, n_frames = 127, 3, 3
    n_words = n_pixels * wpp
    frames = A.synthetic(n_frames, n_words, n_words + 2, SEED + 8)
    r = np.random.default_rng(SEED + 9)
    mean, m2 = r.uniform(0.0, 3.0, size=n_words), r.uniform(0.0, 3.0, size=n_words)
    a = [mean.copy(), m2.copy(), np.empty(n_words)]
    b = [mean.copy(), m2.copy(), np.empty(n_words)]
    accum_frames_host(frames, n_frames, a[0], a[1], n_prior=c, var=a[2], stride=n_words + 2)
    count = np.full(n_pixels, c, dtype=np.uint32)
    accum_frames_counts_host(frames, n_frames, count, b[0], b[1], var=b[2], stride=n_words + 2)
    assert (count == c + n_frames).all()
    for x, y in zip(a, b):
        assert R.same_bits(x, y)


def test_reproject_refusals():
    """Each RP_EINVAL case of rph_reproject arrives with its message, and nothing is written."""
    from rtpotato import _ffi as F
    L = F.host()
    W, H = 5, 4
    cur, prev = R.camera_pairs(W, H)["translated"]
    d = R.synthetic(W, H, SEED + 10)
    out = {"mean": np.full((H, W, 3), A.PAD), "m2": np.full((H, W, 3), A.PAD),
           "count": np.full((H, W), 77, dtype=np.uint32), "stats": np.full(4, 77, dtype=np.uint64)}
    order = ["depth", "normal", "depth_prev", "normal_prev", "mean_prev", "m2_prev", "count_prev", "mean", "m2", "count",
             "stats"]
    bufs = {**d, **out}

    def call(params=None, width=W, height=H, cur_=cur, prev_=prev, **swap):
        ptrs = [None if k in swap and swap[k] is None else swap.get(k, bufs[k]).ctypes.data for k in order]
        cc = ctypes.byref(cur_.to_c()) if cur_ is not None else None
        cp = ctypes.byref(prev_.to_c()) if prev_ is not None else None
        return L.rph_reproject(ctypes.byref(params) if params is not None else None, width, height, cc, cp, *ptrs)

    assert call() == F.RP_OK
    for a in out.values():
        a[...] = 77 if a.dtype != np.float64 else A.PAD
    cases = [({k: None}, b"non-NULL") for k in order]
    cases += [({"cur_": None}, b"non-NULL"), ({"prev_": None}, b"non-NULL")]
    cases += [({"width": 0}, b"1..65535"), ({"height": 0}, b"1..65535"), ({"width": 65536}, b"1..65535"),
              ({"height": 70000}, b"1..65535")]
    for kw in ({"sigma_depth": -0.05}, {"sigma_depth": float("nan")}, {"sigma_depth": float("inf")},
               {"normal_cos": -0.5}, {"normal_cos": 1.5}, {"normal_cos": float("nan")}, {"max_history": 2 ** 31}):
        cases.append(({"params": F.rp_reproject_params(**kw)}, b"out of range"))
    for field, value in (("fov", float("nan")), ("fov", 0.0), ("fov", -0.9), ("aspect", float("inf")),
                         ("focal_dist", float("nan")), ("lens_radius", float("inf"))):
        for which in ("cur_", "prev_"):
            cam = R.Cam(cur.R, cur.pos, cur.fov, cur.aspect)
            setattr(cam, field, value)
            cases.append(({which: cam}, b"camera"))
    bad = R.Cam(cur.R, cur.pos, cur.fov, cur.aspect)
    bad.R[4] = np.nan
    cases.append(({"cur_": bad}, b"camera"))
    bad = R.Cam(cur.R, cur.pos, cur.fov, cur.aspect)
    bad.pos[2] = np.inf
    cases.append(({"prev_": bad}, b"camera"))
    # an output on an input, and on another output
    for o in ("mean", "m2"):
        for i in ("normal", "normal_prev", "mean_prev", "m2_prev"):
            cases.append(({o: bufs[i]}, b"alias an input"))
    cases += [({"count": d["count_prev"]}, b"alias an input"), ({"mean": d["depth"].reshape(-1)[3:]}, b"alias an input"),
              ({"m2": out["mean"]}, b"one another"), ({"stats": out["m2"].reshape(-1)[5:].view(np.uint64)}, b"one another"),
              ({"count": out["mean"].reshape(-1)[50:].view(np.uint32)}, b"one another")]
    for kw, msg in cases:
        assert call(**kw) == F.RP_EINVAL, kw
        assert msg in L.rph_last_error(), (kw, L.rph_last_error())
    assert all((a == (77 if a.dtype != np.float64 else A.PAD)).all() for a in out.values())
    ok = F.rp_reproject_params(sigma_depth=1e-3, normal_cos=1.0, max_history=2 ** 31 - 1)
    assert call(params=ok) == F.RP_OK


def test_counts_fold_refusals():
    """Each RP_EINVAL case of rph_accum_frames_counts arrives with its message, and nothing is written."""
    from rtpotato import _ffi as F
    L = F.host()
    fr = np.ones(40)
    mean, m2, var = np.full(6, A.PAD), np.full(6, A.PAD), np.full(6, A.PAD)
    count = np.full(2, 3, dtype=np.uint32)
    p = lambda a: a.ctypes.data if a is not None else None

    def call(n_pixels=2, wpp=3, n_frames=3, frames=fr, stride=6, count_=count, mean_=mean, m2_=m2, var_=var, var_one=1.0):
        return L.rph_accum_frames_counts(n_pixels, wpp, n_frames, p(frames), stride, p(count_), p(mean_), p(m2_), p(var_),
                                         var_one)

    for kw, msg in (({"frames": None}, b"non-NULL"), ({"mean_": None}, b"non-NULL"), ({"m2_": None}, b"non-NULL"),
                    ({"count_": None}, b"non-NULL"), ({"n_frames": 0}, b"n_frames is zero"),
                    ({"n_pixels": 0}, b"is zero"), ({"wpp": 0}, b"is zero"), ({"stride": 5}, b"frame_stride"),
                    ({"n_frames": 2 ** 31}, b"2^31 - 1"), ({"n_pixels": 2 ** 39}, b"2^40 - 512"),
                    ({"var_one": -1.0}, b"var_one"), ({"var_one": float("inf")}, b"var_one"),
                    ({"var_one": float("nan")}, b"var_one"),
                    ({"mean_": fr[8:]}, b"alias the frames"), ({"m2_": fr[11:]}, b"alias the frames"),
                    ({"var_": fr[1:]}, b"alias the frames"), ({"m2_": mean}, b"one another"),
                    ({"var_": m2[1:]}, b"one another"), ({"count_": fr[3:].view(np.uint32)}, b"count must not alias"),
                    ({"count_": mean[2:].view(np.uint32)}, b"count must not alias"),
                    ({"count_": var.view(np.uint32)}, b"count must not alias")):
        assert call(**kw) == F.RP_EINVAL, kw
        assert msg in L.rph_last_error(), (kw, L.rph_last_error())
    assert (fr == 1.0).all() and all((a == A.PAD).all() for a in (mean, m2, var)) and (count == 3).all()
    assert call(var_=None) == F.RP_OK and (count == 6).all()
    assert call(n_frames=1, var_one=0.0) == F.RP_OK  # one frame: no refusal, the stand-in serves


def test_reproject_params_struct(tmp_path):
    """sizeof and offsets of rp_reproject_params and RP_REPROJECT_STATS_LEN against a tiny C program."""
    from rtpotato import _ffi as F
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rp.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %d\\n", sizeof(rp_reproject_params), offsetof(rp_reproject_params, sigma_depth),\n'
                   '         offsetof(rp_reproject_params, normal_cos), offsetof(rp_reproject_params, max_history),\n'
                   '         offsetof(rp_reproject_params, reserved), RP_REPROJECT_STATS_LEN);\n  return 0;\n}\n')
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = F.rp_reproject_params
    assert sizes == [ctypes.sizeof(P), P.sigma_depth.offset, P.normal_cos.offset, P.max_history.offset, P.reserved.offset,
                     F.RP_REPROJECT_STATS_LEN] == [24, 0, 8, 16, 20, 4]


def test_prev_camera_inverts_a_tilted_lookat():
    """Transformation.lookat leaves x = up x z unnormalised, so a camera that looks down has x and y columns shorter
    than 1 and the transpose of its orientation is not its inverse: taken as `prev` as it is, an unmoved camera lands
    its pixels off themselves (by the factor |x|^2 about the centre); as reproject_prev_camera gives it -- the inverse
    transpose -- every pixel lands on itself to rounding and keeps its count."""
    from rtpotato.render import reproject_prev_camera
    sc, p, cams = R.orbit_scene()
    W, H = p.width, p.height
    cam = R.as_cam(cams[0])
    x = cam.R[:3]
    assert float(x @ x) < 0.95  # the catalogue camera looks down on the bunny
    dual = R.as_cam(reproject_prev_camera(cams[0]))
    assert np.allclose(dual.R.reshape(3, 3) @ cam.R.reshape(3, 3).T, np.eye(3), rtol=0, atol=1e-15)
    d = R.synthetic(W, H, SEED + 11)
    d["depth"] = R.consistent_depth(cam, W, H, plane_z=-1.0)
    d["normal"][:] = [0.0, 0.0, 1.0]
    d["depth_prev"], d["normal_prev"] = d["depth"].copy(), d["normal"].copy()
    d["count_prev"][:] = 3
    ii, jj = np.meshgrid(np.arange(W), np.arange(H))
    raw = model_reproject(cam, cam, d)[4]
    assert float(np.abs(raw["fx"] - ii).max()) > 1.0
    ref = model_reproject(cam, dual, d)
    got = host_reproject(cams[0], reproject_prev_camera(cams[0]), d)
    assert_same(got, ref)
    e = max(float(np.abs(ref[4]["fx"] - ii).max()), float(np.abs(ref[4]["fy"] - jj).max()))
    print("tilted camera: e =", e)
    assert e < 1e-9 and (got[2] == 3).all()


def test_orbit_step_keeps_most_of_the_history():
    """The end-to-end GPU test's orbit, judged on the CPU: the oracle's depth and normals at the last two poses and the
    host model, every previous pixel holding history -- fewer than MASK_SHARE of the pixels start over and more than half
    keep theirs, so the test on the device shows reprojection at work."""
    import aov_ref
    from dataclasses import replace
    from rtpotato.render import reproject_host, reproject_prev_camera
    sc, p, cams = R.orbit_scene()
    W, H = p.width, p.height
    guides = []
    for cam in cams[-2:]:
        s = replace(sc, camera=cam)
        depth, _, _ = aov_ref.depth_ref(s, p)
        normal, _ = aov_ref.normal_ref(s, p)
        guides.append((depth, normal))
    state = np.zeros((H, W, 3))
    count = np.full((H, W), 2, dtype=np.uint32)
    _, _, c, stats = reproject_host(cams[-1], reproject_prev_camera(cams[-2]), guides[1][0], guides[1][1], guides[0][0],
                                    guides[0][1], state, state, count)
    lost = float((c == 0).mean())
    print(f"orbit step {R.ORBIT['step']:.4f} rad: {lost:.3%} of the pixels start over, stats {stats.tolist()}")
    assert lost < R.MASK_SHARE
    assert stats[1] > 0.5 * stats[0]
