"""How a ray enters the conservative f32 box test (raytracing-potato_amd/csrc/rp_ray.h through rph_ray_setup: the
header the kernels' setup_ray32 / trav_step and the CPU traversal model compile).

Per axis the header returns the clamped slope inv and two FMA addends; per ray tmin32 and best32.  The error analysis
(rp_ray.h) needs exactly five inequalities, asserted here on generated ray families:

    nb_a <= -oinv_a - D_a     fb_a >= -oinv_a + D_a     D_a >= E_a     tmin32 <= t_min     best32 >= best

with oinv = fl32(o32 inv), E_a = |o - o32||inv|(1 + 6u) + 2u|o32 inv| (+ u(1 + u)|inv|(2 qbound + |o32|) +
u^2|o32 inv| for the quantized node formats), u = 2^-24.  D_a is the header's f64 formula, restated below with numpy
(elementwise IEEE binary64, no contraction -- the host library is built with -ffp-contract=off); E_a and the two
sums are evaluated in numpy.longdouble (64-bit significand on x86: every f32 and f64 input is exact in it, and the
margins tested are >= 2^-24 relative, against its 2^-64).  The addends may be wider than the exact directed roundings
fl_down(-oinv - D), fl_up(-oinv + D) by the one unconditional step the header takes, never tighter; the slack
assertion allows two floats so that a sloppier margin cannot hide.
"""
import numpy as np
import pytest

U = 2.0 ** -24
K = 1.0 + 2.0 ** -20
COORD_MAX = 2.0 ** 54   # rp_layout.h: coordinates beyond are refused by the builder
RAY_EPSILON = 1e-3
F32, Q8, W8 = 1, 2, 3


def _setup(rays, fmt, qbound):
    from rtpotato import _ffi as F
    r = np.ascontiguousarray(rays, dtype=np.float64)
    out = np.full((len(r), 11), np.nan, dtype=np.float32)
    F.check_host(F.host().rph_ray_setup(fmt, float(qbound), r.ctypes.data, len(r), out.ctypes.data))
    return out


def _families():
    """(n, 8) rays {o, d, t_min, best}: every family of the module docstring's list."""
    rng = np.random.default_rng(0x5e7)
    fam = []

    def rays(o, d, tmin=RAY_EPSILON, best=np.inf):
        n = len(o)
        return np.concatenate([o, d, np.broadcast_to(np.asarray(tmin, dtype=np.float64), (n,)).reshape(n, 1),
                               np.broadcast_to(np.asarray(best, dtype=np.float64), (n,)).reshape(n, 1)], axis=1)

    n = 600
    o = rng.uniform(-3, 3, size=(n, 3))
    d = rng.normal(size=(n, 3))
    fam.append(rays(o, d))                                            # random
    for z in (0.0, -0.0):                                              # axis-parallel, zero of either sign
        dz = rng.normal(size=(n, 3))
        dz[np.arange(n), rng.integers(0, 3, size=n)] = z
        dz[: n // 2, 1] = z
        dz[: n // 4, 2] = z
        fam.append(rays(rng.uniform(-3, 3, size=(n, 3)), dz))
        fam.append(rays(np.zeros((8, 3)), np.array([[z, z, 1.0]] * 8)))  # through 0: the exact-frame case
    sgn = rng.choice([-1.0, 1.0], size=(n, 3))
    fam.append(rays(o, sgn * 2.0 ** rng.uniform(-62, -58, size=(n, 3))))   # tiny direction components
    fam.append(rays(o, sgn * 2.0 ** rng.uniform(58, 62, size=(n, 3))))     # huge ones
    fam.append(rays(sgn * 2.0 ** rng.uniform(-62, -58, size=(n, 3)), d))   # tiny origins
    fam.append(rays(o.astype(np.float32).astype(np.float64), d))           # origins that are f32 values
    fam.append(rays(rng.integers(-4, 5, size=(n, 3)).astype(np.float64), d))
    big = sgn * 2.0 ** rng.uniform(40, 54, size=(n, 3))
    big[:50] = sgn[:50] * COORD_MAX
    fam.append(rays(big, d))                                               # |o| up to COORD_MAX
    fam.append(rays(big.astype(np.float32).astype(np.float64), d))
    for tmin in (0.0, RAY_EPSILON, 1e6, 2.0 ** 100):
        fam.append(rays(o[:100], d[:100], tmin=tmin))
    fam.append(rays(o, d, tmin=rng.uniform(0, 10, size=n)))
    fam.append(rays(o, d, best=2.0 ** rng.uniform(-30, 60, size=n)))       # finite best
    fam.append(rays(o[:100], d[:100], best=0.0))
    fam.append(rays(o[:100], d[:100], best=float(np.finfo(np.float32).max)))
    fam.append(rays(o[:100], d[:100], best=np.finfo(np.float64).max))
    fam.append(rays(o[:100], d[:100], best=np.inf))
    return np.concatenate(fam)


RAYS = _families()


def _ord(f):
    """float32 -> int64, monotone in the float order (+-0 both 0): differences count floats."""
    b = np.asarray(f, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def _down(x):  # the exact directed roundings the addends had before: fl_down / fl_up of an f64
    f = x.astype(np.float32)
    return np.where(f.astype(np.float64) > x, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def _up(x):
    f = x.astype(np.float32)
    return np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


@pytest.mark.parametrize("fmt,qbound", [(F32, 0.0), (Q8, 4.0 * 3.0 + 2.0 ** -50), (W8, 4.0 * COORD_MAX + 2.0 ** -50)])
def test_addends_are_conservative_and_tight(fmt, qbound):
    assert 3000 <= len(RAYS) <= 12000
    out = _setup(RAYS, fmt, qbound)
    LD = np.longdouble
    for a in range(3):
        o, d = RAYS[:, a], RAYS[:, 3 + a]
        inv, nb, fb = out[:, a], out[:, 3 + a], out[:, 6 + a]
        o32 = o.astype(np.float32)
        with np.errstate(divide="ignore"):
            inv_ref = np.clip(np.float32(1.0) / d.astype(np.float32), np.float32(-2.0 ** 64), np.float32(2.0 ** 64))
        assert np.array_equal(inv, inv_ref)
        oinv = (o32 * inv).astype(np.float32)
        # the header's D in f64, operation by operation
        e = np.abs(o - o32.astype(np.float64))
        ai = np.abs(inv.astype(np.float64))
        oi = oinv.astype(np.float64)
        D = e * ai * K + np.abs(oi) * 2.0 ** -23
        exact_frame = (np.abs(inv) == np.float32(2.0 ** 64)) & (o32 == 0)
        if fmt != F32:
            D = D + np.where(exact_frame, 0.0, ai * (2.0 * qbound + np.abs(o32.astype(np.float64))) * 2.0 ** -23 * K)
        D = D * K
        # E_a in extended precision; an oinv in the denormal range carries an absolute rounding error of 2^-150, which
        # times 2u is below 2^-173: part of the box test's own 2^-100 term, allowed for here as 2^-170
        o32inv = np.abs(LD(o32) * LD(inv))
        E = LD(e) * LD(ai) * (1 + 6 * LD(U)) + 2 * LD(U) * o32inv
        if fmt != F32:
            E = E + np.where(exact_frame, LD(0), LD(U) * (1 + LD(U)) * LD(ai) * (2 * LD(qbound) + np.abs(LD(o32)))
                             + LD(U) * LD(U) * o32inv)
        assert np.all(LD(D) + LD(2.0) ** -170 >= E), "D_a >= E_a"
        assert np.all(np.isfinite(nb)) and np.all(np.isfinite(fb)) and np.all(np.isfinite(inv))
        assert np.all(LD(nb) <= -LD(oi) - LD(D)), "nb_a <= -oinv_a - D_a"
        assert np.all(LD(fb) >= -LD(oi) + LD(D)), "fb_a >= -oinv_a + D_a"
        assert np.all(LD(nb) <= -LD(oi) - E + LD(2.0) ** -170) and np.all(LD(fb) >= -LD(oi) + E - LD(2.0) ** -170)
        # slack against the exact directed roundings of the same f64 sums: never tighter, at most 2 floats wider
        nb_old, fb_old = _down(-oi - D), _up(-oi + D)
        sn, sf = _ord(nb_old) - _ord(nb), _ord(fb) - _ord(fb_old)
        assert sn.min() >= 0 and sf.min() >= 0
        assert sn.max() <= 2 and sf.max() <= 2, (sn.max(), sf.max())
        assert sn.max() == 1 or sf.max() == 1  # (the header's step is one float: the test sees it taken)


def test_tmin_and_best():
    out = _setup(RAYS, F32, 0.0)
    tmin, best = RAYS[:, 6], RAYS[:, 7]
    tmin32, best32 = out[:, 9], out[:, 10]
    assert np.all(np.isfinite(tmin32))
    assert np.all(tmin32.astype(np.float64) <= tmin)
    s = _ord(_down(tmin)) - _ord(tmin32)
    assert s.min() >= 0 and s.max() <= 2
    assert np.all(tmin32[tmin == 0.0] == -np.float32(2.0 ** -149))  # zero steps to the smallest denormal below it
    assert np.all(best32.astype(np.float64) >= best)
    assert not np.any(np.isnan(best32))
    # no finite float is >= a best above the largest float: +inf there, as for best = +inf; finite everywhere else
    fits = best <= float(np.finfo(np.float32).max)
    huge = best > float(np.finfo(np.float32).max)
    assert np.all(best32[huge] == np.inf) and huge.sum() >= 200
    lower = fits & (best < float(np.finfo(np.float32).max))
    assert np.all(np.isfinite(best32[lower]))
    s = _ord(best32[lower]) - _ord(_up(best[lower]))
    assert s.min() >= 0 and s.max() <= 2


def test_best_sign_and_nan_are_conservative():
    """A negative or NaN best admits no hit at all; best32 is then +inf (the slabs alone cull), never NaN."""
    r = RAYS[:4].copy()
    r[:, 7] = [-1.0, -0.0, np.nan, -np.inf]
    assert np.all(_setup(r, F32, 0.0)[:, 10] == np.inf)


def test_hook_refuses_bad_arguments():
    from rtpotato import _ffi as F
    out = np.zeros(11, dtype=np.float32)
    r = RAYS[:1].copy()
    assert F.host().rph_ray_setup(0, 0.0, r.ctypes.data, 1, out.ctypes.data) == F.RP_EINVAL
    assert F.host().rph_ray_setup(7, 0.0, r.ctypes.data, 1, out.ctypes.data) == F.RP_EINVAL
    assert F.host().rph_ray_setup(Q8, -1.0, r.ctypes.data, 1, out.ctypes.data) == F.RP_EINVAL
    assert F.host().rph_ray_setup(F32, 0.0, None, 1, out.ctypes.data) == F.RP_EINVAL
