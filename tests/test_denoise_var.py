"""CPU: the variance pass's and the variance-guided denoiser's host models (librp_host.so rph_batch_variance and
rph_denoise_var, loops over csrc/rp_variance.h and csrc/rp_denoise.h -- the headers the device kernels compile) against
the numpy models of tests/denoise_var_ref.py bit for bit, the filter's pass-through and constant properties, its quality
against the oracle's 512-spp frames, and the ABI's host-only parts."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as R
import denoise_var_ref as V
from conftest import REPO

SEED = 20260113


def _host(rgb, var, guides, params):
    from rtpotato.render import denoise_host
    return denoise_host(rgb, params=params, variance=var, **guides)


@pytest.mark.parametrize("variant", list(V.VARIANTS))
@pytest.mark.parametrize("width,height", [(70, 37), (7, 5)])
def test_host_model_equals_numpy(width, height, variant):
    """L = 5 (steps 1 .. 16: on 7 x 5 most taps leave the frame), a quarter of the pixels misses in blocks with zero
    variance, a tenth of the other variances exactly zero; every guide NULL in turn, normal_power 1 and 8."""
    frame, var, guides, params, ref = V.reference(width, height, SEED, variant, 5)
    out = _host(frame["rgb"], var, guides, params)
    assert np.isfinite(ref).all()
    assert (var >= 0.0).all() and (var[~frame["miss"]] == 0.0).any() and not var[frame["miss"]].any()
    diff = np.abs(out - ref)
    print(variant, width, height, "max |host - numpy|", float(diff.max()), "pixels differing", int((diff > 0).any(-1).sum()))
    assert np.array_equal(out, ref)
    # it is another filter than rp_denoise
    assert not np.array_equal(out, R.reference(width, height, SEED, variant, 5)[3])


@pytest.mark.parametrize("spp,sps", [(12, 4), (10, 4), (2, 1)])
def test_batch_variance_equals_numpy(spp, sps):
    """rph_batch_variance against the numpy model, bit for bit: three equal batches, a partial last batch (4, 4, 2) and
    the smallest case B = 2; against the textbook estimator where the batches are equal."""
    from rtpotato.render import batch_variance_host
    B = (spp + sps - 1) // sps
    r = np.random.default_rng(SEED + spp)
    sums = r.uniform(0.0, 3.0, size=(9, 11, B, 3)) * sps
    sums[0, 0] = 0.0
    var = batch_variance_host(sums, spp, sps)
    ref = V.batch_variance(sums, spp, sps)
    assert var.shape == (9, 11, 3) and np.array_equal(var, ref)
    assert (var >= 0.0).all() and not var[0, 0].any()
    if spp % sps == 0:
        # every e_b carries a few ulps of the batch means (<= 3, so ~1e-15): 2 e_b 1e-15, summed and scaled, is far
        # below 1e-13
        textbook = np.var(sums / sps, axis=-2, ddof=1) / B
        print("equal batches: max distance to var(ddof = 1) / B", float(np.max(np.abs(var - textbook))))
        assert np.allclose(var, textbook, rtol=0.0, atol=1e-13)


def test_batch_variance_refusals():
    """B = 1 (spp <= samples_per_stream, the default 32 included) and NULL buffers are RP_EINVAL."""
    from rtpotato import _ffi as F
    H = F.host()
    s, v = np.zeros((4, 3)), np.zeros(3)
    assert H.rph_batch_variance(4, 2, 1, s.ctypes.data, v.ctypes.data) == F.RP_OK
    for spp, sps in ((4, 4), (3, 4), (1, 1), (0, 1), (32, 0)):
        assert H.rph_batch_variance(spp, sps, 1, s.ctypes.data, v.ctypes.data) == F.RP_EINVAL, (spp, sps)
        assert b"batches" in H.rph_last_error()
    assert H.rph_batch_variance(33, 0, 0, s.ctypes.data, v.ctypes.data) == F.RP_OK  # 0: 32 samples per stream, B = 2
    assert H.rph_batch_variance(4, 2, 1, None, v.ctypes.data) == F.RP_EINVAL
    assert H.rph_batch_variance(4, 2, 1, s.ctypes.data, None) == F.RP_EINVAL


def test_pass_through_and_constant():
    """Pixels with nn == 0 return rgb bit for bit (every variant that has a normal guide); a frame whose demodulated
    colour is one constant comes back within 1e-12, whatever the variance."""
    frame = R.random_frame(70, 37, SEED)
    var = V.random_variance(frame, SEED + V.VAR_SEED_OFFSET)
    miss = frame["miss"]
    for variant in ("defaults", "no_albedo", "no_depth"):
        guides, params = V.variant_inputs(frame, variant, 5)
        out = _host(frame["rgb"], var, guides, params)
        assert np.array_equal(out[miss], frame["rgb"][miss]), variant
        assert not np.array_equal(out[~miss], frame["rgb"][~miss]), variant
    eps = R.DEFAULTS["albedo_eps"]
    rgb = np.where(miss[..., None], frame["rgb"], 0.75 * (frame["albedo"] + eps))
    g = {k: frame[k] for k in ("normal", "albedo", "depth")}
    for name, v in (("seeded", var), ("zero", np.zeros_like(var)), ("huge", np.full_like(var, 1e6))):
        out = _host(rgb, v, g, {"iterations": 5})
        err = np.abs(out - rgb) / np.maximum(1.0, np.abs(rgb))
        print(f"constant demodulated colour, {name} variance: max relative error", float(err.max()))
        assert err.max() <= 1e-12


@pytest.mark.parametrize("name", list(V.QUALITY))
def test_quality_against_oracle(name):
    """The oracle's low-spp frame, its guides and the variance of its batch frames, against the oracle at 512 spp and
    another seed: MSE(denoised) < MSE(noisy) on every frame, on bunny_full (glass and metal before a textured sky, where
    rp_denoise loses: 1.77) also below rp_denoise's, and within the frame's measured ratio plus its margin
    (denoise_var_ref.MSE_RATIO, MSE_CAP)."""
    from rtpotato.render import denoise_host
    q = V.quality_case(name)
    g = {k: q[k] for k in ("normal", "albedo", "depth")}
    out = _host(q["noisy"], q["var"], g, None)
    plain = denoise_host(q["noisy"], **g)
    noisy, den, pl = R.mse(q["noisy"], q["target"]), R.mse(out, q["target"]), R.mse(plain, q["target"])
    print(f"{name}: MSE noisy {noisy:.6g}, variance-guided {den:.6g} (ratio {den / noisy:.4f}), rp_denoise {pl:.6g} "
          f"(ratio {pl / noisy:.4f})")
    assert np.isfinite(out).all()
    assert den < noisy
    if name == "bunny_full":
        assert den < pl
    assert den <= V.MSE_CAP[name] * noisy


def test_params_struct_and_defaults(tmp_path):
    """sizeof and offsets of rp_denoise_var_params (and rp_denoise_params, still 40 bytes) against a tiny C program;
    rp_denoise_var_params_init's documented defaults; a zero field and NULL mean the defaults; sigma_color is ignored."""
    from rtpotato import _ffi as F
    from rtpotato.render import denoise_var_defaults, denoise_var_params
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rp.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(rp_denoise_params), sizeof(rp_denoise_var_params),\n'
                   '         offsetof(rp_denoise_var_params, base), offsetof(rp_denoise_var_params, sigma_var),\n'
                   '         offsetof(rp_denoise_var_params, var_eps));\n  return 0;\n}\n')
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = F.rp_denoise_var_params
    assert sizes == [ctypes.sizeof(F.rp_denoise_params), ctypes.sizeof(P), P.base.offset, P.sigma_var.offset,
                     P.var_eps.offset] == [40, 56, 0, 40, 48]
    d = denoise_var_defaults()
    assert (d.sigma_var, d.var_eps) == (3.0, 1e-6)
    assert {k: getattr(d.base, k) for k in R.DEFAULTS} == R.DEFAULTS
    assert {**{k: getattr(d.base, k) for k in R.DEFAULTS}, "sigma_var": d.sigma_var, "var_eps": d.var_eps} == V.DEFAULTS
    assert F.rp().rp_denoise_var_params_init(None) == F.RP_EINVAL
    frame = R.random_frame(7, 5, SEED)
    var = V.random_variance(frame, SEED)
    g = {k: frame[k] for k in ("normal", "albedo", "depth")}
    ref = _host(frame["rgb"], var, g, d)
    assert np.array_equal(_host(frame["rgb"], var, g, None), ref)
    assert np.array_equal(_host(frame["rgb"], var, g, F.rp_denoise_var_params()), ref)
    for sc in (-1.0, 0.25, float("nan")):
        assert np.array_equal(_host(frame["rgb"], var, g, denoise_var_params(sigma_color=sc)), ref), sc
    assert not np.array_equal(_host(frame["rgb"], var, g, {"sigma_var": 1.0}), ref)
    with pytest.raises(KeyError):
        denoise_var_params(sigma_nothing=1.0)


def test_host_refusals():
    """rph_denoise_var: RP_EINVAL for NULL rgb, var or out, a zero size, out aliasing an input (var included),
    non-finite or non-positive sigma_var and var_eps, and the base's ranges."""
    from rtpotato import _ffi as F
    from rtpotato.render import denoise_var_params
    H = F.host()
    frame = R.random_frame(7, 5, SEED)
    rgb, nrm = np.array(frame["rgb"]), np.array(frame["normal"])
    var = np.array(V.random_variance(frame, SEED))
    out = np.empty_like(rgb)

    def call(p=None, w=7, h=5, rgb_=rgb, var_=var, normal=nrm, out_=out):
        ptr = lambda a: a.ctypes.data if a is not None else None
        return H.rph_denoise_var(ctypes.byref(p) if p is not None else None, w, h, ptr(rgb_), ptr(var_), ptr(normal), None,
                                 None, ptr(out_))

    assert call() == F.RP_OK
    assert call(rgb_=None) == F.RP_EINVAL and call(out_=None) == F.RP_EINVAL and call(var_=None) == F.RP_EINVAL
    assert call(w=0) == F.RP_EINVAL and call(h=0) == F.RP_EINVAL
    for alias in (rgb, nrm, var, var.reshape(-1)[3:]):
        assert call(out_=alias) == F.RP_EINVAL
        assert b"alias" in H.rph_last_error()
    for bad in ({"sigma_var": -3.0}, {"sigma_var": float("nan")}, {"sigma_var": float("inf")}, {"var_eps": -1e-6},
                {"var_eps": float("nan")}, {"var_eps": float("inf")}, {"iterations": 9}, {"normal_power": 9},
                {"sigma_depth": -1.0}, {"albedo_eps": float("inf")}):
        assert call(denoise_var_params(**bad)) == F.RP_EINVAL, bad
    for good in ({"sigma_var": 0.5}, {"var_eps": 1e-12}, {"iterations": 8, "normal_power": 1}, {"sigma_color": -1.0}):
        assert call(denoise_var_params(**good)) == F.RP_OK, good


def test_scratch_bytes_without_gpu():
    """rp_denoise_var_scratch_bytes is host only: two colour buffers and two variance buffers, 2 x (24 + 8) bytes per
    pixel; zero sizes are refused; rp_denoise's scratch is what it was."""
    from rtpotato import _ffi as F
    from rtpotato.render import denoise_scratch_bytes, denoise_var_scratch_bytes
    assert denoise_var_scratch_bytes(70, 37) == 2 * (24 + 8) * 70 * 37
    assert denoise_var_scratch_bytes(1920, 1080) == 2 * (24 + 8) * 1920 * 1080
    assert denoise_scratch_bytes(70, 37) == 2 * 24 * 70 * 37
    b = ctypes.c_uint64()
    L = F.rp()
    assert L.rp_denoise_var_scratch_bytes(0, 5, ctypes.byref(b)) == F.RP_EINVAL
    assert L.rp_denoise_var_scratch_bytes(7, 0, ctypes.byref(b)) == F.RP_EINVAL
    assert L.rp_denoise_var_scratch_bytes(7, 5, None) == F.RP_EINVAL
