"""CPU: the guided denoiser's host model (librp_host.so rph_denoise, a loop over csrc/rp_denoise.h -- the header the
device kernel compiles) against the numpy model of tests/denoise_ref.py bit for bit, its pass-through and constant
properties, its quality against the oracle's 512-spp frames, and the ABI's host-only parts."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as R
from conftest import REPO

SEED = 20260113


def _host(frame_rgb, guides, params):
    from rtpotato.render import denoise_host
    return denoise_host(frame_rgb, params=params, **guides)


@pytest.mark.parametrize("variant", list(R.VARIANTS))
@pytest.mark.parametrize("width,height", [(70, 37), (7, 5)])
def test_host_model_equals_numpy(width, height, variant):
    """L = 5 (steps 1 .. 16: on 7 x 5 most taps leave the frame), a quarter of the pixels misses in blocks, some depths
    zero; every guide NULL in turn, the colour term disabled, normal_power 1 and 8."""
    frame, guides, params, ref = R.reference(width, height, SEED, variant, 5)
    out = _host(frame["rgb"], guides, params)
    assert np.isfinite(ref).all()
    diff = np.abs(out - ref)
    print(variant, width, height, "max |host - numpy|", float(diff.max()), "pixels differing", int((diff > 0).any(-1).sum()))
    assert np.array_equal(out, ref)


def test_pass_through_and_constant():
    """Pixels with nn == 0 return rgb bit for bit (every variant that has a normal guide); a frame whose demodulated
    colour is one constant comes back within 1e-12."""
    frame = R.random_frame(70, 37, SEED)
    miss = frame["miss"]
    assert 0.1 < miss.mean() < 0.5
    for variant in ("defaults", "no_albedo", "no_depth", "no_color"):
        guides, params = R.variant_inputs(frame, variant, 5)
        out = _host(frame["rgb"], guides, params)
        assert np.array_equal(out[miss], frame["rgb"][miss]), variant
        assert not np.array_equal(out[~miss], frame["rgb"][~miss]), variant
    eps = R.DEFAULTS["albedo_eps"]
    rgb = np.where(miss[..., None], frame["rgb"], 0.75 * (frame["albedo"] + eps))
    out = _host(rgb, {k: frame[k] for k in ("normal", "albedo", "depth")}, {"iterations": 5})
    err = np.abs(out - rgb) / np.maximum(1.0, np.abs(rgb))
    print("constant demodulated colour: max relative error", float(err.max()))
    assert err.max() <= 1e-12


@pytest.mark.parametrize("name,params", [("variants_sky", {}), ("variants", {"sigma_color": -1.0})])
def test_quality_against_oracle(name, params):
    """The oracle's 4-spp frame with the oracle's guides, against the oracle at 512 spp and another seed:
    MSE(denoised) <= 0.6 MSE(noisy) (a numpy prototype of this formula measured 0.415 and 0.435; the cap leaves room
    for the target's own noise)."""
    q = R.quality_case(name)
    out = _host(q["noisy"], {k: q[k] for k in ("normal", "albedo", "depth")}, params)
    noisy, den = R.mse(q["noisy"], q["target"]), R.mse(out, q["target"])
    print(f"{name}: MSE noisy {noisy:.6g}, denoised {den:.6g}, ratio {den / noisy:.4f}")
    assert np.isfinite(out).all()
    assert den <= R.MSE_CAP * noisy


def test_params_struct_and_defaults(tmp_path):
    """sizeof(rp_denoise_params) against a tiny C program; rp_denoise_params_init's documented defaults."""
    from rtpotato import _ffi as F
    from rtpotato.render import denoise_defaults
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rp.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu\\n", sizeof(rp_denoise_params), offsetof(rp_denoise_params, sigma_depth),\n'
                   '         offsetof(rp_denoise_params, albedo_eps));\n  return 0;\n}\n')
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = F.rp_denoise_params
    assert sizes == [ctypes.sizeof(P), P.sigma_depth.offset, P.albedo_eps.offset] == [40, 8, 32]
    d = denoise_defaults()
    assert (d.iterations, d.normal_power, d.sigma_depth, d.sigma_albedo, d.sigma_color, d.albedo_eps) == \
        (3, 6, 0.05, 0.1, 1.0, 1e-2)
    assert {k: getattr(d, k) for k in R.DEFAULTS} == R.DEFAULTS
    assert F.rp().rp_denoise_params_init(None) == F.RP_EINVAL
    # a zero-initialised struct and NULL mean the defaults
    frame = R.random_frame(7, 5, SEED)
    g = {k: frame[k] for k in ("normal", "albedo", "depth")}
    assert np.array_equal(_host(frame["rgb"], g, None), _host(frame["rgb"], g, d))
    assert np.array_equal(_host(frame["rgb"], g, F.rp_denoise_params()), _host(frame["rgb"], g, d))


def test_host_refusals():
    """rph_denoise: RP_EINVAL for NULL rgb or out, a zero size, out aliasing an input, parameters out of range."""
    from rtpotato import _ffi as F
    H = F.host()
    frame = R.random_frame(7, 5, SEED)
    rgb, nrm = np.array(frame["rgb"]), np.array(frame["normal"])
    out = np.empty_like(rgb)

    def call(p=None, w=7, h=5, rgb_=rgb, normal=nrm, out_=out):
        ptr = lambda a: a.ctypes.data if a is not None else None
        return H.rph_denoise(ctypes.byref(p) if p is not None else None, w, h, ptr(rgb_), ptr(normal), None, None, ptr(out_))

    assert call() == F.RP_OK
    assert call(rgb_=None) == F.RP_EINVAL and call(out_=None) == F.RP_EINVAL
    assert call(w=0) == F.RP_EINVAL and call(h=0) == F.RP_EINVAL
    assert call(out_=rgb) == F.RP_EINVAL and call(out_=nrm) == F.RP_EINVAL
    assert b"alias" in H.rph_last_error()
    assert call(out_=rgb.reshape(-1)[3:]) == F.RP_EINVAL  # a partial overlap
    for bad in ({"iterations": 9}, {"normal_power": 9}, {"sigma_depth": -1.0}, {"sigma_albedo": -0.5},
                {"albedo_eps": -1e-2}, {"sigma_color": float("nan")}, {"sigma_depth": float("inf")}):
        p = F.rp_denoise_params(**bad)
        assert call(p) == F.RP_EINVAL, bad
    for good in ({"iterations": 8}, {"normal_power": 8}, {"iterations": 1, "normal_power": 1}, {"sigma_color": -1.0}):
        assert call(F.rp_denoise_params(**good)) == F.RP_OK, good


def test_scratch_bytes_without_gpu():
    """rp_denoise_scratch_bytes is host only: two colour buffers of 3 doubles per pixel; zero sizes are refused."""
    from rtpotato import _ffi as F
    from rtpotato.render import denoise_scratch_bytes
    assert denoise_scratch_bytes(70, 37) == 2 * 24 * 70 * 37
    assert denoise_scratch_bytes(1920, 1080) == 2 * 24 * 1920 * 1080
    b = ctypes.c_uint64()
    L = F.rp()
    assert L.rp_denoise_scratch_bytes(0, 5, ctypes.byref(b)) == F.RP_EINVAL
    assert L.rp_denoise_scratch_bytes(7, 0, ctypes.byref(b)) == F.RP_EINVAL
    assert L.rp_denoise_scratch_bytes(7, 5, None) == F.RP_EINVAL
