"""CPU: progressive accumulation's host models (librp_host.so rph_accum_frames and rph_accum_error, loops over
csrc/rp_accum.h -- the header the device kernels compile) against the numpy models of tests/accum_ref.py bit for bit,
their refusals, the agreement of the running variance with the batch variance (rph_batch_variance) on the same
samples, and the quality of the variance-guided filter fed from folded frames against the oracle's 512-spp frame."""
import ctypes
import os
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import accum_ref as A
from conftest import REPO

SEED = 20260117


def _host_fold(frames, n_frames, n_words, stride, mean=None, m2=None, n_prior=0, want_var=True):
    from rtpotato.render import accum_frames_host
    mean = np.full(n_words, A.PAD) if mean is None else np.array(mean)
    m2 = np.full(n_words, A.PAD) if m2 is None else np.array(m2)
    var = np.full(n_words, A.PAD) if want_var else None
    accum_frames_host(frames, n_frames, mean, m2, n_prior=n_prior, var=var, n_words=n_words, stride=stride)
    return mean, m2, var


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("n_words", [1, 2, 3, 127])
@pytest.mark.parametrize("n_frames", [1, 2, 3, 5])
def test_host_model_equals_numpy(n_frames, n_words, pad):
    """mean, m2 and var against the numpy model, stride = n_words and n_words + 5; after one frame the mean is the
    frame bit for bit and m2 is zero; a word that is the same in every frame has m2 == 0 exactly."""
    stride = n_words + pad
    frames = A.synthetic(n_frames, n_words, stride, SEED + 100 * n_frames + n_words)
    mean, m2, var = _host_fold(frames, n_frames, n_words, stride, want_var=n_frames >= 2)
    rm, r2, rv = A.accum_frames(frames, n_frames, n_words, stride)
    assert np.array_equal(mean, rm, equal_nan=True) and np.array_equal(m2, r2, equal_nan=True)
    assert A.same_bits(mean, rm) and A.same_bits(m2, r2)
    if n_frames >= 2:
        assert np.array_equal(var, rv, equal_nan=True) and A.same_bits(var, rv)
    if n_frames == 1:
        assert A.same_bits(mean, frames[:n_words]) and not m2[np.isfinite(frames[:n_words])].any()
    assert mean[0] == 0.7 and m2[0] == 0.0
    if n_words >= 8:  # the +inf word and the NaN word poison their own state and nothing else
        assert np.isnan(m2[5]) and np.isnan(mean[6]) and np.isnan(m2[6])
        assert np.isfinite(np.delete(mean, [5, 6])).all() and np.isfinite(np.delete(m2, [5, 6])).all()
        assert (m2 >= 0.0)[np.isfinite(m2)].all()


@pytest.mark.parametrize("n_words,pad", [(3, 0), (127, 5)])
def test_continuation_is_bit_identical(n_words, pad):
    """Five frames at once against two, then three with n_prior = 2 from the same buffer."""
    stride = n_words + pad
    frames = A.synthetic(5, n_words, stride, SEED + 7)
    whole = _host_fold(frames, 5, n_words, stride)
    mean, m2, _ = _host_fold(frames, 2, n_words, stride)
    part = _host_fold(frames[2 * stride:], 3, n_words, stride, mean=mean, m2=m2, n_prior=2)
    for a, b in zip(whole, part):
        assert A.same_bits(a, b)
    ref = A.accum_frames(frames[2 * stride:], 3, n_words, stride, *A.accum_frames(frames, 2, n_words, stride)[:2], n_prior=2)
    for a, b in zip(part, ref):
        assert A.same_bits(a, b)


@pytest.mark.parametrize("tol,eps", [(0.0, 0.0), (0.2, 1e-2), (1e-3, 1e-9)])
def test_error_model_equals_numpy(tol, eps):
    """rph_accum_error against the numpy model, parameters defaulted (zeros, and NULL) and explicit: counts, the bits of
    the largest finite e2 and the non-finite count, on frames with dark pixels, zero, negative, infinite and NaN
    variances and a NaN mean."""
    from rtpotato import _ffi as F
    from rtpotato.render import accum_error_host, error_stats
    mean, var = A.synthetic_error_frames(70 * 37, SEED + 1)
    got = accum_error_host(mean, var, tol=tol, eps=eps)
    ref = A.accum_error(mean, var, tol or 0.05, eps or 1e-4)
    print("stats", error_stats(got))
    assert got.tolist() == ref.tolist()
    assert got[0] == 70 * 37 and 0 < got[1] < got[0] and got[3] == 3 and got[2] > 0
    if not tol and not eps:
        again = np.zeros(4, dtype=np.uint64)
        assert F.host().rph_accum_error(None, len(mean), mean.ctypes.data, var.ctypes.data, again.ctypes.data) == F.RP_OK
        assert again.tolist() == ref.tolist()
    zeros = accum_error_host(mean, np.zeros_like(var), tol=tol, eps=eps)  # no pixel has an error: nothing over, max 0
    assert zeros.tolist() == A.accum_error(mean, np.zeros_like(var), tol or 0.05, eps or 1e-4).tolist()
    assert zeros[1] == 0 and zeros[2] == 0 and zeros[3] == 1


def test_refusals():
    """Each RP_EINVAL case of rph_accum_frames and rph_accum_error arrives with its message, and nothing is written."""
    from rtpotato import _ffi as F
    H = F.host()
    fr = np.ones(40)
    mean, m2, var = np.full(4, A.PAD), np.full(4, A.PAD), np.full(4, A.PAD)
    p = lambda a: a.ctypes.data if a is not None else None

    def call(n_words=4, n_prior=0, n_frames=3, frames=fr, stride=4, mean_=mean, m2_=m2, var_=var):
        return H.rph_accum_frames(n_words, n_prior, n_frames, p(frames), stride, p(mean_), p(m2_), p(var_))

    for kw, msg in (({"frames": None}, b"non-NULL"), ({"mean_": None}, b"non-NULL"), ({"m2_": None}, b"non-NULL"),
                    ({"n_frames": 0}, b"n_frames is zero"), ({"n_words": 0}, b"n_words is zero"),
                    ({"stride": 3}, b"frame_stride"), ({"n_frames": 1}, b"at least two frames"),
                    ({"n_prior": 2 ** 31 - 3}, b"2^31 - 1"), ({"n_prior": 2 ** 32 - 1}, b"2^31 - 1"),
                    ({"mean_": fr[8:]}, b"alias the frames"), ({"m2_": fr[11:]}, b"alias the frames"),
                    ({"var_": fr[1:]}, b"alias the frames"), ({"m2_": mean}, b"one another"),
                    ({"var_": m2[1:]}, b"one another")):
        assert call(**kw) == F.RP_EINVAL, kw
        assert msg in H.rph_last_error(), (kw, H.rph_last_error())
    assert (fr == 1.0).all() and all((a == A.PAD).all() for a in (mean, m2, var))
    assert call(mean_=fr[12:], frames=fr[:12]) == F.RP_OK  # neighbours in one allocation do not alias
    assert call(n_frames=1, var_=None) == F.RP_OK and call(n_frames=1, n_prior=1) == F.RP_OK
    assert call(n_prior=2 ** 31 - 4) == F.RP_OK  # n = 2^31 - 1
    st = np.zeros(4, dtype=np.uint64)
    m, v = np.ones((2, 3)), np.ones((2, 3))
    assert H.rph_accum_error(None, 2, p(m), p(v), p(st)) == F.RP_OK
    for args in ((None, p(v), p(st)), (p(m), None, p(st)), (p(m), p(v), None)):
        assert H.rph_accum_error(None, 2, *args) == F.RP_EINVAL and b"non-NULL" in H.rph_last_error()
    for tol, eps in ((-0.05, 0.0), (float("nan"), 0.0), (0.0, -1e-4), (0.0, float("nan")), (0.0, float("inf"))):
        e = F.rp_error_params(tol, eps)
        assert H.rph_accum_error(ctypes.byref(e), 2, p(m), p(v), p(st)) == F.RP_EINVAL, (tol, eps)
        assert b"out of range" in H.rph_last_error()


def _host_fold_as(tile, n_words, n_prior, n_frames, frames, stride, mean, m2, var):
    """One set of rph_accum_frames arguments (arrays or None) through rph_accum_frames or (tile) through
    rph_accum_frames_tiles as a one-block list -- n_listed = n_state_tiles = 1, tiles = [0], tile_words = n_words: the
    return code and the message after the `rph_<name>: ` prefix."""
    from rtpotato import _ffi as F
    H = F.host()
    p = lambda a: a.ctypes.data if a is not None else None
    one = np.zeros(1, dtype=np.uint32)
    if tile:
        name = b"rph_accum_frames_tiles: "
        rc = H.rph_accum_frames_tiles(n_words, 1, p(one), 1, n_prior, n_frames, p(frames), stride, p(mean), p(m2), p(var))
    else:
        name = b"rph_accum_frames: "
        rc = H.rph_accum_frames(n_words, n_prior, n_frames, p(frames), stride, p(mean), p(m2), p(var))
    msg = H.rph_last_error() if rc else name
    assert msg.startswith(name) and one[0] == 0, msg
    return rc, msg[len(name):]


def test_plain_fold_is_the_tile_fold_with_one_block():
    """rp_accum.h states the two folds' refusals once (check_fold) and the host folds them with one loop: the table of
    test_refusals, and the state above 2^40 - 512 words, is refused by both with one message -- but for the block of no
    words, where each names its own argument -- and accepted arguments give equal bits."""
    from rtpotato import _ffi as F
    fr = np.ones(40)
    mean, m2, var = np.full(4, A.PAD), np.full(4, A.PAD), np.full(4, A.PAD)
    ok = dict(n_words=4, n_prior=0, n_frames=3, frames=fr, stride=4, mean=mean, m2=m2, var=var)
    for kw, want in (({"frames": None}, b"non-NULL"), ({"mean": None}, b"non-NULL"), ({"m2": None}, b"non-NULL"),
                     ({"n_frames": 0}, b"n_frames is zero"), ({"n_words": 0}, (b"n_words is zero", b"tile_words is zero")),
                     ({"stride": 3}, b"frame_stride is below"), ({"n_frames": 1}, b"at least two frames"),
                     ({"n_prior": 2 ** 31 - 3}, b"2^31 - 1"), ({"n_prior": 2 ** 32 - 1}, b"2^31 - 1"),
                     ({"n_words": 2 ** 40, "stride": 2 ** 40}, b"2^40 - 512"),
                     ({"mean": fr[8:]}, b"alias the frames"), ({"m2": fr[11:]}, b"alias the frames"),
                     ({"var": fr[1:]}, b"alias the frames"), ({"m2": mean}, b"alias one another"),
                     ({"var": m2[1:]}, b"alias one another")):
        (rc_a, msg_a), (rc_b, msg_b) = (_host_fold_as(tile, **{**ok, **kw}) for tile in (False, True))
        assert rc_a == rc_b == F.RP_EINVAL, kw
        if isinstance(want, tuple):
            assert (msg_a, msg_b) == want, kw
        else:
            assert msg_a == msg_b and want in msg_a, (kw, msg_a, msg_b)
    assert (fr == 1.0).all() and all((a == A.PAD).all() for a in (mean, m2, var))
    rng = np.random.default_rng(SEED + 3)
    for n_words in (1, 4, 5):
        for n_prior in (0, 2):
            for n_frames in (1, 5):
                for stride in (n_words, n_words + 3):
                    frames = A.synthetic(n_frames, n_words, stride, SEED + 10 * n_words + n_frames)
                    state = rng.random((2, n_words))  # (read only with n_prior frames behind it)
                    got = []
                    for tile in (False, True):
                        m, q = state[0].copy(), state[1].copy()
                        v = np.full(n_words, A.PAD) if n_prior + n_frames >= 2 else None
                        assert _host_fold_as(tile, n_words, n_prior, n_frames, frames, stride, m, q, v)[0] == F.RP_OK
                        got.append((m, q, v))
                    for a, b in zip(*got):
                        assert (a is None and b is None) or A.same_bits(a, b), (n_words, n_prior, n_frames, stride)


def test_error_params_struct(tmp_path):
    """sizeof and offsets of rp_error_params and RP_ERROR_STATS_LEN against a tiny C program."""
    from rtpotato import _ffi as F
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rp.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %d\\n", sizeof(rp_error_params), offsetof(rp_error_params, tol),\n'
                   '         offsetof(rp_error_params, eps), RP_ERROR_STATS_LEN);\n  return 0;\n}\n')
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = F.rp_error_params
    assert sizes == [ctypes.sizeof(P), P.tol.offset, P.eps.offset, F.RP_ERROR_STATS_LEN] == [16, 0, 8, 4]


def test_variance_agrees_with_batch_variance():
    """Four frames of 4 spp are the four batches of a 16-spp pixel at samples_per_stream = 4: S_b = 4 x frame b (exact).
    The batch variance takes e_b = S_b / 16 - x / 4 against the sum-then-divide mean x, Welford the deviations from its
    running mean; both means carry a few ulps (B 2^-53 m) and so does every deviation, hence the two variances differ by
    about 2 sigma x 1e-15 m: rtol 1e-9 covers every pixel with sigma / m >= 1e-6, atol 1e-12 max(frame)^2 the rest."""
    from rtpotato.render import batch_variance_host
    r = np.random.default_rng(SEED + 2)
    n_words = 3 * 11 * 9
    frames = r.uniform(0.05, 3.0, size=(4, n_words))
    frames[:, :3] = 1.25  # a deterministic pixel: both say zero
    _, _, var = _host_fold(frames.reshape(-1), 4, n_words, n_words)
    sums = np.ascontiguousarray(np.moveaxis(4.0 * frames.reshape(4, -1, 3), 0, 1))  # (pixels, B, 3)
    ref = batch_variance_host(sums, 16, 4).reshape(-1)
    rel = np.abs(var - ref) / np.maximum(ref, 1e-300)
    print("largest relative difference", float(rel[ref > 0].max()), "largest absolute", float(np.abs(var - ref).max()))
    assert (var[:3] == 0.0).all() and (ref[:3] == 0.0).all()
    assert np.allclose(var, ref, rtol=1e-9, atol=1e-12 * float(frames.max()) ** 2)
    assert np.allclose(var, np.var(frames, axis=0, ddof=1) / 4, rtol=1e-9, atol=1e-12 * float(frames.max()) ** 2)


def test_quality_from_folded_frames():
    """The oracle's bunny_full at 96 x 64 as tests/test_denoise_var.py makes it -- four frames of 4 spp, one stream
    each, seeds advancing by W H -- folded with rph_accum_frames; the variance-guided filter on the folded mean and
    variance against the oracle's 512-spp frame.  Mean and variance equal that test's 16 / 4 case to rounding, so the
    bounds are its bounds: below the noisy frame, and below the recorded ratio plus its margin."""
    import denoise_ref as R
    import denoise_var_ref as V
    from parity import oracle_render
    from rtpotato.render import denoise_host
    q = V.quality_case("bunny_full")
    p = q["params"]
    assert (p.spp, p.samples_per_stream) == (16, 4)
    frames = np.stack([oracle_render(q["scene"], replace(p, spp=4, seed=p.seed + b * p.width * p.height))[0]
                       for b in range(4)])
    n_words = frames[0].size
    mean, _, var = _host_fold(frames.reshape(-1), 4, n_words, n_words)
    mean, var = mean.reshape(frames[0].shape), var.reshape(frames[0].shape)
    scale = float(frames.max())
    print("folded mean against the 16-spp frame: max |diff|", float(np.abs(mean - q["noisy"]).max()),
          "variance against the batch variance: max |diff|", float(np.abs(var - q["var"]).max()))
    assert np.allclose(mean, q["noisy"], rtol=1e-12, atol=0.0)
    assert np.allclose(var, q["var"], rtol=1e-9, atol=1e-12 * scale * scale)
    g = {k: q[k] for k in ("normal", "albedo", "depth")}
    out = denoise_host(mean, params=None, variance=var, **g)
    noisy, den = R.mse(mean, q["target"]), R.mse(out, q["target"])
    print(f"bunny_full from folded frames: MSE noisy {noisy:.6g}, variance-guided {den:.6g} (ratio {den / noisy:.4f}; "
          f"recorded {V.MSE_RATIO['bunny_full']})")
    assert np.isfinite(out).all()
    assert den < noisy
    assert den <= V.MSE_CAP["bunny_full"] * noisy
