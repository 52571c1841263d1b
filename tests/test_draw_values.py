"""The doubles the keystream ring holds (raytracing-potato_amd/csrc/rp_draw.h value_store / unit_of, through
rph_draw_values).

For a keystream u64 with k = u64 >> 11 the ring stores v = k 2^-52 - 1 (the samplers' 2 r - 1 with the Standard
r = k 2^-53), and the draws that want r itself take (v + 1) / 2.  Both must be exact: v is a multiple of 2^-52 of
magnitude <= 1, v + 1 = k 2^-52 with k < 2^53, and halving only moves the exponent.  numpy's float64 forms both
references exactly too (k < 2^53 converts exactly, the scalings are by powers of two, and k 2^-52 - 1 is exact for the
same reason), so the comparison is bit for bit, as uint64 views.
"""
import ctypes

import numpy as np

DISK = 4
TAIL = 8  # rp_draw.h TAIL_WORDS

EDGE = np.array([
    0x0000000000000000,  # all zero: k = 0, v = -1, r = 0
    0xFFFFFFFFFFFFFFFF,  # all ones: k = 2^53 - 1
    0x00000000000007FF,  # only the low 11 bits: they are dropped, k = 0
    0xFFFFFFFF00000000,  # lo = 0
    0x00000000FFFFFFFF,  # hi = 0
    0xFFFFFFFFFFFFF800,  # k = 2^53 - 1 with the dropped bits clear
    0x0000000000000800,  # k = 1
    0x0000000000000FFF,  # k = 1 with the dropped bits set
    0x8000000000000000,  # k = 2^52: v = 0, r = 1/2
    0x7FFFFFFFFFFFF800,  # k = 2^52 - 1: the largest negative v
], dtype=np.uint64)


def _host():
    from rtpotato import _ffi as F
    return F, F.host()


def _values(F, H, words):
    stored = np.empty(words.size, dtype=np.float64)
    unit = np.empty(words.size, dtype=np.float64)
    F.check_host(H.rph_draw_values(words.ctypes.data, words.size, stored.ctypes.data, unit.ctypes.data))
    return stored, unit


def _expected(words):
    k = (words >> np.uint64(11)).astype(np.float64)  # k < 2^53: exact
    return k * 2.0 ** -52 - 1.0, k * 2.0 ** -53


def _words():
    gen = np.random.default_rng(27)
    return np.concatenate([EDGE, gen.integers(0, 2 ** 64, size=100_000, dtype=np.uint64)])


def test_stored_and_unit_values_are_exact():
    F, H = _host()
    words = _words()
    stored, unit = _values(F, H, words)
    want_s, want_u = _expected(words)
    assert np.array_equal(stored.view(np.uint64), want_s.view(np.uint64))
    assert np.array_equal(unit.view(np.uint64), want_u.view(np.uint64))
    assert stored.min() == -1.0 and stored.max() == 1.0 - 2.0 ** -52
    assert unit.min() == 0.0 and unit.max() == 1.0 - 2.0 ** -53
    # -1 is the only stored value whose sign bit is set with k = 0; v = 0 is +0
    assert stored[8] == 0.0 and not np.signbit(stored[8])


def test_stored_value_is_what_words_sym_gave():
    """Through rph_draw_round, kind 4 (UnitDisk), on a one-try image (the word under test, every other value 0): the
    try (x, 0) with |x| < 1 is accepted, and the x it returns is the draw's `2 r - 1` -- the double words_sym made from
    the raw words before the ring held values (tests/test_draw_site.py pins that double to the oracle's)."""
    F, H = _host()
    words = _words()[:2000]
    stored, _ = _values(F, H, words)
    zero = np.uint64(1) << np.uint64(63)  # k = 2^52: the stored value 0
    out = (ctypes.c_double * 3)()
    npos, acc = ctypes.c_uint32(), ctypes.c_uint32()
    img = np.zeros(16 * 8 + TAIL, dtype=np.uint32)
    img64 = img.view(np.uint64)
    for i, w in enumerate(words):
        img64[:] = zero
        img64[0] = w
        img64[64] = w  # the mirror tail repeats slot 0's first words
        F.check_host(H.rph_draw_round(DISK, 8, img.ctypes.data, 0, out, ctypes.byref(npos), ctypes.byref(acc)))
        assert acc.value == 1
        if stored[i] == -1.0:  # k = 0: x^2 = 1 is not inside the disk, so the round's second try (0, 0) is taken
            assert npos.value == 8 and out[0] == 0.0 and out[1] == 0.0, (i, hex(int(w)))
            continue
        assert npos.value == 4, (i, hex(int(w)))
        got = np.array([out[0], out[1]], dtype=np.float64).view(np.uint64)
        assert got[0] == stored[i:i + 1].view(np.uint64)[0], (i, hex(int(w)), out[0], stored[i])
        assert out[1] == 0.0 and out[2] == 0.0


def test_draw_values_argument_errors():
    F, H = _host()
    w = np.zeros(1, dtype=np.uint64)
    d = np.zeros(1, dtype=np.float64)
    assert H.rph_draw_values(None, 1, d.ctypes.data, d.ctypes.data) != 0
    assert H.rph_draw_values(w.ctypes.data, 1, None, d.ctypes.data) != 0
    assert H.rph_draw_values(w.ctypes.data, 1, d.ctypes.data, None) != 0
    assert H.rph_draw_values(None, 0, None, None) == 0
