"""The tracker skips the interpolation of a level's patches when the window starts on an integer position (lk.hip,
step 1, IDENT).  That rests on two identities of the integer formulas, checked here on the CPU over every input value
they can meet, so that the claim does not rest on the GPU and its oracle alone:

  template:     (w00 p00 + w01 p01 + w10 p10 + w11 p11 + 2^8) >> 9   == 32 p00      at weights (2^14, 0, 0, 0)
  derivatives:  the tile holds 4 d as int16;  (2^14 4d + 4 2^13) >> 16 == d  and the identity path's own form,
                the int16 (4 d) >> 2 (arithmetic), is d as well

and on the weights at fractions (0, 0) being exactly (2^14, 0, 0, 0) in float32 arithmetic."""
import numpy as np

W_BITS = 14


def _weights(a, b):
    """bilinear_weights of lk.hip / the oracle, in float32."""
    a, b, one, s = np.float32(a), np.float32(b), np.float32(1), np.float32(1 << W_BITS)
    w00 = int(np.rint((one - a) * (one - b) * s))
    w01 = int(np.rint(a * (one - b) * s))
    w10 = int(np.rint((one - a) * b * s))
    return w00, w01, w10, (1 << W_BITS) - w00 - w01 - w10


def test_weights_at_an_integer_position_select_one_pixel():
    assert _weights(0.0, 0.0) == (1 << W_BITS, 0, 0, 0)
    assert _weights(-0.0, 0.0) == (1 << W_BITS, 0, 0, 0)
    # the smallest fractions a level can see next to 0 do NOT take the identity path (the kernel tests == 0), and need not
    assert _weights(2.0 ** -20, 0.0)[0] == 1 << W_BITS


def test_template_identity_for_every_pixel_value_and_any_neighbours():
    w00, w01, w10, w11 = _weights(0.0, 0.0)
    p = np.arange(256, dtype=np.int64)
    rng = np.random.default_rng(5)
    for _ in range(16):
        p01, p10, p11 = (rng.integers(0, 256, 256) for _ in range(3))
        s = w00 * p + w01 * p01 + w10 * p10 + w11 * p11 + (1 << (W_BITS - 5 - 1))
        assert np.array_equal(s >> (W_BITS - 5), 32 * p)
    # the packed form: two bytes spread over the halves of a dword, ONE 32-bit shift by 5 scales both
    lo, hi = np.meshgrid(p, p)
    packed = ((lo | (hi << 16)) << 5) & 0xFFFFFFFF
    assert np.array_equal(packed & 0xFFFF, 32 * lo) and np.array_equal(packed >> 16, 32 * hi)


def test_derivative_identity_for_every_tile_value():
    # Scharr of 8-bit pixels: |d| <= (3 + 10 + 3) * 255 = 4080, the tile holds 4 d
    d = np.arange(-4080, 4081, dtype=np.int64)
    w00 = _weights(0.0, 0.0)[0]
    generic = (w00 * (4 * d) + (4 << (W_BITS - 1))) >> 16
    assert np.array_equal(generic, d)
    as_int16 = (4 * d).astype(np.int16)
    assert np.array_equal((as_int16 >> 2).astype(np.int64), d)  # v_pk_ashrrev_i16 by 2 on the tile's halves


def test_identity_patch_equals_interpolated_patch_on_a_random_tile():
    """One whole 21 x 21 x C window both ways, pixel tile and derivative tile random."""
    rng = np.random.default_rng(9)
    w00, w01, w10, w11 = _weights(0.0, 0.0)
    for c in (1, 3):
        img = rng.integers(0, 256, (22, 22 * c)).astype(np.int64)
        d4 = 4 * rng.integers(-4080, 4081, (22, 22 * c)).astype(np.int64)
        n = 21 * c
        tmpl = (w00 * img[:21, :n] + w01 * img[:21, c:n + c] + w10 * img[1:, :n] + w11 * img[1:, c:n + c] + 256) >> 9
        der = (w00 * d4[:21, :n] + w01 * d4[:21, c:n + c] + w10 * d4[1:, :n] + w11 * d4[1:, c:n + c] + (4 << 13)) >> 16
        assert np.array_equal(tmpl, img[:21, :n] << 5)
        assert np.array_equal(der, d4[:21, :n] >> 2)
