"""CPU-only: the NumPy restatement of the elastic deformation (tests/elastic_np.py) against scipy.ndimage, and by hand.
  field         : gaussian_filter(mode='constant', truncate=4) within alpha * 1e-6 (the float32 rounding of the taps);
  warp_nearest  : EQUAL to map_coordinates(order=0, mode='nearest') at the quantised coordinates q / 256;
  warp_bilinear : within 0.5 + 1e-6 of map_coordinates(order=1, mode='nearest') at the same coordinates (the rounding of
                  the result to an integer; the weights are exact at multiples of 1/256)."""
import os
import sys

import numpy as np
import pytest

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import elastic_np as E   # noqa: E402

SHAPES = [((1, 4, 4), 2.0), ((1, 8, 12), 0.6), ((2, 72, 136), 4.0), ((2, 64, 64), 16.0)]


def _noise(shape, seed):
    return np.random.default_rng(seed).uniform(-1, 1, shape + (2,)).astype(np.float32)


@pytest.mark.parametrize("shape,sigma", SHAPES)
def test_field_equals_scipy_gaussian_filter(shape, sigma):
    from scipy.ndimage import gaussian_filter
    noise = _noise(shape, 3)
    tap, radius = E.taps(sigma)
    assert radius == int(4.0 * sigma + 0.5) and len(tap) == 2 * radius + 1 and tap.dtype == np.float32
    alpha = np.linspace(20.0, 50.0, shape[0])
    got = E.field(noise, alpha, tap)
    for b in range(shape[0]):
        for k in range(2):
            want = alpha[b] * gaussian_filter(noise[b, :, :, k].astype(np.float64), sigma, mode='constant', cval=0.0, truncate=4.0)
            assert np.abs(got[b, :, :, k] - want).max() <= alpha[b] * 1e-6, (b, k)
    assert np.array_equal(E.field(noise, 0.0, tap), np.zeros(shape + (2,)))


def test_radius_zero_is_alpha_times_noise():
    noise = _noise((2, 5, 7), 4)
    tap, radius = E.taps(0.1)
    assert radius == 0 and tap.tolist() == [1.0]
    assert np.array_equal(E.field(noise, [2.0, 3.0], tap), noise.astype(np.float64) * np.array([2.0, 3.0])[:, None, None, None])


@pytest.mark.parametrize("shape,sigma", SHAPES)
@pytest.mark.parametrize("c", [1, 3])
def test_warp_equals_scipy_map_coordinates_at_the_quantised_coordinates(shape, sigma, c):
    from scipy.ndimage import map_coordinates
    n, h, w = shape
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, shape + (c,), dtype=np.uint8)
    tap, _ = E.taps(sigma)
    disp = E.field(_noise(shape, 6), 400.0, tap).astype(np.float32)      # large enough to leave the image at the sides
    qx, qy = E.quant(disp)
    near, bil = E.warp_nearest(src, disp), E.warp_bilinear(src, disp)
    assert near.shape == src.shape and bil.shape == src.shape and bil.dtype == np.uint8
    for b in range(n):
        coords = np.stack([qy[b] / 256.0, qx[b] / 256.0])
        for k in range(c):
            plane = src[b, :, :, k].astype(np.float64)
            assert np.array_equal(near[b, :, :, k], map_coordinates(plane, coords, order=0, mode='nearest'))
            want = map_coordinates(plane, coords, order=1, mode='nearest')
            assert np.abs(bil[b, :, :, k] - want).max() <= 0.5 + 1e-6


def _const(shape, dx, dy):
    d = np.empty(shape + (2,), np.float32)
    d[..., 0], d[..., 1] = dx, dy
    return d


def test_zero_field_is_the_identity_and_a_constant_field_is_the_clamped_shift():
    rng = np.random.default_rng(7)
    for c in (None, 3):
        src = rng.integers(0, 256, (2, 9, 11) + (() if c is None else (c,)), dtype=np.uint8)
        zero = _const((2, 9, 11), 0.0, 0.0)
        assert np.array_equal(E.warp_nearest(src, zero), src) and np.array_equal(E.warp_bilinear(src, zero), src)
        ys, xs = np.clip(np.arange(9) - 2, 0, 8), np.clip(np.arange(11) + 3, 0, 10)
        want = src[:, ys][:, :, xs]
        shift = _const((2, 9, 11), 3.0, -2.0)
        assert np.array_equal(E.warp_nearest(src, shift), want) and np.array_equal(E.warp_bilinear(src, shift), want)


def test_ties_round_as_specified():
    # the quantisation rounds half to even in 1/256 pixel
    d = np.array([128.5, 129.5, -128.5, -129.5, 0.5, -0.5], np.float32) / np.float32(256)
    disp = np.zeros((1, 1, 6, 2), np.float32)
    disp[0, 0, :, 0] = d
    qx, _ = E.quant(disp)
    assert (qx[0, 0] - np.arange(6) * 256).tolist() == [128, 130, -128, -130, 0, 0]
    # nearest at +-0.5 and +-1.5: (q + 128) >> 8 is floor(pos + 0.5)
    src = np.arange(10, 110, 10, dtype=np.uint8).reshape(1, 1, 10)
    x = np.arange(10)
    for dx, off in ((0.5, 1), (-0.5, 0), (1.5, 2), (-1.5, -1)):
        got = E.warp_nearest(src, _const((1, 1, 10), dx, 0.0))
        assert np.array_equal(got[0, 0], src[0, 0, np.clip(x + off, 0, 9)]), dx
    # bilinear at a half: (a + b + 1) >> 1 of the two neighbours
    srcb = np.array([[[0, 1, 4, 9, 200, 255, 3, 3, 100, 7]]], np.uint8)
    for dx, lo in ((0.5, 0), (-0.5, -1), (1.5, 1), (-1.5, -2)):
        a = srcb[0, 0, np.clip(x + lo, 0, 9)].astype(int)
        b = srcb[0, 0, np.clip(x + lo + 1, 0, 9)].astype(int)
        got = E.warp_bilinear(srcb, _const((1, 1, 10), dx, 0.0))
        assert np.array_equal(got[0, 0], (a + b + 1) >> 1), dx
    # the same along y
    got = E.warp_nearest(src.reshape(1, 10, 1), _const((1, 10, 1), 0.0, 1.5))
    assert np.array_equal(got[0, :, 0], src[0, 0, np.clip(x + 2, 0, 9)])


def test_nan_inf_and_huge_displacements():
    rng = np.random.default_rng(8)
    src = rng.integers(0, 256, (1, 6, 7, 3), dtype=np.uint8)
    for mode in (E.warp_nearest, E.warp_bilinear):
        assert np.array_equal(mode(src, _const((1, 6, 7), np.nan, np.nan)), src)            # NaN is no displacement
        for big in (np.inf, 1e9, 16384.0):
            got = mode(src, _const((1, 6, 7), big, -big))                                   # the top right corner
            assert np.array_equal(got, np.broadcast_to(src[:, :1, -1:], src.shape))
            got = mode(src, _const((1, 6, 7), -big, big))                                   # the bottom left corner
            assert np.array_equal(got, np.broadcast_to(src[:, -1:, :1], src.shape))
        got = mode(src, _const((1, 6, 7), np.nan, -np.inf))                                 # the first row, column by column
        assert np.array_equal(got, np.broadcast_to(src[:, :1], src.shape))


def test_compaction_rule():
    planes = np.zeros((4, 5, 6), np.uint8)
    planes[0, 0, 0] = planes[1, 1, 2] = planes[2, 2, 3] = 1                                 # planes 0, 2, 3 of 4 real ones
    out, k = E.compact(planes, 4)
    assert k == 3 and np.array_equal(out[:, :, :3], planes[:, :, [0, 2, 3]]) and not out[:, :, 3:].any()
    same, k = E.compact(planes[:, :, [0, 2, 3, 1]], 3)
    assert k == 3 and np.array_equal(same, planes[:, :, [0, 2, 3, 1]])                      # nothing dropped: untouched
    assert E.compact(np.zeros((4, 5, 6), np.uint8), 2) is None
