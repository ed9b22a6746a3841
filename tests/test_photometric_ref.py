"""CPU-only: tests/photometric_np.py - what the device kernels of the five photometric augmentations are held against -
reproduces the installed Pillow byte for byte: Image.blend behind ImageEnhance.Brightness / Contrast / Color, convert('L'),
the RGB -> HSV -> shift -> RGB path of torchvision's PIL adjust_hue over all 2^24 colours, Image.point over a float
table, Image.resize(LANCZOS) and the integer form of Contrast's mean."""
import os
import sys

import numpy as np
import pytest
from PIL import Image, ImageEnhance, ImageStat

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import photometric_np as P   # noqa: E402

FACTORS = [0.6, 0.61, 0.65, 0.7, 0.73, 0.8, 0.85, 0.9, 0.95, 0.999, 1.0, 1.001, 1.05, 1.1, 1.15, 1.2, 1.27, 1.3, 1.35,
           1.39, 1.4]
SHAPES = [(37, 53), (100, 75), (64, 48)]
RATIOS = np.arange(0.7, 1.3, 0.05)


def _all_colours():
    i = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def test_blend_every_byte_against_black_mean_and_luma():
    """A 256 x 256 image whose channels run over every (x, other) byte pair: Brightness blends with 0, Contrast with
    the image's rounded mean luma, Color with each pixel's luma."""
    x, y = np.meshgrid(np.arange(256), np.arange(256))
    img = np.stack([x, y, (x * 7 + y * 3) & 255], -1).astype(np.uint8)
    pil = Image.fromarray(img)
    mean = P.contrast_mean(P.luma(img))
    for f in FACTORS:
        assert np.array_equal(P.blend(img, 0, f), np.asarray(ImageEnhance.Brightness(pil).enhance(f))), f
        assert np.array_equal(P.blend(img, mean, f), np.asarray(ImageEnhance.Contrast(pil).enhance(f))), f
        assert np.array_equal(P.blend(img, P.luma(img)[..., None], f), np.asarray(ImageEnhance.Color(pil).enhance(f))), f
        for d in (0, 1, 127, 128, 254, 255):                      # every byte against a constant degenerate
            deg = Image.new('RGB', pil.size, (d, d, d))
            assert np.array_equal(P.blend(img, d, f), np.asarray(Image.blend(deg, pil, f))), (f, d)


def test_luma_over_a_colour_lattice_and_random_pixels():
    rs = np.random.RandomState(0)
    v = np.array(list(range(0, 256, 5)) + [254, 255], np.uint8)
    lattice = np.stack(np.meshgrid(v, v, v, indexing='ij'), -1).reshape(-1, 54, 3)
    for img in (lattice, rs.randint(0, 256, (211, 157, 3)).astype(np.uint8)):
        assert np.array_equal(P.luma(img), np.asarray(Image.fromarray(img).convert('L')))


def test_contrast_mean_in_integers_equals_imagestat():
    rs = np.random.RandomState(1)
    cases = [rs.randint(0, 256, (37, 53)), rs.randint(200, 256, (64, 48)), np.full((5, 7), 255), np.zeros((3, 3)),
             np.array([[0, 1]]), np.array([[1, 2, 2, 1]]), np.array([[254, 255]] * 3), rs.randint(0, 2, (530, 500))]
    for c in cases:
        g = c.astype(np.uint8)
        assert P.contrast_mean(g) == int(ImageStat.Stat(Image.fromarray(g)).mean[0] + 0.5), g.shape


def test_hue_path_over_all_colours():
    """RGB -> HSV, H += shift (mod 256), -> RGB for two shifts, one from a negative factor."""
    rgb = _all_colours()
    pil_hsv = Image.fromarray(rgb).convert('HSV')
    hsv = P.rgb_to_hsv(rgb)
    assert np.array_equal(hsv, np.asarray(pil_hsv))
    for factor in (0.13, -0.17):
        shift = P.hue_shift_byte(factor)
        assert 0 <= shift < 256 and (factor > 0 or shift > 127)
        h, s, v = pil_hsv.split()
        np_h = np.array(h, dtype=np.uint8)
        with np.errstate(over='ignore'):
            np_h += np.uint8(shift)
        want = np.asarray(Image.merge('HSV', (Image.fromarray(np_h, 'L'), s, v)).convert('RGB'))
        moved = hsv.copy()
        moved[..., 0] = (hsv[..., 0].astype(np.int32) + shift) & 255
        assert np.array_equal(P.hsv_to_rgb(moved), want), factor
    small = rgb[::61, ::67]
    assert np.array_equal(P.shift_hue(small, 33), np.asarray(P.pil_adjust_hue(Image.fromarray(small), 33 / 255.0 + 1e-9)))


def test_hsv_to_rgb_over_all_triples():
    hsv = _all_colours()
    assert np.array_equal(P.hsv_to_rgb(hsv), np.asarray(Image.fromarray(hsv, 'HSV').convert('RGB')))


def test_gamma_lut_is_rounded_not_truncated():
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16)
    img = Image.fromarray(np.stack([ramp, ramp[::-1], ramp.T], -1))
    differs = False
    for g in (0.7, 0.8123, 1.0, 1.05, 1.2999, 0.7 + 0.6 * 0.417022004702574):
        table = [255 * 1 * pow(e / 255., g) for e in range(256)]
        want = np.asarray(img.point(table * 3))
        lut = P.gamma_lut(g)
        assert np.array_equal(lut[np.asarray(img)], want), g
        differs |= bool((lut != np.array([int(t) for t in table], np.uint8)).any())
    assert differs


@pytest.mark.parametrize("h,w", SHAPES)
def test_lanczos_there_and_back_at_the_thirteen_ratios(h, w):
    assert len(RATIOS) == 13 and RATIOS[-1] == 1.3000000000000005
    rs = np.random.RandomState(h)
    a = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    pil = Image.fromarray(a)
    for ratio in RATIOS:
        nh, nw = P.degraded_size(h, w, ratio)
        there = pil.resize((nw, nh), Image.LANCZOS)
        assert np.array_equal(P.resize_lanczos(a, nh, nw), np.asarray(there)), ratio
        back = there.resize((w, h), Image.LANCZOS)
        assert np.array_equal(P.resolution_degrade(a, ratio), np.asarray(back)), ratio


def test_lanczos_single_axis_and_one_channel():
    rs = np.random.RandomState(5)
    a = rs.randint(0, 256, (40, 31, 3)).astype(np.uint8)
    for h, w in ((40, 19), (57, 31), (40, 31), (1, 1)):
        assert np.array_equal(P.resize_lanczos(a, h, w), np.asarray(Image.fromarray(a).resize((w, h), Image.LANCZOS))), (h, w)
    g = a[..., :1]
    assert np.array_equal(P.resize_lanczos(g, 23, 50)[..., 0], np.asarray(Image.fromarray(g[..., 0]).resize((50, 23), Image.LANCZOS)))


def test_run_program_equals_the_pil_sequence():
    """The whole chain as the reference strings it together: ImageEnhance in a drawn order, the hue shift, point,
    channel indexing, convert('L')."""
    rs = np.random.RandomState(3)
    a = rs.randint(0, 256, (37, 53, 3)).astype(np.uint8)
    ops = [("saturation", 1.31), ("hue", -0.11), ("contrast", 0.77), ("brightness", 1.22)]
    for k in range(4):
        order = ops[k:] + ops[:k]
        for gamma, chan, gray in ((0.91, (2, 2, 0), True), (None, None, False), (1.21, (1, 0, 2), False)):
            want = np.asarray(P.pil_photometric(Image.fromarray(a), order, gamma, chan, gray))
            got = P.run_program(a, order, None if gamma is None else P.gamma_lut(gamma), chan or (0, 1, 2), gray)
            assert np.array_equal(got, want), (k, gamma)
