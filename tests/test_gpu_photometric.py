"""isa_photometric_u8 (colour jitter, gamma, channel swap, grayscale in one pass) and isa_resize_lanczos_u8 on the device,
byte for byte against tests/photometric_np.py (pinned against the installed Pillow by tests/test_photometric_ref.py) or
against Pillow itself.  An image of 37 x 53 has 5883 bytes, no multiple of 16: with n = 2 the second image starts off a
16-byte boundary and has a scalar head, and both have tails behind their 48-byte chunks.  One of 64 x 48 has 9216 bytes,
192 whole chunks; test_in_place_and_unaligned_buffers moves both shapes to odd addresses."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import photometric_np as P   # noqa: E402

SMALL = [(37, 53), (64, 48)]
RATIOS = np.arange(0.7, 1.3, 0.05)


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import isa_amd  # noqa: F401
    from isa_amd import data as D
    return D


def _images(h, w, seed, n=2, lo=0):
    return np.random.RandomState(seed).randint(lo, 256, (n, h, w, 3)).astype(np.uint8)


def _want(imgs, specs):
    return np.stack([P.run_program(a, s.get("ops", ()), s.get("lut"), s.get("chan", (0, 1, 2)), s.get("gray", False))
                     for a, s in zip(imgs, specs)])


def _got(D, imgs, specs, **kw):
    return D.photometric(torch.from_numpy(imgs), [D.photo_program(**s) for s in specs], **kw).cpu().numpy()


STAGES = {
    "brightness": [dict(ops=[("brightness", 0.6)]), dict(ops=[("brightness", 1.4)])],
    "contrast": [dict(ops=[("contrast", 0.73)]), dict(ops=[("contrast", 1.27)])],
    "saturation": [dict(ops=[("saturation", 1.4)]), dict(ops=[("saturation", 0.6)])],
    "hue": [dict(ops=[("hue", 0.13)]), dict(ops=[("hue", -0.17)])],
    "gamma": [dict(lut=P.gamma_lut(0.7).tolist()), dict(lut=P.gamma_lut(1.2999).tolist())],
    "channels": [dict(chan=(2, 0, 1)), dict(chan=(1, 1, 1))],
    "gray": [dict(gray=True), dict()],
    "unit_factors": [dict(ops=[("brightness", 1.0), ("contrast", 1.0), ("saturation", 1.0), ("hue", 0.0)]), dict()],
}


@pytest.mark.parametrize("h,w", SMALL)
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_each_stage_alone(stage, h, w):
    D = need_gpu()
    imgs = _images(h, w, h + len(stage))
    got = _got(D, imgs, STAGES[stage])
    assert np.array_equal(got, _want(imgs, STAGES[stage])), stage
    if stage == "unit_factors":                                  # the empty program is the identity
        assert np.array_equal(got[1], imgs[1])


JITTER = [("brightness", 1.22), ("saturation", 1.31), ("hue", -0.11)]


@pytest.mark.parametrize("h,w", SMALL)
@pytest.mark.parametrize("position", [0, 1, 2, 3])
def test_jitter_orders_with_contrast_at_every_position(position, h, w):
    """Contrast's mean is taken from the image as it stands after the ops before it: first, second, third and last."""
    D = need_gpu()
    imgs = _images(h, w, 10 * position + h)
    specs = []
    for b in range(2):
        others = JITTER[b:] + JITTER[:b]                           # another order of the rest per image
        specs.append(dict(ops=others[:position] + [("contrast", (0.77, 1.36)[b])] + others[position:]))
    assert np.array_equal(_got(D, imgs, specs), _want(imgs, specs))


def test_whole_program_530x500():
    D = need_gpu()
    imgs = _images(530, 500, 5)
    specs = [dict(ops=[("saturation", 0.64), ("brightness", 1.4), ("contrast", 1.19), ("hue", 0.2)], lut=P.gamma_lut(0.83).tolist(),
                  chan=(1, 2, 0), gray=False),
             dict(ops=[("hue", -0.2), ("contrast", 0.6), ("brightness", 0.71), ("saturation", 1.4)], lut=P.gamma_lut(1.27).tolist(),
                  chan=(0, 0, 2), gray=True)]
    assert np.array_equal(_got(D, imgs, specs), _want(imgs, specs))


def test_contrast_mean_comes_from_the_brightened_clipped_image():
    D = need_gpu()
    imgs = _images(37, 53, 21, lo=150)                              # bright: x 1.4 clips most of it at 255
    specs = [dict(ops=[("brightness", 1.4), ("contrast", 0.7)])] * 2
    want = _want(imgs, specs)
    for b in range(2):
        bright = P.blend(imgs[b], 0, 1.4)
        m_src, m_now = P.contrast_mean(P.luma(imgs[b])), P.contrast_mean(P.luma(bright))
        assert m_src != m_now
        assert np.array_equal(want[b], P.blend(bright, m_now, 0.7))
        assert not np.array_equal(want[b], P.blend(bright, m_src, 0.7))       # the source's mean gives another image
        assert np.array_equal(want[b], np.asarray(P.pil_photometric(Image.fromarray(imgs[b]), specs[b]["ops"])))
    assert np.array_equal(_got(D, imgs, specs), want)


def test_hue_over_all_colours():
    """The 4096 x 4096 image of all 2^24 colours, twice in one call with two shifts, one from a negative factor."""
    D = need_gpu()
    i = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    factors = (0.13, -0.17)
    got = D.photometric(torch.from_numpy(rgb)[None].expand(2, -1, -1, -1).contiguous(),
                        [D.photo_program([("hue", f)]) for f in factors]).cpu().numpy()
    pil = Image.fromarray(rgb)
    for b, f in enumerate(factors):
        want = np.asarray(P.pil_adjust_hue(pil, f))
        assert np.array_equal(got[b], want), (f, int((got[b] != want).any(-1).sum()))


@pytest.mark.parametrize("h,w", SMALL)
def test_lut_duplicate_channels_and_gray_together(h, w):
    D = need_gpu()
    imgs = _images(h, w, 33)
    specs = [dict(lut=P.gamma_lut(0.9).tolist(), chan=(2, 2, 0), gray=True), dict(lut=P.gamma_lut(1.1).tolist(), chan=(2, 2, 0))]
    got = _got(D, imgs, specs)
    assert np.array_equal(got, _want(imgs, specs))
    assert np.array_equal(got[0], np.asarray(P.pil_photometric(Image.fromarray(imgs[0]), (), 0.9, (2, 2, 0), True)))


@pytest.mark.parametrize("h,w", SMALL)
def test_in_place_and_unaligned_buffers(h, w):
    """src == dst; a source and destination that share an odd offset (vector chunks behind a head in image 0 too); and a
    destination whose offset differs from the source's mod 16 (every pixel one per lane)."""
    D = need_gpu()
    imgs = _images(h, w, 44)
    specs = [dict(ops=[("contrast", 1.3), ("hue", 0.07)], gray=True), dict(ops=[("saturation", 0.8), ("contrast", 0.9)], chan=(1, 0, 0))]
    want = _want(imgs, specs)
    t = torch.from_numpy(imgs).cuda()
    out = D.photometric(t, [D.photo_program(**s) for s in specs], out=t)
    assert out.data_ptr() == t.data_ptr() and np.array_equal(t.cpu().numpy(), want)
    size = imgs.size
    for src_off, dst_off in ((5, 21), (0, 7), (3, 3)):
        a = torch.zeros(size + 64, dtype=torch.uint8, device="cuda")
        b = torch.full((size + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        src = a[src_off:src_off + size].view(imgs.shape)
        src.copy_(torch.from_numpy(imgs))
        dst = b[dst_off:dst_off + size].view(imgs.shape)
        D.photometric(src, [D.photo_program(**s) for s in specs], out=dst)
        assert np.array_equal(dst.cpu().numpy(), want), (src_off, dst_off)
        guard = b.cpu().numpy()
        assert (guard[:dst_off] == 0xAB).all() and (guard[dst_off + size:] == 0xAB).all()     # nothing written outside


@pytest.mark.parametrize("h,w", [(37, 53), (100, 75), (530, 500)])
def test_lanczos_there_and_back(h, w):
    D = need_gpu()
    imgs = _images(h, w, w)
    for ratio in (RATIOS[0], RATIOS[6], RATIOS[11], RATIOS[12]):
        nh, nw = P.degraded_size(h, w, ratio)
        there = D.resize_lanczos(torch.from_numpy(imgs), (nh, nw))
        back = D.resolution_degrade(torch.from_numpy(imgs), ratio)
        assert tuple(there.shape) == (2, nh, nw, 3) and tuple(back.shape) == imgs.shape
        for b in range(2):
            pil = Image.fromarray(imgs[b]).resize((nw, nh), Image.LANCZOS)
            assert np.array_equal(there[b].cpu().numpy(), np.asarray(pil)), (ratio, b)
            assert np.array_equal(back[b].cpu().numpy(), np.asarray(pil.resize((w, h), Image.LANCZOS))), (ratio, b)
            assert np.array_equal(back[b].cpu().numpy(), np.asarray(P.pil_resolution(Image.fromarray(imgs[b]), ratio)))


def test_lanczos_single_axis_and_channel_counts():
    D = need_gpu()
    rs = np.random.RandomState(8)
    a = rs.randint(0, 256, (1, 40, 31, 3)).astype(np.uint8)
    for h, w in ((40, 19), (57, 31), (40, 31)):
        got = D.resize_lanczos(torch.from_numpy(a), (h, w))[0].cpu().numpy()
        assert np.array_equal(got, np.asarray(Image.fromarray(a[0]).resize((w, h), Image.LANCZOS))), (h, w)
    g = rs.randint(0, 256, (3, 45, 38, 1)).astype(np.uint8)
    got = D.resize_lanczos(torch.from_numpy(g), (29, 51)).cpu().numpy()
    for b in range(3):
        assert np.array_equal(got[b, :, :, 0], np.asarray(Image.fromarray(g[b, :, :, 0]).resize((51, 29), Image.LANCZOS)))
