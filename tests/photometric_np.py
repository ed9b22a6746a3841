"""numpy restatements of the Pillow operations behind AlignCollate's five photometric augmentations (colour jitter,
gamma, channel swap, grayscale, resolution), written from Pillow's observed behaviour and pinned against the installed
Pillow by tests/test_photometric_ref.py.  The device kernels (csrc/photometric.hip, isa_resize_lanczos_u8) are held
against these, byte for byte.

    blend            Image.blend(degenerate, image, f): what ImageEnhance.Brightness / Contrast / Color call
    luma             Image.convert('L')
    contrast_mean    int(ImageStat.Stat(image.convert('L')).mean[0] + 0.5), in integers
    rgb_to_hsv / hsv_to_rgb / hue_shift_byte / shift_hue      the PIL path of torchvision's adjust_hue
    gamma_lut        Image.point over a float table
    run_program      one image through a program: jitter ops in order -> LUT -> channel map -> grayscale
    resize_lanczos   Image.resize(size, LANCZOS)
    resolution_degrade   there and back at a ratio
The last section is no restatement but the reference's own sequence of PIL calls for recorded draws (pil_*), which
the loader tests replay on the host."""
import math

import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
NAMES = dict(brightness=BRIGHTNESS, contrast=CONTRAST, saturation=SATURATION, hue=HUE)


def blend(x, d, f):
    """uint8 x (image) and d (degenerate, broadcastable) -> Image.blend(d, x, f): float32 t = d + f * (x - d), each
    operation rounded to float32; truncated for 0 <= f <= 1, else clipped to [0, 255] and truncated."""
    f = np.float32(f)
    xi = np.asarray(x).astype(np.int32)
    di = np.asarray(d).astype(np.int32)
    t = di.astype(np.float32) + (f * (xi - di).astype(np.float32)).astype(np.float32)
    t = t.astype(np.float32)
    if not (0.0 <= float(f) <= 1.0):
        t = np.clip(t, np.float32(0), np.float32(255))
    return t.astype(np.int32).astype(np.uint8)


def luma(rgb):
    """[..., 3] uint8 -> [...] uint8, ITU-R 601-2 in 16-bit fixed point with rounding."""
    a = np.asarray(rgb).astype(np.uint32)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16).astype(np.uint8)


def contrast_mean(gray):
    """int(mean + 0.5) of a uint8 array as (2 * sum + count) // (2 * count)."""
    g = np.asarray(gray)
    s, c = int(g.astype(np.int64).sum()), int(g.size)
    return (2 * s + c) // (2 * c)


def rgb_to_hsv(rgb):
    """convert('HSV'): the quotients in float32, the hue sum in double stored to float32, the wrap into [0, 1) in
    double stored to float32, then the product with 255 in double, truncated."""
    a = np.asarray(rgb)
    r, g, b = (a[..., i].astype(np.int32) for i in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    flat = maxc == minc
    cr = np.where(flat, 1, maxc - minc).astype(np.float32)
    mx = np.where(flat, 1, maxc).astype(np.float32)
    s = (cr / mx).astype(np.float32)
    rc = ((maxc - r).astype(np.float32) / cr).astype(np.float32)
    gc = ((maxc - g).astype(np.float32) / cr).astype(np.float32)
    bc = ((maxc - b).astype(np.float32) / cr).astype(np.float32)
    rc64, gc64, bc64 = rc.astype(np.float64), gc.astype(np.float64), bc.astype(np.float64)
    h = np.where(r == maxc, bc64 - gc64, np.where(g == maxc, 2.0 + rc64 - bc64, 4.0 + gc64 - rc64)).astype(np.float32)
    t = h.astype(np.float64) / 6.0 + 1.0
    h = (t - np.floor(t)).astype(np.float32)                # fmod(t, 1.0) for t > 0, exact
    uh = np.clip((h.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    us = np.clip((s.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    out = np.empty(a.shape, np.uint8)
    out[..., 0] = np.where(flat, 0, uh)
    out[..., 1] = np.where(flat, 0, us)
    out[..., 2] = maxc
    return out


def _round_half_up(x):
    fl = np.floor(x)
    return (fl + ((x - fl) >= 0.5)).astype(np.int32)


def hsv_to_rgb(hsv):
    """convert('RGB') of an HSV image: float32 throughout, products rounded half up."""
    a = np.asarray(hsv)
    f32 = np.float32
    h, s, v = (a[..., i].astype(f32) for i in range(3))
    hf = ((h * f32(6.0)).astype(f32) / f32(255.0)).astype(f32)
    i = np.floor(hf)
    f = (hf - i).astype(f32)
    fs = (s / f32(255.0)).astype(f32)
    one = f32(1.0)
    p = _round_half_up((v * (one - fs).astype(f32)).astype(f32))
    q = _round_half_up((v * (one - (fs * f).astype(f32)).astype(f32)).astype(f32))
    t = _round_half_up((v * (one - (fs * (one - f).astype(f32)).astype(f32)).astype(f32)).astype(f32))
    p, q, t = (np.clip(z, 0, 255) for z in (p, q, t))
    vi = a[..., 2].astype(np.int32)
    sec = i.astype(np.int32) % 6
    r = np.choose(sec, [vi, q, p, p, t, vi])
    g = np.choose(sec, [t, vi, vi, q, p, p])
    b = np.choose(sec, [p, p, t, vi, vi, q])
    gray = a[..., 1] == 0
    out = np.empty(a.shape, np.uint8)
    out[..., 0] = np.where(gray, vi, r)
    out[..., 1] = np.where(gray, vi, g)
    out[..., 2] = np.where(gray, vi, b)
    return out


def hue_shift_byte(factor):
    """The byte added to H: int(factor * 255) & 255 (np.uint8's wrap-around, defined here for negative factors too)."""
    return int(factor * 255) & 255


def shift_hue(rgb, shift):
    hsv = rgb_to_hsv(rgb)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(shift)) & 255
    return hsv_to_rgb(hsv)


def gamma_lut(g):
    """Image.point over [255 * pow(i / 255., g)]: every entry through Python's round()."""
    return np.array([round(255 * pow(i / 255., g)) for i in range(256)], np.uint8)


def jitter_op(rgb, op, factor, shift=None):
    op = NAMES.get(op, op)
    if op == BRIGHTNESS:
        return blend(rgb, 0, factor)
    if op == CONTRAST:
        return blend(rgb, contrast_mean(luma(rgb)), factor)
    if op == SATURATION:
        return blend(rgb, luma(rgb)[..., None], factor)
    assert op == HUE
    return shift_hue(rgb, hue_shift_byte(factor) if shift is None else shift)


def run_program(rgb, ops=(), lut=None, chan=(0, 1, 2), gray=False):
    """One image [h,w,3] through a program.  ops: sequence of (op code or name, factor) in application order."""
    a = np.asarray(rgb)
    for op, factor in ops:
        a = jitter_op(a, op, factor)
    if lut is not None:
        a = np.asarray(lut, np.uint8)[a]
    a = a[..., list(chan)]
    if gray:
        a = np.repeat(luma(a)[..., None], 3, -1)
    return np.ascontiguousarray(a)


# ---- Lanczos resize (Resample.c with the Lanczos filter, support 3) ---------------------------------------------------
PRECISION_BITS = 32 - 8 - 2


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    if -3.0 <= x < 3.0:
        return _sinc(x) * _sinc(x / 3)
    return 0.0


def lanczos_coeffs(n_in, n_out):
    """(bounds int32 [n_out, 2] = (first, count), coefficients int32 [n_out, ksize] in 22-bit fixed point)."""
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 3.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((n_out, 2), np.int32)
    kk = np.zeros((n_out, ksize), np.int32)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [_lanczos((x + xmin - center + 0.5) * ss) * ss for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _resample_axis(a, n_out, axis):
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    bounds, kk = lanczos_coeffs(a.shape[0], n_out)
    out = np.empty((n_out,) + a.shape[1:], np.uint8)
    for xx in range(n_out):
        lo, cnt = bounds[xx]
        k = kk[xx, :cnt].astype(np.int64).reshape((cnt,) + (1,) * (a.ndim - 1))
        acc = (a[lo:lo + cnt] * k).sum(0) + (1 << (PRECISION_BITS - 1))
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_lanczos(a, h, w):
    """[h0,w0,c] uint8 -> [h,w,c]: horizontal pass into a uint8 intermediate, then vertical; an unchanged axis is skipped."""
    a = np.asarray(a)
    if a.shape[1] != w:
        a = _resample_axis(a, w, 1)
    if a.shape[0] != h:
        a = _resample_axis(a, h, 0)
    return np.ascontiguousarray(a)


def degraded_size(h, w, ratio):
    nw, nh = (np.array([w, h]) * ratio).astype('int')
    return int(nh), int(nw)


def resolution_degrade(a, ratio):
    h, w = a.shape[:2]
    nh, nw = degraded_size(h, w, ratio)
    return resize_lanczos(resize_lanczos(a, nh, nw), h, w)


# ---- the reference's PIL calls for recorded draws ----------------------------------------------------------------------
def pil_adjust_hue(img, factor):
    """torchvision's adjust_hue on a PIL image, with the byte that the library adds (hue_shift_byte)."""
    from PIL import Image
    h, s, v = img.convert('HSV').split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over='ignore'):
        np_h += np.uint8(hue_shift_byte(factor))
    return Image.merge('HSV', (Image.fromarray(np_h, 'L'), s, v)).convert('RGB')


def pil_photometric(img, ops=(), gamma=None, chan=None, gray=False):
    """ColorJitter's ops in the given order, adjust_gamma, the channel indexing, RandomGrayscale's conversion."""
    from PIL import Image, ImageEnhance
    for name, factor in ops:
        if name == 'brightness':
            img = ImageEnhance.Brightness(img).enhance(factor)
        elif name == 'contrast':
            img = ImageEnhance.Contrast(img).enhance(factor)
        elif name == 'saturation':
            img = ImageEnhance.Color(img).enhance(factor)
        else:
            img = pil_adjust_hue(img, factor)
    if gamma is not None:
        img = img.point([255 * 1 * pow(ele / 255., gamma) for ele in range(256)] * 3)
    if chan is not None:
        img = Image.fromarray(np.array(img)[:, :, list(chan)])
    if gray:
        l = np.array(img.convert('L'), dtype=np.uint8)
        img = Image.fromarray(np.dstack([l, l, l]), 'RGB')
    return img


def pil_resolution(img, ratio):
    from PIL import Image
    size = np.array(img.size)
    new = (size * ratio).astype('int')
    return img.resize(tuple(int(v) for v in new), Image.LANCZOS).resize(tuple(int(v) for v in size), Image.LANCZOS)


def pil_replay_draws(img, draws):
    """The four pixel-wise stages for a RecordLoader sample's recorded draws (keys absent: flag off)."""
    return pil_photometric(img, draws.get("jitter", ()), draws.get("gamma"), draws.get("channels"), draws.get("gray", False))
