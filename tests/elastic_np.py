"""NumPy restatement of the elastic deformation (include/isa_kernels.h: isa_elastic_field, isa_warp_u8; data.elastic):
the field in float64 from the float32 taps, the warp in int64 exactly as the header specifies it, and the rule that drops
emptied instance planes.  tests/test_elastic_ref.py pins it against scipy; the GPU tests compare the kernels with it."""
import numpy as np


def taps(sigma, truncate=4.0):
    """scipy.ndimage's Gaussian kernel (radius = int(truncate * sigma + 0.5)), rounded to float32: (taps, radius)."""
    radius = int(truncate * float(sigma) + 0.5)
    if radius == 0:
        return np.ones(1, np.float32), 0
    k = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * k ** 2)
    return (phi / phi.sum()).astype(np.float32), radius


def field(noise, alpha, tap):
    """disp[b,y,x,k] = alpha[b] * (blur along x, then along y, zeros outside) in float64.  noise [n,h,w,2]; tap: 2r+1
    weights (radius 0: disp = alpha * noise whatever the one weight is)."""
    x = np.asarray(noise, np.float64)
    n, h, w, _ = x.shape
    t = np.asarray(tap, np.float64)
    r = (len(t) - 1) // 2
    if r == 0:
        t = np.ones(1)
    pad = np.zeros((n, h, w + 2 * r, 2))
    pad[:, :, r:r + w] = x
    rows = sum(t[k] * pad[:, :, k:k + w] for k in range(2 * r + 1))
    pad = np.zeros((n, h + 2 * r, w, 2))
    pad[:, r:r + h] = rows
    cols = sum(t[k] * pad[:, k:k + h] for k in range(2 * r + 1))
    a = np.broadcast_to(np.asarray(alpha, np.float64).reshape(-1), (n,))
    return a[:, None, None, None] * cols


def quant(disp):
    """(qx, qy) int64 [n,h,w]: the sampling position of every pixel in 1/256 pixel.  One rounding, in float32."""
    d = np.asarray(disp, np.float32)
    n, h, w, _ = d.shape
    d = np.where(np.isnan(d), np.float32(0), d)
    d = np.clip(d, np.float32(-16384), np.float32(16384))
    q = np.rint(d * np.float32(256)).astype(np.int64)                    # exact product; half to even
    yy, xx = np.mgrid[0:h, 0:w]
    return xx[None] * 256 + q[..., 0], yy[None] * 256 + q[..., 1]


def _take(src, ys, xs):
    b = np.arange(src.shape[0])[:, None, None]
    return src[b, ys, xs]


def warp_nearest(src, disp):
    """src uint8 [n,h,w,c] or [n,h,w]."""
    src = np.asarray(src)
    h, w = src.shape[1:3]
    qx, qy = quant(disp)
    return _take(src, np.clip((qy + 128) >> 8, 0, h - 1), np.clip((qx + 128) >> 8, 0, w - 1))


def warp_bilinear(src, disp):
    src = np.asarray(src)
    h, w = src.shape[1:3]
    qx, qy = quant(disp)
    x0, y0, fx, fy = qx >> 8, qy >> 8, qx & 255, qy & 255
    xa, xb, ya, yb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1), np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    ex = (lambda v: v[..., None]) if src.ndim == 4 else (lambda v: v)
    acc = (ex((256 - fx) * (256 - fy)) * _take(src, ya, xa).astype(np.int64) + ex(fx * (256 - fy)) * _take(src, ya, xb) +
           ex((256 - fx) * fy) * _take(src, yb, xa) + ex(fx * fy) * _take(src, yb, xb))
    return ((acc + 32768) >> 16).astype(np.uint8)


def compact(planes, n_objects):
    """ONE image's warped planes uint8 [h,w,K], the first n_objects real -> (planes, n_objects') with the real planes the
    warp left without a pixel dropped, the survivors at the front and zero planes behind them; None when no plane would
    stay (the stage then returns the image unwarped).  Nothing dropped: the planes as they are."""
    keep = [i for i in range(n_objects) if planes[:, :, i].any()]
    if len(keep) == n_objects:
        return planes, n_objects
    if not keep:
        return None
    out = np.zeros_like(planes)
    out[:, :, :len(keep)] = planes[:, :, keep]
    return out, len(keep)


def elastic(rgb, sem, planes, n_objects, disp):
    """data.elastic on the host: (rgb, sem, planes, counts)."""
    rgb2, sem2, p2 = warp_bilinear(rgb, disp), warp_nearest(sem, disp), warp_nearest(planes, disp)
    counts = [int(v) for v in n_objects]
    for b in range(len(counts)):
        got = compact(p2[b], counts[b])
        if got is None:
            rgb2[b], sem2[b], p2[b] = rgb[b], sem[b], planes[b]
        else:
            p2[b], counts[b] = got
    return rgb2, sem2, p2, counts
