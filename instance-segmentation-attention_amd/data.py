"""Synthetic stand-in for the LMDB dataset + AlignCollate output (dataset.py:368-378): the reference
ships no data.  Same tensors and dtypes the collate function produces; rectangles/ellipses as instances
(mirrors the zero-padded 32-instance layout, dataset.py:304-310).  numpy RNG only."""
import numpy as np
import torch


def synth_batch(batch, height, width, seed=0, max_objects=32, kmin=3, kmax=8):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((batch, 21, height, width)).astype(np.float32)
    ins = np.zeros((batch, max_objects, height, width), dtype=np.int64)
    n = np.zeros((batch,), dtype=np.int32)
    yy, xx = np.mgrid[0:height, 0:width]
    for b in range(batch):
        k = int(rs.randint(kmin, kmax + 1))
        occupied = np.zeros((height, width), dtype=bool)
        placed = tries = 0
        while placed < k and tries < 200:
            tries += 1
            hh = int(rs.randint(max(2, height // 10), max(3, height // 3)))
            ww = int(rs.randint(max(2, width // 10), max(3, width // 3)))
            y0, x0 = int(rs.randint(0, height - hh + 1)), int(rs.randint(0, width - ww + 1))
            if rs.rand() < 0.5:
                m = (yy >= y0) & (yy < y0 + hh) & (xx >= x0) & (xx < x0 + ww)
            else:
                cy, cx = y0 + hh / 2.0, x0 + ww / 2.0
                m = ((yy + 0.5 - cy) / (hh / 2.0)) ** 2 + ((xx + 0.5 - cx) / (ww / 2.0)) ** 2 <= 1.0
            if m.sum() < 4 or (m & occupied).any():
                continue
            ins[b, placed][m] = 1
            occupied |= m
            placed += 1
        n[b] = placed
        x[b, :3] += occupied[None].astype(np.float32)
    fg = ins.sum(1) > 0
    sem = np.stack([~fg, fg], 1).astype(np.int64)
    return torch.from_numpy(x), torch.from_numpy(sem), torch.from_numpy(ins), torch.from_numpy(n)


class SyntheticLoader(object):
    """Iterable of `n_batches` collated minibatches, re-seeded per epoch like a shuffling DataLoader."""

    def __init__(self, n_batches, batch_size, height=256, width=256, seed=0, compact=False, n_classes=2):
        """compact=True yields the targets as the reference's collate function holds them before its last five lines
        (dataset.py:349-379): sem uint8 [B,H,W], ins uint8 [B,H,W,32]; the model expands them on the device
        (isa_collate_targets) - 8x less host-to-device traffic per step.
        n_classes > 2: semantic labels in [0, n_classes): background 0, instance j of an image class 1 + j % (K - 1)
        (no extra random draws: the stream, and the output at n_classes = 2, are those of the 2-class loader)."""
        self.n, self.bs, self.h, self.w, self.seed, self.epoch = n_batches, batch_size, height, width, seed, 0
        self.compact = compact
        self.n_classes = n_classes

    def __len__(self):
        return self.n

    def __iter__(self):
        self.epoch += 1
        for i in range(self.n):
            x, sem, ins, n = synth_batch(self.bs, self.h, self.w, seed=self.seed + 1000 * self.epoch + i)
            if self.n_classes > 2:
                sem = class_onehot(ins, self.n_classes)
            if self.compact:
                sem = sem.argmax(1).to(torch.uint8) if self.n_classes > 2 else sem[:, 1].contiguous().to(torch.uint8)
                ins = ins.permute(0, 2, 3, 1).contiguous().to(torch.uint8)
            yield x, sem, ins, n


def class_onehot(ins, n_classes):
    """Synthetic K-class targets from instance planes [B,M,H,W]: one-hot int64 [B,K,H,W] of the label map that puts
    instance j in class 1 + j % (K - 1) and the background in class 0."""
    fg = ins.sum(1) > 0
    lab = torch.where(fg, 1 + ins.argmax(1) % (n_classes - 1), torch.zeros_like(fg, dtype=torch.int64))
    return torch.nn.functional.one_hot(lab, n_classes).permute(0, 3, 1, 2).contiguous()


def d4_swaps(op):
    """True when op code `op` exchanges the image axes (transpose XOR an odd number of quarter turns)."""
    return bool(((op >> 2) ^ (op >> 3)) & 1)


def d4_augment(tensors, ops, device="cuda"):
    """The exact augmentations of the reference's collate function (dataset.py:185-233: horizontal / vertical flip,
    transpose, 90x rotation) on the device, one shared op code per image for all of `tensors` (uint8 [n,h,w,c] or
    [n,h,w]: RGB image, semantic map, instance planes).  ops: per-image codes, bit0 hflip, bit1 vflip, bit2 transpose,
    bits 3-4 = rot_angle // 90; the random draws stay on the host in the reference's call order (three
    random.random() < 0.5, one np.random.choice([0, 90, 180, 270]) per image).  Non-square images (the reference
    augments the original image, before the resize): every op of the call must agree on whether it exchanges the axes
    (d4_swaps), the outputs are [n,w,h,...] then.  Returns new device tensors."""
    from . import lib as L
    ops = [int(o) for o in ops]
    ops_dev = torch.as_tensor(ops, dtype=torch.int32).to(device)
    out = []
    for t in tensors:
        assert t.dtype == torch.uint8 and t.dim() in (3, 4), "uint8 [n,h,w(,c)]"
        src = t.to(device).contiguous()
        n, h, w = src.shape[:3]
        swap = d4_swaps(ops[0])
        assert h == w or all(d4_swaps(o) == swap for o in ops), "ops of one call must agree on exchanging the axes of a non-square image"
        swap = swap and h != w
        shape = (n, w, h) + tuple(src.shape[3:]) if swap else tuple(src.shape)
        dst = torch.empty(shape, dtype=torch.uint8, device=src.device)
        c = 1 if t.dim() == 3 else t.shape[3]
        L.checked().isa_d4_augment(src, dst, n, h, w, c, 1 if swap else 0, ops_dev, L.stream_ptr())
        out.append(dst)
    return out


# ---- rotation by a small angle and centre cut: the two non-D4 augmentations the reference ships enabled
# (settings/CVPPP/training_settings.py:40,50; AlignCollate.__preprocess, dataset.py:236-269) -----------------------------
def rotate_geometry(w, h, angle):
    """PIL Image.rotate(angle, expand=True)'s own arithmetic (Python floats, Image.py): the affine matrix that maps an
    output pixel to the source and the expanded output size.  Returns (matrix[6], (nw, nh)), or None when Pillow takes a
    transpose fast path (angle % 360 in {0, 90, 180, 270}: see d4_augment)."""
    import math
    angle = angle % 360.0
    if angle in (0, 90, 180, 270):
        return None
    cx, cy = w / 2, h / 2
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]

    def tf(x, y):
        return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]

    m[2], m[5] = tf(-cx, -cy)
    m[2] += cx
    m[5] += cy
    xs, ys = zip(*(tf(x, y) for x, y in ((0, 0), (w, 0), (w, h), (0, h))))
    nw = math.ceil(max(xs)) - math.floor(min(xs))
    nh = math.ceil(max(ys)) - math.floor(min(ys))
    m[2], m[5] = tf(-(nw - w) / 2.0, -(nh - h) / 2.0)
    return m, (nw, nh)


def _fixed_coeffs(m):
    """Geometry.c affine_fixed: FIX(v) = floor(v * 65536 + 0.5), the half-pixel centre folded into the offsets."""
    import math
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def rotate_nearest(tensors, angle, device="cuda"):
    """The reference's annotation rotator (dataset.py:142,243-249: Image.rotate(angle, NEAREST, expand=True) per instance
    plane and for the semantic map) on the device for uint8 [n,h,w,c] tensors sharing one angle; bit-identical to Pillow."""
    import ctypes as C
    from . import lib as L
    out = []
    for t in tensors:
        src = t.to(device).contiguous()
        assert src.dtype == torch.uint8 and src.dim() == 4
        n, h, w, c = src.shape
        g = rotate_geometry(w, h, angle)
        if g is None:                       # Pillow's transpose fast paths: a quarter-turn op of d4_augment (0 = copy)
            q = int(angle % 360) // 90
            out.append(src.clone() if q == 0 else d4_augment([src], [q << 3] * n, device)[0])
            continue
        m, (nw, nh) = g
        coef = (C.c_int32 * 6)(*_fixed_coeffs(m))
        dst = torch.empty((n, nh, nw, c), dtype=torch.uint8, device=src.device)
        L.checked().isa_rotate_nearest_u8(src, n, h, w, c, dst, nh, nw, coef, L.stream_ptr())
        out.append(dst)
    return out


def background_colour(rgb_host, key):
    """preprocess.py:349-362: the four backgrounds of rotate_with_random_bg - 0 white, 1 black, 2 int(mean), 3 int(median)
    per channel of the source image (host numpy array [h,w,3]; the reference computes them on the host as well)."""
    import numpy as np
    if key == 0:
        return (255, 255, 255)
    if key == 1:
        return (0, 0, 0)
    if key == 2:
        return tuple(int(v) for v in rgb_host.mean((0, 1)))
    return tuple(int(v) for v in np.median(rgb_host, (0, 1)))


def rotate_image(rgb, angle, bg, device="cuda"):
    """The reference's image rotator (dataset.py:140,241 -> preprocess.py:330-365 rotate_with_random_bg: RGBA, BILINEAR,
    expand, composite over the drawn background `bg`) on the device: uint8 [n,h,w,3] -> [n,nh,nw,3], bit-identical to
    Pillow."""
    import ctypes as C
    from . import lib as L
    src = rgb.to(device).contiguous()
    assert src.dtype == torch.uint8 and src.dim() == 4 and src.shape[3] <= 4
    n, h, w, c = src.shape
    g = rotate_geometry(w, h, angle)
    if g is None:
        q = int(angle % 360) // 90
        return src.clone() if q == 0 else d4_augment([src], [q << 3] * n, device)[0]
    m, (nw, nh) = g
    mat = (C.c_double * 6)(*m)
    bgc = (C.c_uint8 * 4)(*([int(v) for v in bg] + [255] * (4 - len(bg))))
    dst = torch.empty((n, nh, nw, c), dtype=torch.uint8, device=src.device)
    L.checked().isa_rotate_bilinear_u8(src, n, h, w, c, dst, nh, nw, mat, bgc, L.stream_ptr())
    return dst


def center_cut_window(H, W, center, h, w):
    """preprocess.py:239-264 CenterCut: the window (y0, x0, height, width) it takes from an H x W array around `center`
    for an h x w output (it doubles both and clamps to the image)."""
    h, w = 2 * h, 2 * w
    if center[0] - h // 2 < 0:
        y0 = 0
    elif center[0] + h // 2 > H:
        y0 = max(0, H - h)
    else:
        y0 = center[0] - h // 2
    if center[1] - w // 2 < 0:
        x0 = 0
    elif center[1] + w // 2 > W:
        x0 = max(0, W - w)
    else:
        x0 = center[1] - w // 2
    return int(y0), int(x0), min(H, y0 + min(H, h)) - int(y0), min(W, x0 + min(W, w)) - int(x0)


def center_cut(rgb, sem, planes, n_objects, draw, out_h, out_w, max_planes=32, device="cuda"):
    """dataset.py:252-269 on the device for ONE image: rgb uint8 [1,H,W,3], sem uint8 [1,H,W,1], planes uint8 [1,H,W,K]
    (the first n_objects are real).  `draw(count)` returns the reference's np.random.choice(count) - the index of the
    chosen centre in the row-major list of pixels covered by exactly one plane.  Returns (rgb, sem, planes [1,h',w',
    max_planes] with the surviving planes first, n_objects') - the has-object filter (window sum > 30) drops planes."""
    from . import lib as L
    lib, st = L.checked(), L.stream_ptr()
    _, H, W, K = planes.shape
    single = torch.empty((1, H, W), dtype=torch.uint8, device=device)
    rows = torch.empty((1, H), dtype=torch.int32, device=device)
    real = planes if n_objects == K else planes[..., :n_objects].contiguous()
    lib.isa_cover_rows_u8(real, 1, H, W, n_objects, single, rows, st)
    counts = rows[0].cpu().numpy().astype("int64")
    total = int(counts.sum())
    assert total > 0, "no pixel is covered by exactly one instance (the reference raises here too)"
    pick = int(draw(total))
    cum = counts.cumsum()
    r = int((cum > pick).argmax())
    j = pick - int(cum[r] - counts[r])
    cols = single[0, r].cpu().numpy().nonzero()[0]
    center = (r, int(cols[j]))
    y0, x0, hh, ww = center_cut_window(H, W, center, out_h, out_w)
    sums = torch.zeros((1, n_objects), dtype=torch.int64, device=device)
    lib.isa_plane_sums_u8(real, 1, H, W, n_objects, y0, x0, hh, ww, sums, st)
    keep = [i for i, v in enumerate(sums[0].cpu().tolist()) if v > 30]
    chan = torch.tensor(keep + [-1] * (max_planes - len(keep)), dtype=torch.int32, device=device)
    p2 = torch.empty((1, hh, ww, max_planes), dtype=torch.uint8, device=device)
    lib.isa_crop_planes_u8(real, 1, H, W, n_objects, y0, x0, p2, hh, ww, max_planes, chan, st)
    r2 = torch.empty((1, hh, ww, rgb.shape[3]), dtype=torch.uint8, device=device)
    lib.isa_crop_planes_u8(rgb, 1, H, W, rgb.shape[3], y0, x0, r2, hh, ww, rgb.shape[3], None, st)
    s2 = torch.empty((1, hh, ww, 1), dtype=torch.uint8, device=device)
    lib.isa_crop_planes_u8(sem, 1, H, W, 1, y0, x0, s2, hh, ww, 1, None, st)
    return r2, s2, p2, len(keep)


_RESIZE_WS = {}


def resize_bilinear(images, size, device="cuda"):
    """The reference's `img_resizer` (dataset.py:160-161, prediction.py:37: PIL Image.resize(BILINEAR)) on the device:
    uint8 [n,h0,w0,c] (c <= 4) -> uint8 [n,size_h,size_w,c], bit-identical to Pillow (isa_resize_bilinear_u8)."""
    from . import lib as L
    h, w = (size, size) if isinstance(size, int) else size
    src = images.to(device).contiguous()
    assert src.dtype == torch.uint8 and src.dim() == 4
    n, h0, w0, c = src.shape
    dst = torch.empty((n, h, w, c), dtype=torch.uint8, device=src.device)
    need = int(L.checked().isa_resize_bilinear_ws_bytes(n, h0, w0, c, h, w))
    ws = _RESIZE_WS.get(src.device)
    if ws is None or ws.numel() < need:
        ws = _RESIZE_WS[src.device] = torch.empty(max(need, 1 << 20), dtype=torch.uint8, device=src.device)
    L.checked().isa_resize_bilinear_u8(src, n, h0, w0, c, dst, h, w, ws, ws.numel(), L.stream_ptr())
    return dst


def resize_lanczos(images, size, device="cuda"):
    """PIL Image.resize(size, LANCZOS) - the reference's `Image.ANTIALIAS` (preprocess.py:451-452) - on the device:
    uint8 [n,h0,w0,c] (c <= 4) -> uint8 [n,size_h,size_w,c], bit-identical to Pillow (isa_resize_lanczos_u8; the
    coefficient tables are computed on the host inside the call)."""
    import ctypes as C
    from . import lib as L
    h, w = (size, size) if isinstance(size, int) else size
    src = images.to(device).contiguous()
    assert src.dtype == torch.uint8 and src.dim() == 4
    n, h0, w0, c = src.shape
    dst = torch.empty((n, h, w, c), dtype=torch.uint8, device=src.device)
    need = C.c_int64(0)
    L.checked().isa_resize_lanczos_ws_bytes(n, h0, w0, c, h, w, C.byref(need))
    need = need.value
    ws = _RESIZE_WS.get(src.device)
    if ws is None or ws.numel() < need:
        ws = _RESIZE_WS[src.device] = torch.empty(max(need, 1 << 20), dtype=torch.uint8, device=src.device)
    L.checked().isa_resize_lanczos_u8(src, n, h0, w0, c, dst, h, w, ws, ws.numel(), L.stream_ptr())
    return dst


def resolution_degrade(rgb, ratio, device="cuda"):
    """The reference's random_resolution (preprocess.py:443-454) for a drawn ratio on the device: Lanczos resize to
    (size * ratio).astype('int'), then back.  uint8 [n,h,w,c] -> the same shape."""
    n, h, w, c = rgb.shape
    nw, nh = (int(v) for v in (np.array([w, h]) * ratio).astype('int'))
    assert nw >= 1 and nh >= 1 and h >= 1 and w >= 1, "resolution ratio %r leaves no pixel of %dx%d" % (ratio, w, h)
    return resize_lanczos(resize_lanczos(rgb, (nh, nw), device), (h, w), device)


def gamma_lut(gamma, gain=1):
    """adjust_gamma's table (preprocess.py:424) as Image.point applies it: every entry through Python's round()."""
    return [round(255 * gain * pow(i / 255., gamma)) for i in range(256)]


_PHOTO_OPS = dict(brightness=0, contrast=1, saturation=2, hue=3)


def photo_program(ops=(), lut=None, chan=(0, 1, 2), gray=False):
    """One image's program for `photometric`.  ops: sequence of (name, factor), name in brightness / contrast /
    saturation / hue, each at most once, applied in the given order (hue's factor is torchvision's hue_factor in
    [-0.5, 0.5]: H moves by int(factor * 255) & 255); lut: 256 bytes or None; chan: the source channel of each output
    channel, duplicates allowed; gray: L to all three channels."""
    from . import lib as L
    p = L.IsaPhotoProg()
    ops = list(ops)
    names = [name for name, _ in ops]
    assert len(ops) <= 4 and len(set(names)) == len(names) and all(name in _PHOTO_OPS for name in names), names
    p.n_ops = len(ops)
    for k, (name, factor) in enumerate(ops):
        p.op[k] = _PHOTO_OPS[name]
        p.factor[k] = float(factor)
        if name == "hue":
            assert -0.5 <= factor <= 0.5, factor
            p.hue_shift = int(factor * 255) & 255
        else:
            assert factor >= 0, (name, factor)
    if lut is not None:
        lut = [int(v) for v in lut]
        assert len(lut) == 256 and all(0 <= v <= 255 for v in lut)
        p.use_lut = 1
        p.lut[:] = lut
    chan = [int(v) for v in chan]
    assert len(chan) == 3 and all(0 <= v <= 2 for v in chan), chan
    p.chan[:] = chan
    p.gray = 1 if gray else 0
    return p


def photometric(rgb, programs, device="cuda", out=None):
    """Colour jitter, gamma, channel swap and grayscale (dataset.py:271-281) in one pass on the device
    (isa_photometric_u8): uint8 [n,h,w,3] and one `photo_program` per image -> uint8 [n,h,w,3], bit-identical to the
    reference's sequence of PIL calls.  out: the tensor to write (may be `rgb` itself), a new one by default."""
    from . import lib as L
    src = rgb.to(device).contiguous()
    assert src.dtype == torch.uint8 and src.dim() == 4 and src.shape[3] == 3
    n, h, w, _ = src.shape
    programs = list(programs)
    assert len(programs) == n, (len(programs), n)
    packed = (L.IsaPhotoProg * n)(*programs)
    progs = torch.frombuffer(bytearray(bytes(packed)), dtype=torch.uint8).to(src.device)
    contrast = any(L.PHOTO_CONTRAST in list(p.op[:p.n_ops]) for p in programs)
    sums = torch.empty(n, dtype=torch.int64, device=src.device) if contrast else None
    dst = torch.empty_like(src) if out is None else out
    assert dst.is_contiguous() and dst.dtype == torch.uint8 and dst.shape == src.shape and dst.device == src.device
    L.checked().isa_photometric_u8(src, dst, n, h, w, progs, int(contrast), sums, L.stream_ptr())
    return dst


# ---- elastic deformation (Simard et al. 2003): not in the reference; the arithmetic is defined in include/isa_kernels.h
# and DESIGN.md section 18 ----------------------------------------------------------------------------------------------
def gaussian_taps(sigma, truncate=4.0):
    """The weights of scipy.ndimage.gaussian_filter1d(sigma, truncate=truncate): radius = int(truncate * sigma + 0.5),
    exp(-0.5 (k / sigma)^2) for k = -radius..radius, normalised in double, rounded to float32.  Returns (taps, radius)."""
    import numpy as np
    from . import lib as L
    sigma = float(sigma)
    assert sigma >= 0 and truncate >= 0
    radius = int(truncate * sigma + 0.5)
    assert radius <= L.ELASTIC_MAX_RADIUS, "radius %d of sigma %g exceeds ISA_ELASTIC_MAX_RADIUS" % (radius, sigma)
    if radius == 0:
        return np.ones(1, np.float32), 0
    k = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    return (phi / phi.sum()).astype(np.float32), radius


def elastic_field(noise, alpha, sigma, device="cuda"):
    """The displacement field of an elastic deformation on the device (isa_elastic_field): noise fp32 [n,h,w,2] in
    [-1, 1) -> disp fp32 [n,h,w,2] = alpha[b] * (Gaussian blur of the noise, sigma pixels, truncated at 4 sigma, zeros
    outside the image).  Component 0 is dx, component 1 is dy.  alpha: a scalar, a sequence of n or a device tensor [n]."""
    import ctypes as C
    from . import lib as L
    src = noise.to(device).contiguous()
    assert src.dtype == torch.float32 and src.dim() == 4 and src.shape[3] == 2, "fp32 [n,h,w,2]"
    n, h, w, _ = src.shape
    if torch.is_tensor(alpha):
        a = alpha.to(device=src.device, dtype=torch.float32).reshape(-1).contiguous()
    else:
        a = torch.as_tensor(alpha, dtype=torch.float32).reshape(-1).to(src.device)
    if a.numel() == 1 and n > 1:
        a = a.repeat(n)
    assert a.numel() == n, (a.numel(), n)
    taps, radius = gaussian_taps(sigma)
    disp = torch.empty_like(src)
    scratch = torch.empty(L.elastic_scratch_bytes(n, h, w), dtype=torch.uint8, device=src.device)
    L.checked().isa_elastic_field(src, a, n, h, w, taps.ctypes.data_as(C.c_void_p), radius, disp, scratch, scratch.numel(),
                                  L.stream_ptr())
    return disp


def warp(tensors, disp, modes, device="cuda"):
    """uint8 tensors [n,h,w,c] or [n,h,w] sampled at (x + disp[...,0], y + disp[...,1]) on the device (isa_warp_u8), any
    displacement field fp32 [n,h,w,2]; modes: one of 'nearest' / 'bilinear' (or lib.WARP_*) per tensor.  Coordinates are
    clamped to the image (replicate border).  Returns new tensors of the inputs' shapes."""
    from . import lib as L
    names = dict(nearest=L.WARP_NEAREST, bilinear=L.WARP_BILINEAR)
    tensors, modes = list(tensors), [names.get(m, m) for m in modes]
    assert len(tensors) == len(modes)
    d = disp.to(device).contiguous()
    assert d.dtype == torch.float32 and d.dim() == 4 and d.shape[3] == 2, "fp32 [n,h,w,2]"
    out = []
    for t, mode in zip(tensors, modes):
        assert t.dtype == torch.uint8 and t.dim() in (3, 4), "uint8 [n,h,w(,c)]"
        src = t.to(device).contiguous()
        assert tuple(src.shape[:3]) == tuple(d.shape[:3]), (tuple(src.shape), tuple(d.shape))
        n, h, w = src.shape[:3]
        dst = torch.empty_like(src)
        L.checked().isa_warp_u8(src, d, n, h, w, 1 if t.dim() == 3 else t.shape[3], int(mode), dst, L.stream_ptr())
        out.append(dst)
    return out


def elastic(rgb, sem, planes, n_objects, disp, max_planes=32, device="cuda"):
    """The loader's elastic stage for a batch: rgb uint8 [n,h,w,3] warped bilinear, sem uint8 [n,h,w(,1)] and planes
    uint8 [n,h,w,K] warped nearest, all by the same field disp fp32 [n,h,w,2].  n_objects: the real planes per image (an
    int, a sequence or a tensor).  An image in which the warp left one of its real planes without a pixel has those planes
    dropped and the survivors compacted to the front, zero planes behind them (isa_plane_sums_u8, isa_crop_planes_u8, as
    the centre cut does); an image that would keep no plane is returned unwarped with its count unchanged.  Returns
    (rgb, sem, planes [n,h,w,max_planes], n_objects as a list)."""
    from . import lib as L
    lib, st = L.checked(), L.stream_ptr()
    n, h, w, K = planes.shape
    if torch.is_tensor(n_objects):
        n_objects = n_objects.reshape(-1).tolist()
    counts = [int(n_objects)] * n if isinstance(n_objects, int) else [int(v) for v in n_objects]
    assert len(counts) == n and all(0 <= k <= K for k in counts), (counts, n, K)
    rgb2, sem2, p2 = warp([rgb, sem, planes], disp, ["bilinear", "nearest", "nearest"], device)
    if K != max_planes:                                  # the hand-over has max_planes planes (zero planes behind the real ones)
        full = torch.zeros((n, h, w, max_planes), dtype=torch.uint8, device=p2.device)
        full[..., :min(K, max_planes)] = p2[..., :max_planes]
        p2, K = full, max_planes
        counts = [min(k, K) for k in counts]
    sums = torch.zeros((n, K), dtype=torch.int64, device=p2.device)
    lib.isa_plane_sums_u8(p2, n, h, w, K, 0, 0, h, w, sums, st)
    sums = sums.cpu().tolist()
    out_counts = list(counts)
    for b in range(n):
        keep = [i for i in range(counts[b]) if sums[b][i] > 0]
        if len(keep) == counts[b]:
            continue
        if not keep:                                     # nothing would be left: this image stays as it was
            rgb2[b], sem2[b] = rgb[b].to(p2.device), sem[b].to(p2.device)
            p2[b].zero_()
            p2[b, :, :, :min(planes.shape[3], K)] = planes[b, :, :, :K].to(p2.device)
            continue
        chan = torch.tensor(keep + [-1] * (K - len(keep)), dtype=torch.int32, device=p2.device)
        packed = torch.empty((1, h, w, K), dtype=torch.uint8, device=p2.device)
        lib.isa_crop_planes_u8(p2[b], 1, h, w, K, 0, 0, packed, h, w, K, chan, st)
        p2[b] = packed[0]
        out_counts[b] = len(keep)
    return rgb2, sem2, p2, out_counts


# ---- copy-paste (Ghiasi et al. 2021): not in the reference; the contract is in include/isa_kernels.h and DESIGN.md
# section 19 ------------------------------------------------------------------------------------------------------------
def _device_i32(v, n, width, device):
    """A sequence (copied to the device) or a device tensor (used where it is) as contiguous int32 [n] or [n,width]."""
    shape = (n,) if width == 1 else (n, width)
    if torch.is_tensor(v):
        if v.dtype == getattr(torch, "uint32", None):
            v = v.view(torch.int32)
        t = v.to(device=device, dtype=torch.int32).reshape(shape)
    else:
        t = torch.from_numpy((np.asarray(v, np.int64).reshape(shape) & 0xffffffff).astype(np.uint32).view(np.int32)).to(device)
    return t.contiguous()


def copy_paste(rgb, sem, planes, n_objects, src, select, flip, shift, min_area=1, device="cuda", out=None, scratch=None):
    """The loader's copy-paste stage for a batch on the device (isa_copy_paste_u8): instances of image src[b], chosen by
    the bits of select[b] (bit j: source plane j is a candidate), flipped (flip[b]: bit 0 along x, bit 1 along y) and
    shifted by shift[b] = (dy, dx), are pasted over image b.  rgb uint8 [n,h,w,c], sem uint8 [n,h,w], planes uint8
    [n,h,w,k]; n_objects, src, select, flip [n] and shift [n,2] are sequences or device tensors (int32; select may be
    uint32) - with device tensors nothing is copied to the host or from it.  src outside 0..n-1: no paste.  A plane whose
    pasted area is below min_area pixels is not pasted, nor is one for which the target has no free plane; target planes the
    paste covers entirely are dropped and the survivors compacted.  Returns (rgb, sem, planes, n_out int32 [n], plan int32
    [n,4] = (pasted bits, kept-target bits, n_out, area-limited flag)), all on the device; nothing is read back, so the
    call can be captured in a HIP graph once `out` (those five tensors, to be written) and `scratch` (uint8, at least
    lib.copy_paste_scratch_bytes(n, k) bytes) are given."""
    from . import lib as L
    rgb, sem, planes = (t.to(device).contiguous() for t in (rgb, sem, planes))
    assert all(t.dtype == torch.uint8 for t in (rgb, sem, planes)) and planes.dim() == 4 and rgb.dim() == 4
    n, h, w, k = planes.shape
    c = rgb.shape[3]
    assert tuple(rgb.shape[:3]) == (n, h, w) and sem.numel() == n * h * w, (tuple(rgb.shape), tuple(sem.shape), tuple(planes.shape))
    dev = planes.device
    nobj = _device_i32(n_objects, n, 1, dev)
    xform = torch.cat([_device_i32(src, n, 1, dev)[:, None], _device_i32(flip, n, 1, dev)[:, None], _device_i32(shift, n, 2, dev)], 1)
    sel = _device_i32(select, n, 1, dev)
    if out is None:
        out = (torch.empty_like(rgb), torch.empty_like(sem), torch.empty_like(planes),
               torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, 4), dtype=torch.int32, device=dev))
    rgb2, sem2, p2, n_out, plan = out
    for t, like in ((rgb2, rgb), (sem2, sem), (p2, planes)):
        assert t.is_contiguous() and t.dtype == torch.uint8 and t.shape == like.shape and t.device == dev
    assert n_out.dtype == torch.int32 and n_out.numel() == n and plan.dtype == torch.int32 and plan.numel() == 4 * n
    need = L.copy_paste_scratch_bytes(n, k)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    assert scratch.dtype == torch.uint8 and scratch.device == dev
    L.checked().isa_copy_paste_u8(rgb, sem, planes, nobj, xform, sel, n, h, w, c, k, int(min_area), rgb2, sem2, p2, n_out,
                                  plan, scratch, scratch.numel(), L.stream_ptr())
    return rgb2, sem2, p2, n_out, plan


class DevicePrefetcher(object):
    """Wraps an iterable of collated host batches (x, sem, ins, n): batch i+1 travels to the device on its own HIP
    stream while step i computes, so the host-to-device time of the reference's hand-over (373 MB per step at bs=16:
    fp32 input, int64 targets) leaves the critical path.  Host tensors are pinned once per batch; `n` stays on the
    host (the model reads it there).  Yields device tensors that the consumer's stream may use immediately."""

    def __init__(self, loader, device="cuda"):
        self.loader, self.device = loader, torch.device(device)
        self.stream = torch.cuda.Stream(device=self.device)

    def __len__(self):
        return len(self.loader)

    def _upload(self, batch):
        x, sem, ins, n = batch
        with torch.cuda.stream(self.stream):
            dev = [t.pin_memory().to(self.device, non_blocking=True) if not t.is_cuda else t for t in (x, sem, ins)]
        return dev[0], dev[1], dev[2], n

    def __iter__(self):
        it = iter(self.loader)
        try:
            nxt = self._upload(next(it))
        except StopIteration:
            return
        while nxt is not None:
            cur = nxt
            torch.cuda.current_stream(self.device).wait_stream(self.stream)     # batch i has landed
            for t in cur[:3]:
                t.record_stream(torch.cuda.current_stream(self.device))
            try:
                nxt = self._upload(next(it))                                     # batch i+1 starts moving now
            except StopIteration:
                nxt = None
            yield cur


def device_collate_targets(planes, sem, ops=None, size=256, device="cuda"):
    """The annotation side of the reference's collate function on the device, in its order (dataset.py:185-233 exact
    augmentations at the source resolution, :293-320 nearest resize, :349-379 int64 planes + one-hot):
    planes uint8 [n,h0,w0,K] (zero planes already appended up to K = 32, :305-311), sem uint8 [n,h0,w0], ops = per-image
    D4 op codes or None (on non-square sources the ops of one call must agree on exchanging the axes).  Returns (sem_onehot int64 [n,2,size,size],
    ins int64 [n,K,size,size]) on the device; three launches instead of ~70 PIL calls per image."""
    from . import lib as L
    planes, sem = planes.to(device).contiguous(), sem.to(device).contiguous()
    n, h0, w0, k = planes.shape
    sem4 = sem.reshape(n, h0, w0, 1)
    if ops is not None:
        planes, sem4 = d4_augment([planes, sem4], ops, device)
        n, h0, w0, k = planes.shape
    st = L.stream_ptr()
    p2 = torch.empty((n, size, size, k), dtype=torch.uint8, device=device)
    s2 = torch.empty((n, size, size, 1), dtype=torch.uint8, device=device)
    L.checked().isa_resize_nearest_u8(planes, n, h0, w0, k, p2, size, size, st)
    L.checked().isa_resize_nearest_u8(sem4, n, h0, w0, 1, s2, size, size, st)
    ins_out = torch.empty((n, k, size, size), dtype=torch.int64, device=device)
    sem_out = torch.empty((n, 2, size, size), dtype=torch.int64, device=device)
    L.checked().isa_collate_targets(p2, s2, n, size, size, k, ins_out, sem_out, st)
    return sem_out, ins_out
