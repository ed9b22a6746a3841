"""NumPy restatement of the copy-paste stage (include/isa_kernels.h: isa_copy_paste_u8): plain loops
over images and planes and index arrays over pixels, written from the contract, not from the kernel.
tests/test_copy_paste_ref.py pins it against hand-written cases; the GPU tests compare the kernels with it."""
import numpy as np


def copy_paste(rgb, sem, planes, n_objects, xform, select, min_area=1):
    """rgb uint8 [n,h,w,c], sem uint8 [n,h,w], planes uint8 [n,h,w,k], n_objects [n], xform [n,4] = (src, flip, dy, dx),
    select [n] (bit j: source plane j is a candidate).  Returns (rgb, sem, planes, n_out int32 [n], plan int64 [n,4] =
    (pasted bits, kept-target bits, n_out, area-limited flag), the bit sets as non-negative integers)."""
    rgb, sem, planes = np.asarray(rgb, np.uint8), np.asarray(sem, np.uint8), np.asarray(planes, np.uint8)
    n, h, w, k = planes.shape
    rgb_out, sem_out, planes_out = rgb.copy(), sem.copy(), np.zeros_like(planes)
    n_out, plan = np.zeros(n, np.int32), np.zeros((n, 4), np.int64)
    threshold = max(int(min_area), 1)
    y, x = np.mgrid[0:h, 0:w]
    for b in range(n):
        nb = min(max(int(n_objects[b]), 0), k)
        s, flip, dy, dx = (int(v) for v in xform[b])
        bits = int(select[b]) & 0xffffffff
        pasted, flag, q = [], 0, None
        if 0 <= s < n:
            u, v = x - dx, y - dy                                        # Python ints behind int64 arrays: no wrap-around
            frame = (u >= 0) & (u < w) & (v >= 0) & (v < h)
            xs = np.where(flip & 1, w - 1 - u, u)
            ys = np.where(flip & 2, h - 1 - v, v)
            xs, ys = np.where(frame, xs, 0), np.where(frame, ys, 0)      # any pixel: masked again below
            q = planes[s][ys, xs] * frame[:, :, None].astype(np.uint8)   # [h,w,k]: the source's planes as the target sees them
            ns = min(max(int(n_objects[s]), 0), k)
            for j in range(ns):
                if not (bits >> j) & 1:
                    continue
                if np.count_nonzero(q[:, :, j]) >= threshold and len(pasted) < k - nb:
                    pasted.append(j)
                else:
                    flag = 1
        if not pasted:
            planes_out[b, :, :, :nb] = planes[b, :, :, :nb]
            kept = list(range(nb))
        else:
            mask = (q[:, :, pasted] != 0).any(2)
            rgb_out[b][mask] = rgb[s][ys, xs][mask]
            sem_out[b][mask] = sem[s][ys, xs][mask]
            target = planes[b, :, :, :nb].copy()
            target[mask] = 0
            kept = [i for i in range(nb) if target[:, :, i].any()]
            for o, i in enumerate(kept):
                planes_out[b, :, :, o] = target[:, :, i]
            for o, j in enumerate(pasted):
                planes_out[b, :, :, len(kept) + o] = q[:, :, j]
        n_out[b] = len(kept) + len(pasted)
        plan[b] = (sum(1 << j for j in pasted), sum(1 << i for i in kept), n_out[b], flag)
    return rgb_out, sem_out, planes_out, n_out, plan
