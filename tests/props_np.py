"""A plain restatement of isa_label_props / isa_instance_props / isa_props_select / isa_relabel_u8 (include/isa_kernels.h)
in numpy, Python integers and fractions.Fraction: per-label masks, sums over the mask's coordinates, the crack count by
shifted comparisons.  tests/test_props_ref.py pins it against scipy.ndimage and hand-written answers; the GPU tests
compare the kernels with it."""
import math
from fractions import Fraction

import numpy as np

ACC, OUT = 16, 24
ORDER_LABEL, ORDER_AREA, ORDER_RASTER = 0, 1, 2
COLUMNS = ("area", "x0", "y0", "x1", "y1", "centroid_x", "centroid_y", "mu_xx", "mu_yy", "mu_xy", "major_axis", "minor_axis",
           "eccentricity", "orientation", "perimeter", "touches_border", "extent", "equivalent_diameter", "compactness",
           "first_pixel", "mean_c0", "mean_c1", "mean_c2", "mean_c3")
EXACT_COLS = (0, 1, 2, 3, 4, 14, 15, 19)                  # integers
RATIONAL_COLS = (5, 6, 7, 8, 9, 16, 20, 21, 22, 23)       # one division of exact integers
FLOAT_COLS = (10, 11, 12, 13, 17, 18)                     # square roots and an arc tangent


def empty_row(h, w):
    return [0, w, -1, h, -1, 0, 0, 0, 0, 0, 0, h * w, 0, 0, 0, 0]


def crack_length(lab, v):
    """(pixel, 4-neighbour) pairs where the pixel holds v and the neighbour another value or lies outside the image."""
    h, w = lab.shape
    pad = np.full((h + 2, w + 2), -1, dtype=np.int32)
    pad[1:-1, 1:-1] = lab
    m = pad[1:-1, 1:-1] == v
    total = 0
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        nb = pad[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx]
        total += int((m & (nb != v)).sum())
    return total


def label_props(labels, image=None, nl=256):
    """(acc int64 [n,nl,16], oob int32 [n]) of uint8 labels [n,h,w] and an optional uint8 image [n,h,w,c]."""
    labels = np.asarray(labels)
    n, h, w = labels.shape
    acc = np.zeros((n, nl, ACC), dtype=np.int64)
    oob = np.zeros((n,), dtype=np.int32)
    for i in range(n):
        lab = labels[i]
        oob[i] = int((lab >= nl).sum())
        acc[i, :] = empty_row(h, w)
        for v in (int(t) for t in np.unique(lab)):
            if v == 0 or v >= nl:
                continue
            ys, xs = np.nonzero(lab == v)
            xs, ys = [int(t) for t in xs], [int(t) for t in ys]             # Python integers from here
            row = [len(xs), min(xs), max(xs), min(ys), max(ys), sum(xs), sum(ys), sum(x * x for x in xs),
                   sum(y * y for y in ys), sum(x * y for x, y in zip(xs, ys)), crack_length(lab, v),
                   min(y * w + x for x, y in zip(xs, ys)), 0, 0, 0, 0]
            if image is not None:
                px = np.asarray(image)[i][lab == v].reshape(len(xs), -1)
                for k in range(px.shape[1]):
                    row[12 + k] = sum(int(t) for t in px[:, k])
            acc[i, v] = row
    return acc, oob


def central_moments(a):
    """(mu_xx, mu_yy, mu_xy) of a non-empty acc row as exact Fractions."""
    A, (sx, sy, sxx, syy, sxy) = int(a[0]), [int(t) for t in a[5:10]]
    return Fraction(A * sxx - sx * sx, A * A), Fraction(A * syy - sy * sy, A * A), Fraction(A * sxy - sx * sy, A * A)


def eigenvalues(a):
    """(l1, l2) of a non-empty acc row as floats: the radicand is an exact Fraction, rounded once, then the root; l2 from
    the exact determinant l1 * l2, without the cancellation of half - rad."""
    mxx, myy, mxy = central_moments(a)
    half, d = (mxx + myy) / 2, (mxx - myy) / 2
    l1 = float(half) + math.sqrt(d * d + mxy * mxy)
    return l1, (max(float(mxx * myy - mxy * mxy) / l1, 0.0) if l1 > 0 else 0.0)


def derive_row(a, h, w, c):
    """The 24 measurements of one acc row: ints, Fractions (the rational columns), floats; None stands for NaN."""
    a = [int(t) for t in a]
    A = a[0]
    if A == 0:
        return [0] + [None] * (OUT - 1)
    x0, x1, y0, y1 = a[1], a[2] + 1, a[3], a[4] + 1
    mxx, myy, mxy = central_moments(a)
    l1, l2 = eigenvalues(a)
    P = a[10]
    out = [A, x0, y0, x1, y1, Fraction(a[5], A), Fraction(a[6], A), mxx, myy, mxy,
           4.0 * math.sqrt(l1), 4.0 * math.sqrt(l2),
           0.0 if l1 == 0 else math.sqrt(max(1.0 - l2 / l1, 0.0)),
           0.0 if (mxy == 0 and mxx == myy) else 0.5 * math.atan2(float(2 * mxy), float(mxx - myy)),
           P, 1 if (x0 == 0 or y0 == 0 or x1 == w or y1 == h) else 0, Fraction(A, (x1 - x0) * (y1 - y0)),
           math.sqrt(4.0 * A / math.pi), 4.0 * math.pi * A / (P * P), a[11]]
    out += [Fraction(a[12 + k], A) if k < c else None for k in range(4)]
    return out


def derive(acc, h, w, c):
    """Nested lists [n][nl][24] of derive_row."""
    return [[derive_row(row, h, w, c) for row in img] for img in np.asarray(acc)]


def as_float(rows):
    """float64 array of derive()'s answer: Fractions rounded once, None -> NaN."""
    return np.array([[[float('nan') if t is None else float(t) for t in row] for row in img] for img in rows],
                    dtype=np.float64)


def select(acc, h, w, min_area=1, max_area=0, clear_border=False, order=ORDER_LABEL, max_objects=255):
    """(table uint8 [n,256], count int32 [n], dropped int32 [n])."""
    acc = np.asarray(acc)
    n, nl = acc.shape[:2]
    table = np.zeros((n, 256), dtype=np.uint8)
    count, dropped = np.zeros((n,), dtype=np.int32), np.zeros((n,), dtype=np.int32)
    for i in range(n):
        present, keep = 0, []
        for v in range(1, nl):
            a = [int(t) for t in acc[i, v]]
            if a[0] == 0:
                continue
            present += 1
            border = a[1] == 0 or a[3] == 0 or a[2] == w - 1 or a[4] == h - 1
            if a[0] >= min_area and (max_area == 0 or a[0] <= max_area) and not (clear_border and border):
                keep.append((v, a[0], a[11]))
        if order == ORDER_AREA:
            keep.sort(key=lambda t: (-t[1], t[0]))
        elif order == ORDER_RASTER:
            keep.sort(key=lambda t: (t[2], t[0]))
        for rank, (v, _, _) in enumerate(keep[:max_objects]):
            table[i, v] = rank + 1
        count[i] = min(len(keep), max_objects)
        dropped[i] = present - count[i]
    return table, count, dropped


def relabel(labels, table):
    labels = np.asarray(labels)
    return np.stack([table[i][labels[i]] for i in range(labels.shape[0])]).astype(np.uint8)
