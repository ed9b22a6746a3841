"""Host statement of what the scoring kernels compute (include/isa_kernels.h: isa_labels_from_planes,
isa_label_pair_hist, isa_instance_scores), for tests/test_gpu_score.py.  Three parts:
  - np.bincount for the joint histogram;
  - evaluate.calc_bd / calc_sbd / calc_dice / calc_dic (this repository's restatement of the reference's metrics) for
    the scores;
  - the empty-map rules, stated here once (scores): a map without objects gives NaN for its own best Dice; objects
    against a map without objects give 0.0 (evaluate.calc_bd raises ValueError there, a kernel cannot); the foreground
    Dice of two empty foregrounds is NaN (calc_dice divides by zero)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import evaluate as EV  # noqa: E402

NAN = float("nan")


def labels_from_planes(planes, pixel_major):
    """planes [n,h,w,k] (pixel_major) or [n,k,h,w] -> uint8 [n,h,w]: 1 + the first non-zero plane, 0 if none."""
    p = np.asarray(planes) != 0
    if not pixel_major:
        p = np.moveaxis(p, 1, -1)
    return np.where(p.any(-1), p.argmax(-1) + 1, 0).astype(np.uint8)


def pair_hist(a, b, na, nb):
    """(hist int64 [n,na,nb], oob int64 [n]) of uint8 maps a, b [n,L]."""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    hist, oob = np.zeros((a.shape[0], na, nb), np.int64), np.zeros(a.shape[0], np.int64)
    for i in range(a.shape[0]):
        ok = (a[i] < na) & (b[i] < nb)
        hist[i] = np.bincount(a[i][ok] * nb + b[i][ok], minlength=na * nb).reshape(na, nb)
        oob[i] = (~ok).sum()
    return hist, oob


def best_dice(x, y):
    """evaluate.calc_bd with the empty-map rules."""
    if not np.any(x):
        return NAN
    if not np.any(y):
        return 0.0
    return EV.calc_bd(x, y)


def scores(a, b, n_a=None, n_b=None):
    """The eight columns for one pair of label maps (any shape)."""
    a, b = np.asarray(a), np.asarray(b)
    objs_a, objs_b = len(np.setdiff1d(np.unique(a), [0])), len(np.setdiff1d(np.unique(b), [0]))
    ab, ba = best_dice(a, b), best_dice(b, a)
    if ab != ab or ba != ba:
        sbd = ba if ab != ab else ab                   # the number if only one is NaN, NaN if both are
    else:
        sbd = min(ab, ba)
    if np.any(a) and np.any(b):
        assert sbd == EV.calc_sbd(a, b)
    fg = EV.calc_dice(a != 0, b != 0) if (np.any(a) or np.any(b)) else NAN
    dic = EV.calc_dic(objs_a if n_a is None else int(n_a), objs_b if n_b is None else int(n_b))
    return np.array([ab, ba, sbd, objs_a, objs_b, float(dic), fg, 0.0], np.float64)


def scores_from_hist(hist):
    """Label maps that have the joint histogram `hist` [na,nb] (pixels in counter order), for scoring a bare histogram."""
    na, nb = hist.shape
    flat = np.repeat(np.arange(na * nb), np.asarray(hist).reshape(-1))
    return flat // nb, flat % nb
