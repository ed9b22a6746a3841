"""CPU-only: the restatement tests/distance_np.py (what the GPU tests compare isa_edt2_u8, isa_border_weights and
isa_fill_labels with) against per-instance scipy.ndimage.distance_transform_edt and against hand-written answers."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests")]
import distance_np as dn     # noqa: E402

INF = dn.INF


def scipy_two_nearest(lab):
    """d1sq, d2sq, nearest of one image from one scipy EDT per instance (float distances, squared and rounded: exact up to
    2^26, far above these maps)."""
    from scipy.ndimage import distance_transform_edt
    ks = [int(k) for k in np.unique(lab) if k]
    h, w = lab.shape
    if not ks:
        return np.full((h, w), INF, np.int32), np.full((h, w), INF, np.int32), np.zeros((h, w), np.uint8)
    D = np.stack([np.rint(distance_transform_edt(lab != k) ** 2).astype(np.int64) for k in ks])
    srt = np.sort(D, axis=0)
    near = np.asarray(ks, np.uint8)[np.argmin(D, axis=0)]              # argmin: the first, i.e. the smallest label
    d2 = srt[1].astype(np.int32) if len(ks) > 1 else np.full((h, w), INF, np.int32)
    return srt[0].astype(np.int32), d2, near


@pytest.mark.parametrize("shape", [(4, 4), (8, 12), (24, 36), (72, 136)])
def test_restatement_matches_per_instance_scipy_edt(shape):
    h, w = shape
    for name, maps in dn.cases(2, h, w, seed=3).items():
        got = dn.edt2(maps, "brute")
        for b in range(2):
            want = scipy_two_nearest(maps[b])
            for g, w_, part in zip(got, want, ("d1sq", "d2sq", "nearest")):
                assert g[b].dtype == w_.dtype and np.array_equal(g[b], w_), (name, b, part)
        if h * w <= 24 * 36:                                            # the index route of the large shapes agrees too
            for g, w_ in zip(dn.edt2(maps, "scipy"), got):
                assert np.array_equal(g, w_), name


def test_sparse_noise_with_few_labels_has_ties_and_still_agrees():
    rng = np.random.default_rng(5)
    ties = 0
    for _ in range(20):
        lab = (rng.integers(1, 4, size=(1, 17, 20)) * (rng.random((1, 17, 20)) < 0.12)).astype(np.uint8)
        d1, d2, near = dn.edt2(lab, "brute")
        w1, w2, wn = scipy_two_nearest(lab[0])
        assert np.array_equal(d1[0], w1) and np.array_equal(d2[0], w2) and np.array_equal(near[0], wn)
        ties += int(((d1 == d2) & (d1 != INF)).sum())
    assert ties > 50


def test_checkerboard_by_hand():
    """Labels 1 and 2 alternate on the even lattice of a 6 x 8 map.  A pixel with one odd coordinate lies between two
    lattice points of different labels, one pixel from each: d1sq = d2sq = 1, nearest = 1.  A pixel with two odd
    coordinates lies in the middle of four (two of each label) at squared distance 2.  On the last column (7, odd, no lattice
    point to its right) and likewise nowhere else - the last row is 5, and row 6 does not exist - the nearest lattice
    points are one to the left and, of the other label, one to the left and two up or down."""
    lab = dn.checkerboard(6, 8)[None]
    assert lab[0, 0, 0] == 1 and lab[0, 0, 2] == 2 and lab[0, 2, 0] == 2 and lab[0, 2, 2] == 1 and lab[0, 1, 1] == 0
    d1, d2, near = dn.edt2(lab)
    yy, xx = np.mgrid[0:6, 0:8]
    on = (yy % 2 == 0) & (xx % 2 == 0)
    assert np.all(d1[0][on] == 0) and np.all(d2[0][on] == 4) and np.array_equal(near[0][on], lab[0][on])
    inner = (xx < 7) & (yy < 5)
    edge = ((yy % 2) + (xx % 2) == 1) & inner
    assert np.all(d1[0][edge] == 1) and np.all(d2[0][edge] == 1) and np.all(near[0][edge] == 1)
    mid = (yy % 2 == 1) & (xx % 2 == 1) & inner
    assert np.all(d1[0][mid] == 2) and np.all(d2[0][mid] == 2) and np.all(near[0][mid] == 1)
    # the last column, even rows: the lattice point at x = 6 is 1 away, the other label sits at (y +- 2, 6): 1 + 4
    assert [int(d1[0, y, 7]) for y in (0, 2, 4)] == [1, 1, 1] and [int(d2[0, y, 7]) for y in (0, 2, 4)] == [5, 5, 5]
    assert [int(near[0, y, 7]) for y in (0, 2, 4)] == [int(lab[0, y, 6]) for y in (0, 2, 4)]
    # wherever the nearest is tied the second distance equals the first
    ks, D = dn.label_distances(lab[0])
    tied = (D == D.min(axis=0)).sum(axis=0) > 1
    assert tied.any() and np.array_equal(d1[0][tied], d2[0][tied])


def test_one_pixel_in_a_corner_by_hand():
    lab = np.zeros((1, 5, 8), np.uint8)
    lab[0, 4, 7] = 9
    d1, d2, near = dn.edt2(lab)
    yy, xx = np.mgrid[0:5, 0:8]
    assert np.array_equal(d1[0], (4 - yy) ** 2 + (7 - xx) ** 2) and d1[0, 0, 0] == 65
    assert np.all(d2 == INF) and np.all(near == 9)
    w = dn.border_weights(lab, d1, d2, 10.0, 5.0)
    assert np.all(w == 1.0)                                            # no second instance: no border anywhere


def test_empty_map_by_hand():
    lab = np.zeros((2, 4, 4), np.uint8)
    d1, d2, near = dn.edt2(lab)
    assert np.all(d1 == INF) and np.all(d2 == INF) and np.all(near == 0)
    assert d1.dtype == np.int32 and d2.dtype == np.int32 and near.dtype == np.uint8
    out, filled = dn.fill(lab, np.ones_like(lab), near, d1)
    assert np.all(out == 0) and filled.tolist() == [0, 0]


def test_weight_map_and_fill_by_hand():
    lab = np.zeros((1, 1, 8), np.uint8)
    lab[0, 0, 1], lab[0, 0, 6] = 3, 5                                   # . 3 . . . . 5 .
    d1, d2, near = dn.edt2(lab)
    assert d1[0, 0].tolist() == [1, 0, 1, 4, 4, 1, 0, 1] and d2[0, 0].tolist() == [36, 25, 16, 9, 9, 16, 25, 36]
    assert near[0, 0].tolist() == [3, 3, 3, 3, 5, 5, 5, 5]
    w = dn.border_weights(lab, d1, d2, 10.0, 5.0)
    assert w[0, 0, 1] == 1.0 and w[0, 0, 6] == 1.0
    assert w[0, 0, 3] == pytest.approx(1 + 10 * np.exp(-25 / 50.0), rel=1e-15)      # d1 + d2 = 2 + 3
    assert w[0, 0, 0] == pytest.approx(1 + 10 * np.exp(-49 / 50.0), rel=1e-15)      # 1 + 6
    fg = np.array([[[0, 1, 1, 1, 1, 1, 1, 1]]], np.uint8)
    out, filled = dn.fill(lab, fg, near, d1, dn.max_dist_sq(None))
    assert out[0, 0].tolist() == [0, 3, 3, 3, 5, 5, 5, 5] and filled.tolist() == [5]
    out, filled = dn.fill(lab, fg, near, d1, dn.max_dist_sq(1))
    assert out[0, 0].tolist() == [0, 3, 3, 0, 0, 5, 5, 5] and filled.tolist() == [3]
    out, filled = dn.fill(lab, fg, near, d1, dn.max_dist_sq(0))
    assert np.array_equal(out, lab) and filled.tolist() == [0]
