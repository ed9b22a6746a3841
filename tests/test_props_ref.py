"""CPU-only: the restatement tests/props_np.py (what the GPU tests compare the kernels with) against scipy.ndimage on
random maps and against answers worked out by hand."""
import math
import os
import sys
from fractions import Fraction as F

import numpy as np
import pytest
from scipy import ndimage

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import props_np as P     # noqa: E402


def one(lab, image=None, nl=8):
    lab = np.asarray(lab, dtype=np.uint8)[None]
    acc, oob = P.label_props(lab, None if image is None else np.asarray(image, dtype=np.uint8)[None], nl)
    c = 0 if image is None else np.asarray(image).shape[-1]
    return acc[0], oob[0], P.derive(acc, lab.shape[1], lab.shape[2], c)[0]


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_against_scipy_on_random_maps(seed):
    rng = np.random.default_rng(seed)
    h, w, nl = 23, 36, 9
    lab = rng.integers(0, nl, (h, w)).astype(np.uint8)
    lab[rng.random((h, w)) < 0.5] = 0
    lab[lab == 5] = 0                                        # an empty label among present ones
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    acc, oob, rows = one(lab, img, nl)
    assert oob == 0
    index = list(range(1, nl))
    boxes = ndimage.find_objects(lab.astype(np.int32), max_label=nl - 1)
    areas = ndimage.sum_labels(np.ones_like(lab, dtype=np.float64), lab, index)
    present = [v for v in index if v != 5]
    coms = dict(zip(present, ndimage.center_of_mass(np.ones_like(lab, dtype=np.float64), lab, present)))
    for v in index:
        if boxes[v - 1] is None:
            assert v == 5 and acc[v].tolist() == P.empty_row(h, w) and rows[v][0] == 0 and rows[v][1:] == [None] * 23
            continue
        ys, xs = boxes[v - 1]
        assert rows[v][0] == int(areas[v - 1])
        assert rows[v][1:5] == [xs.start, ys.start, xs.stop, ys.stop]
        assert float(rows[v][6]) == pytest.approx(coms[v][0], rel=1e-12)
        assert float(rows[v][5]) == pytest.approx(coms[v][1], rel=1e-12)
        for k in range(3):
            mean = ndimage.sum_labels(img[:, :, k].astype(np.float64), lab, [v])[0] / areas[v - 1]
            assert float(rows[v][20 + k]) == pytest.approx(mean, rel=1e-12)
        assert rows[v][23] is None
        # second moments about the centroid, straight from the definition
        yy, xx = np.nonzero(lab == v)
        assert float(rows[v][7]) == pytest.approx(((xx - xx.mean()) ** 2).mean(), rel=1e-9, abs=1e-12)
        assert float(rows[v][8]) == pytest.approx(((yy - yy.mean()) ** 2).mean(), rel=1e-9, abs=1e-12)
        assert float(rows[v][9]) == pytest.approx(((xx - xx.mean()) * (yy - yy.mean())).mean(), rel=1e-9, abs=1e-12)
        assert rows[v][19] == int(np.flatnonzero(lab.reshape(-1) == v)[0])
    assert acc[0].tolist() == P.empty_row(h, w), "label 0 is not measured"


def test_out_of_range_labels_are_counted_not_measured():
    lab = np.zeros((4, 4), dtype=np.uint8)
    lab[0, :2] = 7
    lab[3, 3] = 2
    acc, oob, _ = one(lab, nl=4)
    assert oob == 2 and acc[2, 0] == 1 and acc.shape == (4, 16)


def test_single_pixel():
    lab = np.zeros((4, 8), dtype=np.uint8)
    lab[2, 5] = 1
    acc, _, rows = one(lab)
    assert acc[1].tolist() == [1, 5, 5, 2, 2, 5, 2, 25, 4, 10, 4, 21, 0, 0, 0, 0]
    r = rows[1]
    assert r[:10] == [1, 5, 2, 6, 3, 5, 2, 0, 0, 0]
    assert r[10:14] == [0.0, 0.0, 0.0, 0.0]
    assert r[14:17] == [4, 0, 1] and r[17] == math.sqrt(4 / math.pi) and r[18] == pytest.approx(math.pi / 4) and r[19] == 21


def test_rectangle_2x3():
    lab = np.zeros((6, 8), dtype=np.uint8)
    lab[2:4, 3:6] = 3                                        # 2 rows, 3 columns
    acc, _, rows = one(lab)
    assert acc[3, 10] == 10
    r = rows[3]
    assert r[0] == 6 and r[1:5] == [3, 2, 6, 4] and r[5:7] == [4, F(5, 2)]
    assert r[7:10] == [F(2, 3), F(1, 4), 0]
    assert r[10] == pytest.approx(4 * math.sqrt(2 / 3)) and r[11] == pytest.approx(4 * math.sqrt(1 / 4))
    assert r[12] == pytest.approx(math.sqrt(1 - (1 / 4) / (2 / 3))) and r[13] == 0.0       # long side along x
    assert r[15] == 0 and r[16] == 1 and r[19] == 2 * 8 + 3
    tall = np.zeros((6, 8), dtype=np.uint8)
    tall[1:4, 3:5] = 3
    assert one(tall)[2][3][13] == pytest.approx(math.pi / 2)                                # long side along y: +pi/2


def test_l_shape():
    lab = np.zeros((5, 5), dtype=np.uint8)
    lab[1:4, 1] = 2
    lab[3, 2:4] = 2                                          # pixels (1,1) (1,2) (1,3) (2,3) (3,3) as (x, y)
    acc, _, rows = one(lab)
    assert acc[2].tolist() == [5, 1, 3, 1, 3, 8, 12, 16, 32, 21, 12, 6, 0, 0, 0, 0]
    r = rows[2]
    assert r[5:10] == [F(8, 5), F(12, 5), F(5 * 16 - 64, 25), F(5 * 32 - 144, 25), F(5 * 21 - 96, 25)]
    assert r[16] == F(5, 9) and r[15] == 0
    assert 0 < r[13] < math.pi / 2                           # mxy > 0: the axis runs towards +x, +y (down on the screen)


def test_ring_counts_the_hole():
    lab = np.zeros((5, 5), dtype=np.uint8)
    lab[1:4, 1:4] = 1
    lab[2, 2] = 0
    acc, _, rows = one(lab)
    assert acc[1, 0] == 8 and acc[1, 10] == 12 + 4
    assert rows[1][5:7] == [2, 2] and rows[1][9] == 0 and rows[1][12] == 0.0 and rows[1][13] == 0.0


def test_label_in_two_pieces_and_border():
    lab = np.zeros((4, 8), dtype=np.uint8)
    lab[0, 0] = 1
    lab[3, 6:8] = 1
    lab[1:3, 3] = 2
    acc, _, rows = one(lab)
    assert acc[1].tolist() == [3, 0, 7, 0, 3, 13, 6, 85, 18, 39, 4 + 6, 0, 0, 0, 0, 0]
    assert rows[1][15] == 1 and rows[2][15] == 0 and rows[1][16] == F(3, 32)


def test_full_image_label_and_empty_label():
    lab = np.full((3, 4), 2, dtype=np.uint8)
    img = np.arange(12, dtype=np.uint8).reshape(3, 4, 1)
    acc, _, rows = one(lab, img)
    assert acc[2].tolist() == [12, 0, 3, 0, 2, 18, 12, 42, 20, 18, 14, 0, 66, 0, 0, 0]
    assert rows[2][15] == 1 and rows[2][16] == 1 and rows[2][20] == F(66, 12) and rows[2][21:] == [None] * 3
    assert acc[1].tolist() == [0, 4, -1, 3, -1, 0, 0, 0, 0, 0, 0, 12, 0, 0, 0, 0]
    assert rows[1] == [0] + [None] * 23
    fl = P.as_float([rows])
    assert fl[0, 1, 0] == 0.0 and np.isnan(fl[0, 1, 1:]).all()


def test_select_orders_ties_and_cap():
    h, w = 8, 16
    lab = np.zeros((h, w), dtype=np.uint8)
    lab[1:3, 9:11] = 1           # area 4, first pixel 25
    lab[1, 1:3] = 2              # area 2, first pixel 17
    lab[4:6, 4:6] = 3            # area 4, first pixel 68
    lab[7, 12:15] = 5            # area 3, touches the bottom edge
    lab[4, 10] = 6               # area 1, first pixel 74
    acc, _ = P.label_props(lab[None], None, 8)

    def tab(**kw):
        t, c, d = P.select(acc, h, w, **kw)
        return t[0, :8].tolist(), int(c[0]), int(d[0])

    assert tab() == ([0, 1, 2, 3, 0, 4, 5, 0], 5, 0)
    assert tab(order=P.ORDER_AREA) == ([0, 1, 4, 2, 0, 3, 5, 0], 5, 0)             # the tie 1, 3 by the smaller label
    assert tab(order=P.ORDER_RASTER) == ([0, 2, 1, 3, 0, 5, 4, 0], 5, 0)           # first pixels 17, 25, 68, 74, 124
    assert tab(order=P.ORDER_AREA, max_objects=2) == ([0, 1, 0, 2, 0, 0, 0, 0], 2, 3)
    assert tab(min_area=2, max_area=3) == ([0, 0, 1, 0, 0, 2, 0, 0], 2, 3)
    assert tab(clear_border=True, order=P.ORDER_AREA) == ([0, 1, 3, 2, 0, 0, 4, 0], 4, 1)
    assert tab(min_area=0) == tab(min_area=1)
    t, _, _ = P.select(acc, h, w, order=P.ORDER_AREA)
    out = P.relabel(lab[None], t)[0]
    assert out.dtype == np.uint8 and np.array_equal(out == 2, lab == 3) and np.array_equal(out == 0, lab == 0)
    areas = np.bincount(out.reshape(-1), minlength=6)[1:]
    assert areas.tolist() == [4, 4, 3, 2, 1]
