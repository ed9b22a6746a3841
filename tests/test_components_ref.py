"""CPU-only: the restatement tests/components_np.py (the reference of every GPU test of the connected-component kernels)
against scipy.ndimage.label, and against hand-written maps whose answers are spelled out here."""
import os
import sys

import numpy as np
import pytest

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import components_np as cnp  # noqa: E402

M = np.array([[1, 1, 0, 2, 2, 0, 0, 3],
              [1, 0, 0, 0, 2, 0, 3, 0],
              [0, 0, 1, 0, 0, 0, 0, 0],
              [0, 1, 1, 0, 2, 2, 0, 0],
              [0, 0, 0, 0, 0, 0, 0, 3],
              [4, 0, 0, 0, 0, 0, 0, 3]], np.uint8)[None]
# components at connectivity 8, by root pixel: A = 0 (value 1, area 3), C = 3 (value 2, area 3), E = 7 (value 3, area 2: a
# diagonal pair), B = 18 (value 1, area 3), D = 28 (value 2, area 2), F = 39 (value 3, area 2), G = 40 (value 4, area 1)
COMP8 = np.array([[1, 1, 0, 4, 4, 0, 0, 8],
                  [1, 0, 0, 0, 4, 0, 8, 0],
                  [0, 0, 19, 0, 0, 0, 0, 0],
                  [0, 19, 19, 0, 29, 29, 0, 0],
                  [0, 0, 0, 0, 0, 0, 0, 40],
                  [41, 0, 0, 0, 0, 0, 0, 40]], np.int32)[None]
COMP4 = COMP8.copy()
COMP4[0, 1, 6] = 15                                  # the diagonal pair E falls apart at connectivity 4


def relabel(comp, table):
    out = np.zeros(comp.shape, np.uint8)
    for root, lab in table.items():
        out[comp == root + 1] = lab
    return out


def test_hand_written_components():
    comp, n = cnp.label(M, 8)
    assert np.array_equal(comp, COMP8) and n.tolist() == [7] and comp.dtype == np.int32
    comp, n = cnp.label(M, 4)
    assert np.array_equal(comp, COMP4) and n.tolist() == [8]


@pytest.mark.parametrize("min_area,max_objects,table,count,dropped", [
    (0, 255, {0: 1, 3: 2, 7: 3, 18: 4, 28: 5, 39: 6, 40: 7}, 7, 0),
    (1, 255, {0: 1, 3: 2, 7: 3, 18: 4, 28: 5, 39: 6, 40: 7}, 7, 0),
    (2, 255, {0: 1, 3: 2, 7: 3, 18: 4, 28: 5, 39: 6}, 6, 0),          # at the area of D, E, F; above G's
    (3, 255, {0: 1, 3: 2, 18: 3}, 3, 0),                             # at the area of A, B, C; above the pairs'
    (4, 255, {}, 0, 0),
    (1, 2, {0: 1, 3: 2}, 2, 5),                                      # the cap: raster order, the rest counted in dropped
])
def test_hand_written_split(min_area, max_objects, table, count, dropped):
    out, c, d = cnp.split(M, COMP8, min_area, max_objects)
    assert np.array_equal(out, relabel(COMP8, table)) and c.tolist() == [count] and d.tolist() == [dropped]


@pytest.mark.parametrize("min_area,max_objects,table,count,dropped", [
    # value 1: A and B tie at area 3, the smaller root A wins; value 3: E and F tie at 2, E wins
    (1, 255, {0: 1, 3: 2, 7: 3, 40: 4}, 4, 3),
    (2, 255, {0: 1, 3: 2, 7: 3}, 3, 3),              # value 4's winner G fails; A B C D E F qualify, three of them lost
    (3, 255, {0: 1, 3: 2}, 2, 1),                    # value 3's winner fails as well; A B C qualify, B lost
    (4, 255, {}, 0, 0),
    (1, 3, {0: 1, 3: 2, 7: 3}, 3, 4),                # the cap cuts the survivor of value 4
])
def test_hand_written_largest(min_area, max_objects, table, count, dropped):
    out, c, d = cnp.largest(M, COMP8, min_area, max_objects)
    assert np.array_equal(out, relabel(COMP8, table)) and c.tolist() == [count] and d.tolist() == [dropped]


def test_largest_renumbers_over_a_value_that_fails():
    m = np.array([[1, 1, 0, 2], [0, 0, 0, 0], [3, 3, 3, 0]], np.uint8)[None]
    comp, n = cnp.label(m, 8)
    assert n.tolist() == [3]
    out, c, d = cnp.largest(m, comp, 2, 255)
    assert np.array_equal(out[0], [[1, 1, 0, 0], [0, 0, 0, 0], [2, 2, 2, 0]]) and c.tolist() == [2] and d.tolist() == [0]
    # the bigger fragment wins whatever its position
    m = np.array([[5, 0, 5, 5], [0, 0, 0, 0], [5, 5, 5, 0]], np.uint8)[None]
    comp, _ = cnp.label(m, 4)
    out, c, d = cnp.largest(m, comp, 1, 255)
    assert np.array_equal(out[0], [[0, 0, 0, 0], [0, 0, 0, 0], [1, 1, 1, 0]]) and c.tolist() == [1] and d.tolist() == [2]


def test_split_cap_at_255():
    m = np.zeros((1, 40, 64), np.uint8)
    m[0, ::2, ::2] = 9                               # 20 x 32 = 640 isolated pixels
    comp, n = cnp.label(m, 8)
    assert n.tolist() == [640]
    out, c, d = cnp.split(m, comp, 1, 255)
    rank = np.arange(640).reshape(20, 32)
    want = np.zeros((40, 64), np.uint8)
    want[::2, ::2] = np.where(rank < 255, rank + 1, 0)
    assert np.array_equal(out[0], want) and c.tolist() == [255] and d.tolist() == [385]


def test_no_wrap_and_no_leak_between_images():
    m = np.zeros((2, 4, 8), np.uint8)
    m[0, :, 7] = 1                                   # the last column ..
    m[0, 1:, 0] = 1                                  # .. and the first column of the following rows
    m[1] = m[0]
    comp, n = cnp.label(m, 8)
    assert n.tolist() == [2, 2] and np.array_equal(comp[0], comp[1])
    assert set(np.unique(comp[0])) == {0, 8, 9}


def test_restatement_matches_scipy():
    ndimage = pytest.importorskip("scipy").ndimage
    rng = np.random.default_rng(0)
    structure = {4: ndimage.generate_binary_structure(2, 1), 8: ndimage.generate_binary_structure(2, 2)}
    cases = [(rng.random((2, 37, 52)) < d).astype(np.uint8) for d in (0.30, 0.41, 0.50, 0.59)]
    cases.append(rng.integers(0, 6, (2, 41, 48)).astype(np.uint8))
    cases.append((rng.random((1, 512, 512)) < 0.59).astype(np.uint8))
    for maps in cases:
        for conn in (4, 8):
            comp, n = cnp.label(maps, conn)
            for b, img in enumerate(maps):
                want = np.zeros(img.shape, np.int64)
                total = 0
                for v in np.unique(img[img > 0]):    # scipy joins any non-zero pixels: one value at a time
                    lab, k = ndimage.label(img == v, structure[conn])
                    want += np.where(lab > 0, lab + total, 0)
                    total += k
                assert n[b] == total
                # the same partition: the pairs (ours, scipy's) are a bijection
                pairs = np.unique(np.stack([comp[b].reshape(-1), want.reshape(-1)]), axis=1)
                assert pairs.shape[1] == len(np.unique(comp[b])) == len(np.unique(want))
                # canonical: a component's value is 1 + the index of its first pixel
                values, first = np.unique(comp[b].reshape(-1), return_index=True)
                assert np.array_equal(values[values > 0] - 1, first[values > 0])
