"""CPU-only: the sequential restatement tests/contours_np.py against the invariants the definitions promise (every edge on
one cycle, the area identity, edge count = crack perimeter, outer contours = scipy's components, holes = enclosed
components of the complement under the dual connectivity), against hand-written answers, and through an even-odd fill
back to the map."""
import os
import sys

import numpy as np
import pytest
from scipy import ndimage

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__))]
import contours_np as C   # noqa: E402
import props_np as P      # noqa: E402

FULL = np.ones((3, 3), int)
CROSS = ndimage.generate_binary_structure(2, 1)


def structure(connectivity):
    return FULL if connectivity == 8 else CROSS


def M(rows):
    return np.array(rows, np.uint8)


def random_maps(count, seed):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        h, w = rng.integers(1, 13, 2)
        k = int(rng.integers(1, 4))
        yield (rng.integers(0, k + 1, (h, w)) * (rng.random((h, w)) < rng.uniform(0.3, 1.0))).astype(np.uint8)


@pytest.mark.parametrize("connectivity", (4, 8))
def test_invariants_on_random_maps(connectivity):
    for m in random_maps(300, connectivity):
        cs = C.contours(m, connectivity)                     # asserts one successor and one predecessor per edge
        assert sum(c["edges"] for c in cs) == len(C.edges(m))
        assert [c["start"] for c in cs] == sorted(c["start"] for c in cs)
        h, w = m.shape
        if (h * w) % 4 == 0:
            acc, _ = P.label_props(m[None], None, 256)
        for v in range(1, int(m.max()) + 1):
            mine = [c for c in cs if c["label"] == v]
            assert sum(c["area2"] for c in mine) == 2 * int((m == v).sum())
            if (h * w) % 4 == 0:
                assert sum(c["edges"] for c in mine) == int(acc[0, v, 10])
            outer = sum(c["area2"] > 0 for c in mine)
            holes = sum(c["area2"] < 0 for c in mine)
            assert outer + holes == len(mine)
            assert outer == ndimage.label(m == v, structure(connectivity))[1]
            padded = np.pad(m != v, 1, constant_values=True)
            assert holes == ndimage.label(padded, structure(12 - connectivity))[1] - 1
            topo = C.topology(*C.trace(m[None], connectivity, 64, 1024)[::2], 4)
            assert topo[0, v].tolist() == [outer, holes, outer - holes]


def test_one_pixel():
    (c,) = C.contours(M([[0, 0, 0], [0, 5, 0], [0, 0, 0]]), 8)
    assert c["verts"] == [(1, 1), (2, 1), (2, 2), (1, 2)] and c["area2"] == 2 and c["edges"] == 4
    assert c["label"] == 5 and c["start"] == (1 * 4 + 1) * 4 + C.E and c["pixel"] == 4


def test_rectangle_2x3():
    m = np.zeros((4, 5), np.uint8)
    m[1:3, 1:4] = 1
    for conn in (4, 8):
        (c,) = C.contours(m, conn)
        assert len(c["verts"]) == 4 and c["edges"] == 10 and c["area2"] == 12
        assert c["verts"] == [(1, 1), (4, 1), (4, 3), (1, 3)]


def test_ring_3x3():
    m = M([[1, 1, 1], [1, 0, 1], [1, 1, 1]])
    for conn in (4, 8):
        outer, hole = C.contours(m, conn)
        assert outer["area2"] == 18 and hole["area2"] == -2 and len(hole["verts"]) == 4
        table, _, counts = C.trace(m[None], conn, 4, 16)
        assert C.topology(table, counts, 2)[0, 1].tolist() == [1, 1, 0]


def test_two_diagonal_pixels():
    m = M([[1, 0], [0, 1]])
    (c,) = C.contours(m, 8)
    assert c["edges"] == 8 and len(c["verts"]) == 8 and c["verts"].count((1, 1)) == 2 and c["area2"] == 4
    a, b = C.contours(m, 4)
    assert a["edges"] == b["edges"] == 4 and a["area2"] == b["area2"] == 2


def test_plus_sign():
    m = M([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    for conn in (4, 8):
        (c,) = C.contours(m, conn)
        assert len(c["verts"]) == 12 and c["edges"] == 12 and c["area2"] == 10


def nested():
    m = np.zeros((9, 9), np.uint8)
    m[0:9, 0:9] = 1
    m[1:8, 1:8] = 0
    m[2:7, 2:7] = 2
    m[3:6, 3:6] = 0
    m[4, 4] = 1
    return m


def test_nested_rings_and_island():
    m = nested()
    for conn in (4, 8):
        table, _, counts = C.trace(m[None], conn, 16, 64)
        topo = C.topology(table, counts, 3)
        assert topo[0, 1].tolist() == [2, 1, 1] and topo[0, 2].tolist() == [1, 1, 0]
    m[4, 4] = 0
    topo = C.topology(*C.trace(m[None], 8, 16, 64)[::2], 3)
    assert topo[0, 1].tolist() == [1, 1, 0] and topo[0, 2].tolist() == [1, 1, 0]
    m[2:7, 2:7] = 0
    m[4, 4] = 2
    topo = C.topology(*C.trace(m[None], 8, 16, 64)[::2], 3)
    assert topo[0, 1, 2] == 0 and topo[0, 2, 2] == 1                       # island in hole in ring: Euler 0 and 1


def test_overflow_keeps_the_first_rows_and_whole_contours():
    m = M([[1, 0, 2, 0], [0, 0, 0, 0], [3, 3, 0, 4]])
    full_t, full_v, full_c = C.trace(m[None], 8, 8, 32)
    assert full_c[0].tolist() == [4, 16, 0, 0]
    t, v, c = C.trace(m[None], 8, 3, 32, table=np.full((1, 3, 8), -7, np.int64), verts=np.full((1, 32, 2), -7, np.int16))
    assert c[0].tolist() == [4, 16, 1, 0] and np.array_equal(t[0], full_t[0, :3])
    assert np.array_equal(v[0, :12], full_v[0, :12]) and (v[0, 12:] == -7).all()
    t, v, c = C.trace(m[None], 8, 8, 15, verts=np.full((1, 15, 2), -7, np.int16))
    assert c[0].tolist() == [4, 16, 0, 1] and np.array_equal(t[0, :4], full_t[0, :4])
    assert np.array_equal(v[0, :12], full_v[0, :12]) and (v[0, 12:] == -7).all()


@pytest.mark.parametrize("connectivity", (4, 8))
def test_even_odd_fill_gives_the_map_back(connectivity):
    maps = list(random_maps(40, 100 + connectivity)) + [nested(), M([[1, 0], [0, 1]])]
    for m in maps:
        polys = C.polygons(m, connectivity)
        assert np.array_equal(C.rasterise(polys, *m.shape), m)
        assert len(polys) == sum(ndimage.label(m == v, structure(connectivity))[1] for v in range(1, int(m.max()) + 1))
        for p in polys:
            assert p["outer"].dtype == np.int16 and p["outer"].shape[1] == 2
