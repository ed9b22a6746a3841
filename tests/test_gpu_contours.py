"""Tracing outlines on the GPU: isa_contour_trace / isa_contour_topology, ReSeg.contours / instance_topology / polygons,
Model.predict_polygons, pred_list.py --polygons.

Everything is an integer: table, verts, counts and topo are compared EXACTLY, and over their whole buffers, with the
sequential restatement tests/contours_np.py (which tests/test_contours_ref.py checks against scipy and hand-written
answers).  The buffers are handed in filled with a sentinel and sit between sentinel pads, and the restatement starts from
the same fill: a row or vertex past the counts that the entry touched, or anything written outside, is a difference.  The
capacities are exactly what each batch needs unless a test says otherwise.

Shapes.  The scans work on blocks of 1024 lattice points ((h+1) * (w+1) of them) and of 1024 edges, the jumping rounds on
all edges: 4 x 4 and 8 x 12 (one block, 25 and 117 points), 64 x 64 (5 blocks of points, up to 16 of edges) with n = 1, 3, 16,
72 x 136 (10 blocks of points, the last one ragged, up to 39 of edges), 256 x 256 with n = 2 (65 blocks of points, at most
256 of edges: one trip of the per-image scans of the block sums, 256 blocks a trip), and 520 x 520 (266 blocks of points:
a second trip; with four edges a pixel 1057 blocks of edges: five trips) against answers written by hand.  There is one
load path; the map is still traced once from a pointer 4 bytes off a 16-byte boundary."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import contours_np as C         # noqa: E402
import props_np as P            # noqa: E402
import reseg_ref as R           # noqa: E402
from test_gpu_ops import _gpu   # noqa: E402
from test_gpu_props import Padded, blobs, build, dev_map, dev_props, edge_blobs, same   # noqa: E402

FILL = -77
_found = {}


def _lib():
    L = _gpu()[0]
    return L, L.lib()


def found(maps, conn):
    """[C.contours(image, conn)] of a batch, computed once per batch and connectivity and never changed."""
    key = (maps.shape, maps.tobytes(), conn)
    if key not in _found:
        _found[key] = [C.contours(m, conn) for m in maps]
    return _found[key]


def needed(maps, conn):
    cs = found(maps, conn)
    return max(1, max(len(c) for c in cs)), max(1, max(sum(len(k["verts"]) for k in c) for c in cs))


def want_trace(maps, conn, cmax, vmax):
    n = maps.shape[0]
    return C.trace(maps, conn, cmax, vmax, table=np.full((n, cmax, 8), FILL, np.int64),
                   verts=np.full((n, vmax, 2), FILL, np.int16), found=found(maps, conn))


def dev_trace(maps, conn, cmax, vmax, offset=0, nl=256):
    """isa_contour_trace + isa_contour_topology -> (table, verts, counts, topo) as numpy, pads checked."""
    L, lib = _lib()
    n, h, w = maps.shape
    t = dev_map(maps, offset)
    table, verts = Padded((n, cmax, 8), torch.int64, FILL), Padded((n, vmax, 2), torch.int16, FILL)
    counts, topo = Padded((n, 4), torch.int32, FILL), Padded((n, nl, 3), torch.int32, FILL)
    scratch = torch.empty((L.contour_scratch_bytes(n, h, w) + 64,), dtype=torch.uint8, device="cuda")
    scratch[-64:] = 0xA5
    L.check(lib.isa_contour_trace(t, n, h, w, conn, cmax, vmax, table.view, verts.view, counts.view, scratch,
                                  scratch.numel() - 64, L.stream_ptr()), "isa_contour_trace")
    L.check(lib.isa_contour_topology(table.view, counts.view, n, cmax, nl, topo.view, L.stream_ptr()), "isa_contour_topology")
    assert bool((scratch[-64:] == 0xA5).all()), "written past the scratch"
    return table.host(), verts.host(), counts.host(), topo.host()


def check(maps, what, conns=(4, 8), offset=0):
    """Every output against the restatement at exactly the capacities the batch needs, and the sums per label against
    the perimeter and area slots of isa_label_props on the same map (which equal the measuring restatement's)."""
    maps = np.ascontiguousarray(maps, dtype=np.uint8)
    n, h, w = maps.shape
    acc = dev_props(maps)[0]
    same(acc, P.label_props(maps, None, 256)[0], what + ": isa_label_props")
    for conn in conns:
        tag = "%s, connectivity %d" % (what, conn)
        cmax, vmax = needed(maps, conn)
        table, verts, counts, topo = dev_trace(maps, conn, cmax, vmax, offset)
        wt, wv, wc = want_trace(maps, conn, cmax, vmax)
        same(counts, wc, tag + ": counts")
        same(table, wt, tag + ": table")
        same(verts, wv, tag + ": verts")
        same(topo, C.topology(wt, wc, 256), tag + ": topo")
        for i in range(n):
            rows = table[i, :counts[i, 0]]
            for col, slot, times in ((3, 10, 1), (4, 0, 2)):
                sums = np.bincount(rows[:, 0], weights=rows[:, col], minlength=256).astype(np.int64)
                same(sums[1:], times * acc[i, 1:, slot], "%s, image %d: column %d per label" % (tag, i, col))
    return found(maps, 4), found(maps, 8)


# ---- contents -----------------------------------------------------------------------------------------------------------
def spiral(h, w):
    """A one-pixel-wide arm of label 1 that winds inwards with one pixel of background between its turns."""
    m = np.zeros((h, w), dtype=np.uint8)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    while True:
        for _ in range(2):
            ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < h and 0 <= nx < w and not m[ny, nx] and not (0 <= fy < h and 0 <= fx < w and m[fy, fx]):
                y, x = ny, nx
                m[y, x] = 1
                break
            dy, dx = dx, -dy
        else:
            return m


def rings(h, w):
    """Nested one-pixel rectangular rings of labels 1, 2, 1, 2, .. with one pixel of background between them, down to the
    centre: every ring but the innermost has a hole, and every hole but the innermost holds the next ring."""
    m = np.zeros((h, w), dtype=np.uint8)
    for k in range((min(h, w) + 1) // 2):
        m[k:h - k, k:w - k] = k // 2 % 2 + 1 if k % 2 == 0 else 0
    return m


def saddles(h, w):
    """2 x 2 checkers of pixels: every inner lattice point is a saddle, of labels 1 and 2 against 0 and against each other."""
    yy, xx = np.mgrid[:h, :w]
    m = ((yy + xx) % 2).astype(np.uint8)
    m[(yy + xx) % 2 == 0] = 0
    m[((yy + xx) % 2 == 1) & (yy % 4 < 2)] = 1
    m[((yy + xx) % 2 == 1) & (yy % 4 >= 2)] = 2
    m[(yy % 3 == 0) & ((yy + xx) % 2 == 0)] = 2
    return m


def patterns(h, w):
    yy, xx = np.mgrid[:h, :w]
    every = ((yy // 2 * ((w + 1) // 2) + xx // 2) % 255 + 1).astype(np.uint8)     # 1..255 all present from 32 x 32 on
    return {
        "all background": np.zeros((h, w), dtype=np.uint8),
        "one label everywhere": np.full((h, w), 7, dtype=np.uint8),
        "checkerboard against 0": ((yy + xx) % 2 * 9).astype(np.uint8),
        "three labels, four edges a pixel": ((xx + 2 * yy) % 3 + 1).astype(np.uint8),
        "spiral": spiral(h, w),
        "labels 1..255": every,
        "edge blobs": edge_blobs(h, w),
        "blobs over noise": blobs(h, w, h * 1000 + w, noise=0.1),
        "nested rings": rings(h, w),
        "saddle corners": saddles(h, w),
    }


SMALL = [(4, 4), (8, 12), (64, 64), (72, 136)]


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "%dx%d" % s)
def test_patterns(shape):
    h, w = shape
    pats = patterns(h, w)
    for name, lab in pats.items():
        f4, f8 = check(lab[None], "%s %dx%d" % (name, h, w))
        if name == "all background":
            assert not f4[0] and not f8[0]
        elif name == "one label everywhere":
            for f in (f4, f8):
                assert len(f[0]) == 1 and len(f[0][0]["verts"]) == 4 and f[0][0]["edges"] == 2 * (h + w)
        elif name == "checkerboard against 0":
            assert len(f4[0]) == h * w // 2 and all(c["area2"] == 2 for c in f4[0])
            assert sum(c["area2"] > 0 for c in f8[0]) == 1                            # one component, the rest are holes
        elif name == "three labels, four edges a pixel":
            assert sum(c["edges"] for c in f4[0]) == 4 * h * w == sum(c["edges"] for c in f8[0]) and len(f4[0]) == h * w
        elif name == "spiral":
            assert len(f4[0]) == len(f8[0]) == 1 and f4[0][0]["edges"] == f8[0][0]["edges"] >= h * w * 3 // 4
        elif name == "labels 1..255" and h * w >= 32 * 32:
            assert {c["label"] for c in f8[0]} == set(range(1, 256))


def test_pointer_off_a_16_byte_boundary():
    check(np.stack([patterns(8, 12)["blobs over noise"], patterns(8, 12)["saddle corners"]]), "offset 4", offset=4)


@pytest.mark.parametrize("n", (1, 3, 16))
def test_batches_of_64x64(n):
    maps = np.stack([blobs(64, 64, 50 + i, k=4 + i % 5, noise=0.1) for i in range(n)])
    if n > 1:
        maps[n - 1] = 0                                           # an image without instances among the others
        maps[n - 2] = spiral(64, 64)                              # and the longest cycle next to short ones
    check(maps, "blobs n=%d" % n)


def test_256x256_two_images():
    """The spiral's cycle has about 256 * 256 = 4^8 edges: it needs 8 or 9 of the 9 rounds that 4 h w = 4^9 gives."""
    maps = np.stack([blobs(256, 256, 5, k=12, noise=0.05), spiral(256, 256)])
    f4, f8 = check(maps, "256x256")
    assert f8[1][0]["edges"] > 1 << 15 and len(f8[0]) > 500


# ---- past one trip of the one-workgroup scans --------------------------------------------------------------------------------
# The per-image scans of the block sums take 256 blocks a trip.  520 x 520 has 521^2 lattice points = 266 point blocks, so the
# point-block scan takes a second trip; the edge-block scan takes one per 256 * 1024 edges the map really has.
def hand_rows(items, w):
    """[(table row, its four vertices)] in ascending key order, written out by hand: items are ("outer", label, x0, y0, a, b)
    for a rectangle a wide and b high with top-left corner (x0, y0), and ("hole", ...) for such a hole in that label.  An
    outer contour starts with the E edge at its top-left corner and runs clockwise (y points down): 4 vertices, crack
    length 2 (a + b), twice-area +2 a b, owner pixel (x0, y0).  A hole starts with the S edge at its top-left corner,
    owned by the pixel left of it, and runs the other way: twice-area -2 a b."""
    out = []
    for kind, v, x0, y0, a, b in items:
        pt = y0 * (w + 1) + x0
        if kind == "outer":
            row = [v, 0, 4, 2 * (a + b), 2 * a * b, pt * 4 + C.E, y0 * w + x0, 0]
            vs = [(x0, y0), (x0 + a, y0), (x0 + a, y0 + b), (x0, y0 + b)]
        else:
            row = [v, 0, 4, 2 * (a + b), -2 * a * b, pt * 4 + C.S, y0 * w + x0 - 1, 0]
            vs = [(x0, y0), (x0, y0 + b), (x0 + a, y0 + b), (x0 + a, y0)]
        out.append((row, vs))
    out.sort(key=lambda rv: rv[0][5])
    for i, (row, _) in enumerate(out):
        row[1] = 4 * i
    return out


def test_520x520_rectangles_second_trip_of_the_block_scan():
    """Five rectangles of distinct labels on 520 x 520: one at the origin, one that touches the far corner (its points lie
    in the blocks of the scan's second trip), one with a rectangular hole and one inside that hole.  Answers by hand, the
    restatement as well, both connectivities (nothing touches diagonally: they agree), and a repeat that is bit-identical."""
    h = w = 520
    m = np.zeros((h, w), np.uint8)
    items = [("outer", 1, 0, 0, 8, 4), ("outer", 2, 300, 48, 16, 20), ("outer", 3, 100, 200, 40, 30),
             ("hole", 3, 110, 210, 10, 6), ("outer", 4, 112, 212, 4, 2), ("outer", 5, w - 12, h - 8, 12, 8)]
    for kind, v, x0, y0, a, b in items:
        m[y0:y0 + b, x0:x0 + a] = v if kind == "outer" else 0
    assert m[h - 1, w - 1] == 5 and m[210, 110] == 0 and m[212, 112] == 4
    assert (h + 1) * (w + 1) > 256 * 1024 and 4 * h * w > 256 * 1024
    rows = hand_rows(items, w)
    wt = np.array([[r for r, _ in rows]], np.int64)
    wv = np.array([[p for _, vs in rows for p in vs]], np.int16)
    wc = np.array([[6, 24, 0, 0]], np.int32)
    wtopo = np.zeros((1, 256, 3), np.int32)
    wtopo[0, [1, 2, 4, 5]] = (1, 0, 1)
    wtopo[0, 3] = (1, 1, 0)                                       # Euler number 0: one component, one hole
    maps = m[None]
    for conn in (4, 8):
        tag = "rectangles 520x520, connectivity %d" % conn
        got = dev_trace(maps, conn, 6, 24)
        for g, want, part in zip(got, (wt, wv, wc, wtopo), ("table", "verts", "counts", "topo")):
            same(g, want, "%s: %s by hand" % (tag, part))
        rt, rv, rc = want_trace(maps, conn, 6, 24)
        for g, want, part in zip(got, (rt, rv, rc, C.topology(rt, rc, 256)), ("table", "verts", "counts", "topo")):
            same(g, want, "%s: %s" % (tag, part))
        again = dev_trace(maps, conn, 6, 24)
        assert all(np.array_equal(a, b) for a, b in zip(got, again)), tag + ": the repeat differs"


def test_520x520_four_edges_a_pixel_five_trips_of_the_edge_block_scan():
    """(x + 2 y) % 3 + 1: every pixel differs from its four neighbours, so under 4-connectivity every pixel is a contour of
    its own and the map has all 4 h w = 1 081 600 edges the bound allows: 1057 edge blocks, five trips of the scan that gives
    every contour its row and vertex offset.  Answers by hand (test_patterns holds the same pattern against the restatement
    at small sizes): row r is pixel r in raster order, a unit square from its top-left corner."""
    h = w = 520
    yy, xx = np.mgrid[:h, :w]
    m = ((xx + 2 * yy) % 3 + 1).astype(np.uint8)
    px = np.arange(h * w, dtype=np.int64)
    y, x = px // w, px % w
    wt = np.stack([m.reshape(-1).astype(np.int64), 4 * px, np.full_like(px, 4), np.full_like(px, 4), np.full_like(px, 2),
                   (y * (w + 1) + x) * 4, px, np.zeros_like(px)], axis=1)[None]
    wv = np.stack([np.stack([x, x + 1, x + 1, x], axis=1), np.stack([y, y, y + 1, y + 1], axis=1)], axis=2)
    wv = wv.reshape(1, 4 * h * w, 2).astype(np.int16)
    wc = np.array([[h * w, 4 * h * w, 0, 0]], np.int32)
    assert 4 * h * w > 4 * 256 * 1024
    got = dev_trace(m[None], 4, h * w, 4 * h * w, nl=4)
    wtopo = np.zeros((1, 4, 3), np.int32)
    wtopo[0, 1:, 0] = wtopo[0, 1:, 2] = np.bincount(m.reshape(-1), minlength=4)[1:]
    for g, want, part in zip(got, (wt, wv, wc, wtopo), ("table", "verts", "counts", "topo")):
        same(g, want, "four edges a pixel 520x520: " + part)


# ---- overflow -----------------------------------------------------------------------------------------------------------
def test_overflow_keeps_the_first_rows_and_whole_contours():
    maps = np.stack([blobs(64, 64, 11, noise=0.1), edge_blobs(64, 64), np.zeros((64, 64), np.uint8)])
    for conn in (4, 8):
        cmax, vmax = needed(maps, conn)
        full = want_trace(maps, conn, cmax, vmax)
        for dc, dv in ((1, 0), (0, 1), (1, 1), (cmax - 1, 0), (0, vmax - 1)):
            c, v = cmax - dc, vmax - dv
            table, verts, counts, _ = dev_trace(maps, conn, c, v)
            wt, wv, wc = want_trace(maps, conn, c, v)
            tag = "cmax - %d, vmax - %d, connectivity %d" % (dc, dv, conn)
            same(counts, wc, tag + ": counts")
            same(table, wt, tag + ": table")
            same(verts, wv, tag + ": verts")
            assert (counts[:, 2] > 0).any() == (dc > 0) and (counts[:, 3] > 0).any() == (dv > 0), tag
            same(counts[:, :2], full[2][:, :2], tag + ": what was found does not depend on the capacities")
            for i in range(3):
                k = min(int(counts[i, 0]), c)
                same(table[i, :k], full[0][i, :k], tag + ": the rows kept are the first ones")
                assert (table[i, k:] == FILL).all(), tag


def test_reseg_contours_check_raises_on_overflow():
    m = build()
    lab = np.stack([blobs(64, 64, 11, noise=0.02), edge_blobs(64, 64)])
    labels = torch.from_numpy(lab).cuda()
    cmax, vmax = needed(lab, 8)
    table, verts, counts = m.contours(labels, max_contours=cmax, max_vertices=vmax)
    assert table.is_cuda and verts.is_cuda and counts.is_cuda
    assert (table.dtype, verts.dtype, counts.dtype) == (torch.int64, torch.int16, torch.int32)
    assert tuple(table.shape) == (2, cmax, 8) and tuple(verts.shape) == (2, vmax, 2) and tuple(counts.shape) == (2, 4)
    wt, wv, wc = want_trace(lab, 8, cmax, vmax)
    same(counts.cpu().numpy(), wc, "contours: counts")
    for i in range(2):
        same(table[i, :wc[i, 0]].cpu().numpy(), wt[i, :wc[i, 0]], "contours: table")
        same(verts[i, :wc[i, 1]].cpu().numpy(), wv[i, :wc[i, 1]], "contours: verts")
    for kw in (dict(max_contours=cmax - 1, max_vertices=vmax), dict(max_contours=cmax, max_vertices=vmax - 1)):
        with pytest.raises(ValueError):
            m.contours(labels, **kw)
        _, _, c = m.contours(labels, check=False, **kw)
        assert c is m.last_contour_counts
        same(c.cpu().numpy(), want_trace(lab, 8, kw["max_contours"], kw["max_vertices"])[2], "last_contour_counts")
    t4, _, c4 = m.contours(labels, connectivity=4)                # the default capacities hold these maps
    w4 = needed(lab, 4)
    assert tuple(t4.shape) == (2, 256, 8) and int(c4[:, 2:].sum()) == 0 and int(c4[:, 0].max()) == w4[0]
    with pytest.raises(ValueError):
        m.contours(labels, connectivity=6)
    with pytest.raises(TypeError):
        m.contours(labels.int())
    with pytest.raises(ValueError):
        m.contours(labels[:, :, :62])


# ---- determinism, graphs ---------------------------------------------------------------------------------------------------
def test_ten_repeats_are_bit_identical():
    maps = np.stack([blobs(256, 256, 70, k=30, noise=0.2), blobs(256, 256, 71, k=30, noise=0.2)])
    first = None
    for _ in range(10):
        got = dev_trace(maps, 8, 2048, 16384)
        first = first or got
        assert all(np.array_equal(a, b) for a, b in zip(first, got))
    assert (first[2][:, 2:] == 0).all() and (first[2][:, 0] > 500).all()


def test_graph_replay_follows_new_contents():
    """isa_contour_trace + isa_contour_topology captured in one graph: no host read, a launch count fixed by the shape, no
    buffer that the caller clears - replayed twice on new contents it gives the new answers."""
    L, lib = _lib()
    n, h, w, cmax, vmax = 2, 64, 64, 1024, 8192
    t = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    table = torch.empty((n, cmax, 8), dtype=torch.int64, device="cuda")
    verts = torch.empty((n, vmax, 2), dtype=torch.int16, device="cuda")
    counts = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    topo = torch.empty((n, 256, 3), dtype=torch.int32, device="cuda")
    scratch = torch.empty((L.contour_scratch_bytes(n, h, w),), dtype=torch.uint8, device="cuda")

    def call():
        st = L.stream_ptr()
        L.check(lib.isa_contour_trace(t, n, h, w, 8, cmax, vmax, table, verts, counts, scratch, scratch.numel(), st),
                "isa_contour_trace")
        L.check(lib.isa_contour_topology(table, counts, n, cmax, 256, topo, st), "isa_contour_topology")

    t.copy_(torch.from_numpy(np.stack([blobs(h, w, 30 + i) for i in range(n)])))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for seed in (41, 43):
        maps = np.stack([blobs(h, w, seed, k=3 + seed % 5, noise=0.1), (spiral(h, w) * (seed % 7)).astype(np.uint8)])
        t.copy_(torch.from_numpy(maps))
        table.fill_(FILL), verts.fill_(FILL), counts.fill_(FILL), topo.fill_(FILL), scratch.fill_(seed)
        g.replay()
        torch.cuda.synchronize()
        wt, wv, wc = want_trace(maps, 8, cmax, vmax)
        for got, want, part in ((counts, wc, "counts"), (table, wt, "table"), (verts, wv, "verts"),
                                (topo, C.topology(wt, wc, 256), "topo")):
            same(got.cpu().numpy(), want, "replay %d: %s" % (seed, part))


# ---- end to end ---------------------------------------------------------------------------------------------------------
def components_per_label(m, labels, conn):
    comp, _ = m.components(labels, connectivity=conn)
    comp, lab = comp.cpu().numpy(), labels.cpu().numpy()
    out = np.zeros((lab.shape[0], 256), np.int32)
    for i in range(lab.shape[0]):
        for v in np.unique(lab[i][lab[i] > 0]):
            out[i, v] = len(np.unique(comp[i][lab[i] == v]))
    return out


def test_instance_topology_and_polygons():
    m = build()
    lab = np.stack([blobs(64, 64, 21, k=5, noise=0.1), rings(64, 64), patterns(64, 64)["checkerboard against 0"],
                    np.zeros((64, 64), np.uint8)])
    labels = torch.from_numpy(lab).cuda()
    for conn in (4, 8):
        cmax, vmax = needed(lab, conn)
        wt, _, wc = want_trace(lab, conn, cmax, vmax)
        topo = m.instance_topology(labels, connectivity=conn)
        assert topo.is_cuda and topo.dtype == torch.int32 and tuple(topo.shape) == (4, 256, 3)
        same(topo.cpu().numpy(), C.topology(wt, wc, 256), "instance_topology %d" % conn)
        same(topo[:, :, 0].cpu().numpy(), components_per_label(m, labels, conn), "outer contours = components %d" % conn)
        small = m.instance_topology(labels, connectivity=conn, n_labels=4)
        same(small.cpu().numpy(), C.topology(wt, wc, 4), "instance_topology %d, n_labels 4" % conn)
        polys = m.polygons(labels, connectivity=conn)
        assert len(polys) == 4 and polys[3] == []
        for i in range(4):
            want = C.polygons(lab[i], conn)
            assert len(polys[i]) == len(want), (conn, i)
            for got, ref in zip(polys[i], want):
                assert got["label"] == ref["label"] and len(got["holes"]) == len(ref["holes"])
                same(got["outer"], ref["outer"], "polygons %d image %d: outer" % (conn, i))
                for a, b in zip(got["holes"], ref["holes"]):
                    same(a, b, "polygons %d image %d: hole" % (conn, i))
            same(C.rasterise(polys[i], 64, 64), lab[i], "even-odd fill of polygons %d image %d" % (conn, i))
    # the checkerboard has 2048 contours under 4-connectivity, more than the default 256 rows: traced twice, still right
    assert needed(lab, 4)[0] > m.contour_capacities(64, 64)[0]
    with pytest.raises(ValueError):
        m.instance_topology(labels, n_labels=257)


def test_model_defaults_run_nothing_new_and_predict_polygons_outlines_the_labels():
    _gpu()
    from isa_amd.model import Model
    x, sem, ins, n = R.synth_batch(2, 64, 64, seed=2)
    model = Model("CVPPP", "ReSeg", 2, 5, use_instance_segmentation=True)
    net = model.model

    def trap(*a, **k):
        raise AssertionError("the default arguments reached the contour code")

    new_code = [(net, "contours"), (net, "instance_topology"), (net, "polygons"), (net, "contour_trace"),
                (net, "contour_topology")]
    for obj, name in new_code:
        setattr(obj, name, trap)
    _, labels, count = model.predict_instances(x)
    res = model.evaluate([(x, sem, ins, n)])
    assert res["per_image"].shape[0] == 2
    with pytest.raises(AssertionError):
        model.predict_polygons(x)
    for obj, name in new_code:
        delattr(obj, name)                                                     # the class's methods again
    prob, lab, cnt, polys = model.predict_polygons(x)
    assert lab.shape == labels.shape and cnt.shape == count.shape and len(polys) == 2
    for b in range(2):
        same(C.rasterise(polys[b], 64, 64), lab[b].numpy(), "predict_polygons image %d" % b)
        assert {p["label"] for p in polys[b]} == set(np.unique(lab[b].numpy()).tolist()) - {0}


def ring_area2(ring):
    x, y = np.asarray(ring, np.int64).T
    return int((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())


def test_pred_list_polygons_json(tmp_path):
    """pred_list.py --instances --polygons writes <name>-polygons.json: the sizes and, per label, polygon areas (outer
    minus holes) equal to the pixel counts of the written model-resolution labels."""
    from PIL import Image
    _gpu()
    out = str(tmp_path / "polys")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "pred_list.py"), "--synthetic", "2", "--instances", "--polygons",
                        "--output", out], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = sorted(os.listdir(out))
    assert names == ["synthetic_%04d" % i for i in range(2)]
    for i, name in enumerate(names):
        d = os.path.join(out, name)
        assert {name + "-polygons.json", name + "-ins_mask_model.png", name + "-ins_mask.png"} <= set(os.listdir(d))
        doc = json.load(open(os.path.join(d, name + "-polygons.json")))
        assert [doc[k] for k in ("model_w", "model_h", "orig_w", "orig_h")] == [256, 256, 330, 300 + 7 * (i % 5)]
        model_lab = np.array(Image.open(os.path.join(d, name + "-ins_mask_model.png")))
        assert model_lab.shape == (256, 256) and model_lab.dtype == np.uint8
        area2 = np.zeros(256, np.int64)
        for p in doc["polygons"]:
            a = ring_area2(p["outer"])
            holes = [ring_area2(r_) for r_ in p["holes"]]
            assert a > 0 and all(t < 0 for t in holes)
            area2[p["label"]] += a + sum(holes)
        assert area2[0] == 0 and area2[1:].tolist() == (2 * np.bincount(model_lab.reshape(-1), minlength=256)[1:]).tolist()
        polys = [dict(label=p["label"], outer=np.array(p["outer"]), holes=[np.array(r_) for r_ in p["holes"]])
                 for p in doc["polygons"]]
        same(C.rasterise(polys, 256, 256), model_lab, "even-odd fill of %s" % name)
