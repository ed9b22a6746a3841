"""Sequential restatement of the contour definitions of include/isa_kernels.h (isa_contour_trace / isa_contour_topology)
in plain Python integers: one function per output, no vectorisation, nothing shared with the kernels.

Pixel (row y, column x) is the unit square (x, y) .. (x+1, y+1), y pointing down.  A side of a pixel of label v != 0 whose
4-neighbour holds another value or lies outside the image is one directed edge of v with the pixel on its right:
top E = 0, right S = 1, bottom W = 2, left N = 3.  key = ((y0 * (w + 1) + x0) * 4 + dir) of the start point (x0, y0)."""
import numpy as np

E, S, W, N = 0, 1, 2, 3
STEP = ((1, 0), (0, 1), (-1, 0), (0, -1))            # (dx, dy) of a direction
COLS = 8


def _at(m, y, x):
    h, w = m.shape
    return int(m[y, x]) if 0 <= y < h and 0 <= x < w else -1


def edges(m):
    """{key: (x0, y0, dir, label, owner pixel index)} of one map [h, w]."""
    h, w = m.shape
    out = {}
    for y in range(h):
        for x in range(w):
            v = int(m[y, x])
            if v == 0:
                continue
            sides = ((x, y, E, _at(m, y - 1, x)), (x + 1, y, S, _at(m, y, x + 1)),
                     (x + 1, y + 1, W, _at(m, y + 1, x)), (x, y + 1, N, _at(m, y, x - 1)))
            for x0, y0, d, other in sides:
                if other != v:
                    out[(y0 * (w + 1) + x0) * 4 + d] = (x0, y0, d, v, y * w + x)
    return out


def _ahead(px, py, d):
    """(right pixel, left pixel) as (y, x) ahead of point (px, py) for a walker heading d."""
    if d == E:
        return (py, px), (py - 1, px)
    if d == S:
        return (py, px - 1), (py, px)
    if d == W:
        return (py - 1, px - 1), (py, px - 1)
    return (py - 1, px), (py - 1, px - 1)


def successor(m, edge, connectivity):
    """The key of the edge that follows `edge` = (x0, y0, dir, label, owner)."""
    w = m.shape[1]
    x0, y0, d, v, _ = edge
    px, py = x0 + STEP[d][0], y0 + STEP[d][1]
    r, l = _ahead(px, py, d)
    R, L = _at(m, *r) == v, _at(m, *l) == v
    if connectivity == 8:
        nd = d - 1 if L else d if R else d + 1
    else:
        nd = d + 1 if not R else d - 1 if L else d
    return (py * (w + 1) + px) * 4 + nd % 4


def contours(m, connectivity):
    """The contours of one map in ascending order of start key: a list of dicts with label, verts [(x, y), ...], edges,
    area2, start, pixel."""
    assert connectivity in (4, 8)
    ed = edges(m)
    nxt = {k: successor(m, e, connectivity) for k, e in ed.items()}
    assert set(nxt.values()) == set(ed), "every edge has one successor and one predecessor among the edges"
    for k, s in nxt.items():
        assert ed[s][3] == ed[k][3], "the successor carries the same label"
    prev = {s: k for k, s in nxt.items()}
    seen, out = set(), []
    for k0 in sorted(ed):
        if k0 in seen:
            continue
        cyc, k = [], k0
        while k not in seen:
            seen.add(k)
            cyc.append(k)
            k = nxt[k]
        assert k == k0
        corners = [k for k in cyc if ed[prev[k]][2] != ed[k][2]]
        start = min(corners)
        i = cyc.index(start)
        cyc = cyc[i:] + cyc[:i]
        verts = [(ed[k][0], ed[k][1]) for k in cyc if ed[prev[k]][2] != ed[k][2]]
        area2 = 0
        for j in range(len(verts)):
            (xa, ya), (xb, yb) = verts[j], verts[(j + 1) % len(verts)]
            area2 += xa * yb - xb * ya
        out.append(dict(label=ed[start][3], verts=verts, edges=len(cyc), area2=area2, start=start, pixel=ed[start][4]))
    out.sort(key=lambda c: c["start"])
    return out


def trace(maps, connectivity, cmax, vmax, table=None, verts=None, found=None):
    """(table int64 [n, cmax, 8], verts int16 [n, vmax, 2], counts int32 [n, 4]) of maps uint8 [n, h, w]; what the entry
    leaves alone keeps the value of the arrays handed in (zeros without them).  found: [contours(maps[i], connectivity)
    for every i], when the caller has them already."""
    n = maps.shape[0]
    table = np.zeros((n, cmax, COLS), np.int64) if table is None else table.copy()
    verts = np.zeros((n, vmax, 2), np.int16) if verts is None else verts.copy()
    counts = np.zeros((n, 4), np.int32)
    for i in range(n):
        cs = contours(maps[i], connectivity) if found is None else found[i]
        off = 0
        for r, c in enumerate(cs):
            nv = len(c["verts"])
            if r < cmax:
                table[i, r] = (c["label"], off, nv, c["edges"], c["area2"], c["start"], c["pixel"], 0)
                if off + nv <= vmax:
                    verts[i, off:off + nv] = c["verts"]
            off += nv
        counts[i] = (len(cs), off, max(0, len(cs) - cmax), max(0, off - vmax))
    return table, verts, counts


def topology(table, counts, nl):
    """int32 [n, nl, 3]: outer contours, holes, Euler number per label, of the rows the table holds."""
    n, cmax = table.shape[:2]
    topo = np.zeros((n, nl, 3), np.int32)
    for i in range(n):
        for r in range(min(int(counts[i, 0]), cmax)):
            v, a2 = int(table[i, r, 0]), int(table[i, r, 4])
            if v < nl:
                topo[i, v, 0 if a2 > 0 else 1] += 1
        topo[i, :, 2] = topo[i, :, 0] - topo[i, :, 1]
    return topo


def polygons(m, connectivity):
    """[{label, outer, holes}] of one map, one entry per outer contour in table order; a hole goes to the outer contour
    whose component (scipy-free flood fill under `connectivity`) owns the hole's start pixel."""
    h, w = m.shape
    comp = np.zeros((h, w), np.int64)
    nb = ((0, 1), (1, 0), (0, -1), (-1, 0)) + (((1, 1), (1, -1), (-1, 1), (-1, -1)) if connectivity == 8 else ())
    k = 0
    for y in range(h):
        for x in range(w):
            if m[y, x] and not comp[y, x]:
                k += 1
                comp[y, x] = k
                todo = [(y, x)]
                while todo:
                    cy, cx = todo.pop()
                    for dy, dx in nb:
                        yy, xx = cy + dy, cx + dx
                        if 0 <= yy < h and 0 <= xx < w and m[yy, xx] == m[y, x] and not comp[yy, xx]:
                            comp[yy, xx] = k
                            todo.append((yy, xx))
    cs = contours(m, connectivity)
    out, by_comp = [], {}
    for c in cs:
        if c["area2"] > 0:
            out.append(dict(label=c["label"], outer=np.array(c["verts"], np.int16), holes=[]))
            by_comp[int(comp.reshape(-1)[c["pixel"]])] = out[-1]
    for c in cs:
        if c["area2"] < 0:
            by_comp[int(comp.reshape(-1)[c["pixel"]])]["holes"].append(np.array(c["verts"], np.int16))
    return out


def rasterise(polys, h, w):
    """The label map of polygons()-style output by even-odd fill: pixel (y, x) is inside a ring when a ray from its centre
    towards -x crosses the ring's vertical edges an odd number of times."""
    m = np.zeros((h, w), np.uint8)
    for p in polys:
        par = np.zeros((h, w), np.int64)
        for ring in [p["outer"]] + list(p["holes"]):
            k = len(ring)
            for j in range(k):
                (xa, ya), (xb, yb) = (int(t) for t in ring[j]), (int(t) for t in ring[(j + 1) % k])
                if xa == xb:
                    par[min(ya, yb):max(ya, yb), xa:] += 1
        m[par % 2 == 1] = p["label"]
    return m
