"""numpy / plain-Python restatement of the three contracts of include/isa_kernels.h "connected components":
  label(maps, connectivity)            -> (comp int32 [n,h,w], n_comp int32 [n])           isa_cc_label
  split(maps, comp, min_area, max_objects)   -> (out uint8, count int32 [n], dropped int32 [n])   isa_cc_select, ISA_CC_SPLIT
  largest(maps, comp, min_area, max_objects) -> the same triple                                   isa_cc_select, ISA_CC_LARGEST
Written to be read, not to be fast; labelling works on the horizontal runs of a row (a few tens of thousands at 512 x 512
noise), so the Python loops run over runs and their overlaps, never over pixels.  No test imports anything else as the
reference; tests/test_components_ref.py checks this file against scipy.ndimage.label and hand-written answers."""
import numpy as np


def _row_runs(row):
    """(start, end) of the maximal runs of equal NON-ZERO values of a 1-d array, end exclusive, and their values."""
    cut = np.flatnonzero(row[1:] != row[:-1]) + 1
    start = np.concatenate(([0], cut))
    end = np.concatenate((cut, [row.size]))
    keep = row[start] != 0
    return start[keep], end[keep], row[start][keep]


def _label_image(img, connectivity):
    h, w = img.shape
    reach = 1 if connectivity == 8 else 0          # how far past its ends a run touches the row above
    parent = []                                    # union-find over run ids; ids grow in raster order of the runs' first pixels
    first_pixel = []                               # row-major index of a run's first pixel

    def find(r):
        while parent[r] != r:
            parent[r] = parent[parent[r]]
            r = parent[r]
        return r

    prev = (np.zeros(0, np.int64),) * 3 + (0,)     # start, end, value, id of the first run: the row above
    lengths = []
    for y in range(h):
        start, end, val = _row_runs(img[y])
        base = len(parent)
        parent.extend(range(base, base + start.size))
        first_pixel.extend((y * w + start).tolist())
        lengths.append(end - start)
        p_start, p_end, p_val, p_base = prev
        # the runs above that reach [start - reach, end + reach): p_end > start - reach and p_start < end + reach
        lo = np.searchsorted(p_end, start - reach, side='right')
        hi = np.searchsorted(p_start, end + reach, side='left')
        for j in range(start.size):
            for k in range(lo[j], hi[j]):
                if p_val[k] == val[j]:
                    a, b = find(base + j), find(p_base + k)
                    if a != b:                     # the smaller id (the earlier first pixel) becomes the root
                        parent[max(a, b)] = min(a, b)
        prev = (start, end, val, base)
    roots = np.array([find(r) for r in range(len(parent))], dtype=np.int64)
    first_pixel = np.array(first_pixel, dtype=np.int64)
    comp = np.zeros((h, w), np.int32)
    if roots.size:
        # the foreground pixels in raster order are exactly the runs, in id order, laid end to end
        comp[img != 0] = np.repeat(first_pixel[roots] + 1, np.concatenate(lengths)).astype(np.int32)
    return comp, int(np.count_nonzero(roots == np.arange(roots.size)))


def label(maps, connectivity=8):
    """comp[b,y,x] = 0 for background, else 1 + the smallest row-major index (inside image b) of a pixel of the component of
    (y, x): pixels are joined when adjacent under `connectivity` (4: edges, 8: edges and corners) and equal and non-zero."""
    assert connectivity in (4, 8)
    maps = np.asarray(maps)
    assert maps.ndim == 3
    comps, counts = zip(*[_label_image(m, connectivity) for m in maps])
    return np.stack(comps), np.array(counts, np.int32)


def _components(comp_img):
    """roots (comp values, ascending = raster order of the first pixels) and areas of one image's components."""
    return np.unique(comp_img[comp_img > 0], return_counts=True)


def split(maps, comp, min_area=1, max_objects=255):
    """Every component of area >= min_area, in raster order of its first pixel, is an instance; the first max_objects of
    them get labels 1, 2, ..; everything else is 0.  dropped: qualifying components without a label."""
    assert 1 <= max_objects <= 255
    out = np.zeros(comp.shape, np.uint8)
    count, dropped = np.zeros(len(comp), np.int32), np.zeros(len(comp), np.int32)
    for b in range(len(comp)):
        roots, areas = _components(comp[b])
        qualifying = roots[areas >= max(min_area, 1)]
        for lab, root in enumerate(qualifying[:max_objects], 1):
            out[b][comp[b] == root] = lab
        count[b] = min(qualifying.size, max_objects)
        dropped[b] = qualifying.size - count[b]
    return out, count, dropped


def largest(maps, comp, min_area=1, max_objects=255):
    """Per input value the component of largest area (ties: the smaller root) survives if its area >= min_area; survivors
    are renumbered 1, 2, .. in ascending order of the value, the first max_objects of them.  dropped: qualifying
    components without a label (fragments that lost, survivors past the cap)."""
    assert 1 <= max_objects <= 255
    maps = np.asarray(maps)
    out = np.zeros(comp.shape, np.uint8)
    count, dropped = np.zeros(len(comp), np.int32), np.zeros(len(comp), np.int32)
    for b in range(len(comp)):
        roots, areas = _components(comp[b])
        values = maps[b].reshape(-1)[roots - 1]
        survivors = []
        for v in sorted(set(values.tolist())):
            area, neg_root = max((int(a), -int(r)) for a, r, u in zip(areas, roots, values) if u == v)
            if area >= max(min_area, 1):
                survivors.append(-neg_root)
        for lab, root in enumerate(survivors[:max_objects], 1):
            out[b][comp[b] == root] = lab
        count[b] = min(len(survivors), max_objects)
        dropped[b] = int(np.count_nonzero(areas >= max(min_area, 1))) - count[b]
    return out, count, dropped
