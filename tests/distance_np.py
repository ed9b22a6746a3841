"""Numpy restatement of the distance transform to the two nearest instances (isa_edt2_u8), of the border weight map
(isa_border_weights) and of the instance fill (isa_fill_labels).  Per instance, by brute force over its labelled pixels;
where that would take too long (hw * labelled pixels above BRUTE_LIMIT) the per-instance distances come from
scipy.ndimage.distance_transform_edt's nearest-pixel indices instead, which tests/test_distance_ref.py holds against the
brute force.  Neither shares a line of reasoning with the device's two-entry column pass and pruned row walk."""
import numpy as np

BRUTE_LIMIT = 1 << 25

INF = np.iinfo(np.int32).max


def label_distances(lab, method=None):
    """lab uint8 [h,w] -> (labels present ascending, D int64 [k,h,w]): D[i] = squared distance to the nearest pixel of label i.
    method: 'brute', 'scipy', or None = brute force where it is affordable."""
    h, w = lab.shape
    ks = [int(k) for k in np.unique(lab) if k != 0]
    yy, xx = np.mgrid[0:h, 0:w]
    D = np.empty((len(ks), h, w), np.int64)
    if method is None:
        method = "brute" if h * w * int(np.count_nonzero(lab)) <= BRUTE_LIMIT else "scipy"
    for i, k in enumerate(ks):
        if method == "scipy":
            from scipy.ndimage import distance_transform_edt
            iy, ix = distance_transform_edt(lab != k, return_distances=False, return_indices=True)
            D[i] = (yy - iy.astype(np.int64)) ** 2 + (xx - ix.astype(np.int64)) ** 2      # exact: integers from indices
            continue
        py, px = np.nonzero(lab == k)
        best = np.full((h, w), np.iinfo(np.int64).max, np.int64)
        for s in range(0, len(py), 512):                   # chunks keep the [h,w,m] block small
            d = (yy[..., None] - py[s:s + 512]) ** 2 + (xx[..., None] - px[s:s + 512]) ** 2
            best = np.minimum(best, d.min(axis=-1))
        D[i] = best
    return ks, D


def edt2(labels, method=None):
    """labels uint8 [n,h,w] -> d1sq int32, d2sq int32, nearest uint8, by the rules of include/isa_kernels.h."""
    labels = np.asarray(labels, np.uint8)
    n, h, w = labels.shape
    d1 = np.full((n, h, w), INF, np.int32)
    d2 = np.full((n, h, w), INF, np.int32)
    near = np.zeros((n, h, w), np.uint8)
    for b in range(n):
        ks, D = label_distances(labels[b], method)
        if not ks:
            continue
        order = np.argsort(D, axis=0, kind="stable")       # stable over ascending labels: ties go to the smaller label
        srt = np.take_along_axis(D, order, axis=0)
        d1[b] = srt[0]
        near[b] = np.asarray(ks, np.uint8)[order[0]]
        if len(ks) > 1:
            d2[b] = srt[1]
    return d1, d2, near


def border_weights(labels, d1sq, d2sq, w0, sigma):
    """float64 weight map: 1 on labelled pixels and where no second instance exists, else the U-Net border term."""
    d1 = np.sqrt(d1sq.astype(np.float64))
    d2 = np.sqrt(d2sq.astype(np.float64))
    bump = w0 * np.exp(-(d1 + d2) ** 2 / (2.0 * float(sigma) ** 2))
    return np.where((labels != 0) | (d2sq == INF), 1.0, 1.0 + bump)


def fill(labels, fg, nearest, d1sq, max_dist_sq=-1):
    """-> (out uint8 [n,h,w], filled int32 [n])."""
    take = (labels == 0) & (fg != 0) & (nearest != 0)
    if max_dist_sq >= 0:
        take &= d1sq <= max_dist_sq
    out = np.where(take, nearest, labels).astype(np.uint8)
    return out, take.reshape(take.shape[0], -1).sum(axis=1).astype(np.int32)


def max_dist_sq(max_dist):
    """The integer bound the device compares d1sq with: None = no limit (-1)."""
    if max_dist is None:
        return -1
    return int(min(float(max_dist) ** 2, INF))


# ---- the cases every shape is tested on ------------------------------------------------------------------------------------
def blobs(rng, n, h, w, k):
    """k random discs per image (later ones paint over earlier ones), some background left."""
    out = np.zeros((n, h, w), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    labs = rng.choice(np.arange(1, 256), size=k, replace=False)
    for b in range(n):
        for l in labs:
            cy, cx = rng.integers(0, h), rng.integers(0, w)
            r = rng.uniform(0.5, max(1.0, min(h, w) / 5.0))
            out[b][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = l
    return out


def cases(n, h, w, seed=0):
    """name -> uint8 [n,h,w]"""
    rng = np.random.default_rng(seed + 1000 * h + w)
    c = {"blobs1": blobs(rng, n, h, w, 1), "blobs2": blobs(rng, n, h, w, 2), "blobs12": blobs(rng, n, h, w, 12)}
    c["empty"] = np.zeros((n, h, w), np.uint8)
    one = np.zeros((n, h, w), np.uint8)
    one[:, h // 3:h // 3 + 2, w // 2:w // 2 + 2] = 7
    c["one"] = one
    c["full"] = np.array([1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 255], np.uint8)[rng.integers(0, 12, size=(n, h, w))]
    corners = np.zeros((n, h, w), np.uint8)
    corners[:, 0, 0] = 1
    corners[:, h - 1, w - 1] = 255
    c["corners"] = corners
    c["checker"] = np.broadcast_to(checkerboard(h, w), (n, h, w)).copy()
    return c


def checkerboard(h, w, a=1, b=2):
    """Labels on the even lattice only, a and b alternating like a checkerboard: every unlabelled pixel between two
    lattice points is equally far from both labels."""
    yy, xx = np.mgrid[0:h, 0:w]
    lab = np.where((yy // 2 + xx // 2) % 2 == 0, a, b).astype(np.uint8)
    lab[(yy % 2 == 1) | (xx % 2 == 1)] = 0
    return lab
