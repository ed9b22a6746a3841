"""Float64 numpy restatement of the embedding clustering (include/isa_kernels.h, isa_cluster_*): the
greedy flat-kernel mean-shift and the deterministic Lloyd k-means, one image at a time.  Every distance is the direct form
sum_j (x[j] - c[j])^2.  Each routine also reports `min_margin`, the smallest relative gap it met at a decision:
|d - bw^2| / bw^2 at a ball membership, (d_2nd - d_1st) / d_2nd at an assignment, (v_1st - v_2nd) / v_1st between the two
largest values of a farthest-point pick.  An fp32 run must take the same decisions as long as that margin stays well above
the fp32 rounding of d (about 4e-6 relative for 32 channels)."""
import numpy as np

MAX_K = 32
INF = float("inf")


def sqdist(x, c):
    """d(p, c) of every row of x [P, C] against one centre c [C], direct form."""
    t = x - c[None, :]
    return (t * t).sum(1)


def ball_gap(d, bw2):
    """Relative gaps of ball memberships d <= bw2 (inf for no pixel)."""
    return np.abs(d - bw2) / bw2


def assign(x, centres):
    """(labels 0-based [P], gap [P]) of rows x [P, C] to centres [K, C]: the nearest centre, ties to the lowest index;
    gap = (d_2nd - d_1st) / d_2nd, inf for K == 1 or d_2nd == 0."""
    K = centres.shape[0]
    d = np.stack([sqdist(x, centres[k]) for k in range(K)], 1) if x.shape[0] else np.zeros((0, K))
    lab = d.argmin(1) if x.shape[0] else np.zeros((0,), np.int64)     # argmin: the first minimum
    gap = np.full(x.shape[0], INF)
    if K >= 2 and x.shape[0]:
        s = np.sort(d, 1)
        nz = s[:, 1] > 0
        gap[nz] = (s[nz, 1] - s[nz, 0]) / s[nz, 1]
    return lab, gap


def farthest_init(x, fg, K):
    """Deterministic maximin over the foreground rows of x [L, C]: (centres [K, C], pixel indices [K], min_margin)."""
    idx = np.flatnonzero(fg)
    assert 1 <= K <= idx.size
    xf = x[idx]
    picks, margin = [0], INF
    dmin = sqdist(xf, xf[0])
    for _ in range(1, K):
        j = int(dmin.argmax())                                        # argmax: the first maximum = the smallest index
        if xf.shape[0] >= 2:
            top = np.sort(dmin)[-2:]
            if top[1] > 0:
                margin = min(margin, (top[1] - top[0]) / top[1])
        picks.append(j)
        dmin = np.minimum(dmin, sqdist(xf, xf[j]))
    picks = np.array(picks)
    return xf[picks].copy(), idx[picks], margin


def lloyd(x, fg, centres, iters):
    """`iters` Lloyd iterations over the foreground rows from `centres` [K, C] and a last assignment.  Returns a dict:
    labels [L] (0 background, k + 1), centres [K, C] (those of the last assignment), sizes [K], moved, min_margin."""
    L = x.shape[0]
    K = centres.shape[0]
    labels = np.zeros(L, np.uint8)
    if K == 0:
        return dict(labels=labels, centres=centres.copy(), sizes=np.zeros(0, np.int64), moved=0, min_margin=INF)
    idx = np.flatnonzero(fg)
    xf = x[idx]
    c = centres.astype(np.float64).copy()
    margin, prev = INF, None
    for i in range(iters + 1):
        lab, gap = assign(xf, c)
        if gap.size:
            margin = min(margin, float(gap.min()))
        if i == iters:
            break
        prev = lab
        for k in range(K):
            m = lab == k
            if m.any():                                               # an empty cluster keeps its centre
                c[k] = xf[m].mean(0)
    labels[idx] = lab + 1
    moved = int((lab != prev).sum()) if iters > 0 else 0
    return dict(labels=labels, centres=c, sizes=np.bincount(lab, minlength=K)[:K], moved=moved, min_margin=margin)


def kmeans(x, fg, n_objects, iters=10, init='farthest', kmax=MAX_K):
    """Method 'kmeans' of one image: x [L, C], fg [L] bool.  K = min(n_objects, foreground pixels, kmax)."""
    K = int(min(max(int(n_objects), 0), int(fg.sum()), kmax, MAX_K))
    if K == 0:
        return dict(labels=np.zeros(x.shape[0], np.uint8), n_objects=0, centres=np.zeros((0, x.shape[1])),
                    sizes=np.zeros(0, np.int64), moved=0, min_margin=INF, init=np.zeros((0, x.shape[1])))
    if isinstance(init, str):
        assert init == 'farthest'
        c0, _, m0 = farthest_init(x, fg, K)
    else:
        c0, m0 = np.asarray(init, np.float64)[:K], INF
    out = lloyd(x, fg, c0, iters)
    out.update(n_objects=K, min_margin=min(out["min_margin"], m0), init=c0)
    return out


def ball(x, free, c, bw2):
    """(member mask over all rows, gaps of the free rows) of the ball of radius^2 bw2 around c among the free rows."""
    d = sqdist(x, c)
    return free & (d <= bw2), ball_gap(d[free], bw2)


def meanshift(x, fg, bandwidth, shifts=3, max_objects=MAX_K, min_pixels=1, assign_rest=True, refine=0, max_rounds=None):
    """Method 'meanshift' of one image: x [L, C], fg [L] bool.  max_rounds (default max_objects): the round budget - a round
    ends with an object or with a ball refused as noise, and both kinds count (the device issues a fixed launch sequence);
    `rounds` of the result says how many ran."""
    L, C = x.shape
    bw2 = float(bandwidth) ** 2
    labels = np.zeros(L, np.int64)
    noise = np.zeros(L, bool)
    centres, sizes, margin, rounds = [], [], INF, 0
    k = 0
    max_rounds = max_objects if max_rounds is None else max_rounds
    assert max_rounds >= max_objects
    while k < max_objects and rounds < max_rounds:
        free = fg & (labels == 0) & ~noise
        if not free.any():
            break
        rounds += 1
        s = int(np.flatnonzero(free)[0])
        c = x[s].copy()
        for _ in range(shifts):
            S, gap = ball(x, free, c, bw2)
            margin = min(margin, float(gap.min()))
            if S.any():                                               # (never empty in exact arithmetic)
                c = x[S].mean(0)
        S, gap = ball(x, free, c, bw2)
        others = np.flatnonzero(free) != s                            # the seed joins S whatever its distance
        if others.any():
            margin = min(margin, float(gap[others].min()))
        S[s] = True
        if int(S.sum()) >= min_pixels:
            k += 1
            labels[S] = k
            centres.append(c)
            sizes.append(int(S.sum()))
        else:
            noise |= S
    cen = np.array(centres).reshape(k, C)
    rest = fg & (labels == 0)
    if assign_rest and k > 0 and rest.any():
        lab, gap = assign(x[rest], cen)
        labels[rest] = lab + 1
        margin = min(margin, float(gap.min()))
    out = dict(labels=labels.astype(np.uint8), n_objects=k, centres=cen, sizes=np.array(sizes, np.int64), moved=0,
               min_margin=margin, rounds=rounds)
    if refine > 0 and k > 0:
        r = lloyd(x, fg, cen, refine)
        out.update(labels=r["labels"], centres=r["centres"], sizes=r["sizes"], moved=r["moved"],
                   min_margin=min(margin, r["min_margin"]))
    return out


def cluster(emb, fg, method='meanshift', *, n_objects=None, **kw):
    """The batch form ReSeg.cluster_embedding returns: emb [B, C, H, W], fg [B, H, W] (non-zero = foreground) ->
    dict(labels uint8 [B, H, W], n_objects int32 [B], centres float64 [B, 32, C], sizes int32 [B, 32], moved int32 [B],
    min_margin).  kmeans: n_objects [B]; `init` may be 'farthest' or [B, K, C]."""
    emb = np.asarray(emb, np.float64)
    B, C, H, W = emb.shape
    out = dict(labels=np.zeros((B, H, W), np.uint8), n_objects=np.zeros(B, np.int32), centres=np.zeros((B, MAX_K, C)),
               sizes=np.zeros((B, MAX_K), np.int32), moved=np.zeros(B, np.int32), min_margin=INF)
    init = kw.pop("init", 'farthest')
    for b in range(B):
        x = emb[b].reshape(C, H * W).T.copy()
        f = np.asarray(fg[b]).reshape(-1) != 0
        if method == 'meanshift':
            r = meanshift(x, f, **kw)
        else:
            r = kmeans(x, f, int(n_objects[b]), init=init if isinstance(init, str) else init[b], **kw)
        k = r["n_objects"]
        out["labels"][b] = r["labels"].reshape(H, W)
        out["n_objects"][b] = k
        out["centres"][b, :k] = r["centres"]
        out["sizes"][b, :k] = r["sizes"]
        out["moved"][b] = r["moved"]
        out["min_margin"] = min(out["min_margin"], r["min_margin"])
    return out


def planted(B, H, W, C, n_inst, seed, noise=0.15, sep=3.0, fg_frac=0.7):
    """A planted test input: (emb float32 [B, C, H, W], fg uint8 [B, H, W], truth uint8 [B, H, W]).  The n_inst centres of an
    image lie at pairwise distance `sep` (scaled unit vectors: sep / sqrt 2 along n_inst axes, rotated), the pixels are
    the centres plus Gaussian noise of deviation `noise` per channel; the background is noise around the origin."""
    rng = np.random.RandomState(seed)
    emb = np.zeros((B, C, H, W), np.float32)
    fg = np.zeros((B, H, W), np.uint8)
    truth = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        n = n_inst[b] if hasattr(n_inst, "__len__") else n_inst
        q, _ = np.linalg.qr(rng.randn(max(C, n), max(C, n)))
        cen = (sep / np.sqrt(2.0)) * q[:n, :C] if n <= C else None
        assert cen is not None or n == 0, "at most C planted instances"
        t = np.zeros(H * W, np.int64)
        if n:
            mask = rng.rand(H * W) < fg_frac
            t[mask] = rng.randint(1, n + 1, int(mask.sum()))
            for i in range(1, n + 1):                                 # every instance owns at least one pixel
                t[rng.randint(0, H * W)] = i
        x = noise * rng.randn(H * W, C)
        if n:
            x[t > 0] += cen[t[t > 0] - 1]
        emb[b] = x.T.reshape(C, H, W).astype(np.float32)
        truth[b] = t.reshape(H, W)
        fg[b] = (t > 0).reshape(H, W)
    return emb, fg, truth
