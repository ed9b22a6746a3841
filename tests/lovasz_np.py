"""Float64 restatement of the Lovasz-Softmax criterion (lovasz_softmax, code/lib/losses/lovasz_losses.py:156-196) and of
its gradient with respect to the logits: the yardstick of the HIP kernels (csrc/lovasz.hip) and of the reference fixture.

For class c and pixel i: p = softmax of the logits, fg = [label == c], e = |fg - p_c|.  A segment is (class, whole batch),
or (class, image) when per_image.  Inside a segment the errors are sorted in descending order by a STABLE sort, ties by
ascending pixel index (torch.sort(stable=True, descending=True)); the Lovasz gradient of rank r is
jaccard[r] - jaccard[r-1] of lovasz_grad, here in the closed form that does not cancel (`coefficients`):
    cf, cb = foreground / background elements strictly before r;  G = foreground elements;  I = G - cf;  U = G + cb
    g_r = 1/U for a foreground element, I / (U (U+1)) for a background one;  G == 0: g_0 = 1, else 0.
Segment loss = sum_r e_r g_r.  Counted classes: all K (the reference), or 1..K-1 when optimize_bg is false (the
trainer's option, as for Dice); only_present keeps the counted classes with G > 0 in the segment.  The loss is the mean
over the kept classes (0 when none), then over the images when per_image.  The gradient takes the order as constant
(the subgradient autograd gives): d loss / d p_c(i) = scale * g_rank(i) * (-1 for fg, +1 for bg), and through the softmax
d z_k = p_k (d_k - sum_j p_j d_j)."""
import numpy as np


def softmax(logits):
    """float64 softmax over axis 1 of [B,K,H,W]."""
    z = np.asarray(logits, dtype=np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def coefficients(fg_sorted):
    """Lovasz gradient of every rank from integer counts (float64): fg_sorted is the 0/1 foreground flag in sorted order."""
    fg = np.asarray(fg_sorted).astype(np.int64)
    n, G = fg.size, int(fg.sum())
    if G == 0:
        g = np.zeros(n)
        g[:1] = 1.0
        return g
    cf = np.cumsum(fg) - fg                        # exclusive counts
    cb = np.arange(n, dtype=np.int64) - cf
    I, U = (G - cf).astype(np.float64), (G + cb).astype(np.float64)
    return np.where(fg == 1, 1.0 / U, I / (U * (U + 1.0)))


def jaccard_differences(fg_sorted, dtype=np.float64):
    """lovasz_grad (lovasz_losses.py:17-30) as the reference writes it, in `dtype`."""
    fg = np.asarray(fg_sorted).astype(dtype)
    gts = fg.sum(dtype=dtype)
    inter = gts - np.cumsum(fg, dtype=dtype)
    union = gts + np.cumsum(1 - fg, dtype=dtype)
    jac = (1.0 - inter / union).astype(dtype)
    if fg.size > 1:
        jac[1:] = jac[1:] - jac[:-1]
    return jac


def segment_errors(logits, labels):
    """(p [B,K,H,W], errors [K, B, H*W], fg [K, B, H*W] bool) in float64."""
    p = softmax(logits)
    B, K = p.shape[:2]
    lab = np.asarray(labels).reshape(B, -1)
    fg = lab[None, :, :] == np.arange(K)[:, None, None]
    pe = p.reshape(B, K, -1).transpose(1, 0, 2)
    return p, np.abs(fg.astype(np.float64) - pe), fg


def stable_descending(e):
    """Order of a stable descending sort: ties keep ascending index."""
    return np.argsort(-e, kind="stable")


def lovasz_softmax(logits, labels, optimize_bg=True, only_present=False, per_image=False, orders=None):
    """Loss and d loss / d logits [B,K,H,W] in float64.  `orders` (optional, [K, nimg, seglen] integers): the sorted
    order of every segment, injected in place of the stable descending sort of the errors.  Returns a dict: loss, grad,
    errors [K, nimg, seglen], orders [K, nimg, seglen], G [K, nimg], seg_loss [K, nimg]."""
    p, err, fg = segment_errors(logits, labels)
    B, K = p.shape[:2]
    nimg = B if per_image else 1
    err, fg = err.reshape(K, nimg, -1), fg.reshape(K, nimg, -1)
    seglen = err.shape[2]
    used = np.empty((K, nimg, seglen), dtype=np.int64)
    seg_loss = np.zeros((K, nimg))
    dp = np.zeros((K, nimg, seglen))
    G = fg.sum(2)
    for c in range(K):
        for s in range(nimg):
            order = stable_descending(err[c, s]) if orders is None else np.asarray(orders[c][s], dtype=np.int64)
            used[c, s] = order
            g = coefficients(fg[c, s][order])
            seg_loss[c, s] = float(np.dot(err[c, s][order], g))
            dp[c, s, order] = np.where(fg[c, s][order], -g, g)
    counted = np.zeros(K, dtype=bool)
    counted[0 if optimize_bg else 1:] = True
    keep = counted[:, None] & ((G > 0) if only_present else np.ones_like(G, dtype=bool))
    kept = keep.sum(0)                                            # per image (or the batch)
    scale = np.where(keep, 1.0 / (np.maximum(kept, 1) * nimg)[None, :], 0.0)
    loss = float((seg_loss * scale).sum())
    d = (dp * scale[:, :, None]).reshape(K, B, -1).transpose(1, 0, 2).reshape(p.shape)
    grad = p * (d - (p * d).sum(1, keepdims=True))
    return dict(loss=loss, grad=grad, errors=err, orders=used, G=G, seg_loss=seg_loss)
