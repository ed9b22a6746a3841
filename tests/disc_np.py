"""float64 numpy restatement of the discriminative embedding loss and its analytic gradient (DESIGN.md section 15;
include/isa_kernels.h "discriminative embedding loss").  Shared by tests/test_disc_ref.py (pinned to the reference's own
functions through tests/golden/disc.npz) and tests/test_gpu_disc.py (the kernels against it).

x [B,C,H,W]; labels [B,H,W] integers, 0 = background, i + 1 = instance i (disjoint planes: the first plane wins);
n_objects [B].  Instance i of image b is PRESENT when i < n_objects[b] and it has a pixel.  |.| is the L1 or L2 norm.
    m_i = mean of x over the instance,  mu_i = m_i / |m_i|_2 with unit_means (0 when m_i = 0), else m_i
    var  = 1/B sum_b 1/F_b sum_{i present} sum_{p in i} max(|x_p - mu_i| - delta_v, 0)^2,  F_b = pixels of present instances
    dist = 1/B sum_{b: np >= 2} sum_{i != j present} max(2 delta_d - |mu_i - mu_j|, 0)^2 / (np (np - 1))
    reg  = 1/B sum_{b: np >= 1} mean_{i present} |mu_i|
    qreg = sum_{b,p} ([label != 0] |x_p|_2 - 1)^2 / num,  num = all foreground pixels (counted planes or not)
    loss = alpha var + beta dist + gamma reg + gamma_q qreg
Rules where the reference is 0/0: an empty counted instance is not present; F_b = 0, np < 2, np = 0, num = 0 give a zero
term; d/|d|_2 = 0 at d = 0; the L1 derivative is sign with sign(0) = 0; m = 0 with unit_means: mu = 0, no gradient."""
import numpy as np

FORMS = {"reference": (True, (1.0, 0.0, 0.0, 0.005)), "full": (False, (1.0, 1.0, 0.001, 0.0))}


def labels_from_planes(planes):
    """[B,K,H,W] planes (non-zero = member) -> labels [B,H,W]: 1 + the first plane that holds the pixel, 0 if none."""
    p = np.asarray(planes) != 0
    first = p.argmax(1)
    return np.where(p.any(1), first + 1, 0).astype(np.int64)


def _norm(d, norm):
    """|d| over the last axis and d|d|/dd."""
    if norm == 2:
        n = np.sqrt((d * d).sum(-1))
        safe = np.where(n > 0, n, 1.0)
        return n, np.where((n > 0)[..., None], d / safe[..., None], 0.0)
    return np.abs(d).sum(-1), np.sign(d)


def discriminative(x, labels, n_objects, delta_v=0.5, delta_d=1.5, norm=2, unit_means=True,
                   weights=(1.0, 0.0, 0.0, 0.005), K=32):
    x = np.asarray(x, dtype=np.float64)
    labels = np.asarray(labels)
    assert norm in (1, 2) and x.ndim == 4 and labels.shape == (x.shape[0],) + x.shape[2:]
    alpha, beta, gamma, gamma_q = [float(w) for w in weights]
    B, C = x.shape[:2]
    X = x.transpose(0, 2, 3, 1).reshape(B, -1, C)
    lab = labels.reshape(B, -1)
    n_objects = [max(0, min(K, int(v))) for v in np.asarray(n_objects).reshape(-1)]
    G = np.zeros_like(X)
    mu_all, m_all = np.zeros((B, K, C)), np.zeros((B, K, C))
    var = dist = reg = 0.0
    n_present = fg_counted = 0
    num = int((lab != 0).sum())
    for b in range(B):
        members = [np.nonzero(lab[b] == i + 1)[0] for i in range(n_objects[b])]
        present = [i for i, q in enumerate(members) if q.size]
        F = sum(members[i].size for i in present)
        n_present += len(present)
        fg_counted += F
        if not present:
            continue
        npres = len(present)
        m = np.stack([X[b, members[i]].mean(0) for i in present])
        mn = np.sqrt((m * m).sum(1))
        if unit_means:
            mu = np.where((mn > 0)[:, None], m / np.where(mn > 0, mn, 1.0)[:, None], 0.0)
        else:
            mu = m
        g_mu = np.zeros_like(mu)
        for a, i in enumerate(present):
            q = members[i]
            d = X[b, q] - mu[a]
            nd, unitd = _norm(d, norm)
            h = np.maximum(nd - delta_v, 0.0)
            var += (h * h).sum() / F / B
            direct = (2.0 * alpha * h / (B * F))[:, None] * unitd
            G[b, q] += direct
            g_mu[a] -= direct.sum(0)
        if npres >= 2:
            diff = mu[:, None, :] - mu[None, :, :]
            nd, unitd = _norm(diff, norm)
            t = np.maximum(2.0 * delta_d - nd, 0.0) * (1.0 - np.eye(npres))
            dist += (t * t).sum() / (npres * (npres - 1)) / B
            g_mu += -4.0 * beta / (B * npres * (npres - 1)) * (t[:, :, None] * unitd).sum(1)
        rn, unitr = _norm(mu, norm)
        reg += rn.mean() / B
        g_mu += gamma / (B * npres) * unitr
        if unit_means:
            ok = mn > 0
            g_m = np.where(ok[:, None], (g_mu - mu * (mu * g_mu).sum(1, keepdims=True)) / np.where(ok, mn, 1.0)[:, None], 0.0)
        else:
            g_m = g_mu
        for a, i in enumerate(present):
            G[b, members[i]] += g_m[a] / members[i].size
            mu_all[b, i], m_all[b, i] = mu[a], m[a]
    fgm = lab != 0
    xn = np.sqrt((X * X).sum(-1))
    qreg = float(((np.where(fgm, xn, 0.0) - 1.0) ** 2).sum() / num) if num else 0.0
    if num:
        f = np.where(fgm & (xn > 0), 2.0 * gamma_q * (xn - 1.0) / num / np.where(xn > 0, xn, 1.0), 0.0)
        G += f[..., None] * X
    loss = alpha * var + beta * dist + gamma * reg + gamma_q * qreg
    grad = G.reshape((B,) + x.shape[2:] + (C,)).transpose(0, 3, 1, 2)
    return dict(loss=float(loss), var=float(var), dist=float(dist), reg=float(reg), qreg=qreg, means=mu_all, m=m_all,
                grad=np.ascontiguousarray(grad), n_present=n_present, fg=fg_counted, num=num)


def form(name, x, labels, n_objects, delta_v=0.5, delta_d=1.5, norm=2, K=32):
    unit, w = FORMS[name]
    return discriminative(x, labels, n_objects, delta_v, delta_d, norm, unit, w, K)
