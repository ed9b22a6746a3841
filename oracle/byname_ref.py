"""Plain-torch restatements of the reference's WHOLE named attention operators (modules/utils.py),
evaluated in the dtype the caller names (float64 by default): the yardstick of tests/test_gpu_byname_shapes.py, pinned
to the reference's own classes by tests/test_byname_ref.py over tests/golden/byname_shapes.npz.

  scale_pd_attention     _ScalePDAttention.forward     utils.py:267-303
  multi_head_attention   MultiHeadAttention.forward    utils.py:193-225   (both branches)
  sdp_attention          ScaledDotProductAttention     utils.py:314-329
  sdp_scores             its last=True branch          utils.py:315-318   (raw q k^T, or with MultiHeadAttention's sigmoid)
  point_query_mask       Decoder.forward               utils.py:59-69
  linear_ln, instance_norm_res                         the two small layers the library runs around the cores

Parameters come as a state_dict of the reference class (same names and shapes)."""
import torch
import torch.nn.functional as F

import reseg_ref as R


# The cases of tests/golden/byname_shapes.npz (oracle/gen_golden.py:byname_shape_cases), off the one configuration of
# byname_ops.npz (d_k = d_v = 12, d_model = 24, 2 heads, b = 2, 16x16, dilation 2, lq = 1):
SPD_CASES = [          # (d_k, d_v, d_model, n_head, dilation, b, h, w)
    (12, 12, 32, 2, 1, 3, 9, 14),      # c = 16 != d_k, odd b, h != w
    (8, 16, 48, 2, 3, 1, 7, 5),        # d_k != d_v, b = 1, dilation >= half the map
    (12, 12, 24, 1, 2, 2, 6, 10),      # one head, c = 24
    (12, 6, 40, 4, 5, 2, 5, 4),        # four heads, dilation >= h and w: all eight neighbours are padding
    (12, 12, 20, 2, 1, 2, 8, 8),       # d_model % 8 != 0
]
MHA_CASES = [          # (n_head, d_model, d_k, d_v, b, lq, L); case 0 has one fully masked row
    (2, 24, 12, 12, 3, 3, 777),
    (1, 32, 12, 12, 2, 5, 300),
    (1, 32, 16, 8, 2, 2, 513),
]
DEC_CASES = [(3, 20, 7, 9), (1, 64, 1, 1)]       # (b, c, h, w)
MHA_MASKED_ROW = (1, 2)                          # (image, query) of MHA case 0 with every key masked
STORE_MAX = 4096       # inputs with more elements are not stored: both sides draw them again from the case's seed


def case_seed(kind, i):
    return {"spd": 7100, "mha": 7200, "dec": 7300}[kind] + i


def spd_inputs(i):
    import numpy as np
    dk, dv, dm, G, dil, b, h, w = SPD_CASES[i]
    rs = np.random.RandomState(case_seed("spd", i))
    qk = torch.from_numpy(rs.standard_normal((b, dm, h, w)).astype(np.float32))
    v = torch.from_numpy(rs.standard_normal((b, dm, h, w)).astype(np.float32))
    nomask = torch.from_numpy((rs.rand(b, 1, h, w) < 0.3).astype(np.float32))
    return qk, v, nomask


def mha_inputs(i):
    import numpy as np
    G, dm, dk, dv, b, lq, L = MHA_CASES[i]
    rs = np.random.RandomState(case_seed("mha", i))
    q = torch.from_numpy(rs.standard_normal((b, lq, dm)).astype(np.float32))
    k = torch.from_numpy(rs.standard_normal((b, L, dm)).astype(np.float32))
    v = torch.from_numpy(rs.standard_normal((b, L, dm)).astype(np.float32))
    mask = torch.from_numpy(rs.rand(b, lq, L) < 0.25)
    if i == 0:
        mask[MHA_MASKED_ROW] = True
    return q, k, v, mask


def dec_inputs(i):
    import numpy as np
    b, c, h, w = DEC_CASES[i]
    rs = np.random.RandomState(case_seed("dec", i))
    q = torch.from_numpy(rs.standard_normal((b, c)).astype(np.float32))
    enc = torch.from_numpy(rs.standard_normal((b, c, h, w)).astype(np.float32))
    return q, enc


def _cast(sd, dtype):
    return {k: torch.as_tensor(v).to(dtype) for k, v in sd.items()}


def instance_norm_res(x, res, eps=1e-5):
    """InstanceNorm2d(x + res), affine=False: biased variance over h*w per (image, channel) (utils.py:254,302)."""
    y = x + res
    mean = y.mean((2, 3), keepdim=True)
    var = ((y - mean) ** 2).mean((2, 3), keepdim=True)
    return (y - mean) / torch.sqrt(var + eps)


def linear_ln(x, w, bias=None, residual=None, gamma=None, beta=None, eps=1e-5):
    """LayerNorm(x w^T + bias + residual) with every part optional; gamma None: no LayerNorm (beta is then unused)."""
    y = x @ w.t()
    if bias is not None:
        y = y + bias
    if residual is not None:
        y = y + residual
    if gamma is not None:
        mean = y.mean(1, keepdim=True)
        d = y - mean
        y = d / torch.sqrt((d * d).mean(1, keepdim=True) + eps) * gamma
        if beta is not None:
            y = y + beta
    return y


def scale_pd_attention(sd, qk, v, nomask, dilation, dtype=torch.float64, scale=None, taps=None):
    """_ScalePDAttention.forward.  sd: qk_w.{weight,bias} [2*d_k, c, 1, 1], v_w.{weight,bias} [d_v, c, 1, 1],
    fc.{weight,bias} [d_model, n_head*d_v, 1, 1] with c = d_model // n_head.  qk, v [b, d_model, h, w]; nomask [b, 1, h, w]
    in {0, 1}, 1 = masked key.  scale: factor on the local logits; None is the reference's c ** -0.5 (`c` is read off
    qk AFTER the head view, utils.py:273,293 - the per-head input width, not d_k).  taps: a dict that receives the
    projected `QK` [(b*n_head), 2*d_k, h, w], `V` [(b*n_head), d_v, h, w] and the attended map `att` [b, n_head*d_v, h, w]."""
    P = _cast(sd, dtype)
    qk, v, nomask = qk.to(dtype), v.to(dtype), nomask.to(dtype)
    b, dm, h, w = qk.shape
    dk, c = P["qk_w.weight"].shape[0] // 2, P["qk_w.weight"].shape[1]
    dv = P["v_w.weight"].shape[0]
    G = dm // c
    assert G * c == dm and P["fc.weight"].shape[1] == G * dv
    # the head view: image-head i = image i // G, channels (i % G) * c ... (utils.py:270-271)
    QK = F.conv2d(qk.reshape(b * G, c, h, w), P["qk_w.weight"], P["qk_w.bias"])
    V = F.conv2d(v.reshape(b * G, c, h, w), P["v_w.weight"], P["v_w.bias"])
    nm = nomask.repeat(G, 1, 1, 1)                   # image-head i reads nomask[i % b] (utils.py:272)
    att = R.local_dilated_attention(QK[:, :dk], QK[:, dk:], V, nm, dilation, c ** -0.5 if scale is None else scale)
    att = att.contiguous().view(b, G * dv, h, w)     # utils.py:300: heads back into the channels
    out = instance_norm_res(F.conv2d(att, P["fc.weight"], P["fc.bias"]), qk)
    if taps is not None:
        taps.update(QK=QK, V=V, att=att)
    return out


def multi_head_attention(sd, n_head, d_k, d_v, q, k, v, mask=None, last=False, dtype=torch.float64, taps=None):
    """MultiHeadAttention.forward, dropout off.  sd: w_qs, w_ks, w_vs, fc, layer_norm (.weight, .bias).
    q [b, lq, d_model], k, v [b, L, d_model], mask [b, lq, L] bool (True = masked; repeated per head).
    Returns (LayerNorm(fc(attention) + q), attn [(n_head*b), lq, L]) or, last=True, (sigmoid(q k^T).squeeze(1), None).
    A fully masked row is NaN in attn and in every element of its output row, like the reference's.  taps receives the
    head-major projections `q`, `k`, `v` [(n_head*b), l, d]."""
    P = _cast(sd, dtype)
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    b, lq, dm = q.shape
    L = k.shape[1]
    heads = lambda t, l, d: t.view(b, l, n_head, d).permute(2, 0, 1, 3).contiguous().view(-1, l, d)
    qh = heads(F.linear(q, P["w_qs.weight"], P["w_qs.bias"]), lq, d_k)
    kh = heads(F.linear(k, P["w_ks.weight"], P["w_ks.bias"]), L, d_k)
    vh = heads(F.linear(v, P["w_vs.weight"], P["w_vs.bias"]), L, d_v)
    if taps is not None:
        taps.update(q=qh, k=kh, v=vh)
    if last:
        return sdp_scores(qh, kh, True).squeeze(1), None
    m = mask.repeat(n_head, 1, 1) if mask is not None else None
    o, attn = R.sdp_attention(qh, kh, vh, d_k ** 0.5, m)
    o = o.view(n_head, b, lq, d_v).permute(1, 2, 0, 3).contiguous().view(b, lq, n_head * d_v)
    y = linear_ln(o.reshape(b * lq, -1), P["fc.weight"], P["fc.bias"], q.reshape(b * lq, dm), P["layer_norm.weight"],
                  P["layer_norm.bias"]).view(b, lq, dm)
    return y, attn


def sdp_attention(q, k, v, temperature, mask=None, dtype=torch.float64):
    return R.sdp_attention(q.to(dtype), k.to(dtype), v.to(dtype), temperature, mask)


def sdp_scores(q, k, sigmoid, dtype=None):
    """q [bh, lq, d], k [bh, L, d] -> q k^T [bh, lq, L], through a sigmoid where MultiHeadAttention applies one."""
    if dtype is not None:
        q, k = q.to(dtype), k.to(dtype)
    s = torch.bmm(q, k.transpose(1, 2))
    return torch.sigmoid(s) if sigmoid else s


def point_query_mask(q, enc, dtype=torch.float64):
    return R.point_query_mask(q.to(dtype), enc.to(dtype))
