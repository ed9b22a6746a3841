"""The instance head's hand-derived backward (csrc/head_bwd.hip) against float64 autograd through the oracle.

The reference trains the head with autograd; here every backward of the head is a hand-written kernel.  The whole-step
gate in test_gpu_train.py has to allow for ReLU6 threshold flips upstream, so a wrong term in one of these kernels can
hide inside it.  Each test below drives ONE layer along the product's own path (the InstanceHead method, or the C ABI in
the order instance_head.py uses), runs the same layer in float64 through oracle/reseg_ref.py with torch.autograd, and
compares the forward outputs and every gradient.  The chains are smooth (tanh, softmax, 3x3 means, BatchNorm without
ReLU6; the focal clamp is placed on purpose), so the bounds are fp32-tight.

Per tensor the tests print the relative L2 error and max|got - ref| / max|ref|.  Bounds, fp32 storage: both <= the
per-tensor value in BOUNDS (~10x the worst measured on MI355X, never above 1e-4, the backbone's bound in
test_backbone_gradients_tight_vs_oracle_f64).  bf16 storage: the reference reads the stored inputs rounded with q();
maps and parameter gradients the kernels keep in fp32 then carry the fp32 bound, stored outputs (out, dx, dpred, dup)
TOL[bf16] = 2e-2 (test_gpu_ops.py).

test_head_references_separate_a_missing_term (no GPU) shows that every bound separates a correct kernel from one that
misses a term: the float64 reference with one backward-relevant term changed moves the gradients by >= 100x the bound.
"""
import ctypes as C
import math
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import reseg_ref as R  # noqa: E402
from test_gpu_ops import TOL, _gpu, _run_backward, q, rand, to_act  # noqa: E402

gpu = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
NAN = float("nan")
SP, AT = "decoder.s_sp", "decoder.attend"

# fp32 bounds per compared tensor (relative L2 and max-abs / max|ref| alike); see the module docstring
BOUNDS = {
    # measured worst over the cases and both storage types (bf16: the tensors kept in fp32), MI355X
    "sp": {"out": 3e-6,                         # 2.2e-7
           "beta": 5e-6,                        # 4.2e-7
           "dx": 5e-6,                          # 4.2e-7
           "bn.weight": 5e-6,                   # 3.3e-7
           "bn.bias": 5e-6,                     # 3.7e-7
           "l_v.weight": 1e-5,                  # 7.9e-7
           "l_v.bias": 1e-4,                    # 1.1e-5 (sum of ddot over the masks: cancels)
           "l_h.weight": 6e-5,                  # 6.0e-6 (C = 520, one image)
           "spatial_fc.1.weight": 3e-5,         # 2.4e-6
           "spatial_fc.1.bias": 1e-6,           # 2.6e-8 of sum |dz| (the exact value is 0)
           "bn.running_mean": 2e-6,             # 9.3e-8
           "bn.running_var": 2e-6},             # 1.1e-7
    "ha": {"merge": 2e-6,                       # 2.1e-7
           "de": 2e-6,                          # 2.0e-7
           "ds": 2e-6,                          # 1.8e-7
           "bn.weight": 2e-6,                   # 1.8e-7
           "bn.bias": 3e-6,                     # 2.5e-7
           "l1.weight": 5e-6,                   # 4.5e-7
           "l1.bias": 1e-5,                     # 9.8e-7
           "attend_fc.1.weight": 5e-6,          # 4.1e-7
           "attend_fc.1.bias": 5e-6,            # 4.1e-7 of max|d attend_fc.1.weight|
           "bn.running_mean": 1e-6,             # 4.0e-8
           "bn.running_var": 1e-6},             # 7.8e-8
    "ins": {"alpha": 1e-6,                      # 8.5e-8
            "dmerge": 3e-5},                    # 2.6e-6 (relL2: fp32 rounding of old + grad where grad ~ 1/npix)
    "loss": {"dpred": 3e-6,                     # 2.5e-7
             "dmerge": 1e-6,                    # 6.6e-8
             "scal": 2e-6,                      # 1.5e-7
             "adv": 1e-6,                       # 6.3e-8
             "coef": 1e-6,                      # 4.8e-8
             "baseline": 5e-6},                 # 5.0e-7
    "gate": {"out": 1e-6,                       # 9.6e-8
             "dup": 2e-6,                       # 1.4e-7
             "dpred": 4e-6},                    # 3.2e-7
}
# stored in the activation type: bf16 storage is bounded by TOL[bf16]
STORED = {"sp": ("out", "dx"), "ha": ("de", "ds"), "loss": ("dpred",), "gate": ("out", "dup", "dpred")}
# hard attention with bf16 storage: s, its 3x3 mean, the 1x1 and 3x3 conv outputs and tanh are all stored in bf16 ahead
# of the maskBN, so every tensor of that layer carries those roundings: TOL[bf16] (measured worst 7.3e-3, l1.bias)
HA_BF16 = 2e-2


def _bound(layer, name, dtype):
    name = name.split()[0]                      # "dpred L3" -> "dpred"
    if dtype == torch.bfloat16 and (name in STORED[layer] or layer == "ha"):
        return TOL[torch.bfloat16] if layer != "ha" else HA_BF16
    return BOUNDS[layer][name]


def _err(got, ref, floor=0.0):
    """(relative L2, max-abs / max|ref|); `floor`: the magnitude scale for a tensor whose exact value cancels to ~0."""
    g, r = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    d = g - r
    l2 = float(d.norm()) / max(float(r.norm()), floor, 1e-300)
    mx = float(d.abs().max()) / max(float(r.abs().max()), floor, 1e-300)
    return l2, mx


def _check(tag, layer, dtype, items):
    """items: name -> (got, ref[, floor]).  Prints every error before asserting, so one run measures all of them."""
    bad, worst = [], 0.0
    for name, it in items.items():
        got, ref = it[0], it[1]
        floor = it[2] if len(it) > 2 else 0.0
        assert got.numel() == ref.numel(), name
        l2, mx = _err(got, ref, floor)
        b = _bound(layer, name, dtype)
        worst = max(worst, l2, mx)
        ok = l2 <= b and mx <= b          # NaN fails
        print("  %-44s %-22s relL2 %.2e  max %.2e  bound %.0e%s" % (tag, name, l2, mx, b, "" if ok else "  FAIL"))
        if not ok:
            bad.append((name, l2, mx, b))
    print("  %-44s worst %.2e" % (tag, worst))
    assert not bad, bad


def _nan_act(Act, n, h, w, c, dtype, ld=None, c0=0):
    ld = ld or (c + 7) // 8 * 8
    return Act(torch.full((n, h, w, ld), NAN, dtype=dtype, device="cuda"), c0, c)


def _engine(P, dtype):
    L, Act, Engine, ParamStore, Pro = _gpu()
    schema = [(k, tuple(v.shape)) for k, v in P.items()]
    schema += [(k.replace("running_mean", "num_batches_tracked"), ()) for k in P if k.endswith("running_mean")]
    ps = ParamStore(schema, "cuda")
    ps.load_state_dict(P)
    eng = Engine(ps, dtype)
    eng.begin(bn_train=True, record=True)
    from isa_amd.instance_head import InstanceHead
    return eng, ps, InstanceHead(types.SimpleNamespace(E=eng))


def _record(obj, name):
    """Record what obj.name returns (an instance attribute shadowing the method; del obj.name restores it)."""
    orig, got = getattr(obj, name), []

    def rec(*a, **k):
        t = orig(*a, **k)
        got.append(t)
        return t
    setattr(obj, name, rec)
    return got


def _preset_grad(eng, a, old, dtype):
    """Gradient of `a` already written by another consumer: the next writer must accumulate into it."""
    g = eng.grads.grad_of(a)
    g.buf[..., g.c0:g.c0 + g.c] = old.permute(0, 2, 3, 1).to(dtype).cuda()
    eng.grads.written[a.buf.data_ptr()].append((a.c0, a.c0 + a.c))


def _leaf(P):
    out = {}
    for k, v in P.items():
        if "running" in k:
            out[k] = v.double().clone()
        else:
            out[k] = v.double().clone().requires_grad_(True)
        if k.endswith("running_mean"):
            out[k.replace("running_mean", "num_batches_tracked")] = torch.zeros((), dtype=torch.long)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatements with one switchable term.  Each is checked against the oracle function it restates (as written)
# in test_head_references_separate_a_missing_term before its perturbed form is used.
# ---------------------------------------------------------------------------------------------------------------------
def _spatial_attention(P, x, m, ctx, use_ht=True, empty_zero=False):
    """R.spatial_attention; use_ht=False drops h_t; empty_zero: an image with an empty mask gets beta = 0 where the
    reference's softmax gives NaN (the HIP convention, test_gpu_row_softmax.py)."""
    b, c, h, w = x.shape
    xm = x * m
    base = F.conv2d(xm, P[SP + ".l_v.weight"], P[SP + ".l_v.bias"])
    if use_ht:
        ht = F.linear(xm.reshape(b, c, -1).mean(2), P[SP + ".l_h.weight"])
        base = base + ht[:, :, None, None]
    z = F.conv2d(torch.tanh(base), P[SP + ".spatial_fc.1.weight"], P[SP + ".spatial_fc.1.bias"])
    z = z.masked_fill(m < 0.5, float("-inf")).reshape(b, 1, -1)
    msum = m.sum((1, 2, 3), keepdim=True)
    if empty_zero:      # finite logits for an empty row, times msum = 0: beta = 0 with a zero gradient, no NaN anywhere
        z = torch.where(msum.reshape(b, 1, 1) > 0, z, torch.zeros_like(z))
    beta = torch.softmax(z, 2).reshape(b, 1, h, w) * msum
    ctx.tap("s_sp.beta", beta)
    return x + R.batchnorm(P, SP + ".bn", x * beta, ctx) * m


def _mask_bn(P, pre, x, m, ctx, plus_one=True):
    """R.mask_bn (train mode); plus_one=False drops the +1 of the per-image denominator."""
    b, c, h, w = x.shape
    den = m.reshape(b, -1).sum(1) + (1 if plus_one else 0)
    xf, mf = x.reshape(b, c, -1), m.reshape(b, 1, -1)
    mean = ((xf * mf).sum(2) / den[:, None]).mean(0)
    var = ((((xf - mean[None, :, None]) ** 2) * mf).sum(2) / den[:, None]).mean(0)
    with torch.no_grad():
        f = R.BN_MOMENTUM
        ctx.new_buffers[pre + ".running_mean"] = P[pre + ".running_mean"] * f + (1 - f) * mean
        ctx.new_buffers[pre + ".running_var"] = P[pre + ".running_var"] * f + (1 - f) * var
    return (x - mean[None, :, None, None]) / torch.pow(var[None, :, None, None] + R.BN_EPS, 0.5) \
        * P[pre + ".weight"][None, :, None, None] + P[pre + ".bias"][None, :, None, None]


def _focal_map(logits, target, detach=True):
    """R.focal_map; detach=False lets the gradient through the modulating factor (1 - p)^2."""
    p = torch.softmax(logits, 1)
    pt = p.detach() if detach else p
    pc = p.clamp(1e-7, 1.0 - 1e-7)
    t = target[:, 0]
    return -((1 - pt[:, 1]) ** R.FOCAL_GAMMA) * torch.log(pc[:, 1]) * t \
        - ((1 - pt[:, 0]) ** R.FOCAL_GAMMA) * torch.log(pc[:, 0]) * (1 - t)


def _atten_loss(preds, targets, alpha, s_t, state, ema_first=True, detach=True):
    """The training branch of R.atten_loss -> loss_finite; ema_first=False updates the EMA baseline after the advantage
    is taken (attenet2.py:266 updates it before)."""
    b = alpha.shape[0]
    loss_pred = 0
    for p, t, wl in zip(preds, targets, R.PYRAMID_W):
        focal = _focal_map(p, t, detach).reshape(b, -1).mean(1)
        loss_pred = loss_pred + (R.CE_WEIGHT * focal + R.dice_fg_loss(p, t, time=1)) * wl
    with torch.no_grad():
        log_p_y = -R.dice_fg_loss(preds[-1], targets[-1], time=1)
        new_base = 0.9 * state.baseline + 0.1 * float(log_p_y.mean())
    base = new_base if ema_first else state.baseline
    state.baseline = new_base
    a = alpha.reshape(b, -1)
    picked = torch.stack([a[i, s_t[i]] for i in range(b)])
    per_img = R.LAMBDA_L * loss_pred + R.LAMBDA_R * (-(log_p_y - base) * torch.log(picked))
    return R.LAMBDA_INS * per_img.sum() / b


def _ins_alpha(merge, planes):
    """alpha[b] = softmax of merge[b] over the pixels of planes[b] (utils.py:648-655); an empty plane gives a zero row."""
    rows = []
    for z, pl in zip(merge, planes):
        if bool(pl.any()):
            rows.append(torch.softmax(z.masked_fill(~pl, float("-inf")), 0))
        else:
            rows.append(torch.zeros_like(z))
    return torch.stack(rows)


# ---------------------------------------------------------------------------------------------------------------------
# 1. SpatialAttentionLayer: InstanceHead.spatial_attention -> isa_sp_bwd
# ---------------------------------------------------------------------------------------------------------------------
SP_DENSITY = (0.12, 0.92, 0.5, 0.3, 0.75)         # image b: sparse, dense, ...


def _sp_inputs(n, C, H, W, empty):
    g = torch.Generator().manual_seed(n * 1000 + C * 10 + H)
    off = torch.linspace(-1.0, 1.5, C)                       # channel offsets: h_t and the BN(v) means are not ~0
    x = rand(n, C, H, W, seed=11) + off[None, :, None, None]
    dens = SP_DENSITY if n > 1 else (0.5,)
    sem = torch.stack([(torch.rand(H, W, generator=g) < dens[b % len(dens)]).float() for b in range(n)])
    if empty is not None:
        sem[empty] = 0.0
    dy = rand(n, C, H, W, seed=12)
    if empty is not None:
        dy[empty] *= 1e3                                       # must not leak anywhere but into its own dx
    P = {SP + ".l_v.weight": rand(1, C, 1, 1, seed=13, scale=C ** -0.5), SP + ".l_v.bias": torch.tensor([0.2]),
         SP + ".l_h.weight": rand(1, C, seed=14, scale=C ** -0.5), SP + ".spatial_fc.1.weight": torch.tensor([[[[1.7]]]]),
         SP + ".spatial_fc.1.bias": torch.tensor([-0.3]), SP + ".bn.weight": rand(C, seed=15).abs() + 0.5,
         SP + ".bn.bias": rand(C, seed=16) * 0.1, SP + ".bn.running_mean": rand(C, seed=17) * 0.1,
         SP + ".bn.running_var": rand(C, seed=18).abs() + 0.5}
    return x, sem, dy, P


def _sp_reference(x, sem, dy, P, dtype, empty_zero=False):
    P64 = _leaf(P)
    xr = q(x, dtype).double().requires_grad_(True)
    ctx = R.Ctx(bn_train=True, capture=True)
    m = sem.double()[:, None]
    if empty_zero:
        out = _spatial_attention(P64, xr, m, ctx, empty_zero=True)
    else:
        out = R.spatial_attention(P64, xr, m, ctx)
    beta = ctx.taps["s_sp.beta"]
    beta.retain_grad()
    out.backward(q(dy, dtype).double())
    b = x.shape[0]
    bb, db = beta.detach().reshape(b, -1), beta.grad.reshape(b, -1)
    cnt = m.reshape(b, -1).sum(1, keepdim=True).clamp_min(1)
    dz = bb * (db - (bb * db).sum(1, keepdim=True) / cnt)         # gradient of the softmax logits
    return dict(out=out.detach(), beta=beta.detach()[:, 0], dx=xr.grad, P=P64, ctx=ctx, dz_l1=float(dz.abs().sum()))


def _sp_run(x, sem, dy, P, dtype, acc, old=None):
    L, Act, Engine, ParamStore, Pro = _gpu()
    eng, ps, head = _engine(P, dtype)
    n, C, H, W = x.shape
    xa = to_act(Act, x, dtype)
    maps = _record(eng, "f32")
    out = head.spatial_attention(xa, sem.reshape(n, -1).float().cuda().contiguous())
    del eng.f32
    beta = maps[0]                     # spatial_attention's first fp32 map is beta (instance_head.py:84)
    assert beta.numel() == n * H * W
    out_f = out.nchw().cpu()
    if acc:
        _preset_grad(eng, xa, old, dtype)
    _run_backward(eng, out, dy, Act)
    res = dict(out=out_f, beta=beta.view(n, H, W).float().cpu(), dx=eng.grads.grad_of(xa).nchw().cpu())
    for k in P:
        res[k] = (ps.view(k) if "running" in k else ps.gview(k)).detach().cpu().clone()
    return res


SP_CASES = [  # n, C, H, W, accumulate; the head_bwd.hip branch each case reaches
    (2, 24, 64, 64, 0),        # the network's shape: hw % 256 == 0 (aligned dbeta), one 4096-pixel chunk, fixed reduce
    (3, 24, 72, 72, 1),        # not aligned, two chunks with a ragged tail (5184 = 4096 + 1088), n % 4 != 0
    (5, 24, 9, 37, 0),         # 333 pixels per image: waves straddle images in the dbeta pass
    (2, 20, 16, 16, 1),        # channel tail (C % 8 = 4)
    (2, 8, 33, 33, 0),         # cg = 1
    (1, 520, 8, 8, 1),         # cg = 65 >= 64: non-fixed reduce / dx flush path, one image
]


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,C,H,W,acc", SP_CASES)
def test_spatial_attention_grads(dtype, n, C, H, W, acc):
    """SpatialAttentionLayer forward + isa_sp_bwd vs float64 autograd of R.spatial_attention.  Measured worst on MI355X:
    fp32 6.0e-6 (l_h.weight, C = 520), bf16 3.2e-3 (the stored out / dx; the fp32 tensors 1.1e-5).  Per tensor: BOUNDS."""
    _sp_case(dtype, n, C, H, W, acc, empty=None)


@gpu
@pytest.mark.parametrize("dtype,n,C,H,W,empty", [(torch.float32, 3, 24, 72, 72, 1), (torch.bfloat16, 5, 24, 9, 37, 3)])
def test_spatial_attention_empty_mask(dtype, n, C, H, W, empty):
    """One image without foreground: beta = 0 there (the softmax's NaN -> 0), its pixels still count in the BN(v)
    statistics, it adds exactly nothing to any parameter gradient (its dout is scaled by 1e3 so that any leak shows), and
    its dx is dout exactly.  Measured worst on MI355X: fp32 1.1e-6, bf16 2.1e-3 (stored out / dx)."""
    _sp_case(dtype, n, C, H, W, 1, empty=empty)


def _sp_case(dtype, n, C, H, W, acc, empty):
    x, sem, dy, P = _sp_inputs(n, C, H, W, empty)
    old = rand(n, C, H, W, seed=19) if acc else None
    got = _sp_run(x, sem, dy, P, dtype, acc, old)
    ref = _sp_reference(x, sem, dy, P, dtype, empty_zero=empty is not None)
    dx = got["dx"] - (q(old, dtype) if acc else 0.0)
    keep = [b for b in range(n) if b != empty]
    items = dict(out=(got["out"][keep], ref["out"][keep]), beta=(got["beta"], ref["beta"]), dx=(dx[keep], ref["dx"][keep]))
    for k, v in ref["P"].items():
        if not k.startswith(SP) or "num_batches" in k:
            continue
        name = k[len(SP) + 1:]
        if "running" in k:
            items[name] = (got[k], ref["ctx"].new_buffers[k])
        else:
            floor = ref["dz_l1"] if name == "spatial_fc.1.bias" else 0.0     # sum of dz: exactly 0 by shift invariance
            items[name] = (got[k], v.grad, floor)
    _check("sp n%d C%d %dx%d acc%d %s%s" % (n, C, H, W, acc, str(dtype)[6:], "" if empty is None else " empty"),
           "sp", dtype, items)
    if empty is not None:
        assert float(got["beta"][empty].abs().max()) == 0.0
        assert torch.equal(got["out"][empty], q(x[empty], dtype)), "empty mask: out = x"
        dout_e = q(dy[empty], dtype)
        if acc:
            # dx = old + dout: one fp32 add of stored values, then the store (bf16: one rounding)
            assert torch.equal(got["dx"][empty], q(q(old[empty], dtype) + dout_e, dtype)), "empty mask: dx = dout"
        else:
            assert torch.equal(got["dx"][empty], dout_e), "empty mask: dx = dout"


# ---------------------------------------------------------------------------------------------------------------------
# 2. HardAttentionLayer front + maskBN: InstanceHead.hard_attention_scores -> isa_maskbn_bwd, conv backward, avgpool3
# ---------------------------------------------------------------------------------------------------------------------
def _ha_params():
    sd = R.synth_state_dict(23, True)
    return {k: v for k, v in sd.items() if k.startswith(AT + ".") and ".l2." not in k and "num_batches" not in k}


def _ha_inputs(n, H, W, empty):
    g = torch.Generator().manual_seed(100 + n * 7 + H)
    s = rand(n, 24, H, W, seed=21) + torch.linspace(-0.5, 0.8, 24)[None, :, None, None]
    dens = (0.35, 0.8, 0.15, 0.6)
    sem = torch.stack([(torch.rand(H, W, generator=g) < dens[b % 4]).float() for b in range(n)])
    if empty is not None:
        sem[empty] = 0.0
    dmerge = rand(n, H, W, seed=22)
    return s, sem, dmerge


def _ha_reference(s, sem, dmerge, P, dtype, old_e=None, old_s=None, plus_one=True):
    P64 = _leaf(P)
    sr = q(s, dtype).double().requires_grad_(True)
    n, _, H, W = s.shape
    cap = []
    orig = R.mask_bn

    def mask_bn(P_, pre, x, m, ctx):            # the oracle's own maskBN (or the restatement), capturing its input e
        x.retain_grad()
        cap.append(x)
        return orig(P_, pre, x, m, ctx) if plus_one else _mask_bn(P_, pre, x, m, ctx, plus_one=False)
    R.mask_bn = mask_bn
    try:
        ctx = R.Ctx(bn_train=True)
        _, merge = R.hard_attention(P64, sr, sem.double()[:, None], torch.ones(n, 1, H, W, dtype=torch.float64), ctx)
    finally:
        R.mask_bn = orig
    e = cap[0]
    loss = (merge[:, 0] * dmerge.double()).sum()
    if old_e is not None:
        loss = loss + (e * old_e.double()).sum()          # the e gradient another consumer had already written
    loss.backward()
    ds = sr.grad + (old_s.double() if old_s is not None else 0.0)
    return dict(merge=merge.detach()[:, 0], de=e.grad, ds=ds, P=P64, ctx=ctx)


HA_CASES = [  # n, H, W, empty-sem image, accumulate
    (1, 16, 16, None, 0),
    (4, 15, 17, 2, 1),        # odd H x W: the 3x3 means' borders; den = 0 + 1 for image 2
    (4, 24, 20, None, 0),
]


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,H,W,empty,acc", HA_CASES)
def test_hard_attention_grads(dtype, n, H, W, empty, acc):
    """avgpool3 -> l1 -> tanh -> attend_fc (3x3) -> maskBN -> avgpool3 * sem = merge, then a random dmerge backwards
    through isa_maskbn_bwd, the conv backward and isa_avgpool3 (accumulate), vs float64 autograd of R.hard_attention.
    acc = 1: the gradients of e (isa_maskbn_bwd's output) and of s (isa_avgpool3's) already hold known values.
    Measured worst on MI355X: fp32 9.8e-7 (l1.bias), bf16 7.3e-3 (l1.bias)."""
    L, Act, Engine, ParamStore, Pro = _gpu()
    P = _ha_params()
    s, sem, dmerge = _ha_inputs(n, H, W, empty)
    old_e = rand(n, 1, H, W, seed=23) if acc else None
    old_s = rand(n, 24, H, W, seed=24) if acc else None
    eng, ps, head = _engine(P, dtype)
    sa = to_act(Act, s, dtype)
    acts = _record(eng, "new_act")
    merge = head.hard_attention_scores(sa, sem.reshape(n, -1).float().cuda().contiguous())
    del eng.new_act
    e2 = [a for a in acts if a.c == 1]
    assert len(e2) == 1                                # the attend_fc output: the maskBN input e
    e2 = e2[0]
    merge_f = merge.view(n, H, W).cpu().clone()
    running = {k: ps.view(k).cpu().clone() for k in P if "running" in k}
    head.dmerge[:n * H * W].copy_(dmerge.reshape(-1).cuda())
    if acc:
        _preset_grad(eng, e2, old_e, dtype)
        _preset_grad(eng, sa, old_s, dtype)
    eng.backward()
    torch.cuda.synchronize()
    ref = _ha_reference(s, sem, dmerge, P, dtype, q(old_e, dtype) if acc else None, q(old_s, dtype) if acc else None)
    items = dict(merge=(merge_f, ref["merge"]), de=(eng.grads.grad_of(e2).nchw().cpu(), ref["de"]),
                 ds=(eng.grads.grad_of(sa).nchw().cpu(), ref["ds"]))
    for k, v in ref["P"].items():
        if "num_batches" in k:
            continue
        name = k[len(AT) + 1:]
        if "running" in k:
            items[name] = (running[k], ref["ctx"].new_buffers[k])
        else:
            # attend_fc.1.bias: maskBN removes (almost) every constant shift of e - the gradient is a small remainder
            # of the weight gradient's terms, so it is measured against that scale
            floor = float(ref["P"][AT + ".attend_fc.1.weight"].grad.abs().max()) if name == "attend_fc.1.bias" else 0.0
            items[name] = (ps.gview(k).cpu(), v.grad, floor)
    _check("ha n%d %dx%d empty%s acc%d %s" % (n, H, W, empty, acc, str(dtype)[6:]), "ha", dtype, items)
    if empty is not None:
        assert float(merge_f[empty].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 3. instance softmax + REINFORCE: isa_ins_softmax -> isa_ins_softmax_bwd
# ---------------------------------------------------------------------------------------------------------------------
def _ins_planes(nsrc, nobj, L, seed):
    """[nsrc, nobj, L] int64 instance planes; the last plane of the last image is empty (nobj = 1: image nsrc-1 has
    no instance pixels at all)."""
    g = torch.Generator().manual_seed(seed)
    if nobj == 1:
        ins = (torch.rand(nsrc, 1, L, generator=g) < 0.6).long()
        ins[:, 0, 0] = 1
        ins[:, 0, L - 1] = 1
        ins[:, 0, min(4095, L - 1)] = 1
    else:
        owner = torch.randint(0, nobj - 1, (nsrc, L), generator=g)
        ins = torch.stack([(owner == k) for k in range(nobj)], 1).long()
    ins[nsrc - 1, nobj - 1] = 0
    return ins


def _ins_rows(ins, iters, seed):
    """idx / s_t of iters * nsrc rows [it*nsrc + image]: s_t on the first pixel, the last pixel, the last pixel of the
    first 4096-pixel chunk, then random pixels of the instance; one row selects the empty instance."""
    nsrc, nobj, L = ins.shape
    g = torch.Generator().manual_seed(seed)
    idx, s_t = [], []
    for it in range(iters):
        for b in range(nsrc):
            want = (0, L - 1, min(4095, L - 1))[it] if it < 3 else -1
            if nobj == 1:
                k = 0
            elif want >= 0:
                k = int(ins[b, :, want].nonzero()[0, 0])
            else:
                k = int(torch.randint(0, nobj - 1, (1,), generator=g))
            if b == nsrc - 1 and it == iters - 1:
                k = nobj - 1                                   # the empty instance
            pix = ins[b, k].nonzero()[:, 0]
            if len(pix) == 0:
                p = 0
            elif want >= 0 and bool(ins[b, k, want]):
                p = want
            else:
                p = int(pix[int(torch.randint(0, len(pix), (1,), generator=g))])
            idx.append(k)
            s_t.append(p)
    return torch.tensor(idx, dtype=torch.int32), torch.tensor(s_t, dtype=torch.int32)


@gpu
@pytest.mark.parametrize("nobj,L", [(1, 4096), (5, 5184), (5, 1000), (1, 5184)])
def test_ins_softmax_reinforce_grads(nobj, L):
    """Three decoder iterations in one call (n = 3 * nsrc rows, each accumulating into its image's dmerge row, no atomics)
    vs float64 autograd of -sum_b adv[b] * log(alpha[b, s_t[b]]) w.r.t. merge.  dmerge starts from known values (the
    kernel always adds); an instance without pixels leaves its rows untouched.  Measured worst on MI355X: 2.6e-6."""
    Lm, Act, Engine, ParamStore, Pro = _gpu()
    nsrc, iters = 3, 3
    n = nsrc * iters
    ins = _ins_planes(nsrc, nobj, L, seed=31)
    idx, s_t = _ins_rows(ins, iters, seed=32)
    merge = rand(nsrc, L, seed=33, scale=2.0)
    adv = rand(n, seed=34)
    m64 = merge.double().requires_grad_(True)
    planes = [ins[b % nsrc, int(idx[b])] != 0 for b in range(n)]
    a_ref = _ins_alpha(torch.stack([m64[b % nsrc] for b in range(n)]), planes)
    loss = 0
    for b in range(n):
        if bool(planes[b].any()):
            loss = loss - adv[b].double() * torch.log(a_ref[b, int(s_t[b])])
    loss.backward()
    old = rand(nsrc, L, seed=35) * float(m64.grad.abs().max())      # known values of the gradient's magnitude
    dev = "cuda"
    st = torch.cuda.current_stream().cuda_stream
    alpha = torch.full((n * L,), NAN, device=dev)
    rowstat = torch.full((2 * n,), NAN, device=dev)
    part = torch.full((n * 64 * 4,), NAN, device=dev)
    ins_d, idx_d, s_t_d, merge_d = ins.to(dev), idx.to(dev), s_t.to(dev), merge.to(dev)
    Lm.check(Lm.lib().isa_ins_softmax(Lm.ptr(merge_d), Lm.ptr(ins_d), Lm.ptr(idx_d), n, nobj, L, Lm.ptr(alpha),
                                      Lm.ptr(rowstat), nsrc, Lm.ptr(part), st), "isa_ins_softmax")
    dmerge = old.clone().to(dev)
    adv_d = adv.to(dev)
    Lm.check(Lm.lib().isa_ins_softmax_bwd(Lm.ptr(alpha), Lm.ptr(ins_d), Lm.ptr(idx_d), Lm.ptr(s_t_d), Lm.ptr(adv_d), n,
                                          nobj, L, Lm.ptr(dmerge), nsrc, st), "isa_ins_softmax_bwd")
    torch.cuda.synchronize()
    got_d = dmerge.cpu() - old
    _check("ins nobj%d L%d" % (nobj, L), "ins", torch.float32,
           dict(alpha=(alpha.view(n, L).cpu(), a_ref.detach()), dmerge=(got_d, m64.grad)))
    for b in range(n):
        if not bool(planes[b].any()):
            assert float(alpha.view(n, L)[b].abs().max()) == 0.0
    if nobj == 1:          # image nsrc-1 has no instance pixels: all its rows are empty, its dmerge row is untouched
        assert torch.equal(dmerge[nsrc - 1].cpu(), old[nsrc - 1])
    # the rows reach the positions the cases are about
    assert {0, L - 1, min(4095, L - 1)} <= set(int(v) for v in s_t)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the loss chain: isa_pool_target, isa_mask_loss_sums x 5, isa_head_loss, isa_mask_loss_grad x 5, isa_ins_softmax_bwd
# ---------------------------------------------------------------------------------------------------------------------
FACTORS = (16, 8, 4, 2, 1)                 # pyramid levels (instance_head.py:27)


def _loss_inputs(B, G, H, W, nobj):
    g = torch.Generator().manual_seed(41)
    owner = torch.randint(0, nobj - 1, (B, H // 8, W // 8), generator=g)
    owner = owner.repeat_interleave(8, 1).repeat_interleave(8, 2).reshape(B, -1)     # blocky instances
    ins = torch.stack([(owner == k) for k in range(nobj)], 1).long()                 # plane nobj-1 is empty
    idx_a = torch.randint(0, nobj - 1, (G, B), generator=g).int()
    idx_t = idx_a.clone()
    idx_t[:, 1] = nobj - 1                 # image 1: its target is empty at every level (alpha keeps a real instance)
    s_t = torch.zeros(G, B, dtype=torch.int32)
    for it in range(G):
        for b in range(B):
            pix = ins[b, int(idx_a[it, b])].nonzero()[:, 0]
            s_t[it, b] = int(pix[int(torch.randint(0, len(pix), (1,), generator=g))])
    merge = rand(B, H * W, seed=42, scale=1.5)
    preds = []
    for lvl, f in enumerate(FACTORS):
        p = rand(G * B, 2, H // f, W // f, seed=43 + lvl, scale=1.5)
        sat = torch.where(rand(G * B, 1, H // f, W // f, seed=50 + lvl) > 0, 25.0, -25.0)
        for it in range(G):
            p[it * B + 2, 1] = p[it * B + 2, 0] + sat[it * B + 2, 0]                   # image 2: |l1 - l0| = 25
        preds.append(p)
    return ins, idx_a, idx_t, s_t, merge, preds


def _loss_reference(ins, idx_a, idx_t, s_t, merge, preds, dtype, b0, G, ema_first=True, detach=True):
    """Gradient of inv_iter * sum_it loss_finite_it (instance_head.py:464 passes inv_iter = 1/max_iter; R.atten_loss
    divides by b and applies LAMBDA_L / LAMBDA_R, the kernel folds those into coef and adv), float64."""
    B = merge.shape[0]
    H = W = int(round(math.sqrt(merge.shape[1])))
    m64 = merge.double().requires_grad_(True)
    P = [q(p, dtype).double().requires_grad_(True) for p in preds]
    state = R.HeadState(baseline=b0)
    total, scal = 0, [0.0] * 4
    adv, coef = [], []
    for it in range(G):
        planes = [ins[b, int(idx_a[it, b])] != 0 for b in range(B)]
        alpha = _ins_alpha(m64, planes).reshape(B, 1, H, W)
        gold = torch.stack([ins[b, int(idx_t[it, b])] for b in range(B)]).reshape(B, 1, H, W).double()
        targets = [F.max_pool2d(gold, f) if f > 1 else gold for f in FACTORS]
        pr = [p[it * B:(it + 1) * B] for p in P]
        stl = [int(v) for v in s_t[it]]
        if ema_first and detach:
            out = R.atten_loss(pr, targets, alpha, stl, True, state)
            lf = out["loss_finite"]
            scal[1] += float(out["criterion"]) / G
            scal[2] += float(out["ce"]) / G
            scal[3] += float(out["dice"].mean()) / G
            lp = -out["dice"].detach()
        else:
            lf = _atten_loss(pr, targets, alpha, stl, state, ema_first=ema_first, detach=detach)
            lp = None
        scal[0] += float(lf.detach()) / G
        total = total + lf / G
        if lp is not None:
            adv.append((1.0 / G) / B * R.LAMBDA_R * (lp - state.baseline))
            for lvl, (p, t) in enumerate(zip(pr, targets)):      # {c_t, c_1, c_focal} from float64 sums
                pp = torch.softmax(p.detach(), 1)[:, 1]
                A, S, T = (pp * t[:, 0]).sum((1, 2)), pp.sum((1, 2)), t[:, 0].sum((1, 2))
                den = S + T + 1
                g = (1.0 / G) / B * R.LAMBDA_L * R.PYRAMID_W[lvl]
                coef.append((lvl, it, torch.stack([g * -2 / den, g * (2 * A + 1) / den ** 2,
                                                   torch.full_like(den, g * R.CE_WEIGHT / t[0, 0].numel())], 1)))
    total.backward()
    return dict(dpred=[p.grad for p in P], dmerge=m64.grad, scal=torch.tensor(scal, dtype=torch.float64),
                adv=torch.cat(adv) if adv else None, coef=coef, baseline=state.baseline)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("calls,acc", [(1, 0), (1, 1), (2, 0)])
def test_loss_chain_grads(dtype, calls, acc):
    """B = 3 images, two decoder iterations, 64 x 64: image 1's target is empty at every level, image 2's logits are
    saturated (|l1 - l0| = 25: the focal clamp's zero-gradient branch on both channels).  calls = 1: ONE isa_head_loss
    with iters = 2 (the batched pass); calls = 2: two calls with iters = 1 (the per-iteration pass).  Either way the
    baseline is carried in iteration order (attenet2.py:266).  acc = 1: dpred already holds known values.
    Measured worst on MI355X: fp32 5.0e-7 (baseline), bf16 9.8e-3 (the stored dpred, acc = 1; the fp32 tensors 3.1e-7)."""
    Lm, Act, Engine, ParamStore, Pro = _gpu()
    B, G, H, W, nobj = 3, 2, 64, 64, 4
    Lp, R_ = H * W, G * B
    ins, idx_a, idx_t, s_t, merge, preds = _loss_inputs(B, G, H, W, nobj)
    b0 = 0.137
    ref = _loss_reference(ins, idx_a, idx_t, s_t, merge, preds, dtype, b0, G)
    dev = "cuda"
    st = torch.cuda.current_stream().cuda_stream
    lib = Lm.lib()
    ins_d, merge_d = ins.to(dev), merge.to(dev)
    ia, it_, s_d = idx_a.reshape(-1).to(dev), idx_t.reshape(-1).to(dev), s_t.reshape(-1).to(dev)
    alpha = torch.full((R_ * Lp,), NAN, device=dev)
    Lm.check(lib.isa_ins_softmax(Lm.ptr(merge_d), Lm.ptr(ins_d), Lm.ptr(ia), R_, nobj, Lp, Lm.ptr(alpha),
                                 Lm.ptr(torch.full((2 * R_,), NAN, device=dev)), B,
                                 Lm.ptr(torch.full((R_ * 256,), NAN, device=dev)), st), "isa_ins_softmax")
    targets, pa, dpa, olds = [], [], [], []
    for lvl, f in enumerate(FACTORS):
        t = torch.full((R_ * (H // f) * (W // f),), NAN, device=dev)
        Lm.check(lib.isa_pool_target(Lm.ptr(ins_d), Lm.ptr(it_), None, nobj, R_, H, W, f, Lm.ptr(t), B, st), "isa_pool_target")
        targets.append(t)
        pa.append(to_act(Act, preds[lvl], dtype))
        if acc:
            old = rand(*preds[lvl].shape, seed=60 + lvl) * float(ref["dpred"][lvl].abs().max())   # the gradient's scale
            olds.append(q(old, dtype))
            dpa.append(to_act(Act, old, dtype))
        else:
            dpa.append(_nan_act(Act, R_, H // f, W // f, 2, dtype))
    baseline = torch.tensor([b0], device=dev)
    scal_old = torch.tensor([0.5, -0.25, 1.0, 2.0])
    scal = scal_old.clone().to(dev)
    level_w = (C.c_float * 5)(*R.PYRAMID_W)
    dmerge = torch.zeros(B * Lp, device=dev)                  # zeroed scratch in the network (instance_head.py:155)
    coefs, advs = [], []
    if calls == 1:
        sums = torch.zeros(5 * 8 * R_, device=dev)
        for lvl in range(5):
            Lm.check(lib.isa_mask_loss_sums(pa[lvl].d(), Lm.ptr(targets[lvl]), None, Lm.ptr(sums[lvl * 8 * R_:]), st),
                     "isa_mask_loss_sums")
        coef, adv = torch.full((5 * 4 * R_,), NAN, device=dev), torch.full((R_,), NAN, device=dev)
        Lm.check(lib.isa_head_loss(Lm.ptr(sums), Lm.ptr(alpha), Lm.ptr(s_d), Lp, B, level_w, R.CE_WEIGHT, R.LAMBDA_L,
                                   R.LAMBDA_R, 1.0 / G, Lm.ptr(baseline), 1, Lm.ptr(coef), Lm.ptr(adv), Lm.ptr(scal), G, st),
                 "isa_head_loss")
        for lvl in range(5):
            Lm.check(lib.isa_mask_loss_grad(pa[lvl].d(), Lm.ptr(targets[lvl]), None, Lm.ptr(coef[lvl * 4 * R_:]),
                                            dpa[lvl].d(), acc, st), "isa_mask_loss_grad")
        Lm.check(lib.isa_ins_softmax_bwd(Lm.ptr(alpha), Lm.ptr(ins_d), Lm.ptr(ia), Lm.ptr(s_d), Lm.ptr(adv), R_, nobj, Lp,
                                         Lm.ptr(dmerge), B, st), "isa_ins_softmax_bwd")
        c4 = coef.view(5, G, B, 4)
        coefs = [c4[:, i] for i in range(G)]
        advs = [adv[i * B:(i + 1) * B] for i in range(G)]
    else:
        for i in range(G):
            sums = torch.zeros(5 * 8 * B, device=dev)
            pv = [p.images(i * B, B) for p in pa]
            tv = [t[i * B * t.numel() // R_:] for t in targets]
            for lvl in range(5):
                Lm.check(lib.isa_mask_loss_sums(pv[lvl].d(), Lm.ptr(tv[lvl]), None, Lm.ptr(sums[lvl * 8 * B:]), st),
                         "isa_mask_loss_sums")
            coef, adv = torch.full((5 * 4 * B,), NAN, device=dev), torch.full((B,), NAN, device=dev)
            al, sv = alpha[i * B * Lp:], s_d[i * B:]
            Lm.check(lib.isa_head_loss(Lm.ptr(sums), Lm.ptr(al), Lm.ptr(sv), Lp, B, level_w, R.CE_WEIGHT, R.LAMBDA_L,
                                       R.LAMBDA_R, 1.0 / G, Lm.ptr(baseline), 1, Lm.ptr(coef), Lm.ptr(adv), Lm.ptr(scal), 1,
                                       st), "isa_head_loss")
            for lvl in range(5):
                Lm.check(lib.isa_mask_loss_grad(pv[lvl].d(), Lm.ptr(tv[lvl]), None, Lm.ptr(coef[lvl * 4 * B:]),
                                                dpa[lvl].images(i * B, B).d(), acc, st), "isa_mask_loss_grad")
            Lm.check(lib.isa_ins_softmax_bwd(Lm.ptr(al), Lm.ptr(ins_d), Lm.ptr(ia[i * B:]), Lm.ptr(sv), Lm.ptr(adv), B, nobj,
                                             Lp, Lm.ptr(dmerge), B, st), "isa_ins_softmax_bwd")
            coefs.append(coef.view(5, B, 4))
            advs.append(adv)
    torch.cuda.synchronize()
    items = {}
    for lvl in range(5):
        got = dpa[lvl].nchw().cpu() - (olds[lvl] if acc else 0.0)
        items["dpred L%d" % lvl] = (got, ref["dpred"][lvl])
    items["dmerge"] = (dmerge.view(B, Lp).cpu(), ref["dmerge"])
    items["scal"] = (scal.cpu() - scal_old, ref["scal"])
    items["adv"] = (torch.cat(advs).cpu(), ref["adv"])
    items["coef"] = (torch.stack([coefs[i][lvl, :, :3] for lvl, i, _ in ref["coef"]]).cpu(),
                     torch.stack([c for _, _, c in ref["coef"]]))
    items["baseline"] = (baseline.cpu(), torch.tensor([ref["baseline"]]))
    _check("loss calls%d acc%d %s" % (calls, acc, str(dtype)[6:]), "loss", dtype, items)
    assert all(float(c[..., 3].abs().max()) == 0.0 for c in coefs)      # no CE gradient in training (attenet2.py:273)
    # image 1 has an empty target at every level, image 2 saturated logits
    assert all(float(t.view(R_, -1)[1::B].max()) == 0.0 for t in targets)


# ---------------------------------------------------------------------------------------------------------------------
# 5. UpAttenLayer gate: isa_gate -> isa_gate_bwd
# ---------------------------------------------------------------------------------------------------------------------
GATE_CASES = [  # C, low-res h, w, acc_up, acc_pred
    (32, 5, 7, 0, 0), (32, 8, 8, 1, 1),          # cgs = 4: power-of-two path (shuffle fold, no atomics)
    (24, 5, 7, 1, 0), (24, 8, 8, 0, 1),          # cgs = 3: per-lane atomics into du
    (40, 5, 7, 0, 1), (40, 4, 6, 1, 0),          # cgs = 5
    (1024, 5, 7, 1, 1), (1024, 4, 4, 0, 0),      # cgs = 128 > 64: the non-power-of-two path
]


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C_,h,w,acc_up,acc_pred", GATE_CASES)
def test_gate_grads(dtype, C_, h, w, acc_up, acc_pred):
    """out = up * softmax(bilinear_x2(pred))[:, 1] (utils.py:1047-1056, reseg_ref.py:309-310) and isa_gate_bwd vs float64
    autograd; `up`, `out` and their gradients are channel slices of wider concat buffers, as in the network.  Measured
    worst on MI355X: fp32 3.2e-7, bf16 4.9e-3 (all three are stored tensors)."""
    Lm, Act, Engine, ParamStore, Pro = _gpu()
    n, H, W = 2, 2 * h, 2 * w
    ld, c0 = C_ + 16, 8
    up = rand(n, C_, H, W, seed=71)
    pred = rand(n, 2, h, w, seed=72, scale=2.0)
    dout = rand(n, C_, H, W, seed=73)
    dev = "cuda"
    st = torch.cuda.current_stream().cuda_stream
    upa = to_act(Act, up, dtype, ld=ld, c0=c0)
    pa = to_act(Act, pred, dtype)
    outa = _nan_act(Act, n, H, W, C_, dtype, ld=ld, c0=c0)
    gmap = torch.full((n * H * W,), NAN, device=dev)
    Lm.check(Lm.lib().isa_gate(upa.d(), pa.d(), outa.d(), Lm.ptr(gmap), st), "isa_gate")
    da = to_act(Act, dout, dtype, ld=ld, c0=c0)
    old_up, old_p = rand(n, C_, H, W, seed=74), rand(n, 2, h, w, seed=75)
    dupa = to_act(Act, old_up, dtype, ld=ld, c0=c0) if acc_up else _nan_act(Act, n, H, W, C_, dtype, ld=ld, c0=c0)
    dpa = to_act(Act, old_p, dtype) if acc_pred else _nan_act(Act, n, h, w, 2, dtype)
    du = torch.zeros(n * H * W, device=dev)
    Lm.check(Lm.lib().isa_gate_bwd(da.d(), upa.d(), Lm.ptr(gmap), dupa.d(), acc_up, Lm.ptr(du), dpa.d(), acc_pred, st),
             "isa_gate_bwd")
    torch.cuda.synchronize()
    u64 = q(up, dtype).double().requires_grad_(True)
    p64 = q(pred, dtype).double().requires_grad_(True)
    g = torch.softmax(F.interpolate(p64, (H, W), mode="bilinear", align_corners=False), 1)[:, 1:2]
    out = u64 * g
    out.backward(q(dout, dtype).double())
    dup = dupa.nchw().cpu() - (q(old_up, dtype) if acc_up else 0.0)
    dpr = dpa.nchw().cpu() - (q(old_p, dtype) if acc_pred else 0.0)
    _check("gate C%d %dx%d acc%d%d %s" % (C_, h, w, acc_up, acc_pred, str(dtype)[6:]), "gate", dtype,
           dict(out=(outa.nchw().cpu(), out.detach()), dup=(dup, u64.grad), dpred=(dpr, p64.grad)))
    # the slices' neighbours in the concat buffers are untouched
    assert float((upa.buf[..., :c0].float() - 7.0).abs().max()) == 0.0
    assert torch.isnan(outa.buf[..., :c0].float()).all() and torch.isnan(outa.buf[..., c0 + C_:].float()).all()


# ---------------------------------------------------------------------------------------------------------------------
# the bounds separate a correct kernel from one that misses a term (CPU, float64 only)
# ---------------------------------------------------------------------------------------------------------------------
def _grads_sp(use_ht):
    x, sem, dy, P = _sp_inputs(3, 24, 24, 24, None)
    P64 = _leaf(P)
    xr = x.double().requires_grad_(True)
    if use_ht is None:
        out = R.spatial_attention(P64, xr, sem.double()[:, None], R.Ctx(bn_train=True))
    else:
        out = _spatial_attention(P64, xr, sem.double()[:, None], R.Ctx(bn_train=True), use_ht=use_ht)
    out.backward(dy.double())
    g = {k[len(SP) + 1:]: v.grad for k, v in P64.items() if getattr(v, "grad", None) is not None}
    g["dx"] = xr.grad
    return g


def _grads_ha(plus_one):
    s, sem, dmerge = _ha_inputs(4, 15, 17, None)         # no empty sem: den = 0 without the +1
    P = _ha_params()
    if plus_one is None:
        P64 = _leaf(P)
        sr = s.double().requires_grad_(True)
        _, merge = R.hard_attention(P64, sr, sem.double()[:, None], torch.ones(4, 1, 15, 17, dtype=torch.float64),
                                    R.Ctx(bn_train=True))
        (merge[:, 0] * dmerge.double()).sum().backward()
        ref = dict(ds=sr.grad, **{k[len(AT) + 1:]: v.grad for k, v in P64.items() if getattr(v, "grad", None) is not None})
        return ref
    r = _ha_reference(s, sem, dmerge, P, torch.float32, plus_one=plus_one)
    return dict(ds=r["ds"], **{k[len(AT) + 1:]: v.grad for k, v in r["P"].items() if getattr(v, "grad", None) is not None})


def _grads_loss(ema_first, detach, oracle):
    B, G, H, W, nobj = 3, 2, 64, 64, 4
    ins, idx_a, idx_t, s_t, merge, preds = _loss_inputs(B, G, H, W, nobj)
    if oracle:
        r = _loss_reference(ins, idx_a, idx_t, s_t, merge, preds, torch.float32, 0.137, G)
    else:
        # the restatement with the as-written flags goes through _atten_loss instead of R.atten_loss
        r = _loss_reference(ins, idx_a, idx_t, s_t, merge, preds, torch.float32, 0.137, G, ema_first=ema_first,
                            detach=detach) if not (ema_first and detach) else \
            _loss_reference_restated(ins, idx_a, idx_t, s_t, merge, preds, G)
    g = {"dpred L%d" % lvl: d for lvl, d in enumerate(r["dpred"])}
    g["dmerge"] = r["dmerge"]
    return g


def _loss_reference_restated(ins, idx_a, idx_t, s_t, merge, preds, G):
    B = merge.shape[0]
    H = W = int(round(math.sqrt(merge.shape[1])))
    m64 = merge.double().requires_grad_(True)
    P = [p.double().requires_grad_(True) for p in preds]
    state = R.HeadState(baseline=0.137)
    total = 0
    for it in range(G):
        planes = [ins[b, int(idx_a[it, b])] != 0 for b in range(B)]
        alpha = _ins_alpha(m64, planes).reshape(B, 1, H, W)
        gold = torch.stack([ins[b, int(idx_t[it, b])] for b in range(B)]).reshape(B, 1, H, W).double()
        targets = [F.max_pool2d(gold, f) if f > 1 else gold for f in FACTORS]
        total = total + _atten_loss([p[it * B:(it + 1) * B] for p in P], targets, alpha, [int(v) for v in s_t[it]], state) / G
    total.backward()
    return dict(dpred=[p.grad for p in P], dmerge=m64.grad)


def _grads_gate(exact):
    """The gate's only smooth term that a kernel could lose is the softmax derivative g (1 - g); 'inexact' drops it
    to g, the form a forgotten chain-rule factor takes."""
    up, pred, dout = rand(2, 24, 10, 14, seed=71), rand(2, 2, 5, 7, seed=72, scale=2.0), rand(2, 24, 10, 14, seed=73)
    p64 = pred.double().requires_grad_(True)
    u = F.interpolate(p64, (10, 14), mode="bilinear", align_corners=False)
    d = u[:, 1:2] - u[:, 0:1]
    g = torch.sigmoid(d) if exact else torch.sigmoid(d).detach() + (d - d.detach()) * torch.sigmoid(d).detach()
    (up.double() * g).backward(dout.double())
    return {"dpred": p64.grad}


def test_head_references_separate_a_missing_term():
    """For layers 1-4: the float64 reference as written vs with one backward-relevant term changed.  The gradient
    distance must be >= 100x the GPU bound of the tensor, so a kernel that loses the term cannot pass its test.  The
    restatements used for the change reproduce the oracle exactly when the term is kept."""
    def dist(a, b, names, layer, floor_of=None):
        out = {}
        for k in names:
            floor = floor_of(k, b) if floor_of else 0.0
            out[k] = max(_err(a[k], b[k], floor)) / BOUNDS[layer][k.split()[0]]
        return out

    def same(a, b):
        for k in b:
            assert max(_err(a[k], b[k])) < 1e-12, k

    ratios = {}
    # 1. spatial attention without h_t
    ref = _grads_sp(None)
    same(_grads_sp(True), ref)
    ratios["sp: drop h_t"] = dist(_grads_sp(False), ref, ("dx", "l_v.weight", "l_v.bias", "spatial_fc.1.weight"), "sp")
    # 2. maskBN without the +1 of its denominator
    ref = _grads_ha(None)
    same(_grads_ha(True), ref)
    fl = lambda k, r: float(r["attend_fc.1.weight"].abs().max()) if k == "attend_fc.1.bias" else 0.0  # noqa: E731
    ratios["ha: drop +1"] = dist(_grads_ha(False), ref, ("bn.weight", "ds", "attend_fc.1.weight", "attend_fc.1.bias"), "ha",
                                 fl)
    # 3 / 4. the loss chain: focal modulating factor not detached; EMA baseline updated after the advantage
    ref = _grads_loss(True, True, True)
    same(_grads_loss(True, True, False), ref)
    ratios["loss: focal not detached"] = dist(_grads_loss(True, False, False), ref, ("dpred L0", "dpred L4"), "loss")
    ratios["ins/loss: EMA after advantage"] = dist(_grads_loss(False, True, False), ref, ("dmerge",), "loss")
    # 5. the gate without its softmax derivative factor
    ratios["gate: drop (1 - g)"] = dist(_grads_gate(False), _grads_gate(True), ("dpred",), "gate")
    for what, r in ratios.items():
        print("  %-32s %s" % (what, "  ".join("%s %.1e" % (k, v) for k, v in r.items())))
    for what, r in ratios.items():     # the first tensor named is the one the changed term feeds most directly
        assert next(iter(r.values())) >= 100.0, (what, r)
