"""The two instance stems (InstanceHead.stems: five convs with a bias, each ahead of a train-mode BatchNorm) through the
engine, with the biased fused backward kernels (Engine.fuse_bias, the default) and with ISA_FUSE_BIAS=0's separate kernels,
on 2 images of 8 x 12.  bf16 fuses all five convs; fp32 fuses the two depthwise ones (the fused 1x1 backward is bf16 only).

  * dx and the parameter gradients of the two runs agree within the fused-vs-separate bounds of
    tests/test_gpu_fusion_handover.py (1e-2 / 1.5e-2 in bf16, 1e-5 / 2e-5 in fp32: same arithmetic, other summation order);
  * both runs agree with float64 autograd at test_gpu_ops.TOL.  The float64 run has the engine's rounding points in its
    forward pass: the five conv outputs, e1 and the result are stored in the storage type, the input of a 1x1
    conv is rounded to it after the lazy BatchNorm + ReLU6 (the MFMA operand; the depthwise kernels keep fp32 there) -
    all straight-through in the backward pass - and a BatchNorm takes its batch statistics from the conv output before
    the rounding, as the conv's epilogue does.  Without them the bf16 comparison measures ReLU6 masks that flip between a bf16 and a float64
    forward pass, a whole g per flipped element (0.24 of max |dx| for the separate kernels and the fused ones alike);
  * the five conv-bias gradients are sums of dy that cancel to rounding level behind the BatchNorm (float64 gives ~1e-16
    of their terms), so a relative error says nothing about them.  They get the absolute bound of the kernel tests, per
    channel: 2**-8 * sum |dy| in bf16 and 1e-5 * sum |dy| in fp32, with dy from the float64 run - between the two runs and
    of each against float64;
  * with fusion on, the profile holds no isa_dwconv3x3_wgrad / _dgrad launch and, in bf16, no isa_conv_wgrad or
    isa_bn_bwd_apply launch either, and exactly two isa_bn_bwd_reduce launches (the two materialised BatchNorms; every
    other reduce is produced by the fused consumer).
"""
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from test_gpu_ops import TOL, _gpu, _run_backward, q, rand, rel, to_act  # noqa: E402

B, H, W = 2, 8, 12
P1, P2 = "ins_seg_output_1", "ins_seg_output_2"
# (prefix of the conv, kind, cout, cin, prefix of its BatchNorm)
LAYERS = [(P1 + ".0", "dw", 32, 32, P1 + ".1"), (P1 + ".3", "pw", 24, 32, P1 + ".4"), (P2 + ".0", "pw", 48, 24, P2 + ".1"),
          (P2 + ".3", "dw", 48, 48, P2 + ".4"), (P2 + ".6", "pw", 24, 48, P2 + ".7")]
CONV_BIAS = [pre + ".bias" for pre, *_ in LAYERS]


def _tensors():
    t = {}
    for i, (pre, kind, co, ci, bn) in enumerate(LAYERS):
        t[pre + ".weight"] = rand(co, 1, 3, 3, seed=10 * i + 1, scale=1 / 3.0) if kind == "dw" else rand(co, ci, 1, 1, seed=10 * i + 1, scale=ci ** -0.5)
        t[pre + ".bias"] = rand(co, seed=10 * i + 2) * 0.5
        t[bn + ".weight"] = rand(co, seed=10 * i + 3).abs() + 0.5
        t[bn + ".bias"] = rand(co, seed=10 * i + 4) * 0.5 + (1.0 if i != 4 else 0.0)
        t[bn + ".running_mean"] = torch.zeros(co)
        t[bn + ".running_var"] = torch.ones(co)
    return t


def _run(t, dtype, fuse_bias, x, dy):
    L, Act, Engine, ParamStore, Pro = _gpu()
    from isa_amd.instance_head import InstanceHead
    schema = [(k, tuple(v.shape)) for k, v in t.items()]
    schema += [(k.replace("running_mean", "num_batches_tracked"), ()) for k in t if k.endswith("running_mean")]
    ps = ParamStore(schema, "cuda")
    ps.load_state_dict(t)
    eng = Engine(ps, dtype)
    eng.fuse_bias = fuse_bias
    eng.profile = True
    eng.begin(bn_train=True, record=True)
    xa = to_act(Act, x, dtype)
    out = InstanceHead.stems(types.SimpleNamespace(E=eng, net=None), xa)
    _run_backward(eng, out, dy, Act)
    calls = eng.profile_summary()
    grads = {k: eng.params.gview(k).clone().cpu() for k in t if "running" not in k}
    return eng.grads.grad_of(xa).nchw().float().cpu(), grads, calls, out.nchw().float().cpu()


def _reference(t, dtype, x, dy):
    """float64 autograd of the stems on the stored (quantised) inputs, with the engine's storage roundings in the forward
    pass (see the module docstring); also sum |dy| per channel of every conv output."""
    xt = q(x, dtype).double().requires_grad_(True)
    P = {k: (q(v, dtype) if v.dim() == 4 else v).double().requires_grad_(True) for k, v in t.items() if "running" not in k}
    raws = {}

    def stored(v):                                             # rounded to the storage type, straight-through gradient
        return v + (v.detach().to(dtype).double() - v.detach())

    def layer(v, pre, kind, bn, act):
        w, b = P[pre + ".weight"], P[pre + ".bias"]
        r = F.conv2d(v, w, b, padding=1, groups=v.shape[1]) if kind == "dw" else F.conv2d(stored(v), w, b)
        mean, var = r.mean((0, 2, 3), keepdim=True), r.var((0, 2, 3), unbiased=False, keepdim=True)
        rq = stored(r)
        rq.retain_grad()
        raws[pre] = rq
        o = (rq - mean) / torch.sqrt(var + 1e-5) * P[bn + ".weight"][None, :, None, None] + P[bn + ".bias"][None, :, None, None]
        return o.clamp(0, 6) if act else o
    (a, ka, _, _, ba), (b_, kb, _, _, bb), (c, kc, _, _, bc), (d, kd, _, _, bd), (e, ke, _, _, be) = LAYERS
    y = layer(xt, a, ka, ba, True)
    e1 = stored(layer(y, b_, kb, bb, True))
    y = layer(e1, c, kc, bc, True)
    z = layer(y, d, kd, bd, True)
    out = stored(layer(z, e, ke, be, False) + e1)
    out.backward(q(dy, dtype).double())
    mags = {pre + ".bias": r.grad.abs().sum((0, 2, 3)) for pre, r in raws.items()}
    return xt.grad, {k: v.grad for k, v in P.items()}, mags, out.detach()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_stems_fused_bias_backward(dtype):
    bf = dtype == torch.bfloat16
    t = _tensors()
    x, dy = rand(B, 32, H, W, seed=8) + 0.5, rand(B, 24, H, W, seed=9)
    dx_f, g_f, calls_f, out_f = _run(t, dtype, True, x, dy)
    dx_u, g_u, calls_u, out_u = _run(t, dtype, False, x, dy)
    dx_r, g_r, mags, out_r = _reference(t, dtype, x, dy)
    tag = "bf16" if bf else "f32"
    print("FBENG %s launches fused    %s" % (tag, {k: v[0] for k, v in sorted(calls_f.items())}))
    print("FBENG %s launches separate %s" % (tag, {k: v[0] for k, v in sorted(calls_u.items())}))
    print("FBENG %s forward vs float64: fused %.3e separate %.3e" % (tag, rel(out_f, out_r), rel(out_u, out_r)))
    assert rel(out_f, out_r) < TOL[dtype] and rel(out_u, out_r) < TOL[dtype]
    rest = [k for k in g_u if k not in CONV_BIAS]
    print("FBENG %s fused vs separate: dx %.3e" % (tag, rel(dx_f, dx_u)), {k: "%.3e" % rel(g_f[k].view(-1), g_u[k].view(-1)) for k in rest})
    for name, dx, g in (("fused", dx_f, g_f), ("separate", dx_u, g_u)):
        print("FBENG %s %s vs float64: dx %.3e" % (tag, name, rel(dx, dx_r)), {k: "%.3e" % rel(g[k].view(-1), g_r[k].reshape(-1)) for k in rest})
    bound = 2.0 ** -8 if bf else 1e-5
    worst = {}
    for k in CONV_BIAS:
        m = mags[k].clamp_min(1e-30)
        worst[k] = tuple(float(((a.double() - b.double().reshape(-1)).abs() / m).max())
                         for a, b in ((g_f[k], g_u[k]), (g_f[k], g_r[k]), (g_u[k], g_r[k])))
        print("FBENG %s %-28s of sum |dy|: fused-separate %.3e fused-f64 %.3e separate-f64 %.3e (bound %.3e)" % ((tag, k) + worst[k] + (bound,)))
    # ---- launches
    for gone in ("isa_dwconv3x3_wgrad", "isa_dwconv3x3_dgrad") + (("isa_conv_wgrad", "isa_bn_bwd_apply") if bf else ()):
        assert gone not in calls_f, (gone, calls_f[gone])
        assert gone in calls_u, gone
    assert calls_f["isa_dwconv3x3_bias_bn_backward"][0] == 2 and "isa_dwconv3x3_bias_bn_backward" not in calls_u
    if bf:
        assert calls_f["isa_conv1x1_bias_bn_backward"][0] == 3 and "isa_conv1x1_bias_bn_backward" not in calls_u
        assert calls_f["isa_bn_bwd_reduce"][0] == 2, calls_f["isa_bn_bwd_reduce"]
    # ---- fused vs separate
    assert rel(dx_f, dx_u) < (1e-2 if bf else 1e-5)
    for k in rest:
        assert rel(g_f[k].view(-1), g_u[k].view(-1)) < (1.5e-2 if bf else 2e-5), k
    # ---- both vs float64
    for name, dx, g in (("fused", dx_f, g_f), ("separate", dx_u, g_u)):
        assert rel(dx, dx_r) < TOL[dtype], name + " vs float64: dx"
        for k in rest:
            assert rel(g[k].view(-1), g_r[k].reshape(-1)) < TOL[dtype], name + " vs float64: " + k
    # ---- the conv-bias gradients
    for k in CONV_BIAS:
        assert max(worst[k]) <= bound, (k, worst[k])
