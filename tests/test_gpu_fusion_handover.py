"""The hand-over between a BatchNorm's backward and the convs around it (Engine.conv / dwconv / bn_out), on the paths the
product network never takes:
  * a residual gradient that bn_out defers to the conv reading the residual tensor, when that conv ends up on the separate
    kernels after all (no BatchNorm behind it): depthwise consumer and 1x1 consumer; the deferred gradient must reach dx once;
  * eval mode: eval_bn / bn / bn_out of one layer share one set of constants, filled by one finalize launch and recomputed
    in place after the running statistics changed.
Fused (fuse_dw_bn = fuse_pw_bn = True) against separate kernels at the tolerances of test_gpu_groups.py (same arithmetic,
other summation order), and both against float64 autograd at test_gpu_ops.TOL."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from test_gpu_ops import TOL, _gpu, _run_backward, q, rand, rel, to_act  # noqa: E402

B, H, W = 2, 6, 10


def _bn(c):
    return {"bn.weight": rand(c, seed=20).abs() + 0.5, "bn.bias": rand(c, seed=30) * 0.5,
            "bn.running_mean": rand(c, seed=40) * 0.1, "bn.running_var": rand(c, seed=50).abs() + 0.5}


def _engine(tensors, dtype):
    L, Act, Engine, ParamStore, Pro = _gpu()
    schema = [(k, tuple(v.shape)) for k, v in tensors.items()] + [("bn.num_batches_tracked", ())]
    ps = ParamStore(schema, "cuda")
    ps.load_state_dict(tensors)
    eng = Engine(ps, dtype)
    eng.profile = True
    return L, Act, eng


def _run(first, t, dtype, fuse, x, dy):
    """out = BN(second(first(x))) + x with no BatchNorm between the two convs; `first` is "dw" (then a 1x1) or "pw" (then a
    depthwise).  Returns dx, the parameter gradients and the launch counts."""
    L, Act, eng = _engine(t, dtype)
    eng.fuse_dw_bn = eng.fuse_pw_bn = fuse
    eng.begin(bn_train=True, record=True)
    c = x.shape[1]
    xa = to_act(Act, x, dtype)
    y, z, out = (eng.new_act(B, H, W, c) for _ in range(3))
    if first == "dw":
        eng.dwconv(xa, "first.weight", y)
        _, s = eng.conv(y, "second.weight", z, stats=True)
    else:
        eng.conv(xa, "first.weight", y)
        _, s = eng.dwconv(y, "second.weight", z, stats=True)
    eng.bn_out(z, s, "bn", L.ACT_NONE, out, res=xa)
    _run_backward(eng, out, dy, Act)
    calls = eng.profile_summary()
    grads = {k: eng.params.gview(k).clone().cpu() for k in t if "running" not in k}
    return eng.grads.grad_of(xa).nchw().float().cpu(), grads, calls


def _reference(first, t, dtype, x, dy):
    """float64 autograd of the same three ops on the stored (quantised) inputs."""
    xt = q(x, dtype).double().requires_grad_(True)
    P = {k: (q(v, dtype) if v.dim() == 4 else v).double().requires_grad_(True) for k, v in t.items() if "running" not in k}
    dw = lambda v, w: F.conv2d(v, w, padding=1, groups=v.shape[1])
    y = dw(xt, P["first.weight"]) if first == "dw" else F.conv2d(xt, P["first.weight"])
    z = F.conv2d(y, P["second.weight"]) if first == "dw" else dw(y, P["second.weight"])
    out = F.batch_norm(z, None, None, P["bn.weight"], P["bn.bias"], True, 0.1, 1e-5) + xt
    out.backward(q(dy, dtype).double())
    return xt.grad, {k: v.grad for k, v in P.items()}


def _check(first, c, dtype):
    dwt, pwt = rand(c, 1, 3, 3, seed=4, scale=1 / 3.0), rand(c, c, 1, 1, seed=7, scale=c ** -0.5)
    t = {"first.weight": dwt if first == "dw" else pwt, "second.weight": pwt if first == "dw" else dwt}
    t.update(_bn(c))
    x, dy = rand(B, c, H, W, seed=8) + 0.5, rand(B, c, H, W, seed=9)
    dx_f, g_f, calls_f = _run(first, t, dtype, True, x, dy)
    dx_u, g_u, calls_u = _run(first, t, dtype, False, x, dy)
    dx_r, g_r = _reference(first, t, dtype, x, dy)
    # fused vs separate: the tolerances of test_gpu_groups.py::test_grouped_block_equals_separate_passes
    print("fused vs separate: dx %.3e" % rel(dx_f, dx_u), {k: "%.3e" % rel(g_f[k].view(-1), g_u[k].view(-1)) for k in g_u})
    for tag, dx, g in (("fused", dx_f, g_f), ("separate", dx_u, g_u)):
        print("%s vs float64: dx %.3e" % (tag, rel(dx, dx_r)), {k: "%.3e" % rel(g[k].view(-1), g_r[k].reshape(-1)) for k in g})
    assert rel(dx_f, dx_u) < (1e-5 if dtype == torch.float32 else 1e-2)
    for k in g_u:
        assert rel(g_f[k].view(-1), g_u[k].view(-1)) < (2e-5 if dtype == torch.float32 else 1.5e-2), k
    for tag, dx, g in (("fused", dx_f, g_f), ("separate", dx_u, g_u)):
        assert rel(dx, dx_r) < TOL[dtype], tag + " vs float64: dx"
        for k in g:
            assert rel(g[k].view(-1), g_r[k].reshape(-1)) < TOL[dtype], tag + " vs float64: " + k
    return calls_f


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_deferred_residual_gradient_depthwise_consumer_unfused(dtype):
    """x -> dwconv -> conv1x1 -> bn_out(res = x): bn_out's backward leaves x's residual gradient to the depthwise conv, whose
    backward then finds no BatchNorm to fuse with and adds it itself ahead of the separate wgrad / dgrad kernels."""
    calls = _check("dw", 16, dtype)
    assert calls["isa_dwconv3x3_wgrad"][0] == 1 and calls["isa_dwconv3x3_dgrad"][0] == 1
    assert "isa_dwconv3x3_bn_backward" not in calls


def test_deferred_residual_gradient_pointwise_consumer_unfused():
    """x -> conv1x1 -> dwconv -> bn_out(res = x), bf16 (the fused 1x1 backward exists in bf16 only): the same for a 1x1
    consumer of the residual tensor."""
    calls = _check("pw", 32, torch.bfloat16)
    assert "isa_conv1x1_bn_backward" not in calls
    assert calls["isa_conv_wgrad"][0] == 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_one_eval_constants_path(dtype):
    c = 24
    t = _bn(c)
    L, Act, eng = _engine(t, dtype)
    eng.begin(bn_train=False, record=False)
    x, x2 = rand(B, c, H, W, seed=8), rand(B, c, H, W, seed=9) + 0.5
    consts = eng.eval_bn("bn", c)
    lazy = eng.bn(to_act(Act, x, dtype), None, "bn", L.ACT_RELU6)
    x2a = to_act(Act, x2, dtype)
    out = eng.bn_out(x2a, None, "bn", L.ACT_NONE, eng.new_act(B, H, W, c))
    assert eng.profile_summary()["isa_bn_finalize"][0] == 1
    assert lazy.pro.scale is consts[0] and lazy.pro.shift is consts[1]
    assert all(u is v for u, v in zip(eng.eval_bn_cache["bn"], consts)) and eng.eval_bn("bn", c) is consts
    ref = lambda: F.batch_norm(q(x2, dtype).double(), eng.params.view("bn.running_mean").double().cpu(),
                               eng.params.view("bn.running_var").double().cpu(), t["bn.weight"].double(),
                               t["bn.bias"].double(), False, 0.1, 1e-5)
    assert rel(out.nchw(), ref()) < TOL[dtype]
    # bn_out returns `out`, not its lazy tensor, so identity (`is`) cannot be asserted on it: this stands in for it - bn_out
    # reads these very tensors, with scale = shift = 0 written into them it produces zeros
    keep = [v.clone() for v in consts[:2]]
    consts[0].zero_(); consts[1].zero_()
    out0 = eng.bn_out(x2a, None, "bn", L.ACT_NONE, eng.new_act(B, H, W, c))
    assert float(out0.nchw().abs().max()) == 0.0
    consts[0].copy_(keep[0]); consts[1].copy_(keep[1])
    # new running statistics: recomputed in place by the next begin(), no new buffers, no finalize in bn_out
    ptrs = [v.data_ptr() for v in consts]
    old = out.nchw().clone()
    eng.eval_bn_stale = True
    eng.params.view("bn.running_mean").add_(0.75)
    eng.begin(bn_train=False, record=False)
    assert not eng.eval_bn_stale and [v.data_ptr() for v in eng.eval_bn_cache["bn"]] == ptrs
    out = eng.bn_out(x2a, None, "bn", L.ACT_NONE, eng.new_act(B, H, W, c))
    assert eng.profile_summary()["isa_bn_finalize"][0] == 1         # the refresh; neither bn_out launched one
    assert rel(out.nchw(), ref()) < TOL[dtype] and rel(out.nchw(), old) > 0.1
