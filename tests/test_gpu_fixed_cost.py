"""The wave-private MFMA backward kernels (pw_bn_bwd_kernel, conv_wgrad_bf16_kernel) at the smallest shapes at which
their prologue and their cross-wave fold can go wrong.

test_gpu_backbone_walk.py runs these kernels where every wave walks many chunks, with channel counts that are
multiples of 32.  What it leaves open is what a launch does before and after its pixel loop:

  * the first chunk's loads leave before the constants are staged, for every lane and at clamped addresses; what lies
    past the last pixel or the last channel is zeroed when the registers are stashed.  Shapes: 1 pixel (one partial
    chunk, three waves idle), 15 and 31 (a partial chunk), 32 (exactly one), 33 (a one-pixel second chunk), 65 (three
    chunks: wave 3 is idle and must park zeros), 129 (two workgroups, the second with one busy wave);
  * the fused kernel stages W zero-padded to its 32-channel tiles: N, K of 8, 16, 24, 40, 56 leave pad rows and columns
    inside a tile, 64 leaves none;
  * the four waves park their partial weight gradients side by side and all threads add them: a stale or uninitialised
    slot shows in dW, in the bias gradient (the slab tail), or, through the NaN-filled workspace, as NaN;
  * the BN(x) sums of the fused kernel go through per-wave, per-row slots of the same pass;
  * 2 x 37 x 70 pixels per group with one slab set per group: one workgroup per group, 40 chunks per wave;
  * the weight gradient's lazy prologue now runs at the stash: none, ReLU6 affine, and ReLU6 affine with a per-image
    multiplier whose image changes inside a chunk (three images of 11 and 43 pixels), plus one 3x3 case (taps outside
    the image are zeroed at the stash, their loads clamped into it) and one transposed-conv case.

dgamma / dbeta are added by exactly one workgroup per statistic group, and the bias gradient comes from the slab
tails: both are checked in every case, so an idle wave or workgroup that adds something shows there.

References, rounding points and bounds are those of test_gpu_backbone_walk.py (imported, see its docstring): float64
from the inputs the kernel sees, bf16 operand rounding emulated, FP32_BOUND for fp32-accumulated results, BF16_STORE for
the stored dx, FUSED_DW_BF16 for dW of the fused kernel.  The shapes here are smaller than that file's: fp32 sums are
shorter, so FP32_BOUND has more room (worst measured on MI355X: dgamma 7.0e-8, dbeta 4.4e-8, xred 2.3e-7, db 4.3e-8,
dW of isa_conv_wgrad 1.2e-7), and dx is deterministic (worst 2.2e-4 of BF16_STORE's 3.9e-3).  dW of the fused
kernel is the one result with LESS room than in the walk file: a dy element whose fp32 and float64 values straddle a
bf16 rounding boundary moves by one ulp (2**-8 of its value), and with 1 to 65 pixels it is one of few terms of its
dW entry instead of one of thousands: worst measured 4.1e-4 against FUSED_DW_BF16 = 8e-4 (inputs and slab order are
fixed, so the figure repeats).

One pixel per statistic group: a BatchNorm over one value has no gradient (g' equals its own mean, y its own mean), so
with constants from bn_setup over that pixel alone dy is rounding noise in the kernel and in float64 alike, and a
relative error says nothing.  The 1-pixel launches therefore take their BN(y) constants and sums from bn_setup over TWO
images per group and run over the first image of each group: the kernel only ever sees constants and a pixel count, the
float64 dy of the kept pixel is the same formula, and dgamma / dbeta are the sums bn_setup passes in.
"""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from test_gpu_ops import _gpu, q, rand, to_act  # noqa: E402
from test_gpu_backbone_walk import (BF, BF16_STORE, FP32_BOUND, FUSED_DW_BF16, bn_setup, check, dyadic_pro, make_pro,  # noqa: E402
                                    pro_f32, rb, run_ws_call, stat_sums, wgrad_set_floats, xbn_setup, xred_ref)

# images per group, h, w[, further images per group that only the BN(y) statistics see]
P1, P15, P32, P65, PBIG = (1, 1, 1, 1), (1, 3, 5), (1, 4, 8), (1, 5, 13), (2, 37, 70)
PW = [
    # N, K, xmode, epi, G, (images per group, h, w), k (slab sets in the NaN workspace; None: the 64 MB workspace)
    (8, 8, 0, False, 1, P1, None), (24, 40, 1, True, 2, P1, None), (56, 16, 1, True, 1, P1, None), (64, 64, 2, False, 2, P1, None),
    (56, 16, 2, False, 1, P15, None), (64, 64, 1, True, 1, P15, None), (8, 8, 2, True, 2, P15, None),
    (24, 40, 0, False, 1, P32, None), (56, 16, 1, False, 2, P32, None), (64, 64, 2, True, 1, P32, None),
    (8, 8, 1, False, 1, P65, None), (24, 40, 2, False, 2, P65, None), (56, 16, 0, True, 1, P65, None),
    (64, 64, 0, False, 2, P65, None), (64, 64, 1, False, 1, P65, None),
    # one slab set per group: one workgroup per group walks 162 chunks, 40-41 per wave
    (8, 8, 0, True, 1, PBIG, 1), (24, 40, 1, False, 2, PBIG, 2), (56, 16, 2, True, 1, PBIG, 1), (64, 64, 1, True, 2, PBIG, 2),
]


@pytest.mark.gpu
@pytest.mark.parametrize("N,K,xmode,epi,G,shape,k", PW,
                         ids=["%dx%d-x%d-epi%d-G%d-%dpx-k%s" % (c[0], c[1], c[2], c[3], c[4], c[5][0] * c[5][1] * c[5][2], c[6])
                              for c in PW])
def test_conv1x1_bn_backward_small(N, K, xmode, epi, G, shape, k):
    L, Act, Engine, ParamStore, Pro = _gpu()
    lib = L.lib()
    npg, h, w = shape[:3]
    extra = shape[3] if len(shape) > 3 else 0
    n = npg * G
    W = q(rand(N, K, seed=61, scale=K ** -0.5), BF)
    g = q(rand((npg + extra) * G, N, h, w, seed=62), BF)
    y = q(rand((npg + extra) * G, N, h, w, seed=63, scale=2.0) + 1.0, BF)
    x = q(rand(n, K, h, w, seed=64, scale=2.0), BF)
    yact = L.ACT_LEAKY if xmode == 2 else L.ACT_RELU6
    ydesc, ygpu, dyv, r0, r1 = bn_setup(L, y, g, G, yact, seed=65)
    kept = [gi * (npg + extra) + i for gi in range(G) for i in range(npg)]     # the images the launch runs over
    g, y, dyv = g[kept].contiguous(), y[kept].contiguous(), dyv[kept]
    dyq = rb(dyv)
    ga, ya_, xa = (Act(to_act(Act, t, BF).buf, 0, t.shape[1], None, True, G) for t in (g, y, x))
    xdesc, xpro, xact, sc, sh = None, None, L.ACT_NONE, None, None
    if xmode:
        xact = L.ACT_RELU6 if xmode == 1 else L.ACT_NONE
        sc, sh = dyadic_pro(K, seed=66, groups=G)
        scg, shg = sc.reshape(-1).cuda(), sh.reshape(-1).cuda()
        xpro = Pro(scg, shg, xact)
        xdesc, xgpu, xmean, xinv = xbn_setup(L, x, scg, shg, G)
        xt = pro_f32(x, sc, sh, xact, L, groups=G).double()
    else:
        xt = x.double()
    xt = rb(xt)                                                # the MFMA operand
    old = q(rand(n, K, h, w, seed=67), BF) if epi else None
    add = q(rand(n, K, h, w, seed=68), BF) if epi else None
    dxa = Act(to_act(Act, old if epi else torch.full((n, K, h, w), float("nan")), BF).buf, 0, K, None, True, G)
    adda = to_act(Act, add, BF) if add is not None else None
    Wg = W.contiguous().cuda()
    dw = torch.zeros(N, K, device="cuda")
    tn, tk = (N + 31) // 32, (K + 31) // 32
    set_floats = tn * tk * 1024 + tn * 32
    pc = C.byref(xpro._c) if xpro else None
    xd = C.byref(xdesc) if xdesc is not None else None

    def call(ws, wsf, sa):
        return lib.isa_conv1x1_bn_backward(ga.d(), ya_.d(), C.byref(ydesc), xa.d(), pc, xd, L.ptr(Wg), L.ptr(dw), dxa.d(),
                                           int(epi), adda.d() if adda else None, ws, wsf, sa, L.stream_ptr())
    run_ws_call(L, call, k, set_floats, "isa_conv1x1_bn_backward")
    # dx: bf16 MFMA of dy and W, rounded to bf16; then + old, rounded; then + addend, rounded (conv_fused_bwd.hip)
    dx = rb(torch.einsum("bnhw,nk->bkhw", dyq, W.double()))
    if epi:
        dx = rb(dx + old.double())
        dx = rb(dx + add.double())
    ref_dw = torch.einsum("bnhw,bkhw->nk", dyq, xt)
    tag = "pwsmall %dx%d x%d epi%d G%d %dpx k=%s" % (N, K, xmode, epi, G, npg * h * w, k)
    check(tag + " dx", dxa.nchw(), dx, BF16_STORE)
    check(tag + " dW", dw, ref_dw, FUSED_DW_BF16)
    check(tag + " dgamma", ygpu["dgamma"], r1, FP32_BOUND)
    check(tag + " dbeta", ygpu["dbeta"], r0, FP32_BOUND)
    if xmode:
        ref = xred_ref(L, dxa.nchw().double().cpu(), x, sc, sh, xact, xmean, xinv, G)      # over the stored dx
        check(tag + " xred", stat_sums(xgpu["red"], K, G), ref, FP32_BOUND)


WG_NK = [(8, 8), (40, 24), (128, 96), (512, 256)]
WG_PIX = {1: (1, 1, 1), 31: (1, 1, 31), 33: (3, 1, 11), 129: (3, 1, 43)}            # M -> n, h, w
WG_PRO = ["none", "relu6", "relu6+bs"]


@pytest.mark.gpu
@pytest.mark.parametrize("form", WG_PRO)
@pytest.mark.parametrize("M", sorted(WG_PIX))
@pytest.mark.parametrize("N,K", WG_NK)
def test_conv_wgrad_small(N, K, M, form):
    """bf16 1x1 weight gradient, default workspace (NaN-filled): gx = (chunks + 3) / 4 workgroups, so M <= 128 is one
    workgroup with 3, 3, 2 idle waves, M = 129 two workgroups of which the second has three idle waves."""
    L, Act, Engine, ParamStore, Pro = _gpu()
    n, h, w = WG_PIX[M]
    x = q(rand(n, K, h, w, seed=71, scale=2.0), BF)
    dy = q(rand(n, N, h, w, seed=72), BF)
    pro, sc, sh, act, bs = make_pro(L, Pro, form, K, n, seed=73)
    xa, da = to_act(Act, x, BF), to_act(Act, dy, BF)
    dw = torch.zeros(N, K, device="cuda")
    db = torch.zeros(N, device="cuda")
    lib = L.lib()
    pc = C.byref(pro._c) if pro else None
    run_ws_call(L, lambda ws, wsf, sa: lib.isa_conv_wgrad(xa.d(), pc, da.d(), L.ptr(dw), L.ptr(db), L.IN_1X1, L.OUT_PLAIN,
                                                         None, K, ws, wsf, sa, L.stream_ptr()),
                None, wgrad_set_floats(N, K, 1), "isa_conv_wgrad")
    xt = rb(x if pro is None else pro_f32(x, sc, sh, act, L, bs))
    tag = "wgsmall %dx%d M%d %s" % (N, K, M, form)
    check(tag + " dW", dw, torch.einsum("bnhw,bkhw->nk", dy.double(), xt), FP32_BOUND)
    check(tag + " db", db, dy.double().sum((0, 2, 3)), FP32_BOUND)


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,h,w,K,N", [("3x3", 2, 5, 7, 40, 24), ("shuffle2", 2, 3, 5, 24, 40)])
def test_conv_wgrad_small_forms(name, n, h, w, K, N):
    """IN_3X3 (9 taps, the border taps' loads clamped into the image and zeroed at the stash) and OUT_SHUFFLE2 (4 taps,
    dy rows gathered per quadrant), ReLU6 prologue, with the bias gradient; 70 / 30 input pixels: 3 chunks / 1 chunk."""
    L, Act, Engine, ParamStore, Pro = _gpu()
    lib = L.lib()
    sh2 = name == "shuffle2"
    x = q(rand(n, K, h, w, seed=81, scale=2.0), BF)
    oh, ow = (2 * h, 2 * w) if sh2 else (h, w)
    dy = q(rand(n, N, oh, ow, seed=82), BF)
    sc, sh = dyadic_pro(K, seed=83)
    pro = Pro(sc.reshape(-1).cuda(), sh.reshape(-1).cuda(), L.ACT_RELU6)
    xt = rb(pro_f32(x, sc, sh, L.ACT_RELU6, L))
    xa, da = to_act(Act, x, BF), to_act(Act, dy, BF)
    taps = 4 if sh2 else 9
    dw = torch.zeros((K, N, 2, 2) if sh2 else (N, K, 3, 3), device="cuda")
    db = torch.zeros(N, device="cuda")
    in_mode, out_mode = (L.IN_1X1, L.OUT_SHUFFLE2) if sh2 else (L.IN_3X3, L.OUT_PLAIN)
    run_ws_call(L, lambda ws, wsf, sa: lib.isa_conv_wgrad(xa.d(), C.byref(pro._c), da.d(), L.ptr(dw), L.ptr(db), in_mode, out_mode,
                                                         None, K, ws, wsf, sa, L.stream_ptr()),
                None, wgrad_set_floats(N, K, taps), "isa_conv_wgrad")
    d64 = dy.double()
    if sh2:
        wv = torch.zeros(K, N, 2, 2, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(xt, wv, stride=2).backward(d64)
    else:
        wv = torch.zeros(N, K, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(xt, wv, padding=1).backward(d64)
    check("wgsmall %s dW" % name, dw.reshape(-1), wv.grad.reshape(-1), FP32_BOUND)
    check("wgsmall %s db" % name, db, d64.sum((0, 2, 3)), FP32_BOUND)
