"""The pipelined loader and the one-trip launch prologues of the depthwise kernels (dwconv.hip).

dw2_fwd_kernel (bf16, double-buffered) keeps the loads of the next tile in flight while it converts one: a register
ring of ISA_DW_FWD_PF slots (1 as built, 2 for the comparison in DESIGN section 5), primed ahead of the launch prologue,
a straight-line steady loop that runs while a tile remains to be requested, and a drain for the last tiles.  Which of
those a workgroup executes depends only on its tile count, so the walks here give EVERY workgroup exactly 1, 2, 3 and 4
tiles (drain only; one, two and three steady passes ahead of the drain - and, with two slots, drain with a slot primed
from the dummy tile, drain with both, one steady pass then one / two drained), ragged 1-2, idle workgroups
(no tile: the ring primed from the dummy tile, no loop), border and interior tiles alternating in one walk, channel
counts that leave a channel group or a whole part of the block dead (clamped loads), an image boundary between two
consecutive tiles of a workgroup with a per-image scale that differs per image (the one-tile-ahead refetch of the scale
row), every prologue form, and the data-gradient entry point with and without accumulation.  dw_bn_bwd_kernel's
prologue (first tile requested ahead of the constants, optional constants through pointer selects) runs with every
optional pointer null and non-null at 1x1 px, one full tile and three tiles per workgroup.

tile_range has two forms.  The XCD form (workgroups per group % 8 == 0 and tiles >= 64) can leave workgroups without a
tile ("xcd-idle").  The plain stride cannot: launch_fwd2 caps the grid at the tile count, so every workgroup of a
plain-stride walk owns at least one tile; its sparsest walk (one tile per workgroup) is "stride-1".

References are float64 from the exact inputs, bounds are those of test_gpu_backbone_walk.py (BF16_STORE for the stored
bf16 outputs, FP32_BOUND for everything accumulated in fp32, FUSED_DW_BF16 for the fused backward's bf16 dW); see that
file for their derivation.  Prologue constants are dyadic, so the fp32 prologue is exact on bf16-valued inputs.  With a
pending finalize the kernel derives scale / shift itself: the reference uses the arrays the launch wrote, and those are
checked against float64 (FP32_BOUND).
"""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from test_gpu_backbone_walk import (BF, BF16_STORE, FP32_BOUND, FUSED_DW_BF16, STAT_R, CB, act_grad64, bn_setup, check,  # noqa: E402
                                    dyadic_pro, nan_ws, pro_f32, rb, stat_sums)
from test_gpu_ops import _gpu, q, rand, to_act  # noqa: E402

EPS = 1e-5


def _engine(L, Engine, ParamStore, wt, b):
    ps = ParamStore([("w", wt.shape), ("b", b.shape)], "cuda")
    ps.load_state_dict(dict(w=wt, b=b))
    eng = Engine(ps, BF)
    eng.begin(bn_train=True, record=False)
    reg = eng.reg_dw("w")
    eng.packer.pack()
    return eng, reg


def run_fwd(n, h, w, c, form="relu6", bias=True, stats=True, G=1, bscale=False, tag=""):
    """isa_dwconv3x3 (bf16) against float64; returns the stored y (bits) for the determinism check."""
    L, Act, Engine, ParamStore, Pro = _gpu()
    lib = L.lib()
    wt = q(rand(c, 1, 3, 3, seed=31, scale=1 / 3.0), BF)
    b = rand(c, seed=32)
    x = q(rand(n, c, h, w, seed=33, scale=2.0), BF)
    eng, reg = _engine(L, Engine, ParamStore, wt, b)
    xa = Act(to_act(Act, x, BF).buf, 0, c, None, True, G)
    ya = eng.new_act(n, h, w, c, groups=G)
    ya.buf.fill_(float("nan"))
    st = torch.zeros(G * STAT_R * 2 * c, device="cuda") if stats else None
    bs = ((rand(n, c, seed=35) > 0).float() * 1.5 + 0.5) if bscale else None        # 0.5 or 2.0, differs per image
    keep = []
    if form == "none":
        pc, xt = None, x.float()
        if bscale:
            bsg = bs.cuda()
            pro = L.IsaPro(None, None, L.addr(bsg), L.ACT_NONE, None)
            keep.append(bsg)
            pc, xt = C.byref(pro), x.float() * bs[:, :, None, None]
    elif form == "fin":
        # pending finalize of BN(x): the kernel derives scale / shift from the sums, one workgroup writes the arrays
        cnt = float(n // G * h * w)
        xg = x.double().view(G, n // G, c, h, w)
        s1, s2 = xg.sum((1, 3, 4)).float(), (xg * xg).sum((1, 3, 4)).float()
        sums = torch.zeros(G, STAT_R, 2 * c)
        sums[:, 0, :c], sums[:, 0, c:] = s1 * 0.25, s2 * 0.25          # spread over replicas: the kernel adds them up
        sums[:, 3, :c], sums[:, 3, c:] = s1 * 0.75, s2 * 0.75
        gam, bet = (torch.rand(c, generator=torch.Generator().manual_seed(36)) + 0.5), rand(c, seed=37)
        dev = {k: v.contiguous().cuda() for k, v in dict(sums=sums, gam=gam, bet=bet, rm=torch.zeros(c), rv=torch.ones(c)).items()}
        out = {k: torch.full((G * c,), float("nan"), device="cuda") for k in ("sc", "sh", "mu", "is")}
        fin = L.IsaBnFin(L.addr(dev["sums"]), L.addr(dev["gam"]), L.addr(dev["bet"]), L.addr(dev["rm"]), L.addr(dev["rv"]),
                         L.addr(out["sc"]), L.addr(out["sh"]), L.addr(out["mu"]), L.addr(out["is"]), cnt, 0.1, EPS, 1)
        bsg = bs.cuda() if bscale else None
        pro = L.IsaPro(L.addr(out["sc"]), L.addr(out["sh"]), L.addr(bsg), L.ACT_RELU6, C.pointer(fin))
        keep += [dev, out, fin, bsg]
        pc = C.byref(pro)
    else:
        act = {"relu6": L.ACT_RELU6, "rt": L.ACT_LEAKY, "affine": L.ACT_NONE}[form]
        sc, sh = dyadic_pro(c, seed=34, groups=G)
        p = Pro(sc.reshape(-1).cuda(), sh.reshape(-1).cuda(), act, bs.cuda() if bscale else None)
        keep.append(p)
        pc = C.byref(p._c)
        xt = pro_f32(x, sc, sh, act, L, bs, groups=G)

    def call():
        return lib.isa_dwconv3x3(xa.d(), pc, eng.packer.ptr(reg["fwd"]), eng.params.ptr("b") if bias else None, ya.d(),
                                 L.ptr(st), L.stream_ptr())
    L.check(call(), "isa_dwconv3x3")
    torch.cuda.synchronize()
    tag = "dwpipe %s %s" % (tag, form)
    if form == "fin":
        mean = (s1.double() / cnt)
        var = (s2.double() / cnt - mean * mean).clamp(min=0)
        inv = 1.0 / torch.sqrt(var + EPS)
        check(tag + " fin scale", out["sc"].view(G, c), gam.double()[None] * inv, FP32_BOUND)
        check(tag + " fin shift", out["sh"].view(G, c), bet.double()[None] - mean * gam.double()[None] * inv, FP32_BOUND)
        check(tag + " fin mean", out["mu"].view(G, c), mean, FP32_BOUND)
        check(tag + " fin invstd", out["is"].view(G, c), inv, FP32_BOUND)
        xt = pro_f32(x, out["sc"].view(G, c).cpu(), out["sh"].view(G, c).cpu(), L.ACT_RELU6, L, bs, groups=G)
    ref = F.conv2d(xt.double(), wt.double(), b.double() if bias else None, padding=1, groups=c)
    check(tag + " y", ya.nchw(), ref, BF16_STORE)
    if stats:
        s = stat_sums(st, c, G)
        r = ref.view(G, n // G, c, h, w)
        check(tag + " sum", s[:, :c], r.sum((1, 3, 4)), FP32_BOUND)
        check(tag + " sumsq", s[:, c:], (r * r).sum((1, 3, 4)), FP32_BOUND)
    return ya, call


WALKS = [
    # id, n, h, w, c.  launch_fwd2: bf16 grid gx = min(256 / ceil(c / 32), tiles); tile_range takes the XCD form when
    # gx % 8 == 0 and tiles >= 64 (XCD x owns ceil(tiles / 8) consecutive tiles, its gx / 8 workgroups stride in them)
    # c = 256: 8 channel blocks, gx = 32.  32 / 64 / 96 / 128 tiles of 8x32 px: exactly 1 / 2 / 3 / 4 per workgroup
    ("stride-1:tiles32-grid32-1each", 1, 32, 256, 256),
    ("xcd-2:tiles64-grid32-2each", 1, 64, 256, 256),
    ("xcd-3:tiles96-grid32-3each", 1, 96, 256, 256),
    ("xcd-4:tiles128-grid32-4each", 1, 128, 256, 256),
    # 40 tiles, plain stride: workgroups 0-7 walk 2 tiles, 8-31 walk 1
    ("stride-ragged:tiles40-grid32-1or2", 1, 40, 256, 256),
    # 13 x 5 = 65 tiles, XCD form, chunk 9: XCD 7 owns tiles 63-64, two of its four workgroups get none (idle)
    ("xcd-idle:tiles65-grid32-0to3", 1, 40, 416, 256),
    # c = 1024: 32 channel blocks, gx = 8.  27x100 px: 4 x 4 tiles (last row 3 px, last column 4 px), 3 images = 48 tiles,
    # plain stride, 6 per workgroup: border, interior (ty, tx in 1..2), border ... alternate inside every walk
    ("stride-border-interior:tiles48-grid8-6each", 3, 27, 100, 1024),
    # small images: every halo slot outside but one pixel / one ragged tile per image
    ("1x1:tiles3-grid3-1each", 3, 1, 1, 32),
    ("7x33:tiles4-grid4-1each", 2, 7, 33, 32),
    ("9x31:tiles4-grid4-1each", 2, 9, 31, 32),
    # c = 24 in rows of 24: channel group 3 of the block is dead (clamped to the block's first group)
    ("c24-ld24:tiles6-grid6-1each", 1, 9, 70, 24),
    # c = 40: second channel block with one live channel group
    ("c40:tiles6-grid6-1each", 1, 9, 70, 40),
    # c = 1024, gx = 8, 6 images of 16x32 px = 2 tiles each: workgroup k walks tiles k and k + 8 = images k / 2 and
    # k / 2 + 4: an image boundary between its two tiles (workgroups 4-7: one tile)
    ("image-boundary:tiles12-grid8-1or2", 6, 16, 32, 1024),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", WALKS, ids=[c[0] for c in WALKS])
def test_dw_forward_walks(case):
    name, n, h, w, c = case
    run_fwd(n, h, w, c, "relu6", bias=True, stats=True, bscale=True, tag=name)


FORMS = [
    # form, bias, stats, G, per-image scale.  2 x 20x70 px per group, c = 64: 9 tiles per group, one per workgroup
    ("none", False, False, 1, False), ("none", True, True, 1, False), ("none", True, False, 1, True),
    ("relu6", False, True, 1, False), ("relu6", True, False, 1, True),
    ("rt", True, True, 1, False), ("rt", False, False, 1, True), ("affine", True, True, 1, False),
    ("fin", True, True, 1, False), ("fin", False, False, 1, True),
    ("relu6", True, True, 2, False), ("fin", True, True, 2, False), ("rt", False, True, 2, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("form,bias,stats,G,bscale", FORMS)
def test_dw_forward_prologue_forms(form, bias, stats, G, bscale):
    run_fwd(2 * G, 20, 70, 64, form, bias=bias, stats=stats, G=G, bscale=bscale, tag="forms G%d b%d s%d" % (G, bias, stats))


@pytest.mark.gpu
def test_dw_forward_two_calls_bit_equal():
    """Same inputs, two launches: y has no atomics and must repeat bit for bit (a stale LDS buffer or a load still in
    flight at a swap would not)."""
    ya, call = run_fwd(1, 96, 256, 256, "relu6", bias=True, stats=True, bscale=True, tag="repeat")
    first = ya.buf.clone()
    ya.buf.fill_(float("nan"))
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int16), ya.buf.view(torch.int16))


DGRAD = [
    ("xcd-3:tiles96-grid32-3each", 1, 96, 256, 256), ("stride-ragged:tiles40-grid32-1or2", 1, 40, 256, 256),
    ("xcd-idle:tiles65-grid32-0to3", 1, 40, 416, 256), ("9x31:tiles4-grid4-1each", 2, 9, 31, 32),
    ("c40:tiles6-grid6-1each", 1, 9, 70, 40), ("1x1:tiles3-grid3-1each", 3, 1, 1, 32),
]


@pytest.mark.gpu
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("case", DGRAD, ids=[c[0] for c in DGRAD])
def test_dw_dgrad_walks(case, acc):
    name, n, h, w, c = case
    L, Act, Engine, ParamStore, Pro = _gpu()
    wt = q(rand(c, 1, 3, 3, seed=41, scale=1 / 3.0), BF)
    dy = q(rand(n, c, h, w, seed=42), BF)
    old = q(rand(n, c, h, w, seed=43), BF)
    eng, reg = _engine(L, Engine, ParamStore, wt, rand(c, seed=44))
    da = to_act(Act, dy, BF)
    dxa = to_act(Act, old if acc else torch.full((n, c, h, w), float("nan")), BF)
    L.check(L.lib().isa_dwconv3x3_dgrad(da.d(), eng.packer.ptr(reg["dgrad"]), dxa.d(), acc, L.stream_ptr()), "dgrad")
    torch.cuda.synchronize()
    ref = F.conv_transpose2d(dy.double(), wt.double(), padding=1, groups=c)
    if acc:
        ref = ref + old.double()
    check("dwpipe dgrad %s acc%d dx" % (name, acc), dxa.nchw(), ref, BF16_STORE)


# ------------------------------------------------------------------------------------------------ fused backward prologue
BWD_SHAPES = [("1x1px:tiles1-grid1", 1, 1, 1, None), ("full-tile:tiles1-grid1", 1, 8, 32, None),
              ("3-per-wg:tiles3-grid1-3each", 1, 8, 96, 1)]
BWD_FORMS = [
    # xmode, has xsc, has xsh, has xbn (xmu / xis / out_red), epi (old dx; + addend for xmode 0)
    (0, False, False, False, False), (0, False, False, False, True),
    (1, True, True, True, False), (1, False, True, True, True), (1, True, False, True, False), (1, False, False, True, False),
    (2, True, True, True, False), (2, True, True, False, True), (2, False, True, False, False), (2, True, False, False, False),
    (2, False, False, True, True), (2, False, False, False, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("xmode,hsc,hsh,hbn,epi", BWD_FORMS)
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=[s[0] for s in BWD_SHAPES])
def test_dw_bn_backward_prologue(shape, xmode, hsc, hsh, hbn, epi):
    """isa_dwconv3x3_bn_backward, bf16, c = 64 (two channel blocks).  xmode as the entry point derives it: 0 plain x; 1 a
    BN(x) record with a ReLU6 prologue; 2 any other prologue (LEAKY here), with or without the record.  k = 1 caps the grid
    at one workgroup per channel block (3 tiles each)."""
    name, npg, h, w, k = shape
    L, Act, Engine, ParamStore, Pro = _gpu()
    lib = L.lib()
    c, n, G = 64, npg, 1
    wt = q(rand(c, 1, 3, 3, seed=51, scale=1 / 3.0), BF)
    eng, reg = _engine(L, Engine, ParamStore, wt, rand(c, seed=50))
    g = q(rand(n, c, h, w, seed=52), BF)
    y = q(rand(n, c, h, w, seed=53, scale=2.0) + 1.0, BF)
    x = q(rand(n, c, h, w, seed=54, scale=2.0), BF)
    ydesc, ygpu, dyv, r0, r1 = bn_setup(L, y, g, G, L.ACT_RELU6, seed=55)
    dyq = rb(dyv)
    ga, ya_, xa = (to_act(Act, t, BF) for t in (g, y, x))
    xact = {0: L.ACT_NONE, 1: L.ACT_RELU6, 2: L.ACT_LEAKY}[xmode]
    sc, sh = dyadic_pro(c, seed=56)
    if not hsc:
        sc = torch.ones_like(sc)
    if not hsh:
        sh = torch.zeros_like(sh)
    scg, shg = (sc.reshape(-1).cuda() if hsc else None), (sh.reshape(-1).cuda() if hsh else None)
    xpro = L.IsaPro(L.addr(scg), L.addr(shg), None, xact, None) if xmode else None
    xdesc = None
    if hbn:
        xm = x.double().mean((0, 2, 3)).float()
        xi = (1.0 / torch.sqrt(x.double().var((0, 2, 3), unbiased=False) + EPS)).float()
        if n * h * w == 1:
            xi = torch.full((c,), 2.0)
        xgpu = dict(mean=xm.cuda(), invstd=xi.cuda(), red=torch.zeros(STAT_R * 2 * c, device="cuda"))
        xdesc = L.IsaBnBwd(L.addr(scg), L.addr(shg), L.addr(xgpu["mean"]), L.addr(xgpu["invstd"]), None, L.addr(xgpu["red"]),
                           None, None, 1.0, 0)
    xt = pro_f32(x, sc, sh, xact, L).double() if xmode else x.double()
    old = q(rand(n, c, h, w, seed=57), BF) if epi else None
    add = q(rand(n, c, h, w, seed=58), BF) if (epi and xmode == 0) else None
    dxa = to_act(Act, old if epi else torch.full((n, c, h, w), float("nan")), BF)
    adda = to_act(Act, add, BF) if add is not None else None
    dw = torch.zeros(c, 1, 3, 3, device="cuda")
    set_floats = 10 * CB * 2
    ws = nan_ws(k * set_floats if k else 16 << 20)
    L.check(lib.isa_dwconv3x3_bn_backward(ga.d(), ya_.d(), C.byref(ydesc), xa.d(), C.byref(xpro) if xpro else None,
                                          C.byref(xdesc) if xdesc is not None else None, eng.packer.ptr(reg["dgrad"]),
                                          L.ptr(dw), c, dxa.d(), int(epi), adda.d() if adda else None, L.ptr(ws), ws.numel(),
                                          None, L.stream_ptr()), "isa_dwconv3x3_bn_backward")
    torch.cuda.synchronize()
    dx = F.conv_transpose2d(dyq, wt.double(), padding=1, groups=c)
    if epi:
        dx = dx + old.double()
    if add is not None:
        dx = dx + add.double()
    wv = torch.zeros(c, 1, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xt, wv, padding=1, groups=c).backward(dyq)
    tag = "dwpipe bwd %s x%d sc%d sh%d bn%d epi%d" % (name, xmode, hsc, hsh, hbn, epi)
    check(tag + " dx", dxa.nchw(), dx, BF16_STORE)
    check(tag + " dW", dw, wv.grad, FUSED_DW_BF16)
    check(tag + " dgamma", ygpu["dgamma"], r1, FP32_BOUND)
    check(tag + " dbeta", ygpu["dbeta"], r0, FP32_BOUND)
    if hbn:
        gx = dxa.nchw().double().cpu()                               # over the stored (rounded) dx, as the kernel sums it
        z = x.double() * sc[0][None, :, None, None].double() + sh[0][None, :, None, None].double()
        dz = gx * act_grad64(z, xact, L)
        xh = (x.double() - xm[None, :, None, None].double()) * xi[None, :, None, None].double()
        ref = torch.cat([dz.sum((0, 2, 3)), (dz * xh).sum((0, 2, 3))])[None]
        check(tag + " xred", stat_sums(xgpu["red"], c, 1), ref, FP32_BOUND)
