"""isa_dwconv3x3_bias_bn_backward: the fused depthwise + BatchNorm backward for a conv WITH a bias (dwconv.hip, BIAS).

The bias gradient is the sum of dy over every pixel: each tile adds its own centre pixels (no halo pixel twice, nothing
from outside the image), slab row 9 carries the sums and the existing fold adds them to dbias.  Nothing else depends on
the bias: y is the stored conv output.

C in {8, 24, 48} (one live channel group; a dead group in the block; a second, half-dead channel block) x bf16 / fp32 x
three geometries of tests/test_gpu_dw_pipeline.py: 1 x 1 px images (smaller than a tile; four per group, as BatchNorm's
backward maps one or two samples per channel to exactly zero and leaves rounding noise), two 7 x 33 images per group
(four ragged edge tiles) and
9 x 70 (six tiles, ragged in x and y), each through a workspace of one slab set per statistic group, so that one
workgroup walks every tile of its group.  xmode 0 / 1 / 2, accumulate (+ addend for a plain
x) and G = 1 / 2 are laid over that grid so that every pair of values of two different axes occurs (checked at import).
At most two slabs are folded per address, so the fold's atomics have one possible result.  Per case:

  * dbias == NULL is the old entry point: dx, slabs, dW, dgamma, dbeta and the BN(x) sums bit-identical;
  * with dbias: dx, slab rows 0-8, dW, dgamma, dbeta and the BN(x) sums bit-identical to the call without it;
  * dx and dW against float64 with the bounds of tests/test_gpu_backbone_walk.py;
  * dbias against the float64 sum of the unrounded dy.  Behind a train-mode BatchNorm the sum cancels to rounding level,
    so the bound is absolute, per channel: 2**-8 * sum |dy| in bf16 (twice the worst case of rounding every term to the
    storage type, which the kernel does in LDS) and SUM_BOUND = 1e-5 * sum |dy| in fp32 (the bound of the existing
    tests for fp32 sums);
  * dbias against isa_dwconv3x3_wgrad's db on the applied dy (float64 BatchNorm backward, rounded to storage), same bound.
"""
import ctypes as C
import itertools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from test_gpu_ops import _gpu, rand, to_act  # noqa: E402
from test_gpu_backbone_walk import (BF, CB, F32, FP32_BOUND, acc_bound, bn_setup, check, dyadic_pro, inp, pro_f32, rs,  # noqa: E402
                                    stat_sums, store_bound, workspace, xbn_setup)

SUM_BOUND = 1e-5
CS = [8, 24, 48]
DTYPES = [BF, F32]
# (images per group, h, w), k (slab sets: "G" = one per statistic group)
SHAPES = [("4x1x1px", (4, 1, 1), "G"), ("2x7x33", (2, 7, 33), "G"), ("9x70", (1, 9, 70), "G")]
AXES = (len(CS), len(DTYPES), len(SHAPES), 3, 2, 2)          # C, dtype, shape, xmode, epi, G
CASES = [(i, d, s, (i + s) % 3, (d + s) % 2, (i + d) % 2) for i in range(len(CS)) for d in range(len(DTYPES)) for s in range(len(SHAPES))]
for a, b in itertools.combinations(range(len(AXES)), 2):
    assert len({(c[a], c[b]) for c in CASES}) == AXES[a] * AXES[b], "axis values %d x %d not all paired" % (a, b)


def case_id(c):
    return "c%d-%s-%s-x%d-epi%d-G%d" % (CS[c[0]], "bf16" if DTYPES[c[1]] == BF else "f32", SHAPES[c[2]][0], c[3], c[4], c[5] + 1)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_biased_fused_dw_backward(case):
    L, Act, Engine, ParamStore, Pro = _gpu()
    lib = L.lib()
    c, dtype, (_, shape, k), xmode, epi, G = CS[case[0]], DTYPES[case[1]], SHAPES[case[2]], case[3], case[4], case[5] + 1
    npg, h, w = shape
    n = npg * G
    k = G if k == "G" else k
    wt = inp(rand(c, 1, 3, 3, seed=51, scale=1 / 3.0), dtype)
    ps = ParamStore([("w", wt.shape)], "cuda")
    ps.load_state_dict(dict(w=wt))
    eng = Engine(ps, dtype)
    eng.begin(bn_train=True, record=False)
    reg = eng.reg_dw("w")
    eng.packer.pack()
    g = inp(rand(n, c, h, w, seed=52), dtype)
    y = inp(rand(n, c, h, w, seed=53, scale=2.0) + 1.0, dtype)
    x = inp(rand(n, c, h, w, seed=54, scale=2.0), dtype)
    yact = L.ACT_NONE if xmode == 2 else L.ACT_RELU6          # NONE runs the runtime-act (ACT_RT) instantiation
    ga, ya_, xa = (Act(to_act(Act, t, dtype).buf, 0, c, None, True, G) for t in (g, y, x))
    xpro, xact, sc, sh = None, L.ACT_NONE, None, None
    if xmode:
        xact = L.ACT_RELU6 if xmode == 1 else L.ACT_LEAKY
        sc, sh = dyadic_pro(c, seed=56, groups=G)
        scg, shg = sc.reshape(-1).cuda(), sh.reshape(-1).cuda()
        xpro = Pro(scg, shg, xact)
        xt = pro_f32(x, sc, sh, xact, L, groups=G).double()
    else:
        xt = x.double()
    old = inp(rand(n, c, h, w, seed=57), dtype) if epi else None
    add = inp(rand(n, c, h, w, seed=58), dtype) if (epi and xmode == 0) else None
    adda = Act(to_act(Act, add, dtype).buf, 0, c, None, True, G) if add is not None else None
    ncb = (c + CB - 1) // CB
    set_floats = 10 * CB * ncb
    tiles = npg * ((h + 7) // 8) * ((w + 31) // 32)
    slabs = min(256 // ncb, tiles * G, (k * set_floats if k else 16 << 20) // set_floats) // G * G
    assert slabs <= 2                                          # at most two adders per address: the fold has one result
    pc = C.byref(xpro._c) if xpro else None
    ref = {}

    def launch(entry, with_db):
        ydesc, ygpu, dyv, r0, r1 = bn_setup(L, y, g, G, yact, seed=55)
        ref.update(dyv=dyv)
        xd, xgpu = None, None
        if xmode:
            xdesc, xgpu, _, _ = xbn_setup(L, x, scg, shg, G)
            xd = C.byref(xdesc)
        dxa = Act(to_act(Act, old if epi else torch.full((n, c, h, w), float("nan")), dtype).buf, 0, c, None, True, G)
        dw = torch.zeros(c, 1, 3, 3, device="cuda")
        db = torch.zeros(c, device="cuda")
        ws, wsf, _ = workspace(L, k, set_floats)
        args = (ga.d(), ya_.d(), C.byref(ydesc), xa.d(), pc, xd, eng.packer.ptr(reg["dgrad"]), L.ptr(dw), c, dxa.d(), int(epi),
                adda.d() if adda else None, L.ptr(ws), wsf, None, L.stream_ptr())
        if entry == "old":
            rc = lib.isa_dwconv3x3_bn_backward(*args)
        else:
            rc = lib.isa_dwconv3x3_bias_bn_backward(*args, L.ptr(db) if with_db else None)
        L.check(rc, "isa_dwconv3x3_%sbn_backward" % ("" if entry == "old" else "bias_"))
        torch.cuda.synchronize()
        sl = ws[:slabs * set_floats].clone().view(slabs * ncb, 10, CB)
        out = dict(dx=dxa.buf.clone(), dxa=dxa, dw=dw, db=db, slabs=sl, taps=sl[:, :9].contiguous(), dgamma=ygpu["dgamma"],
                   dbeta=ygpu["dbeta"])
        if xmode:
            out["xred"] = xgpu["red"]
        return out

    tag = "dwbias " + case_id(case)
    keys = ("dx", "dw", "dgamma", "dbeta") + (("xred",) if xmode else ())

    def same(what, a, b, ks):
        for key in ks:
            diff = int((bits(a[key]) != bits(b[key])).sum())
            print("DWBIAS %-34s %-18s %-6s differing elements %d of %d" % (case_id(case), what, key, diff, a[key].numel()))
            assert diff == 0, "%s: %s: %s differs in %d elements" % (tag, what, key, diff)

    o, nn, nb = launch("old", False), launch("new", False), launch("new", True)
    assert torch.isfinite(o["dx"].float()).all() and torch.isfinite(o["slabs"]).all(), tag + ": old entry"
    same("old vs new/NULL", o, nn, keys + ("slabs",))
    assert float(nn["db"].abs().max()) == 0.0 and float(nn["slabs"][:, 9].abs().max()) == 0.0
    same("new/NULL vs dbias", nn, nb, keys + ("taps",))
    # ---- float64: dx, dW
    dyv = ref["dyv"]
    dyq = rs(dyv, dtype)                                       # dy as the kernel holds it in LDS
    dx = F.conv_transpose2d(dyq, wt.double(), padding=1, groups=c)
    if epi:
        dx = dx + old.double()
    if add is not None:
        dx = dx + add.double()
    wv = torch.zeros(c, 1, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xt, wv, padding=1, groups=c).backward(dyq)
    check(tag + " dx", nb["dxa"].nchw(), dx, store_bound(dtype))
    check(tag + " dW", nb["dw"], wv.grad, acc_bound(dtype, True))
    # ---- dbias
    bound = 2.0 ** -8 if dtype == BF else SUM_BOUND
    db_ref, mag = dyv.sum((0, 2, 3)), dyv.abs().sum((0, 2, 3)).clamp_min(1e-30)
    got = nb["db"].double().cpu()
    err = (got - db_ref).abs() / mag
    # isa_dwconv3x3_wgrad on the applied dy
    dya = Act(to_act(Act, dyq.to(dtype), dtype).buf, 0, c, None, True, G)
    dw2, db2 = torch.zeros(c, 1, 3, 3, device="cuda"), torch.zeros(c, device="cuda")
    ws2 = torch.zeros(16 << 20, device="cuda")
    L.check(lib.isa_dwconv3x3_wgrad(xa.d(), pc, dya.d(), L.ptr(dw2), L.ptr(db2), c, L.ptr(ws2), ws2.numel(), None, L.stream_ptr()),
            "isa_dwconv3x3_wgrad")
    torch.cuda.synchronize()
    err2 = (got - db2.double().cpu()).abs() / mag
    print("DWBIAS %-34s dbias vs float64 %.3e, vs isa_dwconv3x3_wgrad %.3e of sum |dy| (bound %.3e); |dbias| max %.3e, sum |dy| max %.3e"
          % (case_id(case), float(err.max()), float(err2.max()), bound, float(db_ref.abs().max()), float(mag.max())))
    assert float(got.abs().max()) > 0, tag + ": dbias not written"
    assert float(err.max()) <= bound, "%s: dbias off float64 by %.3g of sum |dy| (channel %d)" % (tag, float(err.max()), int(err.argmax()))
    assert float(err2.max()) <= bound, "%s: dbias off isa_dwconv3x3_wgrad by %.3g of sum |dy| (channel %d)" % (tag, float(err2.max()), int(err2.argmax()))
