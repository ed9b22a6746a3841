"""isa_conv1x1_bias_bn_backward: the fused 1x1 + BatchNorm backward for a conv WITH a bias (conv_fused_bwd.hip, BIAS).

y comes from the real forward with its bias (Engine.conv -> isa_pack_weights + isa_conv_gemm), W is full-precision fp32
(the forward reads its bf16 packing, the backward rounds it itself), the prologue is dyadic, as in
tests/test_gpu_pw_recompute.py, whose pattern this file follows.  Every case runs the same inputs through

  (a) the old entry point and the new one with bias = dbias = NULL, with the stored y and with y = NULL: dx, the partial
      slabs, the folded dW, dgamma and dbeta bit-identical (the bias-free instantiations are the ones the old entry runs);
  (b) the new entry point with a bias, with the stored y and with y = NULL: the same outputs and dbias bit-identical.  The
      cases keep at most two slabs per fold, so the fold's atomics have one possible result;
  (c) float64 for the biased call: dx (BF16_STORE), dW (FUSED_DW_BF16), dgamma / dbeta and the BN(x) sums (FP32_BOUND),
      the bounds tests/test_gpu_backbone_walk.py applies to isa_conv1x1_bn_backward;
  (d) dbias against the float64 sum of the unrounded dy.  Behind a train-mode BatchNorm that sum cancels to rounding
      level, so the bound is absolute: |dbias - ref| <= 2**-8 * sum |dy| per channel, twice the worst case of rounding
      every term to bf16 (half an ulp, 2**-9 relative), which covers the fp32 evaluation of dy and the summation order.

CASES is the full (N, K) x pixels grid with xmode, the BN(y) activation and accumulate + addend laid over it so that every
pair of values of two different axes occurs (checked at import).  (N, K): the stems' three convs (24 x 32, 48 x 24,
24 x 48: ragged 1 x 1, 2 x 1 and 1 x 2 tiles), 8 x 8 and the full 2 x 2 tile 64 x 64.  Pixels per group: 15 (less than
a chunk), 33 and 65 (ragged last chunk; 65 leaves wave 3 idle), and 2 x 37 x 70 with G = 2 and one slab set per group
(one workgroup per group, 40 chunks per wave).

(e) bias without dbias, or dbias without bias, is ISA_EINVAL before anything is launched: dx, dw, dbias and the outputs of
a pending finalize keep their sentinels (the pattern of tests/test_gpu_checks_first.py).
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

from test_gpu_ops import _gpu, q, rand, to_act  # noqa: E402
from test_gpu_backbone_walk import (BF, BF16_STORE, FP32_BOUND, FUSED_DW_BF16, bn_setup, check, dyadic_pro, pro_f32, rb,  # noqa: E402
                                    stat_sums, workspace, xbn_setup, xred_ref)
from test_gpu_checks_first import CH, H, ISA_EINVAL, N as NB, W as WD, WS_FLOATS, Pending, act_buf, bn_bwd, buf, tensor  # noqa: E402

DBIAS_BOUND = 2.0 ** -8
NK = [(24, 32), (48, 24), (24, 48), (8, 8), (64, 64)]
# (images per group, h, w), G, k (slab sets in the NaN workspace; None: the 64 MB workspace)
PIX = [((1, 3, 5), 1, None), ((1, 3, 11), 1, None), ((1, 5, 13), 1, None), ((2, 37, 70), 2, "G")]
AXES = (len(NK), len(PIX), 3, 2, 2)                          # (N, K), pixels, xmode, yact, epi
CASES = [(i, j, (i + j) % 3, (i + j) % 2, (i + j // 2) % 2) for i in range(len(NK)) for j in range(len(PIX))]
for a, b in itertools.combinations(range(len(AXES)), 2):
    assert len({(c[a], c[b]) for c in CASES}) == AXES[a] * AXES[b], "axis values %d x %d not all paired" % (a, b)


def case_id(c):
    (n, k), (shape, G, _) = NK[c[0]], PIX[c[1]]
    return "%dx%d-%dpx-x%d-%s-epi%d-G%d" % (n, k, shape[0] * shape[1] * shape[2], c[2], ("relu6", "none")[c[3]], c[4], G)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_biased_fused_backward(case):
    L, Act, Engine, ParamStore, Pro = _gpu()
    lib = L.lib()
    (N, K), (shape, G, k), xmode, yact, epi = NK[case[0]], PIX[case[1]], case[2], (L.ACT_RELU6, L.ACT_NONE)[case[3]], case[4]
    npg, h, w = shape
    n = npg * G
    k = G if k == "G" else k
    W = rand(N, K, seed=61, scale=K ** -0.5)
    bvec = rand(N, seed=60)
    g = q(rand(n, N, h, w, seed=62), BF)
    x = q(rand(n, K, h, w, seed=64, scale=2.0), BF)
    xa = Act(to_act(Act, x, BF).buf, 0, K, None, True, G)
    xpro, xact, sc, sh = None, L.ACT_NONE, None, None
    if xmode:
        xact = L.ACT_RELU6 if xmode == 1 else L.ACT_NONE
        sc, sh = dyadic_pro(K, seed=66, groups=G)
        scg, shg = sc.reshape(-1).cuda(), sh.reshape(-1).cuda()
        xpro = Pro(scg, shg, xact)
        xt = pro_f32(x, sc, sh, xact, L, groups=G)
    else:
        xt = x
    # ---- y from the forward kernel with its bias, through the engine's own weight packing
    ps = ParamStore([("w", (N, K, 1, 1)), ("b", (N,))], "cuda")
    ps.load_state_dict(dict(w=W.view(N, K, 1, 1), b=bvec))
    eng = Engine(ps, BF)
    eng.begin(bn_train=True, record=False)
    ya = eng.new_act(n, h, w, N, groups=G)
    ya.buf.fill_(float("nan"))
    eng.conv(xa.with_pro(xpro) if xpro else xa, "w", ya, bias="b")
    torch.cuda.synchronize()
    tag = "pwbias " + case_id(case)
    check(tag + " y", ya.nchw(), F.conv2d(rb(xt), rb(W).view(N, K, 1, 1), bvec.double()), BF16_STORE)
    y = ya.nchw().float().cpu()

    old = q(rand(n, K, h, w, seed=67), BF) if epi else None
    add = q(rand(n, K, h, w, seed=68), BF) if epi else None
    adda = Act(to_act(Act, add, BF).buf, 0, K, None, True, G) if epi else None
    ga = Act(to_act(Act, g, BF).buf, 0, N, None, True, G)
    Wg, bg = W.contiguous().cuda(), bvec.contiguous().cuda()
    tn, tk = (N + 31) // 32, (K + 31) // 32
    set_floats = tn * tk * 1024 + tn * 32
    slabs = min(((npg * h * w + 31) // 32 + 3) // 4 * G, 512, (k * set_floats if k else 16 << 20) // set_floats) // G * G
    assert slabs <= 2                                          # at most two adders per address: the fold has one result
    pc = C.byref(xpro._c) if xpro else None
    ref = {}

    def launch(entry, with_y, with_bias):
        ydesc, ygpu, dyv, r0, r1 = bn_setup(L, y, g, G, yact, seed=65)
        ref.update(dyv=dyv, r0=r0, r1=r1)
        xd, xgpu, xstat = None, None, None
        if xmode:
            xdesc, xgpu, xmean, xinv = xbn_setup(L, x, scg, shg, G)
            xd, xstat = C.byref(xdesc), (xmean, xinv)
        dxa = Act(to_act(Act, old if epi else torch.full((n, K, h, w), float("nan")), BF).buf, 0, K, None, True, G)
        dw = torch.zeros(N, K, device="cuda")
        db = torch.zeros(N, device="cuda")
        ws, wsf, _ = workspace(L, k, set_floats)
        args = (ga.d(), ya.d() if with_y else None, C.byref(ydesc), xa.d(), pc, xd, L.ptr(Wg), L.ptr(dw), dxa.d(), int(epi),
                adda.d() if adda else None, L.ptr(ws), wsf, None, L.stream_ptr())
        if entry == "old":
            rc = lib.isa_conv1x1_bn_backward(*args)
        else:
            rc = lib.isa_conv1x1_bias_bn_backward(*args, L.ptr(bg) if with_bias else None, L.ptr(db) if with_bias else None)
        L.check(rc, "isa_conv1x1_%sbn_backward" % ("" if entry == "old" else "bias_"))
        torch.cuda.synchronize()
        return dict(dx=dxa.buf.clone(), dxa=dxa, dw=dw, db=db, slabs=ws[:slabs * set_floats].clone(), dgamma=ygpu["dgamma"],
                    dbeta=ygpu["dbeta"], xred=xgpu["red"] if xmode else None, xstat=xstat)

    def same(what, a, b, keys):
        for key in keys:
            diff = int((bits(a[key]) != bits(b[key])).sum())
            print("PWBIAS %-40s %-22s %-6s differing elements %d of %d" % (case_id(case), what, key, diff, a[key].numel()))
            assert diff == 0, "%s: %s: %s differs in %d elements" % (tag, what, key, diff)

    # ---- (a) NULL bias / dbias is the old entry point, stored and recomputed y
    for with_y in (True, False):
        o, nw = launch("old", with_y, False), launch("new", with_y, False)
        assert torch.isfinite(o["dx"].float()).all() and torch.isfinite(o["slabs"]).all(), tag + ": old entry"
        same("old vs new/NULL y%d" % with_y, o, nw, ("dx", "slabs", "dw", "dgamma", "dbeta"))
        assert float(nw["db"].abs().max()) == 0.0
    # ---- (b) with the bias: recomputed against stored y
    a, b = launch("new", True, True), launch("new", False, True)
    assert torch.isfinite(a["dx"].float()).all() and torch.isfinite(a["slabs"]).all(), tag + ": biased, stored y"
    same("bias: stored vs NULL y", a, b, ("dx", "slabs", "dw", "db", "dgamma", "dbeta"))
    # ---- (c) float64
    dyv = ref["dyv"]
    dyq = rb(dyv)
    dx = rb(torch.einsum("bnhw,nk->bkhw", dyq, rb(W)))
    if epi:
        dx = rb(dx + old.double())
        dx = rb(dx + add.double())
    check(tag + " dx", a["dxa"].nchw(), dx, BF16_STORE)
    check(tag + " dW", a["dw"], torch.einsum("bnhw,bkhw->nk", dyq, rb(xt.double())), FUSED_DW_BF16)
    check(tag + " dgamma", a["dgamma"], ref["r1"], FP32_BOUND)
    check(tag + " dbeta", a["dbeta"], ref["r0"], FP32_BOUND)
    if xmode:
        xmean, xinv = a["xstat"]
        xr = xred_ref(L, a["dxa"].nchw().double().cpu(), x, sc, sh, xact, xmean, xinv, G)       # over the stored dx
        check(tag + " xred", stat_sums(a["xred"], K, G), xr, FP32_BOUND)
    # ---- (d) the bias gradient
    db_ref, mag = dyv.sum((0, 2, 3)), dyv.abs().sum((0, 2, 3))
    err = ((a["db"].double().cpu() - db_ref).abs() / mag.clamp_min(1e-30))
    print("PWBIAS %-40s dbias  worst %.3e of sum |dy| (bound %.3e); |dbias| max %.3e, sum |dy| max %.3e"
          % (case_id(case), float(err.max()), DBIAS_BOUND, float(db_ref.abs().max()), float(mag.max())))
    assert float(a["db"].abs().max()) > 0, tag + ": dbias not written"
    assert float(err.max()) <= DBIAS_BOUND, "%s: dbias off by %.3g of sum |dy| (channel %d)" % (tag, float(err.max()), int(err.argmax()))


# ---------------------------------------------------------------------------------------------------- (e) refusal
def _call(L, lib, pend, dw, dx, db, keep, with_bias, with_dbias):
    ws = torch.zeros(WS_FLOATS, device="cuda")
    ybn = bn_bwd(L, keep, L.ACT_RELU6)
    g, y, x = act_buf(29, torch.bfloat16), act_buf(30, torch.bfloat16), act_buf(31, torch.bfloat16)
    w, b = buf(CH * CH, 33, offset=-0.5), buf(CH, 34, offset=-0.5)
    keep += [ws, g, y, x, w, b, ybn]
    return lib.isa_conv1x1_bias_bn_backward(tensor(L, g, L.BF16), tensor(L, y, L.BF16), C.pointer(ybn), tensor(L, x, L.BF16),
                                            C.pointer(pend.pro), None, w.data_ptr(), dw.data_ptr(), tensor(L, dx, L.BF16), 0, None,
                                            ws.data_ptr(), WS_FLOATS, None, C.c_void_p(torch.cuda.current_stream().cuda_stream),
                                            b.data_ptr() if with_bias else None, db.data_ptr() if with_dbias else None)


@pytest.mark.parametrize("with_bias,with_dbias", [(True, False), (False, True)])
def test_mismatched_bias_pair_is_refused(with_bias, with_dbias):
    L, *_ = _gpu()
    lib = L.lib()
    pend = Pending(L, L.ACT_RELU6)
    dw = torch.full((CH * CH,), -777.0, device="cuda")
    dx = torch.full((NB * H * WD * CH,), -555.0, device="cuda")    # sized for fp32, as every buffer of that file
    db = torch.full((CH,), -333.0, device="cuda")
    before = {k: v.clone() for k, v in pend.out.items()}
    dw0, dx0, db0 = dw.clone(), dx.clone(), db.clone()
    keep = []
    rc = _call(L, lib, pend, dw, dx, db, keep, with_bias, with_dbias)
    torch.cuda.synchronize()
    assert rc == ISA_EINVAL, (with_bias, with_dbias, rc)
    for k, v in pend.out.items():
        assert torch.equal(v, before[k]), (with_bias, with_dbias, k)
    assert torch.equal(dw, dw0) and torch.equal(dx, dx0) and torch.equal(db, db0)
    # the control: the same call with both runs the finalize and writes dx, dw and dbias
    rc = _call(L, lib, pend, dw, dx, db, keep, True, True)
    torch.cuda.synchronize()
    assert rc == 0, rc
    for k, v in pend.out.items():
        assert not torch.equal(v, before[k]), ("finalize did not write", k)
    assert not torch.equal(dw, dw0) and not torch.equal(dx, dx0) and not torch.equal(db, db0)
