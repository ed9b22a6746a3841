"""isa_conv1x1_bn_backward with y == NULL: the kernel recomputes the conv's raw output from pro(x) and W instead of
reading it (conv_fused_bwd.hip, REC).

1. Recompute against stored y, bit for bit.  y comes from the real forward (Engine.conv -> isa_pack_weights +
   isa_conv_gemm: 1x1, plain output, the same prologue) - the other tests of this entry point feed a random y, which the
   recompute variant rightly ignores.  The same inputs then go through the entry point twice, with that y and with NULL.
   dx, the partial slabs and the folded dW must be bit-identical (the cases keep at most two slabs per fold, so the
   fold's atomics have one possible result), dgamma / dbeta of BN(y) equal, and the BN(x) sums (float atomics into 8
   replicas) within SUM_BOUND = 1e-5 of their sums of |terms|, the bound of scripts/ab_fixed_cost.py.  Identity, not a
   tolerance: a y off by one bf16 ulp next to 0 or 6 flips a ReLU6 mask and moves a gradient by a whole g.
   W is full-precision fp32 (the forward reads its bf16 packing, the backward rounds it itself), the prologue is dyadic
   (tests/test_gpu_backbone_walk.py) so that the reference for y is exact in fp32.
   CASES is the full (N, K) x pixels grid with the other axes laid over it so that every pair of values of two
   different axes occurs (checked when the module is imported):
     (N, K): the four tile instantiations and their ragged forms, and the workload's own 64x32 / 32x64;
     pixels per group: 15 (less than a chunk), 33 and 65 (ragged last chunk; 65 leaves wave 3 idle), and 2 x 37 x 70
     with one slab set per group (one workgroup per group, 40 chunks per wave);
     xmode 0 / 1 / 2, BN(y) activation ReLU6 / none, with and without accumulate + addend, G = 1 / 2.
2. The engine passes y = NULL by default (where one side of the conv has at most 32 channels; the 64 -> 64 conv keeps the
   stored tensor) and the stored tensor with ISA_PW_RECOMPUTE=0, and the parameter gradients of the two runs agree
   within the fused-vs-separate bound of tests/test_gpu_fused_dw.py.
3. y == NULL with a run-time activation is refused with ISA_EINVAL before anything is launched: dx, dw and the
   outputs of a pending finalize keep their sentinels (the pattern of tests/test_gpu_checks_first.py).
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

from test_gpu_ops import _gpu, _run_backward, q, rand, rel, to_act  # noqa: E402
from test_gpu_backbone_walk import (BF, BF16_STORE, act_grad64, bn_setup, check, dyadic_pro, pro_f32, rb, stat_sums,  # noqa: E402
                                    workspace, xbn_setup)
from test_gpu_checks_first import CH, H, ISA_EINVAL, N as NB, W as WD, WS_FLOATS, Pending, act_buf, bn_bwd, buf, tensor  # noqa: E402

SUM_BOUND = 1e-5
NK = [(8, 8), (24, 40), (56, 16), (64, 64), (64, 32), (32, 64)]
# (images per group, h, w), k (slab sets in the NaN workspace; None: the 64 MB workspace)
PIX = [((1, 3, 5), None), ((1, 3, 11), None), ((1, 5, 13), None), ((2, 37, 70), "G")]
AXES = (len(NK), len(PIX), 3, 2, 2, 2)                      # (N, K), pixels, xmode, yact, epi, G
CASES = [(i, j, (i + j) % 3, (i // 3 + j) % 2, (i + j // 2) % 2, (i // 2 + j) % 2) for i in range(len(NK)) for j in range(len(PIX))]
for a, b in itertools.combinations(range(len(AXES)), 2):
    assert len({(c[a], c[b]) for c in CASES}) == AXES[a] * AXES[b], "axis values %d x %d not all paired" % (a, b)


def case_id(c):
    (n, k), (shape, _) = NK[c[0]], PIX[c[1]]
    return "%dx%d-%dpx-x%d-%s-epi%d-G%d" % (n, k, shape[0] * shape[1] * shape[2], c[2], ("relu6", "none")[c[3]], c[4], c[5] + 1)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_recompute_equals_stored_y(case):
    L, Act, Engine, ParamStore, Pro = _gpu()
    lib = L.lib()
    (N, K), (shape, k), xmode, yact, epi, G = NK[case[0]], PIX[case[1]], case[2], (L.ACT_RELU6, L.ACT_NONE)[case[3]], case[4], case[5] + 1
    npg, h, w = shape
    n = npg * G
    k = G if k == "G" else k
    W = rand(N, K, seed=61, scale=K ** -0.5)
    g = q(rand(n, N, h, w, seed=62), BF)
    x = q(rand(n, K, h, w, seed=64, scale=2.0), BF)
    xa = Act(to_act(Act, x, BF).buf, 0, K, None, True, G)
    xdesc, xpro, xact, sc, sh = None, None, L.ACT_NONE, None, None
    if xmode:
        xact = L.ACT_RELU6 if xmode == 1 else L.ACT_NONE
        sc, sh = dyadic_pro(K, seed=66, groups=G)
        scg, shg = sc.reshape(-1).cuda(), sh.reshape(-1).cuda()
        xpro = Pro(scg, shg, xact)
        xt = pro_f32(x, sc, sh, xact, L, groups=G)
    else:
        xt = x
    # ---- y from the forward kernel, through the engine's own weight packing
    ps = ParamStore([("w", (N, K, 1, 1))], "cuda")
    ps.load_state_dict(dict(w=W.view(N, K, 1, 1)))
    eng = Engine(ps, BF)
    eng.begin(bn_train=True, record=False)
    ya = eng.new_act(n, h, w, N, groups=G)
    ya.buf.fill_(float("nan"))
    eng.conv(xa.with_pro(xpro) if xpro else xa, "w", ya)
    torch.cuda.synchronize()
    tag = "pwrec " + case_id(case)
    check(tag + " y", ya.nchw(), F.conv2d(rb(xt), rb(W).view(N, K, 1, 1)), BF16_STORE)
    y = ya.nchw().float().cpu()

    old = q(rand(n, K, h, w, seed=67), BF) if epi else None
    add = q(rand(n, K, h, w, seed=68), BF) if epi else None
    adda = Act(to_act(Act, add, BF).buf, 0, K, None, True, G) if epi else None
    ga = Act(to_act(Act, g, BF).buf, 0, N, None, True, G)
    Wg = W.contiguous().cuda()
    tn, tk = (N + 31) // 32, (K + 31) // 32
    set_floats = tn * tk * 1024 + tn * 32
    slabs = min(((npg * h * w + 31) // 32 + 3) // 4 * G, 512, (k * set_floats if k else 16 << 20) // set_floats) // G * G
    assert slabs <= 2                                          # at most two adders per dW address: the fold has one result
    pc = C.byref(xpro._c) if xpro else None

    def launch(with_y):
        ydesc, ygpu, _, _, _ = bn_setup(L, y, g, G, yact, seed=65)
        xd, xgpu = None, None
        if xmode:
            xdesc, xgpu, xmean, xinv = xbn_setup(L, x, scg, shg, G)
            xd = C.byref(xdesc)
        dxa = Act(to_act(Act, old if epi else torch.full((n, K, h, w), float("nan")), BF).buf, 0, K, None, True, G)
        dw = torch.zeros(N, K, device="cuda")
        ws, wsf, _ = workspace(L, k, set_floats)
        L.check(lib.isa_conv1x1_bn_backward(ga.d(), ya.d() if with_y else None, C.byref(ydesc), xa.d(), pc, xd, L.ptr(Wg),
                                            L.ptr(dw), dxa.d(), int(epi), adda.d() if adda else None, L.ptr(ws), wsf, None,
                                            L.stream_ptr()), "isa_conv1x1_bn_backward")
        torch.cuda.synchronize()
        return dict(dx=dxa.buf.clone(), dw=dw, slabs=ws[:slabs * set_floats].clone(), dgamma=ygpu["dgamma"], dbeta=ygpu["dbeta"],
                    xred=xgpu["red"] if xmode else None, xstat=(xmean, xinv) if xmode else None)
    a, b = launch(True), launch(False)
    assert torch.isfinite(a["dx"].float()).all() and torch.isfinite(a["slabs"]).all(), tag + ": stored-y run"
    for what in ("dx", "slabs", "dw", "dgamma", "dbeta"):
        diff = int((bits(a[what]) != bits(b[what])).sum())
        print("PWREC %-44s %-6s differing elements %d of %d" % (case_id(case), what, diff, a[what].numel()))
        assert diff == 0, "%s: %s differs between stored and recomputed y in %d elements" % (tag, what, diff)
    if xmode:
        # sums of |terms| of the two sums, from the stored dx (as xred_ref in test_gpu_backbone_walk.py, with |.|)
        dxs = a["dx"].float().cpu().permute(0, 3, 1, 2)[:, :K].double()
        xmean, xinv = a["xstat"]
        gi = torch.arange(n) // (n // G)
        bc = lambda t: t[gi][:, :, None, None].double()      # noqa: E731
        dz = dxs * act_grad64(x.double() * bc(sc) + bc(sh), xact, L)
        xh = (x.double() - bc(xmean)) * bc(xinv)
        mag = torch.cat([dz.abs().view(G, n // G, K, -1).sum((1, 3)), (dz * xh).abs().view(G, n // G, K, -1).sum((1, 3))], 1)
        sa, sb = stat_sums(a["xred"], K, G), stat_sums(b["xred"], K, G)
        err = float(((sa - sb).abs() / mag.clamp_min(1e-30)).max())
        print("PWREC %-44s xred   %.3e of sum |terms|, bound %.0e" % (case_id(case), err, SUM_BOUND))
        assert float(sa.abs().max()) > 0 and err < SUM_BOUND, "%s: BN(x) sums differ by %.3g of their sum of |terms|" % (tag, err)


# ---------------------------------------------------------------------------------------------------- 2. the engine
class LaunchLog:
    """Stands in for the engine's library handle: forwards every call, notes whether the fused 1x1 backward got a y."""

    def __init__(self, lib):
        self._lib, self.y_null = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "isa_conv1x1_bn_backward":
            return fn

        def call(*args):
            self.y_null.append(args[1] is None)
            return fn(*args)
        return call


def _block(kind, cin, chid, cout, x, dy, t):
    L, Act, Engine, ParamStore, Pro = _gpu()
    schema = [(k, tuple(v.shape)) for k, v in t.items()]
    schema += [(k.replace("running_mean", "num_batches_tracked"), ()) for k in t if k.endswith("running_mean")]
    ps = ParamStore(schema, "cuda")
    ps.load_state_dict(t)
    eng = Engine(ps, BF)
    log = eng.lib = LaunchLog(eng.lib)
    eng.begin(bn_train=True, record=True)
    xa = to_act(Act, x, BF)
    n, _, h, w = x.shape
    cur = xa
    if kind == "ir":
        e = eng.new_act(n, h, w, chid)
        _, s = eng.conv(cur, "pw1.weight", e, stats=True)
        cur = eng.bn(e, s, "bn1", L.ACT_RELU6)
    d = eng.new_act(n, h, w, chid)
    _, s = eng.dwconv(cur, "dw.weight", d, stats=True)
    cur = eng.bn(d, s, "bn2", L.ACT_RELU6)
    y3 = eng.new_act(n, h, w, cout)
    _, s = eng.conv(cur, "pw2.weight", y3, stats=True)
    out = eng.new_act(n, h, w, cout)
    eng.bn_out(y3, s, "bn3", L.ACT_NONE, out, res=xa if cin == cout else None)
    _run_backward(eng, out, dy, Act)
    torch.cuda.synchronize()
    grads = {k: eng.params.gview(k).clone() for k in t if "running" not in k}
    return grads, eng.grads.grad_of(xa).nchw().float().cpu(), log.y_null


@pytest.mark.parametrize("kind,cin,chid,cout", [("ir", 32, 64, 32), ("v1", 64, 64, 32), ("v1", 64, 64, 64)])
def test_engine_passes_null_y(kind, cin, chid, cout, monkeypatch):
    """The head's InvertedResidual (32 -> 64 -> 32) and the backbone's InvertedV1Residual (64 -> 32) at 16 x 16, batch 2.
    The third block's 1x1 conv has more than 32 channels on both sides: the engine keeps the stored y there (the kernel's
    2 x 2 tile gains nothing from the recompute, profiles/ab_pw_recompute.txt), which is checked as well."""
    n, h, w = 2, 16, 16
    t = {}
    if kind == "ir":
        t["pw1.weight"] = rand(chid, cin, 1, 1, seed=1, scale=cin ** -0.5)
        t.update({"bn1.weight": rand(chid, seed=2).abs() + 0.5, "bn1.bias": rand(chid, seed=3) * 0.5 + 1.0,
                  "bn1.running_mean": torch.zeros(chid), "bn1.running_var": torch.ones(chid)})
    t["dw.weight"] = rand(chid, 1, 3, 3, seed=4, scale=1 / 3.0)
    t.update({"bn2.weight": rand(chid, seed=5).abs() + 0.5, "bn2.bias": rand(chid, seed=6) * 0.5 + 1.0,
              "bn2.running_mean": torch.zeros(chid), "bn2.running_var": torch.ones(chid)})
    t["pw2.weight"] = rand(cout, chid, 1, 1, seed=7, scale=chid ** -0.5)
    t.update({"bn3.weight": rand(cout, seed=10).abs() + 0.5, "bn3.bias": rand(cout, seed=11) * 0.5,
              "bn3.running_mean": torch.zeros(cout), "bn3.running_var": torch.ones(cout)})
    x = rand(n, cin, h, w, seed=8) + (0.5 if kind == "v1" else 0.0)
    dy = rand(n, cout, h, w, seed=9)
    monkeypatch.delenv("ISA_PW_RECOMPUTE", raising=False)
    g_r, dx_r, null_r = _block(kind, cin, chid, cout, x, dy, t)
    monkeypatch.setenv("ISA_PW_RECOMPUTE", "0")
    g_s, dx_s, null_s = _block(kind, cin, chid, cout, x, dy, t)
    calls = 2 if kind == "ir" else 1                           # project conv (+ the expand conv of an InvertedResidual)
    assert null_r == [min(chid, cout) <= 32] * calls, null_r
    assert null_s == [False] * calls, null_s
    tol_same = 1.5e-2                                          # test_gpu_fused_dw.py, bf16: fused against separate kernels
    for k in g_s:
        e = rel(g_r[k], g_s[k])
        print("PWREC engine %s %-12s recompute vs stored %.3e" % (kind, k, e))
        assert e < tol_same, "recompute vs stored y: " + k
    assert rel(dx_r, dx_s) < tol_same, "recompute vs stored y: dx"


# ---------------------------------------------------------------------------------------------------- 3. refusal
def _null_y_call(L, lib, pend, dw, dx, yact, keep):
    ws = torch.zeros(WS_FLOATS, device="cuda")
    ybn = bn_bwd(L, keep, yact)
    g, x = act_buf(29, torch.bfloat16), act_buf(31, torch.bfloat16)
    w = buf(CH * CH, 33, offset=-0.5)
    keep += [ws, g, x, w, ybn]
    return lib.isa_conv1x1_bn_backward(tensor(L, g, L.BF16), None, C.pointer(ybn), tensor(L, x, L.BF16), C.pointer(pend.pro), None,
                                       w.data_ptr(), dw.data_ptr(), tensor(L, dx, L.BF16), 0, None, ws.data_ptr(), WS_FLOATS, None,
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("yact", ["ACT_LEAKY", "ACT_RELU", "ACT_TANH"])
def test_null_y_with_runtime_activation_is_refused(yact):
    L, *_ = _gpu()
    lib = L.lib()
    pend = Pending(L, L.ACT_RELU6)
    dw = torch.full((CH * CH,), -777.0, device="cuda")
    dx = torch.full((NB * H * WD * CH,), -555.0, device="cuda")    # sized for fp32, as every buffer of that file
    before = {k: v.clone() for k, v in pend.out.items()}
    dw0, dx0 = dw.clone(), dx.clone()
    keep = []
    rc = _null_y_call(L, lib, pend, dw, dx, getattr(L, yact), keep)
    torch.cuda.synchronize()
    assert rc == ISA_EINVAL, (yact, rc)
    for k, v in pend.out.items():
        assert torch.equal(v, before[k]), (yact, k)
    assert torch.equal(dw, dw0) and torch.equal(dx, dx0), yact
    # the control: the same call with a compile-time activation runs the finalize and writes dx and dw
    rc = _null_y_call(L, lib, pend, dw, dx, L.ACT_RELU6, keep)
    torch.cuda.synchronize()
    assert rc == 0, rc
    for k, v in pend.out.items():
        assert not torch.equal(v, before[k]), ("finalize did not write", k)
    assert not torch.equal(dw, dw0) and not torch.equal(dx, dx0)
