"""conv_gemm_tiled_kernel (the LDS-tiled small GEMM of the low-resolution 1x1 layers, conv_gemm.hip) at the smallest
shapes at which its K loop can go wrong.

The loop is a steady part of two straight-line steps per trip, which requests a tile in every step (past the end the
last tile again), and a peeled drain of one or two steps; the launch prologue requests the first two tiles before the
scale / shift table (a pending finalize fills the table behind the same requests); the statistics fold reuses the tile
buffers.  Cases:

  * K steps: K = 128 (2 steps: drain only), 192 (3: one trip + one drain step), 256 (4: one trip + two), 320 (5: two trips,
    odd), 2048 (32, the cap), at N = 64 and 300 pixels;
  * rows: 1 pixel (every staged row clamped to row 0), 127, 128, 129, and three images of 49 and of 100 pixels (image
    boundaries inside a 128-row tile, which is where the per-image multiplier changes);
  * columns: N = 64, 80 (column tail at WN = 1), 144 (second column tile mostly dead); for the 128-wide tiles
    M = 8192, N = 1024 at K = 128 and 320 (512 workgroups, the TILED_WIDE_MIN edge), N = 1040 (a dead tail tile) and
    M = 8190;
  * prologue forms at 2 and 5 K steps: none, ReLU6 affine, leaky (the run-time activation), ReLU6 affine with a
    per-image multiplier of 0.5 / 2.0 / 0 that differs per image, a pending finalize (the `conv_tiled` set-up of
    test_gpu_inline_fin.py; test_tiled_gemm_pending_finalize);
  * K = 1024 with a prologue and statistics: M = 8192, N = 128 (the issue's shape: 64 workgroups, so 64-wide tiles) and
    M = 8192, N = 1024 (512 workgroups: the 128-wide kernel at 81 920 B of LDS, two workgroups per CU only because the
    fold's buffer lies inside the tile buffers);
  * epilogue forms at 2 and an odd number of K steps: bias + statistics, no statistics, accumulate = 1 into a
    pre-filled output, the eval epilogue isa_conv_gemm_ep with and without a residual (test_tiled_gemm_eval_epilogue),
    two statistic groups with per-group constants and statistics (test_tiled_gemm_two_groups).
Every case checks that the pad channels of the output rows (ld = N + 8) and GUARD rows past M of the output's
allocation keep their fill value, and that a second call on the same inputs gives bit-identical y.

References and bounds are those of test_gpu_backbone_walk.py (imported; see its docstring): float64 from the inputs the
kernel sees, dyadic prologue constants so that the fp32 prologue is exact, the bf16 operand rounding emulated,
BF16_STORE for the stored y and FP32_BOUND for the statistics.  The pending finalize's constants are not dyadic: its
prologue is one fp32 fma, emulated as the float64 product and sum rounded once to fp32 (the product of a bf16 value and
an fp32 constant is exact in float64); its y must also equal, bit for bit, the y of the same launch with the finalize
run ahead of it (ISA_INLINE_FIN=0), which takes the table-load prologue.
"""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from test_gpu_ops import _gpu, make_engine, q, rand, to_act  # noqa: E402
from test_gpu_backbone_walk import BF, BF16_STORE, FP32_BOUND, check, dyadic_pro, pro_f32, rb, stat_sums  # noqa: E402
from test_gpu_inline_fin import _bn_schema, _bn_tensors, _stats  # noqa: E402

FILL = 3.0
GUARD = 256             # rows past M in the output's allocation: two 128-row tiles' worth


def out_act(Act, n, h, w, N, groups=1):
    """An output of ld = N + 8 whose allocation goes on for GUARD rows past its M rows: (Act, the whole allocation)."""
    ld, M = N + 8, n * h * w
    flat = torch.full(((M + GUARD) * ld,), FILL, dtype=BF, device="cuda")
    return Act(flat[:M * ld].view(n, h, w, ld), 0, N, groups=groups), flat


def run_twice(what, ya, flat, N, launch, prefill=None):
    """Launch twice on a freshly filled allocation: bit-identical y, pad channels and guard rows untouched."""
    got = []
    for _ in range(2):
        flat.fill_(FILL)
        if prefill is not None:
            ya.buf[..., :N] = prefill
        st = launch()
        torch.cuda.synchronize()
        got.append((flat.clone(), st.clone() if st is not None else None))
    assert torch.equal(got[0][0].view(torch.int16), got[1][0].view(torch.int16)), "%s: two calls differ" % what
    assert bool((ya.buf[..., N:].float() == FILL).all()), "%s: pad channels written" % what
    assert bool((flat[ya.buf.numel():].float() == FILL).all()), "%s: rows >= M written" % what
    return got[1][1]


def check_stats(what, st, N, ref, groups=1):
    s = stat_sums(st, N, groups)
    per = ref.shape[0] // groups
    for g in range(groups):
        rg = ref[g * per:(g + 1) * per]
        check("tiled %s sum g%d" % (what, g), s[g][:N], rg.sum((0, 2, 3)), FP32_BOUND)
        check("tiled %s sumsq g%d" % (what, g), s[g][N:], (rg * rg).sum((0, 2, 3)), FP32_BOUND)


P300, P1, P127, P128, P129, I49, I100, P8192, P8190 = ((3, 10, 10), (1, 1, 1), (1, 1, 127), (1, 8, 16), (1, 3, 43), (3, 7, 7),
                                                       (3, 10, 10), (2, 64, 64), (2, 63, 65))
CASES = [
    # (n, h, w), K, N, prologue form, statistics, accumulate
    (P300, 128, 64, "none", True, False), (P300, 192, 64, "relu6", True, False), (P300, 256, 64, "none", False, False),
    (P300, 320, 64, "leaky", True, False), (P300, 2048, 64, "relu6", True, False),
    (P1, 128, 64, "relu6", True, False), (P1, 320, 64, "none", True, False),
    (P127, 192, 80, "none", True, False), (P128, 128, 80, "relu6bs", True, False), (P129, 320, 144, "relu6", False, False),
    (I49, 128, 64, "relu6bs", True, False), (I49, 320, 80, "relu6bs", True, False), (I100, 320, 144, "relu6bs", False, False),
    (I100, 128, 144, "leaky", True, False),
    (P300, 128, 64, "none", False, True), (P300, 320, 80, "relu6", False, True), (I49, 192, 144, "relu6bs", False, True),
    (P8192, 128, 1024, "none", True, False), (P8192, 320, 1024, "relu6", True, False), (P8192, 128, 1040, "leaky", True, False),
    (P8190, 320, 1024, "relu6bs", True, False), (P8190, 128, 1024, "none", False, True),
    (P8192, 1024, 128, "relu6", True, False), (P8192, 1024, 1024, "relu6", True, False),
]


def _id(c):
    (n, h, w), K, N, form, stats, acc = c
    return "%dx%dpx-K%d-N%d-%s%s%s" % (n, h * w, K, N, form, "-stats" if stats else "", "-acc" if acc else "")


def _engine(ParamStore, Engine, wt, b):
    ps = ParamStore([("w", wt.shape), ("b", b.shape)], "cuda")
    ps.load_state_dict(dict(w=wt, b=b))
    eng = Engine(ps, BF)
    eng.begin(bn_train=True, record=False)
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_tiled_gemm(case):
    (n, h, w), K, N, form, stats, acc = case
    L, Act, Engine, ParamStore, Pro = _gpu()
    what = _id(case)
    wt = q(rand(N, K, 1, 1, seed=1, scale=K ** -0.5), BF)
    b = rand(N, seed=2)
    x = q(rand(n, K, h, w, seed=3, scale=2.0), BF)
    eng = _engine(ParamStore, Engine, wt, b)
    xa = to_act(Act, x, BF)
    if form == "none":
        xt = x
    else:
        act = L.ACT_LEAKY if form == "leaky" else L.ACT_RELU6
        sc, sh = dyadic_pro(K, seed=4)
        bs = None
        if form == "relu6bs":                               # differs per image and per channel, zeros included
            bs = torch.tensor([0.5, 2.0, 0.0])[(torch.arange(n)[:, None] + torch.arange(K)[None, :]) % 3]
        xa = xa.with_pro(Pro(sc[0].cuda(), sh[0].cuda(), act, bs.cuda() if bs is not None else None))
        xt = pro_f32(x, sc, sh, act, L, bs)
    ref = F.conv2d(rb(xt), rb(wt), b.double())
    ya, flat = out_act(Act, n, h, w, N)
    y0 = None
    if acc:
        y0 = q(rand(n, N, h, w, seed=6), BF)
        ref = ref + y0.double()

    def launch():
        if acc:
            reg = eng.reg_conv("w", 1, None, False)
            if eng.packer.table is None:
                eng.packer.pack()
            eng.lib.isa_conv_gemm(xa.d(), xa.p_fin(), eng.packer.ptr(reg["fwd"]), reg["kp"], eng.params.ptr("b"), ya.d(),
                                  L.IN_1X1, L.OUT_PLAIN, None, 1, eng.st())
            return None
        return eng.conv(xa, "w", ya, bias="b", stats=stats)[1]

    st = run_twice(what, ya, flat, N, launch, y0.permute(0, 2, 3, 1).to(BF).cuda() if acc else None)
    check("tiled %s y" % what, ya.nchw(), ref, BF16_STORE)
    if stats:
        check_stats(what, st, N, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [128, 320])
def test_tiled_gemm_pending_finalize(K, monkeypatch):
    """The BatchNorm finalize of the lazy input runs inside the launch (2 and 5 K steps)."""
    L, Act, Engine, ParamStore, Pro = _gpu()
    N, B, h, w = 80, 3, 7, 7
    what = "fin-K%d" % K
    x = q(rand(B, K, h, w, seed=3, scale=2.0) + 0.5, BF)
    wt = q(rand(N, K, 1, 1, seed=11, scale=K ** -0.5), BF)
    ys = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("ISA_INLINE_FIN", mode)
        tensors = dict(_bn_tensors(K))
        tensors["w.weight"] = wt
        eng = make_engine(Engine, ParamStore, _bn_schema(K) + [("w.weight", tuple(wt.shape))], tensors, BF)
        eng.profile = True
        xa = to_act(Act, x, BF)
        stx = _stats(x, 1)
        ya, flat = out_act(Act, B, h, w, N)
        lazies = []

        def launch():
            lazy = eng.bn(xa, stx, "bn", L.ACT_RELU6)
            lazies.append(lazy)
            return eng.conv(lazy, "w.weight", ya, stats=True)[1]

        st = run_twice(what + "-inline" + mode, ya, flat, N, launch)
        calls = eng.profile_summary()
        assert ("isa_bn_finalize" in calls) == (mode == "0"), calls
        sc, sh = lazies[-1].bn.scale.double().cpu(), lazies[-1].bn.shift.double().cpu()
        z = (x.double() * sc[None, :, None, None] + sh[None, :, None, None]).float()      # one fp32 fma
        ref = F.conv2d(rb(z.clamp(0, 6)), rb(wt))
        check("tiled %s inline=%s y" % (what, mode), ya.nchw(), ref, BF16_STORE)
        check_stats(what + "-inline" + mode, st, N, ref)
        ys[mode] = ya.buf.clone()
    assert torch.equal(ys["1"].view(torch.int16), ys["0"].view(torch.int16)), "%s: in-kernel finalize changes y" % what


@pytest.mark.gpu
@pytest.mark.parametrize("K", [128, 320])
def test_tiled_gemm_two_groups(K):
    """Two statistic groups: per-group prologue constants, per-group statistics (98 pixels per group: one tile each)."""
    L, Act, Engine, ParamStore, Pro = _gpu()
    G, n, h, w, N = 2, 4, 7, 7, 80
    what = "G2-K%d" % K
    wt = q(rand(N, K, 1, 1, seed=1, scale=K ** -0.5), BF)
    b = rand(N, seed=2)
    x = q(rand(n, K, h, w, seed=3, scale=2.0), BF)
    eng = _engine(ParamStore, Engine, wt, b)
    sc, sh = dyadic_pro(K, seed=4, groups=G)
    assert not torch.equal(sc[0], sc[1]) and not torch.equal(sh[0], sh[1])
    xa = Act(to_act(Act, x, BF).buf, 0, K, groups=G).with_pro(Pro(sc.reshape(-1).cuda(), sh.reshape(-1).cuda(), L.ACT_RELU6, None))
    ref = F.conv2d(rb(pro_f32(x, sc, sh, L.ACT_RELU6, L, None, groups=G)), rb(wt), b.double())
    ya, flat = out_act(Act, n, h, w, N, groups=G)
    st = run_twice(what, ya, flat, N, lambda: eng.conv(xa, "w", ya, bias="b", stats=True)[1])
    check("tiled %s y" % what, ya.nchw(), ref, BF16_STORE)
    check_stats(what, st, N, ref, groups=G)


@pytest.mark.gpu
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("K,form", [(128, "relu6"), (192, "none"), (320, "relu6")])
def test_tiled_gemm_eval_epilogue(K, form, with_res):
    """isa_conv_gemm_ep: y = relu6(scale * (conv + bias) + shift) (+ residual), 2, 3 and 5 K steps."""
    L, Act, Engine, ParamStore, Pro = _gpu()
    (n, h, w), N = I49, 80
    what = "ep-K%d-%s-%s" % (K, form, "res" if with_res else "nores")
    wt = q(rand(N, K, 1, 1, seed=1, scale=K ** -0.5), BF)
    b = rand(N, seed=2)
    x = q(rand(n, K, h, w, seed=3, scale=2.0), BF)
    eng = _engine(ParamStore, Engine, wt, b)
    xa, xt = to_act(Act, x, BF), x
    if form == "relu6":
        sc, sh = dyadic_pro(K, seed=4)
        xa = xa.with_pro(Pro(sc[0].cuda(), sh[0].cuda(), L.ACT_RELU6, None))
        xt = pro_f32(x, sc, sh, L.ACT_RELU6, L)
    es, eh = rand(N, seed=7).abs() + 0.5, rand(N, seed=8) + 1.0
    res = q(rand(n, N, h, w, seed=9), BF)
    ra = to_act(Act, res, BF) if with_res else None
    esd, ehd = es.cuda(), eh.cuda()
    ep = L.IsaConvEp(L.addr(esd), L.addr(ehd), L.ACT_RELU6, C.addressof(ra._c) if ra is not None else None)
    reg = eng.reg_conv("w", 1, None, False)
    if eng.packer.table is None:
        eng.packer.pack()
    ya, flat = out_act(Act, n, h, w, N)

    def launch():
        eng.lib.isa_conv_gemm_ep(xa.d(), xa.p(), eng.packer.ptr(reg["fwd"]), reg["kp"], eng.params.ptr("b"), ya.d(), L.IN_1X1,
                                 C.byref(ep), eng.st())

    run_twice(what, ya, flat, N, launch)
    ref = (F.conv2d(rb(xt), rb(wt), b.double()) * es.double()[None, :, None, None] + eh.double()[None, :, None, None]).clamp(0, 6)
    if with_res:
        ref = ref + res.double()
    check("tiled %s y" % what, ya.nchw(), ref, BF16_STORE)
