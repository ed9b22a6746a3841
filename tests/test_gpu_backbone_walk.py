"""The backbone's persistent kernels at tile counts where every workgroup walks many tiles or chunks.

The op-level tests in test_gpu_ops.py, test_gpu_fused_dw.py, test_gpu_groups.py and test_gpu_inline_fin.py use shapes
at which each workgroup of a persistent grid gets zero or one tile, so the loop-carried code (double-buffer swaps,
TileIter carries, the XCD walk of tile_range, the register prefetch of the next chunk, partial sums kept across tiles,
workspace-capped grids) was reached only through the full train step.  Here every entry point of that family is
compared with a float64 CPU reference of the same operation at shapes whose walks are long:

  * weight-gradient entry points get a NaN-filled workspace of exactly k slab sets, so the grid is k workgroups
    (k = 1: one workgroup walks everything; 3: not a multiple of 8; 8 and 9: exactly 8 and 9 per statistic group),
    plus the default uncapped workspace and deferred folds through an isa_slab_arena;
  * forward kernels, which have no such lever, get shapes whose tile count exceeds the grid; each parametrize entry
    states tiles, grid and tiles per workgroup, computed from the launch code it names;
  * the bf16 depthwise forward and fused backward also run with an XCD range shorter than its workgroups, so that some
    workgroups get no tile at all (and, in the backward, still owe their slab to the NaN workspace).

References are computed in float64 from the exact inputs the kernel sees.  Inputs are values of the storage dtype:
bf16-valued for bf16 storage, full-precision fp32 for fp32 storage (a bf16 rounding anywhere on an fp32 path would show
at ~1e-3, far above FP32_BOUND).  Prologue constants are dyadic (scale in {0.5, ..., 1.5}, shift a multiple of 1/8),
so on bf16-valued inputs the prologue a kernel evaluates in fp32 is exact and reproduced bit for bit here in float32
(with fp32 inputs it differs from the kernel's fma by at most one fp32 ulp, which no rounding point follows).  The
kernels' rounding points are emulated: the bf16 MFMA operand after the prologue (conv GEMM, bf16 weight gradients, the
fused 1x1 backward), the BN-applied gradient dy rounded to storage in the fused backward kernels, and the stored
outputs.

Error = max |got - ref| / max |ref| over the whole output (one bad tile shows); a failure names the worst element and
its 8x32 tile x 32-channel block.  Bounds, and the worst error measured on MI355X over all cases of this file:
  * FP32_BOUND = 1e-5 for everything accumulated in fp32 - dW, db, the BN statistics rows, the xred partials - in both
    storage dtypes, and for fp32-stored outputs.  Every rounding point is emulated, so only the fp32 summation order is
    left: 10x the worst measured value, 9.6e-7 (fused depthwise backward, fp32 dW).
    Measured worst per entry point (fp32 / bf16 storage): conv GEMM y 3.0e-7 / -, stats 7.5e-8 / 9.7e-8;
    isa_conv_wgrad dW 8.4e-7 / 2.7e-7, db 3.7e-7 / 1.1e-7; isa_dwconv3x3 y 1.7e-7 / -, stats 4.7e-8 / 1.3e-7;
    isa_dwconv3x3_wgrad dW 3.3e-7 / 2.3e-7, db 2.2e-7 / 1.3e-7; isa_dwconv3x3_bn_backward dx 1.9e-7 / -, dW 9.6e-7 / -,
    xred 3.0e-7 / 3.4e-7; isa_conv1x1_bn_backward (bf16 only) xred 2.5e-7.
    xred is checked against the sums over the data gradient the kernel stored (the kernels sum the rounded value they
    store, as the unfused reduce pass would); that stored dx is checked against float64 on its own.
    dgamma / dbeta of the fused backward kernels are no walk result: the bx == 0 workgroup of each statistic group adds
    the BN(y) sums the test passes in (`red`).  Their check (same bound) pins that exactly one workgroup per group adds
    them - none of the other, or idle, workgroups and none of the other channel blocks' ones.
  * BF16_STORE = 2**-8 relative to max|ref| for bf16-stored outputs (y, dx): the ceiling of the storage rounding
    itself, half a bf16 ulp, which is 2**-8 of a value at the bottom of its binade and less elsewhere.  The fp32
    accumulation adds a term ~1e-7 of max|ref|; where it moves a value across a rounding boundary relative to the
    float64 sum the stored value is one ulp off, which 2**-8 covers only away from the bottom of a binade.  So this is a
    bound for these fixed inputs (the outputs compared against it are deterministic: no atomics), not a worst case for
    any input; measured: conv GEMM y 3.1e-3 (80 % of it), isa_dwconv3x3 y 2.5e-3, isa_dwpw_eval y 2.6e-3, fused
    depthwise backward dx 2.8e-3, fused 1x1 backward dx 1.9e-3.  One wrong tile costs 0.1 to 1
    (test_walk_bounds_reject_tile_bugs).
  * FUSED_DW_BF16 = 8e-4 for dW of the two fused BatchNorm backward kernels in bf16.  They evaluate the BatchNorm
    backward dy in fp32, in their own operation order, and round it to bf16 before the weight-gradient products; float64
    cannot reproduce that order bit for bit, and an element whose fp32 and float64 values straddle a bf16 rounding
    boundary moves by one ulp.  This rounding point is the one not emulated exactly: the bound is 10x the measured floor
    it leaves, 7.6e-5 (isa_conv1x1_bn_backward; isa_dwconv3x3_bn_backward 6.4e-5).

The file runs in about 20 s on one MI355X.
"""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from test_gpu_ops import _gpu, q, rand, rel, to_act  # noqa: E402

BF = torch.bfloat16
F32 = torch.float32
STAT_R = 8
CB = 32                 # channel block of the depthwise kernels (dwconv.hip)

FP32_BOUND = 1e-5
BF16_STORE = 2.0 ** -8
FUSED_DW_BF16 = 8e-4


# ------------------------------------------------------------------------------------------------ comparison
def walk_err(got, ref):
    """(max |got - ref| / max |ref|, where): `where` names the worst element and, for NCHW tensors, its tile
    (image, 8-row tile, 32-column tile, 32-channel block)."""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = torch.nan_to_num((got - ref).abs(), nan=float("inf"))
    i = int(d.reshape(-1).argmax())
    e = float(d.reshape(-1)[i] / (ref.abs().max() + 1e-30))
    idx = []
    for s in reversed(ref.shape):
        idx.append(i % s)
        i //= s
    idx = tuple(reversed(idx))
    if ref.dim() == 4:
        b, c, y, x = idx
        where = "image %d, tile (ty %d, tx %d), channel block %d (element c=%d y=%d x=%d: got %g, ref %g)" % (
            b, y // 8, x // 32, c // CB, c, y, x, float(got[idx]), float(ref[idx]))
    else:
        where = "element %s: got %g, ref %g" % (idx, float(got[idx]), float(ref[idx]))
    return e, where


def check(what, got, ref, bound):
    e, where = walk_err(got, ref)
    print("WALKERR %-40s %.3e  bound %.1e" % (what, e, bound))
    assert e < bound, "%s: error %.3g >= %.3g at %s" % (what, e, bound, where)


def acc_bound(dtype, fused=False):
    return FUSED_DW_BF16 if (fused and dtype == BF) else FP32_BOUND


def store_bound(dtype):
    return BF16_STORE if dtype == BF else FP32_BOUND


# ------------------------------------------------------------------------------------------------ inputs and prologues
def dyadic_pro(c, seed, groups=1):
    """Prologue constants whose fp32 evaluation on bf16-valued inputs is exact: scale in {0.5 .. 1.5}, shift k/8."""
    g = torch.Generator().manual_seed(seed)
    sc = torch.tensor([0.5, 0.75, 1.0, 1.25, 1.5])[torch.randint(0, 5, (groups, c), generator=g)]
    sh = torch.randint(-8, 13, (groups, c), generator=g).float() / 8
    return sc, sh


def act_f32(z, act, L):
    if act == L.ACT_RELU6:
        return z.clamp(0, 6)
    if act == L.ACT_LEAKY:
        return torch.where(z > 0, z, z * torch.tensor(0.01, dtype=torch.float32))    # 0.01f * z, as the kernels
    assert act == L.ACT_NONE
    return z


def act_grad64(z, act, L):
    if act == L.ACT_RELU6:
        return ((z > 0) & (z < 6)).double()
    if act == L.ACT_LEAKY:
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, 0.01))
    return torch.ones_like(z)


def pro_f32(xq, sc, sh, act, L, bs=None, groups=1):
    """act(scale * x + shift) * bscale in float32, per statistic group (sc, sh: [G, c]; bs: [n, c])."""
    n = xq.shape[0]
    gi = torch.arange(n) // (n // groups)
    z = xq.float() * sc[gi][:, :, None, None] + sh[gi][:, :, None, None]
    t = act_f32(z, act, L)
    if bs is not None:
        t = t * bs[:, :, None, None]
    return t


def inp(t, dtype):
    """A test input in the storage dtype's value set: bf16-valued for bf16 storage, full fp32 precision for fp32 storage
    (so that a bf16 rounding anywhere on an fp32 path shows)."""
    return q(t, BF) if dtype == BF else t.float()


def rb(t):
    """Round to bf16 (the kernels' operand / storage rounding), as float64."""
    return t.to(BF).double()


def rs(t, dtype):
    return rb(t) if dtype == BF else t.double()


def stat_sums(st, c, groups=1):
    """[G][ISA_STAT_R][2c] statistics buffer -> [G][2c] summed over the replicas."""
    return st.double().cpu().view(groups, STAT_R, 2 * c).sum(1)


def nan_ws(floats):
    return torch.full((int(floats),), float("nan"), dtype=torch.float32, device="cuda")


class Arena:
    """isa_slab_arena over a fresh NaN region (deferred folds)."""
    def __init__(self, L):
        self.lib = L.lib()
        self.buf = nan_ws(17 << 20)
        self.h = C.c_void_p()
        L.check(self.lib.isa_slab_arena_create(L.ptr(self.buf), self.buf.numel(), C.byref(self.h)), "arena create")
        L.check(self.lib.isa_slab_arena_begin(self.h), "arena begin")

    def flush(self, L):
        n, used = C.c_int32(-1), C.c_int64(-1)
        L.check(self.lib.isa_slab_arena_flush(self.h, L.stream_ptr(), C.byref(n), C.byref(used)), "arena flush")
        torch.cuda.synchronize()
        self.lib.isa_slab_arena_destroy(self.h)
        return n.value


def workspace(L, k, set_floats):
    """(ws tensor or None, ws_floats, arena or None) for k slab sets; k = None: the engine's 64 MB workspace;
    k = "arena": deferred folds."""
    if k == "arena":
        return None, 0, Arena(L)
    if k is None:
        return nan_ws(16 << 20), 16 << 20, None
    return nan_ws(k * set_floats), k * set_floats, None


def run_ws_call(L, fn, k, set_floats, what):
    ws, wsf, arena = workspace(L, k, set_floats)
    L.check(fn(L.ptr(ws), wsf, arena.h if arena else None), what)
    if arena is not None:
        assert arena.flush(L) == 1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 1. conv GEMM forward
GEMM_CASES = [
    # name, dtype, n, h, w, K, N, taps, act, bscale, stats
    # conv_gemm.hip launch0: M = 4*250*262 = 262000 -> 2047 128-pixel tiles (the last one 112 rows), N = 256 -> nt = 4,
    # gy = 2, gx = min(2047, 768 / 2) = 384: 5.3 tiles per workgroup; no prologue and cin == kp: the FAST kernel
    ("persist-fast", BF, 4, 250, 262, 128, 256, 1, "none", False, True),
    # M = 131000 -> 1024 tiles (last 56 rows), N = 512 -> gy = 4, gx = 768 / 4 = 192: 5.3 tiles per workgroup,
    # ReLU6 prologue with a Dropout2d multiplier: the general kernel (PRO = 1)
    ("persist-pro", BF, 2, 250, 262, 128, 512, 1, "relu6", True, True),
    # fp32, M = 196608 -> 1536 tiles, N = 256 -> gy = 2, gx = 384: 4 tiles per workgroup, LEAKY prologue (PRO = 2)
    ("persist-f32", F32, 3, 256, 256, 32, 256, 1, "leaky", False, True),
    # launch_tiled<2>: bf16, M = 65536 <= TILED_MAX_M (conv_gemm.hip), K = 128, N = 128: (65536/128) * (128/128) = 512 >= 512
    # workgroups -> WN = 2 (one tile each: this kernel is not persistent)
    ("tiled2", BF, 1, 256, 256, 128, 128, 1, "relu6", False, True),
    # conv3x3_tiled.hip: bf16 3x3, cin = 16 (kp 32), N = 16, no prologue / stats: 8x32 tiles, tiles_x = 9 (262 % 32 = 6),
    # tiles_y = 32 (250 % 8 = 2) -> 2304 tiles, gx = min(2304, 512) = 512: 4.5 tiles per workgroup
    ("conv3x3-tiled", BF, 8, 250, 262, 16, 16, 9, "none", False, False),
    # dense 3x3 on the GEMM kernel with the LEAKY 3x3 instantiation (PRO = 3): M = 2*250*262 = 131000 -> 1024 tiles,
    # N = 64 -> nt = 2, gy = 1, gx = min(1024, 768) = 768: 1.3 tiles per workgroup (the prologue form, not the walk)
    ("gemm3x3-leaky", BF, 2, 250, 262, 32, 64, 9, "leaky", False, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", GEMM_CASES, ids=[c[0] for c in GEMM_CASES])
def test_conv_gemm_walk(case):
    name, dtype, n, h, w, K, N, taps, act_name, bscale, stats = case
    L, Act, Engine, ParamStore, Pro = _gpu()
    act = {"none": L.ACT_NONE, "relu6": L.ACT_RELU6, "leaky": L.ACT_LEAKY}[act_name]
    k = 3 if taps == 9 else 1
    wt = inp(rand(N, K, k, k, seed=1, scale=(taps * K) ** -0.5), dtype)
    b = rand(N, seed=2)
    x = inp(rand(n, K, h, w, seed=3, scale=2.0), dtype)
    ps = ParamStore([("w", wt.shape), ("b", b.shape)], "cuda")
    ps.load_state_dict(dict(w=wt, b=b))
    eng = Engine(ps, dtype)
    eng.begin(bn_train=True, record=False)
    xa = to_act(Act, x, dtype)
    bs = None
    if act_name != "none" or bscale:
        sc, sh = dyadic_pro(K, seed=4)
        if bscale:
            bs = (rand(n, K, seed=5) > 0).float() * 2.0
        xa = xa.with_pro(Pro(sc[0].cuda(), sh[0].cuda(), act, bs.cuda() if bs is not None else None))
        xt = pro_f32(x, sc, sh, act, L, bs)
    else:
        xt = x
    xt = rs(xt, dtype)                       # the MFMA operand is rounded once to the storage type
    ya = eng.new_act(n, h, w, N)
    ya.buf.fill_(float("nan"))
    _, st = eng.conv(xa, "w", ya, taps=taps, bias="b", stats=stats)
    torch.cuda.synchronize()
    ref = F.conv2d(xt, rs(wt, dtype), b.double(), padding=k // 2)
    check("gemm %s y" % name, ya.nchw(), ref, store_bound(dtype))
    if stats:
        s = stat_sums(st, N)[0]
        check("gemm %s sum" % name, s[:N], ref.sum((0, 2, 3)), FP32_BOUND)
        check("gemm %s sumsq" % name, s[N:], (ref * ref).sum((0, 2, 3)), FP32_BOUND)


# ------------------------------------------------------------------------------------------------ 2. conv weight gradient
def wgrad_tiles(N, K):
    """dispatch_wg (conv_wgrad.hip): tiles per wave (tn, tk) and the grid's y extent gy."""
    nt, kt = (N + 31) // 32, (K + 31) // 32
    if nt == 1:
        tn, tk = 1, (4 if kt >= 4 else (2 if kt >= 2 else 1))
    elif kt == 1:
        tk, tn = 1, (4 if nt >= 4 else (2 if nt >= 2 else 1))
    else:
        tn, tk = 2, 2
    gy = ((nt + tn - 1) // tn) * ((kt + tk - 1) // tk)
    return tn, tk, gy


def wgrad_set_floats(N, K, taps):
    tn, tk, gy = wgrad_tiles(N, K)
    return (tn * tk * 1024 + tn * 32) * gy * taps


# (N, K) -> (tn, tk) of dispatch_wg, and the prologue form each shape runs
WG_SHAPES = [(32, 32, "leaky"),       # (1,1): bf16 has its own LEAKY instantiation here
             (32, 64, "relu6+bs"),    # (1,2)
             (32, 128, "none"),       # (1,4): no prologue
             (64, 32, "relu6"),       # (2,1)
             (128, 32, "leaky"),      # (4,1): LEAKY through ACT_RT
             (64, 64, "affine")]      # (2,2): scale/shift, act NONE


def make_pro(L, Pro, form, K, n, seed):
    """(Pro or None, sc, sh, act, bs) for a prologue form."""
    if form == "none":
        return None, None, None, L.ACT_NONE, None
    sc, sh = dyadic_pro(K, seed)
    act = {"leaky": L.ACT_LEAKY, "relu6": L.ACT_RELU6, "relu6+bs": L.ACT_RELU6, "affine": L.ACT_NONE}[form]
    bs = (rand(n, K, seed=seed + 1) > 0).float() * 2.0 if form.endswith("+bs") else None
    return Pro(sc[0].cuda(), sh[0].cuda(), act, bs.cuda() if bs is not None else None), sc, sh, act, bs


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3, 8, 9, None])
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("N,K,form", WG_SHAPES)
def test_conv_wgrad_walk(N, K, form, dtype, k):
    """1x1 weight gradient, grid capped to k workgroups by the workspace.  n = 2, 37x45: M = 3330 pixels = 105 chunks
    of 32 (bf16) / 209 of 16 (fp32); k = 1: one workgroup, 26-27 (bf16) / 52-53 (fp32) chunks per wave; uncapped:
    gx = (chunks + 3) / 4 = 27 / 53, so each wave holds at most one chunk and prefetches nothing."""
    L, Act, Engine, ParamStore, Pro = _gpu()
    n, h, w = 2, 37, 45
    x = inp(rand(n, K, h, w, seed=11, scale=2.0), dtype)
    dy = inp(rand(n, N, h, w, seed=12), dtype)
    pro, sc, sh, act, bs = make_pro(L, Pro, form, K, n, seed=13)
    xa = to_act(Act, x, dtype)
    da = to_act(Act, dy, dtype)
    dw = torch.zeros(N, K, device="cuda")
    db = torch.zeros(N, device="cuda")
    lib = L.lib()
    pc = C.byref(pro._c) if pro else None
    run_ws_call(L, lambda ws, wsf, sa: lib.isa_conv_wgrad(xa.d(), pc, da.d(), L.ptr(dw), L.ptr(db), L.IN_1X1, L.OUT_PLAIN,
                                                         None, K, ws, wsf, sa, L.stream_ptr()),
                k, wgrad_set_floats(N, K, 1), "isa_conv_wgrad")
    xt = x if pro is None else pro_f32(x, sc, sh, act, L, bs)
    xt = rs(xt, dtype)            # bf16 kernel: operand rounded after the prologue; fp32: exact-f32 MFMA
    ref_dw = torch.einsum("bnhw,bkhw->nk", dy.double(), xt)
    tag = "wgrad %dx%d %s %s k=%s" % (N, K, form, "bf16" if dtype == BF else "f32", k)
    check(tag + " dW", dw, ref_dw, FP32_BOUND)
    check(tag + " db", db, dy.double().sum((0, 2, 3)), FP32_BOUND)


WG_FORMS = [
    # name, dtype, n, h, w, K, N, G, k
    # dense 3x3 (taps = 9) on conv_wgrad_kernel with a ReLU6 prologue: 2*37*45 = 3330 pixels, k = 3 workgroups per tap
    ("3x3", F32, 2, 37, 45, 32, 32, 1, 3),
    ("3x3", BF, 2, 37, 45, 32, 32, 1, 3),
    ("3x3", BF, 2, 37, 45, 32, 32, 1, "arena"),
    # conv3x3_wgrad_tiled_kernel (bf16, c <= 32, no prologue): tiles_x = 2, tiles_y = 5 -> 20 tiles; cap = ws / (9*1056):
    # k = 3 -> 6.7 tiles per workgroup; uncapped gx = 20
    ("3x3-tiled", BF, 2, 37, 45, 16, 24, 1, 3),
    ("3x3-tiled", BF, 2, 37, 45, 16, 24, 1, None),
    ("3x3-tiled", BF, 2, 37, 45, 16, 24, 1, "arena"),
    # ISA_OUT_SHUFFLE2 (ConvTranspose2d k=2 s=2): taps = 4, 1332 input pixels, k = 3
    ("shuffle2", F32, 2, 18, 37, 32, 32, 1, 3),
    ("shuffle2", BF, 2, 18, 37, 32, 32, 1, 3),
    # statistic groups: per-group prologue constants, M per group; gx = group_grid(min(want, k), G)
    # G = 2, k = 8: 4 workgroups per group; 2 images of 20x40 = 1600 pixels per group = 50 chunks of 32 (bf16), 12-13 per
    # workgroup / 100 chunks of 16 (fp32), 25 per workgroup.  G = 3, k = 9: 3 per group, 50 / 100 chunks over 3
    ("groups", BF, 4, 20, 40, 64, 32, 2, 8),
    ("groups", F32, 4, 20, 40, 64, 32, 2, 8),
    ("groups", BF, 6, 20, 40, 32, 64, 3, 9),
    ("groups", F32, 6, 20, 40, 32, 64, 3, None),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", WG_FORMS, ids=["%s-%s-G%d-k%s" % (c[0], "bf16" if c[1] == BF else "f32", c[7], c[8])
                                                for c in WG_FORMS])
def test_conv_wgrad_forms(case):
    name, dtype, n, h, w, K, N, G, k = case
    L, Act, Engine, ParamStore, Pro = _gpu()
    lib = L.lib()
    x = inp(rand(n, K, h, w, seed=21, scale=2.0), dtype)
    sh2 = name == "shuffle2"
    oh, ow = (2 * h, 2 * w) if sh2 else (h, w)
    dy = inp(rand(n, N, oh, ow, seed=22), dtype)
    sc = sh = None
    if name == "3x3-tiled":
        pro = None
        xt = x.double()
    else:
        sc, sh = dyadic_pro(K, seed=23, groups=G)
        act = L.ACT_LEAKY if name == "groups" else L.ACT_RELU6
        pro = Pro(sc.reshape(-1).cuda(), sh.reshape(-1).cuda(), act)
        xt = rs(pro_f32(x, sc, sh, act, L, groups=G), dtype)
    xa = to_act(Act, x, dtype)
    if G > 1:
        xa = Act(xa.buf, 0, K, None, True, G)
    da = to_act(Act, dy, dtype)
    taps = 9 if name.startswith("3x3") else (4 if sh2 else 1)
    dwshape = (K, N, 2, 2) if sh2 else ((N, K, 3, 3) if taps == 9 else (N, K))
    dw = torch.zeros(dwshape, device="cuda")
    db = torch.zeros(N, device="cuda")
    in_mode = L.IN_3X3 if taps == 9 else L.IN_1X1
    out_mode = L.OUT_SHUFFLE2 if sh2 else L.OUT_PLAIN
    # slab-set size: the tiled 3x3 kernel uses 9 * (1024 + 32) floats per workgroup, the others dispatch_wg's
    set_floats = 9 * (1024 + 32) if name == "3x3-tiled" else wgrad_set_floats(N, K, taps)
    pc = C.byref(pro._c) if pro else None
    if G > 1:          # fewer slab sets than statistic groups: refused, nothing launched
        ws = nan_ws((G - 1) * set_floats)
        rc = lib.isa_conv_wgrad(xa.d(), pc, da.d(), L.ptr(dw), L.ptr(db), in_mode, out_mode, None, K, L.ptr(ws),
                                ws.numel(), None, L.stream_ptr())
        assert rc == -1, "ws_cap < G must be ISA_EINVAL"
    run_ws_call(L, lambda ws, wsf, sa: lib.isa_conv_wgrad(xa.d(), pc, da.d(), L.ptr(dw), L.ptr(db), in_mode, out_mode,
                                                         None, K, ws, wsf, sa, L.stream_ptr()),
                k, set_floats, "isa_conv_wgrad")
    d64 = dy.double()
    if sh2:
        wv = torch.zeros(K, N, 2, 2, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(xt, wv, stride=2).backward(d64)
    elif taps == 9:
        wv = torch.zeros(N, K, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(xt, wv, padding=1).backward(d64)
    else:
        wv = torch.zeros(N, K, 1, 1, dtype=torch.float64, requires_grad=True)
        F.conv2d(xt, wv).backward(d64)
    tag = "wgrad %s %s G%d k=%s" % (name, "bf16" if dtype == BF else "f32", G, k)
    check(tag + " dW", dw.reshape(-1), wv.grad.reshape(-1), FP32_BOUND)
    check(tag + " db", db, d64.sum((0, 2, 3)), FP32_BOUND)


# ------------------------------------------------------------------------------------------------ 3. depthwise forward
DW_FWD = [
    # name, dtype, n, h, w, c, G
    # launch_fwd2 (dwconv.hip): bf16 gx = 256 / ncb, fp32 gx = 768 / ncb, then group_grid.  Only the bf16
    # (double-buffered, DB) instantiation walks tile_range's XCD order, when (workgroups per group) % 8 == 0 and tiles
    # per group >= 64: XCD x = bx % 8 owns tiles [x * chunk, min(ntiles, (x + 1) * chunk)), chunk = ceil(ntiles / 8),
    # and its nbx / 8 workgroups stride through that range.  The fp32 form always strides over all tiles from bx.
    # bf16 c = 1024: ncb = 32, gx = 8 (one workgroup per XCD); 64x128 -> 4 x 8 tiles per image, 64 tiles: XCD walk,
    # chunk 8, 8 tiles per workgroup
    ("xcd", BF, 2, 64, 128, 1024, 1),
    # bf16 c = 1024, 52x70: tiles_x = 3 (70 % 32 = 6), tiles_y = 7 (52 % 8 = 4), 5 images -> 105 tiles (% 8 = 1): XCD
    # walk, chunk 14; seven workgroups walk 14 tiles, the last XCD's one walks 7
    ("xcd-ragged", BF, 5, 52, 70, 1024, 1),
    # bf16 c = 256: ncb = 8, gx = 32, four workgroups per XCD; one 40x416 image -> 13 x 5 = 65 tiles: XCD walk, chunk 9;
    # XCDs 0-6 own 9 tiles each (3, 2, 2, 2 per workgroup), XCD 7 owns tiles 63-64 only: its workgroups j = 2, 3 start
    # at tile 65 and 66 and are IDLE (2 idle workgroups per channel block, 16 in the grid): the zero-tile path
    ("xcd-idle", BF, 1, 40, 416, 256, 1),
    # bf16 c = 96: ncb = 3, gx = 85 (not % 8): plain stride; 100x200 -> 7 x 13 tiles, 4 images = 364 tiles, 4.3 per wg
    ("stride", BF, 4, 100, 200, 96, 1),
    # fp32 c = 1024: ncb = 32, gx = 24; 4 x 64x128 = 128 tiles, plain stride (fp32 has no XCD walk): 5.3 per workgroup
    ("stride", F32, 4, 64, 128, 1024, 1),
    # fp32 c = 800: ncb = 25, gx = 30 (not % 8); 66x130 -> 5 x 9 tiles, 3 images = 135 tiles, 4.5 per workgroup
    ("stride-ragged", F32, 3, 66, 130, 800, 1),
    # statistic groups, bf16 c = 256: ncb = 8, gx = 32.  G = 2: 16 workgroups per group (% 8 = 0), 64 tiles per group:
    # XCD walk on inside each group, 4 tiles per workgroup.  G = 3: group_grid(32, 3) = 30, 10 per group: no XCD walk,
    # 6.4 tiles per workgroup
    ("groups-xcd", BF, 4, 64, 128, 256, 2),
    ("groups", BF, 6, 64, 128, 256, 3),
    # fp32 c = 64: ncb = 2, 2 images of 40x70 per group = 30 tiles; gx = min(384, 90) = 90, 30 per group: one tile each
    ("groups", F32, 6, 40, 70, 64, 3),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", DW_FWD, ids=["%s-%s-G%d" % (c[0], "bf16" if c[1] == BF else "f32", c[6]) for c in DW_FWD])
def test_dwconv_fwd_walk(case):
    name, dtype, n, h, w, c, G = case
    L, Act, Engine, ParamStore, Pro = _gpu()
    wt = inp(rand(c, 1, 3, 3, seed=31, scale=1 / 3.0), dtype)
    b = rand(c, seed=32)
    x = inp(rand(n, c, h, w, seed=33, scale=2.0), dtype)
    sc, sh = dyadic_pro(c, seed=34, groups=G)
    ps = ParamStore([("w", wt.shape), ("b", b.shape)], "cuda")
    ps.load_state_dict(dict(w=wt, b=b))
    eng = Engine(ps, dtype)
    eng.begin(bn_train=True, record=False)
    xa = to_act(Act, x, dtype)
    xa = Act(xa.buf, 0, c, Pro(sc.reshape(-1).cuda(), sh.reshape(-1).cuda(), L.ACT_RELU6), True, G)
    ya = eng.new_act(n, h, w, c, groups=G)
    ya.buf.fill_(float("nan"))
    _, st = eng.dwconv(xa, "w", ya, bias="b", stats=True)
    torch.cuda.synchronize()
    xt = pro_f32(x, sc, sh, L.ACT_RELU6, L, groups=G).double()      # staged as fp32 after the prologue
    ref = F.conv2d(xt, wt.double(), b.double(), padding=1, groups=c)
    tag = "dwfwd %s %s G%d" % (name, "bf16" if dtype == BF else "f32", G)
    check(tag + " y", ya.nchw(), ref, store_bound(dtype))
    s = stat_sums(st, c, G)
    r = ref.view(G, n // G, c, h, w)
    check(tag + " sum", s[:, :c], r.sum((1, 3, 4)), FP32_BOUND)
    check(tag + " sumsq", s[:, c:], (r * r).sum((1, 3, 4)), FP32_BOUND)


# ------------------------------------------------------------------------------------------------ 4. depthwise weight gradient
DW_WG = [
    # dtype, G, k, act.  dw2_wgrad_kernel wants min(512 / ncb, tiles * G) workgroups and slab_grid (slab_plan.hpp) caps them
    # at ws_floats / (10 * 32 * ncb), rounded to a multiple of G.  c = 64
    # (ncb = 2), 3 images of 45x100 per group -> 4 x 6 x 3 = 72 tiles per group.  k = 1: one workgroup, 72 tiles;
    # k = 3: 24; k = 8: 9; k = 9: 8; uncapped: 72 * G workgroups of one tile
    (BF, 1, 1, "relu6"), (BF, 1, 3, "leaky"), (BF, 1, 8, "none"), (BF, 1, 9, "relu6"), (BF, 1, None, "relu6"),
    (F32, 1, 1, "relu6"), (F32, 1, 3, "none"), (F32, 1, 8, "leaky"), (F32, 1, 9, "relu6"), (F32, 1, None, "leaky"),
    (BF, 1, "arena", "relu6"),
    # groups: G = 2, k = 8 -> 4 per group (18 tiles each); G = 3, k = 9 -> 3 per group (24 tiles each)
    (BF, 2, 8, "relu6"), (F32, 2, 8, "leaky"), (BF, 3, 9, "relu6"), (F32, 3, None, "relu6"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,G,k,form", DW_WG)
def test_dwconv_wgrad_walk(dtype, G, k, form):
    L, Act, Engine, ParamStore, Pro = _gpu()
    lib = L.lib()
    c, h, w = 64, 45, 100
    n = 3 * G
    x = inp(rand(n, c, h, w, seed=41, scale=2.0), dtype)
    dy = inp(rand(n, c, h, w, seed=42), dtype)
    act = {"relu6": L.ACT_RELU6, "leaky": L.ACT_LEAKY, "none": L.ACT_NONE}[form]
    if form == "none" and G == 1:
        pro, xt = None, x.double()
    else:
        sc, sh = dyadic_pro(c, seed=43, groups=G)
        pro = Pro(sc.reshape(-1).cuda(), sh.reshape(-1).cuda(), act)
        xt = pro_f32(x, sc, sh, act, L, groups=G).double()
    xa = Act(to_act(Act, x, dtype).buf, 0, c, None, True, G)
    da = to_act(Act, dy, dtype)
    dw = torch.zeros(c, 1, 3, 3, device="cuda")
    db = torch.zeros(c, device="cuda")
    set_floats = 10 * CB * ((c + CB - 1) // CB)
    pc = C.byref(pro._c) if pro else None
    if G > 1:
        ws = nan_ws((G - 1) * set_floats)
        assert lib.isa_dwconv3x3_wgrad(xa.d(), pc, da.d(), L.ptr(dw), L.ptr(db), c, L.ptr(ws), ws.numel(), None,
                                       L.stream_ptr()) == -1, "ws_cap < G must be ISA_EINVAL"
    run_ws_call(L, lambda ws, wsf, sa: lib.isa_dwconv3x3_wgrad(xa.d(), pc, da.d(), L.ptr(dw), L.ptr(db), c, ws, wsf, sa,
                                                              L.stream_ptr()),
                k, set_floats, "isa_dwconv3x3_wgrad")
    wv = torch.zeros(c, 1, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xt, wv, padding=1, groups=c).backward(dy.double())
    tag = "dwwgrad %s G%d k=%s %s" % ("bf16" if dtype == BF else "f32", G, k, form)
    check(tag + " dW", dw, wv.grad, FP32_BOUND)
    check(tag + " db", db, dy.double().sum((0, 2, 3)), FP32_BOUND)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3, "arena"])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_dwconv_wgrad_fold_channel_tail(dtype, k):
    """The second stage (dw_slab_reduce_launch in conv_wgrad.hip: launched at once from a caller workspace, recorded
    in an arena) where the channel block is not full and dW has fewer rows than x has channels: c = 24 in one 32-wide
    block, csrc = 21.  One image of 9 x 33 pixels is 2 x 2 tiles; k = 1: one workgroup walks them, k = 3: three slabs to
    fold.  dW and db are 21 rows followed by guard values that must survive.  FP32_BOUND holds with the margin of the
    c = 64 cases: worst 1.9e-7 (bf16 dW), the same with the fold kernel this launcher replaced."""
    L, Act, Engine, ParamStore, Pro = _gpu()
    lib = L.lib()
    c, csrc, h, w, guard = 24, 21, 9, 33, 12345.0
    x = inp(rand(1, c, h, w, seed=44, scale=2.0), dtype)
    dy = inp(rand(1, c, h, w, seed=45), dtype)
    xa, da = to_act(Act, x, dtype), to_act(Act, dy, dtype)
    dw = torch.zeros(csrc * 9 + 64, device="cuda")
    db = torch.zeros(csrc + 64, device="cuda")
    dw[csrc * 9:] = guard
    db[csrc:] = guard
    set_floats = 10 * CB * ((c + CB - 1) // CB)
    run_ws_call(L, lambda ws, wsf, sa: lib.isa_dwconv3x3_wgrad(xa.d(), None, da.d(), L.ptr(dw), L.ptr(db), csrc, ws, wsf, sa,
                                                              L.stream_ptr()),
                k, set_floats, "isa_dwconv3x3_wgrad")
    wv = torch.zeros(c, 1, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), wv, padding=1, groups=c).backward(dy.double())
    tag = "dwwgrad tail %s k=%s" % ("bf16" if dtype == BF else "f32", k)
    check(tag + " dW", dw[:csrc * 9].view(csrc, 1, 3, 3), wv.grad[:csrc], FP32_BOUND)
    check(tag + " db", db[:csrc], dy.double().sum((0, 2, 3))[:csrc], FP32_BOUND)
    assert bool((dw[csrc * 9:] == guard).all()) and bool((db[csrc:] == guard).all()), "a row past csrc was written"


# ------------------------------------------------------------------------------------------------ 5. fused BN backward
def bn_setup(L, y, g, G, act, seed):
    """BN(y) constants [G][c] and the reduced backward sums of g (replica 0 of [G][8][2c]), float64 references."""
    n, c = y.shape[:2]
    gen = torch.Generator().manual_seed(seed)
    yg = y.double().view(G, n // G, c, *y.shape[2:])
    mean = yg.mean((1, 3, 4)).float()
    invstd = (1.0 / torch.sqrt(yg.var((1, 3, 4), unbiased=False) + 1e-5)).float()
    gamma = (torch.rand(c, generator=gen) + 0.5)
    beta = torch.randn(c, generator=gen)
    scale = (gamma[None] * invstd).float()
    shift = (beta[None] - mean * scale).float()
    gi = torch.arange(n) // (n // G)
    bc = lambda t: t[gi][:, :, None, None].double()      # noqa: E731
    z = y.double() * bc(scale) + bc(shift)
    dz = g.double() * act_grad64(z, act, L)
    yh = (y.double() - bc(mean)) * bc(invstd)
    r0 = dz.view(G, n // G, c, -1).sum((1, 3))
    r1 = (dz * yh).view(G, n // G, c, -1).sum((1, 3))
    red = torch.zeros(G, STAT_R, 2 * c)
    red[:, 0, :c], red[:, 0, c:] = r0.float(), r1.float()
    count = float(n // G * y.shape[2] * y.shape[3])
    k0, k1 = red[:, 0, :c].double() / count, red[:, 0, c:].double() / count
    dyv = bc(scale) * (dz - bc(k0) - yh * bc(k1))
    d = dict(scale=scale, shift=shift, mean=mean, invstd=invstd, red=red)
    gpu = {kk: v.reshape(-1).contiguous().cuda() for kk, v in d.items()}
    gpu["dgamma"] = torch.zeros(c, device="cuda")
    gpu["dbeta"] = torch.zeros(c, device="cuda")
    desc = L.IsaBnBwd(L.addr(gpu["scale"]), L.addr(gpu["shift"]), L.addr(gpu["mean"]), L.addr(gpu["invstd"]),
                      L.addr(gpu["red"]), None, L.addr(gpu["dgamma"]), L.addr(gpu["dbeta"]), count, act)
    return desc, gpu, dyv, r0.sum(0), r1.sum(0)


def xbn_setup(L, x, sc, sh, G):
    """BN(x) of the layer that produced x: mean / invstd [G][c] and the out_red buffer the kernel adds into."""
    n, c = x.shape[:2]
    xg = x.double().view(G, n // G, c, *x.shape[2:])
    mean = xg.mean((1, 3, 4)).float()
    invstd = (1.0 / torch.sqrt(xg.var((1, 3, 4), unbiased=False) + 1e-5)).float()
    gpu = dict(mean=mean.reshape(-1).cuda(), invstd=invstd.reshape(-1).cuda(),
               red=torch.zeros(G * STAT_R * 2 * c, device="cuda"))
    desc = L.IsaBnBwd(L.addr(sc), L.addr(sh), L.addr(gpu["mean"]), L.addr(gpu["invstd"]), None, L.addr(gpu["red"]),
                      None, None, 1.0, 0)
    return desc, gpu, mean, invstd


def xred_ref(L, gx, x, sc, sh, act, mean, invstd, G):
    """sum g_x * act'(z_x), sum g_x * act'(z_x) * xhat per group, from the stored (rounded) data gradient."""
    n, c = x.shape[:2]
    gi = torch.arange(n) // (n // G)
    bc = lambda t: t[gi][:, :, None, None].double()     # noqa: E731
    z = x.double() * bc(sc) + bc(sh)
    dz = gx * act_grad64(z, act, L)
    xh = (x.double() - bc(mean)) * bc(invstd)
    return torch.cat([dz.view(G, n // G, c, -1).sum((1, 3)), (dz * xh).view(G, n // G, c, -1).sum((1, 3))], 1)


FUSED = [
    # xmode, epi, G, k[, (images per group, h, w)].  dw_bn_bwd_kernel wants min(256 / ncb, tiles * G) workgroups, slab_grid
    # caps them at ws_floats / (10 * 32 * ncb), rounded to a multiple of G; c = 64 (ncb = 2).
    # Default shape: 3 images of 45x100 per group -> 72 tiles per group (ragged in x and y).  The XCD walk (see DW_FWD) exists only in the bf16 instantiation; the fp32
    # one strides from bx.  G = 1: k = 1 -> one workgroup walks 72 tiles; k = 3 -> 24 each; k = 8 -> 9 each (bf16: XCD
    # walk, chunk 9); k = 9 -> 8 each, no XCD walk; uncapped 72 workgroups, one tile each (bf16: XCD walk).
    # G = 2, k = 16 -> 8 per group, 9 tiles each (bf16: XCD walk per group); G = 2, k = 6 -> 3 per group, 24 tiles each;
    # G = 3, k = 9 -> 3 per group, 24 each; G = 3 uncapped -> group_grid(128, 3) = 126, 42 per group, 1-2 tiles each.
    # (1, 40, 416): 65 tiles; k = 32 -> bf16 XCD walk with chunk 9 and four workgroups per XCD: XCD 7 owns tiles 63-64,
    # so 2 of its workgroups are IDLE (per channel block) and write all-zero slabs into the NaN workspace; fp32: 32
    # workgroups stride over 65 tiles, 2-3 each.
    # xmode 0: plain x (the only form with a residual addend); 1: ReLU6 prologue + BN(x) sums; 2: LEAKY + BN(x) sums
    (0, False, 1, 1), (0, False, 1, 3), (0, True, 1, 8), (0, False, 1, 9), (0, True, 1, None), (0, False, 1, "arena"),
    (1, False, 1, 1), (1, True, 1, 3), (1, False, 1, 8), (1, True, 1, 9), (1, False, 1, None),
    (2, True, 1, 1), (2, False, 1, 8), (2, False, 1, None),
    (0, True, 2, 16), (1, False, 2, 6), (1, True, 2, 16), (2, False, 3, 9), (1, False, 3, None),
    (0, False, 1, 32, (1, 40, 416)), (1, True, 1, 32, (1, 40, 416)),
]
FUSED = [f if len(f) == 5 else f + ((3, 45, 100),) for f in FUSED]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("xmode,epi,G,k,shape", FUSED)
def test_dwconv_bn_backward_walk(dtype, xmode, epi, G, k, shape):
    L, Act, Engine, ParamStore, Pro = _gpu()
    lib = L.lib()
    c = 64
    npg, h, w = shape
    n = npg * G
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
    ydesc, ygpu, dyv, r0, r1 = bn_setup(L, y, g, G, yact, seed=55)
    dyq = rs(dyv, dtype)                                       # dy as the kernel holds it in LDS
    ga, ya_, xa = (Act(to_act(Act, t, dtype).buf, 0, c, None, True, G) for t in (g, y, x))
    xdesc, xpro, xact, sc, sh = None, None, L.ACT_NONE, None, None
    if xmode:
        xact = L.ACT_RELU6 if xmode == 1 else L.ACT_LEAKY
        sc, sh = dyadic_pro(c, seed=56, groups=G)
        scg, shg = sc.reshape(-1).cuda(), sh.reshape(-1).cuda()
        xpro = Pro(scg, shg, xact)
        xdesc, xgpu, xmean, xinv = xbn_setup(L, x, scg, shg, G)
        xt = pro_f32(x, sc, sh, xact, L, groups=G).double()
    else:
        xt = x.double()
    old = inp(rand(n, c, h, w, seed=57), dtype) if epi else None
    add = inp(rand(n, c, h, w, seed=58), dtype) if (epi and xmode == 0) else None
    dxa = Act(to_act(Act, old if epi else torch.full((n, c, h, w), float("nan")), dtype).buf, 0, c, None, True, G)
    adda = to_act(Act, add, dtype) if add is not None else None
    dw = torch.zeros(c, 1, 3, 3, device="cuda")
    set_floats = 10 * CB * ((c + CB - 1) // CB)
    pc = C.byref(xpro._c) if xpro else None
    xd = C.byref(xdesc) if xdesc is not None else None

    def call(ws, wsf, sa):
        return lib.isa_dwconv3x3_bn_backward(ga.d(), ya_.d(), C.byref(ydesc), xa.d(), pc, xd, eng.packer.ptr(reg["dgrad"]),
                                             L.ptr(dw), c, dxa.d(), int(epi), adda.d() if adda else None, ws, wsf, sa,
                                             L.stream_ptr())
    if G > 1:
        ws = nan_ws((G - 1) * set_floats)
        assert call(L.ptr(ws), ws.numel(), None) == -1, "ws_cap < G must be ISA_EINVAL"
    run_ws_call(L, call, k, set_floats, "isa_dwconv3x3_bn_backward")
    # references
    dx = F.conv_transpose2d(dyq, wt.double(), padding=1, groups=c)
    if epi:
        dx = dx + old.double()
    if add is not None:
        dx = dx + add.double()
    wv = torch.zeros(c, 1, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(xt, wv, padding=1, groups=c).backward(dyq)
    tag = "dwbnbwd %s x%d epi%d G%d k=%s %dx%d" % ("bf16" if dtype == BF else "f32", xmode, epi, G, k, h, w)
    check(tag + " dx", dxa.nchw(), dx, store_bound(dtype))
    check(tag + " dW", dw, wv.grad, acc_bound(dtype, True))
    check(tag + " dgamma", ygpu["dgamma"], r1, FP32_BOUND)
    check(tag + " dbeta", ygpu["dbeta"], r0, FP32_BOUND)
    if xmode:
        ref = xred_ref(L, dxa.nchw().double().cpu(), x, sc, sh, xact, xmean, xinv, G)      # over the stored dx
        check(tag + " xred", stat_sums(xgpu["red"], c, G), ref, FP32_BOUND)


PW = [
    # N, K, xmode, epi, G, k.  pw_bn_bwd_kernel (conv_fused_bwd.hip) wants min((chunks + 3) / 4 * G, 512) workgroups, slab_grid
    # caps them at ws_floats / slab, rounded to a multiple of G.
    # 2 images of 37x70 per group = 5180 pixels = 162 chunks of 32: k = 1 -> 40-41 chunks per wave; k = 3 -> 13-14; k = 8 -> 5; k = 9 -> 4-5; uncapped 41 * G workgroups (one chunk per wave)
    (32, 32, 0, False, 1, 1), (32, 32, 1, True, 1, 3), (64, 32, 2, False, 1, 8), (32, 64, 1, False, 1, 9),
    (64, 64, 0, True, 1, None), (64, 64, 1, False, 1, "arena"), (32, 64, 2, True, 1, 1),
    (64, 32, 1, False, 2, 8), (32, 32, 0, True, 2, 6), (64, 64, 2, False, 3, 9), (32, 64, 1, True, 3, None),
]


@pytest.mark.gpu
@pytest.mark.parametrize("N,K,xmode,epi,G,k", PW)
def test_conv1x1_bn_backward_walk(N, K, xmode, epi, G, k):
    L, Act, Engine, ParamStore, Pro = _gpu()
    lib = L.lib()
    dtype = BF
    h, w = 37, 70
    n = 2 * G
    W = q(rand(N, K, seed=61, scale=K ** -0.5), BF)
    g = q(rand(n, N, h, w, seed=62), BF)
    y = q(rand(n, N, h, w, seed=63, scale=2.0) + 1.0, BF)
    x = q(rand(n, K, h, w, seed=64, scale=2.0), BF)
    yact = L.ACT_LEAKY if xmode == 2 else L.ACT_RELU6
    ydesc, ygpu, dyv, r0, r1 = bn_setup(L, y, g, G, yact, seed=65)
    dyq = rb(dyv)
    ga, ya_, xa = (Act(to_act(Act, t, dtype).buf, 0, t.shape[1], None, True, G) for t in (g, y, x))
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
    dxa = Act(to_act(Act, old if epi else torch.full((n, K, h, w), float("nan")), dtype).buf, 0, K, None, True, G)
    adda = to_act(Act, add, dtype) if add is not None else None
    Wg = W.contiguous().cuda()
    dw = torch.zeros(N, K, device="cuda")
    tn, tk = (N + 31) // 32, (K + 31) // 32
    set_floats = tn * tk * 1024 + tn * 32
    pc = C.byref(xpro._c) if xpro else None
    xd = C.byref(xdesc) if xdesc is not None else None

    def call(ws, wsf, sa):
        return lib.isa_conv1x1_bn_backward(ga.d(), ya_.d(), C.byref(ydesc), xa.d(), pc, xd, L.ptr(Wg), L.ptr(dw), dxa.d(),
                                           int(epi), adda.d() if adda else None, ws, wsf, sa, L.stream_ptr())
    if G > 1:
        ws = nan_ws((G - 1) * set_floats)
        assert call(L.ptr(ws), ws.numel(), None) == -1, "ws_cap < G must be ISA_EINVAL"
    run_ws_call(L, call, k, set_floats, "isa_conv1x1_bn_backward")
    # dx: bf16 MFMA of dy and W, rounded to bf16; then + old, rounded; then + addend, rounded (conv_fused_bwd.hip)
    dx = rb(torch.einsum("bnhw,nk->bkhw", dyq, W.double()))
    if epi:
        dx = rb(dx + old.double())
        dx = rb(dx + add.double())
    ref_dw = torch.einsum("bnhw,bkhw->nk", dyq, xt)
    tag = "pwbnbwd %dx%d x%d epi%d G%d k=%s" % (N, K, xmode, epi, G, k)
    check(tag + " dx", dxa.nchw(), dx, store_bound(dtype))
    check(tag + " dW", dw, ref_dw, acc_bound(dtype, True))
    check(tag + " dgamma", ygpu["dgamma"], r1, FP32_BOUND)
    check(tag + " dbeta", ygpu["dbeta"], r0, FP32_BOUND)
    if xmode:
        ref = xred_ref(L, dxa.nchw().double().cpu(), x, sc, sh, xact, xmean, xinv, G)      # over the stored dx
        check(tag + " xred", stat_sums(xgpu["red"], K, G), ref, FP32_BOUND)


# ------------------------------------------------------------------------------------------------ 6. eval dw + pw block
DWPW = [
    # c, N, images, residual.  launch_dwpw (dwpw_eval.hip): LDS = 340 * halo stride * halo bytes + 256*(c+8)*2
    # + 32*NT*(c+8)*2 + 9*c*4 + 2*c*4, per_cu = 160 KB / LDS (<= 3), gx = 256 * per_cu; 256x256 images = 8 x 32 tiles
    # c = 32, N = 16: fp32 halo, NT = 1, one channel block per tile step: 73 KB -> per_cu 2, gx = 512; 8 images = 2048
    # tiles, 4 per workgroup
    (32, 16, 8, False), (32, 16, 8, True),
    # c = 64, N = 64: bf16 halo, NT = 2, two channel blocks per tile (the next block prefetched while one is computed):
    # 27200 + 36864 + 9216 + 2304 + 512 = 76 KB -> per_cu 2, gx = 512; 8 images = 2048 tiles, 4 per workgroup
    (64, 64, 8, True),
    # c = 96, N = 32: bf16 halo, NT = 1, three channel blocks: 27200 + 53248 + 6656 + 3456 + 768 = 91 KB -> per_cu 1,
    # gx = 256; 4 images = 1024 tiles, 4 per workgroup
    (96, 32, 4, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("c,N,n,with_res", DWPW)
def test_dwpw_eval_walk(c, N, n, with_res):
    """isa_dwpw_eval (bf16 only) at 4 tiles per workgroup; see DWPW for the grid arithmetic."""
    L, Act, Engine, ParamStore, Pro = _gpu()
    h, w = 256, 256
    wd = q(rand(c, 1, 3, 3, seed=71, scale=1 / 3.0), BF)
    wp = q(rand(N, c, 1, 1, seed=72, scale=c ** -0.5), BF)
    ps = ParamStore([("dw", wd.shape), ("pw", wp.shape)], "cuda")
    ps.load_state_dict(dict(dw=wd, pw=wp))
    eng = Engine(ps, BF)
    eng.begin(bn_train=False, record=False)
    rd, rc = eng.reg_dw("dw"), eng.reg_conv("pw")
    eng.packer.pack()
    x = q(rand(n, c, h, w, seed=73, scale=2.0), BF)
    s1, h1 = dyadic_pro(c, seed=74)
    s2, h2 = rand(N, seed=75).abs() + 0.5, rand(N, seed=76)
    res = q(rand(n, N, h, w, seed=77), BF)
    xa = to_act(Act, x, BF)
    ra = to_act(Act, res, BF) if with_res else None
    ya = eng.new_act(n, h, w, N)
    ya.buf.fill_(float("nan"))
    g1, g2 = [t.reshape(-1).contiguous().cuda() for t in (s1, h1)]
    e2, f2 = s2.cuda(), h2.cuda()
    ep = L.IsaConvEp(L.addr(e2), L.addr(f2), L.ACT_NONE, C.addressof(ra._c) if ra else None)
    L.check(L.lib().isa_dwpw_eval(xa.d(), eng.packer.ptr(rd["fwd"]), L.ptr(g1), L.ptr(g2), eng.packer.ptr(rc["fwd"]),
                                  rc["kp"], C.byref(ep), ya.d(), L.stream_ptr()), "isa_dwpw_eval")
    torch.cuda.synchronize()
    # the raw depthwise result is rounded to bf16 (as the op-granular path stores it), goes through BN1 + ReLU6 and is
    # rounded to bf16 again as the 1x1 GEMM's operand (dwpw_eval.hip)
    d = rb(F.conv2d(x.double(), wd.double(), padding=1, groups=c))
    t = rb((d * s1[0][None, :, None, None].double() + h1[0][None, :, None, None].double()).clamp(0, 6))
    ref = F.conv2d(t, wp.double()) * s2.double()[None, :, None, None] + h2.double()[None, :, None, None]
    if with_res:
        ref = ref + res.double()
    check("dwpw c%d N%d res%d y" % (c, N, with_res), ya.nchw(), ref, BF16_STORE)


# ------------------------------------------------------------------------------------------------ 7. the bounds catch tile bugs
def test_walk_bounds_reject_tile_bugs():
    """The comparison and bounds above, applied to float64 references corrupted the way a broken walk would corrupt an
    output, must reject every corruption: a stale LDS tile (one 8x32 x 32-channel block holding the previous tile's
    values), one halo row read from the neighbouring image, the last ragged tile left zero, and one workgroup's slab
    missing from a weight gradient.  The loosest bound of the file is used, so every GPU case would catch them."""
    loosest = max(BF16_STORE, FUSED_DW_BF16, FP32_BOUND)
    n, c, h, w = 2, 64, 20, 70                            # tiles_x = 3 (ragged: 70 % 32 = 6), tiles_y = 3 (20 % 8 = 4)
    x = rand(n, c, h, w, seed=81).double()
    wt = rand(c, 1, 3, 3, seed=82, scale=1 / 3.0).double()
    ref = F.conv2d(x, wt, padding=1, groups=c)
    bad = []
    # 1. stale LDS buffer: tile (b 1, ty 1, tx 1, channel block 1) holds tile (b 1, ty 1, tx 0)'s values
    t = ref.clone()
    t[1, 32:64, 8:16, 32:64] = ref[1, 32:64, 8:16, 0:32]
    bad.append(("stale tile", t))
    # 2. the top halo row of image 1's first tile row read from image 0's last row instead of the zero padding
    t = ref.clone()
    t[1, :, 0, :] += F.conv2d(x[0:1, :, h - 1:h, :], wt[:, :, 0:1, :], padding=(0, 1), groups=c)[0, :, 0, :]
    bad.append(("halo row from the neighbouring image", t))
    # 3. the last ragged tile (ty 2, tx 2: 4 rows x 6 columns) never written
    t = ref.clone()
    t[n - 1, :, 16:20, 64:70] = 0
    bad.append(("last ragged tile zeroed", t))
    for what, t in bad:
        e, where = walk_err(t, ref)
        assert e > 10 * loosest, (what, e, where)
    # 4. weight gradient of 9 workgroups' slabs, one slab dropped
    dy = rand(n, c, h, w, seed=83).double()
    xs = F.pad(x, (1, 1, 1, 1))
    prod = torch.stack([(dy * xs[:, :, ky:ky + h, kx:kx + w]) for ky in range(3) for kx in range(3)], -1)
    slabs = prod.permute(0, 2, 3, 1, 4).reshape(-1, c, 9)
    parts = torch.stack([p.sum(0) for p in slabs.chunk(9)])          # 9 slabs, as from k = 9 workgroups
    dw = parts.sum(0)
    e, where = walk_err(parts[1:].sum(0), dw)
    assert e > 10 * loosest, ("slab dropped", e, where)
    # and the clean references pass the tightest bound
    assert walk_err(ref.clone(), ref)[0] < FP32_BOUND and rel(dw, dw) < FP32_BOUND
