"""The streaming kernels between the convolutions, against float64, at the shapes and walks the product runs.

Entry points: isa_bn_bwd_reduce / isa_bn_bwd_apply (the BatchNorm backward, 16.6 % of a training step), isa_affine_act_res
(materialised BatchNorm + residuals + Dropout2d), the gradient glue isa_axpy / isa_scale_bc / isa_avgpool2(_bwd), the
semantic head's squeeze-excite isa_chan_mean / isa_se_fc / isa_se_bwd, and the optimizer's isa_sqnorm / isa_adadelta.
Before this file they were compared with a reference only at one-trip shapes (test_gpu_fused_dw.py,
test_bn_finalize_and_materialize) or only through the loose gate of the whole train step.

Every call goes through the C ABI (isa_amd.lib).  Tensors are channel slices at c0 = 8 or 16 of wider buffers whose other
channels hold NaN, as the network's concat buffers do; every output's neighbours must stay bit-unchanged.  Inputs are
values of the storage dtype (bf16-valued for bf16, full-precision fp32 for fp32) and prologue / BatchNorm constants are
dyadic (scale in {0.5 .. 1.5}, shift k/8), so z = fma(y, scale, shift) is exact on bf16 inputs; the reference takes
z as that fma's fp32 result, so activation thresholds decide as in the kernel.  Some elements sit exactly at z = 0 and
z = 6, where the ReLU / ReLU6 gradient is 0 as in torch.  Each parametrize entry that claims a long walk states its
grid and trips per workgroup from the launch code it names; test_stated_grids_match_the_launch_code checks the BatchNorm
backward's statements against a mirror of bn_bwd_common.

Bounds (error printed as STREAMERR; worst of each entry point measured on MI355X over all cases of this file):
  * SUM_BOUND = 1e-5, per output relative to its sum of |terms|, for everything accumulated in fp32: the reduce rows,
    dgamma / dbeta, isa_chan_mean, isa_se_fc's hidden layer, isa_se_bwd's dgate / dmean / dW1 / db1 / dW2 / db2 and
    isa_sqnorm.  Only the fp32 summation order is left.  For isa_se_bwd the |terms| are those of the whole expanded
    chain (the same backward run on absolute values), since dgate's rounding reaches the weight gradients.
    Measured: reduce 1.5e-7, apply dgamma / dbeta 2.0e-7 (through Engine in eval mode 1.7e-8), chan_mean 4.7e-7,
    se_fc hidden 1.7e-7, se_bwd 1.8e-8, sqnorm 8.0e-7.
  * FP32_BOUND = 1e-5 relative to max |ref| for fp32-stored outputs.  Measured: bn apply 1.3e-7 (Engine eval dx
    1.2e-7), affine_act_res 1.4e-7, its finalize arrays and running statistics 1.4e-7, axpy 5.7e-8, scale_bc 7.7e-8,
    avgpool2 8.8e-8, se_fc gate 3.6e-7, se_bwd dx 7.8e-8, adadelta square_avg 1.0e-6, acc_delta 5.6e-7, params 1.1e-7.
  * OPT_UPDATE_BOUND = 2e-5 for the parameter change of each adadelta step relative to its max: the clip coefficient
    carries the fp32 rounding of sqrt(sqnorm) into every element and three steps compound it.  Measured 2.1e-6.
  * BF16_STORE = 2**-8 relative to max |ref| for bf16-stored outputs, the storage rounding itself (see
    test_gpu_backbone_walk.py).  Measured: bn apply 3.1e-3 (Engine eval dx 2.1e-3), affine_act_res 3.5e-3, axpy 3.3e-3,
    scale_bc 3.1e-3, avgpool2 3.0e-3, se_bwd dx 3.4e-3.
test_streaming_bounds_reject_bugs re-runs the float64 references with one plausible bug each and checks that the
bounds reject every one by a wide margin.

All cases run in about 15 s on one MI355X.
"""
import ctypes as C
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from test_gpu_backbone_walk import BF16_STORE, FP32_BOUND, dyadic_pro, inp  # noqa: E402
from test_gpu_ops import _gpu, rand  # noqa: E402

BF = torch.bfloat16
F32 = torch.float32
STAT_R = 8
SUM_BOUND = 1e-5
OPT_UPDATE_BOUND = 2e-5
NAN = float("nan")
LEAKY_SLOPE = float(torch.tensor(0.01, dtype=torch.float32))        # the kernels' 0.01f
ACTS = {"none": 0, "relu": 1, "relu6": 2, "leaky": 3, "tanh": 4}     # ISA_ACT_*


def store_bound(dtype):
    return BF16_STORE if dtype == BF else FP32_BOUND


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ comparison
class Err:
    """max |got - ref| / max |ref| accumulated over chunks (images), with the worst element's position."""
    def __init__(self):
        self.num, self.den, self.where = 0.0, 0.0, ""

    def add(self, got, ref, tag=""):
        got, ref = got.double().cpu(), ref.double().cpu()
        assert got.shape == ref.shape, (got.shape, ref.shape)
        d = torch.nan_to_num((got - ref).abs(), nan=float("inf"))
        i = int(d.reshape(-1).argmax())
        if float(d.reshape(-1)[i]) >= self.num:
            self.num = float(d.reshape(-1)[i])
            idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))
            self.where = "%s%s: got %g, ref %g" % (tag, idx, float(got[idx]), float(ref[idx]))
        self.den = max(self.den, float(ref.abs().max()))
        return self

    def value(self):
        return self.num / (self.den + 1e-30)

    def check(self, what, bound):
        e = self.value()
        print("STREAMERR %-52s %.3e  bound %.1e" % (what, e, bound))
        assert e < bound, "%s: error %.3g >= %.3g at %s" % (what, e, bound, self.where)


def check(what, got, ref, bound):
    Err().add(got, ref).check(what, bound)


def sum_err(got, ref, mag):
    """max over outputs of |got - ref| / (sum of |terms| of that output)."""
    got, ref, mag = got.double().cpu(), ref.double().cpu(), mag.double().cpu()
    d = torch.nan_to_num((got - ref).abs(), nan=float("inf")) / mag.clamp_min(1e-30)
    i = int(d.reshape(-1).argmax())
    return float(d.reshape(-1)[i]), "element %d: got %g, ref %g, sum|terms| %g" % (
        i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(mag.reshape(-1)[i]))


def check_sum(what, got, ref, mag, bound=SUM_BOUND):
    e, where = sum_err(got, ref, mag)
    print("STREAMERR %-52s %.3e  bound %.1e (sum)" % (what, e, bound))
    assert e < bound, "%s: error %.3g >= %.3g at %s" % (what, e, bound, where)


def neighbours_equal(buf, orig, c0, c):
    """The channels of a [.., ld] buffer outside [c0, c0 + c) are bit-identical to `orig`."""
    bits = torch.int16 if buf.dtype == BF else torch.int32
    for lo, hi in ((0, c0), (c0 + c, buf.shape[-1])):
        if hi > lo and not torch.equal(buf[..., lo:hi].contiguous().view(bits), orig[..., lo:hi].contiguous().view(bits)):
            return False
    return True


class Slice:
    """An NHWC tensor [n, h, w, c] (given as [n, h*w, c] on the host) stored at channel c0 of a wider buffer whose other
    channels are NaN: the network's concat-buffer slices (network.py buffer plan)."""
    def __init__(self, L, t, h, w, dtype, c0=8, groups=1, fill=None):
        n, P, c = t.shape
        assert P == h * w
        ld = c0 + cdiv(c, 8) * 8 + 8
        self.L, self.c0, self.c, self.n, self.h, self.w, self.dtype = L, c0, c, n, h, w, dtype
        self.buf = torch.full((n, h, w, ld), NAN, dtype=dtype, device="cuda")
        self.buf[..., c0:c0 + c] = (t if fill is None else torch.full_like(t, fill)).view(n, h, w, c).to(dtype).cuda()
        self.orig = self.buf.clone()
        self.t = L.IsaTensor(self.buf.data_ptr() + c0 * self.buf.element_size(), n, h, w, c, ld, L.dtype_code(dtype),
                             groups)

    def d(self):
        return C.byref(self.t)

    def get(self, b=None):
        """[n, h*w, c] (or image b: [h*w, c]) as float64 on the host."""
        v = self.buf[..., self.c0:self.c0 + self.c]
        if b is not None:
            return v[b].reshape(-1, self.c).double().cpu()
        return v.reshape(self.n, -1, self.c).double().cpu()

    def check_neighbours(self, what):
        assert neighbours_equal(self.buf, self.orig, self.c0, self.c), "%s: a neighbouring channel was written" % what


def spread(sums, seed):
    """[G][2c] sums -> [G][8][2c] float32 replicas that add up to them (the consumer adds them in replica order)."""
    G = sums.shape[0]
    w = torch.rand(G, STAT_R, 1, generator=torch.Generator().manual_seed(seed)).double()
    w = w / w.sum(1, keepdim=True)
    return (w * sums[:, None, :]).float()


def nhwc(n, P, c, dtype, seed, scale=1.0, offset=0.0):
    return inp(rand(n, P, c, seed=seed, scale=scale) + offset, dtype)


def rs(t, dtype):
    return t.to(BF).double() if dtype == BF else t.double()


# ------------------------------------------------------------------------------------------------ float64 references
def z_of(y, sc, sh):
    """The kernels' z = fmaf(y, scale, shift): exact in float64 for these inputs, then rounded once to fp32."""
    return (y.double() * sc.double() + sh.double()).float().double()


def act64(z, act):
    if act == ACTS["relu"]:
        return z.clamp_min(0)
    if act == ACTS["relu6"]:
        return z.clamp(0, 6)
    if act == ACTS["leaky"]:
        return torch.where(z > 0, z, (z.float() * torch.tensor(0.01, dtype=torch.float32)).double())
    if act == ACTS["tanh"]:
        return torch.tanh(z)
    return z


def act_grad64(z, act):
    if act == ACTS["relu"]:
        return (z > 0).double()
    if act == ACTS["relu6"]:
        return ((z > 0) & (z < 6)).double()
    if act == ACTS["leaky"]:
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, LEAKY_SLOPE))
    if act == ACTS["tanh"]:
        return 1 - torch.tanh(z) ** 2
    return torch.ones_like(z)


def bn_dz(dt_b, y_b, cst, g, act, bs_b):
    """dz = dt * act'(z) (* bscale) and yhat of one image of statistic group g; cst: float32 [G, c] constants."""
    z = z_of(y_b, cst["scale"][g], cst["shift"][g])
    dz = dt_b.double() * act_grad64(z, act)
    if bs_b is not None:
        dz = dz * bs_b.double()
    yh = (y_b.double() - cst["mean"][g].double()) * cst["invstd"][g].double()
    return dz, yh


def bn_sums(dt, y, cst, act, bs, G, skip=None):
    """[G][2c] reduce sums (sum dz, sum dz*yhat) and their sums of |terms|.  skip(b) -> pixel mask of terms to drop
    (the mutation test)."""
    n, P, c = dt.shape
    s, a = torch.zeros(G, 2 * c, dtype=torch.float64), torch.zeros(G, 2 * c, dtype=torch.float64)
    for b in range(n):
        g = b // (n // G)
        dz, yh = bn_dz(dt[b], y[b], cst, g, act, bs[b] if bs is not None else None)
        if skip is not None:
            keep = (~skip(b)).double()[:, None]
            dz = dz * keep
        t = dz * yh
        s[g, :c] += dz.sum(0)
        s[g, c:] += t.sum(0)
        a[g, :c] += dz.abs().sum(0)
        a[g, c:] += t.abs().sum(0)
    return s, a


def bn_dy(dt_b, y_b, cst, g, act, bs_b, k, train):
    """apply pass of one image: scale * (dz - k0 - yhat * k1), or scale * dz in eval mode."""
    dz, yh = bn_dz(dt_b, y_b, cst, g, act, bs_b)
    sc = cst["scale"][g].double()
    if not train:
        return sc * dz
    return sc * (dz - k[g, 0] - yh * k[g, 1])


def bn_bwd_grid(C, pixels, apply):
    """bn_bwd_common (elementwise.hip): (grid.x, grid.y, trips of the pixel loop for workgroup 0) per statistic group."""
    cg = cdiv(C, 8)
    sh = 0
    while (1 << sh) < cg:
        sh += 1
    sh = min(sh, 8)
    if cg > 16:                        # wide: 32-channel chunks, 64 pixel rows per trip
        sh, gy = 2, cdiv(cg, 4)
        trips = cdiv(pixels, 64)
        grid = (trips + 1) // 2 if apply else (trips + 3) // 4
        grid = max(1, min(grid, 512 if apply else 128))
    else:
        gy, per, iters = 1, 256 >> sh, 16
        if cdiv(pixels, per * 16) < 512:
            iters = max(2, pixels // (per * 512))
        grid = min(max(cdiv(pixels, per * iters), 1), 2048)           # walk_grid -> grid_cap
        if not apply:
            grid = min(grid, 1024)
    return grid, gy, cdiv(pixels, grid * (256 >> sh))


def bn_ppb(C):
    """Pixels a workgroup of bn_bwd_kernel covers per trip: 256 >> sh (sh = 2 on wide tensors)."""
    cg = cdiv(C, 8)
    return 64 if cg > 16 else 256 >> min(8, max(0, math.ceil(math.log2(cg))))


# ------------------------------------------------------------------------------------------------ 1. BatchNorm backward
# name, dtype, n, h, w, C, G, act, bscale, form[, stated walks].  form: "train" = reduce into a pre-filled red, then
# apply (train = 1) from an exact red into a separate dy; "chain" = reduce -> apply with the kernel's own red, in place
# (dy = dt), as Engine.bn; "eval" = reduce -> apply(train = 0) with red, then again with red = NULL; "act" = the
# activation-only form of Engine.act (NULL constants, NULL red, count 1, train 0, in place).
# Stated walks: {"reduce"|"apply": (grid.x, grid.y, trips per workgroup)} from bn_bwd_common, per statistic group.
BN_CASES = [
    # narrow (C <= 128): sh = ceil log2(C / 8), 256 >> sh pixels per trip of a workgroup.
    # sh = 0, 646 px: iters floored at 2 -> grid cdiv(646, 512) = 2; workgroup 0 makes 2 trips, the second ragged
    ("sh0-grid2", F32, 2, 17, 19, 8, 1, "relu6", False, "train", {"reduce": (2, 1, 2), "apply": (2, 1, 2)}),
    # sh = 1, 6000 px: iters 2 -> grid 24, 2 trips, the last ragged
    ("sh1", BF, 3, 40, 50, 16, 1, "none", True, "train", {"reduce": (24, 1, 2), "apply": (24, 1, 2)}),
    # sh = 2 with a tail group (C = 21): 99 px, iters 2 -> grid 1, 2 trips of 64 px (the second 35)
    ("sh2-c21-grid1", BF, 1, 9, 11, 21, 1, "leaky", False, "train", {"reduce": (1, 1, 2), "apply": (1, 1, 2)}),
    # production 8x256x256 at C = 32: 524288 px, iters 16 -> grid 512, 16 trips
    ("sh2-prod", BF, 8, 256, 256, 32, 1, "relu6", True, "chain", {"reduce": (512, 1, 16), "apply": (512, 1, 16)}),
    # sh = 3, G = 3 with bscale and tanh (ACT_RT): 2040 px per group, iters 2 -> grid 32, 2 trips
    ("sh3-G3-tanh", F32, 6, 30, 34, 64, 3, "tanh", True, "train", {"reduce": (32, 1, 2), "apply": (32, 1, 2)}),
    ("sh3-G2-bs", BF, 4, 30, 30, 64, 2, "none", True, "chain", {"reduce": (29, 1, 2), "apply": (29, 1, 2)}),
    # fp32 with bscale and no activation (the one dtype x activation x bscale instantiation no other case launches), C = 20
    ("sh2-c20-none-bs-f32", F32, 2, 9, 11, 20, 1, "none", True, "train"),
    # sh = 4 at the reduce pass's 1024 cap: 263168 px, iters 16 -> walk_grid 1028; reduce capped at 1024 -> 17 trips of
    # 16 px, the 17th covering only 1024 px (64 workgroups); apply keeps 1028 -> 16 trips, the last ragged
    ("sh4-cap1024", BF, 4, 256, 257, 128, 1, "relu6", False, "train", {"reduce": (1024, 1, 17), "apply": (1028, 1, 16)}),
    ("sh4-G2-relu-eval", F32, 4, 20, 24, 128, 2, "relu", True, "eval", {"reduce": (30, 1, 2), "apply": (30, 1, 2)}),
    ("sh2-relu-eval", BF, 2, 31, 33, 24, 1, "relu", False, "eval"),
    # wide (C > 128): sh = 2, blockIdx.y = 32-channel chunk, 64 px per trip; reduce grid (trips + 3) / 4 <= 128, apply
    # (trips + 1) / 2 <= 512.  C = 136, 66560 px = 1040 trips: reduce 128 workgroups x 9 trips (the 9th ragged), apply at
    # the 512 cap, 3 trips for workgroups 0-15 and 2 for the others; 5 chunks, the last one 8 channels
    ("w136-apply512", BF, 4, 128, 130, 136, 1, "relu6", True, "train", {"reduce": (128, 5, 9), "apply": (512, 5, 3)}),
    # C = 246: 8 chunks, the last 22 channels ending in a 6-channel group; 43053 px = 673 trips: reduce at the 128 cap,
    # 6 trips (the last ragged), apply 337 x 2
    ("w246-ragged", F32, 3, 113, 127, 246, 1, "leaky", False, "train", {"reduce": (128, 8, 6), "apply": (337, 8, 2)}),
    # production 16x64x64 at C = 256: 1024 trips -> reduce 128 x 8, apply 512 x 2
    ("w256-prod", BF, 16, 64, 64, 256, 1, "relu6", True, "chain", {"reduce": (128, 8, 8), "apply": (512, 8, 2)}),
    # production 16x16x16 at C = 512: 64 trips -> reduce 16 x 4, apply 32 x 2
    ("w512-prod", BF, 16, 16, 16, 512, 1, "none", False, "train", {"reduce": (16, 16, 4), "apply": (32, 16, 2)}),
    ("w512-G3-tanh", F32, 6, 16, 16, 512, 3, "tanh", False, "chain", {"reduce": (2, 16, 4), "apply": (4, 16, 2)}),
    ("w1024-G2-eval", F32, 4, 12, 14, 1024, 2, "relu6", True, "eval", {"reduce": (2, 32, 3), "apply": (3, 32, 2)}),
    ("w136-G2-bs", BF, 4, 40, 40, 136, 2, "leaky", True, "train", {"reduce": (13, 5, 4), "apply": (25, 5, 2)}),
    # Engine.act's form
    ("act-relu6", BF, 2, 64, 64, 32, 1, "relu6", False, "act"),
    ("act-relu", F32, 2, 33, 35, 24, 1, "relu", False, "act"),
    ("act-leaky", BF, 3, 20, 22, 21, 1, "leaky", False, "act"),
    ("act-tanh", F32, 2, 33, 35, 136, 1, "tanh", False, "act"),
]


def bn_inputs(case):
    name, dtype, n, h, w, c, G, act_name, bscale, form = case[:10]
    P = h * w
    act = ACTS[act_name]
    # a per-channel mean in dt, so that the apply pass's batch-statistics terms (sum dz, sum dz * yhat) are of the
    # order of dy itself and a wrong one shows even at the bf16 bound
    dt = nhwc(n, P, c, dtype, seed=1, offset=rand(c, seed=10))
    y = nhwc(n, P, c, dtype, seed=2, scale=2.0, offset=0.5)
    if form == "act":
        sc, sh = torch.ones(1, c), torch.zeros(1, c)
    else:
        sc, sh = dyadic_pro(c, seed=3, groups=G)
    # ties: z exactly 0 and 6 on the first pixels of every image, in the channels whose scale is a power of two (there
    # (t - shift) / scale is exact and bf16-valued)
    np_ = min(P, 16)
    for b in range(n):
        g = b // (n // G) if form != "act" else 0
        ok = (sc[g] == 0.5) | (sc[g] == 1.0)
        for p in range(np_):
            t = 0.0 if p % 2 == 0 else 6.0
            y[b, p, ok] = (t - sh[g, ok]) / sc[g, ok]
    gen = torch.Generator().manual_seed(4)
    cst = dict(scale=sc.float(), shift=sh.float(),
               mean=(torch.randn(G, c, generator=gen) * 0.5).float() if form != "act" else torch.zeros(1, c),
               invstd=(torch.rand(G, c, generator=gen) + 0.5).float() if form != "act" else torch.ones(1, c))
    bs = (rand(n, c, seed=5) > 0).float() * 2.0 if bscale else None
    return dtype, n, h, w, c, G, act, form, dt, y, cst, bs


@pytest.mark.gpu
@pytest.mark.parametrize("case", BN_CASES, ids=[c[0] for c in BN_CASES])
def test_bn_bwd(case):
    L = _gpu()[0]
    lib = L.lib()
    dtype, n, h, w, c, G, act, form, dt, y, cst, bs = bn_inputs(case)
    tag = "bn %s %s" % (case[0], "bf16" if dtype == BF else "f32")
    P = h * w
    count = float(n // G * P)
    c0 = 16 if c % 16 else 8
    dts = Slice(L, dt, h, w, dtype, c0=c0, groups=G)
    ys = Slice(L, y, h, w, dtype, c0=8, groups=G)
    gp = {k: v.reshape(-1).contiguous().cuda() for k, v in cst.items()}
    bsg = bs.reshape(-1).contiguous().cuda() if bs is not None else None
    st = L.stream_ptr()

    if form == "act":        # Engine.act: dy = dt * act'(y) in place
        L.check(lib.isa_bn_bwd_apply(dts.d(), ys.d(), None, None, None, None, act, None, None, None, 1.0, 0, dts.d(),
                                     None, None, st), "isa_bn_bwd_apply(act)")
        torch.cuda.synchronize()
        err = Err()
        for b in range(n):
            err.add(dts.get(b), dt[b].double() * act_grad64(y[b].double(), act), "image %d " % b)
        err.check(tag + " dy", store_bound(dtype))
        dts.check_neighbours(tag + " dy")
        ys.check_neighbours(tag + " y")
        return

    ref, mag = bn_sums(dt, y, cst, act, bs, G)
    # reduce: adds to `red`, pre-filled with known replicas (train) or zero (chain / eval)
    pre = spread(torch.randn(G, 2 * c, generator=torch.Generator().manual_seed(6)).double(), seed=7) \
        if form == "train" else torch.zeros(G, STAT_R, 2 * c)
    red = pre.reshape(-1).contiguous().cuda()
    L.check(lib.isa_bn_bwd_reduce(dts.d(), ys.d(), L.ptr(gp["scale"]), L.ptr(gp["shift"]), L.ptr(gp["mean"]),
                                  L.ptr(gp["invstd"]), act, L.ptr(bsg), L.ptr(red), st), "isa_bn_bwd_reduce")
    torch.cuda.synchronize()
    got = red.view(G, STAT_R, 2 * c).double().cpu().sum(1)
    check_sum(tag + " reduce", got, pre.double().sum(1) + ref, pre.double().abs().sum(1) + mag)
    dts.check_neighbours(tag + " dt")

    # apply: train form from an exact red (spread over the replicas), chain / eval from the kernel's own red
    red_in = spread(ref, seed=8) if form == "train" else red.view(G, STAT_R, 2 * c).cpu()
    red_dev = red_in.reshape(-1).contiguous().cuda()
    red_sum = red_in.double().sum(1)                                      # [G][2c]
    k = torch.stack([ref[:, :c] / count, ref[:, c:] / count], 1)          # float64 [G][2][c]
    if form == "train":
        k = torch.stack([red_sum[:, :c] / count, red_sum[:, c:] / count], 1)
    dgb0 = torch.randn(2, c, generator=torch.Generator().manual_seed(9))
    dgamma, dbeta = dgb0[0].clone().cuda(), dgb0[1].clone().cuda()
    dys = dts if form == "chain" else Slice(L, dt, h, w, dtype, c0=8, groups=G, fill=NAN)
    train = 0 if form == "eval" else 1
    gamma = torch.ones(c, device="cuda")            # not read by the kernel: scale carries gamma * invstd
    L.check(lib.isa_bn_bwd_apply(dts.d(), ys.d(), L.ptr(gp["scale"]), L.ptr(gp["shift"]), L.ptr(gp["mean"]),
                                 L.ptr(gp["invstd"]), act, L.ptr(bsg), L.ptr(gamma), L.ptr(red_dev), count, train,
                                 dys.d(), L.ptr(dgamma), L.ptr(dbeta), st), "isa_bn_bwd_apply")
    torch.cuda.synchronize()
    err = Err()
    for b in range(n):
        g = b // (n // G)
        err.add(dys.get(b), bn_dy(dt[b], y[b], cst, g, act, bs[b] if bs is not None else None, k, train),
                "image %d " % b)
    err.check(tag + " apply dy", store_bound(dtype))
    dys.check_neighbours(tag + " dy")
    ys.check_neighbours(tag + " y")
    # dgamma / dbeta gain exactly one copy of the folded sums per group and channel
    rabs = red_in.double().abs().sum(1)
    check_sum(tag + " dbeta", dbeta, dgb0[1].double() + red_sum[:, :c].sum(0), dgb0[1].double().abs() + rabs[:, :c].sum(0))
    check_sum(tag + " dgamma", dgamma, dgb0[0].double() + red_sum[:, c:].sum(0), dgb0[0].double().abs() + rabs[:, c:].sum(0))

    if form == "eval":       # red = NULL: the same dy, dgamma / dbeta untouched
        dg_before, db_before = dgamma.clone(), dbeta.clone()
        dy2 = Slice(L, dt, h, w, dtype, c0=8, groups=G, fill=NAN)
        L.check(lib.isa_bn_bwd_apply(dts.d(), ys.d(), L.ptr(gp["scale"]), L.ptr(gp["shift"]), L.ptr(gp["mean"]),
                                     L.ptr(gp["invstd"]), act, L.ptr(bsg), L.ptr(gamma), None, count, 0, dy2.d(),
                                     L.ptr(dgamma), L.ptr(dbeta), st), "isa_bn_bwd_apply(eval, no red)")
        torch.cuda.synchronize()
        bits = torch.int16 if dtype == BF else torch.int32
        assert torch.equal(dy2.buf.view(bits), dys.buf.view(bits)), tag + ": eval dy depends on red"
        assert torch.equal(dgamma, dg_before) and torch.equal(dbeta, db_before), tag + ": red = NULL wrote dgamma"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("layer", ["bn", "bn_out"])
def test_engine_eval_bn_backward(dtype, layer):
    """Engine.bn / Engine.bn_out with bn_train=False, record=True: dgamma / dbeta / dx equal float64 autograd of an
    eval-mode BatchNorm2d + ReLU6 (dbeta = sum dz, dgamma = sum dz * xhat from the running statistics)."""
    L, Act, Engine, ParamStore, Pro = _gpu()
    n, c, h, w = 3, 40, 21, 23
    schema = [("bn.weight", (c,)), ("bn.bias", (c,)), ("bn.running_mean", (c,)), ("bn.running_var", (c,)),
              ("bn.num_batches_tracked", ())]
    prm = {"bn.weight": rand(c, seed=11).abs() + 0.5, "bn.bias": rand(c, seed=12),
           "bn.running_mean": rand(c, seed=13) * 0.3, "bn.running_var": rand(c, seed=14).abs() + 0.5}
    ps = ParamStore(schema, "cuda")
    ps.load_state_dict(prm)
    eng = Engine(ps, dtype)
    eng.begin(bn_train=False, record=True)
    ps.grad.zero_()
    x = inp(rand(n, c, h, w, seed=15, scale=2.0), dtype)
    dt = inp(rand(n, c, h, w, seed=16), dtype)
    buf = torch.full((n, h, w, c + 16), NAN, dtype=dtype, device="cuda")
    buf[..., 8:8 + c] = x.permute(0, 2, 3, 1).to(dtype).cuda()
    xa = Act(buf, 8, c)
    if layer == "bn":
        out = eng.bn(xa, None, "bn", L.ACT_RELU6)
    else:
        out = eng.bn_out(xa, None, "bn", L.ACT_RELU6, eng.new_act(n, h, w, c))
    g = eng.grads.grad_of(out if layer == "bn_out" else xa)
    g.buf[..., g.c0:g.c0 + g.c] = dt.permute(0, 2, 3, 1).to(dtype).cuda()
    eng.grads.written[(out if layer == "bn_out" else xa).buf.data_ptr()].append((g.c0, g.c0 + g.c))
    eng.backward()
    torch.cuda.synchronize()
    xt = x.double().requires_grad_(True)
    gamma = prm["bn.weight"].double().requires_grad_(True)
    beta = prm["bn.bias"].double().requires_grad_(True)
    o = F.batch_norm(xt, prm["bn.running_mean"].double(), prm["bn.running_var"].double(), gamma, beta, training=False,
                     eps=Engine.BN_EPS)
    F.hardtanh(o, 0.0, 6.0).backward(dt.double())
    tag = "engine eval %s %s" % (layer, "bf16" if dtype == BF else "f32")
    # dgamma / dbeta are fp32 sums over n*h*w terms: Sum |terms| per channel as the scale
    z = o.detach()
    dz = dt.double() * ((z > 0) & (z < 6)).double()
    xh = (x.double() - prm["bn.running_mean"].double()[:, None, None]) / torch.sqrt(
        prm["bn.running_var"].double()[:, None, None] + Engine.BN_EPS)
    check_sum(tag + " dbeta", ps.gview("bn.bias"), beta.grad, dz.abs().sum((0, 2, 3)))
    check_sum(tag + " dgamma", ps.gview("bn.weight"), gamma.grad, (dz * xh).abs().sum((0, 2, 3)))
    check(tag + " dx", eng.grads.grad_of(xa).nchw(), xt.grad, store_bound(dtype))


# ------------------------------------------------------------------------------------------------ 2. isa_affine_act_res
# name, dtype, n (of x), h, w, C, G, act, parts, fin.  parts: r = res, 2 = res2, o = oscale, b = bscale, B = broadcast
# (x / res hold n images, out G*n).  fin: None, or the finalize's `repeat` (constants from statistics in the call).
# Grid: walk_grid(mkwalk(C, pixels per group)) = grid_cap(cdiv(pixels, 256 >> sh)), cap 2048.
AFF_CASES = [
    # sh = 2, 524288 px: cdiv(524288, 64) = 8192 -> 2048 workgroups, 4 trips
    ("cap2048", BF, 8, 256, 256, 32, 1, "relu6", "rb", None),
    # sh = 1, 589824 px: cdiv(589824, 128) = 4608 -> 2048, 3 trips (the third ragged: 2.25)
    ("cap2048-f32", F32, 9, 256, 256, 16, 1, "leaky", "2o", None),
    # sh = 7 (C = 1024, 2 px per trip), inline finalize with 2 groups, repeat 2
    ("sh7-fin", F32, 4, 8, 9, 1024, 2, "relu6", "rb", 2),
    # C = 1032 > ISA_FIN_MAX_C: sh = 8 (one pixel per trip, 129 of 256 lanes busy) and fin_standalone
    ("c1032-fin", BF, 2, 6, 7, 1032, 1, "relu6", "r", 1),
    ("groups", BF, 6, 33, 35, 40, 3, "leaky", "r2ob", None),
    ("groups-fin", BF, 6, 20, 22, 48, 3, "relu6", "o", 1),
    ("bcast-fin", F32, 2, 24, 20, 64, 3, "relu6", "Br2o", 3),
    ("bcast", BF, 2, 16, 16, 136, 2, "none", "Bro", None),
    ("tanh", F32, 2, 31, 33, 24, 1, "tanh", "", None),
]


def fin_ref(stats, count, gamma, beta, rm, rv, repeat, momentum=0.1, eps=1e-5):
    """isa_bn_finalize in float64: [G][c] scale, shift, mean, invstd and the running statistics after G * repeat updates."""
    s = stats.double().sum(1)                          # [G][2c]
    c = s.shape[1] // 2
    mean = s[:, :c] / count
    var = (s[:, c:] / count - mean * mean).clamp_min(0)
    inv = 1 / torch.sqrt(var + eps)
    scale = gamma.double() * inv
    shift = beta.double() - mean * scale
    rm, rv = rm.double().clone(), rv.double().clone()
    for g in range(s.shape[0]):
        for _ in range(repeat):
            rm = (1 - momentum) * rm + momentum * mean[g]
            rv = (1 - momentum) * rv + momentum * var[g] * count / (count - 1)
    return scale, shift, mean, inv, rm, rv


@pytest.mark.gpu
@pytest.mark.parametrize("case", AFF_CASES, ids=[c[0] for c in AFF_CASES])
def test_affine_act_res(case):
    name, dtype, n, h, w, c, G, act_name, parts, fin = case
    L = _gpu()[0]
    lib = L.lib()
    act = ACTS[act_name]
    P = h * w
    bcast = "B" in parts
    nout = G * n if bcast else n
    gx = 1 if bcast else G                      # statistic groups of x
    x = nhwc(n, P, c, dtype, seed=21, scale=2.0, offset=0.5)
    xs = Slice(L, x, h, w, dtype, c0=8, groups=gx)
    res = nhwc(n, P, c, dtype, seed=22) if "r" in parts else None
    res2 = nhwc(nout, P, c, dtype, seed=23) if "2" in parts else None
    osc = torch.tensor([0.0, 0.5, 1.25, 2.0])[torch.randint(0, 4, (nout, c), generator=torch.Generator().manual_seed(24))] \
        if "o" in parts else None
    bs = (rand(n, c, seed=25) > 0).float() * 2.0 if "b" in parts else None
    keep = []
    gamma, beta = rand(c, seed=26).abs() + 0.5, rand(c, seed=27)
    rm0, rv0 = rand(c, seed=28) * 0.1, rand(c, seed=29).abs() + 0.5
    if fin is None:
        sc, sh = dyadic_pro(c, seed=20, groups=gx)
        scg, shg = sc.reshape(-1).cuda(), sh.reshape(-1).cuda()
        finp = None
    else:
        count = float(n // gx * P)
        sums = torch.stack([torch.cat([x[g * (n // gx):(g + 1) * (n // gx)].double().sum((0, 1)),
                                       (x[g * (n // gx):(g + 1) * (n // gx)].double() ** 2).sum((0, 1))])
                            for g in range(gx)])
        stats = spread(sums, seed=30)
        sc64, sh64, mean64, inv64, rm64, rv64 = fin_ref(stats, count, gamma, beta, rm0, rv0, fin)
        sc, sh = sc64, sh64
        dev = dict(stats=stats.reshape(-1).contiguous().cuda(), gamma=gamma.cuda(), beta=beta.cuda(), rm=rm0.clone().cuda(),
                   rv=rv0.clone().cuda(), scale=torch.full((gx * c,), NAN, device="cuda"),
                   shift=torch.full((gx * c,), NAN, device="cuda"), mean=torch.full((gx * c,), NAN, device="cuda"),
                   invstd=torch.full((gx * c,), NAN, device="cuda"))
        keep.append(dev)
        finp = L.IsaBnFin(L.addr(dev["stats"]), L.addr(dev["gamma"]), L.addr(dev["beta"]), L.addr(dev["rm"]),
                          L.addr(dev["rv"]), L.addr(dev["scale"]), L.addr(dev["shift"]), L.addr(dev["mean"]),
                          L.addr(dev["invstd"]), count, 0.1, 1e-5, fin)
        scg, shg = dev["scale"], dev["shift"]
    bsg = bs.reshape(-1).contiguous().cuda() if bs is not None else None
    pro = L.IsaPro(L.addr(scg), L.addr(shg), L.addr(bsg), act, C.pointer(finp) if finp is not None else None)
    rss = Slice(L, res, h, w, dtype, c0=16) if res is not None else None
    r2s = Slice(L, res2, h, w, dtype, c0=8, groups=G) if res2 is not None else None
    oscg = osc.reshape(-1).contiguous().cuda() if osc is not None else None
    outs = Slice(L, torch.zeros(nout, P, c), h, w, dtype, c0=8, groups=G, fill=NAN)
    L.check(lib.isa_affine_act_res(xs.d(), C.byref(pro), rss.d() if rss else None, r2s.d() if r2s else None, L.ptr(oscg),
                                   outs.d(), L.stream_ptr()), "isa_affine_act_res")
    torch.cuda.synchronize()
    tag = "affine %s %s" % (name, "bf16" if dtype == BF else "f32")
    err = Err()
    for b in range(nout):
        bx = b % n if bcast else b
        g = bx // (n // gx)
        if fin is None:
            z = z_of(x[bx], sc[g], sh[g])
        else:
            z = x[bx].double() * sc[g] + sh[g]
        v = act64(z, act)
        if bs is not None:
            v = v * bs[bx].double()
        if res is not None:
            v = v + res[bx].double()
        if res2 is not None:
            v = v + res2[b].double()
        if osc is not None:
            v = v * osc[b].double()
        err.add(outs.get(b), v, "image %d " % b)
    err.check(tag + " out", store_bound(dtype))
    outs.check_neighbours(tag + " out")
    if fin is not None:
        check(tag + " fin scale", dev["scale"].view(gx, c), sc64, FP32_BOUND)
        check(tag + " fin shift", dev["shift"].view(gx, c), sh64, FP32_BOUND)
        check(tag + " fin mean", dev["mean"].view(gx, c), mean64, FP32_BOUND)
        check(tag + " fin invstd", dev["invstd"].view(gx, c), inv64, FP32_BOUND)
        check(tag + " running_mean", dev["rm"], rm64, FP32_BOUND)
        check(tag + " running_var", dev["rv"], rv64, FP32_BOUND)
        # exactly `repeat` updates per group: one update more or less moves the running mean by ~momentum * |mean|
        _, _, _, _, rm_more, _ = fin_ref(stats, count, gamma, beta, rm0, rv0, fin + 1)
        assert (rm_more - rm64).abs().max() > 100 * FP32_BOUND * rm64.abs().max()


# ------------------------------------------------------------------------------------------------ 3. gradient glue
# isa_axpy: name, dtype, n, h, w, C, c0.  axpy8 needs C % 8 == 0 and 16-byte aligned views; C = 21 or c0 = 3 take the
# scalar axpy_kernel.  Grid: grid_cap(cdiv(items, 256)); "axpy8-long": 8x128x128 px x 8 groups = 1M items -> 2048
# workgroups, 2 trips; "scalar-c21": 4x64x64 px x 21 = 344064 items -> 1344 workgroups, 1 trip.
AXPY_CASES = [("axpy8-long", BF, 8, 128, 128, 64, 8), ("axpy8-f32", F32, 2, 37, 41, 32, 16),
              ("scalar-c21", F32, 4, 64, 64, 21, 8), ("scalar-c21-bf16", BF, 2, 33, 35, 21, 16),
              ("scalar-unaligned", BF, 2, 40, 44, 32, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [-1.5, 0.0])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", AXPY_CASES, ids=[c[0] for c in AXPY_CASES])
def test_axpy(case, accumulate, alpha):
    name, dtype, n, h, w, c, c0 = case
    L = _gpu()[0]
    P = h * w
    src = nhwc(n, P, c, dtype, seed=31)
    dst0 = nhwc(n, P, c, dtype, seed=32)
    ss = Slice(L, src, h, w, dtype, c0=c0, fill=NAN if alpha == 0 else None)      # alpha = 0: the source is never read
    ds = Slice(L, dst0, h, w, dtype, c0=8)
    L.check(L.lib().isa_axpy(ss.d(), ds.d(), alpha, accumulate, L.stream_ptr()), "isa_axpy")
    torch.cuda.synchronize()
    tag = "axpy %s %s acc%d alpha%g" % (name, "bf16" if dtype == BF else "f32", accumulate, alpha)
    if alpha == 0:
        want = dst0.double() if accumulate else torch.zeros(n, P, c, dtype=torch.float64)
        assert torch.equal(ds.get(), want), tag + ": alpha = 0 must be an exact fill / no-op"
    else:
        ref = alpha * src.double() + (dst0.double() if accumulate else 0)
        check(tag, ds.get(), ref, store_bound(dtype))
    ds.check_neighbours(tag)


# isa_scale_bc: name, dtype, n (of dst), h, w, C, fold.  Grid grid_cap(cdiv(n*h*w*cdiv(C, 8), 256)); "f1-long": 4x128x128
# px x 4 = 262144 items -> 1024 workgroups; the tails (C = 21, 44) leave 5 / 4 channels in the last group.
SBC_CASES = [("f1-long", BF, 4, 128, 128, 32, 1), ("f2-tail", F32, 2, 33, 35, 21, 2), ("f3", BF, 2, 20, 24, 136, 3),
             ("f3-tail", F32, 3, 17, 19, 44, 3), ("f2-tail-bf16", BF, 2, 30, 31, 21, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", SBC_CASES, ids=[c[0] for c in SBC_CASES])
def test_scale_bc(case, accumulate):
    name, dtype, n, h, w, c, fold = case
    L = _gpu()[0]
    P = h * w
    src = nhwc(fold * n, P, c, dtype, seed=41)
    dst0 = nhwc(n, P, c, dtype, seed=42)
    s = torch.tensor([0.0, 0.5, 1.25, 2.0])[torch.randint(0, 4, (fold * n, c), generator=torch.Generator().manual_seed(43))]
    ss = Slice(L, src, h, w, dtype, c0=16)
    ds = Slice(L, dst0, h, w, dtype, c0=8)
    sg = s.reshape(-1).contiguous().cuda()
    L.check(L.lib().isa_scale_bc(ss.d(), L.ptr(sg), ds.d(), accumulate, L.stream_ptr()), "isa_scale_bc")
    torch.cuda.synchronize()
    ref = sum(src[g * n:(g + 1) * n].double() * s[g * n:(g + 1) * n, None, :].double() for g in range(fold))
    if accumulate:
        ref = ref + dst0.double()
    tag = "scale_bc %s %s acc%d" % (name, "bf16" if dtype == BF else "f32", accumulate)
    check(tag, ds.get(), ref, store_bound(dtype))
    ds.check_neighbours(tag)


# isa_avgpool2 / _bwd: name, dtype, n, hs, ws (small side), C.  Grid grid_cap(cdiv(n*hs*ws*C/8, 256)): 8x128x128 x 6 =
# 786432 items -> 2048 workgroups, 1.5 trips; 8x128x128 x 5 = 655360 -> 2048, 1.25 trips.  Outputs go into a slice, as
# Network.unet writes the pooled skip into its concat buffer.
POOL_CASES = [("bf16-long", BF, 8, 128, 128, 48), ("f32-long", F32, 8, 128, 128, 40), ("small", F32, 2, 7, 9, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", POOL_CASES, ids=[c[0] for c in POOL_CASES])
def test_avgpool2(case):
    name, dtype, n, hs, ws, c = case
    L = _gpu()[0]
    lib = L.lib()
    tag = "avgpool2 %s" % name
    x = nhwc(n, 4 * hs * ws, c, dtype, seed=51)
    xs = Slice(L, x, 2 * hs, 2 * ws, dtype, c0=16)
    ys = Slice(L, torch.zeros(n, hs * ws, c), hs, ws, dtype, c0=8, fill=NAN)
    L.check(lib.isa_avgpool2(xs.d(), ys.d(), L.stream_ptr()), "isa_avgpool2")
    torch.cuda.synchronize()
    x4 = x.double().view(n, 2 * hs, 2 * ws, c).permute(0, 3, 1, 2)
    ref = F.avg_pool2d(x4, 2).permute(0, 2, 3, 1).reshape(n, hs * ws, c)
    check(tag + " fwd", ys.get(), ref, store_bound(dtype))
    ys.check_neighbours(tag + " fwd")
    # backward: dx (+)= dy / 4 on every pixel of the 2x2 window
    dy = nhwc(n, hs * ws, c, dtype, seed=52)
    dys = Slice(L, dy, hs, ws, dtype, c0=8)
    for acc in (0, 1):
        old = nhwc(n, 4 * hs * ws, c, dtype, seed=53)
        dxs = Slice(L, old, 2 * hs, 2 * ws, dtype, c0=8, fill=None if acc else NAN)
        L.check(lib.isa_avgpool2_bwd(dys.d(), dxs.d(), acc, L.stream_ptr()), "isa_avgpool2_bwd")
        torch.cuda.synchronize()
        d4 = dy.double().view(n, hs, ws, c).permute(0, 3, 1, 2)
        ref = (F.interpolate(d4, scale_factor=2, mode="nearest") / 4).permute(0, 2, 3, 1).reshape(n, 4 * hs * ws, c)
        if acc:
            ref = ref + old.double()
        check(tag + " bwd acc%d" % acc, dxs.get(), ref, store_bound(dtype))
        dxs.check_neighbours(tag + " bwd")


# isa_avgpool3 (3x3 mean, stride 1, zero border, optional per-pixel mask, optional accumulate): C = 16 takes the 8-channel
# vector kernel, C = 20 the per-element kernel that the head's 24-channel tensors never reach.  2x7x9 pixels.
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("c", [16, 20])
def test_avgpool3(c, dtype):
    L = _gpu()[0]
    n, h, w = 2, 7, 9
    x = nhwc(n, h * w, c, dtype, seed=54)
    m = inp((rand(n, h * w, 1, seed=55) > 0).float() * 1.5, dtype)
    old = nhwc(n, h * w, c, dtype, seed=56)
    xs, ms = Slice(L, x, h, w, dtype, c0=8), Slice(L, m, h, w, dtype, c0=8)
    x4 = x.double().view(n, h, w, c).permute(0, 3, 1, 2)
    mean = F.avg_pool2d(x4, 3, 1, 1).permute(0, 2, 3, 1).reshape(n, h * w, c)       # zero border, always / 9
    for mask in (False, True):
        for acc in (0, 1):
            ys = Slice(L, old, h, w, dtype, c0=8, fill=None if acc else NAN)
            L.check(L.lib().isa_avgpool3(xs.d(), ms.d() if mask else None, ys.d(), acc, L.stream_ptr()), "isa_avgpool3")
            torch.cuda.synchronize()
            ref = mean * m.double() if mask else mean
            if acc:
                ref = ref + old.double()
            tag = "avgpool3 c%d %s mask%d acc%d" % (c, "bf16" if dtype == BF else "f32", mask, acc)
            check(tag, ys.get(), ref, store_bound(dtype))
            ys.check_neighbours(tag)


# ------------------------------------------------------------------------------------------------ 4. squeeze-excite
# isa_chan_mean: name, dtype, n, h, w, C, G, prologue act (None: no prologue), bscale.  Grid (grid_cap(cdiv(hw*cg, 256),
# 128), n): "prod" 256x256 x 4 groups -> 128 workgroups per image, stride 32768 % 4 == 0: a lane keeps its channel
# group for 8 trips; "cg3-flush": 128x128 x 3 = 49152 items -> 128 workgroups, stride 32768 % 3 = 2, so a lane changes
# channel group between its trips and the last_c0 flush runs; "cg5-G2-bs": 100x101 x 5 = 50500 items, stride % 5 = 3.
CM_CASES = [("prod", BF, 8, 256, 256, 32, 1, None, False), ("cg3-flush", F32, 3, 128, 128, 24, 1, "relu6", False),
            ("cg5-G2-bs", BF, 4, 100, 101, 40, 2, "leaky", True), ("G3-bs", F32, 6, 40, 44, 64, 3, "relu6", True),
            ("bs-only", F32, 2, 30, 30, 16, 1, None, True)]


def chan_mean_ref(x, sc, sh, act, bs, G, hw):
    """[n][c] sum_p act(scale*x + shift) * bscale / hw, and the sums of |terms|."""
    n = x.shape[0]
    s, a = [], []
    for b in range(n):
        g = b // (n // G)
        t = act64(z_of(x[b], sc[g], sh[g]), act) if sc is not None else x[b].double()
        if bs is not None:
            t = t * bs[b].double()
        s.append(t.sum(0) / hw)
        a.append(t.abs().sum(0) / hw)
    return torch.stack(s), torch.stack(a)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CM_CASES, ids=[c[0] for c in CM_CASES])
def test_chan_mean(case):
    name, dtype, n, h, w, c, G, act_name, bscale = case
    L = _gpu()[0]
    P = h * w
    x = nhwc(n, P, c, dtype, seed=61, scale=2.0, offset=0.5)
    xs = Slice(L, x, h, w, dtype, c0=16, groups=G)
    sc = sh = None
    act = ACTS[act_name or "none"]
    if act_name is not None:
        sc, sh = dyadic_pro(c, seed=62, groups=G)
    bs = (rand(n, c, seed=63) > 0).float() * 2.0 if bscale else None
    keep = [t.reshape(-1).contiguous().cuda() if t is not None else None for t in (sc, sh, bs)]
    pro = L.IsaPro(L.addr(keep[0]), L.addr(keep[1]), L.addr(keep[2]), act, None)
    pre = rand(n, c, seed=64)
    out = pre.clone().cuda()                                  # the kernel adds to it
    L.check(L.lib().isa_chan_mean(xs.d(), C.byref(pro), L.ptr(out), L.stream_ptr()), "isa_chan_mean")
    torch.cuda.synchronize()
    ref, mag = chan_mean_ref(x, sc, sh, act, bs, G, P)
    check_sum("chan_mean %s" % name, out, pre.double() + ref, pre.double().abs() + mag)
    xs.check_neighbours("chan_mean %s" % name)


@pytest.mark.gpu
@pytest.mark.parametrize("n,c,hidden", [(4, 32, 16), (3, 200, 80)])
def test_se_fc(n, c, hidden):
    """gate = sigmoid(W2 relu(W1 m + b1) + b2): one 64-thread workgroup per image, c and hidden above 64 in the second case."""
    L = _gpu()[0]
    m = rand(n, c, seed=71)
    w1, b1 = rand(hidden, c, seed=72, scale=c ** -0.5), rand(hidden, seed=73)
    w2, b2 = rand(c, hidden, seed=74, scale=hidden ** -0.5), rand(c, seed=75)
    dev = [t.contiguous().cuda() for t in (m, w1, b1, w2, b2)]
    hid = torch.full((n, hidden), NAN, device="cuda")
    gate = torch.full((n, c), NAN, device="cuda")
    L.check(L.lib().isa_se_fc(*[L.ptr(t) for t in dev], n, c, hidden, L.ptr(hid), L.ptr(gate), L.stream_ptr()), "isa_se_fc")
    torch.cuda.synchronize()
    a1 = m.double() @ w1.double().T + b1.double()
    mag = (m.double().abs() @ w1.double().abs().T + b1.double().abs())
    h64 = a1.clamp_min(0)
    check_sum("se_fc c%d hidden" % c, hid, h64, mag)
    check("se_fc c%d gate" % c, gate, torch.sigmoid(h64 @ w2.double().T + b2.double()), FP32_BOUND)


def se_bwd_ref(x, dxa, w1, b1, w2, b2, hw):
    """float64 autograd of y = x * sigmoid(W2 relu(W1 mean(x) + b1) + b2) for dy = dxa; x, dxa [n, P, c].  Also the
    magnitudes of the expanded sums (the same backward on absolute values) and the forward values the kernel reads."""
    xt = x.double().requires_grad_(True)
    W1, B1, W2, B2 = (t.double().requires_grad_(True) for t in (w1, b1, w2, b2))
    m = xt.mean(1)
    m.retain_grad()
    hdn = torch.relu(m @ W1.T + B1)
    gate = torch.sigmoid(hdn @ W2.T + B2)
    (xt * gate[:, None, :]).backward(dxa.double())
    with torch.no_grad():
        prod = dxa.double() * x.double()
        dg = prod.sum(1)
        dg_abs = prod.abs_().sum(1)
        del prod
        gg = gate * (1 - gate)
        da_abs = dg_abs * gg
        dh_abs = (da_abs @ W2.abs()) * (hdn > 0).double()
        mags = dict(dg=dg_abs, dw2=da_abs.T @ hdn.abs(), db2=da_abs.sum(0), dw1=dh_abs.T @ m.abs(), db1=dh_abs.sum(0),
                    dmean=dh_abs @ W1.abs())
    grads = dict(dg=dg, dw1=W1.grad, db1=B1.grad, dw2=W2.grad, db2=B2.grad, dmean=m.grad, dx=xt.grad)
    fwd = dict(mean=m.detach().float(), hid=hdn.detach().float(), gate=gate.detach().float())
    return grads, mags, fwd


SE_CASES = [("prod", BF, 8, 256, 256, 32, 16, 0), ("ragged", F32, 3, 37, 41, 40, 10, 1), ("ragged-bf16", BF, 2, 45, 39, 24, 16, 1),
            ("prod-f32-acc", F32, 2, 128, 128, 32, 16, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SE_CASES, ids=[c[0] for c in SE_CASES])
def test_se_bwd(case):
    name, dtype, n, h, w, c, hidden, acc = case
    L = _gpu()[0]
    P = h * w
    x = nhwc(n, P, c, dtype, seed=81, scale=2.0, offset=0.5)
    dxa = nhwc(n, P, c, dtype, seed=82)
    w1, b1 = rand(hidden, c, seed=83, scale=c ** -0.5), rand(hidden, seed=84)
    w2, b2 = rand(c, hidden, seed=85, scale=hidden ** -0.5), rand(c, seed=86)
    grads, mags, fwd = se_bwd_ref(x, dxa, w1, b1, w2, b2, P)
    xs = Slice(L, x, h, w, dtype, c0=8)
    das = Slice(L, dxa, h, w, dtype, c0=16)
    old = nhwc(n, P, c, dtype, seed=87)
    dxs = Slice(L, old, h, w, dtype, c0=8, fill=None if acc else NAN)
    gate, hid, mean = (fwd[k].contiguous().cuda() for k in ("gate", "hid", "mean"))
    W1, W2 = w1.contiguous().cuda(), w2.contiguous().cuda()
    pre = {k: rand(*s, seed=88 + i) for i, (k, s) in enumerate((("dw1", (hidden, c)), ("db1", (hidden,)),
                                                                 ("dw2", (c, hidden)), ("db2", (c,))))}
    outs = {k: v.clone().cuda() for k, v in pre.items()}
    dg = torch.zeros(n, c, device="cuda")
    dmean = torch.full((n, c), NAN, device="cuda")
    L.check(L.lib().isa_se_bwd(das.d(), xs.d(), L.ptr(gate), L.ptr(hid), L.ptr(mean), L.ptr(W1), L.ptr(W2), hidden,
                               L.ptr(dg), L.ptr(dmean), L.ptr(outs["dw1"]), L.ptr(outs["db1"]), L.ptr(outs["dw2"]),
                               L.ptr(outs["db2"]), dxs.d(), acc, L.stream_ptr()), "isa_se_bwd")
    torch.cuda.synchronize()
    tag = "se_bwd %s" % name
    check_sum(tag + " dgate", dg, grads["dg"], mags["dg"])
    check_sum(tag + " dmean", dmean, grads["dmean"], mags["dmean"])
    for k in ("dw1", "db1", "dw2", "db2"):
        check_sum(tag + " " + k, outs[k], pre[k].double() + grads[k], pre[k].double().abs() + mags[k])
    ref = grads["dx"] + (old.double() if acc else 0)
    check(tag + " dx acc%d" % acc, dxs.get(), ref, store_bound(dtype))
    dxs.check_neighbours(tag + " dx")


# ------------------------------------------------------------------------------------------------ 5. optimizer
# n = 600001: isa_sqnorm's grid is capped at 1024 workgroups (stride 262144, 2.3 trips), isa_adadelta's at 2048 (stride
# 524288, 1.1 trips); both end in a ragged trip.  name, max_norm, gscale, lr_dev, wd, clip engaged on every step
OPT_CASES = [("clip-on", 1.0, 1.0, None, 0.0, True), ("clip-off", 100.0, 1.0, None, 0.0, False),
             ("no-clip-gscale", 0.0, 0.5, None, 0.0, False), ("lr-dev-wd-clip", 2.0, 0.25, 0.3, 1e-3, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", OPT_CASES, ids=[c[0] for c in OPT_CASES])
def test_optimizer(case):
    name, max_norm, gscale, lr_dev, wd, engaged = case
    L = _gpu()[0]
    lib = L.lib()
    N = 600001
    lr, rho, eps = 1.0, 0.9, 1e-6
    p0 = rand(N, seed=91, scale=0.01)       # |p| small: its fp32 rounding (ulp / 2) stays far below the updates
    p = p0.clone().cuda()
    sq, acc = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    lrd = torch.tensor([lr_dev], device="cuda") if lr_dev is not None else None
    pr = p0.double().clone().requires_grad_(True)
    opt = torch.optim.Adadelta([pr], lr=lr_dev if lr_dev is not None else lr, rho=rho, eps=eps, weight_decay=wd)
    for step in range(3):
        g = rand(N, seed=92 + step, scale=0.02)
        gd = g.cuda()
        sqn = torch.zeros(1, device="cuda")
        p_before = p.double().cpu()
        L.check(lib.isa_sqnorm(L.ptr(gd), N, gscale, L.ptr(sqn), L.stream_ptr()), "isa_sqnorm")
        L.check(lib.isa_adadelta(L.ptr(p), L.ptr(gd), L.ptr(sq), L.ptr(acc), N, lr, rho, eps, wd, L.ptr(sqn), max_norm,
                                 gscale, L.ptr(lrd), L.stream_ptr()), "isa_adadelta")
        torch.cuda.synchronize()
        gs = g.double() * gscale
        tag = "opt %s step %d" % (name, step)
        check_sum(tag + " sqnorm", sqn[0], (gs * gs).sum(), (gs * gs).sum())
        pr_before = pr.detach().clone()
        pr.grad = gs.clone()
        if max_norm > 0:
            total = torch.nn.utils.clip_grad_norm_([pr], max_norm)
            assert (float(max_norm / (total + 1e-6)) < 1) == engaged, (tag, float(total))
        opt.step()
        check(tag + " update", p.double().cpu() - p_before, pr.detach() - pr_before, OPT_UPDATE_BOUND)
        st = opt.state[pr]
        check(tag + " square_avg", sq, st["square_avg"], FP32_BOUND)
        check(tag + " acc_delta", acc, st["acc_delta"], FP32_BOUND)
    check("opt %s params" % name, p, pr.detach(), FP32_BOUND)


# ------------------------------------------------------------------------------------------------ 6. the bounds catch bugs
def test_stated_grids_match_the_launch_code():
    """The walks BN_CASES claim follow from bn_bwd_common (mirrored in bn_bwd_grid), and the cases reach the reduce
    pass's narrow 1024 and wide 128 caps with >= 4 ragged trips, the apply pass's 512 cap and the grid-1 small end."""
    for case in BN_CASES:
        if len(case) < 11:
            continue
        name, _, n, h, w, c, G = case[:7]
        for which, stated in case[10].items():
            assert bn_bwd_grid(c, n // G * h * w, which == "apply") == stated, (name, which)
    walks = [(c[5], c[2] // c[6] * c[3] * c[4]) for c in BN_CASES if len(c) > 10]

    def ragged(C_, px, apply):
        return px % (bn_bwd_grid(C_, px, apply)[0] * bn_ppb(C_)) != 0
    assert any(bn_bwd_grid(C_, px, False)[0] == 1024 and bn_bwd_grid(C_, px, False)[2] >= 4 and ragged(C_, px, False)
               for C_, px in walks)
    assert any(C_ > 128 and bn_bwd_grid(C_, px, False)[0] == 128 and bn_bwd_grid(C_, px, False)[2] >= 4
               and ragged(C_, px, False) for C_, px in walks)
    assert any(C_ > 128 and bn_bwd_grid(C_, px, True)[0] == 512 for C_, px in walks)
    assert any(bn_bwd_grid(C_, px, False)[0] == 1 for C_, px in walks)


def test_streaming_bounds_reject_bugs():
    """The float64 references of this file, re-run with one plausible kernel bug each, must miss their bound by a wide
    margin (>= 10x): a dropped replica of red, group 0's constants used for group 1, bscale of the wrong image, the
    sum-dz term missing from apply, the last ragged trip skipped, and a tail channel written past c."""
    margin = 10

    def reject(what, e, bound):
        print("MUTATION %-32s %.3e = %.0fx its bound" % (what, e, e / bound))
        assert e > margin * bound, (what, e)
    # a G = 2 BatchNorm backward with bscale, C = 21 (tail group), 2 images of 17x19 = 646 px per group: iters 2,
    # grid 6 per group, 384 px per trip of the grid; the second (last) trip is ragged
    case = ("mut", BF, 4, 17, 19, 21, 2, "relu6", True, "train")
    dtype, n, h, w, c, G, act, form, dt, y, cst, bs = bn_inputs(case)
    P = h * w
    count = float(n // G * P)
    ref, mag = bn_sums(dt, y, cst, act, bs, G)
    # 1. one replica of red dropped
    reps = spread(ref, seed=8).double()
    e, _ = sum_err(reps[:, 1:].sum(1), ref, mag)
    reject("replica dropped", e, SUM_BOUND)
    # 2. group 0's constants for group 1
    cst_bad = {k: v.clone() for k, v in cst.items()}
    for k in cst_bad:
        cst_bad[k][1] = cst[k][0]
    e, _ = sum_err(bn_sums(dt, y, cst_bad, act, bs, G)[0], ref, mag)
    reject("group 0 constants", e, SUM_BOUND)
    # 3. bscale of the wrong image
    e, _ = sum_err(bn_sums(dt, y, cst, act, bs.roll(1, 0), G)[0], ref, mag)
    reject("bscale of the wrong image", e, SUM_BOUND)
    # 4. the sum-dz term missing from apply (the loosest store bound)
    k = torch.stack([ref[:, :c] / count, ref[:, c:] / count], 1)
    k_bad = k.clone()
    k_bad[:, 0] = 0
    err = Err()
    for b in range(n):
        g = b // (n // G)
        err.add(bn_dy(dt[b], y[b], cst, g, act, bs[b], k_bad, True), bn_dy(dt[b], y[b], cst, g, act, bs[b], k, True))
    reject("sum dz dropped", err.value(), BF16_STORE)
    # 5. the last ragged trip skipped: trips cover [0, 384) and [384, 646) of each group; drop the second
    grid, _, trips = bn_bwd_grid(c, n // G * P, False)
    assert (grid, trips) == (6, 2)
    step = grid * bn_ppb(c)
    e, _ = sum_err(bn_sums(dt, y, cst, act, bs, G, skip=lambda b: (torch.arange(P) + (b % (n // G)) * P) >= step)[0],
                   ref, mag)
    reject("last trip skipped", e, SUM_BOUND)
    # 6. a tail channel written past c: neighbours no longer bit-unchanged
    buf = torch.full((2, 3, 4, 40), NAN, dtype=BF)
    buf[..., 8:29] = 1.0
    orig = buf.clone()
    assert neighbours_equal(buf, orig, 8, c)
    buf[..., 29] = 0.5
    assert not neighbours_equal(buf, orig, 8, c)
    # and a clean reference passes the tightest bound
    assert sum_err(reps.sum(1), ref, mag)[0] < SUM_BOUND
