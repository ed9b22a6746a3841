"""Dense 3x3, transposed-conv and channel-map paths of the conv GEMM family against float64.

test_gpu_backbone_walk.py pins the 1x1 GEMM and the depthwise kernels over long tile walks.  This file does the same for
what that file leaves: isa_pack_weights (all six layouts, with channel maps), isa_conv_gemm in its ISA_IN_3X3,
ISA_IN_GATHER2 and ISA_OUT_SHUFFLE2 forms with chunked weights over more than one 128-pixel tile, `accumulate = 1` in
both epilogue store paths, the two conv3x3_tiled.hip kernels at the head's channel counts, isa_conv_wgrad with a channel
map (`kmap`, `ksrc`) and for ConvTranspose2d at real widths, and the argument refusals of those forms.

Method (the walk file's, whose helpers are imported): float64 CPU reference from the exact operands the kernel sees;
inputs are values of the storage type; prologue constants are dyadic; the kernels' rounding points are emulated (`rs` on
the MFMA operand after the prologue and on the stored output, with `accumulate = 1` the stored value is
rs(old + result)); outputs are NaN-filled before the call and everything around an output slice is a known pattern that
must be bit-equal afterwards; error = max |got - ref| / max |ref| with the worst element named.  Entry points are called
through ctypes; weights are packed by isa_pack_weights itself through engine.Packer.

Operands of the bf16 GEMM cases lie on a dyadic grid on which the whole contraction is exact in fp32: x multiples of
1/4 in [-2, 2], prologue scale in {0.5 .. 1.5} and shift k/8 (so the operand after ReLU6 and the 0 / 2 per-image
multiplier is a multiple of 1/16 below 16: a bf16 value), weights multiples of 1/8 in [-1/4, 1/4], bias and the old
output multiples of 1/8.  Every product is a multiple of 2**-7 below 4 and a sum of up to 4608 of them needs 22 bits, so
fp32 accumulation gives the float64 sum in any order and the stored bf16 value must equal rs(reference) bit for bit.
With full-precision operands it cannot: where the fp32 and the float64 sum fall on different sides of a bf16 rounding
boundary the stored value is one ulp off, 2**-7 of max |ref| for an element in the top binade - twice BF16_STORE - and
among 10**7 outputs some element does (measured on the 3x3 data gradient 128->256 with accumulate: got -8.0625 for
-8, 5.0e-3).  The fp32 cases keep full-precision operands (a bf16 rounding anywhere on an fp32 path shows at ~1e-3).

Every GEMM case carries its tile arithmetic (`plan`), and test_plans_match_launch_code recomputes it from a Python
restatement of launch0 / conv_gemm_impl / conv3x3_tiled_launch (conv_gemm.hip, conv3x3_tiled.hip), so a comment cannot
drift from the shape.  Weight-gradient cases name dispatch_wg's tiles per wave and grid (wgrad_tiles of the walk file).

Bounds (none derived from a measured value):
  * FP32_BOUND = 1e-5 (walk file) for fp32-stored outputs, dW, db and statistics.  It may be used on a case only while the
    same operation evaluated on the CPU in float32 (torch, another summation order) stays within FLOOR = 1e-6 of the
    float64 reference in the same metric, so the bound keeps 10x over the summation-order floor of the reference itself:
    test_fp32_floor_gemm / test_fp32_floor_wgrad assert that for every case of the tables below, without a GPU (the
    weight-gradient floor is evaluated as float32 matrix products per tap; torch's own float32 conv backward on the CPU
    adds pixel by pixel and is at 2.6e-6 for ConvT 512->256).  CPU floors measured: fp32 GEMM cases 1.4e-7 .. 4.8e-7
    (3x3 data gradient 32->64), their statistics 6.8e-8; bf16 GEMM cases 0 (exact grid), statistics 6.8e-8; dW 1.1e-7 ..
    2.9e-7 (ConvT 512->256: 2.2e-7 fp32, 1.1e-7 bf16), db 1.4e-7.
  * BF16_STORE = 2**-8 (walk file) for bf16-stored outputs.
  * isa_pack_weights: bit equality.
Worst error measured on MI355X per entry point (fp32 / bf16 storage):
  isa_conv_gemm y: ConvT forward 2.9e-7 / 0, ConvT data gradient 8.6e-7 / 0, 3x3 forward 9.8e-7 / 0, 3x3 data gradient
  8.0e-7 / 0 (bf16 1- and 2-channel cases on conv3x3_tiled: 0), element-path stores 1.9e-7 / 0; statistics sum 4.5e-8 /
  5.1e-8, sum of squares 8.3e-8 / 7.2e-8.  conv3x3_tiled forward (bf16) 0.
  isa_conv_wgrad: 1x1 with a map dW 6.6e-7 / 2.1e-7, db 4.0e-7 / 9.7e-8; 3x3 with a map dW 5.4e-7 / 2.0e-7; ConvT dW
  6.2e-7 / 2.5e-7, db 4.1e-7 / 1.5e-7; conv3x3_wgrad_tiled (bf16) dW 1.9e-7, db 6.5e-8.

The file runs in about 25 s on one MI355X.
"""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from test_gpu_ops import _gpu, rand  # noqa: E402
from test_gpu_backbone_walk import (BF, BF16_STORE, F32, FP32_BOUND, STAT_R, check, dyadic_pro, inp, nan_ws,  # noqa: E402
                                    pro_f32, rs, run_ws_call, stat_sums, store_bound, walk_err, wgrad_set_floats,
                                    wgrad_tiles)

FLOOR = 1e-6             # float32-vs-float64 floor of a reference that FP32_BOUND may be used on
POISON = -3.0            # what surrounds an output slice; must be bit-equal after the call
NAN = float("nan")


class A:                 # ISA_ACT_* of include/isa_kernels.h (the CPU-only tests do not load the library)
    ACT_NONE, ACT_RELU, ACT_RELU6, ACT_LEAKY = 0, 1, 2, 3


ACTS = {"none": A.ACT_NONE, "relu": A.ACT_RELU, "relu6": A.ACT_RELU6, "leaky": A.ACT_LEAKY}


def rup(x, m):
    return (x + m - 1) // m * m


def tname(dtype):
    return "bf16" if dtype == BF else "f32"


def pro32(x, sc, sh, act, bs=None):
    """The prologue act(scale * x + shift) * bscale in float32 (pro_f32 of the walk file, plus ISA_ACT_RELU)."""
    if act == A.ACT_RELU:
        t = (x.float() * sc[0][None, :, None, None] + sh[0][None, :, None, None]).clamp_min(0)
        return t if bs is None else t * bs[:, :, None, None]
    return pro_f32(x, sc, sh, act, A, bs)


def nhwc(t, dtype, ld=None, c0=0, fill=NAN):
    """NCHW CPU tensor -> NHWC device buffer [n, h, w, ld] holding it at channel offset c0; every other lane = fill."""
    n, c, h, w = t.shape
    ld = ld or rup(c, 8)
    buf = torch.full((n, h, w, ld), fill, dtype=dtype, device="cuda")
    buf[..., c0:c0 + c] = t.permute(0, 2, 3, 1).to(dtype).cuda()
    return buf


def packed(ParamStore, Packer, wt, dtype, kind, n, k, taps, kp, rows, kmap=None):
    """wt in state_dict layout, packed by isa_pack_weights: (packer, key); packer.ptr(key) is the device pointer."""
    ps = ParamStore([("w", tuple(wt.shape))], "cuda")
    ps.load_state_dict({"w": wt})
    pk = Packer(ps, dtype)
    key = pk.add("w", "v", kind, n, k, taps, kp, rows, kmap)
    pk.pack()
    return pk, key


# ------------------------------------------------------------------------------------------------ channel maps
def decoder_map(out_ch, naux):
    """instance_head.py: physical [gated(out_ch) | cross | aux] -> source [cross | gated | aux], ccross = out_ch - naux."""
    ccross = out_ch - naux
    return [ccross + k for k in range(out_ch)] + list(range(ccross)) + [ccross + out_ch + k for k in range(naux)]


def holes_map(kphys, ksrc, seed):
    """kphys physical channels, -1 (padding) scattered through the middle, the others a permutation of all source channels
    but the last one (which therefore receives no gradient and contributes no weight)."""
    g = torch.Generator().manual_seed(seed)
    pos = torch.randperm(kphys, generator=g)[:ksrc - 1].tolist()
    src = torch.randperm(ksrc - 1, generator=g).tolist()
    km = [-1] * kphys
    for p, s in zip(pos, src):
        km[p] = s
    return km


def to_source_order(x_phys, kmap, ksrc):
    """x_src[:, kmap[kd]] = x_phys[:, kd]: the tensor the reference's conv sees."""
    n, _, h, w = x_phys.shape
    xs = torch.zeros(n, ksrc, h, w, dtype=x_phys.dtype)
    for kd, k in enumerate(kmap):
        if k >= 0:
            xs[:, k] = x_phys[:, kd]
    return xs


# ------------------------------------------------------------------------------------------------ 1. isa_pack_weights
def pack_ref(src, kind, n, k, taps, kp, rows, kmap):
    """The layouts documented at isa_pack_entry (include/isa_kernels.h), fp32.  kmap: per destination channel of the K
    axis (kinds 0, 2: contraction index; 1, 3: row; 4, 5: column) the source channel or -1; None = identity."""
    km = list(range(n if kind >= 4 else k)) if kmap is None else list(kmap)
    if kind in (0, 1):
        s = src.reshape(n, k, taps)
        out = torch.zeros(rows, taps, kp)
        for kd, kk in enumerate(km):
            if kk < 0:
                continue
            if kind == 0:                       # dst[N][taps][kp]
                out[:, :, kd] = s[:, kk, :]
            else:                               # dst[Kphys][taps flipped][kp >= N]
                out[kd, :, :n] = s[:, kk, :].flip(-1).t()
    elif kind in (2, 3):
        s = src.reshape(k, n, 4)                # [K][Co][2*2]
        out = torch.zeros(rows, kp) if kind == 2 else torch.zeros(rows, 4, kp)
        for kd, kk in enumerate(km):
            if kk < 0:
                continue
            if kind == 2:                       # dst[4*Co][kp], row = quadrant * Co + co
                out[:, kd] = s[kk].t().reshape(-1)
            else:                               # dst[Kphys][4][kp >= Co]
                out[kd, :, :n] = s[kk].t()
    else:
        s = src.reshape(n, 9)                   # depthwise [C][1][3][3] -> dst[9][rows]
        out = torch.zeros(9, rows)
        for cd, kk in enumerate(km):
            if kk >= 0:
                out[:, cd] = s[kk].flip(-1) if kind == 5 else s[kk]
    return out.reshape(-1)


def pack_table():
    """(source name, source shape, kind, n, k, taps, kp, rows, kmap): every kind with identity, the decoder's permutation
    and a map with -1 entries and more entries than source channels.  n = 21, k = 246 / 46: no multiples of 32."""
    perm246, perm46 = decoder_map(123, 6), decoder_map(23, 3)            # 123 + 117 + 6 = 246; 23 + 20 + 3 = 46
    holes246, holes46 = holes_map(270, 246, 8), holes_map(61, 46, 9)
    t = []
    for tag, km246, km46 in (("id", None, None), ("perm", perm246, perm46), ("holes", holes246, holes46)):
        l246, l46 = (246 if km246 is None else len(km246)), (46 if km46 is None else len(km46))
        taps = 1 if tag == "id" else 9
        # kind 0: [N][taps][kp], kp = rup(len, 32) (+32 once: kp > k by more than the rounding)
        t.append(("c%d" % taps, (21, 246, taps), 0, 21, 246, taps, rup(l246, 32) + (32 if tag == "perm" else 0), 21, km246))
        # kind 1: [Kphys][taps flipped][kp = 32 > 21]
        taps1 = 9 if tag != "perm" else 1
        t.append(("c%d" % taps1, (21, 246, taps1), 1, 21, 246, taps1, 32, l246, km246))
        # kinds 2, 3: ConvTranspose2d [K = 46][Co = 21][2][2], taps 4
        t.append(("t", (46, 21, 2, 2), 2, 21, 46, 4, rup(l46, 32), 4 * 21, km46))
        t.append(("t", (46, 21, 2, 2), 3, 21, 46, 4, 32, l46, km46))
        # kinds 4, 5: depthwise [C = 46][1][3][3] -> [9][rows = rup(len, 8)]
        t.append(("d", (46, 1, 3, 3), 4, 46, 1, 9, 0, rup(l46, 8), km46))
        t.append(("d", (46, 1, 3, 3), 5, 46, 1, 9, 0, rup(l46, 8), km46))
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF], ids=tname)
def test_pack_weights_all_kinds(dtype):
    """One isa_pack_weights launch over 18 entries (six kinds x identity / permutation / map with holes) into a NaN-filled
    buffer, entries separated by guards of different lengths: every entry bit-equal to the documented layout (bf16 =
    .to(bfloat16) of the fp32 value), padding exactly +0, every guard still NaN."""
    L, Act, Engine, ParamStore, Pro = _gpu()
    from isa_amd.engine import Packer
    table = pack_table()
    srcs = {}
    for name, shape, *_ in table:
        if name not in srcs:
            srcs[name] = rand(*shape, seed=100 + len(srcs))
    ps = ParamStore([(nm, tuple(s.shape)) for nm, s in srcs.items()], "cuda")
    ps.load_state_dict(srcs)
    pk = Packer(ps, dtype)
    for i, (name, shape, kind, n, k, taps, kp, rows, kmap) in enumerate(table):
        pk.add(name, "v%d" % i, kind, n, k, taps, kp, rows, kmap)
    off = 48                                              # a guard in front of the first entry too
    for i, e in enumerate(pk.entries):                    # non-contiguous destinations: an overrun lands in a guard
        e["dst_off"] = off
        off += rup(e["size"], 16) + 16 * (1 + i % 3)
    pk.total = off
    pk.finalize()
    pk.buf.fill_(NAN)
    pk.pack()
    torch.cuda.synchronize()
    exp = torch.full((pk.buf.numel(),), NAN, dtype=dtype)
    for e, (name, shape, kind, n, k, taps, kp, rows, kmap) in zip(pk.entries, table):
        r = pack_ref(srcs[name], kind, n, k, taps, kp, rows, kmap)
        assert r.numel() == e["size"]
        exp[e["dst_off"]:e["dst_off"] + e["size"]] = r.to(dtype)
    got = pk.buf.cpu()
    bits = torch.int16 if dtype == BF else torch.int32
    for i, (e, row) in enumerate(zip(pk.entries, table)):
        lo, hi = e["dst_off"], e["dst_off"] + e["size"]
        assert torch.equal(got[lo:hi].view(bits), exp[lo:hi].view(bits)), "entry %d kind %d taps %d: %d elements differ" % (
            i, row[2], row[5], int((got[lo:hi].view(bits) != exp[lo:hi].view(bits)).sum()))
    assert torch.equal(got.view(bits), exp.view(bits)), "a guard region was written"


# ------------------------------------------------------------------------------------------------ 2. isa_conv_gemm
def gemm_plan(c):
    """Tile arithmetic of one case, restated from conv_gemm_impl / launch0 (conv_gemm.hip) and conv3x3_tiled_launch
    (conv3x3_tiled.hip).  GEMM: ("gemm", nt, K-groups, groups_per_chunk, nchunks, tiles, rows of the last tile, gy, gx);
    tiled 3x3: ("tiled3x3", tiles_x, tiles_y, tiles, gx)."""
    op, bf = c["op"], c["dtype"] == BF
    taps = {"convT": 1, "convT-dgrad": 4, "3x3": 9, "3x3-dgrad": 9, "1x1": 1}[op]
    kp = rup(c["cin"], 32)
    N = 4 * c["cout"] if op == "convT" else c["cout"]
    M = c["n"] * c["h"] * c["w"]
    if taps == 9 and bf and c["act"] == "none" and not c["bscale"] and not c["stats"] and kp == 32 and c["cout"] <= 32:
        tx, ty = (c["w"] + 31) // 32, (c["h"] + 7) // 8
        return ("tiled3x3", tx, ty, c["n"] * tx * ty, min(c["n"] * tx * ty, 512))
    assert not (op == "1x1" and bf and kp >= 128), "would take conv_gemm_tiled_kernel"
    nt = 1 if N <= 32 else (2 if N <= 64 else 4)
    tiles = (M + 127) // 128
    while nt > 1 and tiles * ((N + 32 * nt - 1) // (32 * nt)) < 512:
        nt //= 2
    groups = taps * kp // 32
    gpc = max(1, (48 * 1024) // (32 * nt * 32 * (2 if bf else 4)))
    gpc = min(gpc, groups)
    gy = (N + 32 * nt - 1) // (32 * nt)
    gx = min(tiles, max(1, 768 // gy))
    return ("gemm", nt, groups, gpc, (groups + gpc - 1) // gpc, tiles, M - (tiles - 1) * 128, gy, gx)


def G(name, dtype, op, n, h, w, cin, cout, plan, act="none", bscale=False, acc=0, stats=False, bias=False, view=None):
    """h, w: the M grid (input pixels; for convT-dgrad the dx pixels, dy is 2h x 2w).  cin / cout: channels of the GEMM's x
    and y tensors.  view = (c0, ld): y is the slice [c0, c0 + cout) of a buffer of ld channels."""
    return dict(name=name, dtype=dtype, op=op, n=n, h=h, w=w, cin=cin, cout=cout, plan=plan, act=act, bscale=bscale, acc=acc,
                stats=stats, bias=bias, view=view)


def _both_acc(**kw):
    return [G(acc=0, **kw), G(acc=1, **dict(kw, name=kw["name"] + "-acc"))]


GEMM_CASES = [
    # ---- ConvTranspose2d forward (ISA_OUT_SHUFFLE2, pack kind 2)
    # 512->256 bf16, M = 3*128*130 = 49920 -> 390 tiles (full), N = 1024 -> nt 4, gy 8, gx = 768 / 8 = 96: 4.06 tiles per
    # workgroup; 16 K-groups, 6 per chunk (48 KB / (128 rows * 32 * 2 B)) -> 3 chunks re-streamed per tile.  Lazy input
    # (ReLU6 + per-image multiplier), output into the second half of a 512-channel buffer
    G("convT-512-256-chunked", BF, "convT", 3, 128, 130, 512, 256, ("gemm", 4, 16, 6, 3, 390, 128, 8, 96),
      act="relu6", bscale=True, bias=True, view=(256, 512)),
    # 128->64 fp32, M = 2*125*131 = 32750 -> 256 tiles (last 110 rows), N = 256 -> nt 4 (256 * 2 = 512 workgroups), gy 2,
    # gx = 256: one tile each; 4 K-groups, 3 per chunk (fp32) -> 2 chunks
    G("convT-128-64", F32, "convT", 2, 125, 131, 128, 64, ("gemm", 4, 4, 3, 2, 256, 110, 2, 256), act="relu6", bscale=True,
      bias=True, view=(64, 128)),
    # the same at n = 6: M = 98250 -> 768 tiles (last 74 rows), gx = 768 / 2 = 384: 2 tiles per workgroup
    G("convT-128-64-walk", F32, "convT", 6, 125, 131, 128, 64, ("gemm", 4, 4, 3, 2, 768, 74, 2, 384), act="relu6",
      bscale=True, bias=True, view=(64, 128)),
    # resident weights: 64->32 bf16, M = 2*250*262 = 131000 -> 1024 tiles (last 56 rows), N = 128 -> nt 4, gy 1, gx 768:
    # 1.33 tiles per workgroup; 2 K-groups in one chunk, staged once (the `loaded` flag)
    G("convT-64-32-resident", BF, "convT", 2, 250, 262, 64, 32, ("gemm", 4, 2, 2, 1, 1024, 56, 1, 768), bias=True),
    # ---- ConvTranspose2d data gradient (ISA_IN_GATHER2, pack kind 3)
    # dy 256 ch at 256x260 -> dx 512 ch at 128x130, n = 3, bf16: M = 49920 -> 390 tiles, N = 512 -> nt 4, gy 4, gx 192:
    # 2.03 tiles per workgroup; 4 taps * 8 = 32 K-groups, 6 per chunk -> 6 chunks (the last one 2 groups)
    *_both_acc(name="convT-dgrad-256-512", dtype=BF, op="convT-dgrad", n=3, h=128, w=130, cin=256, cout=512,
               plan=("gemm", 4, 32, 6, 6, 390, 128, 4, 192)),
    # fp32 dy 64 ch -> dx 128 ch, n = 8, 125x131: M = 131000 -> 1024 tiles (last 56 rows), N = 128 -> nt 4, gy 1, gx 768:
    # 1.33 per workgroup; 4 * 2 = 8 K-groups, 3 per chunk -> 3 chunks
    *_both_acc(name="convT-dgrad-64-128", dtype=F32, op="convT-dgrad", n=8, h=125, w=131, cin=64, cout=128,
               plan=("gemm", 4, 8, 3, 3, 1024, 56, 1, 768)),
    # ---- dense 3x3 data gradient (ISA_IN_3X3 over tap-flipped weights, pack kind 1)
    # dy 128 -> dx 256, n = 4, 125x131, bf16: M = 65500 -> 512 tiles (last 92 rows), N = 256 -> nt 4, gy 2, gx 384: 1.33 per
    # workgroup; 9 * 4 = 36 K-groups, 6 per chunk -> 6 chunks
    *_both_acc(name="3x3-dgrad-128-256", dtype=BF, op="3x3-dgrad", n=4, h=125, w=131, cin=128, cout=256,
               plan=("gemm", 4, 36, 6, 6, 512, 92, 2, 384)),
    # fp32 dy 32 -> dx 64, n = 4, 250x262: M = 262000 -> 2047 tiles (last 112 rows), N = 64 -> nt 2, gy 1, gx 768: 2.67 per
    # workgroup; 9 K-groups, 6 per chunk (48 KB / (64 * 32 * 4 B)) -> 2 chunks
    *_both_acc(name="3x3-dgrad-32-64", dtype=F32, op="3x3-dgrad", n=4, h=250, w=262, cin=32, cout=64,
               plan=("gemm", 2, 9, 6, 2, 2047, 112, 1, 768)),
    # the head's own shapes: dy with 1 (`last_fc`) and 2 (`pred`) channels, stored with ld = 8 and NaN pad lanes, -> dx 32,
    # n = 8, 250x262: M = 524000 -> 4094 tiles (last 96 rows).  fp32: the GEMM, N = 32 -> nt 1, gy 1, gx 768: 5.33 per
    # workgroup, 9 K-groups resident.  bf16: kp == 32, 32 output channels, no prologue -> conv_gemm_impl hands it to
    # conv3x3_tiled_launch: 9 x 32 tiles of 8x32 per image = 2304 tiles, gx 512: 4.5 per workgroup
    *_both_acc(name="3x3-dgrad-1-32", dtype=F32, op="3x3-dgrad", n=8, h=250, w=262, cin=1, cout=32,
               plan=("gemm", 1, 9, 9, 1, 4094, 96, 1, 768)),
    *_both_acc(name="3x3-dgrad-2-32", dtype=F32, op="3x3-dgrad", n=8, h=250, w=262, cin=2, cout=32,
               plan=("gemm", 1, 9, 9, 1, 4094, 96, 1, 768)),
    *_both_acc(name="3x3-dgrad-1-32", dtype=BF, op="3x3-dgrad", n=8, h=250, w=262, cin=1, cout=32,
               plan=("tiled3x3", 9, 32, 2304, 512)),
    *_both_acc(name="3x3-dgrad-2-32", dtype=BF, op="3x3-dgrad", n=8, h=250, w=262, cin=2, cout=32,
               plan=("tiled3x3", 9, 32, 2304, 512)),
    # ---- dense 3x3 forward, chunked, walked, with prologue and statistics (pack kind 0)
    # 256->128 bf16, ReLU6 with nonzero shifts (a padded tap that contributed act(shift) instead of 0 would show), n = 4,
    # 250x262: M = 262000 -> 2047 tiles (last 112 rows), N = 128 -> nt 4, gy 1, gx 768: 2.67 per workgroup; 72 K-groups, 6
    # per chunk -> 12 chunks
    G("3x3-256-128", BF, "3x3", 4, 250, 262, 256, 128, ("gemm", 4, 72, 6, 12, 2047, 112, 1, 768), act="relu6", stats=True,
      bias=True),
    # fp32 64->32 LEAKY: N = 32 -> nt 1, gx 768: 2.67 per workgroup; 18 K-groups, 12 per chunk -> 2 chunks
    G("3x3-64-32", F32, "3x3", 4, 250, 262, 64, 32, ("gemm", 1, 18, 12, 2, 2047, 112, 1, 768), act="leaky", stats=True,
      bias=True),
    # ---- conv3x3_tiled.hip forward at N = 1, 2, 24 (the walk file has N = 16): bf16, bias, n = 8, 250x262: 2304 tiles of
    # 8x32 (tiles_x 9: 262 % 32 = 6, tiles_y 32: 250 % 8 = 2), gx 512: 4.5 per workgroup.  N = 1, 2: every store is the
    # element path; N = 24: channels 0..15 leave as two 16-byte stores, 16..23 by element
    *[g for N in (1, 2, 24) for cin in (16, 32)
      for g in _both_acc(name="3x3-tiled-%d-%d" % (cin, N), dtype=BF, op="3x3", n=8, h=250, w=262, cin=cin, cout=N,
                         plan=("tiled3x3", 9, 32, 2304, 512), bias=True)],
    # ---- the element (tail) path of the GEMM epilogue: 1x1 32->21 into channels [3, 24) of a 40-channel buffer - no 8-channel
    # segment starts on a 16-byte boundary, so every store is by element - and into [8, 29): segments 0 and 1 are 16-byte
    # stores, the third (5 channels) is the tail.  M = 2*37*45 = 3330 -> 27 tiles (last 2 rows), N = 21 -> nt 1, gx 27
    *[g for dt in (F32, BF) for c0 in (3, 8)
      for g in _both_acc(name="tail-c0=%d" % c0, dtype=dt, op="1x1", n=2, h=37, w=45, cin=32, cout=21,
                         plan=("gemm", 1, 1, 1, 1, 27, 2, 1, 27), bias=True, view=(c0, 40))],
]


def grid(shape, seed, step, lim):
    """Random multiples of `step` in [-lim, lim] (about normal, sigma lim / 2)."""
    return (rand(*shape, seed=seed) * (lim / 2 / step)).round().clamp(-lim / step, lim / step) * step


def case_id(c):
    return "%s-%s" % (c["name"], tname(c["dtype"]))


def gemm_operands(c):
    """CPU operands of a case, values of its storage type: x, w (state_dict layout), b, prologue constants, old output."""
    op, dtype, n, h, w, cin, cout = c["op"], c["dtype"], c["n"], c["h"], c["w"], c["cin"], c["cout"]
    xh, xw = (2 * h, 2 * w) if op == "convT-dgrad" else (h, w)
    oh, ow = (2 * h, 2 * w) if op == "convT" else (h, w)
    taps = {"convT": 1, "convT-dgrad": 4, "3x3": 9, "3x3-dgrad": 9, "1x1": 1}[op]
    wshape = {"convT": (cin, cout, 2, 2), "convT-dgrad": (cout, cin, 2, 2), "3x3": (cout, cin, 3, 3),
              "3x3-dgrad": (cin, cout, 3, 3), "1x1": (cout, cin, 1, 1)}[op]
    if dtype == BF:      # the exact grid (see the module docstring): every partial sum is an fp32 value in any order
        assert c["act"] in ("none", "relu6") and taps * rup(cin, 32) <= 4608
        o = dict(x=grid((n, cin, xh, xw), 31, 0.25, 2.0), w=grid(wshape, 32, 0.125, 0.25),
                 b=grid((cout,), 33, 0.125, 1.0) if c["bias"] else None)
    else:
        o = dict(x=rand(n, cin, xh, xw, seed=31, scale=2.0), w=rand(*wshape, seed=32, scale=(taps * cin) ** -0.5),
                 b=rand(cout, seed=33) if c["bias"] else None)
    o.update(sc=None, sh=None, bs=None, old=None, oh=oh, ow=ow)
    if c["act"] != "none":
        o["sc"], o["sh"] = dyadic_pro(cin, seed=34)
    if c["bscale"]:
        o["bs"] = (rand(n, cin, seed=35) > 0).float() * 2.0
    if c["acc"]:
        o["old"] = grid((n, cout, oh, ow), 36, 0.125, 8.0) if dtype == BF else rand(n, cout, oh, ow, seed=36)
    return o


def gemm_ref(c, o, P):
    """The conv of the case in precision P from the operand the MFMA sees (rounded to storage after the prologue)."""
    dtype, op = c["dtype"], c["op"]
    xt = o["x"] if c["act"] == "none" and o["bs"] is None else pro32(o["x"], o["sc"], o["sh"], ACTS[c["act"]], o["bs"])
    xt = rs(xt, dtype).to(P)
    wq = rs(o["w"], dtype).to(P)
    b = o["b"].to(P) if o["b"] is not None else None
    if op == "convT":
        return F.conv_transpose2d(xt, wq, b, stride=2)
    if op == "convT-dgrad":                   # dx[k] = sum_{co, dy, dx} dy[co, 2y + dy, 2x + dx] * w[k, co, dy, dx]
        return F.conv2d(xt, wq, stride=2)
    if op == "3x3-dgrad":
        return F.conv_transpose2d(xt, wq, padding=1)
    return F.conv2d(xt, wq, b, padding=1 if op == "3x3" else 0)


def stored(c, o, raw):
    """What the kernel stores: rs(result) or rs(old + result)."""
    return rs(raw + o["old"].double() if c["acc"] else raw, c["dtype"])


@pytest.mark.gpu
@pytest.mark.parametrize("c", GEMM_CASES, ids=case_id)
def test_conv_gemm_paths(c):
    L, Act, Engine, ParamStore, Pro = _gpu()
    from isa_amd.engine import Packer
    lib = L.lib()
    op, dtype, n, cin, cout = c["op"], c["dtype"], c["n"], c["cin"], c["cout"]
    o = gemm_operands(c)
    raw = gemm_ref(c, o, torch.float64)
    ref = stored(c, o, raw)
    kp = rup(cin, 32)
    if op == "convT":
        pk, key = packed(ParamStore, Packer, o["w"], dtype, 2, cout, cin, 4, kp, 4 * cout)
    elif op == "convT-dgrad":
        pk, key = packed(ParamStore, Packer, o["w"], dtype, 3, cin, cout, 4, kp, cout)
    elif op == "3x3-dgrad":
        pk, key = packed(ParamStore, Packer, o["w"], dtype, 1, cin, cout, 9, kp, cout)
    else:
        pk, key = packed(ParamStore, Packer, o["w"], dtype, 0, cout, cin, 9 if op == "3x3" else 1, kp, cout)
    in_mode = {"convT": L.IN_1X1, "convT-dgrad": L.IN_GATHER2, "3x3": L.IN_3X3, "3x3-dgrad": L.IN_3X3, "1x1": L.IN_1X1}[op]
    out_mode = L.OUT_SHUFFLE2 if op == "convT" else L.OUT_PLAIN
    xa = Act(nhwc(o["x"], dtype), 0, cin)                           # pad lanes (cin % 8) are NaN
    pro = None
    if c["act"] != "none" or c["bscale"]:
        assert ACTS[c["act"]] == getattr(L, "ACT_" + c["act"].upper())
        pro = Pro(o["sc"][0].cuda(), o["sh"][0].cuda(), ACTS[c["act"]], o["bs"].cuda() if o["bs"] is not None else None)
    c0, ld = c["view"] or (0, rup(cout, 8))
    ybuf = torch.full((n, o["oh"], o["ow"], ld), POISON, dtype=dtype, device="cuda")
    ybuf[..., c0:c0 + cout] = o["old"].permute(0, 2, 3, 1).to(dtype).cuda() if c["acc"] else NAN
    ya = Act(ybuf, c0, cout)
    bias = o["b"].cuda() if o["b"] is not None else None
    st = torch.zeros(STAT_R * 2 * cout, device="cuda") if c["stats"] else None
    L.check(lib.isa_conv_gemm(xa.d(), C.byref(pro._c) if pro else None, pk.ptr(key), kp, L.ptr(bias), ya.d(), in_mode,
                              out_mode, L.ptr(st), c["acc"], L.stream_ptr()), "isa_conv_gemm")
    torch.cuda.synchronize()
    tag = "%s %s" % (gemm_plan(c)[0], case_id(c))
    check(tag + " y", ya.nchw(), ref, store_bound(dtype))
    ybuf[..., c0:c0 + cout] = POISON
    assert bool((ybuf == POISON).all()), "%s: a lane outside the output slice [%d, %d) of %d was written" % (tag, c0, c0 + cout, ld)
    if c["stats"]:
        s = stat_sums(st, cout)[0]
        check(tag + " sum", s[:cout], raw.sum((0, 2, 3)), FP32_BOUND)
        check(tag + " sumsq", s[cout:], (raw * raw).sum((0, 2, 3)), FP32_BOUND)


def test_plans_match_launch_code():
    """The tile arithmetic each case states equals what the launch code computes for its shape, and the table holds the
    forms it is there for: chunked launches that walk (more tiles than workgroups) in every addressing mode, a resident
    one, both kernels for the head's 1- and 2-channel gradients, both dtypes."""
    for c in GEMM_CASES:
        assert gemm_plan(c) == c["plan"], (case_id(c), gemm_plan(c), c["plan"])
    def has(op, dtype, pred):
        return any(c["op"] == op and c["dtype"] == dtype and c["plan"][0] == "gemm" and pred(c["plan"]) for c in GEMM_CASES)
    chunked_walk = lambda p: p[4] > 1 and p[5] > p[8]             # noqa: E731
    for op in ("convT", "convT-dgrad", "3x3", "3x3-dgrad"):
        for dtype in (F32, BF):
            assert has(op, dtype, chunked_walk), (op, dtype)
    assert has("convT", BF, lambda p: p[4] == 1 and p[5] > p[8])
    for dtype, kernel in ((F32, "gemm"), (BF, "tiled3x3")):
        for cin in (1, 2):
            assert any(c["op"] == "3x3-dgrad" and c["cin"] == cin and c["dtype"] == dtype and c["plan"][0] == kernel
                       for c in GEMM_CASES)


# ------------------------------------------------------------------------------------------------ 3. isa_conv_wgrad
def W(name, dtype, mode, K, N, kmap, ksrc, k, act="relu"):
    return dict(name=name, dtype=dtype, mode=mode, K=K, N=N, kmap=kmap, ksrc=ksrc, k=k, act=act)


KS = [1, 3, None, "arena"]         # slab sets in the NaN workspace = workgroups along x (None: uncapped, arena: deferred fold)
WG_N, WG_H, WG_W = 2, 37, 45       # M = 3330 input pixels: 105 chunks of 32 (bf16) / 209 of 16 (fp32)

WG_CASES = [W(k=k, dtype=dt, **kw) for kw in (
    # the decoder's first conv: 1x1 over the cat-free buffer [gated | cross | aux], weights stored [cross | gated | aux].
    # K = 512, N = 256: nt 8, kt 16 -> 2x2 tiles per wave, gy = 4 * 8 = 32; uncapped gx = min(27 | 53, 512 / 32 = 16)
    dict(name="1x1-perm-512", mode="1x1", K=512, N=256, kmap=decoder_map(256, 6), ksrc=512),
    # K = 64, N = 32: nt 1, kt 2 -> 1x2 tiles per wave, gy 1; uncapped gx = 27 (bf16) / 53 (fp32)
    dict(name="1x1-perm-64", mode="1x1", K=64, N=32, kmap=decoder_map(32, 6), ksrc=64),
    # 20 of the 64 physical channels are padding (-1), 45 source channels, one of them unmapped: dW[:, 44] keeps its value
    dict(name="1x1-holes-64", mode="1x1", K=64, N=32, kmap=holes_map(64, 45, 41), ksrc=45),
    # ISA_IN_3X3 (taps 9, grid z = 9): the generic kernel in both dtypes (a map keeps bf16 off conv3x3_wgrad_tiled)
    dict(name="3x3-perm-64", mode="3x3", K=64, N=32, kmap=decoder_map(32, 6), ksrc=64),
    dict(name="3x3-holes-64", mode="3x3", K=64, N=32, kmap=holes_map(64, 45, 42), ksrc=45),
    # ISA_OUT_SHUFFLE2 (taps 4), dW [Ksrc][Co][2][2]
    dict(name="convT-perm-64", mode="convT", K=64, N=32, kmap=decoder_map(32, 6), ksrc=64),
    dict(name="convT-holes-64", mode="convT", K=64, N=32, kmap=holes_map(64, 45, 43), ksrc=45),
    # ConvTranspose2d at the backbone's widths, no map.  512->256: nt 8, kt 16 -> 2x2 per wave, gy 32, taps 4: uncapped
    # gx = 512 / (32 * 4) = 4; 128->64: nt 2, kt 4 -> 2x2, gy 2, gx = min(27 | 53, 512 / 8 = 64)
    dict(name="convT-512-256", mode="convT", K=512, N=256, kmap=None, ksrc=512),
    dict(name="convT-128-64", mode="convT", K=128, N=64, kmap=None, ksrc=128),
) for dt in (F32, BF) for k in KS]

# conv3x3_wgrad_tiled_kernel (bf16, no prologue, no map, channels <= 32) with the head's 1- and 2-channel dy: 2 x 5 tiles per
# image = 20 tiles; k = 1: one workgroup walks all 20; 3: 6.7 each; uncapped gx = 20
WG_TILED = [W(name="3x3-tiled-dy%d" % N, dtype=BF, mode="3x3", K=32, N=N, kmap=None, ksrc=32, k=k, act="none")
            for N in (1, 2) for k in KS]


def wg_id(c):
    return "%s-%s-k%s" % (c["name"], tname(c["dtype"]), c["k"])


def wgrad_operands(c):
    dtype, K, N = c["dtype"], c["K"], c["N"]
    up = 2 if c["mode"] == "convT" else 1
    o = dict(x=inp(rand(WG_N, K, WG_H, WG_W, seed=51, scale=2.0), dtype),
             dy=inp(rand(WG_N, N, up * WG_H, up * WG_W, seed=52), dtype), sc=None, sh=None)
    if c["act"] != "none":
        o["sc"], o["sh"] = dyadic_pro(K, seed=53)
    shape = {"1x1": (N, c["ksrc"]), "3x3": (N, c["ksrc"], 3, 3), "convT": (c["ksrc"], N, 2, 2)}[c["mode"]]
    o["dw0"], o["db0"] = rand(*shape, seed=54), rand(N, seed=55)          # dW, db before the call: the kernel adds
    return o


def wgrad_ref(c, o, P):
    """(dW in state_dict layout, db), the gradient alone, in precision P."""
    dtype = c["dtype"]
    xt = o["x"] if c["act"] == "none" else pro32(o["x"], o["sc"], o["sh"], ACTS[c["act"]])
    xt = rs(xt, dtype)
    if c["kmap"] is not None:
        xt = to_source_order(xt, c["kmap"], c["ksrc"])
    xt, dy = xt.to(P), o["dy"].to(P)
    wv = torch.zeros(o["dw0"].shape if c["mode"] != "1x1" else o["dw0"].shape + (1, 1), dtype=P, requires_grad=True)
    if c["mode"] == "convT":
        F.conv_transpose2d(xt, wv, stride=2).backward(dy)
    else:
        F.conv2d(xt, wv, padding=1 if c["mode"] == "3x3" else 0).backward(dy)
    return wv.grad.reshape(o["dw0"].shape), dy.sum((0, 2, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("c", WG_CASES + WG_TILED, ids=wg_id)
def test_conv_wgrad_maps(c):
    """dW += and db += through a NaN workspace of k slab sets, compared in state_dict layout [N][Ksrc](taps) with the
    float64 gradient of the conv over the source-ordered input x_phys[:, inverse map]; rows of unmapped source channels keep
    their value.  ConvTranspose2d: db sums all four output quadrants."""
    L, Act, Engine, ParamStore, Pro = _gpu()
    lib = L.lib()
    dtype, K, N, mode = c["dtype"], c["K"], c["N"], c["mode"]
    o = wgrad_operands(c)
    g_dw, g_db = wgrad_ref(c, o, torch.float64)
    xa, da = Act(nhwc(o["x"], dtype), 0, K), Act(nhwc(o["dy"], dtype), 0, N)
    pro = None
    if c["act"] != "none":
        assert ACTS[c["act"]] == getattr(L, "ACT_" + c["act"].upper())
        pro = Pro(o["sc"][0].cuda(), o["sh"][0].cuda(), ACTS[c["act"]])
    dw, db = o["dw0"].cuda(), o["db0"].cuda()
    km = torch.tensor(c["kmap"], dtype=torch.int32, device="cuda") if c["kmap"] is not None else None
    taps = {"1x1": 1, "3x3": 9, "convT": 4}[mode]
    in_mode = L.IN_3X3 if mode == "3x3" else L.IN_1X1
    out_mode = L.OUT_SHUFFLE2 if mode == "convT" else L.OUT_PLAIN
    tiled = c in WG_TILED
    set_floats = 9 * (1024 + 32) if tiled else wgrad_set_floats(N, K, taps)
    pc = C.byref(pro._c) if pro else None
    run_ws_call(L, lambda ws, wsf, sa: lib.isa_conv_wgrad(xa.d(), pc, da.d(), L.ptr(dw), L.ptr(db), in_mode, out_mode,
                                                         L.ptr(km), c["ksrc"], ws, wsf, sa, L.stream_ptr()),
                c["k"], set_floats, "isa_conv_wgrad")
    tag = "wgrad %s" % wg_id(c)
    # the bound is relative to the gradient, not to gradient + initial value
    check(tag + " dW", dw.cpu().double() - o["dw0"].double(), g_dw, FP32_BOUND)
    check(tag + " db", db.cpu().double() - o["db0"].double(), g_db, FP32_BOUND)
    if c["kmap"] is not None:
        unmapped = sorted(set(range(c["ksrc"])) - set(c["kmap"]))
        kdim = 0 if mode == "convT" else 1
        for k in unmapped:                    # nothing was added: bit-equal, not merely close
            assert torch.equal(dw.cpu().select(kdim, k), o["dw0"].select(kdim, k)), (tag, "unmapped source channel", k)


def test_wgrad_tiles_of_cases():
    """dispatch_wg's tiles per wave and gy for the shapes the comments of WG_CASES name."""
    assert wgrad_tiles(256, 512) == (2, 2, 32) and wgrad_tiles(32, 64) == (1, 2, 1) and wgrad_tiles(64, 128) == (2, 2, 2)
    for c in WG_CASES:
        holes = c["name"].split("-")[1] == "holes"
        if c["kmap"] is not None:
            assert len(c["kmap"]) == c["K"] and max(c["kmap"]) < c["ksrc"]
            mapped = [k for k in c["kmap"] if k >= 0]
            assert len(set(mapped)) == len(mapped) and (len(mapped) < c["K"]) == holes


# ------------------------------------------------------------------------------------------------ 4. refusals
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF], ids=tname)
def test_conv_forms_refused(dtype):
    """Argument combinations these forms do not have return ISA_EINVAL and launch nothing: every output stays NaN."""
    L, Act, Engine, ParamStore, Pro = _gpu()
    lib = L.lib()
    n, h, w, K, N = 4, 6, 10, 32, 32

    def act(c, hh=h, ww=w, groups=1):
        return Act(torch.full((n, hh, ww, rup(c, 8)), NAN, dtype=dtype, device="cuda"), 0, c, groups=groups)

    wt = torch.zeros(4 * N * 9 * 64, dtype=dtype, device="cuda")
    sc, sh = torch.ones(2 * K, device="cuda"), torch.zeros(2 * K, device="cuda")
    pro = Pro(sc, sh, L.ACT_RELU6)
    outs = []

    def gemm(x, p, y, in_mode, out_mode, stats=False, kp=K, ep=None, control=False):
        st = torch.full((2 * STAT_R * 2 * 4 * N,), NAN, device="cuda") if stats else None
        if not control:
            outs.extend(t for t in (y.buf, st) if t is not None)
        if ep is not None:
            return lib.isa_conv_gemm_ep(x.d(), p, L.ptr(wt), kp, None, y.d(), in_mode, C.byref(ep), L.stream_ptr())
        return lib.isa_conv_gemm(x.d(), p, L.ptr(wt), kp, None, y.d(), in_mode, out_mode, L.ptr(st), 0, L.stream_ptr())

    pc = C.byref(pro._c)
    # statistic groups with per-channel constants or statistics exist for 1x1 / PLAIN only
    assert gemm(act(K, groups=2), pc, act(N, groups=2), L.IN_3X3, L.OUT_PLAIN) == -1
    assert gemm(act(K, groups=2), None, act(N, groups=2), L.IN_3X3, L.OUT_PLAIN, stats=True) == -1
    assert gemm(act(K, 2 * h, 2 * w, groups=2), pc, act(N, groups=2), L.IN_GATHER2, L.OUT_PLAIN) == -1
    assert gemm(act(K, groups=2), pc, act(N, 2 * h, 2 * w, groups=2), L.IN_1X1, L.OUT_SHUFFLE2) == -1
    # ... and the same calls with one statistic group are accepted: it is the groups that were refused
    assert gemm(act(K), pc, act(N), L.IN_3X3, L.OUT_PLAIN, control=True) == 0
    assert gemm(act(K, 2 * h, 2 * w), pc, act(N), L.IN_GATHER2, L.OUT_PLAIN, control=True) == 0
    assert gemm(act(K), pc, act(N, 2 * h, 2 * w), L.IN_1X1, L.OUT_SHUFFLE2, control=True) == 0
    # the pixel shuffle has no statistics and needs 16-channel quadrants
    assert gemm(act(K), None, act(N, 2 * h, 2 * w), L.IN_1X1, L.OUT_SHUFFLE2, stats=True) == -1
    assert gemm(act(K), None, act(24, 2 * h, 2 * w), L.IN_1X1, L.OUT_SHUFFLE2) == -1
    # the eval epilogue has no gather form
    ep = L.IsaConvEp(L.addr(sc), L.addr(sh), L.ACT_NONE, None)
    assert gemm(act(K, 2 * h, 2 * w), None, act(N), L.IN_GATHER2, L.OUT_PLAIN, ep=ep) == -1
    # kp below the input's channels
    assert gemm(act(64), None, act(N), L.IN_1X1, L.OUT_PLAIN, kp=32) == -1
    # weight gradient: no gather form, and the pixel shuffle is 1x1 only
    for x, dy, in_mode, out_mode in ((act(K, 2 * h, 2 * w), act(N), L.IN_GATHER2, L.OUT_PLAIN),
                                     (act(K), act(N, 2 * h, 2 * w), L.IN_3X3, L.OUT_SHUFFLE2)):
        dw, db, ws = nan_ws(N * K * 9), nan_ws(N), nan_ws(1 << 20)
        outs.extend((dw, db, ws))
        assert lib.isa_conv_wgrad(x.d(), None, dy.d(), L.ptr(dw), L.ptr(db), in_mode, out_mode, None, K, L.ptr(ws),
                                  ws.numel(), None, L.stream_ptr()) == -1
    torch.cuda.synchronize()
    for t in outs:
        assert bool(torch.isnan(t.float()).all()), "a refused call wrote to an output"


# ------------------------------------------------------------------------------------------------ bounds: CPU-only tests
FLOOR_GEMM = [c for c in GEMM_CASES if not c["acc"]]              # accumulate does not change the contraction
FLOOR_WG = [c for c in WG_CASES + WG_TILED if c["k"] == 1]                                       # k does not change the math


@pytest.mark.parametrize("c", FLOOR_GEMM, ids=case_id)
def test_fp32_floor_gemm(c):
    """FP32_BOUND may be used on a case only if the float32 CPU evaluation of its reference is within FLOOR of float64."""
    o = gemm_operands(c)
    r64, r32 = gemm_ref(c, o, torch.float64), gemm_ref(c, o, torch.float32)
    e = [walk_err(r32, r64)[0]]
    if c["stats"]:
        e.append(walk_err(r32.sum((0, 2, 3)), r64.sum((0, 2, 3)))[0])
        e.append(walk_err((r32 * r32).sum((0, 2, 3)), (r64 * r64).sum((0, 2, 3)))[0])
    print("FLOOR %-40s %s" % (case_id(c), " ".join("%.2e" % v for v in e)))
    assert max(e) < FLOOR, (case_id(c), e)


def wgrad_gemm32(c, o):
    """The weight gradient of the case as float32 matrix products over the pixels, one per tap (another summation order
    than the float64 autograd reference: torch's float32 conv backward on the CPU adds pixel by pixel)."""
    xt = o["x"] if c["act"] == "none" else pro32(o["x"], o["sc"], o["sh"], ACTS[c["act"]])
    xt = rs(xt, c["dtype"])
    if c["kmap"] is not None:
        xt = to_source_order(xt, c["kmap"], c["ksrc"])
    xt, dy = xt.float(), o["dy"].float()
    if c["mode"] == "convT":
        dw = torch.stack([torch.einsum("bkhw,bnhw->kn", xt, dy[:, :, i::2, j::2]) for i in (0, 1) for j in (0, 1)], -1)
    elif c["mode"] == "3x3":
        xp = F.pad(xt, (1, 1, 1, 1))
        dw = torch.stack([torch.einsum("bnhw,bkhw->nk", dy, xp[:, :, i:i + WG_H, j:j + WG_W]) for i in range(3)
                          for j in range(3)], -1)
    else:
        dw = torch.einsum("bnhw,bkhw->nk", dy, xt)
    return dw.reshape(o["dw0"].shape), dy.sum((0, 2, 3))


@pytest.mark.parametrize("c", FLOOR_WG, ids=wg_id)
def test_fp32_floor_wgrad(c):
    o = wgrad_operands(c)
    (w64, b64), (w32, b32) = wgrad_ref(c, o, torch.float64), wgrad_gemm32(c, o)
    e = [walk_err(w32, w64)[0], walk_err(b32, b64)[0]]
    print("FLOOR %-40s %s" % (wg_id(c), " ".join("%.2e" % v for v in e)))
    assert max(e) < FLOOR, (wg_id(c), e)


def test_bounds_reject_path_bugs():
    """The comparison and the loosest bound of this file, applied to float64 references corrupted the way these paths
    break, reject every corruption by more than 10x."""
    loosest = max(BF16_STORE, FP32_BOUND)
    bad = []
    n, K, Co, h, w = 2, 96, 32, 9, 21                       # 378 input pixels: tiles 0, 1 full, tile 2 ragged
    x, wt = rand(n, K, h, w, seed=91).double(), rand(K, Co, 2, 2, seed=92, scale=K ** -0.5).double()
    ref = F.conv_transpose2d(x, wt, stride=2)
    # 1. two output quadrants of the pixel shuffle swapped: (dy 0, dx 1) <-> (dy 1, dx 0)
    t = ref.clone()
    t[:, :, 0::2, 1::2], t[:, :, 1::2, 0::2] = ref[:, :, 1::2, 0::2], ref[:, :, 0::2, 1::2]
    bad.append(("quadrants swapped", t, ref))
    # 2. the second 128-pixel tile computed with the previous chunk's weights: its last K-chunk (32 of 96 channels) missing
    xm = x.permute(0, 2, 3, 1).reshape(-1, K).clone()
    xm[128:256, 64:] = 0
    t = F.conv_transpose2d(xm.reshape(n, h, w, K).permute(0, 3, 1, 2), wt, stride=2)
    bad.append(("stale weight chunk on the second tile", t, ref))
    # 3. the 3x3 data gradient without the tap flip
    dy, w3 = rand(n, Co, h, w, seed=93).double(), rand(Co, K, 3, 3, seed=94, scale=(9 * Co) ** -0.5).double()
    bad.append(("taps not flipped", F.conv_transpose2d(dy, w3.flip(2, 3), padding=1), F.conv_transpose2d(dy, w3, padding=1)))
    # 4. the channel map applied as its inverse in a weight gradient
    km = decoder_map(48, 6)
    inv = [km.index(k) for k in range(K)]
    g = rand(n, Co, h, w, seed=95).double()
    dws = [torch.einsum("bnhw,bkhw->nk", g, to_source_order(x, m, K)) for m in (km, inv)]
    bad.append(("map inverted", dws[1], dws[0]))
    # 5. the bias gradient of the transposed conv from one quadrant only
    g2 = rand(n, Co, 2 * h, 2 * w, seed=96).double()
    bad.append(("bias gradient of one quadrant", g2[:, :, 0::2, 0::2].sum((0, 2, 3)), g2.sum((0, 2, 3))))
    # 6. accumulate ignored
    old = rand(*ref.shape, seed=97).to(BF).double()
    bad.append(("accumulate ignored", rs(ref, BF), rs(old + ref, BF)))
    for what, t, r in bad:
        e, where = walk_err(t, r)
        assert e > 10 * loosest, (what, e, where)
        assert walk_err(r.clone(), r)[0] < FP32_BOUND
