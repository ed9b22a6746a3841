"""The kernels that turn logits into outputs, and the network's layout boundary, for 2 <= K <= 32 classes.

Entry points: isa_softmax_nchw (Model.predict's probabilities), isa_chan_argmax (the arg-max map of ReSeg.forward,
pred.py and pred_list.py), isa_nchw_to_nhwc (both its row kernel and its element kernel) and isa_nhwc_to_nchw.  Before
this file they were reached only inside model tests with 2 classes, and the element form of isa_nchw_to_nhwc never.

Every call goes through the C ABI (isa_amd.lib).  Inputs sit in channel slices of wider buffers whose other channels hold
NaN, flat outputs are followed by NaN; whatever a kernel must not write has to stay bit-unchanged.
  * isa_softmax_nchw: float64 softmax of the stored logits; max |got - ref| <= 1e-6 and every class sum within 1e-6
    of 1 (SOFTMAX_BOUND; measured worst printed as OUTERR lines).
  * isa_chan_argmax: exactly torch.argmax of the stored logits (first maximum; NaN is the maximum), with equal logits
    planted at two channels.
  * isa_nchw_to_nhwc / isa_nhwc_to_nchw: bit-exact; bf16 stores equal torch's round-to-nearest-even .to(bfloat16).
    What each path does to the channels at or above c is asserted: the row kernel writes whole padded rows (zeros),
    the element kernel leaves them alone.
  * One model-level line: a semantic-only ReSeg(K, use_instance_seg=False) in eval mode against reseg_forward in float64
    (logits at the fp32 bound of test_three_class_step_matches_float64_autograd, the arg-max map with assert_index_map).

Measured on MI355X: softmax_nchw max |err| 6.6e-7 and max |sum - 1| 7.1e-7 (K = 32, 540 672 pixels; 1e-6 is 1.4x above:
the bound is ~8 ulp of 1.0, the kernel's expf and one division per class leave a few); chan_argmax and both converters
exact; ReSeg(K) eval logits 7.6e-6 of max |ref| (bound 1e-4, 13x).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import reseg_ref as R  # noqa: E402
from test_gpu_ops import _gpu, rand  # noqa: E402
from test_oracle_golden import assert_index_map  # noqa: E402

gpu = pytest.mark.gpu
BF = torch.bfloat16
DTYPES = [torch.float32, BF]
KS = [2, 3, 8, 21, 32]
NAN = float("nan")
SOFTMAX_BOUND = 1e-6
LOGIT_BOUND = 1e-4                       # test_gpu_sem_criterion.test_three_class_step_matches_float64_autograd


def _lib():
    L = _gpu()[0]
    return L, L.lib()


def rup8(c):
    return (c + 7) // 8 * 8


def _bits(t):
    t = t.contiguous().cpu()
    return t.view({torch.float32: torch.int32, BF: torch.int16}[t.dtype])


def _bits_equal(a, b):
    return torch.equal(_bits(a), _bits(b))


class NhwcSlice:
    """[n, h, w, c] at channel c0 of a NaN buffer [n, h, w, ld] (channel slices of the network's buffers)."""
    def __init__(self, L, n, h, w, c, ld, c0, dtype, values=None):
        self.buf = torch.full((n, h, w, ld), NAN, dtype=dtype, device="cuda")
        if values is not None:
            self.buf[..., c0:c0 + c] = values.to(dtype).cuda()
        self.orig = self.buf.clone()
        self.c0, self.c = c0, c
        self.t = L.IsaTensor(self.buf.data_ptr() + c0 * self.buf.element_size(), n, h, w, c, ld, L.dtype_code(dtype), 1)

    def d(self):
        return C.byref(self.t)

    def get(self):
        return self.buf[..., self.c0:self.c0 + self.c].cpu()

    def neighbours_unchanged(self):
        b, o = self.buf.cpu(), self.orig.cpu()
        return _bits_equal(b[..., :self.c0], o[..., :self.c0]) and \
            _bits_equal(b[..., self.c0 + self.c:], o[..., self.c0 + self.c:])


def logits(n, h, w, K, seed):
    """[n, h, w, K] fp32 logits: N(0, 3) with a few large ones (+-30) so the max subtraction matters."""
    x = rand(n, h, w, K, seed=seed, scale=3.0)
    g = torch.Generator().manual_seed(seed + 1)
    big = torch.rand(n, h, w, K, generator=g) < 0.01
    return torch.where(big, 30.0 * torch.sign(x), x)


SHAPES = [(2, 13, 11), (1, 768, 704)]         # 286 pixels; 540 672 pixels > the 2048 x 256 grid cap


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", SHAPES)
def test_softmax_nchw(dtype, K, shape):
    """Softmax over the K channels of an NHWC logit slice (ld padding and the channels before it NaN), written NCHW
    fp32: max-abs error vs the float64 softmax of the stored logits <= 1e-6, class sums within 1e-6 of 1."""
    L, lib = _lib()
    n, h, w = shape
    x = logits(n, h, w, K, seed=K * 10 + h)
    c0 = 3
    xs = NhwcSlice(L, n, h, w, K, c0 + rup8(K) + 8, c0, dtype, x)
    numel = n * K * h * w
    buf = torch.full((numel + 512,), NAN, device="cuda")
    L.check(lib.isa_softmax_nchw(xs.d(), L.ptr(buf), L.stream_ptr()), "isa_softmax_nchw")
    got = buf[:numel].view(n, K, h, w).double().cpu()
    ref = torch.softmax(xs.get().double().permute(0, 3, 1, 2), 1)
    err = float(torch.nan_to_num((got - ref).abs(), nan=float("inf")).max())
    sums = float((got.sum(1) - 1).abs().max())
    print("OUTERR softmax_nchw K%-2d %-8s %dx%dx%d  max|err| %.2e  max|sum-1| %.2e  bound %.0e"
          % (K, str(dtype)[6:], n, h, w, err, sums, SOFTMAX_BOUND))
    assert err <= SOFTMAX_BOUND and sums <= SOFTMAX_BOUND, (err, sums)
    assert bool(torch.isnan(buf[numel:]).all()) and xs.neighbours_unchanged()


def argmax_ref(v):
    """torch.argmax over the last dim of the stored values; checked against an explicit first-maximum scan where NaN
    is the maximum."""
    ref = torch.argmax(v, -1)
    nan = torch.isnan(v)
    K = v.shape[-1]
    ar = torch.arange(K).expand_as(v)
    first_nan = torch.where(nan, ar, torch.full_like(ar, K)).min(-1).values
    m = torch.nan_to_num(v, nan=float("-inf")).max(-1, keepdim=True).values
    first_max = torch.where(v == m, ar, torch.full_like(ar, K)).min(-1).values
    scan = torch.where(first_nan < K, first_nan, first_max)
    assert torch.equal(ref, scan)
    return ref


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", SHAPES)
def test_chan_argmax(dtype, K, shape):
    """The arg-max map: exactly torch.argmax of the stored logits.  A quarter of the pixels carry the maximum at two
    channels (the first wins), a few carry NaN (the first NaN wins, as in torch).  The output is a 1-channel slice of
    a NaN buffer."""
    L, lib = _lib()
    n, h, w = shape
    x = logits(n, h, w, K, seed=K * 10 + w + 5)
    g = torch.Generator().manual_seed(K + h)
    P = n * h * w
    flat = x.reshape(P, K)
    tie = torch.nonzero(torch.rand(P, generator=g) < 0.25)[:, 0]
    ca = torch.randint(0, K - 1, (tie.numel(),), generator=g)
    cb = ca + 1 + (torch.rand(tie.numel(), generator=g) * (K - 1 - ca)).long()
    flat[tie, ca] = 40.0
    flat[tie, cb] = 40.0
    nanp = torch.nonzero(torch.rand(P, generator=g) < 0.002)[:, 0]
    flat[nanp, torch.randint(0, K, (nanp.numel(),), generator=g)] = NAN
    flat[nanp[::2], 0] = NAN
    xs = NhwcSlice(L, n, h, w, K, rup8(K) + 8, 8, dtype, flat.view(n, h, w, K))
    ys = NhwcSlice(L, n, h, w, 1, 4, 2, dtype)
    L.check(lib.isa_chan_argmax(xs.d(), ys.d(), L.stream_ptr()), "isa_chan_argmax")
    got = ys.get()[..., 0].float()
    ref = argmax_ref(xs.get().float()).float()
    bad = int((got != ref).sum())
    print("OUTERR chan_argmax K%-2d %-8s %dx%dx%d  mismatches %d of %d (ties %d, NaN pixels %d)"
          % (K, str(dtype)[6:], n, h, w, bad, P, tie.numel(), nanp.numel()))
    assert bad == 0
    assert ys.neighbours_unchanged() and xs.neighbours_unchanged()


def boundary_source(n, c, h, w, seed):
    """NCHW fp32 with round-to-nearest-even ties of bf16 (1 + 2**-8, 1 + 3 * 2**-8 ...), -0, +-inf and a value that
    rounds to inf in bf16."""
    x = rand(n, c, h, w, seed=seed, scale=3.0)
    special = torch.tensor([1 + 2 ** -8, 1 + 3 * 2 ** -8, -(1 + 2 ** -8), 2 ** -8 * (256 + 1.5), -0.0, float("inf"),
                            float("-inf"), 3.4e38, 1e-3 * (1 + 2 ** -8)])
    flat = x.reshape(-1)
    k = min(flat.numel(), special.numel())
    flat[:k] = special[:k]
    flat[-k:] = special[:k]
    return x


def _convert(L, lib, src_nchw, t, offset_floats=0):
    """isa_nchw_to_nhwc of src (csrc = its channels) into the IsaTensor t; offset_floats > 0: the source pointer offset
    by that many floats inside a larger allocation (the element kernel)."""
    n, csrc, h, w = src_nchw.shape
    base = torch.full((offset_floats + src_nchw.numel(),), NAN, device="cuda")
    base[offset_floats:] = src_nchw.reshape(-1).cuda()
    rc = lib.isa_nchw_to_nhwc(C.c_void_p(base.data_ptr() + 4 * offset_floats), csrc, C.byref(t), L.stream_ptr())
    L.check(rc, "isa_nchw_to_nhwc")
    torch.cuda.synchronize()
    return base


def _expected_nhwc(src, c, dtype):
    n, csrc, h, w = src.shape
    ref = torch.zeros(n, h, w, c, dtype=dtype)
    ref[..., :csrc] = src.permute(0, 2, 3, 1).to(dtype)
    return ref


ROW_CASES = [  # c, csrc, n, h, w: ld == rup(c, 8) <= 32, h * w % 4 == 0, aligned: the row kernel
    (1, 1, 2, 24, 20),
    (3, 2, 3, 64, 44),          # 8448 pixels: 8 full 1024-pixel pieces and a partial one
    (8, 7, 2, 24, 20),
    (12, 11, 2, 8, 10),         # ld = 16: the one row width no other case takes
    (21, 20, 2, 16, 36),        # the network input (21 -> 24)
    (24, 21, 1, 12, 12),
    (32, 31, 3, 64, 44),
    (3, 3, 3, 1024, 704),       # 2 162 688 pixels: past the 2048-workgroup grid cap
]
ELEM_CASES = [  # c, csrc, n, h, w, ld, c0, src offset (floats): what sends it to the element kernel
    (21, 17, 2, 7, 9, 24, 0, 0),       # h * w % 4 != 0
    (8, 8, 2, 8, 8, 8, 0, 1),          # source pointer offset by one float
    (48, 40, 3, 64, 63, 48, 0, 0),     # more than 32 channels; 580 608 elements > the grid cap
    (24, 24, 2, 8, 8, 40, 8, 0),       # ld > rup(c, 8)
    (13, 11, 2, 4, 4, 24, 3, 0),       # unaligned data pointer (c0 = 3)
]


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c,csrc,n,h,w", ROW_CASES)
def test_nchw_to_nhwc_rows(dtype, c, csrc, n, h, w):
    """Row kernel: channels < csrc bit-exact (bf16 = RNE), [csrc, ld) written as 0 - the padded channels at or above
    c included; nothing after the tensor is written.  Then isa_nhwc_to_nchw brings the c channels back bit-exactly."""
    L, lib = _lib()
    cp = rup8(c)
    numel = n * h * w * cp
    flat = torch.full((numel + 1024,), NAN, dtype=dtype, device="cuda")
    t = L.IsaTensor(flat.data_ptr(), n, h, w, c, cp, L.dtype_code(dtype), 1)
    src = boundary_source(n, csrc, h, w, seed=c * 3 + h)
    _convert(L, lib, src, t)
    got = flat[:numel].view(n, h, w, cp).cpu()
    ref = torch.zeros(n, h, w, cp, dtype=dtype)
    ref[..., :c] = _expected_nhwc(src, c, dtype)
    assert _bits_equal(got, ref), int((_bits(got) != _bits(ref)).sum())
    assert bool(torch.isnan(flat[numel:]).all())
    _round_trip(L, lib, t, got[..., :c], n, c, h, w)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c,csrc,n,h,w,ld,c0,off", ELEM_CASES)
def test_nchw_to_nhwc_elements(dtype, c, csrc, n, h, w, ld, c0, off):
    """Element kernel: channels < csrc bit-exact (bf16 = RNE), [csrc, c) written as 0, every channel outside [0, c) of
    the slice left alone (NaN neighbours bit-unchanged).  Then the round trip through isa_nhwc_to_nchw."""
    L, lib = _lib()
    dst = NhwcSlice(L, n, h, w, c, ld, c0, dtype)
    src = boundary_source(n, csrc, h, w, seed=c * 5 + w)
    _convert(L, lib, src, dst.t, offset_floats=off)
    got = dst.get()
    assert _bits_equal(got, _expected_nhwc(src, c, dtype)), int((_bits(got) != _bits(_expected_nhwc(src, c, dtype))).sum())
    assert dst.neighbours_unchanged()
    _round_trip(L, lib, dst.t, got, n, c, h, w)


def _round_trip(L, lib, t, stored, n, c, h, w):
    numel = n * c * h * w
    out = torch.full((numel + 512,), NAN, device="cuda")
    L.check(lib.isa_nhwc_to_nchw(C.byref(t), L.ptr(out), L.stream_ptr()), "isa_nhwc_to_nchw")
    back = out[:numel].view(n, c, h, w).cpu()
    assert _bits_equal(back, stored.float().permute(0, 3, 1, 2))
    assert bool(torch.isnan(out[numel:]).all())


# ---------------------------------------------------------------------------------------------------------------------
# model level: semantic-only ReSeg(K) in eval mode against the float64 oracle
# ---------------------------------------------------------------------------------------------------------------------
def k_class_sd(K, seed=77):
    sd = R.synth_state_dict(23, use_instance_seg=False)
    rs = np.random.RandomState(seed + K)
    sd["sem_seg_output.weight"] = torch.from_numpy((rs.standard_normal((K, 32, 1, 1)) * 0.25).astype(np.float32))
    sd["sem_seg_output.bias"] = torch.from_numpy(rs.uniform(-0.1, 0.1, K).astype(np.float32))
    return sd


@gpu
@pytest.mark.parametrize("K", [5, 21])
def test_k_class_eval_forward_matches_float64(K):
    """ReSeg(K, use_instance_seg=False).eval() forward: logits within 1e-4 of max |ref| of reseg_forward in float64,
    and the arg-max map (isa_chan_argmax) equal to the reference's except where its two top logits are within fp32
    rounding (assert_index_map)."""
    _gpu()
    from isa_amd.reseg import ReSeg
    sd = k_class_sd(K)
    x = R.synth_batch(2, 64, 64, seed=4)[0]
    m = ReSeg(K, use_instance_seg=False, dtype=torch.float32)
    m.load_state_dict(sd)
    m.eval()
    sem_out, sem_argmax = m(False, x)
    torch.cuda.synchronize()
    got, amap = sem_out.double().cpu(), sem_argmax.cpu()
    with torch.no_grad():
        ref = R.reseg_forward({k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}, x.double(),
                              use_instance_seg=False, ctx=R.Ctx())["sem_out"]
    err = float((got - ref).abs().max() / ref.abs().max())
    print("OUTERR ReSeg(%d) eval logits rel err %.2e (bound %.0e)" % (K, err, LOGIT_BOUND))
    assert got.shape == ref.shape == (2, K, 64, 64) and err <= LOGIT_BOUND
    top2 = torch.topk(ref, 2, dim=1).values
    assert_index_map(ref.argmax(1).numpy(), amap[:, 0].long().numpy(), (top2[:, 0] - top2[:, 1]).numpy(),
                     float(ref.abs().max()), "ReSeg(%d) arg-max map" % K)
