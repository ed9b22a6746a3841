"""GPU: the stable segmented radix sort (isa_segsort_kv_u32), the Lovasz-Softmax kernels built on it (isa_lovasz_*) and
the trainer wired to them (criteria "Lovasz" and "CELovasz").

Sort: keys and values must EQUAL torch.sort(stable=True) of the same keys on the CPU; values are the indices, so stability
is checked exactly.  Loss kernels: the yardstick is the float64 restatement of tests/lovasz_np.py (pinned to the reference
by tests/test_lovasz_ref.py) on the logits the kernel sees, with the bounds of tests/test_gpu_sem_criterion.py: loss
<= 1e-5 relative, gradient <= 1e-5 relative L2 for fp32 logits and <= 8e-3 for bf16 logits (gradient stored in bf16).  The
gradient yardstick takes the device's own order, injected into the restatement AFTER that order has been checked exactly
against the stable sort of the device's keys and the keys against the restatement's errors (1e-6 absolute): a flip between
two errors that differ in the last fp32 bit then cannot blur the bound."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import lovasz_np as R64  # noqa: E402
from test_sem_criterion_ref import criterion  # noqa: E402

ONE_BITS = 0x3F800000
SENTINEL = 0x5A5A5A5A
PAD = 64


def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    return L


def _rup8(k):
    return (k + 7) // 8 * 8


def _u32(a):
    """numpy uint32 -> int32 torch tensor with the same bits, on the device."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _np_u32(t):
    return t.cpu().numpy().view(np.uint32)


def _rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ------------------------------------------------------------------------------------------------------------ the sort
def _device_sort(L, keys, nseg, seglen, b0, b1):
    """Sorted (keys, values) of numpy uint32 keys [nseg, seglen], values = index in the segment; the outputs carry a
    sentinel tail that must come back untouched."""
    n = nseg * seglen
    T = L.SEGSORT_TILE
    vals = np.tile(np.arange(seglen, dtype=np.uint32), nseg)
    ki, vi = _u32(keys.reshape(-1)), _u32(vals)
    ko = torch.full((n + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    vo = torch.full((n + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    kt, vt = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    table = torch.empty(L.segsort_table_elems(nseg, seglen), dtype=torch.int32, device="cuda")
    L.check(L.lib().isa_segsort_kv_u32(L.ptr(ki), L.ptr(vi), L.ptr(ko), L.ptr(vo), nseg, seglen, b0, b1, L.ptr(kt), L.ptr(vt),
                                       L.ptr(table), table.numel(), L.stream_ptr()), "isa_segsort_kv_u32")
    torch.cuda.synchronize()
    assert np.array_equal(_np_u32(ki), keys.reshape(-1)), "the input keys must stay as they are"
    assert bool((ko[n:] == SENTINEL).all()) and bool((vo[n:] == SENTINEL).all()), "wrote past the end of the output"
    return _np_u32(ko[:n]).reshape(nseg, seglen), _np_u32(vo[:n]).reshape(nseg, seglen)


def _key_sets(rs, nseg, seglen):
    shape = (nseg, seglen)
    full = rs.randint(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
    yield "random", full
    yield "all-equal", np.full(shape, 0x2F0F1E3C, dtype=np.uint32)
    yield "two-valued", np.where(rs.randint(0, 2, size=shape) == 1, 0x3F800000, 0x00000001).astype(np.uint32)
    yield "top-byte", ((full & np.uint32(0xFF)) << np.uint32(24)) | np.uint32(0x00ABCDEF)
    yield "low-byte", (full & np.uint32(0xFF)) | np.uint32(0x12345600)


def _sort_sizes():
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    T = L.SEGSORT_TILE
    sizes = [(1, 1), (1, 63), (3, 64), (2, 65), (5, T - 1), (4, T), (3, T + 1), (2, 3 * T + 5), (96, 561)]
    # Internal thresholds of the implementation:
    #   - a tile is T keys and a wave owns T/4 of it in rounds of 64 (the sizes above sit on both sides of each);
    #   - the digit table is scanned in chunks of 2048 entries = 8 tiles of 256 digits, one workgroup each: 4T+3 keys are
    #     5 tiles (part of one chunk), 8T exactly one chunk, 9T+1 two, 70T+9 nine with a partial last one;
    #   - the chunk sums (and the Lovasz tile counts) are scanned by one workgroup per segment, 1024 entries a trip with
    #     a carried total: 1024 chunks are 2^24 keys, too many for a quick test of the sort, so that carry is exercised
    #     through the same kernel by test_large_batch_wide_segments[1026-tiles].
    sizes += [(2, 4 * T + 3), (3, 8 * T), (2, 9 * T + 1), (2, 70 * T + 9)]
    return sizes


@pytest.mark.parametrize("nseg,seglen", _sort_sizes())
def test_segsort_equals_the_stable_cpu_sort(nseg, seglen):
    L = _lib()
    rs = np.random.RandomState(nseg * 7919 + seglen)
    for name, keys in _key_sets(rs, nseg, seglen):
        for b0, b1 in ((0, 32), (0, 30)):
            mask = (1 << (b1 - b0)) - 1
            part = torch.from_numpy(((keys.astype(np.int64) >> b0) & mask))
            order = torch.sort(part, dim=1, stable=True).indices.numpy()
            gk, gv = _device_sort(L, keys, nseg, seglen, b0, b1)
            tag = (name, b0, b1)
            assert np.array_equal(gv, order.astype(np.uint32)), tag
            assert np.array_equal(gk, np.take_along_axis(keys, order, 1)), tag
            gk2, gv2 = _device_sort(L, keys, nseg, seglen, b0, b1)
            assert np.array_equal(gk, gk2) and np.array_equal(gv, gv2), ("two runs differ", tag)


def test_segsort_middle_bit_range():
    """A bit range that starts above 0 and ends off a digit boundary: bits [5, 18) alone decide the order."""
    L = _lib()
    rs = np.random.RandomState(2)
    keys = rs.randint(0, 1 << 32, size=(3, 777), dtype=np.uint64).astype(np.uint32)
    part = torch.from_numpy((keys.astype(np.int64) >> 5) & ((1 << 13) - 1))
    order = torch.sort(part, dim=1, stable=True).indices.numpy()
    gk, gv = _device_sort(L, keys, 3, 777, 5, 18)
    assert np.array_equal(gv, order.astype(np.uint32)) and np.array_equal(gk, np.take_along_axis(keys, order, 1))


# --------------------------------------------------------------------------------------------------- the loss kernels
def _desc(L, buf, n, h, w, c, dtype):
    return L.IsaTensor(buf.data_ptr(), n, h, w, c, buf.shape[-1], L.dtype_code(dtype), 1)


def _cfg(bg, present, K):
    return torch.tensor([0.0, 0.0, float(bg), float(present)] + [1.0] * K, dtype=torch.float32, device="cuda")


def _inputs(B, K, H, W, dtype, seed, absent=None, background_image=None):
    """NHWC logits with NaN in the ld padding (must never be read), labels uint8, the float64 logits the kernels actually
    see (NCHW) and the labels as int64 numpy.  As tests/test_gpu_sem_criterion.py: randn * 2.5."""
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(B, H, W, K, generator=g, dtype=torch.float64) * 2.5
    lg[..., 0] += 0.5
    buf = torch.full((B, H, W, _rup8(K)), float("nan"), dtype=dtype)
    buf[..., :K] = lg.to(dtype)
    seen = buf[..., :K].double().permute(0, 3, 1, 2).contiguous().numpy()
    lab = torch.randint(0, K, (B, H, W), generator=g, dtype=torch.int64)
    if absent is not None:
        lab[lab == absent] = 0
    if background_image is not None:
        lab[background_image] = 0
    return buf.cuda(), lab.to(torch.uint8).cuda(), seen, lab.numpy()


class Sorted:
    """keys -> sort -> coefficients of all K classes in one group: everything the flag combinations share."""

    def __init__(self, L, buf, lab, B, K, H, W, dtype, per_image, backward=True):
        lib, s, T = L.lib(), L.stream_ptr(), L.SEGSORT_TILE
        self.L, self.B, self.K, self.hw, self.per_image = L, B, K, H * W, int(per_image)
        self.nimg = B if per_image else 1
        self.seglen = B * H * W // self.nimg
        self.nseg = K * self.nimg
        self.ntiles = (self.seglen + T - 1) // T
        n = K * B * H * W
        dev = dict(device="cuda")
        self.x = _desc(L, buf, B, H, W, K, dtype)
        mk = lambda: torch.full((n,), SENTINEL, dtype=torch.int32, **dev)
        self.keys, self.vals, self.skeys, self.svals, kt, vt = mk(), mk(), mk(), mk(), mk(), mk()
        self.G = torch.zeros(self.nseg, dtype=torch.int32, **dev)
        table = torch.empty(L.segsort_table_elems(self.nseg, self.seglen), dtype=torch.int32, **dev)
        tcnt = torch.empty(self.nseg * self.ntiles, dtype=torch.int32, **dev)
        self.partial = torch.full((self.nseg * self.ntiles,), float("nan"), dtype=torch.float64, **dev)
        self.gpix = torch.full((n,), float("nan"), **dev) if backward else None
        L.check(lib.isa_lovasz_keys(C.byref(self.x), L.ptr(lab), 0, K, self.per_image, L.ptr(self.keys), L.ptr(self.vals),
                                    L.ptr(self.G), s), "keys")
        L.check(lib.isa_segsort_kv_u32(L.ptr(self.keys), L.ptr(self.vals), L.ptr(self.skeys), L.ptr(self.svals), self.nseg,
                                       self.seglen, 0, 30, L.ptr(kt), L.ptr(vt), L.ptr(table), table.numel(), s), "sort")
        L.check(lib.isa_lovasz_coef(L.ptr(self.skeys), L.ptr(self.svals), L.ptr(self.G), self.nseg, self.seglen, L.ptr(tcnt),
                                    L.ptr(self.partial), L.ptr(self.gpix), s), "coef")

    def finish(self, cfg, dx=None, acc=0, template=None):
        """assemble (+ grad into dx): (loss as a float32 tensor [1], scale [K, nimg], dx)."""
        L, lib, s = self.L, self.L.lib(), self.L.stream_ptr()
        segloss = torch.empty(self.nseg, dtype=torch.float64, device="cuda")
        scale = torch.full((self.nseg,), float("nan"), device="cuda")
        scal = torch.full((1,), float("nan"), device="cuda")
        L.check(lib.isa_lovasz_assemble(L.ptr(self.partial), L.ptr(self.G), L.ptr(cfg), self.B, self.K, self.per_image,
                                        self.hw, L.ptr(segloss), L.ptr(scale), L.ptr(scal), s), "assemble")
        if self.gpix is not None:
            if dx is None:
                dx = torch.full_like(template, float("nan"))
            d = L.IsaTensor(dx.data_ptr(), self.x.n, self.x.h, self.x.w, self.x.c, dx.shape[-1], self.x.dtype, 1)
            L.check(lib.isa_lovasz_grad(C.byref(self.x), L.ptr(self.gpix), L.ptr(scale), self.per_image, C.byref(d), acc, s),
                    "grad")
        torch.cuda.synchronize()
        return scal.cpu(), scale.cpu().view(self.K, self.nimg), dx

    def checked_orders(self, seen, lab_np):
        """The device's order [K, nimg, seglen] after it was held to the stable sort of the device's own keys, the keys to
        the restatement's errors, the flags to the labels and G to the foreground counts."""
        K, nimg, seglen = self.K, self.nimg, self.seglen
        keys = _np_u32(self.keys).reshape(K, nimg, seglen)
        vals = _np_u32(self.vals).reshape(K, nimg, seglen)
        skeys = _np_u32(self.skeys).reshape(K, nimg, seglen)
        svals = _np_u32(self.svals).reshape(K, nimg, seglen)
        _, err, fg = R64.segment_errors(seen, lab_np)
        err, fg = err.reshape(K, nimg, seglen), fg.reshape(K, nimg, seglen)
        assert keys.max() <= ONE_BITS
        dev_err = (np.uint32(ONE_BITS) - keys).view(np.float32).astype(np.float64)
        assert np.abs(dev_err - err).max() <= 1e-6
        assert np.array_equal(vals & 0x7FFFFFFF, np.broadcast_to(np.arange(seglen, dtype=np.uint32), vals.shape))
        assert np.array_equal(vals >> 31 == 1, fg)
        assert np.array_equal(self.G.cpu().numpy().reshape(K, nimg), fg.sum(2))
        order = torch.sort(torch.from_numpy(keys.astype(np.int64)), dim=2, stable=True).indices.numpy()
        assert np.array_equal(svals & 0x7FFFFFFF, order.astype(np.uint32)), "the device order is not the stable sort of its keys"
        assert np.array_equal(skeys, np.take_along_axis(keys, order, 2))
        assert np.array_equal(svals >> 31 == 1, np.take_along_axis(fg, order, 2))
        return order


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K", [2, 3, 8, 12, 21, 32])       # every class width of the kernels: 8, 16, 24, 32
def test_loss_kernels_match_the_restatement(K, dtype):
    L = _lib()
    gbound = 1e-5 if dtype == torch.float32 else 8e-3
    worst_l = worst_g = 0.0
    # H*W = 540, 561: never a multiple of the tile.  The first shape has an all-background image 1, the second (K > 2)
    # has its last class deleted from the labels
    for B, H, W, absent, bgimg in ((3, 20, 27, None, 1), (16, 17, 33, K - 1 if K > 2 else None, None)):
        buf, lab, seen, lab_np = _inputs(B, K, H, W, dtype, seed=K * 100 + B, absent=absent, background_image=bgimg)
        if absent is not None:
            assert not (lab_np == absent).any()
        for per_image in (False, True):
            S = Sorted(L, buf, lab, B, K, H, W, dtype, per_image)
            S2 = Sorted(L, buf, lab, B, K, H, W, dtype, per_image)          # a second run: must be bit-identical
            torch.cuda.synchronize()
            order = S.checked_orders(seen, lab_np)
            for present in (False, True):
                for bg in (False, True):
                    tag = (K, B, per_image, present, bg)
                    scal, scale, dx = S.finish(_cfg(bg, present, K), template=buf)
                    ref = R64.lovasz_softmax(seen, lab_np, bg, present, per_image, orders=order)
                    got_l = float(scal[0])
                    el = abs(got_l - ref["loss"]) / max(abs(ref["loss"]), 1e-3)
                    got_g = dx[..., :K].double().permute(0, 3, 1, 2).cpu().numpy()
                    eg = _rel_l2(got_g, ref["grad"])
                    worst_l, worst_g = max(worst_l, el), max(worst_g, eg)
                    assert el <= 1e-5, (tag, got_l, ref["loss"])
                    assert eg <= gbound, (tag, eg)
                    assert torch.isnan(dx[..., K:]).all(), "the ld padding of d logits must stay untouched"
                    if bgimg is not None and per_image and present and not bg:
                        # no counted class in the all-background image: it adds exactly 0 to loss and gradient
                        assert bool((scale[:, bgimg] == 0).all()) and bool((dx[bgimg, ..., :K] == 0).all()), tag
                        others = [b for b in range(B) if b != bgimg]
                        keep = (ref["G"][1:] > 0)
                        want = sum(ref["seg_loss"][1:, b][keep[:, b]].mean() for b in others if keep[:, b].any()) / B
                        assert abs(ref["loss"] - want) <= 1e-12
                    # bit-identical over two runs
                    scal2, _, dx2 = S2.finish(_cfg(bg, present, K), template=buf)
                    assert scal2.view(torch.int32).equal(scal.view(torch.int32)), tag
                    assert torch.equal(dx2[..., :K].view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                                       dx[..., :K].view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), tag
    print("K=%d %s: worst loss rel %.2e, worst gradient rel-L2 %.2e" % (K, dtype, worst_l, worst_g))


@pytest.mark.parametrize("B,H,W", [(16, 256, 256), (1, 1025, 2050)], ids=["2^20-per-segment", "1026-tiles"])
def test_large_batch_wide_segments(B, H, W):
    """fp32, K = 2, batch-wide: 2^20 elements a segment (jaccard[r] - jaccard[r-1] in fp32 is orders of magnitude off 1e-5
    there), and 1026 tiles a segment, past the 1024 tile counts one trip of the scan workgroup covers."""
    L = _lib()
    K, dtype = 2, torch.float32
    buf, lab, seen, lab_np = _inputs(B, K, H, W, dtype, seed=B + H)
    S = Sorted(L, buf, lab, B, K, H, W, dtype, False)
    torch.cuda.synchronize()
    order = S.checked_orders(seen, lab_np)
    scal, _, dx = S.finish(_cfg(True, False, K), template=buf)
    ref = R64.lovasz_softmax(seen, lab_np, True, False, False, orders=order)
    el = abs(float(scal[0]) - ref["loss"]) / abs(ref["loss"])
    eg = _rel_l2(dx[..., :K].double().permute(0, 3, 1, 2).cpu().numpy(), ref["grad"])
    print("B=%d %dx%d: loss rel %.2e, gradient rel-L2 %.2e" % (B, H, W, el, eg))
    assert el <= 1e-5 and eg <= 1e-5, (el, eg)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_grad_accumulates_and_forward_only(dtype):
    L = _lib()
    B, K, H, W = 2, 5, 9, 31
    buf, lab, seen, lab_np = _inputs(B, K, H, W, dtype, seed=7)
    cfg = _cfg(True, False, K)
    old = torch.randn(B, H, W, _rup8(K), generator=torch.Generator().manual_seed(3)).to(dtype).cuda()
    S = Sorted(L, buf, lab, B, K, H, W, dtype, True)
    loss, _, fresh = S.finish(cfg, template=buf)
    _, _, acc = S.finish(cfg, dx=old.clone(), acc=1)
    want = old[..., :K].float() + fresh[..., :K].float()
    tol = 1e-6 if dtype == torch.float32 else 1e-2
    assert float((acc[..., :K].float() - want).abs().max()) <= tol
    assert torch.equal(acc[..., K:], old[..., K:])
    fwd = Sorted(L, buf, lab, B, K, H, W, dtype, True, backward=False)      # gpix == NULL: the loss alone
    loss2, _, none = fwd.finish(cfg)
    assert none is None and loss2.view(torch.int32).equal(loss.view(torch.int32))


def test_class_groups_give_the_same_result(monkeypatch):
    """Network._lovasz_loss sorting the classes in groups (the scratch budget of DESIGN.md §13) equals one group."""
    L = _lib()
    from isa_amd import network as N
    from isa_amd.engine import Act
    from isa_amd.reseg import ReSeg
    K, B, H, W = 5, 2, 20, 27
    m = ReSeg(K, use_instance_seg=False, dtype=torch.float32)
    buf, lab, seen, lab_np = _inputs(B, K, H, W, torch.float32, seed=9)
    out = []
    for budget in (N.LOVASZ_SCRATCH_BYTES, 25 * 2 * B * H * W + 4 * K * B * H * W):       # all classes; groups of 2, 2, 1
        monkeypatch.setattr(N, "LOVASZ_SCRATCH_BYTES", budget)
        m.set_criterion("Lovasz", None, True)
        E = m.engine
        E.begin(bn_train=True, record=True, key=("lovasz-groups", budget))
        sem = Act(buf, 0, K)
        scal = m.net.sem_loss(sem, None, lab)
        bwd, _ = E.tape[-1]                                                # the criterion's backward closure
        bwd()
        torch.cuda.synchronize()
        out.append((scal.clone(), E.grads.grad_of(sem).buf.clone()))
    assert N.lovasz_class_group(K, B * H * W, True) == 2
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1][..., :K], out[1][1][..., :K])
    ref = R64.lovasz_softmax(seen, lab_np, True, False, False)
    assert abs(float(out[0][0][2]) - ref["loss"]) <= 1e-5 * ref["loss"] and float(out[0][0][0]) == 0.0
    assert _rel_l2(out[0][1][..., :K].double().permute(0, 3, 1, 2).cpu().numpy(), ref["grad"]) <= 1e-4


# ------------------------------------------------------------------------------------------------------- the trainer
def _need_model():
    _lib()
    import reseg_ref as R
    from isa_amd.reseg import ReSeg
    from isa_amd.trainer import Trainer
    from isa_amd.data import class_onehot
    return R, ReSeg, Trainer, class_onehot


def _three_class_sd(R):
    sd = R.synth_state_dict(23, use_instance_seg=False)
    rs = np.random.RandomState(77)
    sd["sem_seg_output.weight"] = torch.from_numpy((rs.standard_normal((3, 32, 1, 1)) * 0.25).astype(np.float32))
    sd["sem_seg_output.bias"] = torch.from_numpy(rs.uniform(-0.1, 0.1, 3).astype(np.float32))
    return sd


def _torch_lovasz(logits, labels, bg, present, per_image, orders=None):
    """The restatement in torch (autograd carries it back through the oracle network), in the logits' dtype.  `orders`
    [K, nimg, seglen]: the sorted order of every segment, in place of the stable descending sort of the errors."""
    B, K = logits.shape[:2]
    p = torch.softmax(logits, 1).reshape(B, K, -1)
    lab = labels.reshape(B, -1)
    nimg = B if per_image else 1
    total = 0
    for s in range(nimg):
        terms = []
        for c in range(0 if bg else 1, K):
            pc = (p[s, c] if per_image else p[:, c].reshape(-1))
            fg = ((lab[s] if per_image else lab.reshape(-1)) == c)
            if present and not bool(fg.any()):
                continue
            e = (fg.to(pc.dtype) - pc).abs()
            if orders is None:
                order = torch.sort(e.detach(), stable=True, descending=True).indices
            else:
                order = torch.from_numpy(np.ascontiguousarray(orders[c][s]))
            g = torch.from_numpy(R64.coefficients(fg[order].numpy())).to(pc.dtype)
            terms.append((e[order] * g).sum())
        if terms:
            total = total + sum(terms) / len(terms)
    return total / nimg


# ReLU6 inputs of the float64 oracle closer than this to 0 or 6 are undecided for an fp32 forward: a BatchNorm output
# (x - mean) * scale + shift of magnitude up to 6 carries half an ulp, 2.4e-7, from each of its four roundings (the input,
# the subtraction, the product, the sum), 1e-6 in all.
RELU6_UNDECIDED = 1e-6


class _Relu6OneSided(torch.autograd.Function):
    """clamp(z, 0, 6) whose derivative at the listed flat indices is the OTHER one-sided value."""

    @staticmethod
    def forward(ctx, z, idx):
        mask = (z > 0) & (z < 6)
        flat = mask.view(-1)
        flat[idx] = ~flat[idx]
        ctx.save_for_backward(mask)
        return torch.clamp(z, 0.0, 6.0)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0].to(g.dtype), None


@pytest.mark.parametrize("crit,bg,present,per_image", [("Lovasz", True, False, False), ("CELovasz", False, True, True)])
def test_three_class_step_matches_float64_autograd(crit, bg, present, per_image, monkeypatch):
    """A 3-class train step at 64 x 64, B = 2, against float64 autograd through the oracle network; the pattern and the
    bounds (worst tensor 1e-4, median 1e-5 relative L2) of test_gpu_sem_criterion.test_three_class_step_matches_float64_autograd.
    The Lovasz gradient depends on the ORDER of the errors, and an fp32 forward orders near-ties differently from a
    float64 one, so the test measures the oracle's own floor, the same network and criterion in fp32 on the CPU against
    float64; where a third of a bound is below that floor, the bound becomes 4x the floor.  Each side sorts its own errors.

    One thing the backbone adds.  With these weights and this input the float64 oracle has a ReLU6 input 2.8e-7 from a
    threshold (base.up3.conv.conv.down_conv_1.conv.1, image 1, channel 45, pixel (11, 1)) and one 4.6e-7 from it in the
    first block; the next is 1.2e-6 away.  An fp32 forward, whose BatchNorm sums are float atomics, decides such an
    element either way from run to run, and the derivative of ReLU6 there is 0 or 1.  In float64, taking the other side
    at the first element alone moves that BatchNorm's bias gradient by 1.0e-3 and the median tensor by 2.1e-4 under
    `Lovasz` (7.5e-4 / 1.7e-4 under `CELovasz`, 1.3e-3 / 3.3e-4 under plain CE): ten times the bounds, and exactly what a
    device step shows when it lands on the other side.  Neither side is wrong.  So the reference is float64 autograd with
    either one-sided derivative at the inputs within RELU6_UNDECIDED of a threshold: the oracle runs once per choice (at
    most 8), the fp32 floor is taken against the nearest choice, and so is the device's step; bounds and floor rule stay."""
    R, ReSeg, Trainer, class_onehot = _need_model()
    x, _, ins, n = R.synth_batch(2, 64, 64, seed=1)
    sem = class_onehot(ins, 3)
    labels = sem.argmax(1)
    sd = _three_class_sd(R)
    m = ReSeg(3, use_instance_seg=False, dtype=torch.float32)
    m.load_state_dict(sd)
    m.train()
    tr = Trainer(m, criterion=crit, optimize_bg=bg, lovasz_per_image=per_image, lovasz_only_present=present)
    out = tr.forward_backward(x, sem, ins, n)
    logits = m.net.to_nchw(m._last_sem).double().cpu()
    scal = out["sem"].double().cpu()
    torch.cuda.synchronize()
    assert scal.numel() == 3 and float(scal[1]) == 0.0

    plain_relu6 = R.relu6
    state = dict(inputs=[], other_side={})

    def relu6(z):
        call = len(state["inputs"])
        state["inputs"].append(z.detach())
        idx = state["other_side"].get(call)
        return plain_relu6(z) if idx is None else _Relu6OneSided.apply(z, torch.tensor(idx))

    monkeypatch.setattr(R, "relu6", relu6)

    def oracle(dt, other_side):
        state["inputs"], state["other_side"] = [], other_side
        P = {k: (v.to(dt).clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v)
             for k, v in sd.items()}
        ref = R.reseg_forward(P, x.to(dt), sem, use_instance_seg=False, ctx=R.Ctx(bn_train=True, training=True))
        lref = ref["sem_out"]
        cost = _torch_lovasz(lref, labels, bg, present, per_image)
        if crit == "CELovasz":
            cost = cost + torch.nn.functional.cross_entropy(lref.permute(0, 2, 3, 1).reshape(-1, 3), labels.reshape(-1))
        cost.backward()
        return {k: v.grad.double() for k, v in P.items() if getattr(v, "grad", None) is not None}, lref.detach()

    def rel_errors(got, ref):
        gmax = max(float(v.norm()) for v in ref.values())
        return {k: float((got(k) - v).norm() / v.norm()) for k, v in ref.items() if float(v.norm()) > 1e-6 * gmax}

    g64, lref = oracle(torch.float64, {})
    undecided = []
    for call, z in enumerate(state["inputs"]):
        near = torch.nonzero(torch.minimum(z.abs(), (z - 6).abs()).view(-1) < RELU6_UNDECIDED).view(-1)
        undecided += [(call, int(i)) for i in near]
    assert len(undecided) <= 3, undecided
    choices = [g64]
    for pick in range(1, 1 << len(undecided)):
        sides = {}
        for bit, (call, i) in enumerate(undecided):
            if pick >> bit & 1:
                sides.setdefault(call, []).append(i)
        choices.append(oracle(torch.float64, sides)[0])
    g32, _ = oracle(torch.float32, {})
    assert float((logits - lref).abs().max()) <= 1e-4 * float(lref.abs().max())
    want = R64.lovasz_softmax(lref.numpy(), labels.numpy(), bg, present, per_image)["loss"]
    assert abs(float(scal[2]) - want) < 1e-4
    if crit == "CELovasz":
        ce, _ = criterion(lref.numpy(), labels.numpy(), "CE", None, False)
        assert abs(float(scal[0]) - ce) < 1e-4
    else:
        assert float(scal[0]) == 0.0

    def nearest(got):
        """(worst, its tensor, median, number of tensors, choice) against the nearest one-sided choice."""
        best = None
        for pick, ref in enumerate(choices):
            e = rel_errors(got, ref)
            w = max(e, key=e.get)
            cand = (e[w], w, float(np.median(list(e.values()))), len(e), pick)
            best = cand if best is None or cand[0] < best[0] else best
        return best

    fworst, _, fmed, _, fpick = nearest(lambda k: g32[k])
    eworst, worst, med, nt, pick = nearest(lambda k: m.store.gview(k).double().cpu())
    assert nt > 100 and "sem_seg_output.weight" in g64
    bworst = 1e-4 if 1e-4 / 3 >= fworst else 4 * fworst
    bmed = 1e-5 if 1e-5 / 3 >= fmed else 4 * fmed
    print("3-class %s step vs float64: %d tensors, %d undecided ReLU6 inputs %s, device nearest to choice %d, fp32 oracle to %d; "
          "worst rel-L2 %.2e (%s), median %.2e; oracle fp32 floor worst %.2e, median %.2e; bounds %.2e / %.2e"
          % (crit, nt, len(undecided), undecided, pick, fpick, eworst, worst, med, fworst, fmed, bworst, bmed))
    assert eworst <= bworst and med <= bmed, (worst, eworst, med, bworst, bmed)


def test_graph_replay_of_a_celovasz_step():
    """train_step_graphed captures a CELovasz step (fixed launch count, no host read); a replay matches an eager step from
    the same parameters within the 2e-2 of test_gpu_train.test_graph_replayed_step_matches_eager_step; optimize_bg
    flipped in place in the criterion's buffer reaches the replay."""
    R, ReSeg, Trainer, class_onehot = _need_model()
    x, _, ins, n = R.synth_batch(2, 64, 64, seed=2)
    sem = class_onehot(ins, 3)
    m = ReSeg(3, use_instance_seg=False, dtype=torch.float32)
    m.load_state_dict(_three_class_sd(R))
    m.train()
    tr = Trainer(m, criterion="CELovasz")
    cfg = m.net.crit.cfg
    tr.train_step_graphed(x, sem, ins, n)                    # eager (configuration recorded)
    tr.train_step_graphed(x, sem, ins, n)                    # captured, replayed
    assert tr._graphs and list(tr._graphs.values())[0]["state"] == "ready"
    snap = m.store.flat.clone()
    out = tr.train_step_graphed(x, sem, ins, n)["sem"].clone()
    grad_graph = m.store.grad[:m.store.n_train].clone()
    m.store.flat.copy_(snap)
    m.mark_weights_dirty()
    eager = tr.forward_backward(x, sem, ins, n)["sem"].clone()
    grad_eager = m.store.grad[:m.store.n_train].clone()
    torch.cuda.synchronize()
    assert out.numel() == 3 and float(out[1]) == 0.0
    assert abs(float(out[0]) - float(eager[0])) <= 1e-5 * abs(float(eager[0]))
    assert abs(float(out[2]) - float(eager[2])) <= 1e-5 * abs(float(eager[2]))
    d = float((grad_graph - grad_eager).norm() / grad_eager.norm())
    assert d <= 2e-2, d
    # optimize_bg in place: background joins the counted classes of the replayed step
    m.store.flat.copy_(snap)
    m.mark_weights_dirty()
    cfg[2] = 1.0
    flipped = tr.train_step_graphed(x, sem, ins, n)["sem"].clone()
    grad_flipped = m.store.grad[:m.store.n_train].clone()
    m.store.flat.copy_(snap)
    m.mark_weights_dirty()
    eager_bg = tr.forward_backward(x, sem, ins, n)["sem"].clone()
    grad_eager_bg = m.store.grad[:m.store.n_train].clone()
    torch.cuda.synchronize()
    assert abs(float(flipped[2]) - float(eager_bg[2])) <= 1e-5 * abs(float(eager_bg[2]))
    assert abs(float(flipped[2]) - float(out[2])) > 100 * abs(float(flipped[2]) - float(eager_bg[2])) + 1e-4
    d_bg = float((grad_flipped - grad_eager_bg).norm() / grad_eager_bg.norm())
    d_old = float((grad_flipped - grad_eager).norm() / grad_eager.norm())
    assert d_bg <= 2e-2 and d_old > 10 * d_bg, (d_bg, d_old)


def test_instance_model_with_celovasz_and_validation_costs():
    """K = 2 with the instance head: the head is independent of the semantic criterion; sem_costs (forward only) returns
    the same three costs without launching gradient kernels."""
    R, ReSeg, Trainer, _ = _need_model()
    x, sem, ins, n = R.synth_batch(2, 64, 64, seed=3)
    m = ReSeg(2, True, dtype=torch.float32)
    m.load_state_dict(R.synth_state_dict(23, True))
    m.train()
    m.head.drop_rate = 0.0
    tr = Trainer(m, criterion="CELovasz", lovasz_per_image=True)
    assert not m.net.crit.legacy
    out = tr.forward_backward(x, sem, ins, n)
    logits = m.net.to_nchw(m._last_sem).double().cpu().numpy()
    scal = out["sem"].double().cpu().numpy()
    again = m.sem_costs(sem).double().cpu().numpy()
    head = out["head"].cpu()
    torch.cuda.synchronize()
    labels = sem.argmax(1).numpy()
    ce, _ = criterion(logits, labels, "CE", None, False)
    lov = R64.lovasz_softmax(logits, labels, False, False, True)["loss"]
    assert scal.shape == (3,) and abs(scal[0] - ce) <= 1e-5 * ce and scal[1] == 0.0 and abs(scal[2] - lov) <= 1e-5 * lov
    # the Lovasz term is bit-reproducible; the CE sums of isa_sem_loss_k_sums are float atomics (a few ulp from run to run)
    assert again.shape == (3,) and again[2] == scal[2] and again[1] == 0.0 and abs(again[0] - scal[0]) <= 1e-6 * scal[0]
    assert torch.isfinite(head[1:]).all() and torch.isfinite(m.store.grad[:m.store.n_train]).all()


def test_shipped_criteria_are_unchanged():
    R, ReSeg, Trainer, class_onehot = _need_model()
    shipped = Trainer(ReSeg(2, use_instance_seg=False))       # the shipped criterion keeps its 2-class kernels
    assert shipped.model.net.crit.legacy and not shipped.model.net.crit.lovasz
    x, _, ins, n = R.synth_batch(2, 64, 64, seed=1)
    sem = class_onehot(ins, 3)
    m = ReSeg(3, use_instance_seg=False, dtype=torch.float32)
    m.load_state_dict(_three_class_sd(R))
    m.train()
    tr = Trainer(m, criterion="Multi")
    out = tr.forward_backward(x, sem, ins, n)
    logits = m.net.to_nchw(m._last_sem).double().cpu().numpy()
    scal = out["sem"].double().cpu().numpy()
    torch.cuda.synchronize()
    assert scal.shape == (2,)
    ce, dice = criterion(logits, sem.argmax(1).numpy(), "Multi", None, False)
    assert abs(scal[0] - ce) <= 1e-5 * ce and abs(scal[1] - dice) <= 1e-5 * dice
