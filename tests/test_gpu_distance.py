"""The distance transform to the two nearest instances on the GPU: isa_edt2_u8, isa_border_weights, isa_fill_labels and the
ReSeg methods over them.

d1sq, d2sq, nearest, the filled map and the fill counts are integers and are compared EXACTLY with the restatement
tests/distance_np.py (which tests/test_distance_ref.py checks against per-instance scipy EDT and hand-written answers).

Shapes and the geometry they meet.  The column pass gives one lane a column and a workgroup ISA_EDT_COL_LANES = 64 columns
over the full height, read 8 rows at a time; the row pass gives one workgroup a row, with min(ISA_EDT_ROW_LANES = 256, w
rounded up to 64) lanes and 8 w + 16 bytes of LDS.
  4 x 4, 8 x 12   one partial column workgroup (4 and 12 of 64 lanes), a partial 8-row group at 4 rows; row workgroups of
                  64 lanes with 60 and 52 idle;
  72 x 136        3 column workgroups, the last with 8 of 64 lanes; 9 groups of 8 rows exactly; row workgroups of 192
                  lanes with 56 idle - no multiple of 64 or 256 in x, and n = 1;
  64 x 64         n = 1 and n = 3: one full column workgroup per image, row workgroups of 64 lanes, all busy;
  256 x 256       n = 2: 4 column workgroups, row workgroups of 256 lanes, one pixel per lane;
  512 x 512       n = 1, one test: two pixels per lane in the row pass; squared distances past 2^16, column distances
                  past 2^8.
Every output sits between sentinel pads that must stay unchanged, and the scratch is pre-filled with 0xAB."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import distance_np as dn        # noqa: E402
from test_gpu_ops import _gpu   # noqa: E402

PAD = 64                        # elements of padding on either side of every output (keeps 16-byte alignment)
SHAPES = [(1, 4, 4), (1, 8, 12), (1, 72, 136), (1, 64, 64), (3, 64, 64), (2, 256, 256)]
INF = dn.INF


def _lib():
    L = _gpu()[0]
    return L, L.lib()


class Padded:
    """`shape` elements between two runs of PAD sentinel elements."""

    def __init__(self, shape, dtype, fill):
        self.numel, self.fill = int(np.prod(shape)), fill
        self.buf = torch.full((self.numel + 2 * PAD,), fill, dtype=dtype, device="cuda")
        self.view = self.buf[PAD:PAD + self.numel].view(shape)

    def host(self):
        b = self.buf.cpu()
        assert bool((b[:PAD] == self.fill).all()) and bool((b[PAD + self.numel:] == self.fill).all()), "pads overwritten"
        return self.view.cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference(shape):
    """name -> (labels, (d1sq, d2sq, nearest)) of every case at `shape`, computed once and shared (read-only)."""
    out = {}
    for name, maps in dn.cases(*shape).items():
        res = dn.edt2(maps)
        for a in (maps,) + res:
            a.setflags(write=False)
        out[name] = (maps, res)
    return out


def dev_edt2(maps, want=(True, True, True)):
    """isa_edt2_u8 on a numpy uint8 map [n,h,w] -> numpy outputs (None where not wanted) and the device tensors."""
    L, lib = _lib()
    n, h, w = maps.shape
    t = torch.from_numpy(np.array(maps)).cuda()                # (a copy: the shared reference is read-only)
    d1 = Padded((n, h, w), torch.int32, -77) if want[0] else None
    d2 = Padded((n, h, w), torch.int32, -77) if want[1] else None
    near = Padded((n, h, w), torch.uint8, 0xEE) if want[2] else None
    scratch = torch.full((L.edt_scratch_bytes(n, h, w),), 0xAB, dtype=torch.uint8, device="cuda")      # need not be clear
    view = lambda p: None if p is None else p.view
    L.check(lib.isa_edt2_u8(L.ptr(t), n, h, w, L.ptr(view(d1)), L.ptr(view(d2)), L.ptr(view(near)), L.ptr(scratch),
                            scratch.numel(), L.stream_ptr()), "isa_edt2_u8")
    host = tuple(None if p is None else p.host() for p in (d1, d2, near))
    return host, (t, view(d1), view(d2), view(near))


def same(got, want, what, parts=("d1sq", "d2sq", "nearest")):
    for g, w_, part in zip(got, want, parts):
        g, w_ = np.asarray(g), np.asarray(w_)
        assert g.shape == w_.shape and g.dtype == w_.dtype, (what, part, g.shape, w_.shape, g.dtype, w_.dtype)
        bad = np.argwhere(g != w_)
        assert bad.size == 0, "%s: %s differs at %d places, first %s: got %s want %s" % (
            what, part, len(bad), bad[0].tolist(), g[tuple(bad[0])], w_[tuple(bad[0])])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_transform_is_exact_on_every_case(shape):
    """Random blobs of 1, 2 and 12 labels, an empty map, one instance, a fully labelled map, labels 1 and 255 in opposite
    corners (the answer lies at the full diagonal: a pruning window that is too small fails) and the two-label
    checkerboard (ties everywhere)."""
    ref = reference(shape)
    assert set(ref) == {"blobs1", "blobs2", "blobs12", "empty", "one", "full", "corners", "checker"}
    for name, (maps, want) in ref.items():
        got, _ = dev_edt2(maps)
        same(got, want, "%s %s" % (shape, name))
    d1, d2, near = ref["corners"][1]
    n, h, w = shape
    assert d2[0, 0, 0] == (h - 1) ** 2 + (w - 1) ** 2 and near[0, h - 1, w - 1] == 255
    d1, d2, near = ref["one"][1]
    assert (d2 == INF).all() and (near == 7).all() and (d1 != INF).all()
    d1, d2, near = ref["empty"][1]
    assert (d1 == INF).all() and (d2 == INF).all() and (near == 0).all()
    d1, d2, near = ref["checker"][1]
    assert ((d1 == d2) & (d1 > 0)).any()


def test_any_output_may_be_null_and_two_runs_are_bit_identical():
    maps, want = reference((1, 72, 136))["blobs12"]
    full, _ = dev_edt2(maps)
    again, _ = dev_edt2(maps)
    same(again, full, "second run")
    for k in range(3):
        only = tuple(i == k for i in range(3))
        got, _ = dev_edt2(maps, only)
        assert [g is None for g in got] == [not o for o in only]
        same((got[k],), (want[k],), "only output %d" % k, parts=(("d1sq", "d2sq", "nearest")[k],))


def test_512_two_pixels_need_32_bit_squares_and_wide_column_distances():
    """One labelled pixel at (0,0) and one at (511,0): the squared distances reach 511^2 + 511^2 = 522 242 (past 16 bits)
    and the column distances 511 (past 8 bits)."""
    maps = np.zeros((1, 512, 512), np.uint8)
    maps[0, 0, 0], maps[0, 511, 0] = 3, 200
    want = dn.edt2(maps)
    assert want[1].max() == 522242 and want[1][0, 0, 511] == 522242 and want[0][0, 255, 0] == 255 ** 2
    got, _ = dev_edt2(maps)
    same(got, want, "512 x 512")


@pytest.mark.parametrize("shape", [(1, 8, 12), (1, 72, 136), (3, 64, 64)], ids=lambda s: "%dx%dx%d" % s)
def test_fill_is_exact_with_and_without_a_limit(shape):
    L, lib = _lib()
    n, h, w = shape
    rng = np.random.default_rng(11)
    fg = (rng.random(shape) < 0.7).astype(np.uint8) * rng.integers(1, 256, size=shape).astype(np.uint8)   # any non-zero value
    fg_dev = torch.from_numpy(fg).cuda()
    for name in ("blobs12", "blobs2", "empty", "full", "checker", "corners"):
        maps, (d1, _, near) = reference(shape)[name]
        _, (t, d1_dev, _, near_dev) = dev_edt2(maps)
        for max_dist in (None, 0, 3):
            bound = dn.max_dist_sq(max_dist)
            out, filled = Padded(shape, torch.uint8, 0xEE), Padded((n,), torch.int32, -77)
            L.check(lib.isa_fill_labels(L.ptr(t), L.ptr(fg_dev), L.ptr(near_dev), L.ptr(d1_dev), bound, n, h * w,
                                        L.ptr(out.view), L.ptr(filled.view), L.stream_ptr()), "isa_fill_labels")
            want = dn.fill(maps, fg, near, d1, bound)
            same((out.host(), filled.host()), want, "%s %s max_dist %s" % (shape, name, max_dist), parts=("out", "filled"))
            if max_dist == 0:
                assert np.array_equal(want[0], maps) and not want[1].any()
            if max_dist is None and name.startswith("blobs"):
                assert want[1].all() and not ((want[0] == 0) & (fg != 0)).any()      # no foreground pixel is left at 0


@pytest.mark.parametrize("w0", [1.0, 10.0])
@pytest.mark.parametrize("sigma", [2.0, 5.0])
def test_border_weights_against_float64(w0, sigma):
    """|got - ref| <= 1e-6 (1 + w0): one fp32 rounding of a value up to 1 + w0 (6e-8 (1 + w0)), w0 max(a e^-a) = 0.37 w0 times
    the four roundings of the argument a (sqrt, sqrt, square, scale: 2.4e-7 relative) and a 2-ulp expf (1.2e-7 w0) - about
    3e-7 (1 + w0) in all."""
    L, lib = _lib()
    cfg = torch.tensor([w0, sigma], dtype=torch.float32, device="cuda")
    worst = 0.0
    for shape in [(1, 8, 12), (1, 72, 136), (3, 64, 64)]:
        n, h, w = shape
        for name in ("blobs2", "blobs12", "one", "empty", "full", "checker", "corners"):
            maps, (d1, d2, _) = reference(shape)[name]
            _, (t, d1_dev, d2_dev, _) = dev_edt2(maps)
            out = Padded(shape, torch.float32, -7.0)
            L.check(lib.isa_border_weights(L.ptr(t), L.ptr(d1_dev), L.ptr(d2_dev), L.ptr(cfg), n, h * w, L.ptr(out.view),
                                           L.stream_ptr()), "isa_border_weights")
            got, want = out.host().astype(np.float64), dn.border_weights(maps, d1, d2, w0, sigma)
            err = float(np.abs(got - want).max())
            worst = max(worst, err)
            assert err <= 1e-6 * (1 + w0), (shape, name, err)
            assert (got[(maps != 0) | (d2 == INF)] == 1.0).all()
    print("border weights w0 %g sigma %g: worst |got - ref| %.3g (bound %.3g)" % (w0, sigma, worst, 1e-6 * (1 + w0)))


def test_captured_transform_follows_a_changed_input():
    L, lib = _lib()
    shape = (3, 64, 64)
    n, h, w = shape
    first, second = reference(shape)["blobs12"], reference(shape)["corners"]
    t = torch.from_numpy(first[0].copy()).cuda()
    d1, d2 = torch.empty(shape, dtype=torch.int32, device="cuda"), torch.empty(shape, dtype=torch.int32, device="cuda")
    near = torch.empty(shape, dtype=torch.uint8, device="cuda")
    scratch = torch.full((L.edt_scratch_bytes(n, h, w),), 0xAB, dtype=torch.uint8, device="cuda")

    def launch():
        L.check(lib.isa_edt2_u8(L.ptr(t), n, h, w, L.ptr(d1), L.ptr(d2), L.ptr(near), L.ptr(scratch), scratch.numel(),
                                L.stream_ptr()), "isa_edt2_u8")
    launch()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch()
    for maps, want in (second, first):
        t.copy_(torch.from_numpy(maps.copy()))
        g.replay()
        torch.cuda.synchronize()
        same((d1.cpu().numpy(), d2.cpu().numpy(), near.cpu().numpy()), want, "replay")


def test_reseg_methods_give_the_same_answers():
    from isa_amd.reseg import ReSeg
    shape = (3, 64, 64)
    maps, want = reference(shape)["blobs12"]
    m = ReSeg(2, use_instance_seg=False)
    t = torch.from_numpy(maps.copy())
    got = m.distance_transform(t)
    same(tuple(g.cpu().numpy() for g in got), want, "ReSeg.distance_transform")
    # the weight map from a label map and from planes of either form
    ref_w = dn.border_weights(maps, want[0], want[1], 10.0, 5.0)
    ids = np.unique(maps[maps != 0])
    planes = np.stack([(maps == k) for k in ids], axis=-1).astype(np.uint8)            # [B,H,W,K]; label = plane + 1 below
    relabel = np.zeros(256, np.uint8)
    relabel[ids] = np.arange(1, len(ids) + 1)
    w_lab = m.border_weights(torch.from_numpy(relabel[maps])).cpu().numpy()
    w_u8 = m.border_weights(torch.from_numpy(planes)).cpu().numpy()
    w_i64 = m.border_weights(torch.from_numpy(planes).permute(0, 3, 1, 2).contiguous().to(torch.int64)).cpu().numpy()
    assert w_lab.shape == shape and w_lab.dtype == np.float32
    assert np.abs(w_lab - ref_w).max() <= 1e-6 * 11 and np.array_equal(w_lab, w_u8) and np.array_equal(w_lab, w_i64)
    rng = np.random.default_rng(2)
    fg = rng.random(shape) < 0.8
    for max_dist in (None, 3):
        out, filled = m.fill_instances(t, torch.from_numpy(fg), max_dist)
        want_f = dn.fill(maps, fg, want[2], want[0], dn.max_dist_sq(max_dist))
        same((out.cpu().numpy(), filled.cpu().numpy()), want_f, "ReSeg.fill_instances", parts=("out", "filled"))
    with pytest.raises(ValueError):
        m.distance_transform(torch.zeros((1, 8, 10), dtype=torch.uint8))
    with pytest.raises(TypeError):
        m.distance_transform(torch.zeros((1, 8, 12), dtype=torch.int32))
