"""Measuring instances on the GPU: isa_label_props / isa_instance_props / isa_props_select / isa_relabel_u8,
ReSeg.instance_properties / select_instances, Model.predict_instances / measure_instances, pred_list.py --properties.

acc, oob, table, count, dropped and the relabelled maps are integers and are compared EXACTLY with the restatement
tests/props_np.py (which tests/test_props_ref.py checks against scipy and hand-written answers).  Of the derived columns
the integer ones are exact, the single divisions of exact integers are held to 1e-12 relative (the bound of
tests/test_gpu_score.py for such divisions) and the columns behind a square root or an arc tangent to 1e-9 on a set of
shapes whose eigenvalues are separated (see test_axes_on_ellipses_and_rectangles).

Shapes.  A workgroup walks a chunk of at least 4096 pixels, at most ISA_ROW_CHUNKS = 64 chunks an image, a lane 4 or 16
pixels a trip: 4 x 4 (one lane holds the image), 8 x 12 and 72 x 136 (w % 16 != 0: a lane's pixels straddle rows, runs are
cut at row ends), 64 x 64 with n = 1, 3, 16, 256 x 256 with n = 2 (16 chunks), 512 x 512 with n = 1 in one test only (the
64-chunk cap; a full-image label pushes the second-order sums past 2^32).  Every map is measured through both load paths:
a pointer 4 bytes off a 16-byte boundary takes the 4-pixel one.  Every output sits between sentinel pads."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import props_np as P            # noqa: E402
import reseg_ref as R           # noqa: E402
from test_gpu_ops import _gpu   # noqa: E402

PAD = 64                        # elements of padding on either side of every output
ORDERS = (P.ORDER_LABEL, P.ORDER_AREA, P.ORDER_RASTER)


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


def dev_map(maps, offset):
    """The uint8 array on the device, `offset` bytes past a 16-byte boundary."""
    flat = torch.zeros((maps.size + 16,), dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 16 == 0
    t = flat[offset:offset + maps.size].view(maps.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(maps)))
    return t


def dev_props(maps, image=None, nl=256, offset=0):
    """isa_label_props -> (acc, oob) as numpy and the device acc."""
    L, lib = _lib()
    n, h, w = maps.shape
    t = dev_map(maps, offset)
    img = None if image is None else torch.from_numpy(np.ascontiguousarray(image)).cuda()
    acc, oob = Padded((n, nl, P.ACC), torch.int64, -77), Padded((n,), torch.int32, -77)
    L.check(lib.isa_label_props(t, img, n, h, w, 0 if image is None else image.shape[3], nl, acc.view, oob.view,
                                L.stream_ptr()), "isa_label_props")
    return acc.host(), oob.host(), acc.view, t


def dev_derive(acc, h, w, c):
    L, lib = _lib()
    n, nl = acc.shape[:2]
    out = Padded((n, nl, P.OUT), torch.float64, -77.0)
    L.check(lib.isa_instance_props(acc, n, nl, h, w, c, out.view, L.stream_ptr()), "isa_instance_props")
    return out.host()


def dev_select(acc, h, w, t, **kw):
    """isa_props_select + isa_relabel_u8 -> (table, count, dropped, relabelled map)."""
    L, lib = _lib()
    n, nl = acc.shape[:2]
    table = Padded((n, 256), torch.uint8, 0xEE)
    count, dropped = Padded((n,), torch.int32, -77), Padded((n,), torch.int32, -77)
    L.check(lib.isa_props_select(acc, n, nl, h, w, kw.get("min_area", 1), kw.get("max_area", 0),
                                 int(kw.get("clear_border", False)), kw.get("order", P.ORDER_LABEL), kw.get("max_objects", 255),
                                 table.view, count.view, dropped.view, L.stream_ptr()), "isa_props_select")
    out = Padded(tuple(t.shape), torch.uint8, 0xEE)
    L.check(lib.isa_relabel_u8(t, table.view, n, t.numel() // n, out.view, L.stream_ptr()), "isa_relabel_u8")
    return table.host(), count.host(), dropped.host(), out.host()


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s differs at %d places, first %s: got %s want %s" % (
        what, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def check_derived(out, rows, what):
    """Columns 0-4, 14, 15, 19 exactly; 5-9, 16, 20-23 within 1e-12 relative of the exact rational; NaN where stated."""
    want = P.as_float(rows)
    assert out.shape == want.shape, what
    for k in P.EXACT_COLS:
        assert np.array_equal(out[..., k], want[..., k], equal_nan=True), (what, "column", k)
    for k in P.RATIONAL_COLS:
        g, w_ = out[..., k], want[..., k]
        assert np.array_equal(np.isnan(g), np.isnan(w_)), (what, "NaN pattern of column", k)
        ok = ~np.isnan(w_)
        err = np.abs(g[ok] - w_[ok])
        assert (err <= 1e-12 * np.abs(w_[ok])).all(), (what, "column", k, float(err.max()) if err.size else 0.0)
    for k in P.FLOAT_COLS:
        assert np.array_equal(np.isnan(out[..., k]), np.isnan(want[..., k])), (what, "NaN pattern of column", k)


def check(maps, what, image=None, nl=256, selects=None, offsets=(0, 4)):
    """Every output of the four entries against the restatement, through both load paths."""
    maps = np.ascontiguousarray(maps, dtype=np.uint8)
    n, h, w = maps.shape
    c = 0 if image is None else image.shape[3]
    want_acc, want_oob = P.label_props(maps, image, nl)
    rows = P.derive(want_acc, h, w, c)
    if selects is None:
        selects = [dict(order=o) for o in ORDERS] + [dict(order=P.ORDER_AREA, min_area=3, max_area=max(3, h * w // 8),
                                                          clear_border=True, max_objects=3)]
    for off in offsets:
        tag = "%s (pointer offset %d)" % (what, off)
        acc, oob, acc_dev, t = dev_props(maps, image, nl, off)
        same(acc, want_acc, tag + ": acc")
        same(oob, want_oob, tag + ": oob")
        check_derived(dev_derive(acc_dev, h, w, c), rows, tag)
        for kw in selects:
            got = dev_select(acc_dev, h, w, t, **kw)
            table, count, dropped = P.select(want_acc, h, w, **kw)
            for g, w_, part in zip(got, (table, count, dropped, P.relabel(np.minimum(maps, 255), table)),
                                   ("table", "count", "dropped", "relabelled map")):
                same(g, w_, "%s %s: %s" % (tag, kw, part))
    return want_acc


# ---- contents -----------------------------------------------------------------------------------------------------------
def blobs(h, w, seed, k=6, noise=0.05):
    """k discs of random centre and radius over sparse noise of other labels."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    lab = np.zeros((h, w), dtype=np.uint8)
    speck = rng.random((h, w)) < noise
    lab[speck] = rng.integers(k + 1, k + 9, int(speck.sum()))
    for v in range(1, k + 1):
        cy, cx, r = rng.integers(0, h), rng.integers(0, w), rng.integers(1, max(2, min(h, w) // 3))
        lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = v
    return lab


def edge_blobs(h, w):
    """One blob on each of the four edges and one that touches none (as far as the size allows)."""
    lab = np.zeros((h, w), dtype=np.uint8)
    a, b = max(1, h // 4), max(1, w // 4)
    lab[0:a, w // 2:w // 2 + b] = 1
    lab[h - a:h, 1:1 + b] = 2
    lab[h // 2:h // 2 + a, 0:b] = 3
    lab[1:1 + a, w - b:w] = 4
    lab[h // 2, w // 2] = 5
    return lab


def patterns(h, w):
    yy, xx = np.mgrid[:h, :w]
    every = ((yy * w + xx) % 255 + 1).astype(np.uint8)            # labels 1..255 all present when h * w >= 255
    return {
        "one label everywhere": np.full((h, w), 7, dtype=np.uint8),
        "all background": np.zeros((h, w), dtype=np.uint8),
        "checkerboard": ((yy + xx) % 2 + 1).astype(np.uint8),
        "checkerboard with background": ((yy + xx) % 2 * 9).astype(np.uint8),
        "vertical stripes": (xx % 2 * 3 + 1).astype(np.uint8),
        "horizontal stripes": (yy % 3).astype(np.uint8),
        "labels 1..255": every,
        "edge blobs": edge_blobs(h, w),
        "blobs over noise": blobs(h, w, h * 1000 + w),
    }


SMALL = [(4, 4), (8, 12), (72, 136), (64, 64)]


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "%dx%d" % s)
def test_patterns(shape):
    h, w = shape
    for name, lab in patterns(h, w).items():
        check(lab[None], "%s %dx%d" % (name, h, w))


@pytest.mark.parametrize("n", (3, 16))
def test_batches_of_64x64(n):
    maps = np.stack([blobs(64, 64, 50 + i, k=4 + i % 5) for i in range(n)])
    maps[n - 1] = 0                                               # an image without instances among the others
    check(maps, "blobs n=%d" % n)


def test_several_chunks_256():
    maps = np.stack([blobs(256, 256, 5, k=12, noise=0.01), ((np.mgrid[:256, :256].sum(0)) % 2 + 1).astype(np.uint8)])
    check(maps, "256x256", selects=[dict(order=P.ORDER_AREA), dict(order=P.ORDER_RASTER, clear_border=True)])


def test_largest_image_512():
    """64 chunks; the full-image label carries sums of squares and products past 2^32."""
    full = np.full((1, 512, 512), 3, dtype=np.uint8)
    acc = check(full, "512x512 one label", selects=[dict(order=P.ORDER_AREA)])
    assert min(int(acc[0, 3, k]) for k in (7, 8, 9)) > 1 << 32
    check(blobs(512, 512, 9, k=20, noise=0.002)[None], "512x512 blobs", selects=[dict(order=P.ORDER_AREA)], offsets=(0,))


def test_labels_outside_nl_are_counted():
    lab = blobs(64, 64, 3, k=6)                                   # labels up to 14
    for nl in (1, 2, 7, 15):
        acc = check(lab[None], "nl=%d" % nl, nl=nl, selects=[dict(order=P.ORDER_AREA)])
        assert acc.shape == (1, nl, 16)
    _, oob, _, _ = dev_props(lab[None], None, 7)
    assert int(oob[0]) == int((lab >= 7).sum()) > 0


@pytest.mark.parametrize("c", (0, 1, 3, 4))
def test_image_channels(c):
    rng = np.random.default_rng(c)
    maps = np.stack([blobs(72, 136, 11), blobs(72, 136, 12)])
    image = None if c == 0 else rng.integers(0, 256, (2, 72, 136, c)).astype(np.uint8)
    acc = check(maps, "c=%d" % c, image=image, selects=[])
    if c:
        assert (acc[:, 1:, 12:12 + c].sum(axis=(0, 1)) > 0).all() and not acc[:, :, 12 + c:].any()
    full = np.full((1, 64, 64), 1, dtype=np.uint8)                # every pixel reads its channels
    check(full, "c=%d, one label" % c, image=None if c == 0 else rng.integers(0, 256, (1, 64, 64, c)).astype(np.uint8),
          selects=[])


# ---- derived columns behind a root or an arc tangent --------------------------------------------------------------------
def ellipses_and_rectangles():
    """uint8 [2,128,128]: rotated ellipses and axis-parallel and rotated rectangles, every one elongated (axis ratio
    between 1.3 and 4) and at least 5 pixels thick, so that the eigenvalues are well apart and neither is small."""
    yy, xx = np.mgrid[:128, :128].astype(np.float64)
    maps = np.zeros((2, 128, 128), dtype=np.uint8)
    v = 0
    for i in range(2):
        for j, (cy, cx) in enumerate([(22, 22), (22, 64), (22, 106), (64, 22), (64, 64), (64, 106), (106, 22), (106, 64),
                                      (106, 106)]):
            v += 1
            a, ratio, th = 10 + (j + i) % 8, (1.3, 1.7, 2.0, 2.6, 3.1, 4.0)[(j + 2 * i) % 6], (0.37 * v + 0.1) % np.pi
            b = max(a / ratio, 2.5)
            u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
            t = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
            if j % 3 == 0:
                m = (np.abs(xx - cx) <= a) & (np.abs(yy - cy) <= b) if i == 0 else (np.abs(xx - cx) <= b) & (np.abs(yy - cy) <= a)
            elif j % 3 == 1:
                m = (np.abs(u) <= a) & (np.abs(t) <= b)
            else:
                m = (u / a) ** 2 + (t / b) ** 2 <= 1.0
            maps[i][m & (maps[i] == 0)] = v
    return maps


def test_axes_on_ellipses_and_rectangles():
    """Columns 10-13, 17, 18 within 1e-9 relative (the orientation: absolute).  With l2 >= 1e-3 l1 and l1 - l2 >= 1e-3 l1
    the subtraction half - rad and the quotient l2 / l1 amplify the few ulp of their inputs by at most 1e3: 1e-13, three
    orders inside the bound.  The condition is asserted for EVERY label on the restatement's values before the GPU runs."""
    maps = ellipses_and_rectangles()
    n, h, w = maps.shape
    want_acc, _ = P.label_props(maps, None, 32)
    labels = [(i, v) for i in range(n) for v in range(1, 32) if want_acc[i, v, 0]]
    assert len(labels) == 18
    for i, v in labels:
        l1, l2 = P.eigenvalues(want_acc[i, v])
        assert l2 >= 1e-3 * l1 and l1 - l2 >= 1e-3 * l1, (i, v, l1, l2)
    rows = P.derive(want_acc, h, w, 0)
    for off in (0, 4):
        acc, _, acc_dev, _ = dev_props(maps, None, 32, off)
        same(acc, want_acc, "acc")
        out = dev_derive(acc_dev, h, w, 0)
        check_derived(out, rows, "ellipses")
        seen = set()
        for i, v in labels:
            for k in P.FLOAT_COLS:
                got, want = float(out[i, v, k]), float(rows[i][v][k])
                bound = 1e-9 if k == 13 else 1e-9 * abs(want)
                assert abs(got - want) <= bound, (i, v, P.COLUMNS[k], got, want)
            assert -np.pi / 2 < out[i, v, 13] <= np.pi / 2
            seen.add(round(float(out[i, v, 13]), 2))
        assert len(seen) >= 8, "the set must hold many orientations"


def test_degenerate_shapes_give_the_stated_special_values():
    lab = np.zeros((32, 32), dtype=np.uint8)
    lab[3, 4] = 1                      # a single pixel
    lab[8, 2:20] = 2                   # a horizontal line
    lab[10:30, 25] = 3                 # a vertical line
    lab[12:18, 4:10] = 4               # a square
    acc, _, acc_dev, _ = dev_props(lab[None])
    out = dev_derive(acc_dev, 32, 32, 0)[0]
    assert out[1, 10] == 0 and out[1, 11] == 0 and out[1, 12] == 0 and out[1, 13] == 0
    assert out[2, 11] == 0 and out[2, 12] == 1 and out[2, 13] == 0 and out[2, 10] > 0
    assert out[3, 11] == 0 and out[3, 12] == 1 and out[3, 13] == np.pi / 2
    assert out[4, 12] == 0 and out[4, 13] == 0 and out[4, 10] == out[4, 11] > 0
    assert out[0, 0] == 0 and np.isnan(out[0, 1:]).all() and out[5, 0] == 0 and np.isnan(out[5, 1:]).all()


# ---- determinism, graphs, in place ----------------------------------------------------------------------------------------
def test_ten_repeats_are_bit_identical():
    maps = np.stack([blobs(256, 256, 70, k=30, noise=0.2), blobs(256, 256, 71, k=30, noise=0.2)])
    image = np.random.default_rng(1).integers(0, 256, (2, 256, 256, 3)).astype(np.uint8)
    first = None
    for _ in range(10):
        acc, oob, acc_dev, t = dev_props(maps, image)
        got = (acc, oob, dev_derive(acc_dev, 256, 256, 3)) + dev_select(acc_dev, 256, 256, t, order=P.ORDER_AREA, min_area=2)
        first = first or got
        assert all(np.array_equal(a, b, equal_nan=a.dtype == np.float64) for a, b in zip(first, got))


def test_graph_replay_follows_new_contents():
    """isa_label_props + isa_instance_props + isa_props_select + isa_relabel_u8 captured in one graph: no host read, a
    fixed launch count, every buffer cleared by a kernel - replayed twice on new contents it gives the new answers."""
    L, lib = _lib()
    n, h, w = 2, 64, 64
    t = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    acc = torch.empty((n, 256, P.ACC), dtype=torch.int64, device="cuda")
    out = torch.empty((n, 256, P.OUT), dtype=torch.float64, device="cuda")
    table = torch.empty((n, 256), dtype=torch.uint8, device="cuda")
    new = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    small = torch.empty((3, n), dtype=torch.int32, device="cuda")

    def call():
        st = L.stream_ptr()
        L.check(lib.isa_label_props(t, None, n, h, w, 0, 256, acc, small[0], st), "isa_label_props")
        L.check(lib.isa_instance_props(acc, n, 256, h, w, 0, out, st), "isa_instance_props")
        L.check(lib.isa_props_select(acc, n, 256, h, w, 2, 0, 0, P.ORDER_AREA, 255, table, small[1], small[2], st),
                "isa_props_select")
        L.check(lib.isa_relabel_u8(t, table, n, h * w, new, st), "isa_relabel_u8")

    first = np.stack([blobs(h, w, 30 + i) for i in range(n)])
    t.copy_(torch.from_numpy(first))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for seed in (41, 43):
        maps = np.stack([blobs(h, w, seed + i, k=3 + seed % 5) for i in range(n)])
        t.copy_(torch.from_numpy(maps))
        acc.fill_(-5), out.fill_(-5.0), table.fill_(77), new.fill_(77), small.fill_(-5)
        g.replay()
        torch.cuda.synchronize()
        want_acc, want_oob = P.label_props(maps, None, 256)
        same(acc.cpu().numpy(), want_acc, "replay %d: acc" % seed)
        same(small[0].cpu().numpy(), want_oob, "replay %d: oob" % seed)
        check_derived(out.cpu().numpy(), P.derive(want_acc, h, w, 0), "replay %d" % seed)
        wt, wc, wd = P.select(want_acc, h, w, min_area=2, order=P.ORDER_AREA)
        for got, want, part in ((table, wt, "table"), (small[1], wc, "count"), (small[2], wd, "dropped"),
                                (new, P.relabel(maps, wt), "relabelled map")):
            same(got.cpu().numpy(), want, "replay %d: %s" % (seed, part))


@pytest.mark.parametrize("offset", (0, 4))
def test_relabel_in_place(offset):
    L, lib = _lib()
    maps = np.stack([blobs(72, 136, 90), blobs(72, 136, 91)])
    rng = np.random.default_rng(2)
    table = np.stack([rng.permutation(256), rng.permutation(256)]).astype(np.uint8)
    t = dev_map(maps, offset)
    L.check(lib.isa_relabel_u8(t, torch.from_numpy(table).cuda(), 2, 72 * 136, t, L.stream_ptr()), "isa_relabel_u8")
    same(t.cpu().numpy(), P.relabel(maps, table), "in place")


# ---- end to end ---------------------------------------------------------------------------------------------------------
def build():
    _gpu()
    from isa_amd.reseg import ReSeg
    m = ReSeg(2, True)
    m.load_state_dict(R.synth_state_dict())
    m.eval()
    m.head.drop_rate = 0.0
    return m


def test_reseg_methods_and_scoring():
    """instance_properties and select_instances on device tensors; select_instances(order='area') goes into
    score_instances unchanged."""
    from isa_amd import reseg
    B, size = 3, 64
    x, sem, ins, n = R.synth_batch(B, size, size, seed=7)
    m = build()
    lab = np.stack([blobs(size, size, 20 + i, k=5) for i in range(B)])
    labels = torch.from_numpy(lab).cuda()
    rgb = np.random.default_rng(4).integers(0, 256, (B, size, size, 3)).astype(np.uint8)
    want_acc, _ = P.label_props(lab, rgb, 256)
    props = m.instance_properties(labels, torch.from_numpy(rgb))
    assert props.is_cuda and props.dtype == torch.float64 and tuple(props.shape) == (B, 256, 24) == (B, 256, len(reseg.PROPS_COLUMNS))
    check_derived(props.cpu().numpy(), P.derive(want_acc, size, size, 3), "instance_properties")
    assert not int(m.last_props_oob.sum())
    with pytest.raises(ValueError):
        m.instance_properties(labels, n_labels=4)
    small = m.instance_properties(labels, n_labels=4, check=False)
    assert tuple(small.shape) == (B, 4, 24)
    same(m.last_props_oob.cpu().numpy(), (lab >= 4).sum(axis=(1, 2)).astype(np.int32), "last_props_oob")
    for kw, ref in ((dict(order='area'), dict(order=P.ORDER_AREA)),
                    (dict(order='raster', min_area=3, max_area=400, clear_border=True, max_objects=4),
                     dict(order=P.ORDER_RASTER, min_area=3, max_area=400, clear_border=True, max_objects=4)),
                    (dict(), dict())):
        got = m.select_instances(labels, **kw)
        table, count, dropped = P.select(want_acc, size, size, **ref)
        for g, w_, part in zip(got, (P.relabel(lab, table), count, dropped), ("labels", "n_objects", "dropped")):
            assert g.is_cuda
            same(g.cpu().numpy(), w_, "select_instances %s: %s" % (kw, part))
    by_area = m.select_instances(labels, order='area')
    scores = m.score_instances(by_area[0], by_area[1], ins, n)
    assert tuple(scores.shape) == (B, 8) and scores.dtype == torch.float64
    assert np.array_equal(scores[:, 4].cpu().numpy(), by_area[1].cpu().numpy().astype(np.float64))
    areas = m.instance_properties(by_area[0])[:, 1:, 0].cpu().numpy()
    assert (np.diff(areas, axis=1) <= 0).all(), "largest first"
    with pytest.raises(ValueError):
        m.select_instances(labels, order='size')
    with pytest.raises(TypeError):
        m.instance_properties(labels.int())


def test_model_defaults_run_nothing_new_and_the_keywords_select():
    """Model.predict_instances / evaluate with the default keywords never reach the new code (every new method is replaced
    by one that raises); with the keywords they return the restatement's selection of what segment() produced in that
    call, and measure_instances describes exactly the labels it returns."""
    _gpu()
    from isa_amd.model import Model
    x, sem, ins, n = R.synth_batch(2, 64, 64, seed=2)
    model = Model("CVPPP", "ReSeg", 2, 5, use_instance_segmentation=True)
    net = model.model
    seen, real_segment = [], net.segment

    def segment(*a, **k):
        seen.append(real_segment(*a, **k))
        return seen[-1]

    def trap(*a, **k):
        raise AssertionError("the default arguments reached the measuring code")

    net.segment = segment
    new_code = [(net, "instance_properties"), (net, "select_instances"), (net, "label_props"),
                (net, "instance_props"), (net, "props_select"), (net, "relabel")]
    for obj, name in new_code:
        setattr(obj, name, trap)
    prob, labels, count = model.predict_instances(x)
    assert len(seen) == 1 and torch.equal(labels, seen[0][2].cpu()) and torch.equal(count, seen[0][3].cpu())
    batch = [(x, sem, ins, n)]
    for kwargs in ({}, dict(order=None, clear_border=False, max_area=None)):
        res = model.evaluate(batch, **kwargs)
        _, sem_arg, lab, cnt = seen[-1]
        want_rows = net.score_instances(lab, cnt, ins, n, sem_arg, sem, max_objects=5).cpu().numpy()
        assert np.array_equal(res["per_image"], want_rows, equal_nan=True)
    for obj, name in new_code:
        delattr(obj, name)                                                     # the class's methods again
    for kw, ref in ((dict(order='area'), dict(order=P.ORDER_AREA)),
                    (dict(clear_border=True, max_area=2000), dict(clear_border=True, max_area=2000))):
        _, sl, sc = model.predict_instances(x, **kw)
        lab = seen[-1][2].cpu().numpy()
        acc, _ = P.label_props(lab, None, 256)
        table, cnt, _ = P.select(acc, 64, 64, max_objects=5, **ref)
        same(sl.numpy(), P.relabel(lab, table), "predict_instances %s: labels" % kw)
        same(sc.numpy(), cnt, "predict_instances %s: n_objects" % kw)
    res = model.evaluate(batch, order='area')
    _, sem_arg, lab, cnt = seen[-1]
    sl, sc, _ = net.select_instances(lab, order='area', max_objects=5)
    want_rows = net.score_instances(sl, sc, ins, n, sem_arg, sem, max_objects=5).cpu().numpy()
    assert np.array_equal(res["per_image"], want_rows, equal_nan=True)
    prob, labels, count, rows = model.measure_instances(x, order='area')
    lab = labels.numpy()
    assert len(rows) == 2
    for b in range(2):
        k = int(count[b])
        assert rows[b].shape == (k, 24) and rows[b].dtype == np.float64
        assert rows[b][:, 0].tolist() == np.bincount(lab[b].reshape(-1), minlength=k + 1)[1:k + 1].tolist()
        assert (np.diff(rows[b][:, 0]) <= 0).all()
    with pytest.raises(ValueError):
        model.predict_instances(x, order='size')


def test_pred_list_properties_csv(tmp_path):
    """pred_list.py --instances --properties --order area writes <name>-instances.csv: PROPS_COLUMNS and the two sizes; the
    areas equal the pixel counts of the written model-resolution labels and do not increase."""
    from PIL import Image
    _gpu()
    from isa_amd.reseg import PROPS_COLUMNS
    out = str(tmp_path / "props")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "pred_list.py"), "--synthetic", "2", "--instances", "--properties",
                        "--order", "area", "--output", out], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = sorted(os.listdir(out))
    assert names == ["synthetic_%04d" % i for i in range(2)]
    for i, name in enumerate(names):
        d = os.path.join(out, name)
        assert {name + "-instances.csv", name + "-ins_mask_model.png", name + "-ins_mask.png"} <= set(os.listdir(d))
        lines = open(os.path.join(d, name + "-instances.csv")).read().splitlines()
        assert lines[0].split(",") == list(PROPS_COLUMNS) + ["model_w", "model_h", "orig_w", "orig_h"]
        table = np.array([[float(t) for t in ln.split(",")] for ln in lines[1:]], dtype=np.float64).reshape(-1, 28)
        model_lab = np.array(Image.open(os.path.join(d, name + "-ins_mask_model.png")))
        k = int(np.load(os.path.join(d, name + "-n_objects.npy")))
        assert model_lab.shape == (256, 256) and model_lab.dtype == np.uint8 and table.shape[0] == k == int(model_lab.max())
        assert table[:, 0].tolist() == np.bincount(model_lab.reshape(-1), minlength=k + 1)[1:k + 1].tolist()
        assert (np.diff(table[:, 0]) <= 0).all()
        assert (table[:, 24:] == [256, 256, 330, 300 + 7 * (i % 5)]).all()
        assert not np.isnan(table[:, 20:23]).any() and np.isnan(table[:, 23]).all()      # RGB means, no fourth channel
