"""Connected components and instance clean-up on the GPU: isa_cc_label / isa_cc_select, ReSeg.components /
split_components / clean_instances, Model.predict_instances / predict_components, pred_list.py --components.

Everything is an integer and is compared EXACTLY with the restatement tests/components_np.py (which
tests/test_components_ref.py checks against scipy and hand-written answers): comp, n_comp, labels, count, dropped.

Shapes.  The tile of the labelling kernel is 32 rows x 64 columns (ISA_CC_TILE_H x ISA_CC_TILE_W), the shapes the issue
names for that tile: 4 x 4 and 8 x 12 (one partial tile: no merge launch), 72 x 136 (3 x 3 tiles, the last ones partial in
both directions), 64 x 64 with n = 1, 3, 16 (two full tiles above each other, no partial tile), 256 x 256 with n = 2 (16
chunks per image in the selection passes), 512 x 512 with n = 1 in one test only (64 chunks: the cap ISA_ROW_CHUNKS).
Every output sits between sentinel pads that must stay unchanged."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import components_np as cnp     # noqa: E402
import reseg_ref as R           # noqa: E402
from test_gpu_ops import _gpu   # noqa: E402

PAD = 64                        # elements of padding on either side of every output (keeps 16-byte alignment)
CONNS = (4, 8)
SMALL = [(1, 4, 4), (1, 8, 12), (1, 72, 136), (1, 64, 64), (3, 64, 64)]


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


def dev_label(maps, conn):
    """isa_cc_label on a numpy uint8 map [n,h,w] -> (comp, n_comp) as numpy, and the device tensors (map, comp)."""
    L, lib = _lib()
    n, h, w = maps.shape
    t = torch.from_numpy(np.ascontiguousarray(maps)).cuda()
    comp, n_comp = Padded((n, h, w), torch.int32, -77), Padded((n,), torch.int32, -77)
    scratch = torch.full((L.cc_label_scratch_bytes(n, h, w),), 0xAB, dtype=torch.uint8, device="cuda")     # need not be clear
    L.check(lib.isa_cc_label(L.ptr(t), n, h, w, conn, L.ptr(comp.view), L.ptr(n_comp.view), L.ptr(scratch), scratch.numel(),
                             L.stream_ptr()), "isa_cc_label")
    return comp.host(), n_comp.host(), (t, comp.view)


def dev_select(t, comp, mode, min_area=1, max_objects=255):
    L, lib = _lib()
    n, h, w = t.shape
    out = Padded((n, h, w), torch.uint8, 0xEE)
    count, dropped = Padded((n,), torch.int32, -77), Padded((n,), torch.int32, -77)
    scratch = torch.full((L.cc_select_scratch_bytes(n, h, w),), 0xAB, dtype=torch.uint8, device="cuda")    # cleared by the entry
    L.check(lib.isa_cc_select(L.ptr(t), L.ptr(comp), n, h, w, mode, min_area, max_objects, L.ptr(out.view),
                              L.ptr(count.view), L.ptr(dropped.view), L.ptr(scratch), scratch.numel(), L.stream_ptr()),
            "isa_cc_select")
    return out.host(), count.host(), dropped.host()


def same(got, want, what):
    for g, w_, part in zip(got, want, ("labels / comp", "count", "dropped")):
        g, w_ = np.asarray(g), np.asarray(w_)
        assert g.shape == w_.shape and g.dtype == w_.dtype, (what, part, g.shape, w_.shape, g.dtype, w_.dtype)
        bad = np.argwhere(g != w_)
        assert bad.size == 0, "%s: %s differs at %d places, first %s: got %s want %s" % (
            what, part, len(bad), bad[0].tolist(), g[tuple(bad[0])], w_[tuple(bad[0])])


def check(maps, what, conns=CONNS, select=((1, 255),)):
    """Labelling, and both selection modes for every (min_area, max_objects) of `select`, against the restatement."""
    L, _ = _lib()
    maps = np.ascontiguousarray(maps, dtype=np.uint8)
    for conn in conns:
        comp, n_comp, (t, comp_dev) = dev_label(maps, conn)
        want_comp, want_n = cnp.label(maps, conn)
        same((comp, n_comp), (want_comp, want_n), "%s connectivity %d" % (what, conn))
        for min_area, cap in select:
            same(dev_select(t, comp_dev, L.CC_SPLIT, min_area, cap), cnp.split(maps, want_comp, min_area, cap),
                 "%s connectivity %d SPLIT min_area %d cap %d" % (what, conn, min_area, cap))
            same(dev_select(t, comp_dev, L.CC_LARGEST, min_area, cap), cnp.largest(maps, want_comp, min_area, cap),
                 "%s connectivity %d LARGEST min_area %d cap %d" % (what, conn, min_area, cap))


# ---- patterns ---------------------------------------------------------------------------------------------------------
def serpentine(h, w):
    """One-pixel-wide path: the even rows in full, joined alternately at the right and the left end."""
    m = np.zeros((h, w), np.uint8)
    m[::2] = 1
    m[1::4, w - 1] = 1
    m[3::4, 0] = 1
    return m


def spiral(h, w):
    """A one-pixel-wide path that winds inwards: forward while the cell after the next one is free, else turn right."""
    m = np.zeros((h, w), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    free = lambda yy, xx: not (0 <= yy < h and 0 <= xx < w) or m[yy, xx] == 0
    turns = 0
    while turns < 2:
        ny, nx = y + dy, x + dx
        if 0 <= ny < h and 0 <= nx < w and m[ny, nx] == 0 and free(ny + dy, nx + dx):
            y, x, turns = ny, nx, 0
            m[y, x] = 1
        else:
            dy, dx, turns = dx, -dy, turns + 1
    return m


def comb(h, w):
    """Teeth in the even columns that join only in the bottom row."""
    m = np.zeros((h, w), np.uint8)
    m[:, ::2] = 1
    m[h - 1] = 1
    return m


def patterns(h, w):
    yield "serpentine", serpentine(h, w)
    yield "serpentine upside down", serpentine(h, w)[::-1]
    yield "serpentine mirrored", serpentine(h, w)[:, ::-1]
    yield "serpentine in columns", serpentine(w, h).T
    yield "serpentine in columns, mirrored", serpentine(w, h).T[:, ::-1]
    yield "U shapes joined in the last column", comb(w, h).T
    yield "spiral", spiral(h, w)
    yield "comb joined in the bottom row", comb(h, w)
    yield "comb of two values", comb(h, w) * (1 + (np.arange(w) // 2 % 2)).astype(np.uint8)[None]
    yy, xx = np.mgrid[0:h, 0:w]
    yield "checkerboard", ((yy + xx) % 2).astype(np.uint8)
    yield "checkerboard of two values", (((yy + xx) % 2) * (1 + yy % 2)).astype(np.uint8)
    yield "all foreground", np.full((h, w), 7, np.uint8)
    yield "all background", np.zeros((h, w), np.uint8)
    corners = np.zeros((h, w), np.uint8)
    corners[[0, 0, h - 1, h - 1], [0, w - 1, 0, w - 1]] = 255
    yield "corner pixels", corners
    wrap = np.zeros((h, w), np.uint8)
    wrap[:, w - 1] = 1                               # the last column, and the first column of the following rows
    wrap[1:, 0] = 1
    yield "no wrap-around", wrap


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "%dx%dx%d" % s)
def test_patterns(shape):
    n, h, w = shape
    for name, m in patterns(h, w):
        check(np.repeat(np.ascontiguousarray(m)[None], n, 0), "%s %s" % (name, shape))


def test_patterns_across_many_tiles():
    """256 x 256, n = 2: chains through 8 x 4 tiles; image 0 and image 1 hold different patterns."""
    pats = dict(patterns(256, 256))
    for a, b in (("serpentine", "serpentine in columns, mirrored"), ("spiral", "serpentine upside down"),
                 ("comb joined in the bottom row", "U shapes joined in the last column"), ("checkerboard", "all foreground")):
        check(np.stack([pats[a], pats[b]]), "%s | %s" % (a, b))


@pytest.mark.parametrize("seed", (0, 1, 2))
@pytest.mark.parametrize("density", (0.30, 0.41, 0.50, 0.59))
def test_noise(density, seed):
    """Binary noise around the site-percolation thresholds of the two lattices (0.41 and 0.59): huge winding components."""
    rng = np.random.default_rng(1000 * seed + int(100 * density))
    for shape in ((1, 72, 136), (3, 64, 64), (2, 256, 256)):
        check((rng.random(shape) < density).astype(np.uint8), "noise %.2f seed %d %s" % (density, seed, shape))


@pytest.mark.parametrize("shape", [(1, 8, 12), (1, 72, 136), (16, 64, 64), (2, 256, 256)], ids=lambda s: "%dx%dx%d" % s)
def test_multi_valued_maps(shape):
    """Values 0..5 at random: equal-valued regions must not leak into each other; then the same in 4 x 4 blocks."""
    rng = np.random.default_rng(shape[0] + shape[1])
    check(rng.integers(0, 6, shape).astype(np.uint8), "values 0..5 %s" % (shape,))
    n, h, w = shape
    blocks = rng.integers(0, 6, (n, (h + 3) // 4, (w + 3) // 4)).astype(np.uint8)
    check(np.kron(blocks, np.ones((1, 4, 4), np.uint8))[:, :h, :w], "blocks of values 0..5 %s" % (shape,))


def test_largest_image_512():
    rng = np.random.default_rng(5)
    maps = (rng.random((1, 512, 512)) < 0.59).astype(np.uint8)
    check(maps, "noise 0.59 512 x 512")


def test_blobs_that_touch_at_a_corner_of_four_tiles():
    """(31, 63) | (32, 64) and (31, 64) | (32, 63) meet where four tiles meet: one component at 8, two at 4."""
    m = np.zeros((2, 72, 136), np.uint8)
    m[0, 24:32, 56:64] = 1
    m[0, 32:40, 64:72] = 1
    m[1, 24:32, 64:72] = 1
    m[1, 32:40, 56:64] = 1
    check(m, "diagonal blobs")
    assert cnp.label(m, 8)[1].tolist() == [1, 1] and cnp.label(m, 4)[1].tolist() == [2, 2]
    m[:, 31, 63] = m[:, 32, 64] = m[:, 31, 64] = m[:, 32, 63] = 0
    m[0, 31, 63] = m[0, 32, 64] = 2                 # single pixels of another value at the same corner
    m[1, 31, 64] = m[1, 32, 63] = 2
    check(m, "diagonal pixels")


def test_images_do_not_leak():
    rng = np.random.default_rng(11)
    one = (rng.random((64, 64)) < 0.5).astype(np.uint8)
    one[63, :] = 1                                   # the last row of an image and the first row of the next
    one[0, :] = 1
    maps = np.stack([one, one, one])
    comp, n_comp, _ = dev_label(maps, 8)
    assert np.array_equal(comp[0], comp[1]) and np.array_equal(comp[0], comp[2]) and len(set(n_comp.tolist())) == 1
    check(maps, "three equal images")
    maps[1] = 0
    check(maps, "image 1 empty")
    comp, n_comp, _ = dev_label(maps, 4)
    assert not comp[1].any() and n_comp[1] == 0 and np.array_equal(comp[0], comp[2])


# ---- selection --------------------------------------------------------------------------------------------------------
def test_split_cap_and_raster_order():
    """2448 isolated pixels: labels 1..cap in raster order, the rest dropped."""
    L, _ = _lib()
    m = np.zeros((1, 72, 136), np.uint8)
    m[0, ::2, ::2] = 3
    check(m, "isolated pixels", select=((1, 255), (1, 100), (1, 1), (2, 255)))
    comp, n_comp, (t, comp_dev) = dev_label(m, 8)
    out, count, dropped = dev_select(t, comp_dev, L.CC_SPLIT, 1, 255)
    rank = np.arange(36 * 68).reshape(36, 68)
    assert n_comp.tolist() == [2448] and count.tolist() == [255] and dropped.tolist() == [2448 - 255]
    assert np.array_equal(out[0, ::2, ::2], np.where(rank < 255, rank + 1, 0))
    # more than 255 components of several sizes over two images, some of them under min_area
    rng = np.random.default_rng(3)
    noise = (rng.random((2, 256, 256)) < 0.2).astype(np.uint8)
    areas = np.unique(cnp.label(noise, 4)[0], return_counts=True)[1][1:]
    assert (areas >= 3).sum() > 600 and (areas < 3).sum() > 600
    check(noise, "sparse noise", select=((3, 255), (3, 17)))


def fragments(seed, n=3, size=64):
    """A label map as segment() leaves it: blocks of labels 1..6 with speckles of other labels in them."""
    rng = np.random.default_rng(seed)
    m = np.kron(rng.integers(0, 7, (n, size // 8, size // 8)), np.ones((1, 8, 8), np.int64))
    speck = rng.random(m.shape) < 0.08
    m[speck] = rng.integers(0, 7, m.shape)[speck]
    return m.astype(np.uint8)


def test_largest_on_fragments():
    for seed in (0, 1):
        check(fragments(seed), "fragments %d" % seed, select=((1, 255), (6, 255), (1, 3)))
    # ties: value 3 in two 4 x 4 squares (the one that comes first wins), value 9 in pieces of 3 and 5 pixels, value 200
    # alone under every min_area above 2; the survivors are renumbered in value order 3, 9, 200 -> 1, 2, 3
    m = np.zeros((1, 64, 64), np.uint8)
    m[0, 40:44, 8:12] = 3
    m[0, 2:6, 50:54] = 3
    m[0, 60, 0:3] = 9
    m[0, 20, 30:35] = 9
    m[0, 33, 63] = m[0, 34, 63] = 200
    L, _ = _lib()
    comp, _, (t, comp_dev) = dev_label(m, 8)
    out, count, dropped = dev_select(t, comp_dev, L.CC_LARGEST)
    want = np.zeros((64, 64), np.uint8)
    want[2:6, 50:54], want[20, 30:35], want[33:35, 63] = 1, 2, 3
    assert np.array_equal(out[0], want) and count.tolist() == [3] and dropped.tolist() == [2]
    # min_area 0, 1, an exact area (16, 5, 3, 2) and that area plus one
    check(m, "ties", select=[(a, 255) for a in (0, 1, 2, 3, 4, 5, 6, 16, 17)])


# ---- determinism, graphs ------------------------------------------------------------------------------------------------
def test_ten_repeats_are_bit_identical():
    L, _ = _lib()
    rng = np.random.default_rng(8)
    maps = (rng.random((2, 256, 256)) < 0.59).astype(np.uint8) * rng.integers(1, 3, (2, 256, 256)).astype(np.uint8)
    first = None
    for _ in range(10):
        comp, n_comp, (t, comp_dev) = dev_label(maps, 8)
        got = (comp, n_comp) + dev_select(t, comp_dev, L.CC_SPLIT, 2, 255) + dev_select(t, comp_dev, L.CC_LARGEST, 2, 255)
        first = first or got
        assert all(np.array_equal(a, b) for a, b in zip(first, got))


def test_graph_replay_follows_new_contents():
    """One isa_cc_label + isa_cc_select call pair captured in a graph: no host read, a launch count fixed by the shape -
    replayed on new contents of the same buffers it gives the new answer."""
    L, lib = _lib()
    n, h, w = 2, 64, 64
    rng = np.random.default_rng(21)
    t = torch.zeros((n, h, w), dtype=torch.uint8, device="cuda")
    comp = torch.empty((n, h, w), dtype=torch.int32, device="cuda")
    out = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    small = torch.empty((3, n), dtype=torch.int32, device="cuda")
    s1 = torch.empty((L.cc_label_scratch_bytes(n, h, w),), dtype=torch.uint8, device="cuda")
    s2 = torch.empty((L.cc_select_scratch_bytes(n, h, w),), dtype=torch.uint8, device="cuda")

    def call():
        L.check(lib.isa_cc_label(L.ptr(t), n, h, w, 8, L.ptr(comp), L.ptr(small[0]), L.ptr(s1), s1.numel(), L.stream_ptr()),
                "isa_cc_label")
        L.check(lib.isa_cc_select(L.ptr(t), L.ptr(comp), n, h, w, L.CC_LARGEST, 3, 255, L.ptr(out), L.ptr(small[1]),
                                  L.ptr(small[2]), L.ptr(s2), s2.numel(), L.stream_ptr()), "isa_cc_select")

    t.copy_(torch.from_numpy(fragments(30, n, h)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for seed in (31, 32):
        maps = fragments(seed, n, h)
        t.copy_(torch.from_numpy(maps))
        comp.fill_(-5), out.fill_(77), small.fill_(-5)
        g.replay()
        torch.cuda.synchronize()
        want_comp, want_n = cnp.label(maps, 8)
        same((comp.cpu().numpy(), small[0].cpu().numpy()), (want_comp, want_n), "replay %d" % seed)
        same((out.cpu().numpy(), small[1].cpu().numpy(), small[2].cpu().numpy()), cnp.largest(maps, want_comp, 3, 255),
             "replay %d LARGEST" % seed)


# ---- end to end ---------------------------------------------------------------------------------------------------------
def build():
    _gpu()
    from isa_amd.reseg import ReSeg
    m = ReSeg(2, True)
    m.load_state_dict(R.synth_state_dict())
    m.eval()
    m.head.drop_rate = 0.0
    return m


def test_reseg_methods_on_segment_output():
    B, size, cap = 3, 64, 6
    x, sem, ins, n = R.synth_batch(B, size, size, seed=7)
    m = build()
    _, sem_arg, labels, count = m.segment(x, max_objects=cap)
    lab = labels.cpu().numpy()
    assert lab.max() >= 1, "the case must hold predicted instances"
    for conn in CONNS:
        comp, n_comp = m.components(labels, connectivity=conn)
        assert comp.is_cuda and comp.dtype == torch.int32 and n_comp.dtype == torch.int32
        want_comp, want_n = cnp.label(lab, conn)
        same((comp.cpu().numpy(), n_comp.cpu().numpy()), (want_comp, want_n), "components %d" % conn)
        for min_area in (1, 4):
            got = m.clean_instances(labels, connectivity=conn, min_area=min_area)
            same([v.cpu().numpy() for v in got], cnp.largest(lab, want_comp, min_area, 255), "clean largest %d" % conn)
            got_all = m.clean_instances(labels, keep='all', connectivity=conn, min_area=min_area, max_objects=40)
            same([v.cpu().numpy() for v in got_all], cnp.split(lab, want_comp, min_area, 40), "clean all %d" % conn)
            # the outputs go straight into score_instances
            scores = m.score_instances(got[0], got[1], ins, n, sem_arg, sem)
            assert tuple(scores.shape) == (B, 8) and scores.dtype == torch.float64
            assert np.array_equal(scores[:, 4].cpu().numpy(), got[1].cpu().numpy().astype(np.float64))
            m.score_instances(got_all[0], got_all[1], ins, n, sem_arg, sem, max_objects=40)
    # the blob-counting baseline: components of the foreground map
    fg = (sem_arg[:, 0] > 0.5).to(torch.uint8)
    got = m.split_components(fg, min_area=2)
    fg_np = fg.cpu().numpy()
    same([v.cpu().numpy() for v in got], cnp.split(fg_np, cnp.label(fg_np, 8)[0], 2, 255), "split_components")
    with pytest.raises(ValueError):
        m.clean_instances(labels, keep='some')
    with pytest.raises(ValueError):
        m.components(labels, connectivity=6)
    with pytest.raises(TypeError):
        m.components(labels.int())


def test_model_defaults_are_untouched_and_the_keywords_clean():
    """Model.predict_instances / evaluate with the default keywords never reach the new code (every new method is replaced
    by one that raises) and hand back exactly what segment() produced in that call; with the keywords they return the
    restatement's clean-up of what segment() produced in that call.
    The comparison is made inside ONE call (segment is wrapped to keep what it returned) and not between two calls: the
    eval-mode semantic logits of this model differ in the last bit from run to run (measured on MI355X before this test
    was written: 3 of 6 identical segment() calls gave logits 1 ulp away from the first), so two calls are not bit-identical
    with or without the new keywords."""
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
        raise AssertionError("the default arguments reached the component code")

    net.segment = segment
    new_code = [(net, "clean_instances"), (net, "split_components"), (net, "components"), (net, "cc_label"),
                (net, "cc_select")]
    for obj, name in new_code:
        setattr(obj, name, trap)
    prob, labels, count = model.predict_instances(x)
    assert len(seen) == 1
    want_prob = net.net.softmax_nchw(net._last_sem)[:, 1]                      # the logits of that call, still in its arena
    assert torch.equal(prob, want_prob.cpu()) and torch.equal(labels, seen[0][2].cpu()) and torch.equal(count, seen[0][3].cpu())
    batch = [(x, sem, ins, n)]
    for kwargs in ({}, dict(min_area=0, keep=None, connectivity=8), dict(min_area=1)):
        res = model.evaluate(batch, **kwargs)
        _, sem_arg, lab, cnt = seen[-1]
        want_rows = net.score_instances(lab, cnt, ins, n, sem_arg, sem, max_objects=5).cpu().numpy()
        assert np.array_equal(res["per_image"], want_rows, equal_nan=True)
    for obj, name in new_code:
        delattr(obj, name)                                                     # the class's methods again
    for keep, fn in (('largest', cnp.largest), ('all', cnp.split)):
        _, cl, cc = model.predict_instances(x, keep=keep, min_area=3, connectivity=4)
        lab = seen[-1][2].cpu().numpy()
        same((cl.numpy(), cc.numpy()), fn(lab, cnp.label(lab, 4)[0], 3, 5)[:2], "predict_instances keep=%s" % keep)
    _, cl, cc = model.predict_instances(x, min_area=3)                          # min_area alone: every piece of 3 pixels
    lab = seen[-1][2].cpu().numpy()
    same((cl.numpy(), cc.numpy()), cnp.split(lab, cnp.label(lab, 8)[0], 3, 5)[:2], "predict_instances min_area alone")
    cleaned = model.evaluate(batch, keep='largest', min_area=3)
    _, sem_arg, lab, cnt = seen[-1]
    cl, cc, _ = net.clean_instances(lab, min_area=3, max_objects=5)
    want_rows = net.score_instances(cl, cc, ins, n, sem_arg, sem, max_objects=5).cpu().numpy()
    assert np.array_equal(cleaned["per_image"], want_rows, equal_nan=True)
    with pytest.raises(ValueError):
        model.predict_instances(x, keep='some')
    # the blob-counting baseline needs no instance head
    calls = len(seen)
    p2, l2, c2 = model.predict_components(x, min_area=2)
    assert len(seen) == calls, "predict_components runs no instance inference"
    fg = (net.class_map().cpu().numpy() != 0).astype(np.uint8)
    same((l2.numpy(), c2.numpy()), cnp.split(fg, cnp.label(fg, 8)[0], 2, 5)[:2], "predict_components")
    assert torch.equal(p2, net.net.softmax_nchw(net._last_sem)[:, 1].cpu())
    sem_only = Model("CVPPP", "ReSeg", 2, 5, use_instance_segmentation=False)
    p3, l3, c3 = sem_only.predict_components(x)
    assert tuple(l3.shape) == (2, 64, 64) and l3.dtype == torch.uint8 and c3.dtype == torch.int32
    assert all(int(l3[b].max()) == int(c3[b]) for b in range(2))


def test_pred_list_components_and_evaluate(tmp_path):
    """pred_list.py --components needs no instance head and writes the files evaluate.py reads: a data root whose label
    images are copies of the predictions scores SBD = 1 and |DiC| = 0 on every image (the file contract of
    tests/test_pred_list.py and tests/test_gpu_segment.py)."""
    from PIL import Image
    _gpu()
    out = str(tmp_path / "comp")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "pred_list.py"), "--synthetic", "4", "--batch", "4", "--components",
                        "--min-area", "2", "--max-objects", "20", "--output", out], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = sorted(os.listdir(out))
    assert names == ["synthetic_%04d" % i for i in range(4)]
    root = tmp_path / "data"
    img_dir = root / "raw/CVPPP/CVPPP2017_LSC_training/training/A1"
    os.makedirs(img_dir)
    os.makedirs(root / "metadata/CVPPP")
    rows = []
    for i, name in enumerate(names):
        d = os.path.join(out, name)
        assert sorted(os.listdir(d)) == sorted(name + s for s in ("-fg_mask.png", "-ins_mask.png", "-ins_mask_color.png",
                                                                  "-n_objects.npy", ".png"))
        ins = np.array(Image.open(os.path.join(d, name + "-ins_mask.png")))
        fgm = np.array(Image.open(os.path.join(d, name + "-fg_mask.png")))
        k = int(np.load(os.path.join(d, name + "-n_objects.npy")))
        assert ins.shape == (300 + 7 * (i % 5), 330) and ins.dtype == np.uint8
        assert k == int(ins.max()) and 1 <= k <= 20, (name, k, int(ins.max()), int((fgm == 255).sum()))
        assert not ins[fgm == 0].any()
        Image.fromarray(ins).save(img_dir / (name + "_label.png"))
        Image.fromarray((fgm == 255).astype(np.uint8)).save(img_dir / (name + "_fg.png"))
        rows.append("%s,%d" % (name, k))
    (root / "metadata/CVPPP/validation_image_paths.txt").write_text("".join("x/%s.png\n" % nm for nm in names))
    (root / "metadata/CVPPP/number_of_instances.txt").write_text("\n".join(rows) + "\n")
    from evaluate import evaluate_cvppp
    sbds, dics, fg_dices, scored = evaluate_cvppp(out, str(root))
    assert scored == names
    assert sbds == [1.0] * 4 and [int(v) for v in dics] == [0] * 4 and fg_dices == [1.0] * 4
