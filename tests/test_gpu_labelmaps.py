"""The label-map operators on a bare isa_amd.labelmaps.LabelOps handle - no model is built in this module.

Every family once, on maps uint8 [2,8,12] (one blob on the border, one ring around a hole, one label in two pieces, one
pair of pixels that meet at a corner), against the numpy restatements the per-family tests use (components_np, distance_np,
contours_np, score_np, props_np) and with their comparisons: integers exactly, scores within test_gpu_score's 1e-12,
measurements by test_gpu_props' check_derived.  Then the two hooks: a handle whose alloc hands out 0xFF-filled memory (NaN
in every float type, -1 in every integer) and records what it hands out must give the same bytes as the default handle,
and every tensor that comes back must be one it handed out - the training step's arena-bound handle relies on that alone.
Last, evaluate.py's device path against score_instances, bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import components_np as cnp       # noqa: E402
import contours_np as C           # noqa: E402
import distance_np as dn          # noqa: E402
import props_np as P              # noqa: E402
import score_np as S              # noqa: E402
from test_gpu_ops import _gpu     # noqa: E402
from test_gpu_props import check_derived                          # noqa: E402
from test_gpu_score import close as close_scores, host_scores     # noqa: E402

MAPS = np.array([
    [[1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0],        # label 1: a blob in the corner and a smaller piece at the right edge
     [1, 1, 1, 0, 0, 2, 2, 2, 2, 2, 0, 0],        # label 2: a ring around a 2 x 3 hole
     [0, 0, 0, 0, 0, 2, 0, 0, 0, 2, 0, 0],
     [0, 0, 0, 0, 0, 2, 0, 0, 0, 2, 0, 0],
     [0, 3, 3, 0, 0, 2, 2, 2, 2, 2, 0, 0],        # label 3: inside the image
     [0, 3, 3, 0, 0, 0, 0, 0, 0, 0, 0, 1],
     [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1],
     [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]],
    [[0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
     [0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0],
     [0, 1, 1, 1, 0, 4, 0, 0, 0, 0, 0, 0],        # label 4: two pixels that touch at a corner (one piece only under 8)
     [0, 0, 0, 0, 4, 0, 0, 0, 0, 0, 0, 0],
     [0, 0, 0, 0, 0, 0, 2, 2, 2, 2, 2, 0],        # label 2: a hole of one pixel
     [0, 0, 0, 0, 0, 0, 2, 2, 0, 2, 2, 0],
     [3, 3, 0, 0, 0, 0, 2, 2, 2, 2, 2, 0],        # label 3: in the bottom left corner
     [3, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]]], np.uint8)
# a ground truth for the scores: the same leaves shifted by a column, label 4 missing
TRUTH = np.where(np.roll(MAPS, 1, axis=2) == 4, 0, np.roll(MAPS, 1, axis=2)).astype(np.uint8)
B, H, W = MAPS.shape


def same(got, want, what):
    got, want = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4].tolist())


@pytest.fixture(scope="module")
def ops():
    _gpu()
    from isa_amd.labelmaps import LabelOps
    return LabelOps()


@pytest.fixture(scope="module")
def maps():
    return torch.from_numpy(MAPS).cuda()


class Recorder:
    """alloc(shape, dtype) for a handle: memory filled with 0xFF, and a list of everything handed out."""

    def __init__(self):
        self.handed = []

    def __call__(self, shape, dtype):
        t = torch.empty(shape, dtype=dtype, device="cuda")
        t.view(-1).view(torch.uint8).fill_(0xFF)
        self.handed.append(t)
        return t

    def owns(self, *tensors):
        """Every tensor starts inside a buffer handed out (the scalars of a loss are elements of one)."""
        spans = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in self.handed]
        return all(any(lo <= t.data_ptr() < hi for lo, hi in spans) for t in tensors)

    def has(self, numel, dtype):
        return any(t.dim() == 1 and t.numel() == numel and t.dtype == dtype for t in self.handed)


# ---------------------------------------------------------------------------------------------- components, distance, contours
@pytest.mark.parametrize("conn", [4, 8])
def test_components_and_clean_instances(ops, maps, conn):
    comp, count = ops.components(maps, connectivity=conn)
    want_comp, want_count = cnp.label(MAPS, conn)
    same(comp, want_comp.astype(np.int32), "components %d" % conn)
    same(count, want_count, "n_components %d" % conn)
    assert want_count.tolist() == ([4, 5] if conn == 4 else [4, 4])                # the corner pair is one piece only under 8
    for got, want, what in ((ops.clean_instances(maps, connectivity=conn), cnp.largest(MAPS, want_comp, 1, 255), "largest"),
                            (ops.clean_instances(maps, keep='all', connectivity=conn, min_area=2, max_objects=3),
                             cnp.split(MAPS, want_comp, 2, 3), "all"),
                            (ops.split_components(maps, connectivity=conn), cnp.split(MAPS, want_comp, 1, 255), "split")):
        for g, w_, part in zip(got, want, ("labels", "n_objects", "dropped")):
            same(g, w_, "%s %d: %s" % (what, conn, part))
    with pytest.raises(ValueError):
        ops.components(maps, connectivity=6)
    with pytest.raises(TypeError):
        ops.components(maps.int())
    with pytest.raises(ValueError):
        ops.components(maps[:, :, :10])


def test_distance_transform_and_fill(ops, maps):
    want = dn.edt2(MAPS)
    got = ops.distance_transform(maps)
    for g, w_, part in zip(got, want, ("d1sq", "d2sq", "nearest")):
        same(g, w_, "distance_transform: " + part)
    fg = np.random.default_rng(3).random(MAPS.shape) < 0.7
    for max_dist in (None, 2):
        out, filled = ops.fill_instances(maps, torch.from_numpy(fg), max_dist)
        want_out, want_filled = dn.fill(MAPS, fg, want[2], want[0], dn.max_dist_sq(max_dist))
        same(out, want_out, "fill_instances max_dist %s" % max_dist)
        same(filled, want_filled, "filled max_dist %s" % max_dist)
        assert want_filled.min() > 0
    with pytest.raises(ValueError):
        ops.distance_transform(maps[:, :, :10])


@pytest.mark.parametrize("conn", [4, 8])
def test_contours_topology_and_polygons(ops, maps, conn):
    wt, wv, wc = C.trace(MAPS, conn, 64, 512)
    assert int(wc[:, 2:].sum()) == 0
    table, verts, counts = ops.contours(maps, connectivity=conn)
    assert tuple(table.shape) == (B, 256, 8) and tuple(verts.shape) == (B, 2048, 2) and counts is ops.last_contour_counts
    same(counts, wc, "contours %d: counts" % conn)
    for i in range(B):
        same(table[i, :wc[i, 0]], wt[i, :wc[i, 0]], "contours %d: table" % conn)
        same(verts[i, :wc[i, 1]], wv[i, :wc[i, 1]], "contours %d: verts" % conn)
    want_topo = C.topology(wt, wc, 256)
    same(ops.instance_topology(maps, connectivity=conn), want_topo, "instance_topology %d" % conn)
    assert want_topo[0, 2].tolist() == [1, 1, 0] and want_topo[0, 1].tolist() == [2, 0, 2]      # the ring, the two pieces
    assert want_topo[1, 4].tolist() == ([2, 0, 2] if conn == 4 else [1, 0, 1])
    polys = ops.polygons(maps, connectivity=conn)
    for i in range(B):
        want = C.polygons(MAPS[i], conn)
        assert len(polys[i]) == len(want)
        for got, ref in zip(polys[i], want):
            assert got["label"] == ref["label"] and len(got["holes"]) == len(ref["holes"])
            same(got["outer"], ref["outer"], "polygons %d image %d: outer" % (conn, i))
            for a, b in zip(got["holes"], ref["holes"]):
                same(a, b, "polygons %d image %d: hole" % (conn, i))


# ---------------------------------------------------------------------------------------------- scores and measurements
def truth_planes():
    return np.stack([(TRUTH == v) for v in (1, 2, 3)], axis=1).astype(np.int64)              # [B,K,H,W]


def test_score_instances(ops, maps):
    planes = truth_planes()
    n_gt, n_pred = np.array([3, 3]), np.array([3, 4])
    fg_pred = MAPS != 0
    fg_gt = np.roll(fg_pred, 1, axis=1)
    sem_arg = torch.from_numpy(fg_pred[:, None].astype(np.float32))
    for compact in (False, True):
        ins_t = torch.from_numpy(planes.transpose(0, 2, 3, 1).astype(np.uint8).copy() if compact else planes)
        sem_t = torch.from_numpy(fg_gt.astype(np.uint8) if compact else
                                 np.stack([~fg_gt, fg_gt], axis=1).astype(np.int64))
        out = ops.score_instances(maps, torch.from_numpy(n_pred), ins_t, torch.from_numpy(n_gt), sem_arg, sem_t, max_objects=4)
        assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (B, 8)
        close_scores(out.cpu().numpy(), host_scores(MAPS, n_pred, planes, n_gt, fg_pred, fg_gt), "compact=%s" % compact)
        assert int(ops.last_score_oob.sum()) == 0
        out2 = ops.score_instances(maps, torch.from_numpy(n_pred), ins_t, torch.from_numpy(n_gt), max_objects=4)
        close_scores(out2.cpu().numpy(), np.stack([S.scores(TRUTH[i], MAPS[i], n_gt[i], n_pred[i]) for i in range(B)]),
                     "label-map foreground, compact=%s" % compact)


def test_instance_properties_and_select(ops, maps):
    rgb = np.random.default_rng(4).integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    want_acc, _ = P.label_props(MAPS, rgb, 256)
    props = ops.instance_properties(maps, torch.from_numpy(rgb))
    assert props.is_cuda and props.dtype == torch.float64 and tuple(props.shape) == (B, 256, 24)
    check_derived(props.cpu().numpy(), P.derive(want_acc, H, W, 3), "instance_properties")
    assert int(ops.last_props_oob.sum()) == 0
    got = ops.select_instances(maps, order='area', min_area=3)
    table, count, dropped = P.select(want_acc, H, W, order=P.ORDER_AREA, min_area=3)
    for g, w_, part in zip(got, (P.relabel(MAPS, table), count, dropped), ("labels", "n_objects", "dropped")):
        same(g, w_, "select_instances: " + part)
    assert dropped.tolist() == [0, 1]                                                     # the corner pair has two pixels


# ---------------------------------------------------------------------------------------------- out-of-range labels
def test_out_of_range_labels_raise_or_stay_counted(ops, maps):
    ins_t, n = torch.from_numpy(truth_planes()), torch.tensor([3, 3])
    with pytest.raises(ValueError, match="outside the histogram"):
        ops.score_instances(maps, n, ins_t, n, max_objects=0)
    ops.score_instances(maps, n, ins_t, n, max_objects=0, check=False)
    same(ops.last_score_oob, np.stack([(MAPS > 0).sum(axis=(1, 2)), np.zeros(B)]).astype(np.int32), "last_score_oob")
    wide = torch.zeros((1, H, W, 64), dtype=torch.uint8)
    with pytest.raises(ValueError, match="16384"):                                        # 65 x 256 counters
        ops.score_instances(maps[:1], n[:1], wide, n[:1])
    with pytest.raises(ValueError, match="n_labels = 2"):
        ops.instance_properties(maps, n_labels=2)
    small = ops.instance_properties(maps, n_labels=2, check=False)
    assert tuple(small.shape) == (B, 2, 24)
    same(ops.last_props_oob, (MAPS >= 2).sum(axis=(1, 2)).astype(np.int32), "last_props_oob")
    with pytest.raises(ValueError, match="max_contours = 1"):
        ops.contours(maps, max_contours=1)
    _, _, counts = ops.contours(maps, max_contours=1, check=False)
    assert counts is ops.last_contour_counts
    same(counts, C.trace(MAPS, 8, 1, 2048)[2], "last_contour_counts")


# ---------------------------------------------------------------------------------------------- the alloc hook
def embedding():
    """fp32 [2,4,8,12]: a centre per label of MAPS and a little noise around it."""
    rs = np.random.RandomState(5)
    centres = rs.standard_normal((5, 4)) * 2.0
    x = centres[MAPS] + rs.standard_normal((B, H, W, 4)) * 0.1
    return torch.from_numpy(x.transpose(0, 3, 1, 2).astype(np.float32).copy()).cuda()


def test_a_recording_poisoning_alloc_gives_the_same_bytes(ops, maps):
    from isa_amd import lib as L
    from isa_amd.labelmaps import LabelOps
    rec = Recorder()
    hooked = LabelOps(alloc=rec)
    # border weights: d1sq, d2sq, the transform's scratch, the map
    w_def, w_hook = ops.border_weights(maps), hooked.border_weights(maps)
    assert torch.equal(w_def, w_hook) and float(w_def.max()) > 1.0
    assert rec.owns(w_hook) and len(rec.handed) == 4 and rec.has(L.edt_scratch_bytes(B, H, W), torch.uint8)
    # clustering with one refinement pass: five outputs, the scratch, and the refinement's copies of counts and centres
    emb, fg = embedding(), maps != 0
    del rec.handed[:]
    kw = dict(bandwidth=1.0, max_objects=8, refine=1)
    c_def, c_hook = ops.cluster_embedding(emb, fg, **kw), hooked.cluster_embedding(emb, fg, **kw)
    assert sorted(c_def) == sorted(c_hook) == ["centres", "labels", "moved", "n_objects", "sizes"]
    for key in c_def:
        assert torch.equal(c_def[key].contiguous().view(torch.uint8), c_hook[key].contiguous().view(torch.uint8)), key
    assert c_def["n_objects"].tolist() == [3, 4] and torch.equal(c_def["labels"] != 0, fg)
    assert rec.owns(*c_hook.values()) and len(rec.handed) == 8 and rec.has(L.cluster_scratch_bytes(B, H * W), torch.uint8)
    # the loss and its gradient: twelve scratch and result buffers of the forward launches, then the gradient
    del rec.handed[:]
    n = torch.tensor([3, 4])
    kw = dict(delta_var=0.05, delta_dist=3.0, form='full', grad=True)
    d_def, d_hook = ops.discriminative_loss(emb, maps, n, **kw), hooked.discriminative_loss(emb, maps, n, **kw)
    assert sorted(d_def) == sorted(d_hook) == ["dist", "grad", "loss", "means", "qreg", "reg", "var"]
    for key in d_def:
        assert torch.equal(d_def[key].contiguous().view(-1).view(torch.uint8),
                           d_hook[key].contiguous().view(-1).view(torch.uint8)), key
    assert float(d_def["loss"]) > 0 and float(d_def["grad"].abs().max()) > 0 and bool(torch.isfinite(d_def["grad"]).all())
    assert rec.owns(*d_hook.values()) and len(rec.handed) == 13


# ---------------------------------------------------------------------------------------------- evaluate.py --device
def test_evaluate_device_scores_is_score_instances(ops):
    from evaluate import device_scores
    rs = np.random.RandomState(6)
    a, b = rs.randint(0, 4, (6, 10)), rs.randint(0, 6, (6, 10))                 # 60 pixels: device_scores pads them to 60
    assert a.max() == 3 and b.max() == 5
    got = device_scores(a, b, 3, 5)
    pad = lambda m: np.pad(m, ((0, 0), (0, 2))).astype(np.uint8)[None]          # [1,6,12]: the same two zero pixels more
    planes = np.stack([pad(a) == v for v in (1, 2, 3)], axis=-1).astype(np.uint8)
    want = ops.score_instances(torch.from_numpy(pad(b)), torch.tensor([5]), torch.from_numpy(planes), torch.tensor([3]),
                               max_objects=5)
    assert np.array_equal(got.view(np.uint64), want[0].cpu().numpy().view(np.uint64)), (got, want)
    close_scores(got, S.scores(a, b, 3, 5), "device_scores")
