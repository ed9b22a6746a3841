"""Scoring instance predictions on the GPU: isa_labels_from_planes / isa_label_pair_hist / isa_instance_scores,
ReSeg.score_instances, Model.evaluate, evaluate.py --device and fit()'s validation_scores.log.

1. Planes -> labels: integer equality with numpy, both target layouts (and the fp32 map form).
2. The joint histogram: integer equality of hist and oob with np.bincount, two runs bit-identical.
3. The scores against evaluate.py's host functions in float64 (tests/score_np.py), |diff| <= 1e-12: a pair Dice is ONE
   correctly rounded double division of exact integers on both sides, so the two can differ only in the order in which at
   most 255 values in [0, 1] are summed, which is bounded by about 255 * 2^-53 = 3e-14; 1e-12 leaves a margin of 30.  NaN
   positions must match exactly.
4. segment() -> score_instances() against evaluate.py on the downloaded maps (both see the same device labels, so the
   storage precision does not enter: the same 1e-12).
5. Model.evaluate, 6. evaluate.py --device, 7. fit() with and without val_scores.
Outputs of the kernels sit inside sentinel-padded buffers whose padding must stay unchanged.

Measured on MI355X (the SCORE lines): histograms and labels integer-equal; scores at most 3.4e-16 from the host functions
(127 x 127 objects), 0 in every other case; the file runs in about 15 s."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import reseg_ref as R           # noqa: E402
import score_np as S            # noqa: E402
from test_gpu_ops import _gpu   # noqa: E402

PAD = 64                        # elements of padding on either side of every output (keeps 16-byte alignment)
TOL = 1e-12
DTYPES = [torch.float32, torch.bfloat16]


def _lib():
    L = _gpu()[0]
    return L, L.lib()


class Padded:
    """`numel` elements between two runs of PAD sentinel elements."""

    def __init__(self, numel, dtype, fill):
        self.numel, self.fill = numel, fill
        self.buf = torch.full((numel + 2 * PAD,), fill, dtype=dtype, device="cuda")
        self.view = self.buf[PAD:PAD + numel]

    def pads_unchanged(self):
        b = self.buf.cpu()
        return bool((b[:PAD] == self.fill).all()) and bool((b[PAD + self.numel:] == self.fill).all())


def close(got, want, what):
    """NaN in the same places, the numbers within TOL."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN positions", got, want)
    ok = ~np.isnan(want)
    diff = np.abs(got[ok] - want[ok])
    print("SCORE %s: max |diff| %.3e over %d numbers" % (what, diff.max() if diff.size else 0.0, diff.size))
    assert (diff <= TOL).all(), (what, float(diff.max()), got, want)


# ---- 1. planes -> labels --------------------------------------------------------------------------------------------
def random_planes(n, k, h, w, seed):
    """[n,k,h,w] {0,1} planes: disjoint blobs, then overlaps (a pixel in several planes) and pixels in none."""
    rs = np.random.RandomState(seed)
    owner = rs.randint(0, k + 1, (n, h, w))                          # 0: no plane
    planes = np.zeros((n, k, h, w), np.int64)
    for j in range(k):
        planes[:, j] = owner == j + 1
    extra = rs.rand(n, k, h, w) < 0.02                               # overlaps: any plane may also claim any pixel
    planes |= extra.astype(np.int64)
    planes[:, :, : h // 4] = 0                                       # a band that is all zero
    return planes


@pytest.mark.parametrize("k", [1, 32, 255])
@pytest.mark.parametrize("layout", ["u8_nhwk", "i64_nkhw", "f32_nkhw"])
def test_labels_from_planes(layout, k):
    L, lib = _lib()
    n, h, w = 3, 20, 24 if k < 255 else 12
    planes = random_planes(n, k, h, w, seed=k)
    assert (k == 1 or (planes.sum(1) > 1).any()) and (planes.sum(1) == 0).any()
    want = S.labels_from_planes(planes, pixel_major=False)
    assert want.max() == k or k == 255
    if layout == "u8_nhwk":
        dev = torch.from_numpy(np.ascontiguousarray(np.moveaxis(planes, 1, -1)).astype(np.uint8) * 3).cuda()
        form = L.PLANES_U8_NHWK
    elif layout == "i64_nkhw":
        dev, form = torch.from_numpy(planes * -5).cuda(), L.PLANES_I64_NKHW
    else:
        dev, form = torch.from_numpy(planes.astype(np.float32) * 0.25).cuda(), L.PLANES_F32_NKHW
    out = Padded(n * h * w, torch.uint8, 0xFF)
    L.check(lib.isa_labels_from_planes(L.ptr(dev), form, n, k, h * w, L.ptr(out.view), L.stream_ptr()),
            "isa_labels_from_planes")
    torch.cuda.synchronize()
    got = out.view.cpu().numpy().reshape(n, h, w)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert out.pads_unchanged()


# ---- 2. the joint histogram -----------------------------------------------------------------------------------------
def label_maps(dist, n, Lp, na, nb, seed):
    rs = np.random.RandomState(seed)
    if dist == "uniform":
        a, b = rs.randint(0, na, (n, Lp)), rs.randint(0, nb, (n, Lp))
    elif dist == "background":                                       # at least 95 % of the pixels are the pair (0, 0)
        keep = np.zeros((n, Lp), bool)                               # exactly 4 % of the pixels may differ (none at L = 4)
        for i in range(n):
            keep[i, rs.choice(Lp, Lp * 4 // 100, replace=False)] = True
        a, b = rs.randint(0, na, (n, Lp)) * keep, rs.randint(0, nb, (n, Lp)) * keep
    elif dist == "single":                                           # one single pair
        a, b = np.full((n, Lp), na - 1), np.full((n, Lp), nb - 1)
    else:                                                            # values at and above na / nb (where uint8 allows)
        a, b = rs.randint(0, min(na + 3, 256), (n, Lp)), rs.randint(0, min(nb + 3, 256), (n, Lp))
        a[:, 0], b[:, 0] = min(na, 255), 0
    return a.astype(np.uint8), b.astype(np.uint8)


def run_hist(L, lib, a_dev, b_dev, n, Lp, na, nb, mode=0):
    hist, oob = Padded(n * na * nb, torch.int32, -7), Padded(n, torch.int32, -7)
    L.check(lib.isa_label_pair_hist(L.ptr(a_dev), L.ptr(b_dev), n, Lp, na, nb, L.ptr(hist.view), L.ptr(oob.view), mode,
                                    L.stream_ptr()), "isa_label_pair_hist")
    torch.cuda.synchronize()
    assert hist.pads_unchanged() and oob.pads_unchanged()
    return hist.view.cpu().numpy().reshape(n, na, nb), oob.view.cpu().numpy()


@pytest.mark.parametrize("dist", ["uniform", "background", "single", "outside"])
@pytest.mark.parametrize("na,nb", [(1, 1), (2, 2), (33, 33), (33, 256), (128, 128)])
@pytest.mark.parametrize("Lp", [4, 4096, 65536, 1024 * 1024])
@pytest.mark.parametrize("n", [1, 16])
def test_pair_hist(n, Lp, na, nb, dist):
    L, lib = _lib()
    a, b = label_maps(dist, n, Lp, na, nb, seed=n + Lp % 1001 + na * 7 + nb)
    if dist == "background":
        assert ((a == 0) & (b == 0)).mean() >= 0.95
    want_h, want_o = S.pair_hist(a, b, na, nb)
    if dist == "outside" and (na < 256 or nb < 256):
        assert want_o.min() > 0
    a_dev, b_dev = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    got_h, got_o = run_hist(L, lib, a_dev, b_dev, n, Lp, na, nb)
    assert np.array_equal(got_h, want_h), np.argwhere(got_h != want_h)[:4]
    assert np.array_equal(got_o, want_o), (got_o, want_o)
    again_h, again_o = run_hist(L, lib, a_dev, b_dev, n, Lp, na, nb)
    assert np.array_equal(again_h, got_h) and np.array_equal(again_o, got_o)
    assert (got_h.sum((1, 2)) + got_o == Lp).all()


@pytest.mark.parametrize("Lp", [4, 1020, 4096, 4100, 65536 + 8])
def test_pair_hist_four_pixel_loads_offsets_and_the_plain_counter(Lp):
    """L % 16 != 0 or maps that are only 4-byte aligned (L = 4096 at offset 4) take the 4-pixel loads; the
    one-atomic-per-pixel mode counts the same."""
    L, lib = _lib()
    n, na, nb = 3, 9, 11
    a, b = label_maps("outside", n, Lp, na, nb, seed=Lp)
    want_h, want_o = S.pair_hist(a, b, na, nb)
    store_a = torch.zeros(n * Lp + 16, dtype=torch.uint8, device="cuda")
    store_b = torch.zeros(n * Lp + 16, dtype=torch.uint8, device="cuda")
    for off in (0, 4):
        va, vb = store_a[off:off + n * Lp], store_b[off:off + n * Lp]
        va.copy_(torch.from_numpy(a).reshape(-1)); vb.copy_(torch.from_numpy(b).reshape(-1))
        for mode in (L.HIST_AGGREGATE, L.HIST_NAIVE):
            got_h, got_o = run_hist(L, lib, va, vb, n, Lp, na, nb, mode)
            assert np.array_equal(got_h, want_h) and np.array_equal(got_o, want_o), (off, mode)


# ---- 3. the scores --------------------------------------------------------------------------------------------------
def device_scores(a, b, na, nb, n_a=None, n_b=None):
    """a, b: uint8 numpy [n, L]; returns float64 [n, 8]."""
    L, lib = _lib()
    n, Lp = a.shape
    a_dev, b_dev = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    hist = torch.empty(n * na * nb, dtype=torch.int32, device="cuda")
    oob = torch.empty(n, dtype=torch.int32, device="cuda")
    L.check(lib.isa_label_pair_hist(L.ptr(a_dev), L.ptr(b_dev), n, Lp, na, nb, L.ptr(hist), L.ptr(oob), 0,
                                    L.stream_ptr()), "isa_label_pair_hist")
    cnt = lambda v: None if v is None else torch.tensor(v, dtype=torch.int32, device="cuda")
    ca, cb = cnt(n_a), cnt(n_b)
    out = Padded(n * 8, torch.float64, -7.0)
    L.check(lib.isa_instance_scores(L.ptr(hist), n, na, nb, L.ptr(ca), L.ptr(cb), L.ptr(out.view), L.stream_ptr()),
            "isa_instance_scores")
    torch.cuda.synchronize()
    assert out.pads_unchanged() and int(oob.sum()) == 0
    return out.view.cpu().numpy().reshape(n, 8)


def blobs(n, h, w, ids, seed, fg_share=0.6):
    """Label maps [n, h*w] whose objects are vertical stripes of random width carrying the given ids."""
    rs = np.random.RandomState(seed)
    out = np.zeros((n, h, w), np.uint8)
    for i in range(n):
        cuts = np.sort(rs.choice(np.arange(1, w), len(ids) - 1, replace=False)) if len(ids) > 1 else np.array([], int)
        for j, (x0, x1) in enumerate(zip(np.r_[0, cuts], np.r_[cuts, w])):
            out[i, :, x0:x1] = ids[j]
        out[i][rs.rand(h, w) > fg_share] = 0
    return out.reshape(n, -1)


def test_scores_non_contiguous_ids_and_counts():
    """Ids with gaps (labels 3, 7, 200 present, the others absent); n_a / n_b given, one given, and NULL."""
    n = 4
    a = blobs(n, 32, 64, [3, 7, 200, 9], seed=1)
    b = blobs(n, 32, 64, [1, 2, 40, 41, 80], seed=2)
    want = np.stack([S.scores(a[i], b[i]) for i in range(n)])
    assert (want[:, 3] == 4).all() and (want[:, 4] == 5).all()
    close(device_scores(a, b, 201, 81), want, "ids with gaps, counts NULL")      # 201 * 81 = 16281 counters
    n_a, n_b = [4, 9, 0, 2], [5, 1, 7, 2]
    want_c = np.stack([S.scores(a[i], b[i], n_a[i], n_b[i]) for i in range(n)])
    assert want_c[:, 5].tolist() == [1.0, 8.0, 7.0, 0.0]
    close(device_scores(a, b, 201, 81, n_a, n_b), want_c, "ids with gaps, counts given")
    want_one = np.stack([S.scores(a[i], b[i], n_a[i], None) for i in range(n)])
    close(device_scores(a, b, 201, 81, n_a, None), want_one, "n_a given, n_b NULL")


def test_scores_many_objects():
    """127 objects a side, random pixels: the longest sums."""
    rs = np.random.RandomState(3)
    a = rs.randint(0, 128, (2, 128 * 128)).astype(np.uint8)
    b = np.where(rs.rand(2, 128 * 128) < 0.7, a, rs.randint(0, 128, (2, 128 * 128))).astype(np.uint8)
    want = np.stack([S.scores(a[i], b[i]) for i in range(2)])
    assert (want[:, 3] == 127).all()
    close(device_scores(a, b, 128, 128), want, "127 x 127 objects")
    a255 = (rs.randint(0, 256, (1, 256 * 256))).astype(np.uint8)
    b1 = (rs.rand(1, 256 * 256) < 0.5).astype(np.uint8)
    want = np.stack([S.scores(a255[0], b1[0])])
    assert want[0, 3] == 255
    close(device_scores(a255, b1, 256, 2), want, "255 objects against one")


def test_scores_empty_maps():
    """Both maps empty: NaN, NaN, NaN and a NaN foreground Dice; exactly one empty: SBD 0.0 (evaluate.calc_bd raises
    there), foreground Dice 0.0."""
    full = blobs(1, 16, 16, [1, 2, 5], seed=4)[0]
    zero = np.zeros_like(full)
    a = np.stack([zero, zero, full, full])
    b = np.stack([zero, full, zero, full])
    want = np.stack([S.scores(a[i], b[i]) for i in range(4)])
    assert np.isnan(want[0, [0, 1, 2, 6]]).all() and want[0, 5] == 0
    assert np.isnan(want[1, 0]) and want[1, 1] == 0.0 and want[1, 2] == 0.0 and want[1, 6] == 0.0
    assert want[2, 0] == 0.0 and np.isnan(want[2, 1]) and want[2, 2] == 0.0
    assert want[3, 2] == 1.0 and want[3, 6] == 1.0
    with pytest.raises(ValueError):
        S.EV.calc_bd(full.reshape(16, 16), zero.reshape(16, 16))
    close(device_scores(a, b, 6, 6), want, "empty maps")


def test_scores_two_by_two_is_calc_dice():
    rs = np.random.RandomState(5)
    a = (rs.rand(5, 4096) < 0.3).astype(np.uint8)
    b = np.where(rs.rand(5, 4096) < 0.8, a, 1 - a).astype(np.uint8)
    got = device_scores(a, b, 2, 2)
    want = np.array([S.EV.calc_dice(a[i] == 1, b[i] == 1) for i in range(5)])
    close(got[:, 6], want, "2 x 2 foreground Dice")
    close(got, np.stack([S.scores(a[i], b[i]) for i in range(5)]), "2 x 2 all columns")


# ---- 4. segment -> score_instances ----------------------------------------------------------------------------------
def build(dtype):
    _gpu()
    from isa_amd.reseg import ReSeg
    m = ReSeg(2, True, dtype=dtype)
    m.load_state_dict(R.synth_state_dict())
    m.eval()
    m.head.drop_rate = 0.0
    return m


def host_scores(labels, n_pred, ins_planes, n_gt, fg_pred, fg_gt):
    """evaluate.py on downloaded maps: labels [B,H,W], ins_planes [B,K,H,W], fg_* boolean [B,H,W]."""
    gt = S.labels_from_planes(ins_planes, pixel_major=False)
    rows = []
    for i in range(labels.shape[0]):
        row = S.scores(gt[i], labels[i], n_gt[i], n_pred[i])
        row[6] = S.EV.calc_dice(fg_gt[i], fg_pred[i]) if (fg_gt[i].any() or fg_pred[i].any()) else S.NAN
        rows.append(row)
    return np.stack(rows)


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_segment_then_score(dtype, compact):
    B, size, cap = 3, 64, 6
    x, sem, ins, n = R.synth_batch(B, size, size, seed=7)
    m = build(dtype)
    _, sem_arg, labels, count = m.segment(x, max_objects=cap)
    if compact:
        sem_t, ins_t = sem[:, 1].contiguous().to(torch.uint8), ins.permute(0, 2, 3, 1).contiguous().to(torch.uint8)
    else:
        sem_t, ins_t = sem, ins
    out = m.score_instances(labels, count, ins_t, n, sem_arg, sem_t, max_objects=cap)
    assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (B, 8)
    lab = labels.cpu().numpy()
    want = host_scores(lab, count.cpu().numpy(), ins.numpy(), n.view(-1).numpy(), sem_arg.cpu().numpy()[:, 0] > 0.5,
                       sem[:, 1].numpy() == 1)
    assert lab.max() >= 1, "the case must hold predicted instances"
    close(out.cpu().numpy(), want, "segment -> score_instances %s compact=%s" % (dtype, compact))
    # without the semantic pair column 6 compares the foregrounds of the label maps
    out2 = m.score_instances(labels, count, ins_t, n, max_objects=cap, check=False)
    gt = S.labels_from_planes(ins.numpy(), pixel_major=False)
    close(out2.cpu().numpy(), np.stack([S.scores(gt[i], lab[i], int(n.view(-1)[i]), int(count[i])) for i in range(B)]),
          "label-map foreground")
    assert int(m.last_score_oob.sum()) == 0
    # labels above the stated cap: an error that names the limit, not a silently smaller score
    with pytest.raises(ValueError, match="outside the histogram"):
        m.score_instances(labels, count, ins_t, n, max_objects=0)


# ---- 5. Model.evaluate ----------------------------------------------------------------------------------------------
def test_model_evaluate():
    _gpu()
    from isa_amd.model import Model
    from isa_amd.data import SyntheticLoader
    cap = 5
    model = Model("CVPPP", "ReSeg", 2, cap, use_instance_segmentation=True)
    batches = list(SyntheticLoader(2, 2, 64, 64, seed=5)) + list(SyntheticLoader(1, 2, 64, 64, seed=9, compact=True))
    res = model.evaluate(batches)
    assert sorted(res) == sorted(["SBD", "|DiC|", "FG Dice", "n_images", "n_skipped", "per_image"])
    rows = []
    for x, sem, ins, n in batches:
        _, sem_arg, labels, count = model.model.segment(x, cap)
        if ins.dtype == torch.uint8:
            ins, fg_gt = ins.permute(0, 3, 1, 2), sem.numpy() == 1
        else:
            fg_gt = sem[:, 1].numpy() == 1
        rows.append(host_scores(labels.cpu().numpy(), count.cpu().numpy(), ins.numpy(), n.view(-1).numpy(),
                                sem_arg.cpu().numpy()[:, 0] > 0.5, fg_gt))
    want = np.concatenate(rows)
    assert res["n_images"] == 6 and res["per_image"].shape == (6, 8) and res["per_image"].dtype == np.float64
    close(res["per_image"], want, "Model.evaluate per image")
    assert res["n_skipped"] == int(np.isnan(want[:, 2]).sum())
    with np.errstate(all="ignore"):
        close([res["SBD"], res["|DiC|"], res["FG Dice"]],
              [np.nanmean(want[:, 2]), np.nanmean(want[:, 5]), np.nanmean(want[:, 6])], "Model.evaluate means")
    empty = model.evaluate([])
    assert empty["n_images"] == 0 and empty["n_skipped"] == 0 and empty["SBD"] != empty["SBD"]
    sem_only = Model("CVPPP", "ReSeg", 2, cap, use_instance_segmentation=False)
    with pytest.raises(RuntimeError):
        sem_only.evaluate(batches)


# ---- 6. evaluate.py --device ----------------------------------------------------------------------------------------
def test_evaluate_script_on_the_device(tmp_path):
    """A synthetic prediction directory and data root in the layout evaluate.py walks (the one pred_list.py --instances
    writes); image sizes that are and are not multiples of 4 pixels; the three printed numbers within 1e-12."""
    from PIL import Image
    _gpu()
    pred, root = tmp_path / "pred", tmp_path / "data"
    img_dir = root / "raw/CVPPP/CVPPP2017_LSC_training/training/A1"
    os.makedirs(img_dir)
    os.makedirs(root / "metadata/CVPPP")
    names, rows = [], []
    for i, (h, w) in enumerate([(48, 64), (51, 37), (30, 30), (64, 64)]):
        name = "plant%03d_rgb" % i
        stem = name.replace("_rgb", "")
        gt = blobs(1, h, w, [1, 2, 3, 4, 5, 6][: 3 + i], seed=20 + i).reshape(h, w)
        pr = blobs(1, h, w, [1, 2, 3, 4][: 2 + i % 3], seed=40 + i).reshape(h, w)
        os.makedirs(pred / name)
        Image.fromarray(pr).save(pred / name / (name + "-ins_mask.png"))
        Image.fromarray(((pr != 0) * 255).astype(np.uint8)).save(pred / name / (name + "-fg_mask.png"))
        np.save(pred / name / (name + "-n_objects.npy"), np.int64(len(np.unique(pr)) - 1 + (i == 2)))
        Image.fromarray(gt).save(img_dir / (stem + "_label.png"))
        Image.fromarray((gt != 0).astype(np.uint8)).save(img_dir / (stem + "_fg.png"))
        names.append(name)
        rows.append("%s,%d" % (stem, len(np.unique(gt)) - 1))
    (root / "metadata/CVPPP/validation_image_paths.txt").write_text("".join("x/%s.png\n" % nm for nm in names))
    (root / "metadata/CVPPP/number_of_instances.txt").write_text("\n".join(rows) + "\n")
    printed = []
    for extra in ([], ["--device"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--pred_dir", str(pred), "--dataset", "CVPPP",
                            "--data_root", str(root)] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.strip().splitlines()
        assert [ln.split(":")[0].strip() for ln in lines] == ["MEAN SBD", "MEAN |DIC|", "MEAN FG DICE"], r.stdout
        printed.append([float(re.split(r":\s+", ln)[1]) for ln in lines])
    assert 0.0 < printed[0][0] < 1.0 and printed[0][1] > 0.0 and 0.0 < printed[0][2] < 1.0
    close(printed[1], printed[0], "evaluate.py --device against evaluate.py")
    # ids beyond the histogram: the error names the limit
    sys.path.insert(0, ROOT)
    from evaluate import device_scores as script_scores
    wide = np.arange(256, dtype=np.uint8).reshape(16, 16)
    with pytest.raises(ValueError, match="16384"):
        script_scores(wide, wide)


# ---- 7. fit() -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", [True, False])
def test_fit_validation_scores_log(tmp_path, on):
    _gpu()
    from isa_amd.model import Model
    from isa_amd.data import SyntheticLoader
    m = Model("CVPPP", "ReSeg", 2, 4, use_instance_segmentation=True)
    assert m.val_scores is False
    m.val_scores = on
    tr, te = SyntheticLoader(2, 2, 64, 64, seed=1), SyntheticLoader(2, 2, 64, 64, seed=2, compact=on)
    m.fit('Multi', 0.5, 1.5, 2, 1.0, 0.001, 10.0, 0.5, 25, False, 'Adadelta', True, 2, None, tr, te, str(tmp_path), False)
    vlog = open(os.path.join(str(tmp_path), "validation.log")).read().strip().splitlines()
    assert vlog[0] == "Epoch,Cost" and len(vlog) == 3 and [ln.split(",")[0] for ln in vlog[1:]] == ["0", "1"]
    assert all(np.isfinite(float(ln.split(",")[1])) for ln in vlog[1:])
    path = os.path.join(str(tmp_path), "validation_scores.log")
    if not on:
        assert not os.path.exists(path)
        return
    slog = open(path).read().strip().splitlines()
    assert slog[0] == "Epoch,SBD,DiC,FG Dice" and len(slog) == 3
    for epoch, ln in enumerate(slog[1:]):
        cells = ln.split(",")
        assert len(cells) == 4 and int(cells[0]) == epoch
        vals = [float(c) for c in cells[1:]]
        assert all(v != v or np.isfinite(v) for v in vals), ln
        assert all(v != v or 0.0 <= v <= 1.0 for v in (vals[0], vals[2])) and (vals[1] != vals[1] or vals[1] >= 0.0)
