"""Scoring K-class semantic predictions on the GPU: isa_sem_confusion / isa_sem_scores, ReSeg.class_map /
score_semantic / semantic_scores, Model.predict_classes / evaluate_semantic, fit()'s validation_sem_scores.log and
pred_list.py --n-classes.

1. isa_sem_confusion against the numpy restatement (tests/sem_score_np.py): INTEGER EQUALITY of the class map, the
   confusion matrix and the out-of-range counts.  The kernel and numpy see the same stored logits (bf16 inputs are rounded
   on the host and numpy gets the rounded values), so there is no margin and no pixel is left out.
2. isa_sem_scores against scores(): columns 0, 3 and every per-class column exactly equal (one correctly rounded double
   division of exact integers on both sides), NaN positions equal, the two means within 1e-12 (sums of at most 32 values in
   [0, 1] can differ from numpy's only by summation order, below 32 * 2^-53 = 4e-15).
3. Through the network, 4. Model.evaluate_semantic and predict_classes, 5. fit(), 6. pred_list.py.
Outputs of the kernels sit inside sentinel-padded buffers whose padding must stay unchanged.

Measured on MI355X (the SEMSCORE lines): class maps, confusion matrices and counts integer-equal in all cases; the means
0 away from numpy in every case; predict_classes: 0 pixels excluded; the file (109 tests) runs in about 17 s."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import reseg_ref as R           # noqa: E402
import sem_score_np as S        # noqa: E402
from test_gpu_ops import _gpu   # noqa: E402

PAD = 64                        # elements of padding on either side of every output (keeps 16-byte alignment)
TOL = 1e-12
DTYPES = [torch.float32, torch.bfloat16]
INF, NAN = float("inf"), float("nan")


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


def rup8(k):
    return (k + 7) // 8 * 8


# ---- 1. isa_sem_confusion -------------------------------------------------------------------------------------------
def make_logits(K, n, Lp, ld, dtype, seed, pad_fill, background=None):
    """(device tensor [n, Lp, ld] of `dtype`, the same values as float32 numpy).  Half of the pixels draw from seven
    half-integers, so exact ties inside and across the 8-channel vectors are everywhere; the others are normal deviates
    (rounded to the storage type).  Then NaN pixels, all -inf pixels and +inf ties; the first four pixels of every image
    hold one of each kind.  background: boolean [n, Lp], pixels whose class 0 must win.  Channels K..ld-1 = pad_fill."""
    rs = np.random.RandomState(seed)
    x = np.where(rs.rand(n, Lp, 1) < 0.5, rs.randint(-3, 4, (n, Lp, ld)) * 0.5, rs.standard_normal((n, Lp, ld))).astype(np.float32)
    kind = rs.rand(n, Lp)
    kind[:, :4] = [0.005, 0.015, 0.025, 0.5]
    pix = np.arange(Lp)
    for i in range(n):
        for p in pix[kind[i] < 0.01]:                                 # one or two NaN channels
            x[i, p, rs.randint(0, K, 2)] = NAN
        x[i, (kind[i] >= 0.01) & (kind[i] < 0.02)] = -INF             # all -inf
        for p in pix[(kind[i] >= 0.02) & (kind[i] < 0.03)]:           # +inf in two channels (possibly one)
            x[i, p, rs.randint(0, K, 2)] = INF
    x[:, 3, :K] = 1.5                                                 # pixel 3: all K channels tie
    if background is not None:
        x[..., 0] = np.where(background, 100.0, x[..., 0])
        x[..., 1:] = np.where(background[..., None] & ~np.isfinite(x[..., 1:]), 0.0, x[..., 1:])
    x[..., K:] = pad_fill
    dev = torch.from_numpy(x).to(dtype).cuda()
    return dev, dev.float().cpu().numpy()


def make_labels(dist, n, Lp, K, seed):
    """(labels uint8 [n, Lp], background mask or None)"""
    rs = np.random.RandomState(seed)
    if dist == "uniform":
        return rs.randint(0, K, (n, Lp)).astype(np.uint8), None
    if dist == "single":
        return np.full((n, Lp), K - 1, np.uint8), None
    if dist == "background":                                          # at least 95 % of the pixels are the pair (0, 0)
        keep = np.zeros((n, Lp), bool)
        for i in range(n):
            keep[i, rs.choice(Lp, Lp * 4 // 100, replace=False)] = True
        return (rs.randint(0, K, (n, Lp)) * keep).astype(np.uint8), ~keep
    lab = rs.randint(0, K + 3, (n, Lp)).astype(np.uint8)              # labels at and above K
    lab[:, 0], lab[:, 1] = K, 255
    return lab, None


def tensor_desc(L, dev, n, Lp, K, ld, dtype):
    return L.IsaTensor(dev.data_ptr(), n, 4, Lp // 4, K, ld, L.dtype_code(dtype), 1)


def run_confusion(L, lib, desc, labels_dev, n, Lp, K, want_map=True, want_conf=True):
    conf, oob = Padded(n * K * K, torch.int64, -7), Padded(n, torch.int32, -7)
    cmap = Padded(n * Lp, torch.uint8, 0xEE)
    import ctypes as C
    L.check(lib.isa_sem_confusion(C.byref(desc), L.ptr(labels_dev) if want_conf else None, K, L.ptr(conf.view),
                                  L.ptr(oob.view), L.ptr(cmap.view) if want_map else None, L.stream_ptr()),
            "isa_sem_confusion")
    torch.cuda.synchronize()
    assert conf.pads_unchanged() and oob.pads_unchanged() and cmap.pads_unchanged()
    return conf.view.cpu().numpy().reshape(n, K, K), oob.view.cpu().numpy(), cmap.view.cpu().numpy().reshape(n, Lp)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Lp", [4, 256, 4100, 65536])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("K", [2, 3, 8, 9, 32])
def test_sem_confusion(K, n, Lp, dtype):
    L, lib = _lib()
    ld = rup8(K)
    for j, dist in enumerate(["uniform", "background", "single", "outside"]):
        seed = K * 1000 + n * 100 + Lp % 997 + j
        labels, bg = make_labels(dist, n, Lp, K, seed)
        dev, x = make_logits(K, n, Lp, ld, dtype, seed + 1, INF if j % 2 == 0 and ld > K else NAN, bg)
        want_map = S.class_map(x, K)
        want_conf, want_oob = S.confusion(labels, want_map, K)
        if dist == "background":
            assert (want_conf[:, 0, 0] >= Lp * 95 // 100).all()
        if dist == "outside":
            assert (want_oob >= 2).all()
        lab_dev = torch.from_numpy(labels).cuda()
        desc = tensor_desc(L, dev, n, Lp, K, ld, dtype)
        conf, oob, cmap = run_confusion(L, lib, desc, lab_dev, n, Lp, K)
        assert np.array_equal(cmap, want_map), (dist, np.argwhere(cmap != want_map)[:4])
        assert np.array_equal(conf, want_conf), (dist, conf, want_conf)
        assert np.array_equal(oob, want_oob), (dist, oob, want_oob)
        assert (conf.sum((1, 2)) + oob == Lp).all()
        if j == 0:
            conf2, oob2, cmap2 = run_confusion(L, lib, desc, lab_dev, n, Lp, K)          # two runs are bit-identical
            assert np.array_equal(conf2, conf) and np.array_equal(oob2, oob) and np.array_equal(cmap2, cmap)
            # class_map = NULL: the counters alone
            conf3, oob3, cmap3 = run_confusion(L, lib, desc, lab_dev, n, Lp, K, want_map=False)
            assert np.array_equal(conf3, conf) and np.array_equal(oob3, oob) and (cmap3 == 0xEE).all()
            # labels = NULL: the class map alone, the sentinel-filled conf and oob stay as they are
            conf4, oob4, cmap4 = run_confusion(L, lib, desc, lab_dev, n, Lp, K, want_conf=False)
            assert np.array_equal(cmap4, cmap) and (conf4 == -7).all() and (oob4 == -7).all()


def test_sem_confusion_special_pixels_are_present():
    """The generator really produces what the case list promises (checked once, on the host values of one case)."""
    _lib()
    K, ld = 9, 16
    _, x = make_logits(K, 1, 4100, ld, torch.bfloat16, 3, NAN)
    v = x[0, :, :K]
    assert np.isnan(v).any(1).sum() > 10 and (v == -INF).all(1).sum() > 10 and ((v == INF).sum(1) == 2).sum() > 5
    mx = np.nanmax(np.where(np.isnan(v), -INF, v), 1)
    tie = (v == mx[:, None])
    assert (tie[:, :8].any(1) & tie[:, 8:].any(1)).sum() > 10, "ties across the two 8-channel vectors"
    assert (tie[:, :8].sum(1) > 1).sum() > 10, "ties inside a vector"
    assert np.isnan(x[0, :, K:]).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K,ld,c0,width", [(3, 16, 8, 32), (9, 24, 0, 24), (32, 32, 16, 64)])
def test_sem_confusion_on_a_view_into_a_wider_buffer(K, ld, c0, width, dtype):
    """An isa_tensor with ld > c whose data pointer sits c0 channels into rows of `width` channels: row stride `width`,
    neighbours full of NaN and +inf."""
    L, lib = _lib()
    n, Lp = 2, 4100
    dev, x = make_logits(K, n, Lp, width - c0, dtype, 11, NAN)
    wide = torch.full((n, Lp, width), INF, dtype=dtype, device="cuda")
    wide[..., c0:] = dev
    labels, _ = make_labels("uniform", n, Lp, K, 12)
    desc = L.IsaTensor(wide.data_ptr() + c0 * wide.element_size(), n, 4, Lp // 4, K, width, L.dtype_code(dtype), 1)
    conf, oob, cmap = run_confusion(L, lib, desc, torch.from_numpy(labels).cuda(), n, Lp, K)
    want_map = S.class_map(x, K)
    want_conf, want_oob = S.confusion(labels, want_map, K)
    assert np.array_equal(cmap, want_map) and np.array_equal(conf, want_conf) and np.array_equal(oob, want_oob)


# ---- 2. isa_sem_scores ----------------------------------------------------------------------------------------------
def device_scores(L, lib, conf):
    n, K = conf.shape[0], conf.shape[1]
    out = Padded(n * (4 + 2 * K), torch.float64, -3.0)
    dev = torch.from_numpy(np.ascontiguousarray(conf)).cuda()
    L.check(lib.isa_sem_scores(L.ptr(dev), n, K, L.ptr(out.view), L.stream_ptr()), "isa_sem_scores")
    torch.cuda.synchronize()
    assert out.pads_unchanged()
    return out.view.cpu().numpy().reshape(n, 4 + 2 * K)


def check_scores(got, want, K, what):
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN positions", got, want)
    exact = [0, 3] + list(range(4, 4 + 2 * K))
    ok = ~np.isnan(want[:, exact])
    assert np.array_equal(got[:, exact][ok], want[:, exact][ok]), (what, got, want)
    ok = ~np.isnan(want[:, 1:3])
    diff = np.abs(got[:, 1:3][ok] - want[:, 1:3][ok])
    print("SEMSCORE %s: max |diff| of the means %.3e over %d numbers" % (what, diff.max() if diff.size else 0.0, diff.size))
    assert (diff <= TOL).all(), (what, got, want)


@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("K", [2, 5, 32])
def test_sem_scores(K, n):
    L, lib = _lib()
    rs = np.random.RandomState(K * 10 + n)
    conf = rs.randint(0, 1 << 40, (n, K, K), dtype=np.int64)          # counts up to 2^40: int64 matters
    conf[0] >>= rs.randint(0, 40, (K, K))                             # ... and every magnitude below
    check_scores(device_scores(L, lib, conf), S.scores(conf), K, "random K=%d n=%d" % (K, n))
    special = np.zeros((4, K, K), np.int64)
    special[1] = np.diag(rs.randint(1, 1 << 40, K, dtype=np.int64))                      # diagonal: everything 1.0
    special[2] = rs.randint(0, 1000, (K, K))
    special[2, K - 1, :] = 0
    special[2, :, K - 1] = 0                                          # class K-1 absent from both maps
    special[3, 0, 0] = 12345                                          # only the background
    want = S.scores(special)
    assert np.isnan(want[0]).sum() == 3 + 2 * K and want[0, 3] == 0   # all-zero matrix
    assert (want[1, [0, 1, 2]] == 1.0).all() and np.isnan(want[2, 4 + K - 1]) and want[3, 3] == 1
    check_scores(device_scores(L, lib, special), want, K, "special K=%d" % K)


# ---- 3. through the network -----------------------------------------------------------------------------------------
def k_class_sd(K, use_instance_seg=False):
    sd = R.synth_state_dict(23, use_instance_seg)
    if K != 2:
        rs = np.random.RandomState(77)
        sd["sem_seg_output.weight"] = torch.from_numpy((rs.standard_normal((K, 32, 1, 1)) * 0.25).astype(np.float32))
        sd["sem_seg_output.bias"] = torch.from_numpy(rs.uniform(-0.1, 0.1, K).astype(np.float32))
    return sd


def sem_targets(ins, K, compact):
    from isa_amd.data import class_onehot
    onehot = class_onehot(ins, K)
    return onehot.argmax(1).to(torch.uint8) if compact else onehot


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [2, 5])
def test_network_class_map_and_score_semantic(K, dtype, compact):
    _gpu()
    from isa_amd.reseg import ReSeg
    B, size = 2, 64
    x, _, ins, _ = R.synth_batch(B, size, size, seed=7)
    m = ReSeg(K, use_instance_seg=False, dtype=dtype)
    m.load_state_dict(k_class_sd(K))
    m.eval()
    target = sem_targets(ins, K, compact)
    lab = sem_targets(ins, K, True).numpy()
    with torch.no_grad():
        _, sem_argmax = m(False, x)
    cmap = m.class_map()
    assert cmap.is_cuda and cmap.dtype == torch.uint8 and tuple(cmap.shape) == (B, size, size)
    cm = cmap.cpu().numpy()
    assert np.array_equal(cm, sem_argmax.cpu().numpy()[:, 0].astype(np.uint8)), "class_map() is forward's sem_argmax"
    assert len(np.unique(cm)) >= 2, "the case must predict more than one class"
    scores, conf = m.score_semantic(target)
    assert scores.is_cuda and scores.dtype == torch.float64 and tuple(scores.shape) == (B, 4 + 2 * K)
    assert conf.is_cuda and conf.dtype == torch.int64 and tuple(conf.shape) == (B, K, K)
    want_conf, want_oob = S.confusion(lab, cm, K)
    assert not want_oob.any() and int(m.last_sem_oob.sum()) == 0
    assert np.array_equal(conf.cpu().numpy(), want_conf)
    check_scores(scores.cpu().numpy(), S.scores(want_conf), K, "score_semantic K=%d %s compact=%s" % (K, dtype, compact))
    # a dataset total through semantic_scores, both shapes
    total = conf.sum(0)
    check_scores(m.semantic_scores(total).cpu().numpy()[None], S.scores(want_conf.sum(0))[None], K, "semantic_scores [K,K]")
    check_scores(m.semantic_scores(conf).cpu().numpy(), S.scores(want_conf), K, "semantic_scores [n,K,K]")
    # a label >= K: an error that names K with check=True, a count with check=False
    bad = sem_targets(ins, K, True).clone()
    bad[1, 0, :3] = K
    bad[1, 5, 5] = 200
    with pytest.raises(ValueError, match="K = %d" % K):
        m.score_semantic(bad)
    _, conf_bad = m.score_semantic(bad, check=False)
    assert m.last_sem_oob.cpu().tolist() == [0, 4]
    want_bad, _ = S.confusion(bad.numpy(), cm, K)
    assert np.array_equal(conf_bad.cpu().numpy(), want_bad)


@pytest.mark.parametrize("dtype", DTYPES)
def test_instance_model_semantic_dice_is_the_foreground_dice(dtype):
    _gpu()
    from isa_amd.reseg import ReSeg
    B, size, cap = 3, 64, 4
    x, sem, ins, n = R.synth_batch(B, size, size, seed=7)
    m = ReSeg(2, True, dtype=dtype)
    m.load_state_dict(R.synth_state_dict())
    m.eval()
    m.head.drop_rate = 0.0
    _, sem_arg, labels, count = m.segment(x, max_objects=cap)
    scores, conf = m.score_semantic(sem)
    cm = m.class_map().cpu().numpy()
    assert np.array_equal(cm, sem_arg.cpu().numpy()[:, 0].astype(np.uint8))
    inst = m.score_instances(labels, count, ins, n, sem_arg, sem, max_objects=cap)
    got, want = scores[:, 4 + 2 + 1].cpu().numpy(), inst[:, 6].cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and not np.isnan(want).all()
    ok = ~np.isnan(want)
    assert (np.abs(got[ok] - want[ok]) <= TOL).all(), (got, want)
    assert np.array_equal(conf.cpu().numpy(), S.confusion(sem[:, 1].numpy().astype(np.uint8), cm, 2)[0])


# ---- 4. Model.evaluate_semantic and predict_classes -----------------------------------------------------------------
def k_class_model(K, instance=False):
    _gpu()
    from isa_amd.model import Model
    model = Model("CVPPP", "ReSeg", K, 4, use_instance_segmentation=instance)
    model.model.load_state_dict(k_class_sd(K, instance))
    return model


def test_model_evaluate_semantic():
    from isa_amd.data import SyntheticLoader
    K = 5
    model = k_class_model(K)
    batches = list(SyntheticLoader(2, 2, 64, 64, seed=5, n_classes=K)) + \
        list(SyntheticLoader(1, 2, 64, 64, seed=9, compact=True, n_classes=K))
    assert batches[0][1].dtype == torch.int64 and batches[2][1].dtype == torch.uint8
    res = model.evaluate_semantic(batches)
    assert sorted(res) == sorted(["mIoU", "Pixel Acc", "mDice", "IoU", "Dice", "confusion", "n_images", "per_image"])
    confs = []
    for x, sem, _, _ in batches:
        with torch.no_grad():
            model.model(False, x)
        cm = model.model.class_map().cpu().numpy()
        lab = sem.numpy() if sem.dtype == torch.uint8 else sem.argmax(1).numpy().astype(np.uint8)
        confs.append(S.confusion(lab, cm, K)[0])
    per = np.concatenate(confs)
    total = per.sum(0)
    assert res["confusion"].dtype == np.int64 and np.array_equal(res["confusion"], total)
    assert res["n_images"] == 6 and res["per_image"].shape == (6, 4 + 2 * K) and res["per_image"].dtype == np.float64
    check_scores(res["per_image"], S.scores(per), K, "evaluate_semantic per image")
    want = S.scores(total)
    head = np.concatenate([[res["Pixel Acc"], res["mIoU"], res["mDice"], want[3]], res["IoU"], res["Dice"]])
    check_scores(head[None], want[None], K, "evaluate_semantic headline")
    assert 0.0 <= res["mIoU"] <= 1.0 and 0.0 < res["Pixel Acc"] <= 1.0
    empty = model.evaluate_semantic([])
    assert empty["n_images"] == 0 and empty["per_image"].shape == (0, 4 + 2 * K) and not empty["confusion"].any()
    assert all(np.isnan(empty[k]) for k in ("mIoU", "Pixel Acc", "mDice")) and np.isnan(empty["IoU"]).all()
    with pytest.raises(RuntimeError):
        model.evaluate(batches)


def test_model_evaluate_semantic_instance_model():
    """The K = 2 semantic head of an instance model: the same figures as the class map and the foreground give."""
    from isa_amd.data import SyntheticLoader
    model = k_class_model(2, instance=True)
    batches = list(SyntheticLoader(1, 2, 64, 64, seed=5)) + list(SyntheticLoader(1, 2, 64, 64, seed=9, compact=True))
    res = model.evaluate_semantic(batches)
    confs = []
    for x, sem, _, _ in batches:
        model.model._semantic_logits(x.cuda())
        cm = model.model.class_map().cpu().numpy()
        lab = sem.numpy() if sem.dtype == torch.uint8 else sem.argmax(1).numpy().astype(np.uint8)
        confs.append(S.confusion(lab, cm, 2)[0])
    assert np.array_equal(res["confusion"], np.concatenate(confs).sum(0)) and res["n_images"] == 4


def test_predict_classes_is_the_argmax_of_predict():
    """Every pixel whose two largest probabilities differ must carry predict()'s arg-max; where they are equal and the
    logits tie exactly, the first class.  The other pixels (softmax rounding merged two different logits) are excluded:
    the share is printed and capped at 0.1 %.  On the float64 oracle, same weights and input, no pixel has two equal
    largest fp32 probabilities (checked on the CPU), so the share expected here is 0."""
    K = 5
    model = k_class_model(K)
    x, _, _, _ = R.synth_batch(2, 64, 64, seed=7)
    probs = model.predict(x)
    logits = model.model.net.to_nchw(model.model._last_sem).float().cpu().numpy()
    classes = model.predict_classes(x)
    assert not classes.is_cuda and classes.dtype == torch.uint8 and tuple(classes.shape) == (2, 64, 64)
    p = probs.numpy()
    top = np.sort(p, 1)
    differ = top[:, -1] > top[:, -2]
    got = classes.numpy()
    assert np.array_equal(got[differ], p.argmax(1)[differ])
    tie = (logits == logits.max(1, keepdims=True)).sum(1) > 1
    must_first = ~differ & tie
    assert np.array_equal(got[must_first], logits.argmax(1)[must_first])
    excluded = float((~differ & ~tie).mean())
    print("SEMSCORE predict_classes: %.4f %% of the pixels excluded (equal top probabilities, different logits)" % (100 * excluded))
    assert excluded <= 0.001


# ---- 5. fit() -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", [True, False])
def test_fit_validation_sem_scores_log(tmp_path, on):
    _gpu()
    from isa_amd.model import Model
    from isa_amd.data import SyntheticLoader
    K = 3
    m = Model("CVPPP", "ReSeg", K, 4, use_instance_segmentation=False)
    assert m.val_sem_scores is False
    m.val_sem_scores = on
    tr = SyntheticLoader(2, 2, 64, 64, seed=1, n_classes=K)
    te = SyntheticLoader(2, 2, 64, 64, seed=2, compact=on, n_classes=K)
    m.fit('Multi', 0.5, 1.5, 2, 1.0, 0.001, 10.0, 0.5, 25, False, 'Adadelta', True, 2, None, tr, te, str(tmp_path), False)
    vlog = open(os.path.join(str(tmp_path), "validation.log")).read().strip().splitlines()
    assert vlog[0] == "Epoch,Cost" and len(vlog) == 3
    assert not os.path.exists(os.path.join(str(tmp_path), "validation_scores.log"))
    path = os.path.join(str(tmp_path), "validation_sem_scores.log")
    if not on:
        assert not os.path.exists(path)
        return
    slog = open(path).read().strip().splitlines()
    assert slog[0] == "Epoch,mIoU,PixelAcc,mDice" and len(slog) == 3
    for epoch, ln in enumerate(slog[1:]):
        cells = ln.split(",")
        assert len(cells) == 4 and int(cells[0]) == epoch
        vals = [float(c) for c in cells[1:]]
        assert all(v != v or 0.0 <= v <= 1.0 for v in vals), ln
    assert any(float(c) == float(c) for c in slog[1].split(",")[1:]), "a validation set with pixels has a pixel accuracy"


# ---- 6. pred_list.py --n-classes ------------------------------------------------------------------------------------
def test_pred_list_writes_class_maps(tmp_path):
    from PIL import Image
    _gpu()
    script = os.path.join(ROOT, "pred_list.py")
    out = tmp_path / "k5"
    r = subprocess.run([sys.executable, script, "--synthetic", "3", "--n-classes", "5", "--output", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for i in range(3):
        name = "synthetic_%04d" % i
        d = out / name
        src = np.asarray(Image.open(d / (name + ".png")))
        sem = np.asarray(Image.open(d / (name + "-sem_mask.png")))
        color = np.asarray(Image.open(d / (name + "-sem_mask_color.png")))
        fg = np.asarray(Image.open(d / (name + "-fg_mask.png")))
        assert src.shape == (300 + 7 * (i % 5), 330, 3)
        assert sem.dtype == np.uint8 and sem.shape == src.shape[:2] and int(sem.max()) < 5
        assert color.shape == src.shape and fg.shape == sem.shape
        assert np.array_equal(fg, ((sem != 0) * 255).astype(np.uint8))
        assert not os.path.exists(d / (name + "-ins_mask.png"))
    r = subprocess.run([sys.executable, script, "--synthetic", "1", "--n-classes", "5", "--instances", "--output",
                        str(tmp_path / "bad")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "--instances" in r.stderr
    plain = tmp_path / "plain"
    r = subprocess.run([sys.executable, script, "--synthetic", "2", "--output", str(plain)], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    written = sorted(f for _, _, fs in os.walk(str(plain)) for f in fs)
    assert written == sorted("synthetic_%04d%s" % (i, s) for i in range(2) for s in (".png", "-fg_mask.png"))
