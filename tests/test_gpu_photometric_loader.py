"""RecordLoader with AlignCollate's five photometric augmentations on: every training sample equals the reference's own
sequence of PIL calls (dataset.py:175-330) replayed on the host with the loader's recorded draws - resize(LANCZOS)
twice, ImageEnhance in the drawn order, the HSV hue shift, point, channel indexing, convert('L'), resize(BILINEAR) -
alone (case a) and behind the geometric augmentations (case b); the targets are what the same draws give without them."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))]
import photometric_np as P   # noqa: E402
import rotate_ref as RR      # noqa: E402

FIVE = dict(color_jitter=True, gamma=True, channel_swap=True, grayscale=True, resolution=True)


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import isa_amd  # noqa: F401
    from isa_amd import records
    return records


def _records(tmp_path):
    rng = np.random.default_rng(17)
    imgs, sems, inss = [], [], []
    for i, (h, w) in enumerate([(90, 120), (118, 92), (96, 124)]):       # non-square originals
        kk = 3 + i
        ins = np.zeros((h, w, kk), np.uint8)
        for j in range(kk):
            y0, x0 = rng.integers(0, h - 30), rng.integers(0, w - 30)
            ins[y0:y0 + rng.integers(8, 30), x0:x0 + rng.integers(8, 30), j] = 1
        imgs.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)); sems.append((ins.sum(2) > 0).astype(np.uint8)); inss.append(ins)
    root = str(tmp_path / "training-lmdb")
    need_gpu().create_dataset(root, imgs, sems, inss)
    return root, imgs, sems, inss


def _host_sample(img, sem, ins, draws, out_h, out_w, k):
    """AlignCollate.__preprocess with PIL / numpy on the host for the draws the loader made: the geometric replay of
    tests/test_gpu_rotate_cut.py with the five photometric stages at the reference's positions."""
    image = Image.fromarray(img)
    if "ratio" in draws:                                                   # dataset.py:182-183
        image = P.pil_resolution(image, draws["ratio"])
    planes = [ins[:, :, i] for i in range(ins.shape[2])]
    op = draws["op"]

    def pil_d4(a, resample):
        im = a if isinstance(a, Image.Image) else Image.fromarray(a)
        if op & 1:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        if op & 2:
            im = im.transpose(Image.FLIP_TOP_BOTTOM)
        if op & 4:
            im = im.transpose(Image.TRANSPOSE)
        return im.rotate(90 * ((op >> 3) & 3), resample=resample, expand=True)

    image = pil_d4(image, Image.BILINEAR)
    planes = [np.array(pil_d4(p, Image.NEAREST)) for p in planes]
    sem = np.array(pil_d4(sem, Image.NEAREST))
    angle = draws["angle"]
    if draws["bg_key"] is not None:
        bg = RR.background(np.array(image), draws["bg_key"])
        rgba = image.convert('RGBA').rotate(angle, resample=Image.BILINEAR, expand=True)
        back = Image.new('RGBA', rgba.size, (bg[0], bg[1], bg[2], 255))
        image = Image.composite(rgba, back, rgba).convert('RGB')
        planes = [np.array(Image.fromarray(p).rotate(angle, resample=Image.NEAREST, expand=True)) for p in planes]
        sem = np.array(Image.fromarray(sem).rotate(angle, resample=Image.NEAREST, expand=True))
    if draws["pick"] is not None:
        stack = np.stack(planes, 2)
        img_c, sem, stack, keep = RR.center_cut(np.array(image), sem, stack, draws["pick"], out_h, out_w)
        image = Image.fromarray(img_c)
        planes = [stack[:, :, i] for i in range(stack.shape[2])]
    image = P.pil_replay_draws(image, draws)                               # dataset.py:271-281
    rgb = np.asarray(image.resize((out_w, out_h), Image.BILINEAR))
    semr = np.asarray(Image.fromarray(sem).resize((out_w, out_h), Image.NEAREST))
    out = np.zeros((out_h, out_w, k), np.uint8)
    for i, p in enumerate(planes):
        out[:, :, i] = np.asarray(Image.fromarray(np.ascontiguousarray(p)).resize((out_w, out_h), Image.NEAREST))
    return rgb, semr, out, len(planes)


def _check_epochs(loader, imgs, sems, inss, epochs):
    seen = []
    for epoch in range(epochs):
        order = None
        for bi, (rgb, sem, ins, n) in enumerate(loader):
            order = loader.indices() if order is None else order
            for j, draws in enumerate(loader.last_draws):
                i = order[3 * bi + j]
                want_rgb, want_sem, want_ins, want_n = _host_sample(imgs[i], sems[i], inss[i], draws, 32, 32, 32)
                assert np.array_equal(rgb[j].cpu().numpy(), want_rgb), (epoch, bi, j, draws)
                assert np.array_equal(sem[j].cpu().numpy(), want_sem), (epoch, bi, j, draws)
                assert np.array_equal(ins[j].cpu().numpy(), want_ins), (epoch, bi, j, draws)
                assert int(n[j]) == want_n
                # the targets know nothing of the five: the same geometric draws alone give the same annotations
                plain = {key: draws[key] for key in ("op", "angle", "bg_key", "pick")}
                _, plain_sem, plain_ins, plain_n = _host_sample(imgs[i], sems[i], inss[i], plain, 32, 32, 32)
                assert np.array_equal(plain_sem, want_sem) and np.array_equal(plain_ins, want_ins) and plain_n == want_n
                seen.append(draws)
    return seen


def test_photometric_alone_equals_the_pil_sequence(tmp_path):
    """Case (a): no geometric augmentation, all five on."""
    R = need_gpu()
    root, imgs, sems, inss = _records(tmp_path)
    loader = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, mode='training', seed=4, d4=False, rotation=False,
                            center_cut=False, **FIVE)
    seen = _check_epochs(loader, imgs, sems, inss, 3)
    assert len(seen) == 9
    assert all(len(d["jitter"]) == 4 and 0.7 <= d["gamma"] <= 1.3 and 0.7 <= d["ratio"] < 1.31 for d in seen)
    assert len({tuple(name for name, _ in d["jitter"]) for d in seen}) > 3          # shuffled orders
    swaps = [d["channels"] for d in seen]
    assert None in swaps and any(c is not None and len(set(c)) < 3 for c in swaps)  # no swap, and one drawn with replacement
    assert {d["gray"] for d in seen} == {False, True}
    # the targets are those of a loader without the five (no geometric draw either: the permutation is all they share)
    plain = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, mode='training', seed=4, d4=False, rotation=False, center_cut=False)
    both = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, mode='training', seed=4, d4=False, rotation=False,
                          center_cut=False, **FIVE)
    for (rgb0, sem0, ins0, n0), (rgb1, sem1, ins1, n1) in zip(plain, both):
        assert torch.equal(sem0, sem1) and torch.equal(ins0, ins1) and torch.equal(n0, n1)
        assert not torch.equal(rgb0, rgb1)


def test_photometric_behind_the_geometric_augmentations(tmp_path):
    """Case (b): everything on."""
    R = need_gpu()
    root, imgs, sems, inss = _records(tmp_path)
    loader = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, mode='training', seed=6, **FIVE)
    seen = _check_epochs(loader, imgs, sems, inss, 2)
    assert len(seen) == 6 and all(d["pick"] is not None and "jitter" in d and "channels" in d and "gray" in d for d in seen)


def test_flags_off_make_no_draw(tmp_path):
    """With the five off the loader's batches and recorded draws are those of a loader that was never given the flags;
    in test mode the flags are ignored."""
    R = need_gpu()
    root, imgs, sems, inss = _records(tmp_path)
    off = dict.fromkeys(FIVE, False)
    a = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, mode='training', seed=9)
    b = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, mode='training', seed=9, **off)
    for x, y in zip(a, b):
        assert all(torch.equal(u, v) for u, v in zip(x, y)) and a.last_draws == b.last_draws
        assert all(set(d) == {"op", "angle", "bg_key", "pick"} for d in b.last_draws)
    t0 = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, mode='test')
    t1 = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, mode='test', **FIVE)
    for x, y in zip(t0, t1):
        assert all(torch.equal(u, v) for u, v in zip(x, y))
