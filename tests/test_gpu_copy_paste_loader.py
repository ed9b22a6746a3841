"""RecordLoader(copy_paste=True): the stage is what tests/copy_paste_np.py makes of the same loader's batch without it.
Two loaders with one seed, the flag off and on, with d4, rotation and centre cut on: the on-batch equals the restatement
applied to the off-batch with the recorded draws, counts and plan included; an image whose recorded source is -1 is
byte-equal to the off-batch's; the recorded draws agree on every key the two share; a second on-loader with the same seed
yields the same bytes.  With elastic=True as well the stage runs BEFORE the deformation and leaves the noise generator
alone.  With copy_paste_p = 1 and no shift, an image pasted onto itself unflipped keeps its image and semantic map."""
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
import copy_paste_np as CP   # noqa: E402
import elastic_np as E       # noqa: E402

KW = dict(mode='training', copy_paste_p=0.5, copy_paste_min_area=4, copy_paste_shift=0.25)


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import isa_amd  # noqa: F401
    from isa_amd import records
    return records


def _records(tmp_path):
    """Three non-square images with 3 to 5 instances, as tests/test_gpu_elastic_loader.py builds them."""
    rng = np.random.default_rng(17)
    imgs, sems, inss = [], [], []
    for i, (h, w) in enumerate([(90, 120), (118, 92), (96, 124)]):
        kk = 3 + i
        ins = np.zeros((h, w, kk), np.uint8)
        for j in range(kk):
            y0, x0 = rng.integers(0, h - 30), rng.integers(0, w - 30)
            ins[y0:y0 + rng.integers(8, 30), x0:x0 + rng.integers(8, 30), j] = 1
        imgs.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)); sems.append((ins.sum(2) > 0).astype(np.uint8)); inss.append(ins)
    root = str(tmp_path / "training-lmdb")
    need_gpu().create_dataset(root, imgs, sems, inss)
    return root


def _host(batch):
    rgb, sem, ins, n = batch
    assert n.dtype == torch.int32 and not n.is_cuda and rgb.dtype == sem.dtype == ins.dtype == torch.uint8
    return rgb.cpu().numpy(), sem.cpu().numpy(), ins.cpu().numpy(), [int(v) for v in n]


def _restate(off, draws, min_area):
    cp = [d["copy_paste"] for d in draws]
    return CP.copy_paste(off[0], off[1], off[2], off[3], [(d["src"], d["flip"], d["dy"], d["dx"]) for d in cp],
                         [d["select"] for d in cp], min_area)


def _check_draws(loader, batch_size, h, w, rng):
    """The recorded draws are the documented ones, in the documented order, from a generator `rng` seeded as the loader's."""
    ry, rx = int(loader.copy_paste_shift * h), int(loader.copy_paste_shift * w)
    for d in loader.last_draws:
        u, s, bits, fl = rng.random(), rng.randrange(batch_size), rng.getrandbits(32), rng.getrandbits(2)
        dy, dx = rng.randint(-ry, ry), rng.randint(-rx, rx)
        assert d["copy_paste"] == dict(src=s if u < loader.copy_paste_p else -1, select=bits, flip=fl, dy=dy, dx=dx)


def test_on_batch_is_the_restatement_of_the_off_batch(tmp_path):
    R = need_gpu()
    root = _records(tmp_path)
    off = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, seed=7, **KW)
    on = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, seed=7, copy_paste=True, **KW)
    twin = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, seed=7, copy_paste=True, **KW)
    sources, pasted = [], 0
    for epoch in range(1, 4):
        rng = random.Random(3000017 * 7 + epoch + 611953)
        for b0, b1, b2 in zip(off, on, twin):
            assert off.last_paste_plan is None and "copy_paste" not in off.last_draws[0]
            for d0, d1 in zip(off.last_draws, on.last_draws):
                assert set(d1) == set(d0) | {"copy_paste"} and all(d0[k] == d1[k] for k in d0)
            _check_draws(on, 3, 32, 32, rng)
            assert all(torch.equal(u, v) for u, v in zip(b1, b2)) and torch.equal(on.last_paste_plan, twin.last_paste_plan)
            assert b1[2].shape == (3, 32, 32, 32) and on.last_paste_plan.is_cuda and on.last_paste_plan.dtype == torch.int32
            h0, h1 = _host(b0), _host(b1)
            want = _restate(h0, on.last_draws, 4)
            assert np.array_equal(h1[0], want[0]) and np.array_equal(h1[1], want[1]) and np.array_equal(h1[2], want[2])
            assert h1[3] == want[3].tolist()
            assert np.array_equal(on.last_paste_plan.cpu().numpy().view(np.uint32).astype(np.int64), want[4])
            for j, d in enumerate(on.last_draws):
                sources.append(d["copy_paste"]["src"])
                pasted += bool(want[4][j][0])
                if d["copy_paste"]["src"] == -1:
                    assert all(np.array_equal(x[j], y[j]) for x, y in zip(h0[:3], h1[:3])) and h0[3][j] == h1[3][j]
    assert len(sources) == 9 and -1 in sources and any(s >= 0 for s in sources) and pasted >= 1


def test_flag_is_ignored_in_test_mode(tmp_path):
    R = need_gpu()
    root = _records(tmp_path)
    t0 = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, mode='test')
    t1 = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, mode='test', copy_paste=True, copy_paste_p=1.0)
    for x, y in zip(t0, t1):
        assert all(torch.equal(u, v) for u, v in zip(x, y))
    assert t1.last_paste_plan is None and "copy_paste" not in t1.last_draws[0]


def test_stage_runs_before_the_deformation_and_leaves_its_noise_alone(tmp_path):
    R = need_gpu()
    root = _records(tmp_path)
    el = dict(elastic_alpha=(20.0, 60.0), elastic_sigma=2.0, elastic_p=1.0)
    kw = dict(KW, copy_paste_p=1.0)
    plain = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, seed=5, **kw)
    bent = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, seed=5, elastic=True, **el, **kw)
    on = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, seed=5, elastic=True, copy_paste=True, **el, **kw)
    pasted = 0
    for epoch in range(2):
        for b0, b1, b2 in zip(plain, bent, on):
            assert torch.equal(on.last_field, bent.last_field)                # the same noise and the same alphas
            for d1, d2 in zip(bent.last_draws, on.last_draws):
                assert set(d2) == set(d1) | {"copy_paste"} and all(d1[k] == d2[k] for k in d1)
            h0, h2 = _host(b0), _host(b2)
            field = on.last_field.cpu().numpy()
            mid = _restate(h0, on.last_draws, 4)
            pasted += int((mid[4][:, 0] != 0).sum())
            want = E.elastic(mid[0], mid[1], mid[2], mid[3].tolist(), field)
            assert np.array_equal(h2[0], want[0]) and np.array_equal(h2[1], want[1]) and np.array_equal(h2[2], want[2])
            assert h2[3] == [int(v) for v in want[3]]
            assert np.array_equal(on.last_paste_plan.cpu().numpy().view(np.uint32).astype(np.int64), mid[4])
    assert pasted >= 1


def test_an_image_pasted_onto_itself_keeps_image_and_semantic_map(tmp_path):
    R = need_gpu()
    root = _records(tmp_path)
    kw = dict(KW, copy_paste_p=1.0, copy_paste_shift=0.0)
    off = R.RecordLoader(R.RecordDataset(root), 1, 32, 32, seed=11, **kw)
    on = R.RecordLoader(R.RecordDataset(root), 1, 32, 32, seed=11, copy_paste=True, **kw)
    unflipped = 0
    for epoch in range(3):
        for b0, b1 in zip(off, on):
            d = on.last_draws[0]["copy_paste"]
            assert d["src"] == 0 and d["dy"] == 0 and d["dx"] == 0             # a batch of one: the image itself, unmoved
            h0, h1 = _host(b0), _host(b1)
            want = _restate(h0, on.last_draws, 4)
            assert all(np.array_equal(x, y) for x, y in zip(h1[:3], want[:3])) and h1[3] == want[3].tolist()
            if d["flip"] == 0:
                unflipped += 1
                assert np.array_equal(h0[0], h1[0]) and np.array_equal(h0[1], h1[1])
                assert np.array_equal(h0[2].any(3), h1[2].any(3))             # the same pixels are covered by an instance
    assert unflipped >= 1
