"""RecordLoader(elastic=True): the stage is what tests/elastic_np.py makes of the same loader's batch without it.
Two loaders with one seed, the flag off and on, with d4, rotation and centre cut on: the on-batch equals the restatement
applied to the off-batch with the on-loader's `last_field`, compaction and object counts included; an image whose recorded
alpha is 0 is byte-equal to the off-batch's; the recorded draws agree on every key the two share; a second on-loader with
the same seed yields the same bytes.  Then, with alpha pinned (elastic_alpha=(A, A), elastic_p=1), an A chosen on the host
from the restatement empties some but not all planes of an image (the drop and the compaction), and a huge A empties all
of them (the image passes through unwarped)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
import elastic_np as E   # noqa: E402

SIGMA = 2.0              # radius 8 on 32 x 32 batches


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import isa_amd  # noqa: F401
    from isa_amd import records
    return records


def _records(tmp_path, interior=False):
    """Three non-square images with 3 to 5 instances, as tests/test_gpu_photometric_loader.py builds them.  interior: one
    large instance and small ones, all well inside the image (nothing touches the border, whatever the rotation)."""
    rng = np.random.default_rng(17)
    imgs, sems, inss = [], [], []
    for i, (h, w) in enumerate([(90, 120), (118, 92), (96, 124)]):
        kk = 3 + i
        ins = np.zeros((h, w, kk), np.uint8)
        for j in range(kk):
            if interior:
                side = 30 if j == 0 else 7
                y0, x0 = rng.integers(h // 4, 3 * h // 4 - side), rng.integers(w // 4, 3 * w // 4 - side)
                ins[y0:y0 + side, x0:x0 + side, j] = 1
            else:
                y0, x0 = rng.integers(0, h - 30), rng.integers(0, w - 30)
                ins[y0:y0 + rng.integers(8, 30), x0:x0 + rng.integers(8, 30), j] = 1
        imgs.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)); sems.append((ins.sum(2) > 0).astype(np.uint8)); inss.append(ins)
    root = str(tmp_path / "training-lmdb")
    need_gpu().create_dataset(root, imgs, sems, inss)
    return root


def _host(batch):
    rgb, sem, ins, n = batch
    return rgb.cpu().numpy(), sem.cpu().numpy(), ins.cpu().numpy(), [int(v) for v in n]


def _check_against_restatement(off, on, field):
    """The on-batch is elastic_np.elastic of the off-batch by `field`; returns the restatement's counts."""
    rgb0, sem0, ins0, n0 = off
    rgb1, sem1, ins1, n1 = on
    want_rgb, want_sem, want_ins, want_n = E.elastic(rgb0, sem0, ins0, n0, field)
    assert np.array_equal(rgb1, want_rgb) and np.array_equal(sem1, want_sem)
    assert np.array_equal(ins1, want_ins) and n1 == want_n
    return want_n


def test_on_batch_is_the_restatement_of_the_off_batch(tmp_path):
    R = need_gpu()
    root = _records(tmp_path)
    kw = dict(mode='training', seed=7, elastic_alpha=(20.0, 60.0), elastic_sigma=SIGMA, elastic_p=0.5)
    off = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, **kw)
    on = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, elastic=True, **kw)
    twin = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, elastic=True, **kw)
    alphas = []
    for epoch in range(2):
        for b0, b1, b2 in zip(off, on, twin):
            assert off.last_field is None and "elastic_alpha" not in off.last_draws[0]
            for d0, d1 in zip(off.last_draws, on.last_draws):
                assert set(d1) == set(d0) | {"elastic_alpha"} and all(d0[k] == d1[k] for k in d0)
            assert all(torch.equal(u, v) for u, v in zip(b1, b2)) and torch.equal(on.last_field, twin.last_field)
            assert b1[0].dtype == torch.uint8 and b1[3].dtype == torch.int32 and b1[2].shape == (3, 32, 32, 32)
            field = on.last_field.cpu().numpy()
            assert field.shape == (3, 32, 32, 2) and field.dtype == np.float32
            h0, h1 = _host(b0), _host(b1)
            _check_against_restatement(h0, h1, field)
            for j, d in enumerate(on.last_draws):
                a = d["elastic_alpha"]
                assert a == 0.0 or 20.0 <= a <= 60.0
                alphas.append(a)
                if a == 0.0:
                    assert not field[j].any()
                    assert all(np.array_equal(x[j], y[j]) for x, y in zip(h0[:3], h1[:3])) and h0[3][j] == h1[3][j]
                else:
                    assert np.abs(field[j]).max() > 0.25 and not np.array_equal(h0[0][j], h1[0][j])
    assert len(alphas) == 6 and 0.0 in alphas and any(a > 0 for a in alphas)


def test_flag_is_ignored_in_test_mode(tmp_path):
    R = need_gpu()
    root = _records(tmp_path)
    t0 = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, mode='test')
    t1 = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, mode='test', elastic=True, elastic_p=1.0)
    for x, y in zip(t0, t1):
        assert all(torch.equal(u, v) for u, v in zip(x, y))
    assert t1.last_field is None


def test_emptied_planes_are_dropped_and_an_emptied_image_passes_through(tmp_path):
    R = need_gpu()
    root = _records(tmp_path, interior=True)
    kw = dict(mode='training', seed=3, center_cut=False, elastic_sigma=SIGMA, elastic_p=1.0)

    def first(**more):
        loader = R.RecordLoader(R.RecordDataset(root), 3, 32, 32, **kw, **more)
        batch = _host(next(iter(loader)))
        return batch, loader

    off, _ = first()
    assert off[3] == [int(off[2][b].reshape(-1, 32).any(0).sum()) for b in range(3)]       # every real plane has a pixel
    _, unit_loader = first(elastic=True, elastic_alpha=(1.0, 1.0))
    unit = unit_loader.last_field.cpu().numpy()              # the blurred noise itself: alpha A gives fp32(A) * unit
    # the smallest alpha of a geometric ladder at which some image loses a plane and keeps another, found on the host
    partial = None
    for A in 8.0 * 1.25 ** np.arange(48):
        counts = E.elastic(*off, np.float32(A) * unit)[3]
        if any(0 < k < k0 for k, k0 in zip(counts, off[3])):
            partial = float(np.float32(A))
            break
    assert partial is not None, "no alpha of the ladder empties some but not all planes of an image"
    on, loader = first(elastic=True, elastic_alpha=(partial, partial))
    assert [d["elastic_alpha"] for d in loader.last_draws] == [partial] * 3
    field = loader.last_field.cpu().numpy()
    assert np.array_equal(field, np.float32(partial) * unit)
    counts = _check_against_restatement(off, on, field)
    dropped = [b for b in range(3) if 0 < counts[b] < off[3][b]]
    assert dropped
    for b in dropped:                                        # the survivors sit at the front, zero planes behind them
        has = on[2][b].reshape(-1, 32).any(0)
        assert has[:counts[b]].all() and not has[counts[b]:].any()
    # an alpha that throws every sample onto the border: no plane of these interior instances is left
    huge, loader = first(elastic=True, elastic_alpha=(1e7, 1e7))
    field = loader.last_field.cpu().numpy()
    counts = _check_against_restatement(off, huge, field)
    warped = E.warp_nearest(off[2], field)
    through = [b for b in range(3) if not warped[b].any()]
    assert through, "the huge field left a plane in every image"
    for b in through:
        assert counts[b] == off[3][b] and all(np.array_equal(x[b], y[b]) for x, y in zip(off[:3], huge[:3]))
