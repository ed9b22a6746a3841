"""GPU: Model.predict_instances(fill=True) and Model.evaluate(fill=True) - the unlabelled foreground of the predicted class
map goes to the nearest instance after the clean-up (ReSeg.fill_instances), exactly as tests/distance_np.py fills it.

Every comparison is made inside ONE call (segment and fill_instances are wrapped to keep what they were given and what they
returned), not between two calls: the eval-mode logits of this model differ in the last bit from run to run
(tests/test_gpu_components.py measured it), so a fill=False call and a fill=True call do not see the same label map."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import distance_np as dn        # noqa: E402
import reseg_ref as R           # noqa: E402
from test_gpu_ops import _gpu   # noqa: E402


def _model():
    _gpu()
    from isa_amd.model import Model
    torch.manual_seed(0)
    model = Model("CVPPP", "ReSeg", 2, 5, use_instance_segmentation=True)
    net = model.model
    seen, fills = [], []
    real_segment, real_fill = net.segment, net.fill_instances

    def segment(*a, **k):
        seen.append(real_segment(*a, **k))
        return seen[-1]

    def fill(labels, fg, max_dist=None):
        out = real_fill(labels, fg, max_dist)
        fills.append((labels.clone(), fg.clone(), max_dist, out[0].clone(), out[1].clone()))
        return out

    net.segment, net.fill_instances = segment, fill
    return model, net, seen, fills


@pytest.mark.parametrize("clean", [{}, dict(keep='largest')], ids=["raw", "cleaned"])
@pytest.mark.parametrize("max_dist", [None, 2.0])
def test_predict_instances_fill_is_the_restatement_of_that_call(clean, max_dist):
    model, net, seen, fills = _model()
    x, _, _, _ = R.synth_batch(2, 64, 64, seed=2)
    _, plain, _ = model.predict_instances(x, **clean)
    assert not fills, "with the defaults none of the fill runs"
    prob, labels, count = model.predict_instances(x, fill=True, fill_max_dist=max_dist, **clean)
    assert len(fills) == 1 and len(seen) == 2
    before, fg, md, after, filled = (t.cpu().numpy() if torch.is_tensor(t) else t for t in fills[0])
    assert md == max_dist
    classes = net.class_map().cpu().numpy()                 # of that call's logits, still in its arena
    assert np.array_equal(fg, classes)                      # the fill ran against the predicted class map
    if not clean:
        assert np.array_equal(before, seen[-1][2].cpu().numpy())                  # and on what segment() produced
    d1, _, near = dn.edt2(before)
    want, want_filled = dn.fill(before, classes, near, d1, dn.max_dist_sq(max_dist))
    assert np.array_equal(labels.numpy(), want) and np.array_equal(after, want)
    assert np.array_equal(filled, want_filled)
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (2, 64, 64) and tuple(prob.shape) == (2, 64, 64)
    print("fill %s max_dist %s: %s pixels filled, %s instances" % (sorted(clean), max_dist, filled.tolist(), count.tolist()))
    assert before.any(axis=(1, 2)).all() and filled.sum() > 0, "the seeded model leaves nothing to fill: the test is empty"
    assert np.array_equal(labels.numpy()[before != 0], before[before != 0])       # no label is changed
    assert not (labels.numpy()[classes == 0] != before[classes == 0]).any()       # nothing outside the foreground
    if max_dist is None:
        for b in range(2):
            if before[b].any():                             # at least one instance: no foreground pixel is left at 0
                assert not ((labels.numpy()[b] == 0) & (classes[b] != 0)).any()
    else:
        assert not ((labels.numpy() != before) & (d1 > 4)).any()


def test_evaluate_with_fill_runs_and_does_not_lower_the_foreground_dice():
    """Filling only ADDS labelled pixels, all of them inside the predicted foreground.  The targets here are one object that
    covers the whole image, so the ground-truth foreground contains the predicted one: with P labelled pixels (all inside
    the ground truth's N) the foreground Dice of the label maps is 2 P / (P + N), which rises with P.  So the filled map's
    is >= the unfilled one's, and greater where a pixel was filled - an inequality, not a measurement; both are scored from
    the label maps of the same call.  The 'FG Dice' evaluate() itself reports compares the predicted CLASS map with the
    semantic target (score_instances, column 6 with sem_argmax and sem_target given): the fill leaves that map alone, so
    that column is >= by being equal, which is asserted too."""
    model, net, seen, fills = _model()
    x, _, _, _ = R.synth_batch(2, 64, 64, seed=2)
    ins = torch.zeros((2, 32, 64, 64), dtype=torch.int64)
    ins[:, 0] = 1
    sem = torch.zeros((2, 2, 64, 64), dtype=torch.int64)
    sem[:, 1] = 1
    n = torch.tensor([[1], [1]], dtype=torch.int32)
    batch = [(x, sem, ins, n)]
    res = model.evaluate(batch, fill=True, keep='largest')
    assert len(fills) == 1 and res["n_images"] == 2
    before, fg, _, after, filled = fills[0]
    _, sem_arg, _, _ = seen[-1]
    cnt = torch.tensor([int(v.max()) for v in before.cpu()], dtype=torch.int32, device=before.device)
    rows_filled = net.score_instances(after, cnt, ins, n, sem_arg, sem, max_objects=5).cpu().numpy()
    rows_plain = net.score_instances(before, cnt, ins, n, sem_arg, sem, max_objects=5).cpu().numpy()
    assert np.array_equal(res["per_image"][:, 6], rows_filled[:, 6], equal_nan=True)
    print("FG Dice unfilled %s filled %s, filled pixels %s" % (rows_plain[:, 6], rows_filled[:, 6], filled.tolist()))
    assert int(filled.sum()) > 0 and not np.isnan(rows_plain[:, 6]).any()
    lab_filled = net.score_instances(after, cnt, ins, n, max_objects=5).cpu().numpy()      # column 6: the label maps' foregrounds
    lab_plain = net.score_instances(before, cnt, ins, n, max_objects=5).cpu().numpy()
    print("label-map FG Dice unfilled %s filled %s" % (lab_plain[:, 6], lab_filled[:, 6]))
    for b in range(2):
        assert rows_filled[b, 6] >= rows_plain[b, 6]
        assert lab_filled[b, 6] >= lab_plain[b, 6]
        assert int(filled[b]) == 0 or lab_filled[b, 6] > lab_plain[b, 6]
    plain = model.evaluate(batch)
    assert len(fills) == 1 and plain["n_images"] == 2        # the default runs none of it


def test_pred_list_fill_end_to_end(tmp_path):
    """pred_list.py --instances --keep largest --fill: the tool runs the fill on the device and writes the instance files."""
    _gpu()
    from PIL import Image
    out = str(tmp_path / "out")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "pred_list.py"), "--synthetic", "2", "--batch", "2", "--instances",
                        "--max-objects", "4", "--keep", "largest", "--fill", "--fill-max-dist", "6", "--output", out],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in sorted(os.listdir(out)):
        mask = np.asarray(Image.open(os.path.join(out, name, name + "-ins_mask.png")))
        fg = np.asarray(Image.open(os.path.join(out, name, name + "-fg_mask.png")))
        assert mask.shape == fg.shape and mask.max() <= 4
        assert os.path.isfile(os.path.join(out, name, name + "-n_objects.npy"))
