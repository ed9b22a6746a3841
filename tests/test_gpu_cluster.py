"""GPU: clustering the instance embedding (isa_cluster_meanshift, isa_cluster_kmeans) through ReSeg.cluster_embedding,
ReSeg.segment_embedding, Model.predict_instances and pred_list.py, against the float64 restatement tests/cluster_np.py
(itself pinned to sklearn's KMeans by tests/test_cluster_ref.py).  Restatement and device get the same inputs: float32
values, rounded to bf16 first where the storage is bf16.

Whole runs on clear inputs.  Planted centres at pairwise distance 3, Gaussian noise around them.  The seeds in CASES are
chosen so that the restatement's min_margin - the smallest relative gap at any ball membership, assignment or farthest-point
pick of the run - is at least 1e-4, and every test asserts that of the restatement first.  Why 1e-4: the direct-form fp32
distance of at most 32 terms is good to about 4e-6 relative, and an fp32 centre that is off by 1e-6 |c| moves d by about
2 |dc| / bw, roughly 1e-5; 1e-4 leaves tenfold room above both.  Under that condition labels, n_objects, sizes and moved
must be bit-equal to the restatement, and the centres within the fp32 bound tests/test_gpu_disc.py uses for means:
max(8 x ref32_gap_loss, 1e-6) from tests/golden/disc.npz, largest error over largest value.

Single passes on hard inputs.  Overlapping clusters (noise 0.35, separation 1.2): one assignment against given centres and
one ball pass against a given centre.  A pixel whose own float64 relative gap is below 1e-4 is exempt, every other pixel must
match exactly, and at most 0.5 % of the foreground may be exempt - a condition on the input that the test asserts of the
restatement alone.

Shapes (a workgroup owns a chunk of ISA_DISC_CHUNKS(L) per image, a wave a tile of 64 pixels): 3x40x52 (three chunks and a
tail; one image without foreground, one with a single cluster), 2x64x64 (full chunks), 1x4x8 (less than a tile), 1x48x36 with
32 planted instances (the cap), C = 24 in rows of 32 with NaN in the padding, max_objects below the planted count, and
inputs whose refused balls plus objects exceed max_objects, so that the round budget max_rounds decides what is visited."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import cluster_np as CN     # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "disc.npz"))
TOL_C = max(8 * max(float(GOLD[k]) for k in GOLD.files if k.endswith("ref32_gap_loss")), 1e-6)
MARGIN = 1e-4
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}

# name: (B, H, W, C, ld or None, planted instances per image, outliers in image 0, {storage: seed})
CASES = {
    "3x40x52-c24": (3, 40, 52, 24, None, [5, 0, 1], 0, {"fp32": 24, "bf16": 20}),
    "2x64x64-c32": (2, 64, 64, 32, None, [7, 4], 0, {"fp32": 36, "bf16": 36}),
    "1x4x8-c5": (1, 4, 8, 5, None, [2], 0, {"fp32": 43, "bf16": 43}),
    "1x48x36-c32-k32": (1, 48, 36, 32, None, [32], 0, {"fp32": 48, "bf16": 9}),
    "2x40x52-c24-ld32": (2, 40, 52, 24, 32, [4, 3], 0, {"fp32": 11, "bf16": 11}),
    "1x40x52-c24-outliers": (1, 40, 52, 24, None, [4], 3, {"fp32": 59, "bf16": 59}),
    "1x40x52-c24-outlier-first": (1, 40, 52, 24, None, [4], 3, {"fp32": 51, "bf16": 45}),     # pixel 0 is one of the outliers
}
# run id: (case, method, keywords)
RUNS = {
    "A-ms": ("3x40x52-c24", "meanshift", {}),
    "A-ms-cap3": ("3x40x52-c24", "meanshift", dict(max_objects=3)),
    "A-ms-cap3-norest": ("3x40x52-c24", "meanshift", dict(max_objects=3, assign_rest=False)),
    "A-ms-refine2": ("3x40x52-c24", "meanshift", dict(refine=2)),
    "A-ms-shifts1": ("3x40x52-c24", "meanshift", dict(shifts=1)),
    "A-km": ("3x40x52-c24", "kmeans", dict(n_objects=[5, 3, 0])),
    "A-km-3of5": ("3x40x52-c24", "kmeans", dict(n_objects=[3, 0, 1], iters=6)),
    "B-ms": ("2x64x64-c32", "meanshift", {}),
    "B-ms-refine1": ("2x64x64-c32", "meanshift", dict(refine=1)),
    "B-km": ("2x64x64-c32", "kmeans", dict(n_objects=[7, 4], iters=3)),
    "C-ms": ("1x4x8-c5", "meanshift", {}),
    "C-km": ("1x4x8-c5", "kmeans", dict(n_objects=[2], iters=2)),
    "D-ms": ("1x48x36-c32-k32", "meanshift", {}),
    "D-km": ("1x48x36-c32-k32", "kmeans", dict(n_objects=[32], iters=2)),
    "D-km-over": ("1x48x36-c32-k32", "kmeans", dict(n_objects=[40], iters=1, max_objects=20)),
    "E-ms": ("2x40x52-c24-ld32", "meanshift", {}),
    "E-km": ("2x40x52-c24-ld32", "kmeans", dict(n_objects=[4, 3], iters=2)),
    "F-ms-noise": ("1x40x52-c24-outliers", "meanshift", dict(min_pixels=4)),
    "F-ms-noise-norest": ("1x40x52-c24-outliers", "meanshift", dict(min_pixels=4, assign_rest=False)),
    # the round budget: refused balls + objects exceed max_objects, so max_rounds decides what is visited
    "G-ms-budget4": ("1x40x52-c24-outlier-first", "meanshift", dict(min_pixels=4, max_objects=4)),
    "G-ms-budget4-norest": ("1x40x52-c24-outlier-first", "meanshift", dict(min_pixels=4, max_objects=4, assign_rest=False)),
    "G-ms-budget8": ("1x40x52-c24-outlier-first", "meanshift", dict(min_pixels=4, max_objects=4, max_rounds=8)),
    "G-ms-budget8-norest": ("1x40x52-c24-outlier-first", "meanshift",
                            dict(min_pixels=4, max_objects=4, max_rounds=8, assign_rest=False)),
    "G-ms-one-object": ("1x40x52-c24-outlier-first", "meanshift", dict(min_pixels=2, max_objects=1)),
    "G-ms-one-object-2rounds": ("1x40x52-c24-outlier-first", "meanshift", dict(min_pixels=2, max_objects=1, max_rounds=2)),
    "G-ms-one-object-2rounds-norest": ("1x40x52-c24-outlier-first", "meanshift",
                                       dict(min_pixels=2, max_objects=1, max_rounds=2, assign_rest=False)),
}


def storage(a, dt):
    """float32 array -> the float32 values the storage dtype holds."""
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    return t.to(DTYPES[dt]).float().numpy()


@functools.lru_cache(maxsize=None)
def inputs(case, dt, seed=None):
    """(emb float32 [B,C,H,W] as stored, fg uint8 [B,H,W], truth)."""
    B, H, W, C, _, n, outliers, seeds = CASES[case]
    emb, fg, truth = CN.planted(B, H, W, C, n, seeds[dt] if seed is None else seed, noise=0.1)
    if outliers:                                       # lone foreground pixels far from everything and from each other
        rs = np.random.RandomState(99)
        where = rs.permutation(H * W)[:outliers]
        if case.endswith("outlier-first"):
            where[0] = 0
        for i, p in enumerate(where):
            v = np.zeros(C, np.float32)
            v[i] = -10.0
            emb[0].reshape(C, -1)[:, p] = v
            fg[0].reshape(-1)[p] = 1
            truth[0].reshape(-1)[p] = 0
    return storage(emb, dt), fg, truth


@functools.lru_cache(maxsize=None)
def reference(run, dt, seed=None):
    case, method, kw = RUNS[run]
    emb, fg, _ = inputs(case, dt, seed)
    kw = dict(kw)
    if method == "meanshift":
        kw.setdefault("bandwidth", 1.5)
    elif "max_objects" in kw:
        kw["kmax"] = kw.pop("max_objects")
    return CN.cluster(emb, fg, method, **kw)


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import isa_amd  # noqa: F401
    from isa_amd.reseg import ReSeg
    return ReSeg


_MODEL = {}


def model(instance=False):
    """A small model: the operator needs an engine, not the weights."""
    ReSeg = need_gpu()
    if instance not in _MODEL:
        _MODEL[instance] = ReSeg(2, instance, dtype=torch.float32)
        _MODEL[instance].eval()
    return _MODEL[instance]


def device_emb(emb, dt, ld):
    """The NCHW tensor, or (ld given) an engine Act with ld > c whose pad channels hold NaN."""
    from isa_amd.engine import Act
    t = torch.tensor(emb, dtype=torch.float32, device="cuda").to(DTYPES[dt])
    if ld is None:
        return t
    B, C, H, W = t.shape
    buf = torch.full((B, H, W, ld), float("nan"), dtype=t.dtype, device="cuda")
    buf[..., :C] = t.permute(0, 2, 3, 1)
    return Act(buf, 0, C)


def device_args(run, dt):
    """(emb, fg, keywords) of a run with every tensor on the device."""
    case, _, kw = RUNS[run]
    e, fg, _ = inputs(case, dt)
    kw = dict(kw)
    if "n_objects" in kw:
        kw["n_objects"] = torch.tensor(kw["n_objects"], dtype=torch.int32, device="cuda")
    return device_emb(e, dt, CASES[case][4]), torch.tensor(fg, device="cuda"), kw


def run_device(m, run, dt, args=None):
    x, fg, kw = device_args(run, dt) if args is None else args
    return m.cluster_embedding(x, fg, method=RUNS[run][1], **kw)


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def centre_error(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("run", list(RUNS))
def test_whole_run_equals_the_restatement(run, dt):
    ref = reference(run, dt)
    print("%s %s: min_margin %.3e, n_objects %s, moved %s" % (run, dt, ref["min_margin"], ref["n_objects"].tolist(),
                                                              ref["moved"].tolist()))
    assert ref["min_margin"] >= MARGIN, "the input is not clear enough for an exact comparison: pick another seed"
    m = model()
    got = host(run_device(m, run, dt))
    err = centre_error(got["centres"], ref["centres"])
    print("  centres: largest error over largest value %.3e (bound %.3e)" % (err, TOL_C))
    assert got["labels"].dtype == np.uint8 and got["labels"].shape == ref["labels"].shape
    assert got["n_objects"].tolist() == ref["n_objects"].tolist()
    assert np.array_equal(got["labels"], ref["labels"])
    assert np.array_equal(got["sizes"], ref["sizes"])
    assert got["moved"].tolist() == ref["moved"].tolist()
    assert got["centres"].shape == ref["centres"].shape and err <= TOL_C


def test_the_cases_cover_the_edges():
    """What the table promises of its inputs, in the restatement alone."""
    a = reference("A-ms", "fp32")
    assert a["n_objects"].tolist() == [5, 0, 1] and not inputs("3x40x52-c24", "fp32")[1][1].any()
    assert reference("D-ms", "fp32")["n_objects"].tolist() == [32] and reference("D-km-over", "bf16")["n_objects"].tolist() == [20]
    cap, nocap = reference("A-ms-cap3", "fp32"), reference("A-ms-cap3-norest", "fp32")
    fg0 = inputs("3x40x52-c24", "fp32")[1][0] != 0
    assert cap["n_objects"][0] == nocap["n_objects"][0] == 3
    assert (cap["labels"][0][fg0] != 0).all() and (nocap["labels"][0][fg0] == 0).any()
    k = reference("A-km", "fp32")
    assert k["n_objects"].tolist() == [5, 0, 0] and not k["labels"][1:].any()
    assert reference("A-km-3of5", "fp32")["n_objects"].tolist() == [3, 0, 1]
    on, off = reference("F-ms-noise", "fp32"), reference("F-ms-noise-norest", "fp32")
    assert on["n_objects"].tolist() == off["n_objects"].tolist() == [4]
    fg = inputs("1x40x52-c24-outliers", "fp32")[1][0] != 0
    assert int((off["labels"][0][fg] == 0).sum()) == 3 and (on["labels"][0][fg] != 0).all()
    # the round budget: with pixel 0 a refused outlier, 4 rounds find 3 of the 4 clusters, 8 rounds all of them; one round and
    # max_objects = 1 find nothing (all-zero labels whatever assign_rest says), two rounds find one object
    fg = inputs("1x40x52-c24-outlier-first", "fp32")[1][0] != 0
    assert fg[0, 0]
    b4, b4n, b8, b8n = (reference("G-ms-budget" + t, "fp32") for t in ("4", "4-norest", "8", "8-norest"))
    assert b4["n_objects"].tolist() == b4n["n_objects"].tolist() == [3] and b8["n_objects"].tolist() == [4]
    assert (b4["labels"][0][fg] != 0).all() and int((b4n["labels"][0][fg] == 0).sum()) > 3
    assert (b8["labels"][0][fg] != 0).all() and int((b8n["labels"][0][fg] == 0).sum()) == 3
    one, two, twon = (reference("G-ms-one-object" + t, "fp32") for t in ("", "-2rounds", "-2rounds-norest"))
    assert one["n_objects"].tolist() == [0] and not one["labels"].any()
    assert two["n_objects"].tolist() == twon["n_objects"].tolist() == [1]
    assert (two["labels"][0][fg] == 1).all() and 0 < int((twon["labels"][0][fg] == 1).sum()) < int(fg.sum())


HARD_SEED = 13


@functools.lru_cache(maxsize=None)
def hard_input(dt):
    emb, fg, truth = CN.planted(1, 40, 52, 24, 6, HARD_SEED, noise=0.35, sep=1.2)
    emb = storage(emb, dt)
    x = emb[0].reshape(24, -1).T.astype(np.float64)
    t = truth[0].reshape(-1)
    cen = np.stack([x[t == i].mean(0) for i in range(1, 7)]).astype(np.float32)
    return emb, fg, x, cen


@pytest.mark.parametrize("dt", list(DTYPES))
def test_one_assignment_on_overlapping_clusters(dt):
    emb, fg, x, cen = hard_input(dt)
    f = fg[0].reshape(-1) != 0
    lab, gap = CN.assign(x[f], cen.astype(np.float64))
    exempt = gap < MARGIN
    print("assignment %s: %d of %d foreground pixels exempt, smallest gap %.3e" % (dt, int(exempt.sum()), int(f.sum()), gap.min()))
    assert exempt.sum() <= 0.005 * f.sum()
    assert len(set(lab.tolist())) == 6
    m = model()
    got = host(m.cluster_embedding(device_emb(emb, dt, None), torch.tensor(fg, device="cuda"), method="kmeans",
                                   n_objects=torch.tensor([6], dtype=torch.int32), iters=0,
                                   init=torch.tensor(cen)[None]))
    g = got["labels"].reshape(-1)
    assert not g[~f].any() and got["n_objects"].tolist() == [6] and got["moved"].tolist() == [0]
    assert np.array_equal(g[f][~exempt], (lab + 1)[~exempt].astype(np.uint8))
    assert int(got["sizes"].sum()) == int(f.sum())
    assert np.array_equal(got["centres"][0, :6], cen)          # iters = 0: the centres are the given ones, to the bit


@pytest.mark.parametrize("dt", list(DTYPES))
def test_one_ball_pass_on_overlapping_clusters(dt):
    emb, fg, x, cen = hard_input(dt)
    emb, fg = emb.copy(), fg.copy()
    fg[0, 0, 0] = 1                                            # the first pixel seeds the ball: give it a centre's value
    c = storage(cen[2], dt)
    emb[0, :, 0, 0] = c
    f = fg[0].reshape(-1) != 0
    xs = emb[0].reshape(24, -1).T.astype(np.float64)
    d = CN.sqdist(xs, c.astype(np.float64))
    bw = float(np.float32(np.sqrt(np.median(d[f]))))           # half of the foreground lies inside
    gap = CN.ball_gap(d, float(np.float32(bw) * np.float32(bw)))
    exempt = f & (gap < MARGIN)
    exempt[0] = False                                          # the seed belongs to the ball whatever its distance
    print("ball %s: %d of %d foreground pixels exempt, bandwidth %.4f" % (dt, int(exempt.sum()), int(f.sum()), bw))
    assert exempt.sum() <= 0.005 * f.sum()
    ref = CN.meanshift(xs, f, bw, shifts=0, max_objects=1, assign_rest=False)
    assert 0.4 * f.sum() < ref["sizes"][0] < 0.6 * f.sum()
    m = model()
    got = host(m.cluster_embedding(device_emb(emb, dt, None), torch.tensor(fg, device="cuda"), method="meanshift",
                                   bandwidth=bw, shifts=0, max_objects=1, assign_rest=False))
    g = got["labels"].reshape(-1)
    assert got["n_objects"].tolist() == [1] and set(g.tolist()) <= {0, 1} and not g[~f].any()
    assert np.array_equal(g[~exempt], ref["labels"][~exempt])
    assert abs(int(got["sizes"][0, 0]) - int(ref["sizes"][0])) <= int(exempt.sum())
    assert np.array_equal(got["centres"][0, 0], c)


@pytest.mark.parametrize("run", ["A-ms-refine2", "B-km"])
def test_three_runs_give_the_same_bits(run):
    m = model()
    outs = []
    for i in range(3):
        outs.append(host(run_device(m, run, "bf16")))
        other = torch.randn(257, 129, device="cuda")           # an unrelated launch in between
        (other @ other.t()).sum().item()
    for o in outs[1:]:
        for k in outs[0]:
            assert o[k].tobytes() == outs[0][k].tobytes(), k


@pytest.mark.parametrize("run", ["A-ms", "A-km-3of5"])
def test_capture_and_replay_equals_eager(run):
    """Nothing is read back and the launch sequence does not depend on the data: one capture on one stream replays."""
    m = model()
    args = device_args(run, "fp32")                             # nothing is copied from the host inside the capture
    eager = host(run_device(m, run, "fp32", args))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run_device(m, run, "fp32", args)
    for v in out.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    got = host(out)
    for k in eager:
        assert got[k].tobytes() == eager[k].tobytes(), k
    assert eager["n_objects"].tolist() == reference(run, "fp32")["n_objects"].tolist()


def _images(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g)


def test_segment_embedding_feeds_scoring_and_cleaning():
    m = model(instance=True)
    x = _images(2, 64, 64, 3)
    emb = m.embedding(x)
    assert emb.shape == (2, 24, 64, 64) and emb.dtype == torch.float32 and bool(torch.isfinite(emb).all())
    sem_map = torch.zeros(2, 64 * 64)
    sem_map[0, 100:3000] = 1.0
    bw = float(emb.std()) * 3.0                                # a radius on the scale of this random embedding
    sem_out, sem_arg, labels, n = m.segment_embedding(x, sem_map=sem_map, bandwidth=bw, max_objects=6)
    assert sem_out.shape == (2, 2, 64, 64) and sem_arg.shape == (2, 1, 64, 64)
    assert labels.dtype == torch.uint8 and labels.shape == (2, 64, 64) and n.dtype == torch.int32
    lab, cnt = labels.cpu().numpy(), n.cpu().numpy()
    assert 1 <= cnt[0] <= 6 and cnt[1] == 0 and not lab[1].any()
    f = sem_map.view(2, 64, 64).numpy() != 0
    assert (lab[0][f[0]] != 0).all() and not lab[0][~f[0]].any() and lab.max() == cnt[0]
    # the same embedding through cluster_embedding gives the same labels
    again = m.cluster_embedding(emb, sem_map.view(2, 64, 64), bandwidth=bw, max_objects=6)
    assert np.array_equal(again["labels"].cpu().numpy(), lab)
    # scored against themselves as ground-truth planes: a perfect score; cleaned: a valid map again
    planes = torch.stack([(labels == i + 1) for i in range(32)], 3).to(torch.uint8)
    s = m.score_instances(labels, n, planes, n, max_objects=32).cpu().numpy()
    assert s[0, 2] == 1.0 and s[0, 5] == 0.0 and s[0, 4] == cnt[0]
    cl, cn, _ = m.clean_instances(labels, max_objects=32)
    assert cl.shape == labels.shape and int(cn[0]) >= 1 and int(cn[1]) == 0
    km = m.segment_embedding(x, sem_map=sem_map, method="kmeans", n_objects=torch.tensor([3, 2]), iters=4)
    assert km[3].tolist() == [3, 0] and set(np.unique(km[2][0].cpu().numpy()).tolist()) <= {0, 1, 2, 3}


def test_predict_instances_default_is_the_attention_path():
    """Model.predict_instances / evaluate with the default keywords (and with method='attention') never reach the new code -
    every new method is replaced by one that raises - and hand back exactly, bit for bit, what segment() produced in that
    call: the probability map, the labels and the counts.  The comparison is made inside ONE call (segment is wrapped to
    keep what it returned), as tests/test_gpu_components.py does, because the eval-mode logits of this model differ in the
    last bit from one forward to the next.  With method='meanshift' / 'kmeans' the call hands back what segment_embedding
    produced in it."""
    import reseg_ref as R
    from isa_amd.model import Model
    need_gpu()
    x, sem, ins, n = R.synth_batch(2, 64, 64, seed=2)
    model_ = Model("CVPPP", "ReSeg", 2, 5, use_instance_segmentation=True)
    net = model_.model
    seen, real_segment = [], net.segment

    def segment(*a, **k):
        seen.append(real_segment(*a, **k))
        return seen[-1]

    def trap(*a, **k):
        raise AssertionError("the default arguments reached the clustering code")

    net.segment = segment
    new_code = [(net, "segment_embedding"), (net, "cluster_embedding"), (net, "embedding"), (net, "cluster")]
    real = [getattr(obj, name) for obj, name in new_code]
    for obj, name in new_code:
        setattr(obj, name, trap)
    for kwargs in ({}, dict(method="attention"), dict(method="attention", bandwidth=None, n_objects=None)):
        del seen[:]
        prob, labels, count = model_.predict_instances(x, **kwargs)
        assert len(seen) == 1
        want_prob = net.net.softmax_nchw(net._last_sem)[:, 1]                  # the logits of that call, still in its arena
        assert torch.equal(prob, want_prob.cpu())
        assert torch.equal(labels, seen[0][2].cpu()) and torch.equal(count, seen[0][3].cpu())
    for kwargs in ({}, dict(method="attention")):
        del seen[:]
        res = model_.evaluate([(x, sem, ins, n)], **kwargs)
        assert len(seen) == 1
        _, sem_arg, lab, cnt = seen[0]
        want = net.score_instances(lab, cnt, ins, n, sem_arg, sem, max_objects=5).cpu().numpy()
        assert np.array_equal(res["per_image"], want, equal_nan=True)
    with pytest.raises(AssertionError, match="reached the clustering code"):
        model_.predict_instances(x, method="meanshift")
    # the new methods: what segment_embedding returned in the call, and never the attention decoder
    for (obj, name), fn in zip(new_code, real):
        setattr(obj, name, fn)
    got, real_embed = [], net.segment_embedding

    def segment_embedding(*a, **k):
        got.append(real_embed(*a, **k))
        return got[-1]

    def no_attention(*a, **k):
        raise AssertionError("an embedding method reached segment()")

    net.segment_embedding, net.segment = segment_embedding, no_attention
    for kwargs, cap in ((dict(method="meanshift", bandwidth=0.5), 5), (dict(method="kmeans", n_objects=torch.tensor([2, 3])), 3)):
        del got[:]
        prob, labels, count = model_.predict_instances(x, **kwargs)
        assert len(got) == 1
        assert torch.equal(prob, net.net.softmax_nchw(net._last_sem)[:, 1].cpu())
        assert torch.equal(labels, got[0][2].cpu()) and torch.equal(count, got[0][3].cpu())
        assert labels.dtype == torch.uint8 and int(count.max()) <= cap and int(labels.max()) <= int(count.max())
    res = model_.evaluate([(x, sem, ins, n)], method="kmeans")                 # the ground-truth counts of the batch, capped
    assert all(g <= min(int(v), 5) for g, v in zip(got[-1][3].tolist(), n.view(-1))) and res["n_images"] == 2
    with pytest.raises(ValueError):
        model_.predict_instances(x, method="kmeans")
    with pytest.raises(ValueError):
        model_.predict_instances(x, method="dbscan")


def test_pred_list_instances_from_embedding(tmp_path):
    """pred_list.py --instances --instances-from embedding writes the five files per image that evaluate.py reads."""
    from PIL import Image
    need_gpu()
    out = str(tmp_path / "emb")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "pred_list.py"), "--synthetic", "4", "--batch", "4", "--instances",
                        "--instances-from", "embedding", "--output", out], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    names = sorted(os.listdir(out))
    assert names == ["synthetic_%04d" % i for i in range(4)]
    for i, name in enumerate(names):
        d = os.path.join(out, name)
        assert sorted(os.listdir(d)) == sorted(name + s for s in ("-fg_mask.png", "-ins_mask.png", "-ins_mask_color.png",
                                                                  "-n_objects.npy", ".png"))
        ins = np.array(Image.open(os.path.join(d, name + "-ins_mask.png")))
        fgm = np.array(Image.open(os.path.join(d, name + "-fg_mask.png")))
        k = int(np.load(os.path.join(d, name + "-n_objects.npy")))
        assert ins.shape == (300 + 7 * (i % 5), 330) and ins.dtype == np.uint8
        assert k == int(ins.max()) and 0 <= k <= 32
        assert not ins[fgm == 0].any()
        assert (ins[fgm == 255] != 0).all()                    # assign_rest: the whole predicted foreground is explained
