"""Adam, RMSprop and SGD (csrc/optim.hip) and fit()'s train_cnn=False, against the installed torch.optim - what the
reference calls (model.py:145-166) - from the C ABI up to Model.fit.

The bound is derived in each test, not chosen: torch.optim runs twice on the CPU from the same fp32 start and the same
clipped gradient, once in float64 (the reference) and once in fp32.  The fp32 run's error against the float64 run, per
quantity and relative to that quantity's max, is the floor any fp32 implementation has; the kernel is allowed
FLOOR_FACTOR = 4 times it.  The margin covers the rounding order of the fused clip and decay and sqrtf / division being an
ulp off torch's.  The clip coefficient the reference uses is computed in double from the very fp32 squared norm the
kernel reads (isa_sqnorm's accuracy has its own test in test_gpu_streaming.py), so the comparison isolates the update.

Measured on MI355X, worst over steps and cases, the kernel's error (torch's fp32 floor), relative to the quantity's max:
  kernel level (n = 600001 and 2500003, clip on and off, three steps):
    Adam     params 1.1e-7 (1.1e-7)   exp_avg 1.1e-7 (1.2e-7)   exp_avg_sq 2.3e-7 (2.3e-7)
    RMSprop  params 1.2e-7 (1.2e-7)   square_avg 2.0e-7 (1.8e-7)
    SGD      params 1.1e-7 (1.1e-7)   momentum_buffer 1.2e-7 (1.5e-7)
  replayed Trainer.apply_update (n = 4 759 800, four updates):
    Adam     params 1.3e-7 (1.3e-7)   exp_avg 1.2e-7 (1.4e-7)   exp_avg_sq 2.1e-7 (2.4e-7)
    RMSprop  params 1.1e-7 (1.1e-7)   square_avg 1.8e-7 (2.3e-7)
    SGD      params 1.0e-7 (1.0e-7)   momentum_buffer 1.3e-7 (2.0e-7)
  model level (train_64 fixture, worst tensor of two steps; frozen backbone in brackets):
    Adam 2.9e-6, floor 8.7e-5 [2.3e-6, 1.2e-4];  RMSprop 2.7e-5, floor 2.1e-4 [1.2e-5, 1.7e-4];
    SGD 9.8e-8 = its floor [9.4e-8];  Adadelta frozen 1.0e-7 = its floor
  At model level Adam's and RMSprop's own fp32 floors exceed the project's 1e-5: real gradients hold elements where
  g*clip + wd*p nearly cancels, and the first steps of both divide by sqrt(v) + 1e-8 with v ~ gr^2.  There the bound is
  4x the tensor's floor, as for the kernel tests (RMSprop needs it: 2.7e-5 on one tensor whose floor is 2.1e-4).
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

from test_gpu_ops import _gpu, rand  # noqa: E402

FLOOR_FACTOR = 4.0
MODEL_BOUND = 1e-5                     # tests/test_gpu_train.py: the project's bound for a model-level update, of the tensor's max
SUM_BOUND = 1e-5                       # tests/test_gpu_streaming.py: isa_sqnorm, relative to its sum of terms
NEW = ("Adam", "RMSprop", "SGD")
LR = {"Adadelta": 1.0, "Adam": 1e-3, "RMSprop": 1e-3, "SGD": 1e-2}
STATE = {"Adadelta": ("square_avg", "acc_delta"), "Adam": ("exp_avg", "exp_avg_sq"), "RMSprop": ("square_avg",),
         "SGD": ("momentum_buffer",)}


def make_opt(name, params, lr, wd):
    """The optimizer as model.py:150-162 constructs it."""
    if name == "Adam":
        return torch.optim.Adam(params, lr=lr, weight_decay=wd)
    if name == "RMSprop":
        return torch.optim.RMSprop(params, lr=lr, weight_decay=wd)
    if name == "SGD":
        return torch.optim.SGD(params, lr=lr, momentum=0.9, weight_decay=wd)
    return torch.optim.Adadelta(params, lr=lr, weight_decay=wd)


def rel_err(got, ref):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float(torch.nan_to_num((got - ref).abs(), nan=float("inf")).max() / (ref.abs().max() + 1e-300))


def check_vs_floor(tag, got, ref64, ref32, least=0.0):
    """got within max(least, FLOOR_FACTOR x the fp32 floor) of the float64 reference; returns (error, floor)."""
    e, floor = rel_err(got, ref64), rel_err(ref32, ref64)
    bound = max(least, FLOOR_FACTOR * floor)
    print("OPTERR %-56s %.3e  floor %.3e  bound %.3e" % (tag, e, floor, bound))
    assert e <= bound, "%s: error %.3g > %.3g (fp32 floor %.3g)" % (tag, e, bound, floor)
    return e, floor


def clip_coef(sqnorm32, max_norm):
    """clip_grad_norm_'s coefficient, in double, from the fp32 squared norm the kernel reads."""
    return min(1.0, max_norm / (float(np.sqrt(np.float64(sqnorm32))) + 1e-6)) if max_norm > 0 else 1.0


class TwoRefs:
    """torch.optim on one flat CPU tensor, in float64 and in fp32, fed the same already-clipped gradient."""
    def __init__(self, name, p0, lr, wd):
        self.name = name
        self.p64 = p0.detach().double().cpu().clone().requires_grad_(True)
        self.p32 = p0.detach().float().cpu().clone().requires_grad_(True)
        self.o64, self.o32 = make_opt(name, [self.p64], lr, wd), make_opt(name, [self.p32], lr, wd)

    def step(self, g64):
        self.p64.grad, self.p32.grad = g64.clone(), g64.float()
        self.o64.step(); self.o32.step()

    def state(self, key):
        return self.o64.state[self.p64][key], self.o32.state[self.p32][key]


def seeded_grad(n, seed, lo):
    """A seeded gradient: every seventh element (at random positions) exactly 0, the others of either sign with magnitude
    in [lo, 3 lo].  The lower end keeps g*gscale*clip clear of -wd*p (the callers assert a factor 2): where the two cancel to
    within eps = 1e-8, Adam's and RMSprop's first steps divide by that eps, torch.optim's own fp32 run is then 1e-4 off
    its float64 run in a handful of elements, and comparing two fp32 implementations against such a floor is a lottery
    of which element rounds which way.  With that ruled out the floor is what fp32 rounding leaves on well-conditioned
    elements, and 4x it is a bound that means something.  (Elements with g = 0 have gr = wd*p: one product, no cancellation.)"""
    gen = torch.Generator().manual_seed(seed)
    mag = lo * (1.0 + 2.0 * torch.rand(n, generator=gen))
    g = torch.where(torch.rand(n, generator=gen) < 0.5, -mag, mag)
    g[torch.randperm(n, generator=gen)[:n // 7]] = 0.0
    return g


# ------------------------------------------------------------------------------------------------ 1. kernel level
def call_update(L, lib, name, p, g, states, n, lr, wd, sqn, max_norm, gscale, lrd, extra):
    args = (L.ptr(sqn), max_norm, gscale, L.ptr(lrd), L.stream_ptr())
    if name == "Adam":
        rc = lib.isa_adam(L.ptr(p), L.ptr(g), L.ptr(states[0]), L.ptr(states[1]), L.ptr(extra["step"]), L.ptr(extra["aux"]),
                          n, lr, 0.9, 0.999, 1e-8, wd, *args)
    elif name == "RMSprop":
        rc = lib.isa_rmsprop(L.ptr(p), L.ptr(g), L.ptr(states[0]), n, lr, 0.99, 1e-8, wd, *args)
    else:
        rc = lib.isa_sgd(L.ptr(p), L.ptr(g), L.ptr(states[0]), n, lr, 0.9, wd, *args)
    L.check(rc, name)


# n = 600001: 150000 groups of 4 floats = 586 workgroups (one trip each) and a 1-element tail; n = 2500003: 625000 groups
# on the capped grid of 1024 workgroups (stride 262144 groups: 2.4 trips, the last one ragged) and a 3-element tail
@pytest.mark.parametrize("n", [600001, 2500003])
@pytest.mark.parametrize("clip_on", [True, False], ids=["clip-on", "clip-off"])
@pytest.mark.parametrize("name", NEW)
def test_kernel_matches_torch_optim(name, clip_on, n):
    """Three consecutive steps through the C ABI: parameters and every state tensor after each step.  gscale = 0.5,
    weight decay 1e-2, a seeded gradient with exact zeros (seeded_grad); clip-on sets max_norm to half the first
    gradient's norm, so the clip is engaged (at about 0.5) on every step, clip-off to 1000, which never engages it.
    clip-on passes lr through the device scalar (and a wrong host value), clip-off through the argument."""
    L = _gpu()[0]
    lib = L.lib()
    gscale, wd, lr, glo = 0.5, 1e-2, LR[name], 0.01
    max_norm = 0.5 * gscale * float(seeded_grad(n, 192, glo).double().norm()) if clip_on else 1000.0
    p0 = rand(n, seed=191, scale=0.01)
    bufs = [torch.full((n + 8,), 7.0, device="cuda") for _ in range(1 + len(STATE[name]))]   # 8 guard floats behind each range
    p, states = bufs[0][:n], [b[:n] for b in bufs[1:]]
    p.copy_(p0)
    for s in states:
        s.zero_()
    extra = dict(step=torch.zeros(1, dtype=torch.int32, device="cuda"), aux=torch.zeros(4, device="cuda"))
    lrd = torch.tensor([lr], device="cuda") if clip_on else None
    refs = TwoRefs(name, p0, lr, wd)
    for step in range(3):
        g = seeded_grad(n, 192 + step, glo)
        sq64 = float(((g.double() * gscale) ** 2).sum())
        sqn = torch.tensor([sq64], dtype=torch.float32, device="cuda")
        clip = clip_coef(float(sqn[0]), max_norm)
        assert (clip < 1.0) == clip_on and clip > 0.4, (step, clip)
        assert 2 * wd * float(p.abs().max()) < glo * gscale * clip, "seeded_grad: gradient too close to the decay term"
        call_update(L, lib, name, p, g.cuda(), states, n, 123.0 if clip_on else lr, wd, sqn, max_norm, gscale, lrd, extra)
        torch.cuda.synchronize()
        refs.step(g.double() * gscale * clip)
        tag = "%s %s n=%d step %d " % (name, "clip-on" if clip_on else "clip-off", n, step)
        check_vs_floor(tag + "params", p, refs.p64, refs.p32)
        for key, s in zip(STATE[name], states):
            check_vs_floor(tag + key, s, *refs.state(key))
        if name == "Adam":
            assert int(extra["step"]) == step + 1
    assert all(bool((b[n:] == 7.0).all()) for b in bufs)            # the scalar tail stops at n


def test_refused_update_changes_nothing():
    """ISA_EINVAL for a null pointer and for n <= 0 with nothing launched: parameters, state and Adam's step count keep
    their bits (the CPU half of this check, with every other bad argument, is in test_train_flags.py)."""
    L = _gpu()[0]
    lib = L.lib()
    n = 1024
    for name in NEW:
        p, g = rand(n, seed=1).cuda(), rand(n, seed=2).cuda()
        states = [torch.full((n,), 3.0, device="cuda") for _ in STATE[name]]
        extra = dict(step=torch.zeros(1, dtype=torch.int32, device="cuda"), aux=torch.zeros(4, device="cuda"))
        sqn = torch.ones(1, device="cuda")
        p0 = p.clone()
        for bad in ("n0", "n-1", "p", "g", "state"):
            with pytest.raises(L.IsaError, match="ISA_EINVAL"):
                call_update(L, lib, name, None if bad == "p" else p, None if bad == "g" else g,
                            [None] + states[1:] if bad == "state" else states, {"n0": 0, "n-1": -1}.get(bad, n),
                            LR[name], 1e-3, sqn, 1.0, 1.0, None, extra)
        torch.cuda.synchronize()
        assert torch.equal(p, p0) and all(bool((s == 3.0).all()) for s in states) and int(extra["step"]) == 0, name


# ------------------------------------------------------------------------------------------------ 2. replay
def _model(dtype=torch.float32):
    import isa_amd  # noqa: F401
    import reseg_ref as R
    from isa_amd.reseg import ReSeg
    from isa_amd.trainer import Trainer
    m = ReSeg(2, True, dtype=dtype)
    m.load_state_dict(R.synth_state_dict(23, True))
    m.train()
    return m, Trainer, R


@pytest.mark.parametrize("name", NEW)
def test_replayed_update_keeps_counting_steps(name):
    """Trainer.apply_update() alone in a hipGraph (one straight line of launches), gradient contents fixed: one eager
    update, capture, three replays = four updates, against four torch.optim steps at the kernel test's bound.  A step count
    baked in at capture would give Adam the bias correction of t = 2 on every replay (a 1.9x, then 2.7x, too long step).
    The clip (max_norm 10) is engaged; the reference reads the squared norm isa_sqnorm left for the update, which is itself
    checked against float64.  Weight decay is 1e-4 here: the clipped gradient of 4.8 M elements has norm 10, hence
    magnitudes from 2.4e-3, and the weights reach 2.1 - at the reference's 1e-3 the two would meet (see seeded_grad)."""
    _gpu()
    m, Trainer, _ = _model()
    st = m.store
    n = st.n_train
    wd = 1e-4
    tr = Trainer(m, lr=LR[name], weight_decay=wd, optimizer=name)
    g = seeded_grad(n, 77, 0.01)
    st.grad[:n].copy_(g)
    sq64 = float((g.double() ** 2).sum())
    assert sq64 > 4 * 10.0 ** 2                          # norm > 2 x max_norm: the clip is engaged
    assert 2 * wd * (float(st.flat[:n].abs().max()) + 4 * LR[name]) < 0.01 * 10.0 / sq64 ** 0.5
    refs = TwoRefs(name, st.flat[:n], LR[name], wd)
    graph = torch.cuda.CUDAGraph()

    def after_update(k):
        torch.cuda.synchronize()
        sqn = float(tr.sqnorm[0])
        assert abs(sqn - sq64) <= SUM_BOUND * sq64, (k, sqn, sq64)
        refs.step(g.double() * clip_coef(sqn, 10.0))
        tag = "%s replay update %d " % (name, k)
        check_vs_floor(tag + "params", st.flat[:n], refs.p64, refs.p32)
        for key in STATE[name]:
            check_vs_floor(tag + key, tr.state[key], *refs.state(key))
        if name == "Adam":
            assert int(tr.state["step"]) == k

    tr.apply_update()
    after_update(1)
    with torch.cuda.graph(graph):
        tr.apply_update()
    for k in (2, 3, 4):
        graph.replay()
        after_update(k)
    assert torch.equal(st.grad[:n].cpu(), g)             # world 1: the update reads the gradient, never writes it


# ------------------------------------------------------------------------------------------------ 3. model level
def _fixture(optimizer, train_cnn=True):
    from test_gpu_train import need_gpu, setup
    ReSeg, Trainer = need_gpu()
    z = np.load(os.path.join(ROOT, "tests", "golden", "train_64.npz"))
    m, _, batch, sel, inj = setup(ReSeg, Trainer, z, torch.float32)
    tr = Trainer(m, lr=LR[optimizer], optimizer=optimizer, train_cnn=train_cnn)
    return m, tr, batch, sel, inj


class ModelRefs:
    """torch.optim + clip_grad_norm_(10) over the named tensors, in float64 and fp32 on the CPU."""
    def __init__(self, name, start, keys, lr, wd=1e-3):
        self.p64 = {k: torch.nn.Parameter(start[k].double().cpu().clone()) for k in keys}
        self.p32 = {k: torch.nn.Parameter(start[k].float().cpu().clone()) for k in keys}
        self.o64, self.o32 = make_opt(name, self.p64.values(), lr, wd), make_opt(name, self.p32.values(), lr, wd)

    def step(self, grads):
        for k in self.p64:
            self.p64[k].grad, self.p32[k].grad = grads[k].double().cpu(), grads[k].float().cpu()
        for ps, o in ((self.p64, self.o64), (self.p32, self.o32)):
            torch.nn.utils.clip_grad_norm_(ps.values(), 10.0)
            o.step()

    def check(self, tag, after):
        worst = (0.0, 0.0, "")
        for k in self.p64:
            e, f = rel_err(after[k], self.p64[k]), rel_err(self.p32[k], self.p64[k])
            assert e <= max(MODEL_BOUND, FLOOR_FACTOR * f), (tag, k, e, f)
            worst = max(worst, (e, f, k))
        print("OPTERR %-56s %.3e  floor %.3e  (%s; %d tensors)" % (tag, worst[0], worst[1], worst[2], len(self.p64)))


@pytest.mark.parametrize("name", NEW)
def test_model_update_matches_torch_optim(name):
    """test_optimizer_matches_torch_adadelta's pattern for the other three: two steps on the train_64 fixture, the step's
    own gradients fed to torch.optim with clip_grad_norm_(10), every trained tensor within 1e-5 of its max (the project's
    bound for this check) - or within 4x that tensor's own fp32 floor where torch's fp32 run itself is further than that
    from its float64 run.  Never-trained tensors and all running statistics keep their bits across the update."""
    m, tr, batch, sel, inj = _fixture(name)
    st = m.store
    before = {k: v.clone() for k, v in m.state_dict().items()}
    trained = [k for k, _ in m.named_parameters() if st.offsets[k] < st.n_train]
    refs = ModelRefs(name, before, trained, LR[name])
    for step in range(2):
        tr.forward_backward(*batch, selected_idx=sel, injected_s_t=inj)
        refs.step({k: p.grad.clone() for k, p in m.named_parameters() if k in refs.p64})
        untouched = st.flat[st.n_train:].clone()
        tr.apply_update()
        torch.cuda.synchronize()
        after = m.state_dict()
        refs.check("%s model step %d" % (name, step), after)
        assert torch.equal(st.flat[st.n_train:], untouched)          # never-trained tensors and running statistics
        for k in ("decoder.pred.l_i.weight", "decoder.embedding.sigma.0.weight"):
            assert torch.equal(after[k].cpu(), before[k].cpu())
    assert any(not torch.equal(after[k], before[k]) for k in trained)


# ------------------------------------------------------------------------------------------------ 4. train_cnn=False
@pytest.mark.parametrize("name", ("Adadelta",) + NEW)
def test_frozen_backbone(name):
    """fit(..., train_cnn=False) (model.py:196-202): after two train_steps every base.* parameter keeps its bits, weight
    decay included, while the backbone's BatchNorm still runs on batch statistics and moves its running means; every other
    trained tensor matches torch.optim fed the non-base gradients only and clipped on THEIR norm alone."""
    m, tr, batch, sel, inj = _fixture(name, train_cnn=False)
    st = m.store
    before = {k: v.clone() for k, v in m.state_dict().items()}
    trained = [k for k, _ in m.named_parameters() if st.offsets[k] < st.n_train]
    base = [k for k in trained if k.startswith("base.")]
    rest = [k for k in trained if not k.startswith("base.")]
    assert base and rest and tr.lo == sum((st.numel(k) + 3) // 4 * 4 for k in base)      # every tensor starts 16-byte aligned
    assert all(st.offsets[k] < tr.lo for k in base) and all(st.offsets[k] >= tr.lo for k in rest)
    assert all(t.numel() == st.n_train - tr.lo for k, t in tr.state.items() if k != "step")
    refs = ModelRefs(name, before, rest, LR[name])
    for step in range(2):
        tr.train_step(*batch, selected_idx=sel, injected_s_t=inj)
        torch.cuda.synchronize()
        grads = {k: p.grad.clone() for k, p in m.named_parameters()}
        assert float(max(grads[k].abs().max() for k in base)) > 0   # the tape still computes them; the update ignores them
        refs.step({k: grads[k] for k in rest})
        after = m.state_dict()
        for k in base:
            assert torch.equal(after[k], before[k]), (step, k)
        refs.check("%s frozen step %d" % (name, step), after)
    means = [k for k in before if k.startswith("base.") and k.endswith("running_mean")]
    assert means and all(not torch.equal(after[k], before[k]) for k in means)


def test_frozen_backbone_in_the_captured_step():
    """train_step_graphed with train_cnn=False and Adam: eager first sight, capture + replay, replay.  The frozen prefix
    keeps its bits, the rest moves on every step, and the device step count follows the replays."""
    from test_gpu_train import _graph_fixture
    m, _, batch, order, inj = _graph_fixture()
    from isa_amd.trainer import Trainer
    tr = Trainer(m, lr=LR["Adam"], optimizer="Adam", train_cnn=False)
    st = m.store
    start = st.flat.clone()
    prev = start
    for k in range(3):
        tr.train_step_graphed(*batch, selected_idx=order, injected_s_t=inj)
        torch.cuda.synchronize()
        now = st.flat.clone()
        assert torch.equal(now[:tr.lo], start[:tr.lo]), k
        assert float((now[tr.lo:st.n_train] - prev[tr.lo:st.n_train]).abs().max()) > 0, k
        assert int(tr.state["step"]) == k + 1
        prev = now
    assert any(s.get("state") == "ready" for s in tr._graphs.values()), "graph was never captured"
    assert torch.isfinite(st.flat).all()


# ------------------------------------------------------------------------------------------------ 5. defaults
def test_defaults_are_todays_adadelta_over_the_whole_slice():
    _gpu()
    m, Trainer, _ = _model()
    st = m.store
    tr = Trainer(m)
    assert tr.optimizer == "Adadelta" and tr.train_cnn is True and tr.lo == 0
    assert tr.sq.numel() == tr.acc.numel() == st.n_train
    assert tr.state["square_avg"] is tr.sq and tr.state["acc_delta"] is tr.acc
    st.grad[:st.n_train].fill_(1.2345e-3)
    start = st.flat.clone()
    tr.apply_update()
    torch.cuda.synchronize()
    # square_avg = 0.1 * gr^2 with gr = g + wd * p: positive wherever the update ran (no weight equals -1.2345)
    assert bool((tr.sq > 0).all()) and bool((tr.acc > 0).all())
    assert not torch.equal(st.flat[:st.n_train], start[:st.n_train])
    assert torch.equal(st.flat[st.n_train:], start[st.n_train:])
    with pytest.raises(AssertionError):
        Trainer(m, optimizer="Adagrad")


# ------------------------------------------------------------------------------------------------ 6. entry point
def test_fit_with_adam_on_a_frozen_backbone(tmp_path):
    _gpu()
    from isa_amd.data import SyntheticLoader
    from isa_amd.model import Model
    m = Model('CVPPP', 'ReSeg', 2, 32, use_instance_segmentation=True)
    before = {k: v.clone().cpu() for k, v in m.model.state_dict().items()}
    tr, te = SyntheticLoader(2, 2, 64, 64, seed=1), SyntheticLoader(1, 2, 64, 64, seed=2)
    m.fit('Multi', 0.5, 1.5, 2, 1e-3, 0.001, 10.0, 0.5, 25, False, 'Adam', False, 1, None, tr, te, str(tmp_path), False)
    assert m.trainer.optimizer == "Adam" and m.trainer.train_cnn is False
    assert int(m.trainer.state["step"]) == 2
    for log in ("training.log", "validation.log"):
        assert len(open(os.path.join(str(tmp_path), log)).read().strip().splitlines()) == 2
    ckpts = [f for f in os.listdir(str(tmp_path)) if f.endswith(".pth")]
    assert len(ckpts) == 1
    loaded = torch.load(os.path.join(str(tmp_path), ckpts[0]), map_location="cpu", weights_only=True)
    params = [k for k, _ in m.model.named_parameters()]
    base = [k for k in params if k.startswith("base.")]
    assert base
    for k in base:
        assert torch.equal(loaded[k], before[k]), k
    moved = [k for k in params if not k.startswith("base.") and not torch.equal(loaded[k], before[k])]
    assert len(moved) > 100 and all(bool(torch.isfinite(loaded[k]).all()) for k in params)
