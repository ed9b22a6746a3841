"""GPU: the discriminative embedding loss kernels (isa_disc_*) through ReSeg.discriminative_loss and the trainer, against
the float64 restatement tests/disc_np.py (itself pinned to the reference by tests/test_disc_ref.py).

Bounds.  fp32 storage: every scalar and the means within max(8 x ref32_gap_loss, 1e-6) relative, the gradient within
max(8 x ref32_gap_grad, 1e-6) relative L2, where the gaps are what the reference's own fp32 run loses against its fp64 run
(tests/golden/disc.npz, the largest of its cases: 2.5e-7 and 5.4e-7 when the fixture was made, so 2.0e-6 and 4.3e-6); the
factor 8 allows another fp32 summation order than the reference's, the floor is a few ulp of an fp32 sum.  The means are
compared as a tensor: largest error over largest value.  bf16 storage: the restatement gets the same bf16-rounded inputs
in float64; arithmetic is fp32, so the scalars and means keep the fp32 bound; a gradient written to a bf16 tensor gets
2^-8 relative L2 (half an ulp, 2^-9, per element, times two).
Shapes are the ones where the kernels can go wrong, not the workload's: 40 x 52 (three chunks and a tail, no multiple of
a tile), 64 x 64 (four full chunks), 4 x 8 (less than one MFMA tile); C in {24, 32, 5}; ld > c; n_objects 0, 1, 2, 32."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import disc_np as NP        # noqa: E402
import reseg_ref as R       # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "disc.npz"))
GAP_LOSS = max(float(GOLD[k]) for k in GOLD.files if k.endswith("ref32_gap_loss"))
GAP_GRAD = max(float(GOLD[k]) for k in GOLD.files if k.endswith("ref32_gap_grad"))
TOL_S, TOL_G, TOL_G_BF16 = max(8 * GAP_LOSS, 1e-6), max(8 * GAP_GRAD, 1e-6), 2.0 ** -8
SCALARS = ("loss", "var", "dist", "reg", "qreg")


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import isa_amd  # noqa: F401
    from isa_amd.reseg import ReSeg
    from isa_amd.trainer import Trainer
    return ReSeg, Trainer


_MODEL = {}


def model():
    """One small semantic-only model for every operator test (the operator needs an engine, not the weights)."""
    ReSeg, _ = need_gpu()
    if "m" not in _MODEL:
        _MODEL["m"] = ReSeg(2, False, dtype=torch.float32)
    return _MODEL["m"]


def _labels(kind, H, W, rs):
    lab = np.zeros((H, W), dtype=np.int64)
    if kind == "runs":                        # long runs: bands of rows; label 5 is left out (an empty counted instance)
        for r in range(H):
            lab[r] = (0, 1, 2, 3, 4, 6)[(r * 6) // H]
    elif kind == "checker":
        lab = 1 + (np.add.outer(np.arange(H), np.arange(W)) % 2)
    elif kind == "pixels32":                  # 32 one-pixel instances, everything else background
        lab.flat[rs.permutation(H * W)[:32]] = np.arange(1, 33)
    elif kind == "random3":
        lab = rs.randint(0, 4, size=(H, W))
    elif kind == "random2":
        lab = rs.randint(0, 3, size=(H, W))
    return lab                                # "background": zeros


CASES = {
    # name: (H, W, C, ld or None, [(label pattern, n_objects)] per image)
    "3x40x52-c24": (40, 52, 24, None, [("runs", 6), ("background", 2), ("checker", 2)]),
    "2x64x64-c32": (64, 64, 32, None, [("pixels32", 32), ("random3", 1)]),
    "1x4x8-c5": (4, 8, 5, None, [("random2", 2)]),
    "2x64x64-c24-ld32": (64, 64, 24, 32, [("random3", 0), ("random3", 3)]),
}


def make_case(name):
    H, W, C, ld, images = CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    labels = np.stack([_labels(kind, H, W, rs) for kind, _ in images])
    B = len(images)
    centres = rs.standard_normal((B, 33, C)) * 0.3
    x = rs.standard_normal((B, H, W, C)) * 0.6 + np.take_along_axis(
        centres, labels.reshape(B, -1, 1).repeat(C, 2), 1).reshape(B, H, W, C)
    return x.transpose(0, 3, 1, 2).copy(), labels, [n for _, n in images], ld


def deltas(C, norm):
    """(delta_v, delta_d) for embeddings spread 0.6 around centres spread 0.3.  delta_v sits at the typical |x - mu|, so about
    half of the pull hinges are active and the sum is carried by the clearly active ones.  The push margin 2 delta_d lies
    well above the distances between means (unit means: at most 2 / sqrt(C); plain means and one-pixel instances: about
    0.95 sqrt(C) / 0.76 C), so the pairs are clearly active too.  A margin AT the typical distance leaves a term that is
    the sum of a few squares of near-cancelled differences (2 delta_d - |mu_i - mu_j| ~ 1e-2 of either): its relative
    error is the fp32 rounding of the distance amplified a hundredfold, in any fp32 evaluation including the
    reference's, and says nothing about the kernels."""
    return (0.6 * np.sqrt(C), 0.75 * np.sqrt(C)) if norm == 2 else (0.6 * 0.8 * C, 0.75 * C)


def run_operator(m, x_t, labels, n_objects, ld, **kw):
    """The operator on an NCHW tensor, or (ld given) on an engine Act with ld > c whose pad channels hold NaN."""
    from isa_amd.engine import Act
    lab = torch.tensor(labels, dtype=torch.uint8, device="cuda")
    n = torch.tensor(n_objects, dtype=torch.int32)
    if ld is None:
        out = m.discriminative_loss(x_t, lab, n, grad=True, **kw)
        return out, out["grad"].float()
    B, C, H, W = x_t.shape
    buf = torch.full((B, H, W, ld), float("nan"), dtype=x_t.dtype, device="cuda")
    buf[..., :C] = x_t.permute(0, 2, 3, 1)
    out = m.discriminative_loss(Act(buf, 0, C), lab, n, grad=True, **kw)
    g = out["grad"]
    assert isinstance(g, Act) and g.ld == ld and g.c == C
    return out, g.buf[..., :C].permute(0, 3, 1, 2).float()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_operator_matches_the_float64_restatement(name, dtype):
    m = model()
    x, labels, n_objects, ld = make_case(name)
    x_t = torch.tensor(x, dtype=torch.float32, device="cuda").to(dtype)
    x64 = x_t.double().cpu().numpy()                                      # what the kernels read, exactly
    tol_g = TOL_G if dtype == torch.float32 else TOL_G_BF16
    worst = dict(scalar=0.0, means=0.0, grad=0.0)
    for form in ("reference", "full"):
        for norm in (1, 2):
            for unit in (False, True):
                dv, dd = deltas(x.shape[1], norm)
                ref = NP.discriminative(x64, labels, n_objects, dv, dd, norm, unit, NP.FORMS[form][1])
                out, grad = run_operator(m, x_t, labels, n_objects, ld, delta_var=dv, delta_dist=dd, norm=norm, form=form,
                                         unit_means=unit)
                tag = "%s %s %s norm%d unit%d" % (name, str(dtype)[6:], form, norm, unit)
                for key in SCALARS:
                    got = float(out[key])
                    err = abs(got - ref[key]) / abs(ref[key]) if ref[key] else abs(got)
                    worst["scalar"] = max(worst["scalar"], err)
                    print("%s %-5s got %.9g want %.9g rel %.2e" % (tag, key, got, ref[key], err))
                    assert err <= TOL_S, (tag, key, got, ref[key])
                means = out["means"].double().cpu().numpy()
                assert means.shape == (x.shape[0], 32, x.shape[1])
                em = float(np.abs(means - ref["means"]).max() / max(np.abs(ref["means"]).max(), 1e-30))
                g = grad.double().cpu().numpy()
                assert np.isfinite(g).all()
                eg = float(np.linalg.norm(g - ref["grad"]) / np.linalg.norm(ref["grad"]))
                worst["means"], worst["grad"] = max(worst["means"], em), max(worst["grad"], eg)
                print("%s means rel %.2e  grad rel L2 %.2e" % (tag, em, eg))
                assert em <= TOL_S, (tag, em)
                assert eg <= tol_g, (tag, eg)
                assert (g[labels[:, None].repeat(x.shape[1], 1) == 0] == 0).all()       # background: exactly no gradient
    print("WORST %s %s: scalar %.2e means %.2e (bound %.2e), grad %.2e (bound %.2e)"
          % (name, str(dtype)[6:], worst["scalar"], worst["means"], TOL_S, worst["grad"], tol_g))


def test_the_cases_hold_what_they_claim():
    """CPU-side facts of the inputs above (no kernel): the counted-but-empty instance, the all-background image, the 32
    one-pixel instances, n_objects 0 with foreground, planes past n_objects."""
    need_gpu()
    x, labels, n, _ = make_case("3x40x52-c24")
    assert n == [6, 2, 2] and not (labels[0] == 5).any() and (labels[0] == 6).any() and not labels[1].any()
    assert 40 * 52 == 2080 and 2080 % 64 and 2080 > 2 * 1024
    ref = NP.discriminative(x, labels, n, 1.0, 1.5, 2, False, (1, 1, 1, 1))
    assert ref["n_present"] == 5 + 0 + 2
    x, labels, n, _ = make_case("2x64x64-c32")
    assert all((labels[0] == i).sum() == 1 for i in range(1, 33)) and (labels[1] > 1).any() and n == [32, 1]
    x, labels, n, _ = make_case("2x64x64-c24-ld32")
    assert n[0] == 0 and labels[0].any()


def test_three_runs_and_an_unrelated_launch_give_the_same_bits():
    m = model()
    x, labels, n_objects, _ = make_case("3x40x52-c24")
    x_t = torch.tensor(x, dtype=torch.float32, device="cuda")
    runs = []
    for i in range(4):
        if i == 3:                                                        # an unrelated launch in between
            junk = torch.randn(1 << 20, device="cuda").sum()
        out, g = run_operator(m, x_t, labels, n_objects, None, delta_var=2.9, delta_dist=1.5, norm=2, form="full")
        runs.append((out["loss"].clone(), out["means"].clone(), g.clone(), torch.stack([out[k] for k in SCALARS])))
    torch.cuda.synchronize()
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], r))
    assert float(runs[0][0]) > 0 and float(junk) == float(junk)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_accumulate_adds_and_zero_overwrites(dtype):
    from isa_amd.engine import Act
    from isa_amd.labelmaps import LabelOps
    from isa_amd.network import DiscCriterion
    m = model()
    x, labels, n_objects, _ = make_case("3x40x52-c24")
    B, C, H, W = x.shape
    ld = 32
    buf = torch.zeros((B, H, W, ld), dtype=dtype, device="cuda")
    buf[..., :C] = torch.tensor(x, dtype=torch.float32, device="cuda").permute(0, 2, 3, 1).to(dtype)
    a = Act(buf, 0, C)
    lab = torch.tensor(labels, dtype=torch.uint8, device="cuda").view(B, -1)
    n = torch.tensor(n_objects, dtype=torch.int32, device="cuda")
    crit = DiscCriterion("cuda")
    crit.set(1.0, 2.9, 1.5, 2, "full")
    alloc = lambda shape, dt: torch.full(shape, float("nan") if dt.is_floating_point else -1, dtype=dt, device="cuda")
    # every scratch buffer starts poisoned
    scal, mu, grad = LabelOps(lib=m.engine.lib, alloc=alloc).disc_loss(a, lab, 32, n, crit.cfg, crit.norm)
    over = Act(torch.full_like(buf, float("nan")), 0, C)
    grad(over, 0)
    pre = torch.randn(B, H, W, ld, device="cuda").to(dtype)
    added = Act(pre.clone(), 0, C)
    grad(added, 1)
    torch.cuda.synchronize()
    g = over.buf[..., :C].float()
    assert torch.isfinite(scal).all() and torch.isfinite(mu).all() and torch.isfinite(g).all() and float(g.abs().max()) > 0
    assert torch.isnan(over.buf[..., C:]).all(), "pad channels of the row must stay untouched"
    assert torch.equal(added.buf[..., C:], pre[..., C:])
    want = pre[..., :C].float() + g
    got = added.buf[..., :C].float()
    if dtype == torch.float32:            # one fp32 rounding of the sum on either side: 2^-24 relative each
        assert float((got - want).abs().max()) <= 2.0 ** -23 * float(want.abs().max())
    else:       # g and the sum are each rounded to bf16 once; an element's worst case is half an ulp = 2^-8 of its value
        assert bool(((got - want).abs() <= 2.0 ** -7 * (pre[..., :C].float().abs() + g.abs())).all())


# ---------------------------------------------------------------------------------------------------------------- training
W_DISC = 1.0e4


def _train_fixture(**trainer_kw):
    ReSeg, Trainer = need_gpu()
    x, sem, ins, n = R.synth_batch(2, 64, 64, seed=1)
    m = ReSeg(2, True, dtype=torch.float32)
    m.load_state_dict(R.synth_state_dict(23, True))
    m.train()
    m.head.drop_rate = 0.0
    m.head.sample_in_training = False
    inj = [torch.tensor([64 * 20 + 9, 64 * 41 + 30], dtype=torch.int32, device="cuda"),
           torch.tensor([64 * 12 + 50, 64 * 33 + 17], dtype=torch.int32, device="cuda")]
    return m, Trainer(m, **trainer_kw), (x, sem, ins, n), [[0, 1], [1, 0]], inj


def _x_enc_grad(m, cap):
    """d(x_enc) as the engine's gradient book holds it after the backward (read before the next begin)."""
    a = cap["x_enc"]
    g = m.engine.grads.bufs[a.buf.data_ptr()]
    return g[..., a.c0:a.c0 + a.c].float().clone(), a.buf[..., a.c0:a.c0 + a.c].float().permute(0, 3, 1, 2).contiguous()


class _Launches:
    """Stands in for Engine.lib and logs the name of every entry point the step calls, in order."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self._log.append(name)
            return fn(*args)
        return call


def test_wiring_of_the_loss_into_the_training_step():
    """(a) weight 0 is the step as it was: no `disc` key, and against a Trainer built without the new arguments the same
    sequence of kernel entries, the same arena allocations, the same gradients.  Bit-equal gradients cannot be asked of two
    runs: this step's backward sums with float atomics, and the Trainer without the new arguments differs from ITSELF run
    to run (measured here and printed: parameter gradients not bit-equal, up to 1.3 apart at a largest value of 319; x_enc
    gradient 1.2e-7 .. 1.7e-7 apart at a largest value of 2.7e-2).  So the deterministic facts are asserted exactly - not one launch or allocation more - and the gradients
    to the bound tests/test_gpu_train.py holds two eager runs of one step to (cosine > 0.9995, largest difference below
    1e-1 of the largest value).
    (b) the gradient of x_enc at weight w minus the one at weight 0, read from the engine's gradient book, equals w x the
    operator's gradient on the captured x_enc, to the fp32 bound.  The run-to-run difference of the rest of the head's
    backward is about 1e-5 of ITS gradient; w = 1e4 keeps that far below the bound (measured: 5.4e-8).
    (c) the step's scalars equal the operator's on the captured x_enc."""
    m, tr_plain, batch, order, inj = _train_fixture()
    _, Trainer = need_gpu()
    x, sem, ins, n = batch
    real_lib = m.engine.lib

    def step(tr):
        m.head.baseline = None
        cap, log = {}, []
        m.engine.lib = _Launches(real_lib, log)
        try:
            out = tr.forward_backward(*batch, selected_idx=order, injected_s_t=inj, capture=cap)
        finally:
            m.engine.lib = real_lib
        torch.cuda.synchronize()
        gx, xe = _x_enc_grad(m, cap)
        arena = m.engine.arena
        allocs = [(tuple(t.shape), t.dtype) for t in arena.slots[:arena.cursor]] + [arena.stats_cursor]
        return out, m.store.grad[:m.store.n_train].clone(), gx, xe, log, allocs

    step(tr_plain)                                                        # first sight: one-time set-up calls
    out_p, g_plain, gx_plain, _, log_p, alloc_p = step(tr_plain)
    _, g_plain2, gx_plain2, _, log_p2, alloc_p2 = step(tr_plain)
    print("plain trainer, two runs: parameter gradients bit-equal %s (max diff %.3e of max %.3e), x_enc gradient max diff "
          "%.3e of max %.3e" % (torch.equal(g_plain, g_plain2), float((g_plain - g_plain2).abs().max()),
                                float(g_plain.abs().max()), float((gx_plain - gx_plain2).abs().max()),
                                float(gx_plain.abs().max())))
    assert log_p == log_p2 and alloc_p == alloc_p2 and len(log_p) > 100
    tr0 = Trainer(m, disc_weight=0.0, delta_var=0.5, delta_dist=1.5, disc_norm=2, disc_form='reference')
    out0, g0, gx0, _, log_0, alloc_0 = step(tr0)
    assert "disc" not in out0 and set(out0) == set(out_p)
    assert log_0 == log_p and alloc_0 == alloc_p                         # not one launch or allocation more
    assert not any(name.startswith("isa_disc") or name == "isa_labels_from_planes" for name in log_0)
    cos = float(torch.nn.functional.cosine_similarity(g0.double(), g_plain.double(), dim=0))
    gdiff = float((g0 - g_plain).abs().max() / g_plain.abs().max())
    print("weight 0 vs plain trainer: cosine %.7f, max diff %.3e of the largest gradient" % (cos, gdiff))
    assert cos > 0.9995 and gdiff < 1e-1
    dv, dd = deltas(24, 2)
    trw = Trainer(m, disc_weight=W_DISC, delta_var=dv, delta_dist=dd, disc_norm=2, disc_form='full')
    outw, gw, gxw, x_enc, log_w, _ = step(trw)
    extra = sorted(set(log_w) - set(log_p))
    assert extra == ["isa_disc_assemble", "isa_disc_grad", "isa_disc_hinge", "isa_disc_means", "isa_disc_sums",
                     "isa_labels_from_planes"] and len(log_w) == len(log_p) + 6
    assert set(outw) == set(out_p) | {"disc"} and tuple(outw["disc"].shape) == (8,)
    op = m.discriminative_loss(x_enc, ins, n, delta_var=dv, delta_dist=dd, norm=2, form='full', grad=True)
    want = W_DISC * op["grad"].float().permute(0, 2, 3, 1)
    diff = gxw - gx0
    err = float((diff - want).norm() / want.norm())
    print("x_enc gradient: |w g_disc| %.3e, |g_head| %.3e, (i) vs (ii) rel L2 %.3e (bound %.2e)"
          % (float(want.norm()), float(gx0.norm()), err, TOL_G))
    assert err <= TOL_G
    disc = outw["disc"].cpu()
    for i, key in enumerate(SCALARS):
        ref = float(op[key]) * (W_DISC if key == "loss" else 1.0)
        assert abs(float(disc[i]) - ref) <= TOL_S * abs(ref), (key, float(disc[i]), ref)
    assert 0 < float(disc[5]) <= float(n.sum()) and float(disc[6]) > 0 and float(disc[7]) == 0
    assert float((gw - g0).abs().max()) > 0                               # the loss reaches the parameters


def test_graphed_step_with_the_loss():
    """warm, capture, two replays: the replayed step's `disc` scalars equal an eager step's from the same state (1e-4
    relative: the forward's BatchNorm sums use float atomics, the bound test_gpu_train.py measured for forward scalars);
    a weight changed in the settings buffer reaches the next replay without a re-capture; the loss switched off is another
    graph key."""
    dv, dd = deltas(24, 2)
    m, tr, batch, order, inj = _train_fixture(disc_weight=0.5, delta_var=dv, delta_dist=dd, disc_form='full')
    from test_gpu_train import _restore, _snapshot
    tr.train_step_graphed(*batch, selected_idx=order, injected_s_t=inj)  # warm
    torch.cuda.synchronize()
    snap = _snapshot(m, tr)

    def run(stepfn):
        _restore(m, tr, snap)
        out = stepfn(*batch, selected_idx=order, injected_s_t=inj)
        torch.cuda.synchronize()
        return out["disc"].cpu().clone()

    eager = run(tr.train_step)
    captured = run(tr.train_step_graphed)
    assert [s.get("state") for s in tr._graphs.values()] == ["ready"]
    replay1, replay2 = run(tr.train_step_graphed), run(tr.train_step_graphed)
    assert float(eager[0]) > 0 and float(eager[1]) > 0 and float(eager[2]) > 0
    for name, got in (("capture", captured), ("replay1", replay1), ("replay2", replay2)):
        for i in range(8):
            assert abs(float(got[i]) - float(eager[i])) <= 1e-4 * abs(float(eager[i])), (name, i, got, eager)
    tr.set_disc_weight(1.5)
    tripled = run(tr.train_step_graphed)
    assert len(tr._graphs) == 1
    assert abs(float(tripled[0]) / float(replay2[0]) - 3.0) <= 1e-4
    assert abs(float(tripled[1]) - float(replay2[1])) <= 1e-4 * float(replay2[1])
    m.net.disc.set(0.0)
    _restore(m, tr, snap)
    out = tr.train_step_graphed(*batch, selected_idx=order, injected_s_t=inj)
    torch.cuda.synchronize()
    assert "disc" not in out and len(tr._graphs) == 2
    assert sorted(k[-1] for k in tr._graphs) == [(False, None, None), (True, "full", 2)]
