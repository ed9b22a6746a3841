"""The instance head's forward-only kernels against exact or float64 restatements, at the shapes where they walk.

Entry points: isa_row_argmax (the glimpse point s_t: eval argmax and the training exponential race), isa_pool_target
(pyramid targets and mask_all), isa_concat_aux (mask_all + position code + point marker), isa_onehot_map,
isa_dropout_mask, and the head's eval-mode forward: SpatialAttentionLayer with isa_bn_finalize(stats = NULL) and
HardAttentionLayer with isa_maskbn_finalize(train = 0), followed by the eval s_t (isa_ins_softmax + isa_row_argmax).
Before this file they were checked only through the golden fixtures, which inject s_t and the Dropout2d masks.

A / B are exact: the argmax against torch.argmax (first maximum), the race against the first maximum of alpha / race
divided in fp32 on the CPU (the library builds without fast-math, and HIP divides fp32 correctly rounded by default,
so both sides divide identically), targets against F.max_pool2d, the aux channels against R.position_code plus the pos
scatter of R.up_atten_level, the masks bit for bit.  Every output with a neighbourhood (a channel slice, or the floats
after a flat array) is written into NaN and the neighbours must stay bit-unchanged.

The race's distribution: Pearson's chi-square of the draws against alpha, rejected at p < 1e-6 (CHI2_CRIT, quantiles of
the chi-square distribution), in two settings: a short steep row with two zero bins (2**20 draws from 2**18 rows per
launch) and 65536-pixel instance rows binned into 8 equal-mass bins (4096 draws from 64 launches of 64 rows).  Zero-alpha
bins must stay empty.  test_head_forward_references_reject_bugs (no GPU) shows at the same sample sizes and seeds that
the statistic accepts the exponential race and rejects argmax(alpha / U), argmax(alpha * E), draws in proportion to
alpha**2 and a race row shared by all rows.

C (eval forward) compares with the oracle under Ctx(bn_train=False) at the forward bounds of
test_gpu_head_grads.BOUNDS (fp32; bf16: stored outputs TOL[bf16], the hard-attention layer HA_BF16), with running
statistics away from 0 and 1 so that batch statistics or none at all fail by >= 100x the bound (shown on the CPU).
Errors are printed per tensor (HEADFWD lines, and the _check lines of test_gpu_head_grads).

Measured on MI355X: chi-square 19.7 on the short row (df 13, quantile 52.7), 3.1 on the instance rows (df 7, quantile
40.5), no draw in a zero bin; eval forward fp32 worst 4.0e-7 (SP out / beta, bounds 3e-6 / 5e-6) and 3.0e-7 (HA merge,
bound 2e-6), bf16 2.8e-3 (SP out, TOL 2e-2) and 4.2e-3 (HA, HA_BF16 2e-2) - the 16 x 256 x 256 case needs no wider
bound; eval s_t: no near-tie row in fp32, one of 8 rows in bf16.  All of this file runs in about 10 s.
"""
import ctypes as C
import math
import os
import sys
import types

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

import reseg_ref as R  # noqa: E402
from test_gpu_head_grads import (AT, BOUNDS, HA_BF16, HA_CASES, SP, SP_CASES, _check, _ha_inputs,  # noqa: E402
                                 _ha_params, _ins_alpha, _record, _sp_inputs)
from test_gpu_ops import _gpu, q, rand, to_act  # noqa: E402

gpu = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
NAN = float("nan")
FACTORS = (16, 8, 4, 2, 1)                 # pyramid levels (instance_head.py:27)
ROW_PART = 64 * 4                          # ISA_ROW_CHUNKS * 4 floats of partials per softmax row
EINVAL = -1

# Pearson chi-square quantiles at p = 1e-6 (upper tail) by degrees of freedom
CHI2_CRIT = {7: 40.521831, 13: 52.747068}


def _lib():
    """Device inputs are bound to names before a launch: L.ptr(t.cuda()) would free the temporary (and let the next
    allocation reuse its memory) before the kernel has read it."""
    L = _gpu()[0]
    return L, L.lib()


def _padded(numel, pad=512, dtype=torch.float32, fill=NAN):
    """A flat output of `numel` elements followed by `pad` elements of `fill`: (buffer, view of the first numel)."""
    buf = torch.full((numel + pad,), fill, dtype=dtype, device="cuda")
    return buf, buf[:numel]


def _tail_unchanged(buf, numel, fill=NAN):
    tail = buf[numel:].cpu()
    if math.isnan(fill):
        return bool(torch.isnan(tail).all())
    return bool((tail == fill).all())


def _bits_equal(a, b):
    a, b = a.contiguous().cpu(), b.contiguous().cpu()
    bits = {torch.float32: torch.int32, torch.bfloat16: torch.int16}[a.dtype]
    return torch.equal(a.view(bits), b.view(bits))


# ---------------------------------------------------------------------------------------------------------------------
# A. the glimpse point: isa_row_argmax
# ---------------------------------------------------------------------------------------------------------------------
def first_max(v):
    """Index of the first maximum of each row of a CPU fp32 [n, L] tensor, NaN never chosen (isa_kernels.h); a row
    without a value above -inf gives 0."""
    v = torch.nan_to_num(v, nan=float("-inf"))
    m = v.max(1, keepdim=True).values
    hit = (v == m) & (m > float("-inf"))
    idx = torch.where(hit, torch.arange(v.shape[1]).expand_as(v), torch.full_like(v, v.shape[1], dtype=torch.long))
    out = idx.min(1).values
    return torch.where(out == v.shape[1], torch.zeros_like(out), out)


def _tie_positions(kind, L):
    """Planted equal maxima (the launch: one 1024-thread workgroup per row, thread t reads p = t, t + 1024, ...):
    0: inside one thread's stride, 1: across lanes of one wave (the higher lane holds the lower index), 2: across
    waves (wave 14 against wave 1), 3: p = 0 against p = L - 1."""
    cand = {0: [(5, 1029), (7, 3079)], 1: [(40, 1027), (40, 3)], 2: [(900, 1094), (900, 70)], 3: [(0, L - 1)]}[kind]
    for a, b in cand:
        if max(a, b) < L and a != b:
            return [a, b]
    return [min(L - 1, 1)]


def _argmax_rows(n, L, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(n, L, generator=g)
    for r in range(n):
        kind = (r + L) % 5
        if kind == 4:
            a[r] = 0.0                        # an instance without pixels: alpha = 0 everywhere -> index 0
        else:
            a[r, _tie_positions(kind, L)] = 2.0
    return a


@gpu
@pytest.mark.parametrize("L_", [1, 2, 63, 64, 1023, 1024, 1025, 4097, 65536, 262144])
def test_row_argmax_first_maximum(L_):
    """Eval form (race = NULL) == torch.argmax exactly, n in {1, 3, 32} rows, planted equal maxima in one thread's
    stride, across lanes, across waves and at both ends; all-zero rows give 0."""
    L, lib = _lib()
    for n in (1, 3, 32):
        a = _argmax_rows(n, L_, seed=L_ * 7 + n)
        buf, out = _padded(n, dtype=torch.int32, fill=-7)
        ad = a.cuda()
        L.check(lib.isa_row_argmax(L.ptr(ad), None, n, L_, L.ptr(out), L.stream_ptr()), "isa_row_argmax")
        got = out.cpu().long()
        assert torch.equal(got, torch.argmax(a, 1)), (n, L_, got.tolist()[:8])
        assert torch.equal(got, first_max(a))
        assert _tail_unchanged(buf, n, fill=-7)


@gpu
def test_row_argmax_nan_contract():
    """NaN never wins (a 0/0 of the race cannot be drawn); a row without any value above -inf gives 0, never an
    index outside [0, L) (it gave 2**31 - 1, which isa_head_loss then read alpha at).  L = 0 is refused."""
    L, lib = _lib()
    n, L_ = 4, 3000
    a = torch.rand(n, L_)
    a[0, 10] = NAN                              # NaN ahead of the maximum
    a[0, 2000] = 5.0
    a[1] = NAN                                  # all NaN
    a[2] = float("-inf")                        # all -inf
    a[3, :] = NAN
    a[3, 2999] = 0.25                           # one number among NaN
    out = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ad = a.cuda()
    L.check(lib.isa_row_argmax(L.ptr(ad), None, n, L_, L.ptr(out), L.stream_ptr()), "isa_row_argmax")
    assert out.cpu().tolist() == [2000, 0, 0, 2999]
    assert torch.equal(out.cpu().long(), first_max(a))
    assert lib.isa_row_argmax(L.ptr(ad), None, n, 0, L.ptr(out), L.stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [2000, 0, 0, 2999]


@gpu
@pytest.mark.parametrize("n,L_", [(3, 1025), (32, 4097), (16, 65536), (2, 262144)])
def test_row_argmax_race_matches_fp32_division(n, L_):
    """Training form: the first maximum of alpha / race, race = Exp(1) draws made exactly as instance_head.py makes
    them, divided in fp32 on the CPU from the same tensors.  Planted: alpha = 0 beside tiny race values (1e-30), race =
    +inf on the largest alphas, and instance-like rows with alpha = 0 on most pixels.  Zero-alpha pixels never win."""
    L, lib = _lib()
    g = torch.Generator().manual_seed(n * 31 + L_)
    a = torch.rand(n, L_, generator=g) ** 3
    a[:, ::3] = 0.0
    a = a / a.sum(1, keepdim=True)
    torch.manual_seed(1000 + L_)
    race = torch.empty(n, L_, dtype=torch.float32, device="cuda").exponential_(1.0)
    rc = race.cpu()
    for r in range(n):
        if r % 3 == 0:                         # alpha = 0 beside a tiny race value: 0 / 1e-30 = 0 must not win
            zero = torch.nonzero(a[r] == 0)[:64, 0]
            rc[r, zero] = 1e-30
        elif r % 3 == 1:                       # race = +inf on the largest alphas: alpha / inf = 0
            top = torch.topk(a[r], min(8, L_)).indices
            rc[r, top] = float("inf")
        else:                                  # an instance of ~1/16 of the row
            keep = torch.zeros(L_, dtype=torch.bool)
            keep[L_ // 3:L_ // 3 + max(1, L_ // 16)] = True
            a[r] = torch.where(keep, a[r] + 1e-3, torch.zeros(()))
    race = rc.cuda()
    ad = a.cuda()
    buf, out = _padded(n, dtype=torch.int32, fill=-7)
    L.check(lib.isa_row_argmax(L.ptr(ad), L.ptr(race), n, L_, L.ptr(out), L.stream_ptr()), "isa_row_argmax(race)")
    got = out.cpu().long()
    ref = first_max(a / rc)                    # fp32 on the CPU, IEEE division
    assert torch.equal(got, ref), [(r, int(got[r]), int(ref[r])) for r in range(n) if got[r] != ref[r]][:5]
    assert bool((a[torch.arange(n), got] > 0).all()), "a zero-alpha pixel won the race"
    assert _tail_unchanged(buf, n, fill=-7)


# ---- the race's distribution --------------------------------------------------------------------------------------
SHORT_L, SHORT_ROWS, SHORT_LAUNCHES, SHORT_SEED = 16, 1 << 18, 4, 51
LONG_H, LONG_ROWS, LONG_LAUNCHES, LONG_SEED, LONG_BINS = 256, 64, 64, 52, 8


def short_alpha():
    """A steep profile 0.6**k over 16 pixels with zero bins at 3 and 11 (fp32, normalised)."""
    a = torch.tensor([0.6 ** k for k in range(SHORT_L)], dtype=torch.float64)
    a[3] = a[11] = 0.0
    return (a / a.sum()).float()


def long_alpha():
    """An instance-like alpha over 256 x 256 pixels: a softmax of a smooth field over an elliptic instance (~15 k
    pixels), 0 outside.  Returns (alpha [65536] fp32, bin of every pixel: 0..7 equal-mass contiguous runs, 8 = zero)."""
    yy, xx = torch.meshgrid(torch.arange(LONG_H, dtype=torch.float64), torch.arange(LONG_H, dtype=torch.float64),
                            indexing="ij")
    inside = ((yy - 100) / 60) ** 2 + ((xx - 140) / 80) ** 2 < 1
    z = 3 * torch.cos(xx / 17) + 2 * torch.sin(yy / 23)
    a = torch.softmax(z.masked_fill(~inside, float("-inf")).reshape(-1), 0).float()
    a64 = a.double()
    before = torch.cumsum(a64, 0) - a64
    bins = torch.clamp((before / a64.sum() * LONG_BINS).floor().long(), 0, LONG_BINS - 1)
    bins[a == 0] = LONG_BINS
    return a, bins


def chi2(counts, probs):
    """Pearson's statistic over the bins with probability > 0: (statistic, degrees of freedom, draws in zero bins)."""
    counts, probs = counts.double(), probs.double()
    N = float(counts.sum())
    nz = probs > 0
    exp = probs[nz] / probs[nz].sum() * N
    stat = float(((counts[nz] - exp) ** 2 / exp).sum())
    return stat, int(nz.sum()) - 1, int(counts[~nz].sum())


def short_counts(draw):
    """Bin counts of the short setting; draw(alpha [rows, 16], launch) -> [rows] indices."""
    a = short_alpha()
    counts = torch.zeros(SHORT_L, dtype=torch.long)
    for k in range(SHORT_LAUNCHES):
        counts += torch.bincount(draw(a, k).long().cpu(), minlength=SHORT_L)
    return counts, a


def long_counts(draw):
    a, bins = long_alpha()
    counts = torch.zeros(LONG_BINS + 1, dtype=torch.long)
    for k in range(LONG_LAUNCHES):
        s = draw(a, k).long().cpu()
        counts += torch.bincount(bins[s], minlength=LONG_BINS + 1)
    probs = torch.zeros(LONG_BINS + 1, dtype=torch.float64).index_add_(0, bins, a.double())
    return counts, probs


def _gpu_race_draw(rows, seed):
    L, lib = _lib()

    def draw(a, k):
        ad = a.reshape(1, -1).expand(rows, -1).contiguous().cuda()
        torch.manual_seed(seed * 1000 + k)
        race = torch.empty(rows, ad.shape[1], dtype=torch.float32, device="cuda").exponential_(1.0)
        out = torch.empty(rows, dtype=torch.int32, device="cuda")
        L.check(lib.isa_row_argmax(L.ptr(ad), L.ptr(race), rows, ad.shape[1], L.ptr(out), L.stream_ptr()),
                "isa_row_argmax(race)")
        return out
    return draw


def _accept(tag, counts, probs):
    stat, df, zero = chi2(counts, probs)
    print("HEADFWD chi2 %-28s stat %8.2f  df %d  crit(p=1e-6) %.2f  zero-bin draws %d" % (tag, stat, df, CHI2_CRIT[df], zero))
    return stat, df, zero


@gpu
def test_race_distribution_short_steep_row():
    """2**20 race draws over a 16-pixel row 0.6**k with two zero bins: chi-square vs alpha below the p = 1e-6 quantile
    (df 13), zero bins never drawn."""
    counts, a = short_counts(_gpu_race_draw(SHORT_ROWS, SHORT_SEED))
    stat, df, zero = _accept("short row (GPU)", counts, a)
    assert zero == 0, counts.tolist()
    assert stat < CHI2_CRIT[df], (stat, counts.tolist())


@gpu
def test_race_distribution_instance_rows():
    """4096 race draws over a 65536-pixel instance row, 8 equal-mass bins: chi-square vs alpha below the p = 1e-6
    quantile (df 7), no draw outside the instance.  Every launch's 64 rows share alpha: a race row reused by all rows
    would clump the counts by 64 and fail."""
    counts, probs = long_counts(_gpu_race_draw(LONG_ROWS, LONG_SEED))
    stat, df, zero = _accept("instance rows (GPU)", counts, probs)
    assert zero == 0, counts.tolist()
    assert stat < CHI2_CRIT[df], (stat, counts.tolist())


@gpu
def test_training_draws_differ_between_rows_and_forwards():
    """Engine level: a training forward with sampling on over two identical images (same alpha in both rows of an
    iteration, the iterations batched into one race).  The draws are inside the selected instance and not the same
    for the two images, nor the same from one forward to the next: a race that is reused or broadcast would be."""
    _gpu()
    from isa_amd.reseg import ReSeg
    sd = R.synth_state_dict(23, True)
    x, sem, ins, nins = R.synth_batch(1, 64, 64, seed=3)
    x, sem, ins, nins = (t.repeat(2, *([1] * (t.dim() - 1))) for t in (x, sem, ins, nins))
    sel = [list(range(int(nins[0]))) for _ in range(2)]
    model = ReSeg(2, True, dtype=torch.float32)
    model.load_state_dict(sd)
    model.train()
    model.head.drop_rate = 0.0
    assert model.head.sample_in_training
    draws = []
    for step in range(4):
        torch.manual_seed(100 + step)
        model(True, x, sem, ins, nins, selected_idx=sel)
        rec = model.last_record
        torch.cuda.synchronize()
        st = torch.stack([it["s_t"].cpu().long() for it in rec["iters"]])          # [iteration, image]
        assert st.shape == (rec["max_iter"], 2)
        for it in range(st.shape[0]):
            plane = ins[0, sel[0][it]].reshape(-1)
            assert bool((plane[st[it]] != 0).all()), ("draw outside the instance", step, st.tolist())
        draws.append(st)
    d = torch.stack(draws)                                                      # [step, iteration, image]
    same_pair = int((d[..., 0] == d[..., 1]).sum())
    print("HEADFWD engine draws %s; identical image pairs %d of %d" % (d.tolist(), same_pair, d[..., 0].numel()))
    assert same_pair <= 2, d.tolist()
    assert not all(torch.equal(d[0], d[k]) for k in range(1, len(d))), d.tolist()


# ---------------------------------------------------------------------------------------------------------------------
# B. targets, position codes, masks
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("f", FACTORS)
def test_pool_target_instance_planes(f):
    """Instance-plane form, batched [iteration][image] rows: n = 6 rows over nsrc = 3 images, idx per row;
    == F.max_pool2d of the selected plane."""
    L, lib = _lib()
    nsrc, nobj, n, H, W = 3, 5, 6, 48, 32
    g = torch.Generator().manual_seed(f)
    owner = torch.randint(0, nobj + 2, (nsrc, H, W), generator=g)              # >= nobj: background
    ins = torch.stack([(owner == k) for k in range(nobj)], 1).long()
    ins[1, 4] = 0                                                               # an empty instance
    idx = torch.tensor([0, 4, 2, 3, 4, 1], dtype=torch.int32)
    h, w = H // f, W // f
    buf, out = _padded(n * h * w)
    ins_d, idx_d = ins.cuda(), idx.cuda()
    L.check(lib.isa_pool_target(L.ptr(ins_d), L.ptr(idx_d), None, nobj, n, H, W, f, L.ptr(out), nsrc,
                                L.stream_ptr()), "isa_pool_target")
    planes = torch.stack([ins[b % nsrc, int(idx[b])] for b in range(n)]).float()[:, None]
    ref = F.max_pool2d(planes, f)[:, 0] if f > 1 else planes[:, 0]
    assert torch.equal(out.view(n, h, w).cpu(), ref)
    assert _tail_unchanged(buf, n * h * w)


@gpu
@pytest.mark.parametrize("f", FACTORS)
@pytest.mark.parametrize("nsrc", [2, 4])
def test_pool_target_fp32_map(f, nsrc):
    """fp32-map form (mask_all): negative values included, so the maximum must start from -inf; == F.max_pool2d."""
    L, lib = _lib()
    n, H, W = 4, 32, 48
    src = rand(nsrc, H, W, seed=f) - 3.0                                        # mostly negative
    src[0, :16, :16] = -1e30
    h, w = H // f, W // f
    buf, out = _padded(n * h * w)
    src_d = src.cuda()
    L.check(lib.isa_pool_target(None, None, L.ptr(src_d), 0, n, H, W, f, L.ptr(out), nsrc, L.stream_ptr()),
            "isa_pool_target(map)")
    planes = torch.stack([src[b % nsrc] for b in range(n)])[:, None]
    ref = F.max_pool2d(planes, f)[:, 0] if f > 1 else planes[:, 0]
    assert torch.equal(out.view(n, h, w).cpu(), ref)
    assert _tail_unchanged(buf, n * h * w)


@gpu
def test_pool_target_refusals():
    """H % f != 0, W % f != 0 and n % nsrc != 0 are refused before any launch: the output stays untouched."""
    L, lib = _lib()
    src = torch.zeros(4, 32, 32, device="cuda")
    buf, out = _padded(64)
    for H, W, f, n, nsrc in ((24, 32, 16, 4, 4), (32, 24, 16, 4, 4), (32, 32, 8, 4, 3), (32, 32, 3, 4, 4)):
        rc = lib.isa_pool_target(None, None, L.ptr(src), 0, n, H, W, f, L.ptr(out), nsrc, L.stream_ptr())
        assert rc == EINVAL, (H, W, f, n, nsrc, rc)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


def position_code(rows, cols, f, lsb_first=False, swap=False):
    """R.position_code restated with one switchable bug each: lsb_first = the code bits LSB first, swap = the row and
    column bits exchanged.  Checked against R.position_code (as written) in test_head_forward_references_reject_bugs."""
    nb = int(round(math.log2(f)))
    codes = []
    for r, c in zip(rows, cols):
        rr, cc = (c % f, r % f) if swap else (r % f, c % f)
        order = range(nb) if lsb_first else range(nb - 1, -1, -1)
        codes.append([(rr >> k) & 1 for k in order] + [(cc >> k) & 1 for k in order])
    return [r // f for r in rows], [c // f for c in cols], codes


def aux_expected(mask_all, s_t, H, W, f, mask_n, code=R.position_code):
    """isa_concat_aux's channels [mask_all | 2 nb code bits | marker] of every row: mask_all of image b % mask_n, then
    the pos tensor of R.up_atten_level (the code bits and the marker at the coarse cell of s_t, 0 elsewhere)."""
    n, h, w = s_t.numel(), H // f, W // f
    nb = int(round(math.log2(f)))
    rows, cols = [int(s) // W for s in s_t], [int(s) % W for s in s_t]
    pr, pc, codes = code(rows, cols, f)
    out = torch.zeros(n, h, w, 2 * nb + 2)
    out[..., 0] = mask_all[torch.arange(n) % mask_n]
    bi, pr, pc = torch.arange(n), torch.tensor(pr), torch.tensor(pc)
    out[bi, pr, pc, 2 * nb + 1] = 1.0
    if nb:
        out[bi, pr, pc, 1:2 * nb + 1] = torch.tensor(codes, dtype=torch.float32)
    return out


AUX_H, AUX_W, AUX_MASK_N = 32, 48, 3          # full-resolution sweep map; rows share mask_all modulo 3


def aux_inputs(f):
    n = AUX_H * AUX_W                                             # one row per full-resolution position
    s_t = torch.randperm(n, generator=torch.Generator().manual_seed(f)).to(torch.int32)
    g = torch.Generator().manual_seed(100 + f)
    mask_all = torch.randint(0, 9, (AUX_MASK_N, AUX_H // f, AUX_W // f), generator=g).float() / 8   # bf16-exact
    return s_t, mask_all


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("f", FACTORS)
def test_concat_aux_position_code(dtype, f):
    """Every full-resolution position of a 32 x 48 map as s_t (one row each, 1536 rows sharing mask_all over 3
    images), written into a channel slice of a wider NaN buffer as level_main does; == aux_expected exactly."""
    L, lib = _lib()
    nb = int(round(math.log2(f)))
    naux = 2 * nb + 2
    s_t, mask_all = aux_inputs(f)
    n, h, w = s_t.numel(), AUX_H // f, AUX_W // f
    c0 = 5
    ld = c0 + naux + 3
    buf = torch.full((n, h, w, ld), NAN, dtype=dtype, device="cuda")
    orig = buf.clone()
    t = L.IsaTensor(buf.data_ptr() + c0 * buf.element_size(), n, h, w, naux, ld, L.dtype_code(dtype), 1)
    mask_d, s_t_d = mask_all.cuda(), s_t.cuda()
    L.check(lib.isa_concat_aux(C.byref(t), L.ptr(mask_d), L.ptr(s_t_d), AUX_W, f, nb, AUX_MASK_N, L.stream_ptr()),
            "isa_concat_aux")
    got = buf.cpu()
    ref = aux_expected(mask_all, s_t, AUX_H, AUX_W, f, AUX_MASK_N)
    assert torch.equal(got[..., c0:c0 + naux].float(), ref), int((got[..., c0:c0 + naux].float() != ref).sum())
    assert _bits_equal(got[..., :c0], orig[..., :c0]) and _bits_equal(got[..., c0 + naux:], orig[..., c0 + naux:])


@gpu
def test_onehot_map():
    """argmax(1) of the int64 2-class one-hot, all four pixel kinds including (0,0) and (1,1) -> 0 (first maximum);
    n * hw = 600 002 elements: more than the 2048-workgroup grid cap covers in one sweep."""
    L, lib = _lib()
    for n, hw in ((3, 1000), (2, 300001)):
        g = torch.Generator().manual_seed(hw)
        oh = torch.randint(0, 2, (n, 2, hw), generator=g)
        oh[0, :, :4] = torch.tensor([[0, 1, 0, 1], [0, 0, 1, 1]])
        buf, out = _padded(n * hw)
        oh_d = oh.cuda()
        L.check(lib.isa_onehot_map(L.ptr(oh_d), n, hw, L.ptr(out), L.stream_ptr()), "isa_onehot_map")
        assert torch.equal(out.cpu(), oh.argmax(1).float().reshape(-1))
        assert out[:4].cpu().tolist() == [0.0, 0.0, 1.0, 0.0]
        assert _tail_unchanged(buf, n * hw)


@gpu
@pytest.mark.parametrize("keep", [0.5, 0.9, 1.0])
def test_dropout_mask_bit_exact(keep):
    """(u < keep) / keep bit for bit in fp32, with u == keep, u at the float just below keep, 0 and the largest float
    below 1; sizes not multiples of 256 and past the 256-workgroup grid cap."""
    L, lib = _lib()
    k32 = torch.tensor(keep, dtype=torch.float32)
    below = torch.nextafter(k32, torch.tensor(0.0))
    for n in (1, 255, 1000, 65537, 1000003):
        u = torch.rand(n, generator=torch.Generator().manual_seed(n))
        plant = torch.stack([k32, below, torch.tensor(0.0), torch.nextafter(torch.tensor(1.0), torch.tensor(0.0))])
        m = min(n, 4)
        u[:m] = plant[:m]
        if n > 8:
            u[n - 4:] = plant
        buf, out = _padded(n)
        u_d = u.cuda()
        L.check(lib.isa_dropout_mask(L.ptr(u_d), n, keep, L.ptr(out), L.stream_ptr()), "isa_dropout_mask")
        ref = torch.where(u < k32, torch.ones(()) / k32, torch.zeros(()))
        assert _bits_equal(out, ref), (keep, n)
        assert _tail_unchanged(buf, n)
        if n >= 4:
            assert out[:2].cpu().tolist() == [0.0, float(torch.ones(()) / k32)]     # u == keep drops, just below keeps


# ---------------------------------------------------------------------------------------------------------------------
# C. the head's forward in eval mode (running statistics)
# ---------------------------------------------------------------------------------------------------------------------
def eval_running(P, pre, c, seed):
    """Running statistics away from 0 and 1 (an untrained layer's defaults): |mean| in [0.3, 0.8], var in [1.6, 3.2]."""
    g = torch.Generator().manual_seed(seed)
    sign = torch.where(torch.rand(c, generator=g) < 0.5, -1.0, 1.0)
    P[pre + ".running_mean"] = sign * (0.3 + 0.5 * torch.rand(c, generator=g))
    P[pre + ".running_var"] = 1.6 + 1.6 * torch.rand(c, generator=g)
    return P


def _eval_engine(P, dtype):
    L, Act, Engine, ParamStore, Pro = _gpu()
    schema = [(k, tuple(v.shape)) for k, v in P.items()]
    schema += [(k.replace("running_mean", "num_batches_tracked"), ()) for k in P if k.endswith("running_mean")]
    ps = ParamStore(schema, "cuda")
    ps.load_state_dict(P)
    eng = Engine(ps, dtype)
    eng.begin(bn_train=False, record=False)
    from isa_amd.instance_head import InstanceHead
    return eng, ps, InstanceHead(types.SimpleNamespace(E=eng))


def _snapshot(ps, P):
    run = {k: ps.view(k).detach().cpu().clone() for k in P if "running" in k}
    nbt = {k: v for k, v in ps.int_buffers.items()}
    return run, nbt


def _assert_state_unchanged(ps, P, before):
    run, nbt = _snapshot(ps, P)
    for k, v in before[0].items():
        assert _bits_equal(run[k], v), "eval changed " + k
    assert nbt == before[1], "eval changed num_batches_tracked"


def sp_eval_reference(x, sem, P, dtype, bn_train=False):
    P64 = {k: v.double() for k, v in P.items()}
    for k in [k for k in P if k.endswith("running_mean")]:
        P64[k.replace("running_mean", "num_batches_tracked")] = torch.zeros((), dtype=torch.long)
    ctx = R.Ctx(bn_train=bn_train, capture=True)
    out = R.spatial_attention(P64, q(x, dtype).double(), sem.double()[:, None], ctx)
    return out, ctx.taps["s_sp.beta"][:, 0]


def ha_eval_reference(s, sem, P, dtype, bn_train=False):
    P64 = {k: v.double() for k, v in P.items()}
    for k in [k for k in P if k.endswith("running_mean")]:
        P64[k.replace("running_mean", "num_batches_tracked")] = torch.zeros((), dtype=torch.long)
    n, _, H, W = s.shape
    _, merge = R.hard_attention(P64, q(s, dtype).double(), sem.double()[:, None],
                                torch.ones(n, 1, H, W, dtype=torch.float64), R.Ctx(bn_train=bn_train))
    return merge[:, 0]


SP_EVAL_CASES = [c[:4] for c in SP_CASES] + [(16, 24, 256, 256)]     # + the production shape: chunked row softmaxes
HA_EVAL_CASES = [c[:4] for c in HA_CASES] + [(16, 256, 256, None)]


def sp_eval_inputs(n, C, H, W):
    x, sem, _, P = _sp_inputs(n, C, H, W, None)
    return x, sem, eval_running(P, SP + ".bn", C, seed=C + H)


def ha_eval_inputs(n, H, W, empty):
    s, sem, _ = _ha_inputs(n, H, W, empty)
    return s, sem, eval_running(_ha_params(), AT + ".bn", 1, seed=H + W)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,C,H,W", SP_EVAL_CASES)
def test_spatial_attention_eval(dtype, n, C, H, W):
    """SpatialAttentionLayer in eval mode (isa_bn_finalize with stats = NULL: running statistics) vs R.spatial_attention
    under Ctx(bn_train=False) in float64: out and beta at the forward bounds; running statistics and
    num_batches_tracked bit-unchanged."""
    L, Act, *_ = _gpu()
    x, sem, P = sp_eval_inputs(n, C, H, W)
    eng, ps, head = _eval_engine(P, dtype)
    before = _snapshot(ps, P)
    maps = _record(eng, "f32")
    out = head.spatial_attention(to_act(Act, x, dtype), sem.reshape(n, -1).float().cuda().contiguous())
    del eng.f32
    beta = maps[0]                      # spatial_attention's first fp32 map is beta (instance_head.py:84)
    got_out, got_beta = out.nchw().cpu(), beta.view(n, H, W).float().cpu()
    torch.cuda.synchronize()
    ref_out, ref_beta = sp_eval_reference(x, sem, P, dtype)
    _check("sp eval n%d C%d %dx%d %s" % (n, C, H, W, str(dtype)[6:]), "sp", dtype,
           dict(out=(got_out, ref_out), beta=(got_beta, ref_beta)))
    _assert_state_unchanged(ps, P, before)


def _ins_planes_in(sem, nobj, seed):
    """[n, nobj, L] int64 instance planes inside the foreground: every foreground pixel belongs to one of nobj."""
    n = sem.shape[0]
    g = torch.Generator().manual_seed(seed)
    owner = torch.randint(0, nobj, sem.reshape(n, -1).shape, generator=g)
    fg = sem.reshape(n, -1) > 0.5
    return torch.stack([(owner == k) & fg for k in range(nobj)], 1).long()


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,H,W,empty", HA_EVAL_CASES)
def test_hard_attention_eval_and_glimpse(dtype, n, H, W, empty):
    """HardAttentionLayer in eval mode (isa_maskbn_finalize with train = 0: running statistics) vs R.hard_attention
    under Ctx(bn_train=False): merge at the forward bound; running statistics and num_batches_tracked bit-unchanged.
    Then the eval glimpse point of two decoder iterations - isa_ins_softmax of the product's merge, then
    isa_row_argmax - against the first maximum of the float64 instance softmax: exact, except where the two top
    pixels are within the merge bound of each other (fp32: at most one such row, as assert_index_map allows)."""
    L, Act, *_ = _gpu()
    lib = L.lib()
    s, sem, P = ha_eval_inputs(n, H, W, empty)
    eng, ps, head = _eval_engine(P, dtype)
    before = _snapshot(ps, P)
    merge = head.hard_attention_scores(to_act(Act, s, dtype), sem.reshape(n, -1).float().cuda().contiguous())
    merge_f = merge.view(n, H, W).cpu().clone()
    ref = ha_eval_reference(s, sem, P, dtype)
    _check("ha eval n%d %dx%d empty%s %s" % (n, H, W, empty, str(dtype)[6:]), "ha", dtype, dict(merge=(merge_f, ref)))
    if empty is not None:
        assert float(merge_f[empty].abs().max()) == 0.0
    _assert_state_unchanged(ps, P, before)
    # the eval glimpse point (the per-iteration path of InstanceHead.forward)
    nobj, Lp = 4, H * W
    ins = _ins_planes_in(sem, nobj, seed=n + H)
    bound = HA_BF16 if dtype == torch.bfloat16 else BOUNDS["ha"]["merge"]
    scale = float(ref.abs().max())
    near = 0
    for it in range(2):
        idx = torch.tensor([(b + it) % nobj for b in range(n)], dtype=torch.int32)
        # every buffer the launches read or write stays referenced until the synchronize (they run on eng.st())
        bufs = dict(ins=ins.cuda(), idx=idx.cuda(), alpha=torch.full((n * Lp,), NAN, device="cuda"),
                    rowstat=torch.empty(2 * n, device="cuda"), part=torch.empty(n * ROW_PART, device="cuda"),
                    s_t=torch.full((n,), -7, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        L.check(lib.isa_ins_softmax(L.ptr(merge), L.ptr(bufs["ins"]), L.ptr(bufs["idx"]), n, nobj, Lp,
                                    L.ptr(bufs["alpha"]), L.ptr(bufs["rowstat"]), n, L.ptr(bufs["part"]), eng.st()),
                "isa_ins_softmax")
        L.check(lib.isa_row_argmax(L.ptr(bufs["alpha"]), None, n, Lp, L.ptr(bufs["s_t"]), eng.st()), "isa_row_argmax")
        torch.cuda.synchronize()
        got = bufs["s_t"].cpu().long()
        planes = torch.stack([ins[b, int(idx[b])] for b in range(n)]).bool()
        ref_alpha = _ins_alpha(ref.reshape(n, -1), planes)
        want = torch.argmax(ref_alpha, 1)
        for b in range(n):
            if int(got[b]) == int(want[b]):
                continue
            assert bool(planes[b, got[b]]), ("s_t outside the instance", it, b)
            m = ref.reshape(n, -1)[b]
            margin = float(m[want[b]] - m[got[b]])
            assert margin <= 2 * bound * scale, ("eval s_t differs beyond a near-tie", it, b, margin, bound * scale)
            near += 1
    print("HEADFWD ha eval s_t n%d %dx%d %s: near-tie rows %d of %d" % (n, H, W, str(dtype)[6:], near, 2 * n))
    if dtype == torch.float32:
        assert near <= 1


# ---------------------------------------------------------------------------------------------------------------------
# E. the references and bounds reject plausible bugs (no GPU)
# ---------------------------------------------------------------------------------------------------------------------
def _cpu_race(exp_fn, rows, seed, support=None):
    """argmax(alpha / race) on the CPU with race = exp_fn(generator, shape); `support`: the only pixels that can win
    (alpha > 0), so that a 65536-pixel row needs random numbers for its ~15 k instance pixels only."""
    def draw(a, k):
        g = torch.Generator().manual_seed(seed * 1000 + k)
        cols = support if support is not None else torch.arange(a.numel())
        r = exp_fn(g, (rows, cols.numel()))
        return cols[torch.argmax(a[cols][None, :] / r, 1)]
    return draw


def _exp(g, shape):
    return torch.empty(shape).exponential_(1.0, generator=g)


def _unif(g, shape):
    return torch.rand(shape, generator=g).clamp_min(1e-30)


def _inv_exp(g, shape):                # argmax(alpha * E) = argmax(alpha / (1 / E))
    return 1.0 / torch.empty(shape).exponential_(1.0, generator=g)


def _squared(rows, seed):
    def draw(a, k):
        return torch.multinomial(a.double() ** 2, rows, replacement=True,
                                 generator=torch.Generator().manual_seed(seed * 1000 + k))
    return draw


def _broadcast(rows, seed, support):
    """The correct race, but one race row for all rows of a launch."""
    one = _cpu_race(_exp, 1, seed, support)
    return lambda a, k: one(a, k).expand(rows)


def test_head_forward_references_reject_bugs():
    """Each reference or bound of this file fails a plausible bug.

    * Chi-square, at the GPU tests' sample sizes and seeds: the exponential race is accepted in both settings;
      argmax(alpha / U), argmax(alpha * E) and draws in proportion to alpha**2 are rejected on the short steep row, and
      alpha * E, alpha**2 and one race row shared by every row of a launch on the instance rows.  (alpha / U is not
      separable on a 65536-pixel row: the maximum lies in the tail of 1 / U, where P(alpha / U > t) = alpha / t is
      proportional to alpha, so its bias is of the order of max alpha ~ 1e-3.)
    * The position code: with the row and column bits exchanged the aux channels differ at every level with nb >= 1,
      with the bits LSB first at every level with nb >= 2 (one bit has no order).
    * The eval forward with batch statistics in place of the running ones moves SP's out and HA's merge by >= 100x
      the fp32 bound (beta comes before the BatchNorm)."""
    a_long, _ = long_alpha()
    support = torch.nonzero(a_long > 0)[:, 0]
    short = {"race": _cpu_race(_exp, SHORT_ROWS, SHORT_SEED), "alpha/U": _cpu_race(_unif, SHORT_ROWS, SHORT_SEED),
             "alpha*E": _cpu_race(_inv_exp, SHORT_ROWS, SHORT_SEED), "alpha^2": _squared(SHORT_ROWS, SHORT_SEED)}
    for name, draw in short.items():
        counts, probs = short_counts(draw)
        stat, df, zero = _accept("short row, %s (CPU)" % name, counts, probs)
        if name == "race":
            assert stat < CHI2_CRIT[df] and zero == 0
        else:
            assert stat > 10 * CHI2_CRIT[df], (name, stat)
    long = {"race": _cpu_race(_exp, LONG_ROWS, LONG_SEED, support), "alpha/U": _cpu_race(_unif, LONG_ROWS, LONG_SEED, support),
            "alpha*E": _cpu_race(_inv_exp, LONG_ROWS, LONG_SEED, support), "alpha^2": _squared(LONG_ROWS, LONG_SEED),
            "shared race row": _broadcast(LONG_ROWS, LONG_SEED, support)}
    for name, draw in long.items():
        counts, probs = long_counts(draw)
        stat, df, zero = _accept("instance rows, %s (CPU)" % name, counts, probs)
        if name == "race":
            assert stat < CHI2_CRIT[df] and zero == 0
        elif name != "alpha/U":
            assert stat > 2 * CHI2_CRIT[df], (name, stat)

    # position code: the restatement is the oracle's, and each bug changes the aux channels
    for f in FACTORS:
        s_t, mask_all = aux_inputs(f)
        rows, cols = [int(s) // AUX_W for s in s_t], [int(s) % AUX_W for s in s_t]
        assert tuple(position_code(rows, cols, f)) == tuple(R.position_code(rows, cols, f))
        good = aux_expected(mask_all, s_t, AUX_H, AUX_W, f, AUX_MASK_N)
        assert torch.equal(good, aux_expected(mask_all, s_t, AUX_H, AUX_W, f, AUX_MASK_N, code=position_code))
        nb = int(round(math.log2(f)))
        for bug, min_nb in (("swap", 1), ("lsb_first", 2)):
            bad = aux_expected(mask_all, s_t, AUX_H, AUX_W, f, AUX_MASK_N,
                               code=lambda r, c, f_, b=bug: position_code(r, c, f_, **{b: True}))
            differs = not torch.equal(good, bad)
            print("HEADFWD position code f=%d %-9s differs: %s" % (f, bug, differs))
            assert differs == (nb >= min_nb), (f, bug)

    # eval forward: batch statistics instead of the running ones
    n, C, H, W = SP_EVAL_CASES[0]
    x, sem, P = sp_eval_inputs(n, C, H, W)
    out_r, beta_r = sp_eval_reference(x, sem, P, torch.float32)
    out_b, beta_b = sp_eval_reference(x, sem, P, torch.float32, bn_train=True)
    d = float((out_b - out_r).abs().max() / out_r.abs().max())
    print("HEADFWD sp eval with batch statistics: out moves %.2e (bound %.0e)" % (d, BOUNDS["sp"]["out"]))
    assert d >= 100 * BOUNDS["sp"]["out"]
    n, H, W, empty = HA_EVAL_CASES[1]
    s, sem, P = ha_eval_inputs(n, H, W, empty)
    m_r = ha_eval_reference(s, sem, P, torch.float32)
    m_b = ha_eval_reference(s, sem, P, torch.float32, bn_train=True)
    d = float((m_b - m_r).abs().max() / m_r.abs().max())
    print("HEADFWD ha eval with batch statistics: merge moves %.2e (bound %.0e)" % (d, BOUNDS["ha"]["merge"]))
    assert d >= 100 * BOUNDS["ha"]["merge"]
