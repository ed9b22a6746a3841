"""The named attention operators (a19-a21: byname_attention.hip through attention_ops.py) OFF the one configuration of
tests/golden/byname_ops.npz: odd and non-square maps, one / two / four heads, d_k != d_v, d_model / n_head != d_k (where
the local logit scale c ** -0.5 differs from d_k ** -0.5), every dilation regime, grid-stride sizes, every flag
combination of the small layers, the raw-score and per-head-mask paths.

Operands are drawn here; the yardstick is the float64 restatement of oracle/byname_ref.py (pinned to the reference's
own classes by tests/test_byname_ref.py) on the STORAGE-ROUNDED operands.  Errors are relative to the reference's
largest element.  fp32 bounds are those test_gpu_byname.py uses for the same operator (1e-5 local core, sdp core and point
query, 2e-5 MultiHeadAttention, 1e-4 ScalePDAttention), bf16 / f16 bounds likewise (2e-2 / 3e-3 sdp core, 3e-2 / 4e-3
MultiHeadAttention, 3e-2 ScalePDAttention); a bound of this file's own says where it comes from.  NaN positions must be
the reference's; results that are exactly zero or exactly beta are compared exactly."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]

import byname_ref as B  # noqa: E402

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import isa_amd  # noqa: F401
    from isa_amd import attention_ops as A
    return A


def rel(got, ref, what=None):
    """max |got - ref| / max |ref| over the non-NaN elements of ref; NaN positions must agree exactly."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), (what, "NaN positions")
    ok = ~torch.isnan(ref)
    if not ok.any():
        return 0.0
    return float((got[ok] - ref[ok]).abs().max() / (ref[ok].abs().max() + 1e-30))


def check(got, ref, tol, what):
    err = rel(got, ref, what)
    print("%-70s err %.3e  bound %.1e" % (what, err, tol))
    assert err < tol, (what, err, tol)


def rounded(t, dtype):
    """The operand as the kernel reads it from `dtype` storage, in float64."""
    return t.to(dtype).double()


def fixture_sd(kind, i):
    z = np.load(os.path.join(ROOT, "tests", "golden", "byname_shapes.npz"))
    pre = "%s%d/sd/" % (kind, i)
    return {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}


# ---------------------------------------------------------------------------------------------------------------------
# whole operators on the fixture's cases (its state_dicts; operands drawn from the cases' seeds)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tol", [(F32, 1e-4), (BF16, 3e-2)])
@pytest.mark.parametrize("i", range(len(B.SPD_CASES)))
def test_scale_pd_attention_cases(i, dtype, tol):
    """ScalePDAttention on every ScalePD case of byname_shapes.npz: c = d_model / n_head of 16, 24, 24, 10 and 10 against
    d_k of 12, 8, 12, 12, 12, so a d_k ** -0.5 scale misses each of them by > 1e-2 (test_byname_ref.py's guard).  The
    library runs all five, d_model = 20 through the zero-padded NHWC path: none is pinned as raising."""
    A = ops()
    dk, dv, dm, G, dil, b, h, w = B.SPD_CASES[i]
    sd = fixture_sd("spd", i)
    qk, v, nomask = B.spd_inputs(i)
    m = A.ScalePDAttention(dk, dv, dm, dil, n_head=G, dtype=dtype).cuda().eval()
    m.load_state_dict(sd)
    out = m(qk.cuda(), v.cuda(), nomask.cuda())
    torch.cuda.synchronize()
    ref = B.scale_pd_attention(sd, rounded(qk, dtype), rounded(v, dtype), nomask, dil)
    check(out, ref, tol, "ScalePDAttention %s %s" % (B.SPD_CASES[i], dtype))


MHA_TOL = {F32: 2e-5, BF16: 3e-2, F16: 4e-3}


def mha_reference(sd, case, q, k, v, mask, dtype):
    G, dm, dk, dv = case[:4]
    # bf16 storage rounds the K / V stream's input once more (the projections run in the storage type); f16 storage
    # projects in fp32 and rounds only the projected rows, like the golden test of test_gpu_byname.py
    kr, vr = (rounded(t, dtype) if dtype == BF16 else t.double() for t in (k, v))
    out, attn = B.multi_head_attention(sd, G, dk, dv, q, kr, vr, mask)
    last, _ = B.multi_head_attention(sd, G, dk, dv, q, kr, vr, mask, last=True)
    return out, attn, last


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
@pytest.mark.parametrize("i", range(len(B.MHA_CASES)))
def test_multi_head_attention_cases(i, dtype):
    """MultiHeadAttention, both branches, on every MHA case of byname_shapes.npz.  Case 0 carries a fully masked row:
    NaN in its attention rows of both heads and in every element of its output row, nowhere else.
    Pinned as raising: case 2 (d_k, d_v = 16, 8) with f16 storage - the streaming kernel reads f16 at the reference's
    head width (12) only; its last=True branch (isa_sdp_scores) serves every width and is compared."""
    A = ops()
    case = B.MHA_CASES[i]
    G, dm, dk, dv, b, lq, L = case
    sd = fixture_sd("mha", i)
    q, k, v, mask = B.mha_inputs(i)
    m = A.MultiHeadAttention(G, dm, dk, dv, dtype=dtype).cuda().eval()
    m.load_state_dict(sd)
    ref_out, ref_attn, ref_last = mha_reference(sd, case, q, k, v, mask, dtype)
    tol = MHA_TOL[dtype]
    last, none = m(q.cuda(), k.cuda(), v.cuda(), mask=mask.cuda(), last=True)
    torch.cuda.synchronize()
    assert none is None
    check(last, ref_last, tol, "MHA last %s %s" % (case, dtype))
    if dtype == F16 and dk != 12:
        with pytest.raises(A.L.IsaError):
            m(q.cuda(), k.cuda(), v.cuda(), mask=mask.cuda())
        return
    out, attn = m(q.cuda(), k.cuda(), v.cuda(), mask=mask.cuda())
    torch.cuda.synchronize()
    if i == 0:
        planted = torch.zeros(b, lq, dtype=torch.bool)
        planted[B.MHA_MASKED_ROW] = True
        assert torch.equal(torch.isnan(ref_out).all(2), planted)
    check(out, ref_out, tol, "MHA out %s %s" % (case, dtype))
    check(attn, ref_attn, tol, "MHA attn %s %s" % (case, dtype))


@pytest.mark.parametrize("G,dm,dk,dv,dtype", [(2, 32, 16, 16, F32), (2, 32, 16, 16, BF16), (2, 24, 12, 8, F32),
                                              (4, 48, 12, 12, F32), (1, 32, 16, 16, F16), (1, 24, 12, 8, F16)])
def test_multi_head_attention_refuses_what_no_kernel_serves(G, dm, dk, dv, dtype):
    """Interleaved heads exist for 2 heads of the reference's width (d_k = d_v = 12) and f16 at that width only: everything
    else must raise, never fall back.  None of these configurations is a fixture case."""
    A = ops()
    assert (G, dm, dk, dv) not in [c[:4] for c in B.MHA_CASES]
    g = torch.Generator().manual_seed(3)
    m = A.MultiHeadAttention(G, dm, dk, dv, dtype=dtype).cuda().eval()
    q, k = torch.randn(2, 2, dm, generator=g).cuda(), torch.randn(2, 130, dm, generator=g).cuda()
    with pytest.raises(A.L.IsaError):
        m(q, k, k, mask=None)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# local dilated attention core
# ---------------------------------------------------------------------------------------------------------------------
LOCAL_SHAPES = [(1, 1, 1, 1, 1, 1), (2, 5, 300, 12, 12, 1), (1, 17, 3, 32, 32, 4), (3, 9, 14, 8, 16, 3), (2, 513, 520, 12, 12, 2)]
# bf16: the reference reads the same rounded operands, so what is left is the fp32 arithmetic (1e-5) and ONE rounding
# of the result to bf16's 8 significant bits: half an ulp, at most 2^-8 = 3.9e-3 of an element (just above a power of two)
BF16_ROUND = 2.0 ** -8 + 1e-5
LOCAL_TOL = {F32: 1e-5, BF16: BF16_ROUND}


def local_reference(Q, K, V, nm, dil, scale, dtype):
    import reseg_ref as R
    # image by image: the float64 stack of nine shifted V maps of the largest case is 230 MB per image
    return torch.cat([R.local_dilated_attention(rounded(Q[i:i + 1], dtype), rounded(K[i:i + 1], dtype), rounded(V[i:i + 1], dtype),
                                                nm[i:i + 1].double(), dil, scale) for i in range(Q.shape[0])])


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("n,h,w,dk,dv,dil", LOCAL_SHAPES)
def test_local_dilated_attention_shapes(n, h, w, dk, dv, dil, dtype):
    """local_dilated_attention: h != w, one pixel, the widest head (32), d_k != d_v, dilation past the map, n = 3; nomask
    absent, random (0.3) and with one image fully masked (its output is exactly 0); the default scale and an explicit one.
    The 2 x 513 x 520 case (533 520 pixels) is the smallest that passes the kernel's grid cap of 2 048 x 256 pixels and
    enters its grid-stride loop; it runs one mask and one scale only (its float64 reference takes about a second)."""
    A = ops()
    g = torch.Generator().manual_seed(n * 1000 + h)
    Q, K, V = (torch.randn(n, c, h, w, generator=g) for c in (dk, dk, dv))
    masks = {"none": torch.zeros(n, 1, h, w), "random": (torch.rand(n, 1, h, w, generator=g) < 0.3).float()}
    masks["image"] = masks["random"].clone()
    masks["image"][n - 1] = 1.0
    big = n * h * w > 100000
    for name, scale in ([("random", None)] if big else itertools.product(("none", "random", "image"), (None, 0.61))):
        nm = masks[name]
        got = A.local_dilated_attention(Q.cuda(), K.cuda(), V.cuda(), nm.cuda(), dil, dtype=dtype, scale=scale)
        torch.cuda.synchronize()
        ref = local_reference(Q, K, V, nm, dil, scale, dtype)
        check(got, ref, LOCAL_TOL[dtype], "local %s %s nomask=%s scale=%s" % ((n, h, w, dk, dv, dil), dtype, name, scale))
        if name == "image":
            assert float(ref[n - 1].abs().max()) == 0.0 and float(got[n - 1].abs().max()) == 0.0
    if not big and dk > 1:
        # the two scales must differ by far more than the bound, or the explicit one proves nothing
        nm = masks["random"]
        a, b = (local_reference(Q, K, V, nm, dil, s, F32) for s in (None, 0.61))
        assert rel(a, b) > 1e-2


# ---------------------------------------------------------------------------------------------------------------------
# isa_instance_norm_res, called directly
# ---------------------------------------------------------------------------------------------------------------------
def inorm_operands(n, hw, c, offsets, seed):
    g = torch.Generator().manual_seed(seed)
    x, res = torch.randn(n, c, 1, hw, generator=g), torch.randn(n, c, 1, hw, generator=g)
    if offsets:            # per-channel offsets of mean 8, std 1 on both addends
        x = x + (8 + torch.randn(1, c, 1, 1, generator=g))
        res = res + (8 + torch.randn(1, c, 1, 1, generator=g))
    return x, res


# fp32 bound: 4 x the error of the restatement evaluated in float32 torch on the CPU against its float64 evaluation on the
# same operands (measured over the shapes below, largest value: 1.6e-7 plain, 8.2e-7 with the offsets), which covers
# another summation order and the kernel's fp32 atomics.  A float32 emulation of the one-pass E[v^2] - mean^2 sums the
# kernel used to take is 1.4e-5 to 3.7e-5 away on the offset operands (the finding behind its two shifted passes, whose
# emulation stays under 4e-7 everywhere).
INORM_TOL = {(F32, False): 4 * 1.6e-7, (F32, True): 4 * 8.2e-7,
             # bf16: the fp32 arithmetic and one rounding of the result, as for the local core
             (BF16, False): BF16_ROUND, (BF16, True): BF16_ROUND}


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("offsets", [False, True])
@pytest.mark.parametrize("hw", [1, 255, 4099])
def test_instance_norm_res_direct(hw, offsets, dtype):
    """isa_instance_norm_res on c in {1, 24, 40, 64} (40 does not divide the 256 lanes), n = 3, one image row of 1, 255 or
    4 099 pixels (one statistics workgroup / its stride loop and the cross-workgroup atomics), x, res and out as channel
    slices of wider buffers whose other channels must stay untouched, and inputs with a per-channel offset of mean 8
    (the variance as E[x^2] - mean^2 would lose its digits there).  One pixel: exactly zero."""
    A = ops()
    from isa_amd.engine import Act
    L = A.L
    n = 3
    for c in (1, 24, 40, 64):
        x, res = inorm_operands(n, hw, c, offsets, 100 + c)
        xb = torch.full((n, 1, hw, c + 13), 7.0, dtype=dtype, device="cuda")
        rb = torch.full((n, 1, hw, c + 3), 7.0, dtype=dtype, device="cuda")
        ob = torch.full((n, 1, hw, c + 16), 7.0, dtype=dtype, device="cuda")
        xb[..., 5:5 + c] = x.permute(0, 2, 3, 1).to(dtype)
        rb[..., 3:3 + c] = res.permute(0, 2, 3, 1).to(dtype)
        xa, ra, oa = Act(xb, 5, c), Act(rb, 3, c), Act(ob, 8, c)
        sums = torch.zeros(n * 2 * c, dtype=torch.float32, device="cuda")
        L.check(L.lib().isa_instance_norm_res(xa.d(), ra.d(), oa.d(), 1e-5, L.ptr(sums), L.stream_ptr()), "isa_instance_norm_res")
        torch.cuda.synchronize()
        ref = B.instance_norm_res(rounded(x, dtype), rounded(res, dtype))
        what = "instance_norm_res c=%d hw=%d offsets=%s %s" % (c, hw, offsets, dtype)
        if hw == 1:
            assert float(ref.abs().max()) == 0.0 and float(oa.nchw().abs().max()) == 0.0, what
        else:
            check(oa.nchw(), ref, INORM_TOL[(dtype, offsets)], what)
        assert bool((ob[..., :8] == 7).all()) and bool((ob[..., 8 + c:] == 7).all()), what      # the slice's neighbours


# ---------------------------------------------------------------------------------------------------------------------
# isa_linear_ln, called directly
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3, 70000])
def test_linear_ln_direct(rows):
    """isa_linear_ln over (K, N) in {(1,1), (24,24), (100,33), (7,64)} and all sixteen presences of bias, residual, gamma
    and beta (the kernel accepts every one; beta without gamma is unused).  N = 1 under LayerNorm is exactly beta (or 0).
    Bound: MultiHeadAttention's 2e-5 (the deepest contraction here, K = 100, leaves the float32 restatement 3.8e-7 from its
    float64 evaluation).  N = 65 is refused."""
    A = ops()
    g = torch.Generator().manual_seed(rows)
    for K, N in ((1, 1), (24, 24), (100, 33), (7, 64)):
        x, w = torch.randn(rows, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
        bias, res = torch.randn(N, generator=g), torch.randn(rows, N, generator=g)
        gamma, beta = 1 + 0.3 * torch.randn(N, generator=g), torch.randn(N, generator=g)
        dev = [t.cuda() for t in (x, w, bias, res, gamma, beta)]
        f64 = [t.double() for t in (x, w, bias, res, gamma, beta)]
        for hb, hr, hg, hbe in itertools.product((False, True), repeat=4):
            pick = lambda ts: ts[:2] + [t if has else None for t, has in zip(ts[2:], (hb, hr, hg, hbe))]
            got = A._linear_ln(*pick(dev))
            torch.cuda.synchronize()
            ref = B.linear_ln(*pick(f64))
            what = "linear_ln rows=%d K=%d N=%d bias=%d res=%d gamma=%d beta=%d" % (rows, K, N, hb, hr, hg, hbe)
            if N == 1 and hg:
                want = beta.expand(rows, 1) if hbe else torch.zeros(rows, 1)
                assert torch.equal(got.cpu(), want), what
                assert torch.equal(ref.float(), want), what
            else:
                check(got, ref, 2e-5, what)
    with pytest.raises(A.L.IsaError):
        A._linear_ln(torch.randn(2, 8).cuda(), torch.randn(65, 8).cuda(), None)


# ---------------------------------------------------------------------------------------------------------------------
# isa_sdp_scores (the last=True branch)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16, F16])
@pytest.mark.parametrize("L_", [1, 255, 1000, 262147])
def test_sdp_scores_direct(L_, dtype):
    """isa_sdp_scores: raw and sigmoid, 1 and 2 interleaved heads, 1 and 3 queries, d in {7, 12, 40}; 262 147 keys are three
    past its grid (1 024 x 256), so the stride loop runs.  The result is fp32 whatever the storage, and the reference reads
    the same rounded operands: 1e-5 (the sdp core's fp32 bound) holds for the three storage types."""
    A = ops()
    L = A.L
    b = 2
    g = torch.Generator().manual_seed(L_)
    combos = list(itertools.product((0, 1), (1, 2), (1, 3), (7, 12, 40)))
    if L_ > 1000:        # every value of every argument once more at the long length (the full product there is 370 M draws)
        combos = [(0, 1, 1, 7), (1, 2, 3, 12), (1, 1, 3, 40), (0, 2, 1, 40)]
    for sig, heads, lq, d in combos:
        q, k = torch.randn(b, lq, heads * d, generator=g), torch.randn(b, L_, heads * d, generator=g)
        qd, kd = q.cuda().to(dtype), k.cuda().to(dtype)
        out = torch.empty(heads * b, lq, L_, dtype=torch.float32, device="cuda")
        L.check(L.lib().isa_sdp_scores(L.ptr(qd), L.ptr(kd), L.ptr(out), b, heads, lq, L_, d, L.dtype_code(dtype), sig,
                                       L.stream_ptr()), "isa_sdp_scores")
        torch.cuda.synchronize()
        # head-major rows (h*b + image), the reference's (n*b) batch
        hm = lambda t, l: rounded(t, dtype).view(b, l, heads, d).permute(2, 0, 1, 3).reshape(heads * b, l, d)
        ref = B.sdp_scores(hm(q, lq), hm(k, L_), bool(sig))
        check(out, ref, 1e-5, "sdp_scores L=%d %s sigmoid=%d heads=%d lq=%d d=%d" % (L_, dtype, sig, heads, lq, d))


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_scaled_dot_product_attention_module_last(dtype):
    """ScaledDotProductAttention.forward(last=True): the raw q k^T, no temperature, no mask (utils.py:315-318)."""
    A = ops()
    g = torch.Generator().manual_seed(11)
    q, k = torch.randn(3, 2, 12, generator=g), torch.randn(3, 300, 12, generator=g)
    att = A.ScaledDotProductAttention(temperature=12 ** 0.5)
    out = att(q.cuda().to(dtype), k.cuda().to(dtype), k.cuda().to(dtype), mask=torch.ones(3, 2, 300, dtype=torch.bool).cuda(), last=True)
    torch.cuda.synchronize()
    check(out, B.sdp_scores(rounded(q, dtype), rounded(k, dtype), False), 1e-5, "ScaledDotProductAttention last %s" % dtype)


# ---------------------------------------------------------------------------------------------------------------------
# scaled_dot_product_attention, forward
# ---------------------------------------------------------------------------------------------------------------------
SDP_TOL = {F32: 1e-5, BF16: 2e-2, F16: 3e-3}


def sdp_heads_reference(q, k, v, temp, mask_hm, heads, dtype):
    """Per head on the rounded operands.  mask_hm: head-major [(heads*b), lq, L] or None.  Returns (out [b, lq, heads*dv]
    with the heads interleaved, attn head-major)."""
    b, lq, L_ = q.shape[0], q.shape[1], k.shape[1]
    d, dv = q.shape[2] // heads, v.shape[2] // heads
    outs, attns = [], []
    for h in range(heads):
        m = None if mask_hm is None else mask_hm[h * b:(h + 1) * b]
        o, a = B.sdp_attention(rounded(q[..., h * d:(h + 1) * d], dtype), rounded(k[..., h * d:(h + 1) * d], dtype),
                               rounded(v[..., h * dv:(h + 1) * dv], dtype), temp, m)
        outs.append(o)
        attns.append(a)
    return torch.cat(outs, 2), torch.cat(attns, 0)


@pytest.fixture(scope="module")
def two_head_operands():
    g = torch.Generator().manual_seed(4097)
    b, lq, L_ = 3, 3, 4097
    q, k, v = torch.randn(b, lq, 24, generator=g), torch.randn(b, L_, 24, generator=g), torch.randn(b, L_, 24, generator=g)
    shared = torch.rand(b, lq, L_, generator=g) < 0.3
    per_head = torch.rand(2 * b, lq, L_, generator=g) < 0.3
    per_head[1 * b + 1, 2] = True                       # (head 1, image 1, query 2): every key masked
    return q, k, v, shared, per_head


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_sdp_forward_two_interleaved_heads(two_head_operands, dtype):
    """2 interleaved heads, b = 3, lq = 3 (a pass of two queries and a pass of one), L = 4 097 (two splits, the second of one
    key): out and the head-major attn directly, with the mask shared by the heads (the reference's repeat), with a mask per
    head (one (head, row) fully masked: NaN there alone), with none, and without the attention map (the same out, bit
    for bit: nothing of its arithmetic depends on the map)."""
    A = ops()
    q, k, v, shared, per_head = two_head_operands
    temp = 12 ** 0.5
    qd, kd, vd = (t.cuda().to(dtype) for t in (q, k, v))
    tol = SDP_TOL[dtype]
    for name, mask, per, mask_hm in (("shared", shared, False, shared.repeat(2, 1, 1)), ("per head", per_head, True, per_head),
                                     ("none", None, False, None)):
        out, attn = A.scaled_dot_product_attention(qd, kd, vd, temp, None if mask is None else mask.cuda(), heads=2,
                                                   mask_per_head=per)
        out2, none = A.scaled_dot_product_attention(qd, kd, vd, temp, None if mask is None else mask.cuda(), heads=2,
                                                    mask_per_head=per, return_attn=False)
        torch.cuda.synchronize()
        ref_o, ref_a = sdp_heads_reference(q, k, v, temp, mask_hm, 2, dtype)
        if name == "per head":
            nan = torch.zeros(3, 3, 24, dtype=torch.bool)
            nan[1, 2, 12:] = True
            assert torch.equal(torch.isnan(ref_o), nan)
        else:
            assert not torch.isnan(ref_o).any()
        check(out.float(), ref_o, tol, "sdp 2 heads out, mask %s %s" % (name, dtype))
        check(attn, ref_a, tol, "sdp 2 heads attn, mask %s %s" % (name, dtype))
        assert none is None
        assert torch.equal(torch.nan_to_num(out2.float(), nan=-7.0), torch.nan_to_num(out.float(), nan=-7.0)), name
        if mask_hm is not None:
            assert float(attn[mask_hm.cuda() & ~torch.isnan(attn)].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_sdp_forward_dk_not_dv(dtype):
    """(d_k, d_v) = (16, 8): the one-workgroup-per-query kernel (one head, f32 / bf16), masked, with a fully masked row,
    several tiles of 256 keys and a ragged last one."""
    A = ops()
    g = torch.Generator().manual_seed(168)
    bh, lq, L_ = 3, 2, 777
    q, k, v = torch.randn(bh, lq, 16, generator=g), torch.randn(bh, L_, 16, generator=g), torch.randn(bh, L_, 8, generator=g)
    mask = torch.rand(bh, lq, L_, generator=g) < 0.3
    mask[2, 1] = True
    for m in (mask, None):
        out, attn = A.scaled_dot_product_attention(q.cuda().to(dtype), k.cuda().to(dtype), v.cuda().to(dtype), 4.0,
                                                   None if m is None else m.cuda())
        out2, _ = A.scaled_dot_product_attention(q.cuda().to(dtype), k.cuda().to(dtype), v.cuda().to(dtype), 4.0,
                                                 None if m is None else m.cuda(), return_attn=False)
        torch.cuda.synchronize()
        ref_o, ref_a = sdp_heads_reference(q, k, v, 4.0, m, 1, dtype)
        assert bool(torch.isnan(ref_o[2, 1]).all()) == (m is not None)
        check(out.float(), ref_o, SDP_TOL[dtype], "sdp (16, 8) out %s masked=%s" % (dtype, m is not None))
        check(attn, ref_a, SDP_TOL[dtype], "sdp (16, 8) attn %s masked=%s" % (dtype, m is not None))
        assert torch.equal(torch.nan_to_num(out2.float(), nan=-7.0), torch.nan_to_num(out.float(), nan=-7.0))
    with pytest.raises(A.L.IsaError):                    # f16 and interleaved heads exist at d_k = d_v = 12 only
        A.scaled_dot_product_attention(q.cuda().half(), k.cuda().half(), v.cuda().half(), 4.0, None)
    with pytest.raises(A.L.IsaError):
        A.scaled_dot_product_attention(q.cuda(), k.cuda(), v.cuda(), 4.0, None, heads=2)


# ---------------------------------------------------------------------------------------------------------------------
# point_query_mask (Decoder.forward)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("b,c,h,w", [(3, 1, 7, 9), (3, 20, 7, 9), (3, 24, 7, 9), (3, 64, 7, 9), (1, 64, 1, 1), (2, 24, 513, 520)])
def test_point_query_mask_shapes(b, c, h, w, dtype):
    """point_query_mask over c in {1, 20, 24, 64} (20: the padded NHWC path), the fixture's Decoder shapes, and 2 x 513 x 520
    pixels (past the grid cap of 2 048 x 256: the stride loop).  The map is fp32 and q stays fp32 whatever enc's storage:
    1e-5, the point query's fp32 bound, for both."""
    A = ops()
    g = torch.Generator().manual_seed(c * 100 + h)
    q, enc = torch.randn(b, c, generator=g), torch.randn(b, c, h, w, generator=g)
    got = A.point_query_mask(q.cuda(), enc.cuda(), dtype=dtype)
    torch.cuda.synchronize()
    check(got, B.point_query_mask(q, rounded(enc, dtype)), 1e-5, "point_query %s %s" % ((b, c, h, w), dtype))
