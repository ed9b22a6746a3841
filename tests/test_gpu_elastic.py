"""isa_elastic_field and isa_warp_u8 on the device against the NumPy restatement (tests/elastic_np.py).
Field: within alpha * (4 * radius + 8) * 2**-24 absolute - the first-order rounding bound of two recursive fp32 sums of
2 * radius + 1 products with |x| <= 1 and weights that sum to 1, plus the final scale, rounded up (FMA contraction only
tightens it); an image with alpha 0 is exactly zero; two runs give the same bits.  Warp: EXACTLY equal, both modes, every
lane mapping (c = 1, 3: a lane per pixel; 7: a lane per byte; 32: a lane per 16-byte group).  Every output sits between
sentinel pads that must stay unchanged; the scratch is pre-filled with 0xAB."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
import elastic_np as E   # noqa: E402

PAD_F = 64               # sentinel floats on either side of a field
PAD_B = 68               # sentinel bytes on either side of a warped tensor: the output is 4-byte aligned and no more
SENT_F, SENT_B = -12345.5, 0xCD


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    return L


def _noise(shape, seed):
    return np.random.default_rng(seed).uniform(-1, 1, shape + (2,)).astype(np.float32)


def run_field(L, noise, alpha, taps, radius):
    """isa_elastic_field over `noise` [n,h,w,2] (numpy) -> disp (numpy); checks the pads."""
    n, h, w, _ = noise.shape
    dn = torch.from_numpy(noise).cuda()
    da = torch.tensor(alpha, dtype=torch.float32, device="cuda")
    buf = torch.full((2 * PAD_F + noise.size,), SENT_F, dtype=torch.float32, device="cuda")
    need = L.elastic_scratch_bytes(n, h, w)
    scratch = torch.full((need + 32,), 0xAB, dtype=torch.uint8, device="cuda")
    tp = np.ascontiguousarray(taps, np.float32)
    L.check(L.lib().isa_elastic_field(L.ptr(dn), L.ptr(da), n, h, w, tp.ctypes.data_as(C.c_void_p), radius,
                                      C.c_void_p(buf.data_ptr() + 4 * PAD_F), L.ptr(scratch), need, L.stream_ptr()),
            "isa_elastic_field")
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:PAD_F] == SENT_F).all() and (out[-PAD_F:] == SENT_F).all(), "the field wrote outside its output"
    assert (scratch[need:].cpu().numpy() == 0xAB).all(), "the field wrote behind its scratch"
    assert np.array_equal(dn.cpu().numpy(), noise)
    return out[PAD_F:-PAD_F].reshape(noise.shape)


def run_warp(L, src, disp, mode):
    """isa_warp_u8 of src uint8 [n,h,w,c] (numpy) by disp (numpy) -> numpy; source and output 4-byte aligned only."""
    n, h, w, c = src.shape
    sbuf = torch.zeros((4 + src.size,), dtype=torch.uint8, device="cuda")
    sbuf[4:] = torch.from_numpy(src).cuda().reshape(-1)
    dd = torch.from_numpy(np.ascontiguousarray(disp, np.float32)).cuda()
    buf = torch.full((2 * PAD_B + src.size,), SENT_B, dtype=torch.uint8, device="cuda")
    L.check(L.lib().isa_warp_u8(C.c_void_p(sbuf.data_ptr() + 4), L.ptr(dd), n, h, w, c, mode, C.c_void_p(buf.data_ptr() + PAD_B),
                                L.stream_ptr()), "isa_warp_u8")
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[:PAD_B] == SENT_B).all() and (out[-PAD_B:] == SENT_B).all(), "the warp wrote outside its output"
    assert np.array_equal(sbuf[4:].cpu().numpy().reshape(src.shape), src)
    return out[PAD_B:-PAD_B].reshape(src.shape)


FIELD_CASES = [((1, 4, 4), 8, (25.0,)),                     # the halo is larger than the image, one partial wave
               ((1, 8, 12), 2, (10.0,)),
               ((1, 8, 12), 0, (10.0,)),                     # disp = alpha * noise
               ((2, 72, 136), 16, (0.0, 37.5)),              # no multiple of 64 either way; the first image exactly zero
               ((3, 64, 64), 64, (100.0, 1.0, 50.0)),        # the maximum radius, full-wave widths
               ((2, 256, 256), 32, (100.0, 60.0))]           # the loader's shape


@pytest.mark.parametrize("shape,radius,alpha", FIELD_CASES)
def test_field_matches_the_float64_restatement_and_is_reproducible(shape, radius, alpha):
    L = need_gpu()
    taps, r = E.taps(radius / 4.0)
    assert r == radius
    noise = _noise(shape, 11 + radius)
    got = run_field(L, noise, alpha, taps, radius)
    want = E.field(noise, alpha, taps)
    for b, a in enumerate(alpha):
        err = np.abs(got[b] - want[b]).max()
        bound = a * (4 * radius + 8) * 2.0 ** -24
        print("field %s radius %d image %d alpha %g: max error %.3g, bound %.3g" % (shape, radius, b, a, err, bound))
        assert err <= bound, (b, err, bound)
        if a == 0.0:
            assert not got[b].any()
    assert np.abs(got).max() > 0
    again = run_field(L, noise, alpha, taps, radius)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "two runs differ"
    if radius == 0:                                          # whatever the single tap says
        assert np.array_equal(run_field(L, noise, alpha, np.array([0.25], np.float32), 0).view(np.uint32), got.view(np.uint32))
        assert np.array_equal(got, noise * np.float32(alpha[0]))


def hand_fields(shape):
    n, h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(h * w)

    def both(dx, dy):
        d = np.empty(shape + (2,), np.float32)
        d[..., 0], d[..., 1] = dx, dy
        return d

    tie = np.array([0.5, -0.5, 1.5, -1.5, 128.5 / 256, -129.5 / 256], np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 1e9, -1e9, 0.25, -3.0], np.float32)
    out = {"zero": both(0.0, 0.0), "shift": both(3.0, -2.0),
           "ties": both(tie[(xx + yy) % 6], tie[(xx + 2 * yy + 1) % 6]),
           "fractions": both(((xx * 7 + yy * 3) % 512 - 256) / 256.0, ((xx * 5 + yy * 11) % 512 - 256) / 256.0),
           "outside": both(rng.uniform(-(w + 8), w + 8, shape), rng.uniform(-(h + 8), h + 8, shape)),
           "special": both(special[(xx + 3 * yy) % 7], special[(2 * xx + yy + 2) % 7])}
    return out


_FIELDS = {}


def fields_of(L, shape):
    """The hand-made fields and the device's own (downloaded), once per shape."""
    if shape not in _FIELDS:
        f = hand_fields(shape)
        taps, radius = E.taps(2.0)
        f["device"] = run_field(L, _noise(shape, 21), [300.0] * shape[0], taps, radius)
        assert np.abs(f["device"]).max() > 2.0
        _FIELDS[shape] = f
    return _FIELDS[shape]


@pytest.mark.parametrize("c", [1, 3, 7, 32])
@pytest.mark.parametrize("shape", [(1, 4, 4), (2, 72, 136), (2, 256, 256)])
def test_warp_equals_the_restatement_bit_for_bit(shape, c):
    L = need_gpu()
    src = np.random.default_rng(31 + c).integers(0, 256, shape + (c,), dtype=np.uint8)
    for name, disp in fields_of(L, shape).items():
        want_n, want_b = E.warp_nearest(src, disp), E.warp_bilinear(src, disp)
        got_n, got_b = run_warp(L, src, disp, L.WARP_NEAREST), run_warp(L, src, disp, L.WARP_BILINEAR)
        assert np.array_equal(got_n, want_n), (name, "nearest", int((got_n != want_n).sum()))
        assert np.array_equal(got_b, want_b), (name, "bilinear", int((got_b != want_b).sum()))
        if name == "zero":
            assert np.array_equal(got_n, src) and np.array_equal(got_b, src)


def test_stage_pads_compacts_and_passes_through():
    """data.elastic on hand-made planes and per-image constant fields: 5 planes padded to max_planes = 8; image 0 loses its
    first plane (shifted out of the image) and keeps two, image 1 would lose both and passes through, image 2 is not moved."""
    L = need_gpu()
    from isa_amd import data as D
    n, h, w, K = 3, 12, 16, 5
    rng = np.random.default_rng(51)
    rgb, sem = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8), rng.integers(0, 2, (n, h, w), dtype=np.uint8)
    planes = np.zeros((n, h, w, K), np.uint8)
    planes[0, :, 0:3, 0] = planes[0, :, 6:9, 1] = planes[0, 2:5, 13:16, 2] = 1
    planes[1, :, 0:3, 0] = planes[1, 4:8, 4:6, 1] = 1
    for k in range(K):
        planes[2, k:k + 3, 2 * k:2 * k + 4, k] = 1
    counts = [3, 2, 5]
    disp = np.zeros((n, h, w, 2), np.float32)
    disp[0, :, :, 0], disp[1, :, :, 0] = 6.0, 20.0
    got = D.elastic(*(torch.from_numpy(a).cuda() for a in (rgb, sem, planes)), counts, torch.from_numpy(disp).cuda(), max_planes=8)
    padded = np.zeros((n, h, w, 8), np.uint8)
    padded[..., :K] = planes
    want = E.elastic(rgb, sem, padded, counts, disp)
    assert got[3] == want[3] == [2, 2, 5]
    assert all(np.array_equal(g.cpu().numpy(), x) for g, x in zip(got[:3], want[:3]))
    out = got[2].cpu().numpy()
    assert out.shape == (n, h, w, 8)
    assert np.array_equal(out[0, :, :, 0], E.warp_nearest(planes[:1, :, :, 1], disp[:1])[0]) and out[0, :, 0:3, 0].all()
    assert not out[0, :, :, 2:].any()                                    # the survivors at the front, zero planes behind
    assert np.array_equal(out[1], padded[1]) and np.array_equal(got[0][1].cpu().numpy(), rgb[1])    # unwarped
    assert np.array_equal(out[2], padded[2])
    assert isinstance(got[3], list) and D.elastic(*(torch.from_numpy(a).cuda() for a in (rgb, sem, padded)), torch.tensor(counts),
                                                  torch.from_numpy(disp).cuda())[3] == [2, 2, 5]


def test_host_functions_call_the_entries():
    """data.elastic_field and data.warp against the entries called directly; [n,h,w] inputs keep their shape."""
    L = need_gpu()
    from isa_amd import data as D
    shape = (2, 40, 72)
    noise = _noise(shape, 41)
    taps, radius = D.gaussian_taps(1.5)
    want = run_field(L, noise, [30.0, 80.0], taps, radius)
    for alpha in ([30.0, 80.0], torch.tensor([30.0, 80.0], device="cuda")):
        got = D.elastic_field(torch.from_numpy(noise).cuda(), alpha, 1.5)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    one = D.elastic_field(torch.from_numpy(noise).cuda(), 30.0, 1.5).cpu().numpy()
    assert np.array_equal(one[0], want[0]) and not np.array_equal(one[1], want[1])
    rng = np.random.default_rng(42)
    rgb, sem = rng.integers(0, 256, shape + (3,), dtype=np.uint8), rng.integers(0, 2, shape, dtype=np.uint8)
    a, b = D.warp([torch.from_numpy(rgb).cuda(), torch.from_numpy(sem).cuda()], torch.from_numpy(want).cuda(),
                  ["bilinear", "nearest"])
    assert a.shape == rgb.shape and b.shape == sem.shape
    assert np.array_equal(a.cpu().numpy(), E.warp_bilinear(rgb, want)) and np.array_equal(b.cpu().numpy(), E.warp_nearest(sem, want))
