"""CPU-only: isa_elastic_field and isa_warp_u8 refuse bad arguments before they launch or write anything (so this runs
without a GPU: every pointer below is host memory that no kernel may ever see); the constants and the size helper mirror
the header; train.py carries the flags; the host functions and the loader's arguments exist with the documented defaults."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

ISA_EINVAL, ISA_EALIGN, ISA_ENOMEM = -1, -2, -5
N, H, W, C, R = 2, 8, 12, 3, 2


def _lib():
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    return L, L.lib()


def _valid_args(L, name, keep):
    """A complete, valid argument list of entry `name` over host buffers (64-byte aligned), as a dict in ABI order."""
    buf = lambda: keep.append(torch.zeros(16384)) or keep[-1].data_ptr()            # 64 KiB each
    if name == "isa_elastic_field":
        a = dict(noise=buf(), alpha_dev=buf(), n=N, h=H, w=W, taps_host=buf(), radius=R, disp=buf(), scratch=buf(),
                 scratch_bytes=L.elastic_scratch_bytes(N, H, W), stream=None)
    else:
        a = dict(src=buf(), disp=buf(), n=N, h=H, w=W, c=C, mode=L.WARP_BILINEAR, dst=buf(), stream=None)
    assert len(a) == len(L.SIGNATURES[name]), name
    return a


POINTERS = {"isa_elastic_field": ("noise", "alpha_dev", "taps_host", "disp", "scratch"), "isa_warp_u8": ("src", "disp", "dst")}
BAD_VALUES = {"isa_elastic_field": dict(n=(0, -1, 65536), h=(0, -8, 1025), w=(0, -12, 1025), radius=(-1, 65, 1 << 20)),
              "isa_warp_u8": dict(n=(0, -1, 65536), h=(0, -8, 1025), w=(0, -12, 1025), c=(0, -3, 65), mode=(-1, 2, 7))}
MISALIGNED = {"isa_elastic_field": (("noise", 4), ("disp", 4), ("scratch", 8), ("scratch", 4)),
              "isa_warp_u8": (("src", 1), ("src", 2), ("dst", 1), ("dst", 2), ("disp", 4))}


@pytest.mark.parametrize("name", sorted(POINTERS))
def test_elastic_entries_refuse_bad_arguments_before_launching(name):
    L, lib = _lib()
    fn = getattr(lib, name)
    keep = []
    for ptr in POINTERS[name]:
        a = _valid_args(L, name, keep)
        a[ptr] = None
        assert fn(*a.values()) == ISA_EINVAL, (name, ptr)
    for key, values in BAD_VALUES[name].items():
        for v in values:
            a = _valid_args(L, name, keep)
            a[key] = v
            assert fn(*a.values()) == ISA_EINVAL, (name, key, v)
    for ptr, off in MISALIGNED[name]:
        a = _valid_args(L, name, keep)
        a[ptr] += off
        assert fn(*a.values()) == ISA_EALIGN, (name, ptr, off)


def test_field_refuses_short_scratch_and_a_field_over_its_noise():
    L, lib = _lib()
    keep = []
    a = _valid_args(L, "isa_elastic_field", keep)
    a["scratch_bytes"] -= 1
    assert lib.isa_elastic_field(*a.values()) == ISA_ENOMEM
    a = _valid_args(L, "isa_elastic_field", keep)
    a["scratch_bytes"] = 0
    a["radius"] = 0                                       # the maximum and the minimum radius are valid: the next refusal
    assert lib.isa_elastic_field(*a.values()) == ISA_ENOMEM
    a["radius"] = L.ELASTIC_MAX_RADIUS
    assert lib.isa_elastic_field(*a.values()) == ISA_ENOMEM
    for off in (0, 8, N * H * W * 8 - 8):                 # equal, and overlapping at either end
        a = _valid_args(L, "isa_elastic_field", keep)
        a["disp"] = a["noise"] + off
        assert lib.isa_elastic_field(*a.values()) == ISA_EINVAL, off
        a = _valid_args(L, "isa_elastic_field", keep)
        a["noise"] = a["disp"] + off
        assert lib.isa_elastic_field(*a.values()) == ISA_EINVAL, off
    a = _valid_args(L, "isa_elastic_field", keep)         # right behind the noise: no overlap, so the next refusal is the
    a["disp"] = a["noise"] + N * H * W * 8                # scratch size
    a["scratch_bytes"] = 8
    assert lib.isa_elastic_field(*a.values()) == ISA_ENOMEM


def test_warp_refuses_an_output_that_overlaps_the_source():
    L, lib = _lib()
    keep = []
    for off in (0, 4, N * H * W * C - 4):
        a = _valid_args(L, "isa_warp_u8", keep)
        a["dst"] = a["src"] + off
        assert lib.isa_warp_u8(*a.values()) == ISA_EINVAL, off
        a = _valid_args(L, "isa_warp_u8", keep)
        a["src"] = a["dst"] + off
        assert lib.isa_warp_u8(*a.values()) == ISA_EINVAL, off
    a = _valid_args(L, "isa_warp_u8", keep)               # right behind the source: no overlap, so the next refusal is the
    a["dst"] = a["src"] + N * H * W * C                   # alignment of another argument
    a["disp"] += 4
    assert lib.isa_warp_u8(*a.values()) == ISA_EALIGN
    for c in (1, 32, 64):                                 # every lane mapping checks before it launches
        a = _valid_args(L, "isa_warp_u8", keep)
        a["c"], a["mode"] = c, L.WARP_NEAREST
        a["disp"] += 4
        assert lib.isa_warp_u8(*a.values()) == ISA_EALIGN, c


def test_constants_and_scratch_formula_match_the_header():
    L, _ = _lib()
    text = open(os.path.join(ROOT, "include", "isa_kernels.h")).read()
    assert "#define ISA_ELASTIC_MAX_RADIUS %d\n" % L.ELASTIC_MAX_RADIUS in text
    assert "#define ISA_WARP_MAX_SIDE %d\n" % L.WARP_MAX_SIDE in text
    assert "#define ISA_WARP_MAX_CHANNELS %d\n" % L.WARP_MAX_CHANNELS in text
    assert "#define ISA_WARP_NEAREST %d\n" % L.WARP_NEAREST in text and "#define ISA_WARP_BILINEAR %d\n" % L.WARP_BILINEAR in text
    assert "#define ISA_ELASTIC_SCRATCH_BYTES(n, h, w) ((int64_t)(n) * (h) * (w) * 8)\n" in text
    assert L.elastic_scratch_bytes(3, 8, 12) == 3 * 8 * 12 * 8
    assert (L.ELASTIC_MAX_RADIUS, L.WARP_MAX_SIDE, L.WARP_MAX_CHANNELS) == (64, 1024, 64)


def test_gaussian_taps_are_scipys_kernel_in_float32():
    import isa_amd  # noqa: F401
    from isa_amd import data as D
    from scipy.ndimage import gaussian_filter1d
    for sigma in (0.6, 2.0, 4.0, 8.0, 16.0):
        taps, radius = D.gaussian_taps(sigma)
        assert radius == int(4.0 * sigma + 0.5) and taps.dtype == np.float32 and taps.shape == (2 * radius + 1,)
        impulse = np.zeros(2 * radius + 1)
        impulse[radius] = 1.0
        want = gaussian_filter1d(impulse, sigma, mode='constant', truncate=4.0)
        assert np.array_equal(taps, want.astype(np.float32)), sigma
    assert D.gaussian_taps(3.0, truncate=2.0)[1] == 6
    taps, radius = D.gaussian_taps(0.1)
    assert radius == 0 and taps.tolist() == [1.0]
    with pytest.raises(AssertionError):
        D.gaussian_taps(16.2)                             # radius 65


def test_train_flags_and_host_signatures():
    import isa_amd  # noqa: F401
    from isa_amd import data as D
    from isa_amd.records import RecordLoader
    sys.path[:0] = [ROOT]
    import train
    plain = train.parse_args([])
    assert plain.elastic is False and list(plain.elastic_alpha) == [0.0, 100.0]
    assert plain.elastic_sigma == 8.0 and plain.elastic_p == 0.5
    assert train.elastic_arguments(plain) == dict(elastic=False, elastic_alpha=(0.0, 100.0), elastic_sigma=8.0, elastic_p=0.5)
    on = train.parse_args(['--elastic', '--elastic-alpha', '10', '60', '--elastic-sigma', '4', '--elastic-p', '0.25'])
    assert train.elastic_arguments(on) == dict(elastic=True, elastic_alpha=(10.0, 60.0), elastic_sigma=4.0, elastic_p=0.25)
    assert train.fit_arguments(on) == train.fit_arguments(plain) and train.fit_keywords(on) == train.fit_keywords(plain)
    assert train.photometric_arguments(on) == train.photometric_arguments(plain)
    for bad in (['--elastic-alpha', '5', '1'], ['--elastic-p', '1.5'], ['--elastic-sigma', '17']):
        with pytest.raises(SystemExit):
            train.parse_args(bad)
    sig = inspect.signature(RecordLoader.__init__).parameters
    assert [sig[k].default for k in ("elastic", "elastic_alpha", "elastic_sigma", "elastic_p")] == [False, (0.0, 100.0), 8.0, 0.5]
    assert set(train.elastic_arguments(plain)) <= set(sig)
    assert list(inspect.signature(D.gaussian_taps).parameters) == ["sigma", "truncate"]
    assert inspect.signature(D.gaussian_taps).parameters["truncate"].default == 4.0
    assert list(inspect.signature(D.elastic_field).parameters) == ["noise", "alpha", "sigma", "device"]
    assert list(inspect.signature(D.warp).parameters) == ["tensors", "disp", "modes", "device"]
    p = inspect.signature(D.elastic).parameters
    assert list(p) == ["rgb", "sem", "planes", "n_objects", "disp", "max_planes", "device"] and p["max_planes"].default == 32
    assert all(inspect.signature(f).parameters["device"].default == "cuda" for f in (D.elastic_field, D.warp, D.elastic))
