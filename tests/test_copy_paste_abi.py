"""CPU-only: isa_copy_paste_u8 refuses bad arguments before it launches, clears or writes anything (so this runs without a
GPU: every pointer below is host memory that no kernel may ever see); the constants and the scratch helper mirror the
header; train.py carries the flags; data.copy_paste and the loader's arguments exist with the documented defaults."""
import inspect
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

ISA_EINVAL, ISA_EALIGN, ISA_ENOMEM = -1, -2, -5
N, H, W, C, K = 2, 8, 12, 3, 32
NAME = "isa_copy_paste_u8"
INPUTS = ("rgb", "sem", "planes", "n_objects", "xform", "select")
OUTPUTS = ("rgb_out", "sem_out", "planes_out", "n_out", "plan", "scratch")
BYTES = dict(rgb=N * H * W * C, sem=N * H * W, planes=N * H * W * K, n_objects=N * 4, xform=N * 16, select=N * 4,
             rgb_out=N * H * W * C, sem_out=N * H * W, planes_out=N * H * W * K, n_out=N * 4, plan=N * 16, scratch=N * K * 8)


def _lib():
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    return L, L.lib()


def _valid_args(L, keep, k=K):
    """A complete, valid argument list over host buffers (64-byte aligned, 0x5a in every byte), as a dict in ABI order."""
    buf = lambda: keep.append(torch.full((65536,), 0x5a, dtype=torch.uint8)) or keep[-1].data_ptr()
    a = dict(rgb=buf(), sem=buf(), planes=buf(), n_objects=buf(), xform=buf(), select=buf(), n=N, h=H, w=W, c=C, k=k, min_area=1,
             rgb_out=buf(), sem_out=buf(), planes_out=buf(), n_out=buf(), plan=buf(), scratch=buf(),
             scratch_bytes=L.copy_paste_scratch_bytes(N, k), stream=None)
    assert len(a) == len(L.SIGNATURES[NAME]) == 20
    return a


def _untouched(keep):
    return all(bool((t == 0x5a).all()) for t in keep)


def test_refuses_bad_arguments_before_launching():
    L, lib = _lib()
    fn = getattr(lib, NAME)
    keep = []
    for ptr in INPUTS + OUTPUTS:
        a = _valid_args(L, keep)
        a[ptr] = None
        assert fn(*a.values()) == ISA_EINVAL, ptr
    bad = dict(n=(0, -1, 65536), h=(0, -8, 4097), w=(0, -12, 4097), c=(0, -3, 5), k=(0, -1, 33, 64))
    for key, values in bad.items():
        for v in values:
            a = _valid_args(L, keep)
            a[key] = v
            assert fn(*a.values()) == ISA_EINVAL, (key, v)
    for ptr in ("n_objects", "xform", "select", "n_out", "plan", "scratch"):
        for off in (1, 2):
            a = _valid_args(L, keep)
            a[ptr] += off
            assert fn(*a.values()) == ISA_EALIGN, (ptr, off)
    for k in (16, 32):                                    # whole pixel vectors move as 16-byte loads and stores
        for ptr in ("planes", "planes_out"):
            for off in (1, 4, 8):
                a = _valid_args(L, keep, k)
                a[ptr] += off
                assert fn(*a.values()) == ISA_EALIGN, (k, ptr, off)
    # any other k moves bytes, and the image and the semantic map always do: no alignment asked, so the next refusal
    for ptr in ("planes", "planes_out", "rgb", "rgb_out", "sem", "sem_out"):
        a = _valid_args(L, keep, 6)
        a[ptr] += 1
        a["scratch_bytes"] -= 1
        assert fn(*a.values()) == ISA_ENOMEM, ptr
    assert _untouched(keep)


def test_refuses_a_short_scratch():
    L, lib = _lib()
    keep = []
    for k in (1, 6, 16, 32):
        for short in (0, 8, L.copy_paste_scratch_bytes(N, k) - 1, -1):
            a = _valid_args(L, keep, k)
            a["scratch_bytes"] = short
            assert lib.isa_copy_paste_u8(*a.values()) == ISA_ENOMEM, (k, short)
    for min_area in (-7, 0, 1 << 30):                     # every min_area is legal
        a = _valid_args(L, keep)
        a["min_area"] = min_area
        a["scratch_bytes"] -= 1
        assert lib.isa_copy_paste_u8(*a.values()) == ISA_ENOMEM
    assert _untouched(keep)


def test_refuses_outputs_that_alias_an_input_or_each_other():
    L, lib = _lib()
    keep = []
    for out, inp in (("rgb_out", "rgb"), ("sem_out", "sem"), ("planes_out", "planes"), ("n_out", "n_objects"), ("plan", "xform"),
                     ("scratch", "select"), ("planes_out", "rgb"), ("n_out", "select"), ("scratch", "planes")):
        for off in (0, 4, BYTES[inp] - 4):                # equal, and overlapping at either end
            assert 0 <= off < BYTES[inp]
            a = _valid_args(L, keep)
            a[out] = a[inp] + off
            assert lib.isa_copy_paste_u8(*a.values()) == ISA_EINVAL, (out, inp, off)
        for off in (0, 4, BYTES[out] - 4):
            assert 0 <= off < BYTES[out]
            a = _valid_args(L, keep)
            a[inp] = a[out] + off
            assert lib.isa_copy_paste_u8(*a.values()) == ISA_EINVAL, (inp, out, off)
    for one, two in (("rgb_out", "sem_out"), ("planes_out", "scratch"), ("n_out", "plan")):
        a = _valid_args(L, keep)
        a[one] = a[two]
        assert lib.isa_copy_paste_u8(*a.values()) == ISA_EINVAL, (one, two)
    a = _valid_args(L, keep)                              # right behind the input: no overlap, so the next refusal
    a["planes_out"] = a["planes"] + BYTES["planes"]
    a["scratch_bytes"] = 0
    assert lib.isa_copy_paste_u8(*a.values()) == ISA_ENOMEM
    assert _untouched(keep)


def test_constants_and_scratch_formula_match_the_header():
    L, _ = _lib()
    text = open(os.path.join(ROOT, "include", "isa_kernels.h")).read()
    assert "#define ISA_PASTE_MAX_SIDE %d\n" % L.PASTE_MAX_SIDE in text
    assert "#define ISA_PASTE_MAX_PLANES %d\n" % L.PASTE_MAX_PLANES in text
    assert "#define ISA_COPY_PASTE_SCRATCH_BYTES(n, k) ((int64_t)(n) * (k) * 8)\n" in text
    assert L.copy_paste_scratch_bytes(3, 32) == 3 * 32 * 8 and L.copy_paste_scratch_bytes(5, 6) == 5 * 6 * 8
    assert (L.PASTE_MAX_SIDE, L.PASTE_MAX_PLANES) == (4096, 32)
    assert "int isa_copy_paste_u8(" in text


def test_train_flags_and_host_signatures():
    import isa_amd  # noqa: F401
    from isa_amd import data as D
    from isa_amd.records import RecordLoader
    import train
    plain = train.parse_args([])
    assert train.copy_paste_arguments(plain) == dict(copy_paste=False, copy_paste_p=0.5, copy_paste_min_area=16, copy_paste_shift=0.5)
    on = train.parse_args(['--copy-paste', '--copy-paste-p', '0.25', '--copy-paste-min-area', '40', '--copy-paste-shift', '1'])
    assert train.copy_paste_arguments(on) == dict(copy_paste=True, copy_paste_p=0.25, copy_paste_min_area=40, copy_paste_shift=1.0)
    assert train.fit_arguments(on) == train.fit_arguments(plain) and train.fit_keywords(on) == train.fit_keywords(plain)
    assert train.photometric_arguments(on) == train.photometric_arguments(plain)
    assert train.elastic_arguments(on) == train.elastic_arguments(plain)
    for good in (['--copy-paste-p', '0'], ['--copy-paste-p', '1'], ['--copy-paste-min-area', '1'], ['--copy-paste-shift', '0']):
        train.parse_args(good)
    for bad in (['--copy-paste-p', '1.5'], ['--copy-paste-p', '-0.1'], ['--copy-paste-min-area', '0'], ['--copy-paste-min-area', '-3'],
                ['--copy-paste-shift', '1.01'], ['--copy-paste-shift', '-0.5']):
        with pytest.raises(SystemExit):
            train.parse_args(bad)
    sig = inspect.signature(RecordLoader.__init__).parameters
    assert [sig[k].default for k in ("copy_paste", "copy_paste_p", "copy_paste_min_area", "copy_paste_shift")] == [False, 0.5, 16, 0.5]
    assert set(train.copy_paste_arguments(plain)) <= set(sig)
    p = inspect.signature(D.copy_paste).parameters
    assert list(p) == ["rgb", "sem", "planes", "n_objects", "src", "select", "flip", "shift", "min_area", "device", "out", "scratch"]
    assert p["min_area"].default == 1 and p["device"].default == "cuda" and p["out"].default is None and p["scratch"].default is None
