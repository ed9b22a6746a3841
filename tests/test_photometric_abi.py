"""CPU-only: isa_photometric_u8 and isa_resize_lanczos_u8 refuse bad arguments before they launch or copy anything (so
this runs without a GPU: every pointer below is host memory that no kernel may ever see), isa_photo_prog is mirrored
byte for byte by lib.IsaPhotoProg, data.photo_program packs what the header says, and train.py's five photometric flags
reach the training loader and leave fit's argument tuple alone."""
import ctypes as C
import inspect
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

ISA_EINVAL, ISA_EALIGN, ISA_ENOMEM = -1, -2, -5


def _lib():
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    return L, L.lib()


def _valid_args(L, name, keep):
    """A complete, valid argument list of entry `name` over host buffers (64-byte aligned), as a dict in ABI order."""
    buf = lambda: keep.append(torch.zeros(4096)) or keep[-1].data_ptr()
    if name == "isa_photometric_u8":
        a = dict(src=buf(), dst=buf(), n=2, h=5, w=7, progs=buf(), has_contrast=1, sums=buf(), stream=None)
    else:
        a = dict(src=buf(), n=1, h0=8, w0=9, c=3, dst=buf(), h=5, w=6, ws=buf(), ws_bytes=16384, stream=None)
    assert len(a) == len(L.SIGNATURES[name]), name
    return a


POINTERS = {"isa_photometric_u8": ("src", "dst", "progs", "sums"), "isa_resize_lanczos_u8": ("src", "dst", "ws")}
BAD_VALUES = {"isa_photometric_u8": dict(n=(0, -1, 65536), h=(0, -5), w=(0, -7)),
              "isa_resize_lanczos_u8": dict(n=(0, -1), h0=(0, -8, 65536), w0=(0, -9, 65536), c=(0, -1, 5), h=(0, -5, 65536),
                                            w=(0, -6, 65536))}


@pytest.mark.parametrize("name", sorted(POINTERS))
def test_entries_refuse_bad_arguments_before_launching(name):
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


def test_photometric_workspace_rules():
    """The int64 sums need 8-byte alignment; without contrast no workspace is asked for (checked through the argument
    test alone: a NULL workspace with has_contrast = 1 is refused above)."""
    L, lib = _lib()
    keep = []
    a = _valid_args(L, "isa_photometric_u8", keep)
    a["sums"] += 4
    assert lib.isa_photometric_u8(*a.values()) == ISA_EALIGN


def test_lanczos_workspace_rules():
    L, lib = _lib()
    keep = []
    a = _valid_args(L, "isa_resize_lanczos_u8", keep)
    out = C.c_int64(-1)
    assert lib.isa_resize_lanczos_ws_bytes(a["n"], a["h0"], a["w0"], a["c"], a["h"], a["w"], C.byref(out)) == 0
    need = out.value
    # tables: 2 w + w kx + 2 h + h ky ints (kx = ceil(3 * 9/6) * 2 + 1 = 11, ky = ceil(3 * 8/5) * 2 + 1 = 11), rounded up to
    # 256 bytes, then the horizontal pass's intermediate n * h0 * w * c
    assert need == ((4 * (2 * 6 + 6 * 11 + 2 * 5 + 5 * 11) + 255) & ~255) + 1 * 8 * 6 * 3
    a["ws_bytes"] = need - 1
    assert lib.isa_resize_lanczos_u8(*a.values()) == ISA_ENOMEM
    a = _valid_args(L, "isa_resize_lanczos_u8", keep)
    a["ws"] += 2
    assert lib.isa_resize_lanczos_u8(*a.values()) == ISA_EALIGN
    a = _valid_args(L, "isa_resize_lanczos_u8", keep)
    a["dst"] = a["src"]                                               # out of place only
    assert lib.isa_resize_lanczos_u8(*a.values()) == ISA_EINVAL
    for bad in ((0, 8, 9, 3, 5, 6), (1, 8, 9, 5, 5, 6), (1, 65536, 9, 3, 5, 6), (1, 8, 9, 3, 5, 0)):
        assert lib.isa_resize_lanczos_ws_bytes(*bad, C.byref(out)) == ISA_EINVAL, bad
    assert lib.isa_resize_lanczos_ws_bytes(1, 8, 9, 3, 5, 6, None) == ISA_EINVAL
    # up-scaling keeps the filter's own support: ksize 7
    assert lib.isa_resize_lanczos_ws_bytes(1, 5, 6, 1, 8, 9, C.byref(out)) == 0
    assert out.value == ((4 * (2 * 9 + 9 * 7 + 2 * 8 + 8 * 7) + 255) & ~255) + 5 * 9


def test_photo_program_packs_the_header_layout():
    L, _ = _lib()
    from isa_amd import data as D
    assert C.sizeof(L.IsaPhotoProg) == 288
    offs = {f[0]: getattr(L.IsaPhotoProg, f[0]).offset for f in L.IsaPhotoProg._fields_}
    assert offs == dict(n_ops=0, op=4, factor=8, hue_shift=24, use_lut=25, gray=26, chan=27, pad=30, lut=32)
    p = D.photo_program()
    assert p.n_ops == 0 and list(p.chan) == [0, 1, 2] and not p.use_lut and not p.gray
    lut = D.gamma_lut(0.8)
    p = D.photo_program([("hue", -0.17), ("contrast", 1.25), ("brightness", 0.75)], lut, (2, 2, 0), True)
    assert p.n_ops == 3 and list(p.op)[:3] == [L.PHOTO_HUE, L.PHOTO_CONTRAST, L.PHOTO_BRIGHTNESS]
    assert p.hue_shift == (int(-0.17 * 255) & 255) == 213 and list(p.factor)[1:3] == [1.25, 0.75]
    assert p.use_lut == 1 and list(p.lut) == lut and list(p.chan) == [2, 2, 0] and p.gray == 1
    assert lut[0] == 0 and lut[255] == 255 and lut[1] == round(255 * pow(1 / 255., 0.8))
    for bad in (dict(ops=[("hue", 0.6)]), dict(ops=[("contrast", 1.0), ("contrast", 1.1)]), dict(ops=[("sharpness", 1.0)]),
                dict(chan=(0, 1, 3)), dict(lut=[0] * 255), dict(ops=[("brightness", -0.1)])):
        with pytest.raises(AssertionError):
            D.photo_program(**bad)


def test_loader_and_train_flags():
    import train
    from isa_amd.records import RecordLoader
    flags = ("color_jitter", "gamma", "channel_swap", "grayscale", "resolution")
    sig = inspect.signature(RecordLoader.__init__).parameters
    assert all(sig[f].default is False for f in flags)
    plain = train.parse_args([])
    on = train.parse_args(['--color-jitter', '--gamma', '--channel-swap', '--grayscale', '--resolution'])
    assert train.photometric_arguments(plain) == dict.fromkeys(flags, False)
    assert train.photometric_arguments(on) == dict.fromkeys(flags, True)
    assert train.photometric_arguments(train.parse_args(['--gamma'])) == dict(dict.fromkeys(flags, False), gamma=True)
    assert train.fit_arguments(on) == train.fit_arguments(plain)
