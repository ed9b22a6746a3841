"""CPU-only: isa_edt2_u8, isa_border_weights, isa_fill_labels and the pixel-weighted isa_sem_loss_k_*_pw refuse bad
arguments before they launch or write anything (so this runs without a GPU: every pointer below is host memory that no
kernel may ever see); the size helper mirrors the header; the host methods exist with the documented defaults."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

ISA_EINVAL, ISA_EALIGN, ISA_ENOMEM = -1, -2, -5
N, H, W = 2, 8, 12


def _lib():
    import isa_amd  # noqa: F401
    from isa_amd import lib as L
    return L, L.lib()


def _valid_args(L, name, keep):
    """A complete, valid argument list of entry `name` over host buffers (64-byte aligned), as a dict in ABI order."""
    buf = lambda: keep.append(torch.zeros(16384)) or keep[-1].data_ptr()            # 64 KiB each
    if name == "isa_edt2_u8":
        a = dict(labels=buf(), n=N, h=H, w=W, d1sq=buf(), d2sq=buf(), nearest=buf(), scratch=buf(),
                 scratch_bytes=L.edt_scratch_bytes(N, H, W), stream=None)
    elif name == "isa_border_weights":
        a = dict(labels=buf(), d1sq=buf(), d2sq=buf(), cfg=buf(), n=N, hw=H * W, out=buf(), stream=None)
    else:
        a = dict(labels=buf(), fg=buf(), nearest=buf(), d1sq=buf(), max_dist_sq=-1, n=N, hw=H * W, out=buf(), filled=buf(),
                 stream=None)
    assert len(a) == len(L.SIGNATURES[name]), name
    return a


POINTERS = {"isa_edt2_u8": ("labels", "scratch"), "isa_border_weights": ("labels", "d1sq", "d2sq", "cfg", "out"),
            "isa_fill_labels": ("labels", "fg", "nearest", "d1sq", "out", "filled")}
BAD_VALUES = {"isa_edt2_u8": dict(n=(0, -1, 65536), h=(0, -8, 4097), w=(0, -12, 10, 13, 14, 4100)),   # w % 4 != 0 is refused
              "isa_border_weights": dict(n=(0, -1), hw=(0, -96, 94, 97, 1 << 30)),
              "isa_fill_labels": dict(n=(0, -1, 65536), hw=(0, -96, 94, 97, 1 << 30))}
MISALIGNED = {"isa_edt2_u8": (("labels", 1), ("labels", 2), ("d1sq", 4), ("d1sq", 8), ("d2sq", 4), ("nearest", 1),
                              ("nearest", 2), ("scratch", 8)),
              "isa_border_weights": (("labels", 2), ("d1sq", 4), ("d2sq", 8), ("cfg", 2), ("out", 4), ("out", 8)),
              "isa_fill_labels": (("labels", 1), ("fg", 2), ("nearest", 1), ("d1sq", 4), ("d1sq", 8), ("out", 2),
                                  ("filled", 2))}


@pytest.mark.parametrize("name", sorted(POINTERS))
def test_distance_entries_refuse_bad_arguments_before_launching(name):
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


def test_transform_refuses_short_scratch_and_takes_null_outputs_as_valid():
    L, lib = _lib()
    keep = []
    a = _valid_args(L, "isa_edt2_u8", keep)
    a["scratch_bytes"] -= 1
    assert lib.isa_edt2_u8(*a.values()) == ISA_ENOMEM
    for out in ("d1sq", "d2sq", "nearest"):              # a NULL output is allowed: the call gets as far as the scratch check
        a = _valid_args(L, "isa_edt2_u8", keep)
        a[out] = None
        a["scratch_bytes"] = 0
        assert lib.isa_edt2_u8(*a.values()) == ISA_ENOMEM, out


def test_fill_refuses_an_output_that_aliases_the_labels():
    L, lib = _lib()
    keep = []
    a = _valid_args(L, "isa_fill_labels", keep)
    a["out"] = a["labels"]
    assert lib.isa_fill_labels(*a.values()) == ISA_EINVAL
    for off in (4, N * H * W - 4):                                                   # overlapping, not equal
        a = _valid_args(L, "isa_fill_labels", keep)
        a["out"] = a["labels"] + off
        assert lib.isa_fill_labels(*a.values()) == ISA_EINVAL, off
    a = _valid_args(L, "isa_fill_labels", keep)          # right behind the labels: no overlap, so the next refusal is the
    a["out"] = a["labels"] + N * H * W                   # alignment of another argument
    a["filled"] += 2
    assert lib.isa_fill_labels(*a.values()) == ISA_EALIGN


def _tensor(L, data, n, h, w, c, ld, dtype):
    return L.IsaTensor(data, n, h, w, c, ld, dtype, 1)


def test_pixel_weighted_criterion_entries_refuse_bad_arguments_before_launching():
    L, lib = _lib()
    keep = []
    buf = lambda: keep.append(torch.zeros(16384)) or keep[-1].data_ptr()
    x, dx = _tensor(L, buf(), 2, 8, 12, 5, 8, L.F32), _tensor(L, buf(), 2, 8, 12, 5, 8, L.F32)
    labels, cfg, pixw, sums, coef = buf(), buf(), buf(), buf(), buf()
    ok_s = [C.byref(x), labels, cfg, pixw, sums, None]
    ok_g = [C.byref(x), labels, cfg, coef, pixw, C.byref(dx), 0, None]
    assert len(ok_s) == len(L.SIGNATURES["isa_sem_loss_k_sums_pw"]) and len(ok_g) == len(L.SIGNATURES["isa_sem_loss_k_grad_pw"])
    for i in (0, 1, 2, 3, 4):
        a = list(ok_s)
        a[i] = None
        assert lib.isa_sem_loss_k_sums_pw(*a) == ISA_EINVAL, i
    for i in (0, 1, 2, 3, 4, 5):
        a = list(ok_g)
        a[i] = None
        assert lib.isa_sem_loss_k_grad_pw(*a) == ISA_EINVAL, i
    a = list(ok_s)
    a[3] = pixw + 2
    assert lib.isa_sem_loss_k_sums_pw(*a) == ISA_EALIGN
    a = list(ok_g)
    a[4] = pixw + 2
    assert lib.isa_sem_loss_k_grad_pw(*a) == ISA_EALIGN
    bad = _tensor(L, x.data, 2, 8, 12, 33, 40, L.F32)                              # more classes than ISA_SEM_MAX_CLASSES
    assert lib.isa_sem_loss_k_sums_pw(C.byref(bad), labels, cfg, pixw, sums, None) == ISA_EINVAL
    other = _tensor(L, dx.data, 2, 8, 12, 5, 8, L.BF16)                            # d logits of another dtype
    assert lib.isa_sem_loss_k_grad_pw(C.byref(x), labels, cfg, coef, pixw, C.byref(other), 0, None) == ISA_EINVAL


def test_scratch_formula_and_geometry_match_the_header():
    L, _ = _lib()
    text = open(os.path.join(ROOT, "include", "isa_kernels.h")).read()
    assert "#define ISA_EDT_MAX_SIDE %d\n" % L.EDT_MAX_SIDE in text
    assert "#define ISA_EDT_COL_LANES %d\n" % L.EDT_COL_LANES in text and "#define ISA_EDT_ROW_LANES %d\n" % L.EDT_ROW_LANES in text
    assert "#define ISA_EDT_SCRATCH_BYTES(n, h, w) ((int64_t)(n) * (h) * (w) * 8)\n" in text
    assert L.edt_scratch_bytes(3, 8, 12) == 3 * 8 * 12 * 8


def test_the_new_methods_exist():
    import inspect
    import isa_amd  # noqa: F401
    from isa_amd.model import Model
    from isa_amd.labelmaps import LabelOps
    from isa_amd.network import SemCriterion
    from isa_amd.reseg import ReSeg
    from isa_amd.trainer import Trainer
    for cls, names in ((LabelOps, ("edt2", "border_map", "fill_labels")),
                       (ReSeg, ("distance_transform", "border_weights", "fill_instances")),
                       (SemCriterion, ("set_border", "border_key")), (Trainer, ("set_border",))):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    p = inspect.signature(ReSeg.border_weights).parameters
    assert [p[k].default for k in ("w0", "sigma")] == [10.0, 5.0]
    assert inspect.signature(ReSeg.fill_instances).parameters["max_dist"].default is None
    for fn in (Model.predict_instances, Model.evaluate):
        p = inspect.signature(fn).parameters
        assert [p[k].default for k in ("fill", "fill_max_dist")] == [False, None]
        assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("fill", "fill_max_dist"))
    p = inspect.signature(Model.fit).parameters
    assert [p[k].default for k in ("border_weight", "border_sigma")] == [0.0, 5.0]
    p = inspect.signature(Trainer.__init__).parameters
    assert [p[k].default for k in ("border_weight", "border_sigma")] == [0.0, 5.0]
